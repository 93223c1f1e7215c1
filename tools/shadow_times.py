#!/usr/bin/env python3
"""Per-dispatch device times of shadow mapping (mirhi_device_timeline), one GPU process:
  (a) depth-only SHADOW scopes of C3's sphere into 2048^2 and of C5's box hall into 4096^2, with bytes and HBM roofline share
      (vertices + indices + W x H x 4 over the raster + geometry + vertex time);
  (b) the same geometry drawn with the MODEL program into RGBA8 + D32 of the same size;
  (c) the MODEL_PBR main-pass raster of shadowed_ground_case at 1920 x 1080 with and without a bound shadow map;
  (d) the depth-only scopes of (a) again with depth bias (constant 1, slope 2) and depth clamp on the map's pipelines.
Prints one JSON object (median microseconds per dispatch over the timed repeats) with the build id."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

m = ge.load_package()
S = m.scenes
HBM_PEAK_GBS = 8000.0
REPS = int(os.environ.get("SHADOW_TIMES_REPS", "32"))


def light_for(scene):
    """An orthographic light that holds every draw of the scene (bounds of its world positions)."""
    pts = []
    for d in scene.draws:
        v = np.ascontiguousarray(d.vertices, dtype=np.float32).reshape(-1, d.stride // 4)[:, 0:3].astype(np.float64)
        model = np.frombuffer(d.object[:64], dtype=np.float32).reshape(4, 4).T.astype(np.float64)
        pts.append((np.c_[v, np.ones(len(v))] @ model.T)[:, :3])
    p = np.concatenate(pts)
    lo, hi = p.min(0), p.max(0)
    c, r = (lo + hi) / 2, float(np.linalg.norm(hi - lo) / 2) * 1.05
    return S.light_space_matrix((0.35, -1.0, 0.25), center=tuple(c), half_extent=r, near=0.1, far=4 * r, distance=2 * r), r


def caster_scene(scene, size):
    ls, _ = light_for(scene)
    casters = [S.DrawSpec(vertices=d.vertices, stride=d.stride, count=d.count, indices=d.indices, program=S.PROGRAM_SHADOW,
                          cull_mode=S.CULL_NONE, camera=S.shadow_constants_ubo(S.flip_clip_y(ls), np.frombuffer(d.object[:64], dtype=np.float32).reshape(4, 4)))
               for d in scene.draws]
    return ls, casters


def timed(dev, fn):
    for _ in range(4):
        fn()
    dev.wait_idle()
    dev.reset_kernel_times()
    dev.set_profiling(m.Profile.TIMING)
    for _ in range(REPS):
        fn()
        dev.wait_idle()
    tl = dev.timeline()
    dev.set_profiling(0)
    dev.reset_kernel_times()
    return tl


def per_kernel(tl, n_scopes=1):
    """median us per dispatch of each kernel id; with n_scopes scopes per submit the raster dispatches are split by their place in the submit"""
    out = {}
    for k, name in enumerate(m.Kernel.NAMES):
        ds = [e - b for (kk, _, b, e) in tl if kk == k]
        if not ds:
            continue
        if n_scopes > 1 and len(ds) % n_scopes == 0:
            for s in range(n_scopes):
                out[f"{name}[{s}]"] = round(statistics.median(ds[s::n_scopes]), 2)
        else:
            out[name] = round(statistics.median(ds), 2)
    return out


def depth_only(dev, scene, size, **depth_state):
    """depth_state: ShadowSpec's depth_bias=(constant, clamp, slope) / depth_clamp=True for the map's pipelines"""
    ls, casters = caster_scene(scene, size)
    sc = S.Scene(scene.name + "-shadow", 64, 64, [], shadow=S.ShadowSpec(casters, (size, size), S.shadow_ubo(ls, size=(size, size)), **depth_state))
    res = m.SceneResources(dev, sc, m.Format.B8G8R8A8_SRGB, shadow_cmd=True)
    t = per_kernel(timed(dev, lambda: dev.submit([res.shadow_cmd])))
    nbytes = size * size * 4
    seen = set()
    for d in scene.draws:
        if id(d.vertices) not in seen:
            seen.add(id(d.vertices)); nbytes += d.vertex_bytes().size
        if d.indices is not None and id(d.indices) not in seen:
            seen.add(id(d.indices)); nbytes += d.indices.size * d.indices.dtype.itemsize
    total_us = sum(v for v in t.values())
    res.destroy()
    return dict(kernels_us=t, bytes=nbytes, gbs=round(nbytes / (total_us * 1e3), 1) if total_us else None,
                hbm_frac=round(nbytes / (total_us * 1e3) / HBM_PEAK_GBS, 4) if total_us else None)


def model_same_geometry(dev, scene, size):
    ls, _ = light_for(scene)
    z = np.zeros(32, dtype=np.float32).tobytes()
    cam = z + S.flip_clip_y(ls).astype(np.float32).tobytes() + np.zeros(4, dtype=np.float32).tobytes()
    draws = [S.DrawSpec(vertices=d.vertices, stride=d.stride, count=d.count, indices=d.indices, program=S.PROGRAM_MODEL, cull_mode=S.CULL_NONE,
                        camera=cam, object=d.object) for d in scene.draws]
    res = m.SceneResources(dev, S.Scene(scene.name + "-model", size, size, draws), m.Format.B8G8R8A8_SRGB, want_depth=True)
    t = per_kernel(timed(dev, res.render))
    res.destroy()
    return dict(kernels_us=t)


def main():
    dev = m.Device(0)
    out = {"build_id": m.lib().mirhi_build_id().decode(), "reps": REPS}
    for name, make, size in (("c3", S.displaced_sphere, 2048), ("c5", S.box_hall, 4096)):
        scene = make()
        out[f"a_{name}_depth_only_{size}"] = depth_only(dev, scene, size)
        out[f"b_{name}_model_rgba8_d32_{size}"] = model_same_geometry(dev, scene, size)
        out[f"d_{name}_depth_only_bias_clamp_{size}"] = depth_only(dev, scene, size, depth_bias=(1.0, 0.0, 2.0), depth_clamp=True)
    ground = S.shadowed_ground_case(1920, 1080, map_size=2048)
    with_map = m.SceneResources(dev, ground, m.Format.B8G8R8A8_SRGB)
    out["c_pbr_with_map"] = per_kernel(timed(dev, with_map.render), n_scopes=2)
    with_map.destroy()
    import dataclasses
    without = m.SceneResources(dev, dataclasses.replace(ground, shadow=None), m.Format.B8G8R8A8_SRGB)
    out["c_pbr_without_map"] = per_kernel(timed(dev, without.render))
    without.destroy()
    dev.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
