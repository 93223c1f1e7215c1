#!/usr/bin/env python3
"""Per-dispatch device times of cascaded shadow maps (mirhi_device_timeline), one GPU process, the method of tools/shadow_times.py:
  (d) the lit MODEL_PBR raster of cascaded_ground_case at 1920 x 1080 with the cascade array bound (raster_kernel_csm), with nothing bound
      (variant 4) and with one single shadow map bound (raster_kernel_shadow);
  (e) its four depth-only scopes (vertex / geometry / raster per layer) at 1024^2 and 2048^2 layers;
  (f) the lit raster with blended cascades (raster_kernel_csm_blend) at thresholds 0.1 and 1.0, and with stabilised cascades.
Prints one JSON object (median microseconds per dispatch over the timed repeats) with the build id."""
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import shadow_times as st  # noqa: E402

m, S = st.m, st.S


def main():
    dev = m.Device(0)
    out = {"build_id": m.lib().mirhi_build_id().decode(), "reps": st.REPS}
    for size in (1024, 2048):
        scene = S.cascaded_ground_case(1920, 1080, map_size=size)
        res = m.SceneResources(dev, scene, m.Format.B8G8R8A8_SRGB)
        t = st.per_kernel(st.timed(dev, res.render), n_scopes=5)            # scopes 0..3: the layers, 4: the lit scope
        res.destroy()
        out[f"e_four_depth_scopes_{size}"] = {k: v for k, v in t.items() if not k.endswith("[4]")}
        out[f"d_pbr_with_cascades_{size}"] = {k: v for k, v in t.items() if k.endswith("[4]")}
    # (f) the lit scope with blended cascades (raster_kernel_csm_blend) at thresholds 0.1 and 1.0, beside d_pbr_with_cascades_2048 of this run: 0.1 is what
    # a frame uses (few lanes take the second sample), 1.0 bounds the cost from above (every lane of cascades 0..2 takes it); stabilised cascades and
    # threshold 0 (raster_kernel_csm again) beside them, for the cost of the coarser texels alone
    for name, kw in (("f_pbr_blended_0.1_2048", dict(blend_threshold=0.1)), ("f_pbr_blended_1.0_2048", dict(blend_threshold=1.0)),
                     ("f_pbr_stabilised_unblended_2048", dict(stabilize=True)), ("f_pbr_stabilised_blended_0.1_2048", dict(stabilize=True, blend_threshold=0.1))):
        res = m.SceneResources(dev, S.cascaded_ground_case(1920, 1080, map_size=2048, **kw), m.Format.B8G8R8A8_SRGB)
        t = st.per_kernel(st.timed(dev, res.render), n_scopes=5)
        res.destroy()
        out[name] = {k: v for k, v in t.items() if k.endswith("[4]")}
    scene = S.cascaded_ground_case(1920, 1080, map_size=2048)
    plain = dataclasses.replace(scene, cascades=None)
    res = m.SceneResources(dev, plain, m.Format.B8G8R8A8_SRGB)
    out["d_pbr_nothing_bound"] = st.per_kernel(st.timed(dev, res.render))
    res.destroy()
    # the same frame with ONE map that holds the whole cascaded range (cascade 3's matrix is the widest; a single light matrix over the same casters)
    ls = S.light_space_matrix(S.CASCADED_GROUND_LIGHT, center=(0.0, 0.0, -25.0), half_extent=45.0, near=0.1, far=160.0, distance=80.0)
    casters = [dataclasses.replace(c, camera=S.shadow_constants_ubo(S.flip_clip_y(ls), __import__("numpy").frombuffer(c.camera[64:], dtype="float32").reshape(4, 4)))
               for c in scene.cascades.casters[0]]
    single = dataclasses.replace(plain, shadow=S.ShadowSpec(casters, (2048, 2048), S.shadow_ubo(ls, 0.005, 0.01, (2048, 2048), 1.0)))
    res = m.SceneResources(dev, single, m.Format.B8G8R8A8_SRGB)
    out["d_pbr_single_map_2048"] = st.per_kernel(st.timed(dev, res.render), n_scopes=2)
    res.destroy()
    dev.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
