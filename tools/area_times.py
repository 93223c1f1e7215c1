#!/usr/bin/env python3
"""Per-dispatch device times (mirhi_device_timeline, the method of tools/shadow_times.py) of a render-area scope beside the only way
a library without render areas can produce those pixels: a full-extent LOAD scope with the scissor set to the rectangle.
  atlas   a 512 x 512 rectangle in the middle of a 4096 x 4096 D32 image, tile-aligned and unaligned: a depth-only (SHADOW) scope of 10k
          triangles whose viewport is the rectangle;
  target  the same rectangle of a 3840 x 2160 B8G8R8A8_SRGB target with C2's 10k triangles (at that extent) scissored to it.
--mode area: render_area with CLEAR; --mode scissor: the baseline (runs on any build: MIRHI_LIB_NAME names another library); both: default.
Prints one JSON object: median microseconds per dispatch over the timed repeats and their sum per case, with the build id."""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import shadow_times as st  # noqa: E402

m, S = st.m, st.S
RECTS = {"aligned": (1792, 1792, 512, 512), "unaligned": (1787, 1799, 512, 512)}
TARGET_RECTS = {"aligned": (1664, 832, 512, 512), "unaligned": (1659, 839, 512, 512)}


def summed(kernels):
    kernels["sum"] = round(sum(kernels.values()), 2)
    return kernels


def atlas(dev, rect, mode):
    tris = S.random_triangles(10000, 512, 512).draws[0]          # positions in NDC: the first 12 bytes of each 24-byte vertex
    eye = np.eye(4, dtype=np.float32)
    vp = (float(rect[0]), float(rect[1]), float(rect[2]), float(rect[3]), 0.0, 1.0)
    caster = S.DrawSpec(vertices=tris.vertices, stride=24, count=tris.count, program=S.PROGRAM_SHADOW, cull_mode=S.CULL_NONE,
                        camera=S.shadow_constants_ubo(eye, eye), viewport=vp, scissor=None if mode == "area" else rect)
    spec = S.ShadowSpec([caster], (4096, 4096), S.shadow_ubo(eye, size=(4096, 4096)),
                        load_op=S.LOAD_OP_CLEAR if mode == "area" else S.LOAD_OP_LOAD, render_area=rect if mode == "area" else None)
    res = m.SceneResources(dev, S.Scene("area-atlas", 64, 64, [], shadow=spec), m.Format.B8G8R8A8_SRGB, shadow_cmd=True)
    t = summed(st.per_kernel(st.timed(dev, lambda: dev.submit([res.shadow_cmd]))))
    res.destroy()
    return t


def target(dev, rect, mode):
    scene = S.random_triangles(10000, 3840, 2160)
    if mode == "area":
        scene = dataclasses.replace(scene, render_area=rect)
    else:
        scene = dataclasses.replace(scene, draws=[dataclasses.replace(d, scissor=rect) for d in scene.draws])
    res = m.SceneResources(dev, scene, m.Format.B8G8R8A8_SRGB, color_load_op=m.LoadOp.CLEAR if mode == "area" else m.LoadOp.LOAD)
    t = summed(st.per_kernel(st.timed(dev, res.render)))
    res.destroy()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("area", "scissor", "both"), default="both")
    args = ap.parse_args()
    dev = m.Device(0)
    out = {"build_id": m.lib().mirhi_build_id().decode(), "library": os.path.basename(m.LIB_PATH), "reps": st.REPS}
    for mode in (("area", "scissor") if args.mode == "both" else (args.mode,)):
        for name, rect in RECTS.items():
            out[f"atlas_{name}_{mode}"] = atlas(dev, rect, mode)
        for name, rect in TARGET_RECTS.items():
            out[f"target_{name}_{mode}"] = target(dev, rect, mode)
    dev.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
