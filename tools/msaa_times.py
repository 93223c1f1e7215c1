#!/usr/bin/env python3
"""Per-dispatch device times of 4x MSAA (mirhi_device_timeline), one GPU process, the method of tools/shadow_times.py: geometry and raster of
the C2 scene (10,000 random triangles, TRIANGLE program) and of the dancer asset (MODEL_FULL) at 1920 x 1080 into B8G8R8A8_SRGB, at 1x and at 4x of the
same build, with the 4x / 1x ratios.  Beside the times: the bytes the frame's attachments hold in HBM (mirhi_image_size_bytes) -- a 4x frame's are a 1x
frame's, because a multisampled attachment is transient and owns no memory; the HBM traffic itself is a counter run (tools/collect_profiles.sh).
Prints one JSON object (median microseconds per dispatch over the timed repeats) with the build id."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import shadow_times as st  # noqa: E402

m, S = st.m, st.S
W, H = 1920, 1080


def attachment_bytes(res):
    images = [res.color, res.depth, res.prim, res.ms_color, res.ms_depth]
    return {"resolve_or_1x_targets": sum(int(m.lib().mirhi_image_size_bytes(i.handle)) for i in images[:3] if i is not None),
            "multisampled": sum(int(m.lib().mirhi_image_size_bytes(i.handle)) for i in images[3:] if i is not None)}


def one(dev, scene, samples):
    try:
        res = m.SceneResources(dev, scene, m.Format.B8G8R8A8_SRGB, samples=samples)
    except m.RhiError as e:           # (a scene a multisampled scope refuses: say so instead of timing something else)
        return {"refused": str(e)}
    t = st.per_kernel(st.timed(dev, res.render))
    t["attachment_bytes"] = attachment_bytes(res)
    res.destroy()
    return t


def main():
    dev = m.Device(0)
    out = {"build_id": m.lib().mirhi_build_id().decode(), "reps": st.REPS, "target": [W, H, "B8G8R8A8_SRGB"]}
    scenes = {"c2_random_10000": S.random_triangles(10000, W, H),
              "dancer": S.gltf_model(os.path.join(ROOT, "tests", "golden", "dancer", "scene.gltf"), W, H)}
    for name, scene in scenes.items():
        a, b = one(dev, scene, 1), one(dev, scene, 4)
        out[name] = {"triangles": scene.num_triangles, "1x": a, "4x": b}
        if "raster" in a and "raster" in b:
            out[name]["ratio_4x_over_1x"] = {k: round(b[k] / a[k], 2) for k in ("geometry", "raster") if k in a and k in b and a[k] > 0}
    dev.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
