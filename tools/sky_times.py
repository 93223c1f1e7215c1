#!/usr/bin/env python3
"""Per-dispatch device times (mirhi_device_timeline, the method of tools/shadow_times.py) of the SKYBOX segment (sky_kernel) at 1920 x 1080 on
B8G8R8A8_SRGB, environment 512^2 x 1: the sky alone (CLEAR), the sky behind cascaded_ground_case WITHOUT its four cascade scopes (shadow term 1) under MODEL_PBR_IBL
(LESS_OR_EQUAL, no write: it reads the lit segment's depth), and the same lit scope without the sky.  Prints one JSON object: median microseconds
per dispatch over the timed repeats, in dispatch order, with the build id.  "seamless": the sky alone and the sky behind the lit scope with the environment's
seamless state off and on (mirhi_image_set_cube_seamless, sky_kernel against sky_kernel_seamless), three rounds interleaved in this one process, the raster
medians of each round and the ratio of their means."""
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
W, H = 1920, 1080


def main():
    dev = m.Device(0)
    out = {"build_id": m.lib().mirhi_build_id().decode(), "reps": st.REPS}
    I = m.Image
    env = I.create_cube(dev, 512, 1)
    env.upload(m.ibl.pack_cube([m.ibl.analytic_environment(512).astype(np.float32)]))
    irr, pre, lut = I.create_cube(dev, 32, 1), I.create_cube(dev, 128, 8), I(dev, 512, 512, m.Format.R32G32B32A32_SFLOAT)
    irr.ibl_irradiance(env); pre.ibl_prefilter(env, 64); lut.ibl_brdf_lut()
    cam = S.skybox_case(W, H, 0, 1, 1)      # (the camera and matrix of the test case; its own 1^2 cube is not used)
    ground = dataclasses.replace(S.cascaded_ground_case(W, H, map_size=2048), cascades=None)
    lit = dataclasses.replace(ground, draws=[dataclasses.replace(d, program=S.PROGRAM_MODEL_PBR_IBL) if d.program == S.PROGRAM_MODEL_PBR else d for d in ground.draws])
    spec = S.SkySpec(inv_view_proj=cam.sky.inv_view_proj, image=env)
    sky_alone = S.Scene("sky-alone", W, H, [], clear_color=cam.clear_color, sky=spec)
    for name, scene, n in (("sky_alone", sky_alone, 1), ("lit_with_sky", dataclasses.replace(lit, sky=spec), 2), ("lit_alone", lit, 1)):
        res = m.SceneResources(dev, scene, m.Format.B8G8R8A8_SRGB, ibl_images=(irr, pre, lut), want_depth=(name != "sky_alone"))
        out[name] = st.per_kernel(st.timed(dev, res.render), n_scopes=n)
        res.destroy()
    rounds = {"sky_alone": {"clamped": [], "seamless": []}, "lit_with_sky": {"clamped": [], "seamless": []}}
    for _ in range(3):
        for state, on in (("clamped", False), ("seamless", True)):
            env.set_cube_seamless(on)      # (latched when SceneResources records)
            for name, scene, n in (("sky_alone", sky_alone, 1), ("lit_with_sky", dataclasses.replace(lit, sky=spec), 2)):
                res = m.SceneResources(dev, scene, m.Format.B8G8R8A8_SRGB, ibl_images=(irr, pre, lut), want_depth=(name != "sky_alone"))
                t = st.per_kernel(st.timed(dev, res.render), n_scopes=n)
                res.destroy()
                rounds[name][state].append(t.get("raster", t.get(f"raster[{n - 1}]")))
    env.set_cube_seamless(False)
    for name, r in rounds.items():
        r["ratio"] = round(sum(r["seamless"]) / sum(r["clamped"]), 3)
    out["seamless"] = rounds
    for im in (env, irr, pre, lut):
        im.destroy()
    dev.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
