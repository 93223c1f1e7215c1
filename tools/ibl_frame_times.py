#!/usr/bin/env python3
"""Per-dispatch device times (mirhi_device_timeline, the method of tools/shadow_times.py) of the lit scope of cascaded_ground_case at
1920 x 1080 under MODEL_PBR and under MODEL_PBR_IBL (raster_kernel_ibl; irradiance 32^2, prefiltered 128^2 x 8, LUT 512^2 made by the precompute
passes), each with the shadow term none / a single 2048^2 map / four 2048^2 cascades.  Prints one JSON object (median microseconds per dispatch
over the timed repeats) with the build id.  "seamless": the MODEL_PBR_IBL lit scope per shadow term with both cubes' seamless state off and on
(mirhi_image_set_cube_seamless, raster_kernel_ibl against raster_kernel_ibl_seamless), three rounds interleaved in this one process, the lit scope's raster
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


def main():
    dev = m.Device(0)
    out = {"build_id": m.lib().mirhi_build_id().decode(), "reps": st.REPS}
    I = m.Image
    src = I(dev, 512, 256, m.Format.R32G32B32A32_SFLOAT)
    src.upload(m.ibl.analytic_equirect(512, 256).astype(np.float32))
    env, irr, pre, lut = I.create_cube(dev, 128, 8), I.create_cube(dev, 32, 1), I.create_cube(dev, 128, 8), I(dev, 512, 512, m.Format.R32G32B32A32_SFLOAT)
    env.ibl_equirect_to_cube(src); env.ibl_cube_generate_mips(); irr.ibl_irradiance(env); pre.ibl_prefilter(env, 256); lut.ibl_brdf_lut()
    scene = S.cascaded_ground_case(1920, 1080, map_size=2048)
    plain = dataclasses.replace(scene, cascades=None)
    ls = S.light_space_matrix(S.CASCADED_GROUND_LIGHT, center=(0.0, 0.0, -25.0), half_extent=45.0, near=0.1, far=160.0, distance=80.0)
    casters = [dataclasses.replace(c, camera=S.shadow_constants_ubo(S.flip_clip_y(ls), np.frombuffer(c.camera[64:], dtype="float32").reshape(4, 4)))
               for c in scene.cascades.casters[0]]
    single = dataclasses.replace(plain, shadow=S.ShadowSpec(casters, (2048, 2048), S.shadow_ubo(ls, 0.005, 0.01, (2048, 2048), 1.0)))
    for shadow, sc, n_scopes in (("none", plain, 1), ("single_map", single, 2), ("cascades", scene, 5)):
        for prog_name, prog in (("model_pbr", S.PROGRAM_MODEL_PBR), ("model_pbr_ibl", S.PROGRAM_MODEL_PBR_IBL)):
            sc2 = dataclasses.replace(sc, draws=[dataclasses.replace(d, program=prog) if d.program == S.PROGRAM_MODEL_PBR else d for d in sc.draws])
            res = m.SceneResources(dev, sc2, m.Format.B8G8R8A8_SRGB, ibl_images=(irr, pre, lut))
            t = st.per_kernel(st.timed(dev, res.render), n_scopes=n_scopes)
            res.destroy()
            out[f"{prog_name}_{shadow}"] = {k: v for k, v in t.items() if n_scopes == 1 or k.endswith(f"[{n_scopes - 1}]")}
    rounds = {shadow: {"clamped": [], "seamless": []} for shadow in ("none", "single_map", "cascades")}
    for _ in range(3):
        for state, on in (("clamped", False), ("seamless", True)):
            irr.set_cube_seamless(on); pre.set_cube_seamless(on)      # (latched when SceneResources records)
            for shadow, sc, n_scopes in (("none", plain, 1), ("single_map", single, 2), ("cascades", scene, 5)):
                sc2 = dataclasses.replace(sc, draws=[dataclasses.replace(d, program=S.PROGRAM_MODEL_PBR_IBL) if d.program == S.PROGRAM_MODEL_PBR else d for d in sc.draws])
                res = m.SceneResources(dev, sc2, m.Format.B8G8R8A8_SRGB, ibl_images=(irr, pre, lut))
                t = st.per_kernel(st.timed(dev, res.render), n_scopes=n_scopes)
                res.destroy()
                rounds[shadow][state].append(t.get("raster", t.get(f"raster[{n_scopes - 1}]")))
    irr.set_cube_seamless(False); pre.set_cube_seamless(False)
    for r in rounds.values():
        r["ratio"] = round(sum(r["seamless"]) / sum(r["clamped"]), 3)
    out["seamless"] = rounds
    for im in (src, env, irr, pre, lut):
        im.destroy()
    dev.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
