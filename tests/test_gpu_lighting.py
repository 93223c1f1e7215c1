"""The lit fragment programs on the GPU against the float64 model of renderer-rs_amd/lighting.py: the plain route on every case of
tests/lighting_cases.py, the sRGB8 store, and the other instantiations of the same fragment code -- wide variants, two teams, the generic and the
predicate key, an ordered segment, the alpha-masked variant, mixed program sets, a render area, 4x MSAA, the shadow family and the IBL family.
Each frame is measured as DESIGN.md 8d states: err over RGB against max(8 E32, 1e-4), E32 from the float32 model alone; alpha within 1e-5."""
import dataclasses

import numpy as np
import pytest

import lighting_cases as lc

pytestmark = pytest.mark.gpu


def _render(mirhi, device, scene, fmt=None, **kw):
    res = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT if fmt is None else fmt, want_prim=True, **kw)
    res.render()
    out = res.read()
    res.destroy()
    return out


_refs = {}


def _oracle_prim(oracle, scene):
    if scene.name not in _refs:
        _refs[scene.name] = oracle.render(scene, want_bgra8=False)["prim"]
    return _refs[scene.name]


def _same_prims(out, ref_prim, name):
    diff = out["prim"] != ref_prim
    assert not diff.any(), f"{name}: {int(diff.sum())} pixels differ in winning primitive id (first at {np.argwhere(diff)[0]})"


def _with(scene, suffix, **draw_changes):
    """The scene under another name with every draw changed alike."""
    return dataclasses.replace(scene, name=f"{scene.name} {suffix}", draws=[dataclasses.replace(d, **draw_changes) for d in scene.draws])


def _sphere_pair(scenes):
    return lc.sphere(scenes.PROGRAM_MODEL_PBR, 0.3), lc.sphere(scenes.PROGRAM_MODEL_FULL, 0.3, True)


@pytest.mark.parametrize("i", range(lc.CASE_COUNT))
def test_plain_route(mirhi, oracle, device, i):
    """Every case / program / roughness on the float target: the prim-id image is the oracle's bit for bit, the colour the model's within the bound."""
    sc = lc.case(i)
    out = _render(mirhi, device, sc)
    _same_prims(out, _oracle_prim(oracle, sc), sc.name)
    lc.check(None, sc, out["prim"], out["color"], "GPU")
    bg = out["prim"] == lc.NO_PRIM
    assert np.array_equal(out["color"][bg], np.broadcast_to(np.array(sc.clear_color, dtype=np.float32), out["color"][bg].shape))


def test_srgb8_target(mirhi, oracle, device, scenes):
    """B8G8R8A8_SRGB: every byte within 1 of the float64 OETF of M64 (alpha: of round(255 a))."""
    for sc in _sphere_pair(scenes):
        out = _render(mirhi, device, sc, fmt=mirhi.Format.B8G8R8A8_SRGB)
        _same_prims(out, _oracle_prim(oracle, sc), sc.name)
        m = lc.model(sc, out["prim"])
        k = m.keep
        got = out["color"][m.py[k], m.px[k]].astype(np.int64)
        want = lc.srgb8_oetf(m.m64[k, :3])
        d_rgb = np.abs(got[:, [2, 1, 0]] - want)
        d_a = np.abs(got[:, 3] - np.rint(np.clip(m.m64[k, 3], 0.0, 1.0) * 255.0))
        print(f"LIGHT {sc.name} sRGB8: pixels {int(k.sum())} max byte difference {int(d_rgb.max())} (alpha {int(d_a.max())})")
        assert k.sum() > 3000 and d_rgb.max() <= 1 and d_a.max() <= 1
        assert np.unique(want).size > 100                # (the frame uses the byte range; highlights may saturate)


@pytest.mark.parametrize("knobs", [dict(MIRHI_RASTER_WIDE="8", MIRHI_RASTER_TEAMS="1", MIRHI_TP_DENSITY="0"),
                                   dict(MIRHI_RASTER_WIDE="16", MIRHI_RASTER_TEAMS="1", MIRHI_TP_DENSITY="0"),
                                   dict(MIRHI_RASTER_TEAMS="2", MIRHI_TP_DENSITY="0")], ids=["wide8", "wide16", "two-teams"])
def test_mesh_variants(mirhi, oracle, device, scenes, monkeypatch, knobs):
    """raster_kernel_wide with eight and sixteen waves per tile (the knobs of test_wide_mesh_variants) and two teams per tile."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    for sc in _sphere_pair(scenes) + (lc.sphere(scenes.PROGRAM_MODEL_FULL, 0.3, False),):      # program sets 4, 4 and 2
        out = _render(mirhi, device, sc)
        _same_prims(out, _oracle_prim(oracle, sc), sc.name)
        lc.check(f"{sc.name} [{' '.join(knobs.values())}]", sc, out["prim"], out["color"], "GPU")


@pytest.mark.parametrize("key", ["generic", "predicate", "ordered", "masked"])
def test_depth_keys_and_resolve_paths(mirhi, oracle, device, scenes, key):
    """GREATER against a depth cleared to 0 (generic key), ALWAYS (predicate key), a blended segment whose factors ONE / ZERO / ADD leave the source
    unchanged (ordered resolve), and fragment_discard_enable with a cutoff below every alpha (the alpha-masked variant; Cook-Torrance only)."""
    for base in _sphere_pair(scenes):
        if key == "generic":
            sc = dataclasses.replace(_with(base, "GREATER", depth_compare=scenes.CMP_GREATER), clear_depth=0.0)
        elif key == "predicate":
            sc = _with(base, "ALWAYS", depth_compare=scenes.CMP_ALWAYS)
        elif key == "ordered":
            sc = _with(base, "blend ONE ZERO", blend=(scenes.BF_ONE, scenes.BF_ZERO, scenes.BO_ADD, scenes.BF_ONE, scenes.BF_ZERO, scenes.BO_ADD, 0xF))
        else:
            if base.draws[0].program != scenes.PROGRAM_MODEL_PBR:
                continue
            mat = np.frombuffer(base.draws[0].material, dtype=np.float32).copy()
            mat[11] = 0.25                               # alphaCutoff; the least alpha of the case is 0.9 * 200 / 255
            sc = _with(base, "masked", material=mat.tobytes(), alpha_test=True)
        out = _render(mirhi, device, sc)
        _same_prims(out, _oracle_prim(oracle, sc), sc.name)
        lc.check(None, sc, out["prim"], out["color"], "GPU")
        if key in ("ordered", "masked"):                 # the same winners as the plain frame
            assert np.array_equal(out["prim"], _oracle_prim(oracle, base))


def test_mixed_program_sets(mirhi, oracle, device, scenes):
    """A TRIANGLE draw beside the mesh: MODEL + TRIANGLE (program set 3) and every lit program + TRIANGLE in turn (the full-featured variant)."""
    tri = scenes.DrawSpec(vertices=scenes._tri_verts([[-0.97, -0.97, 0.5], [-0.97, -0.7, 0.5], [-0.7, -0.97, 0.5]]), stride=24, count=3,
                          program=scenes.PROGRAM_TRIANGLE, cull_mode=scenes.CULL_NONE)
    for base in (lc.sphere(scenes.PROGRAM_MODEL),) + _sphere_pair(scenes):
        sc = dataclasses.replace(base, name=f"{base.name} + TRIANGLE", draws=[tri] + list(base.draws))
        out = _render(mirhi, device, sc)
        _same_prims(out, _oracle_prim(oracle, sc), sc.name)
        assert (out["prim"] == 0).sum() > 50 and (out["prim"] != lc.NO_PRIM).sum() > 3000
        lc.check(None, sc, out["prim"], out["color"], "GPU")


def test_unaligned_render_area(mirhi, oracle, device, scenes):
    """A render area no multiple of the tile at any edge: inside it the frame is the model's, on the oracle's winners."""
    area = (41, 37, 71, 53)
    inside = np.zeros((lc.H, lc.W), dtype=bool)
    inside[area[1]:area[1] + area[3], area[0]:area[0] + area[2]] = True
    for base in _sphere_pair(scenes):
        sc = dataclasses.replace(base, render_area=area)
        out = _render(mirhi, device, sc)
        ref = _oracle_prim(oracle, base)
        assert np.array_equal(out["prim"][inside], ref[inside])
        prim = np.where(inside, ref, np.uint32(lc.NO_PRIM)).astype(np.uint32)
        assert (prim != lc.NO_PRIM).sum() > 2000 and (ref[~inside] != lc.NO_PRIM).any()         # the area cuts the mesh
        lc.check(f"{base.name} in area {area}", base, prim, out["color"], "GPU", min_pixels=2000)


def test_msaa_interior(mirhi, oracle, device, scenes):
    """4x MSAA on `ground`: where the eight neighbours of a pixel belong to the same quad in the single-sample image, all four samples lie inside it
    (convexity), every shading is the pixel centre's, and the resolve averages equal values."""
    for base in (lc.ground(scenes.PROGRAM_MODEL_PBR), lc.ground(scenes.PROGRAM_MODEL_FULL)):
        ref = _oracle_prim(oracle, base)
        mask = lc.interior_mask(ref)
        out = _render(mirhi, device, base, samples=4)
        samples = out["prim"]
        assert samples.shape == (lc.H, lc.W, 4) and np.all(samples[mask] != lc.NO_PRIM)
        lc.check(f"{base.name} 4x MSAA", base, ref, out["color"], "GPU", mask=mask, min_pixels=5000)


def test_shadow_family_with_a_map_cleared_to_one(mirhi, oracle, device, scenes):
    """MODEL_PBR with a shadow map bound and nothing drawn into it: PCF is exactly 1, the frame the unshadowed model's (raster_kernel_shadow)."""
    for base in (lc.sphere(scenes.PROGRAM_MODEL_PBR, 0.3), lc.ground(scenes.PROGRAM_MODEL_PBR)):
        direction = lc.SPHERE_LIGHTS["directional"]["direction"] if base.name.startswith("sphere") else lc.GROUND_LIGHTS["directional"]["direction"]
        spec = scenes.ShadowSpec(casters=[], size=(64, 64), params=scenes.shadow_ubo(scenes.light_space_matrix(direction), size=(64, 64)), clear_depth=1.0)
        out = _render(mirhi, device, dataclasses.replace(base, shadow=spec))
        _same_prims(out, _oracle_prim(oracle, base), base.name)
        lc.check(f"{base.name} shadow map = 1", base, out["prim"], out["color"], "GPU")


def test_ibl_family_with_a_zero_environment(mirhi, oracle, device, scenes):
    """MODEL_PBR_IBL under an all-zero environment: direct light not scaled by ao, no hemisphere ambient (the model's ibl_zero_env)."""
    for base in (lc.sphere(scenes.PROGRAM_MODEL_PBR, 0.3), lc.ground(scenes.PROGRAM_MODEL_PBR)):
        sc = dataclasses.replace(_with(base, "IBL zero", program=scenes.PROGRAM_MODEL_PBR_IBL), ibl=scenes.ibl_test_images(zero=True))
        out = _render(mirhi, device, sc)
        _same_prims(out, _oracle_prim(oracle, base), sc.name)
        lc.check(None, sc, out["prim"], out["color"], "GPU", ibl_zero_env=True)


def test_lights_that_contribute_nothing_change_no_bit(mirhi, device, scenes):
    """A point light of intensity 0 and one out of reach of the whole mesh: the frame without them, bit for bit."""
    dark = (((0.5, 0.5, 2.0), 6.0, (1.0, 0.8, 0.6), 0.0), ((40.0, 30.0, -20.0), 3.0, (1.0, 1.0, 1.0), 50.0))
    for program, srgb in ((scenes.PROGRAM_MODEL_PBR, False), (scenes.PROGRAM_MODEL_FULL, True)):
        a = _render(mirhi, device, lc.sphere(program, 0.3, srgb))
        b = _render(mirhi, device, lc.sphere(program, 0.3, srgb, extra_points=dark))
        assert np.array_equal(a["prim"], b["prim"]) and np.array_equal(a["color"].view(np.uint32), b["color"].view(np.uint32))
