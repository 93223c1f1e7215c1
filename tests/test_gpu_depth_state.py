"""Depth bias and depth clamp on the GPU.  The oracle has neither state: the yardsticks are its unbiased depth, closed forms on
dyadic coordinates (every operation of the bias is then exact in binary32, so results are compared bit for bit) and the float64 model
scenes.depth_bias_offset.  All window coordinates below are in pixels of a 256 x 256 viewport (clip = (window - 128) / 128: dyadic for whole and
quarter pixels) over targets of 96 x 96 to 160 x 160 -- a 3 x 3 to 5 x 5 tile grid, partial tiles at 100 x 70."""
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VP = 256.0
NONE = 0xFFFFFFFF
Q = 2.0 ** -8
SLOPED = [(8, 8, 0.25), (72, 8, 0.5), (8, 72, 0.25)]          # dz/dx = 2^-8, dz/dy = 0; 3 x 3 tiles
FLAT = [(8, 8, 0.5), (72, 8, 0.5), (8, 72, 0.5)]


def _clip(pts):
    return [((x - VP / 2) / (VP / 2), (y - VP / 2) / (VP / 2), z) for x, y, z in pts]


def _draw(scenes, pts, **kw):
    """TRIANGLE-program draw of the triangles whose (window x, window y, depth) vertices are `pts`, cull none, full 256 x 256 viewport"""
    kw.setdefault("cull_mode", scenes.CULL_NONE)
    return scenes.DrawSpec(vertices=scenes._tri_verts(_clip(pts)), stride=24, count=len(pts), viewport=(0.0, 0.0, VP, VP, 0.0, 1.0), **kw)


def _scene(scenes, draws, w=96, h=96, **kw):
    return scenes.Scene("depth-state", w, h, draws if isinstance(draws, list) else [draws], **kw)


def _render(mirhi, device, scene, **kw):
    res = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT, want_prim=True, want_depth=True, **kw)
    res.render()
    out = res.read()
    res.destroy()
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_offset(base, out, offset, name, clear=1.0):
    """out = base with `offset` added to every covered depth, bit for bit (the sum is exact on the inputs used here); same coverage; clear elsewhere"""
    covered = base["prim"] != NONE
    assert covered.sum() > 0, name
    assert np.array_equal(out["prim"], base["prim"]), f"{name}: coverage differs from the unbiased render"
    want = (base["depth"].astype(np.float64) + offset)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want), f"{name}: the expectation is not exact in binary32"
    got = out["depth"]
    bad = _bits(got)[covered] != _bits(want)[covered]
    assert not bad.any(), f"{name}: {int(bad.sum())} of {int(covered.sum())} depths differ; first got {got[covered][bad][0]!r} want {want[covered][bad][0]!r}"
    assert np.all(got[~covered] == np.float32(clear)), f"{name}: uncovered pixels do not hold the clear value"


@pytest.fixture(scope="module")
def sloped_base(mirhi, scenes, device):
    """the unbiased render of SLOPED, rendered once"""
    return _render(mirhi, device, _scene(scenes, _draw(scenes, SLOPED)))


# 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1.0, 1000.0, -1000.0, 2.0 ** 20])
def test_constant_bias_is_exact(mirhi, scenes, device, c):
    base = _render(mirhi, device, _scene(scenes, _draw(scenes, FLAT)))
    out = _render(mirhi, device, _scene(scenes, _draw(scenes, FLAT, depth_bias=(c, 0.0, 0.0))))
    covered = base["prim"] != NONE
    assert 1900 < covered.sum() < 2200                           # half of 64 x 64
    assert np.all(_bits(base["depth"])[covered] == _bits(np.float32(0.5)))
    want = np.float32(0.5 + c * 2.0 ** -24)                       # r = 2^(-1 - 23) at z = 0.5
    assert float(want) == 0.5 + c * 2.0 ** -24
    assert np.all(_bits(out["depth"])[covered] == _bits(want)), (c, out["depth"][covered][0], want)
    assert np.all(out["depth"][~covered] == np.float32(1.0))
    assert np.array_equal(out["prim"], base["prim"])


# 2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("s", [1.0, 4.0, -4.0])
def test_slope_bias_is_exact(mirhi, scenes, device, sloped_base, s, reverse):
    pts = [SLOPED[0], SLOPED[2], SLOPED[1]] if reverse else SLOPED          # (reversed winding: the setup swaps vertices 1 and 2)
    out = _render(mirhi, device, _scene(scenes, _draw(scenes, pts, depth_bias=(0.0, 0.0, s))))
    assert scenes.depth_bias_offset([p[2] for p in pts], [p[:2] for p in pts], (0.0, 0.0, s)) == s * Q
    _assert_offset(sloped_base, out, s * Q, f"slope {s} reverse {reverse}")


# 3 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s, clamp", [(4.0, Q), (-4.0, -Q), (4.0, -Q), (-4.0, Q)])
def test_bias_clamp(mirhi, scenes, device, sloped_base, s, clamp):
    """clamp > 0 bounds the offset from above, clamp < 0 from below: the first two cases give exactly the clamp, the other two leave s * 2^-8"""
    out = _render(mirhi, device, _scene(scenes, _draw(scenes, SLOPED, depth_bias=(0.0, clamp, s))))
    want = scenes.depth_bias_offset([p[2] for p in SLOPED], [p[:2] for p in SLOPED], (0.0, clamp, s))
    assert want == (clamp if (s > 0) == (clamp > 0) else s * Q)
    _assert_offset(sloped_base, out, want, f"slope {s} clamp {clamp}")


# 4 ---------------------------------------------------------------------------------------------------------------------------------------
GENERAL_FACTORS = (64.0, 0.0, 1.5)
# Largest relative difference |constant - o| / |o| between a triangle's measured offset and the float64 model on the first GPU run, and the bound
# asserted: four times that (other seeds see worse conditioning in zx's numerator); DESIGN.md 8h carries both.  Never above 1e-3.
GENERAL_MEASURED = 1.577e-5
GENERAL_TOL = 4.0 * GENERAL_MEASURED


def _general_triangles(scenes, seed=0x5EED0D5):
    """64 triangles, one per 16 x 16 cell of a 128 x 128 target, under a perspective camera; returns the draws and per triangle the window-space
    vertices (x, y, z) recomputed in float64 from the float32 inputs, x / y snapped to 1/256 px as the setup snaps them."""
    rng = np.random.default_rng(seed)
    size = 128
    view, proj, cam = scenes.default_camera(size, size, eye=(0.0, 0.0, 3.0))
    vp = scenes.mat_mul(proj, view).astype(np.float64).T          # [row, col]
    inv = np.linalg.inv(vp)
    eye4 = np.eye(4, dtype=np.float32)
    draws, windows = [], []
    for cell in range(64):
        cx, cy = 16.0 * (cell % 8), 16.0 * (cell // 8)
        while True:
            xy = rng.uniform(1.0, 15.0, size=(3, 2)) + (cx, cy)
            z = rng.uniform(0.3, 0.7, size=3)
            area = abs((xy[1, 0] - xy[0, 0]) * (xy[2, 1] - xy[0, 1]) - (xy[2, 0] - xy[0, 0]) * (xy[1, 1] - xy[0, 1])) / 2.0
            if area >= 70.0:
                break
        ndc = np.concatenate([(xy - size / 2) / (size / 2), z[:, None], np.ones((3, 1))], axis=1)
        world = (inv @ ndc.T).T
        world = (world[:, :3] / world[:, 3:4]).astype(np.float32)
        clip = (vp @ np.concatenate([world.astype(np.float64), np.ones((3, 1))], axis=1).T).T
        win = np.stack([np.rint((clip[:, 0] / clip[:, 3] * (size / 2) + size / 2) * 256.0) / 256.0,
                        np.rint((clip[:, 1] / clip[:, 3] * (size / 2) + size / 2) * 256.0) / 256.0, clip[:, 2] / clip[:, 3]], axis=1)
        windows.append(win)
        verts = scenes._pack_vertex48(world, np.tile([0.0, 0.0, 1.0], (3, 1)), np.zeros((3, 2)), np.tile([1.0, 0.0, 0.0, 1.0], (3, 1)))
        draws.append(scenes.DrawSpec(vertices=verts, stride=48, count=3, program=scenes.PROGRAM_MODEL, cull_mode=scenes.CULL_NONE, camera=cam,
                                     object=scenes.object_ubo(eye4)))
    return size, draws, windows


def test_general_triangles_against_the_float64_model(mirhi, scenes, device):
    size, draws, windows = _general_triangles(scenes)
    model = []
    for win in windows:                                           # the constraint, checked on the CPU before anything is launched
        o = scenes.depth_bias_offset(win[:, 2], win[:, :2], GENERAL_FACTORS)
        x, y = win[:, 0], win[:, 1]
        area = abs((x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])) / 2.0
        assert 0.25 <= win[:, 2].min() and win[:, 2].max() <= 0.75 and area >= 64.0 and abs(o) <= 0.1, (win, o)
        assert win[:, 2].min() + min(o, 0.0) > 0.0 and win[:, 2].max() + max(o, 0.0) < 1.0
        model.append(o)
    base = _render(mirhi, device, scenes.Scene("general", size, size, draws))
    biased = _render(mirhi, device, scenes.Scene("general-biased", size, size, [dataclasses.replace(d, depth_bias=GENERAL_FACTORS) for d in draws]))
    assert np.array_equal(base["prim"], biased["prim"])
    diff = biased["depth"].astype(np.float64) - base["depth"].astype(np.float64)
    worst_rel, worst_spread = 0.0, 0.0
    for k, o in enumerate(model):
        mine = base["prim"] == k
        assert mine.sum() >= 40, (k, int(mine.sum()))
        d = diff[mine]
        const = float(np.median(d))
        worst_spread = max(worst_spread, float(np.abs(d - const).max()))
        worst_rel = max(worst_rel, abs(const - o) / abs(o))
    print(f"general triangles: offset constant within {worst_spread / 2.0 ** -24:.3f} x 2^-24 (bound 3), largest relative difference to the model {worst_rel:.3e} "
          f"(asserted {GENERAL_TOL:.3e})")
    assert worst_spread <= 3.0 * 2.0 ** -24
    assert GENERAL_TOL <= 1e-3
    assert worst_rel <= GENERAL_TOL


# 5 ---------------------------------------------------------------------------------------------------------------------------------------
SMALL = [(10.25, 10.25, 0.25), (11.25, 10.25, 0.25 + Q), (10.25, 11.25, 0.25)]                   # covers the centre of pixel (10, 10): the one-bin path
BIG = [(0, 0, 0.25), (160, 0, 0.25 + 160 * 2.0 ** -9), (0, 160, 0.25)]                           # 5 x 5 tiles: the big list; dz/dx = 2^-9
# crosses the left guard-band plane (clip x = -124 w): its two cut points are exact (t = 124 / 128), so the pieces' planes are too; dz/dx = 2^-17 and
# all depths within [0.25, 0.5)
GUARD = [(-16256, 40, 0.25), (128, 8, 0.375), (128, 72, 0.375)]
ROUTES = {"small": (SMALL, Q, 96, 96), "partial-tiles": (SLOPED, Q, 100, 70), "big": (BIG, 2.0 ** -9, 160, 160), "guard-band": (GUARD, 2.0 ** -17, 160, 96)}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("s", [4.0, -4.0])
def test_routes_through_the_geometry_stage(mirhi, scenes, device, route, s):
    pts, slope, w, h = ROUTES[route]
    base = _render(mirhi, device, _scene(scenes, _draw(scenes, pts), w, h))
    out = _render(mirhi, device, _scene(scenes, _draw(scenes, pts, depth_bias=(0.0, 0.0, s)), w, h))
    covered = int((base["prim"] != NONE).sum())
    assert covered >= {"small": 1, "partial-tiles": 1900, "big": 12000, "guard-band": 2000}[route], covered
    _assert_offset(base, out, s * slope, f"{route} slope {s}")


def test_route_blended_pipeline(mirhi, scenes, device, sloped_base):
    """an ordered segment (blending on: src * 1 + dst * 0), depth read back"""
    M = mirhi
    blend = (M.BlendFactor.One, M.BlendFactor.Zero, M.BlendOp.Add, M.BlendFactor.One, M.BlendFactor.Zero, M.BlendOp.Add, 0xF)
    base = _render(mirhi, device, _scene(scenes, _draw(scenes, SLOPED, blend=blend)))
    assert np.array_equal(_bits(base["depth"]), _bits(sloped_base["depth"])) and np.array_equal(base["prim"], sloped_base["prim"])
    for s in (4.0, -4.0):
        out = _render(mirhi, device, _scene(scenes, _draw(scenes, SLOPED, blend=blend, depth_bias=(0.0, 0.0, s))))
        _assert_offset(sloped_base, out, s * Q, f"blended slope {s}")
    # ... and a clipped triangle in an ordered segment: its pieces go through setup_triangle three times (count, reserve, store)
    pts, slope, w, h = ROUTES["guard-band"]
    base = _render(mirhi, device, _scene(scenes, _draw(scenes, pts, blend=blend), w, h))
    out = _render(mirhi, device, _scene(scenes, _draw(scenes, pts, blend=blend, depth_bias=(0.0, 0.0, 4.0)), w, h))
    _assert_offset(base, out, 4.0 * slope, "blended guard-band")


def _model_draw(scenes, pts, program, **kw):
    """the same triangle through the MODEL vertex stage: identity camera and object matrices, so clip = position"""
    eye4 = np.eye(4, dtype=np.float32)
    pos = np.asarray(_clip(pts), dtype=np.float32)
    verts = scenes._pack_vertex48(pos, np.tile([0.0, 0.0, 1.0], (3, 1)), np.zeros((3, 2)), np.tile([1.0, 0.0, 0.0, 1.0], (3, 1)))
    return scenes.DrawSpec(vertices=verts, stride=48, count=3, program=program, cull_mode=scenes.CULL_NONE, viewport=(0.0, 0.0, VP, VP, 0.0, 1.0),
                           camera=scenes.camera_ubo(eye4, eye4, (0.0, 0.0, 1.0)), object=scenes.object_ubo(eye4), **kw)


def test_route_fragment_discard_pipeline(mirhi, scenes, device, sloped_base):
    """MODEL_PBR with fragment_discard_enable, alpha 1 above the cutoff 0.5: the alpha scope"""
    kw = dict(light=scenes.light_ubo(direction=(0.0, 0.0, -1.0), intensity=1.0), material=scenes.pbr_material_ubo((0.8, 0.7, 0.6, 1.0), 0.0, 0.5, alpha_cutoff=0.5),
              alpha_test=True)
    base = _render(mirhi, device, _scene(scenes, _model_draw(scenes, SLOPED, scenes.PROGRAM_MODEL_PBR, **kw)))
    assert np.array_equal(_bits(base["depth"]), _bits(sloped_base["depth"])) and np.array_equal(base["prim"], sloped_base["prim"])
    for s in (4.0, -4.0):
        out = _render(mirhi, device, _scene(scenes, _model_draw(scenes, SLOPED, scenes.PROGRAM_MODEL_PBR, depth_bias=(0.0, 0.0, s), **kw)))
        _assert_offset(sloped_base, out, s * Q, f"discard slope {s}")


def _shadow_map(mirhi, scenes, device, pts, size, **spec_kw):
    """`pts` (in pixels of the map, whose viewport is its extent) drawn by the SHADOW program into a size x size map -- identity light matrix: clip =
    position; returns the map"""
    eye4 = np.eye(4, dtype=np.float32)
    pos = np.asarray([((x - size / 2) / (size / 2), (y - size / 2) / (size / 2), z) for x, y, z in pts], dtype=np.float32)
    verts = scenes._pack_vertex48(pos, np.tile([0.0, 0.0, 1.0], (len(pts), 1)), np.zeros((len(pts), 2)), np.tile([1.0, 0.0, 0.0, 1.0], (len(pts), 1)))
    caster = scenes.DrawSpec(vertices=verts, stride=48, count=len(pts), program=scenes.PROGRAM_SHADOW, cull_mode=scenes.CULL_NONE,
                             camera=scenes.shadow_constants_ubo(eye4, eye4))
    scene = scenes.Scene("depth-only", 32, 32, [], shadow=scenes.ShadowSpec([caster], (size, size), scenes.shadow_ubo(eye4, 0.0, 0.0, (size, size)), **spec_kw))
    res = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT)
    res.render()
    device.wait_idle()
    out = res.shadow_map.read().reshape(size, size).copy()
    res.destroy()
    return out


def test_route_depth_only_shadow_scope(mirhi, scenes, device, sloped_base):
    """SLOPED in a 128 x 128 map: the same window coordinates as in the colour scope, so the same depth bits"""
    base = _shadow_map(mirhi, scenes, device, SLOPED, 128)
    assert np.array_equal(_bits(base[:96, :96]), _bits(sloped_base["depth"])), "the SHADOW scope's depth differs from the TRIANGLE program's"
    covered = base != np.float32(1.0)
    assert 1900 < covered.sum() < 2200
    for s in (4.0, -4.0):
        out = _shadow_map(mirhi, scenes, device, SLOPED, 128, depth_bias=(0.0, 0.0, s))       # (the ShadowSpec's factors: the caster has none of its own)
        want = np.where(covered, base.astype(np.float64) + s * Q, 1.0)
        assert np.array_equal(_bits(out), _bits(want)), f"shadow scope slope {s}"


@pytest.mark.skipif(os.environ.get("MIRHI_NATIVE_DISPATCH") == "0", reason="native dispatch switched off for this run")
def test_route_both_dispatch_paths(mirhi, scenes, sloped_base):
    dev = mirhi.Device(0, stream=0)
    outs, used = [], []
    try:
        res = mirhi.SceneResources(dev, _scene(scenes, _draw(scenes, SLOPED, depth_bias=(0.0, 0.0, 4.0))), want_prim=True, want_depth=True)
        fence = mirhi.Fence(dev)
        for native in (False, True):
            dev.set_native_dispatch(native)
            before = dev.stats().native_dispatches
            res.render(fence)
            fence.wait(); fence.reset()
            used.append((dev.dispatch_path(), dev.stats().native_dispatches - before))
            outs.append(res.read())
        res.destroy(); fence.destroy()
    finally:
        dev.destroy()
    assert used[0][1] == 0 and used[1][1] > 0 and used[1][0].startswith("native:"), used
    for out in outs:
        _assert_offset(sloped_base, out, 4.0 * Q, "dispatch path")


# 6 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op, clear, winner", [("CMP_LESS", 1.0, 1), ("CMP_LESS_OR_EQUAL", 1.0, 1), ("CMP_GREATER", 0.0, 0), ("CMP_GREATER_OR_EQUAL", 0.0, 0),
                                               ("CMP_EQUAL", 0.5, 0)])
def test_compare_ops_see_the_biased_depth(mirhi, scenes, device, op, clear, winner):
    """Two coplanar triangles at z = 0.5, the second with constant bias -1000 (depth 0.5 - 1000 * 2^-24): the decal case.  Without the bias the second
    ties with the first: LESS / GREATER keep the first, the OR_EQUAL ops and EQUAL (clear 0.5) take the second."""
    cmp_op = getattr(scenes, op)
    mk = lambda bias: _scene(scenes, [_draw(scenes, FLAT, depth_compare=cmp_op), _draw(scenes, FLAT, depth_compare=cmp_op, depth_bias=bias)], clear_depth=clear)
    out = _render(mirhi, device, mk((-1000.0, 0.0, 0.0)))
    tie = _render(mirhi, device, mk(None))
    covered = tie["prim"] != NONE
    assert 1900 < covered.sum() < 2200 and np.array_equal(out["prim"] != NONE, covered)
    lower = np.float32(0.5 - 1000.0 * 2.0 ** -24)
    assert np.all(out["prim"][covered] == winner), (op, np.unique(out["prim"][covered]))
    assert np.all(_bits(out["depth"])[covered] == _bits(lower if winner == 1 else np.float32(0.5)))
    assert np.all(tie["prim"][covered] == (0 if op in ("CMP_LESS", "CMP_GREATER") else 1)), (op, np.unique(tie["prim"][covered]))
    assert np.all(_bits(tie["depth"])[covered] == _bits(np.float32(0.5)))


# 7 ---------------------------------------------------------------------------------------------------------------------------------------
RAMP = [(8, 8, -0.5), (136, 8, 1.5), (8, 72, -0.5)]               # depth plane -0.5 + (x - 8) / 64


def test_depth_clamp_colour_scope(mirhi, scenes, oracle, device):
    le = scenes.CMP_LESS_OR_EQUAL
    on = _render(mirhi, device, _scene(scenes, _draw(scenes, RAMP, depth_compare=le, depth_clamp=True), 160, 96))
    flat = _render(mirhi, device, _scene(scenes, _draw(scenes, [(x, y, 0.5) for x, y, _ in RAMP], depth_compare=le), 160, 96))
    off_scene = _scene(scenes, _draw(scenes, RAMP, depth_compare=le), 160, 96)
    off = _render(mirhi, device, off_scene)
    ref = oracle.render(off_scene, want_bgra8=False)
    footprint = flat["prim"] != NONE
    assert 3900 < footprint.sum() < 4300                          # half of 128 x 64
    assert np.array_equal(on["prim"], flat["prim"]), "clamp on: coverage is not the triangle's full 2-D footprint"
    px = np.arange(160)[None, :] + 0.5
    plane = np.broadcast_to(np.clip(-0.5 + (px - 8.0) / 64.0, 0.0, 1.0), (96, 160))
    assert np.all(on["depth"][footprint] == plane[footprint].astype(np.float32)), "clamp on: depth is not min(max(plane, 0), 1)"
    assert np.all(on["depth"][~footprint] == np.float32(1.0))
    assert (on["depth"][footprint] == 0.0).sum() > 500 and (on["depth"][footprint] == 1.0).sum() > 100      # both ends are there
    # clamp off: as today, the two ends cut away
    assert np.array_equal(off["prim"], ref["prim"]) and np.array_equal(_bits(off["depth"]), _bits(ref["depth"]))
    cut = off["prim"] != NONE
    assert cut.sum() < footprint.sum() - 600 and not (cut & ~footprint).any()
    assert np.array_equal(_bits(on["depth"])[cut], _bits(off["depth"])[cut]), "inside the depth range clamp changes nothing"


def _perspective_draws(scenes, size, far, tri, **kw):
    view = scenes.look_at_rh((0.0, 0.0, 2.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    proj = scenes.projection_vulkan(np.radians(60.0), 1.0, 0.25, far)
    cam = scenes.camera_ubo(view, proj, (0.0, 0.0, 2.0))
    pos = np.asarray(tri, dtype=np.float32)
    verts = scenes._pack_vertex48(pos, np.tile([0.0, 0.0, 1.0], (3, 1)), np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), np.tile([1.0, 0.0, 0.0, 1.0], (3, 1)))
    return scenes.DrawSpec(vertices=verts, stride=48, count=3, program=scenes.PROGRAM_MODEL, cull_mode=scenes.CULL_NONE, camera=cam,
                           object=scenes.object_ubo(np.eye(4, dtype=np.float32)), depth_compare=scenes.CMP_LESS_OR_EQUAL, **kw)


@pytest.mark.parametrize("case", ["beyond-far", "behind-eye"])
def test_depth_clamp_perspective(mirhi, scenes, oracle, device, case):
    """beyond-far: a vertex behind the far plane (far 2, all w >= 0.25).  x, y and w do not depend on the far plane: the clamped frame covers what the
    oracle covers with the far plane moved out to 100, with the same primitive and colour.  behind-eye: one vertex behind the eye (w < 0) as well --
    the guard-band planes cut it at w >= 0, and wherever the oracle (which cuts at the near plane) has coverage, the frame is the oracle's."""
    size = 96
    tri = {"beyond-far": [(-0.6, -0.5, 1.0), (0.7, -0.4, 0.5), (0.1, 0.6, -6.0)],
           "behind-eye": [(-1.5, -1.0, -1.0), (2.7, 1.4, -6.0), (0.1, -0.3, 2.5)]}[case]
    got = _render(mirhi, device, scenes.Scene(case, size, size, [_perspective_draws(scenes, size, 2.0, tri, depth_clamp=True)]))
    ref = oracle.render(scenes.Scene(case, size, size, [_perspective_draws(scenes, size, 100.0, tri)]), want_bgra8=False)
    near_cut = oracle.render(scenes.Scene(case, size, size, [_perspective_draws(scenes, size, 2.0, tri)]), want_bgra8=False)
    seen = ref["prim"] != NONE
    assert seen.sum() > 300 and (near_cut["prim"] != NONE).sum() < seen.sum() - 100, "the far plane cuts nothing away: the case tests nothing"
    assert np.all(got["prim"][seen] == 0), f"{case}: {int((got['prim'][seen] != 0).sum())} pixels the oracle covers are missing"
    if case == "beyond-far":
        assert np.array_equal(got["prim"], ref["prim"])
    a, b = got["color"][..., :3].astype(np.float64)[seen], ref["rgba"][..., :3].astype(np.float64)[seen]
    err = float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())
    assert err < 1e-4, f"{case}: max |dRGB| = {err}"          # the parity tests' bound
    # the oracle's far-plane cut is an edge of its own, snapped like any other: a pixel beside it can be on the other side by a fraction of a pixel.  A pixel
    # the far-cut render does not cover in its whole 3 x 3 neighbourhood is beyond the far plane for certain
    inside = near_cut["prim"] != NONE
    near_inside = np.zeros_like(inside)
    pad = np.pad(inside, 1)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            near_inside |= pad[dy:dy + size, dx:dx + size]
    beyond = got["depth"][seen & ~near_inside]
    assert beyond.size > 100 and np.all(beyond == 1.0), "fragments beyond the far plane are not clamped to 1"
    edge = got["depth"][seen & ~inside & near_inside]
    assert np.all((edge > 0.9) & (edge <= 1.0))
    # In-range depth against the far = 2 oracle render, away from its cut edges.  Two float32 planes of the same exact plane, built from different vertex
    # sets (the oracle's clipped pieces, this build's whole triangle or its guard-band pieces): no closed-form bound.  Largest difference measured on
    # the first GPU run: 9.477e-6 (beyond-far), 3.4e-5 (behind-eye, whose pieces are cut where w -> 0+ and carry window depths of the order of -100,
    # DESIGN.md 8h); asserted: four times that, the rule of the general-triangle test.
    eroded = inside.copy()
    padc = np.pad(inside, 1)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            eroded &= padc[dy:dy + size, dx:dx + size]
    worst = float(np.abs(got["depth"][eroded].astype(np.float64) - near_cut["depth"][eroded]).max())
    bound = 4.0 * {"beyond-far": 9.477e-6, "behind-eye": 3.4e-5}[case]
    print(f"{case}: largest in-range depth difference to the far-cut oracle {worst:.3e} on {int(eroded.sum())} pixels (asserted {bound:.3e})")
    assert eroded.sum() > 500 and worst <= bound
    if case == "beyond-far":
        # Inside the depth range the clamp must change nothing.  With the far plane at 100 the whole triangle is inside it and nothing is clipped on
        # either side: the clamped draw is then the oracle's frame bit for bit, depth included (all w >= 0.25; the behind-eye triangle is cut where
        # w -> 0+, the one place the depth of a clamped draw is documented as ill-conditioned)
        whole = _render(mirhi, device, scenes.Scene(case, size, size, [_perspective_draws(scenes, size, 100.0, tri, depth_clamp=True)]))
        assert np.array_equal(whole["prim"], ref["prim"])
        assert np.array_equal(_bits(whole["depth"])[seen], _bits(ref["depth"])[seen]), "a clamped draw inside the depth range differs from the oracle's depth"
        assert np.all(whole["depth"][~seen] == np.float32(1.0))


# 8 / 9 -----------------------------------------------------------------------------------------------------------------------------------
# The rig of test_gpu_shadow.py's PCF test: an orthographic light straight down, the camera has the light's frustum at twice the map's resolution, so
# pixel centres sit at quarter-texel points and pixel (px, py) samples the map at u = (px + 1/2) / size, v = 1 - (py + 1/2) / size.  NormalBias 0 and
# ShadowBias 0: CalculateShadow's reference depth is the fragment's light-space depth -- the depth the main scope stores -- minus its floor of 0.0005.
RIG_MAP, RIG_SIZE, RGB_TOL = 64, 128, 1e-4          # (RGB_TOL: test_gpu_shadow.py's bound)


def _rig_light(scenes):
    return scenes.light_space_matrix((0.0, -1.0, 0.0), half_extent=2.0, near=0.1, far=20.0)


def _quad(scenes, corners, normal):
    pos = np.asarray(corners, dtype=np.float64)
    verts = scenes._pack_vertex48(pos, np.tile(np.asarray(normal, dtype=np.float64), (4, 1)), np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]),
                                  np.tile([1.0, 0.0, 0.0, 1.0], (4, 1)))
    return verts, np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32)


def _rig_scene(scenes, receiver, casters, intensity=3.0, shadow=True, **spec_kw):
    """receiver: (vertices, indices) drawn by MODEL_PBR through the light's own frustum and, with every quad of `casters`, by SHADOW into the map"""
    ls = _rig_light(scenes)
    eye4 = np.eye(4, dtype=np.float32)
    zero = np.zeros((4, 4), dtype=np.float32)
    cam = zero.tobytes() + zero.tobytes() + ls.astype(np.float32).tobytes() + np.array([0.0, 10.0, 0.0, 0.0], dtype=np.float32).tobytes()
    rv, ri = receiver
    d = scenes.DrawSpec(vertices=rv, stride=48, count=ri.size, indices=ri, program=scenes.PROGRAM_MODEL_PBR, cull_mode=scenes.CULL_NONE, camera=cam,
                        object=scenes.object_ubo(eye4), light=scenes.light_ubo(direction=(0.0, -1.0, 0.0), intensity=intensity, color=(1.0, 0.9, 0.8)),
                        material=scenes.pbr_material_ubo((0.7, 0.7, 0.7, 1.0), 0.0, 0.6))
    sh = None
    if shadow:
        cs = [scenes.DrawSpec(vertices=v, stride=48, count=i.size, indices=i, program=scenes.PROGRAM_SHADOW, cull_mode=scenes.CULL_NONE,
                              camera=scenes.shadow_constants_ubo(scenes.flip_clip_y(ls), eye4)) for v, i in [receiver] + list(casters)]
        sh = scenes.ShadowSpec(cs, (RIG_MAP, RIG_MAP), scenes.shadow_ubo(ls, 0.0, 0.0, (RIG_MAP, RIG_MAP), 1.0), **spec_kw)
    return scenes.Scene("depth-state-rig", RIG_SIZE, RIG_SIZE, [d], shadow=sh)


def _rig_frame(mirhi, scenes, oracle, device, receiver, casters, **spec_kw):
    """renders the rig; returns the map read back, the numpy PCF factor of that map per pixel, and checks the frame against unlit + s (lit - unlit)"""
    res = mirhi.SceneResources(device, _rig_scene(scenes, receiver, casters, **spec_kw), mirhi.Format.R32G32B32A32_SFLOAT, want_depth=True)
    res.render()
    out = res.read()
    smap = res.shadow_map.read().reshape(RIG_MAP, RIG_MAP).copy()
    res.destroy()
    lit = oracle.render(_rig_scene(scenes, receiver, casters, shadow=False), want_bgra8=False)["rgba"]
    unlit = oracle.render(_rig_scene(scenes, receiver, casters, intensity=0.0, shadow=False), want_bgra8=False)["rgba"]
    px, py = np.meshgrid(np.arange(RIG_SIZE), np.arange(RIG_SIZE), indexing="xy")
    u, v = (px + 0.5) / RIG_SIZE, 1.0 - (py + 0.5) / RIG_SIZE
    s = scenes.pcf_factor(smap, u, v, out["depth"].astype(np.float64) - 0.0005)
    expect = unlit[..., :3].astype(np.float64) + s[..., None] * (lit[..., :3].astype(np.float64) - unlit[..., :3])
    err = np.abs(out["color"][..., :3].astype(np.float64) - expect) / np.maximum(1.0, np.abs(expect))
    assert float(np.abs(lit[..., :3] - unlit[..., :3]).max()) > 0.05, "the light changes nothing: the frame cannot show a shadow"
    assert float(err.max()) < RGB_TOL, f"frame differs from the PCF model of the map read back: max |dRGB| = {float(err.max())} at {np.argwhere(err.max(axis=-1) == err.max())[0]}"
    return smap, s


def test_pancaking_in_the_light_aligned_rig(mirhi, scenes, oracle, device):
    """A caster in front of the light's near plane (light at y = 10, near 0.1: the quad at y = 9.95 has clip z < 0) over flat ground.  Without depth
    clamp it is clipped away, the map is the ground's depth and the ground is lit; with clamp the map holds 0 under it and the ground there is shadowed."""
    ground = _quad(scenes, [(-3, 0, 3), (3, 0, 3), (3, 0, -3), (-3, 0, -3)], (0, 1, 0))
    caster = _quad(scenes, [(-0.75, 9.95, 1.0), (0.5, 9.95, 1.0), (0.5, 9.95, -0.25), (-0.75, 9.95, -0.25)], (0, 1, 0))
    smap, s = _rig_frame(mirhi, scenes, oracle, device, ground, [caster])
    ground_depth = np.float32(smap[0, 0])
    assert 0.4 < ground_depth < 0.6 and np.all(smap == ground_depth), "without clamp the caster must leave no trace in the map"
    assert np.all(s == 1.0)
    smap, s = _rig_frame(mirhi, scenes, oracle, device, ground, [caster], depth_clamp=True)
    under = smap == 0.0
    assert 300 < under.sum() < 500 and np.all(smap[~under] == ground_depth), int(under.sum())       # 1.25 x 1.25 world units of 4 x 4 = 20 x 20 texels
    assert (s == 0.0).sum() > 1000 and (s == 1.0).sum() > 10000


def test_acne_and_its_cure_by_slope_bias(mirhi, scenes, oracle, device):
    """A receiver tilted 60 degrees to the light, map 64 x 64, ShadowBias 0: one texel's depth step is ten times CalculateShadow's floor of 0.0005, and
    the numpy PCF model of the unbiased map predicts self-shadow stripes.  A slope factor of 2 lifts every texel by two steps: factor 1 everywhere."""
    t, q = np.sqrt(3.0), 3.0
    plane = _quad(scenes, [(-q, -t * q, q), (q, t * q, q), (q, t * q, -q), (-q, -t * q, -q)], (-t / 2.0, 0.5, 0.0))
    # the depth step per texel from the model: the caster's first triangle in the map's window space
    m = scenes.flip_clip_y(_rig_light(scenes)).astype(np.float64).T
    clip = (m @ np.concatenate([np.asarray(plane[0], dtype=np.float64).reshape(-1, 12)[:3, 0:3], np.ones((3, 1))], axis=1).T).T
    win_xy, win_z = (clip[:, :2] / clip[:, 3:4] + 1.0) * RIG_MAP / 2.0, clip[:, 2] / clip[:, 3]
    step = scenes.depth_bias_offset(win_z, win_xy, (0.0, 0.0, 1.0))
    assert step > 10 * 0.0005 and abs(step - 4.0 / RIG_MAP * t / 19.9) < 1e-6
    factors = (0.0, 0.0, 2.0)
    assert scenes.depth_bias_offset(win_z, win_xy, factors) > 1.5 * step
    smap, s = _rig_frame(mirhi, scenes, oracle, device, plane, [])
    assert 0.25 < (s < 1.0).mean() and s.min() < 0.7, "the model predicts no acne: the scene does not have the problem"
    smap_b, s_b = _rig_frame(mirhi, scenes, oracle, device, plane, [], depth_bias=factors)
    assert np.all(s_b == 1.0), "the model still predicts self-shadowing with the slope bias"
    d = smap_b.astype(np.float64) - smap
    assert np.all(np.abs(d - 2.0 * step) < 1e-6)


# 8, on the issue's scenes ---------------------------------------------------------------------------------------------------------------
# shadowed_ground_case / cascaded_ground_case with the caster box moved towards the light until all of it lies in front of the light's near plane.  The
# lit scope is the scene's ground draw: CalculateShadow needs a fragment's world position and normal, and the ground gives both in closed form for
# every pixel (the pixel's ray cut with y = 0, normal +y) -- a model of the interpolated normals of the sphere would be a second renderer.
def _ground_hits(scenes, w, h, eye, target=(0.0, 0.0, 0.0)):
    """world position of the y = 0 plane under every pixel centre (float64), as test_gpu_shadow.py's footprint model has it"""
    view, proj, _ = scenes.default_camera(w, h, eye=eye, target=target)
    inv = np.linalg.inv(scenes.mat_mul(proj, view).T.astype(np.float64))
    px, py = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5, indexing="xy")
    nx, ny = px / w * 2 - 1, py / h * 2 - 1

    def unproject(z):
        p = np.stack([nx, ny, np.full_like(nx, z), np.ones_like(nx)], axis=-1) @ inv.T
        return p[..., :3] / p[..., 3:4]
    a, b = unproject(0.0), unproject(1.0)
    t = a[..., 1] / (a[..., 1] - b[..., 1])
    return a + (b - a) * t[..., None]


def _lift_in_front_of_near(scenes, light_matrix, light_dir, vertices):
    """model matrix that moves the mesh towards the light until its largest clip z (w = 1: orthographic) is -0.02; checked in float64"""
    d = np.asarray(light_dir, dtype=np.float64)
    d = d / np.linalg.norm(d)
    pos = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 12)[:, 0:3].astype(np.float64)
    m = np.asarray(light_matrix, dtype=np.float64)

    def zmax(delta):
        p4 = np.concatenate([pos - d * delta, np.ones((len(pos), 1))], axis=1) @ m
        assert np.allclose(p4[:, 3], 1.0)
        return float(p4[:, 2].max())
    z0, z1 = zmax(0.0), zmax(1.0)
    delta = (-0.02 - z0) / (z1 - z0)
    assert delta > 0 and zmax(delta) < -0.01
    return scenes.trs((1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 1.0), tuple(-d * delta)), delta


def _single_map_factor(scenes, smap, light_matrix, world, normal, to_light, bias, normal_bias):
    """CalculateShadow (shadow.hlsli:49-121) in float64 over scenes.pcf_factor: bounds test on the position, the nine taps on the offset position"""
    m = np.asarray(light_matrix, dtype=np.float64)
    n = np.asarray(normal, dtype=np.float64)
    p = np.concatenate([world, np.ones(world.shape[:-1] + (1,))], axis=-1) @ m
    p = p[..., :3] / p[..., 3:4]
    u0, v0 = p[..., 0] * 0.5 + 0.5, 1.0 - (p[..., 1] * 0.5 + 0.5)
    inside = (u0 >= 0) & (u0 <= 1) & (v0 >= 0) & (v0 <= 1) & (p[..., 2] >= 0) & (p[..., 2] <= 1)
    ab = max(bias * (1.0 - float(n @ np.asarray(to_light, dtype=np.float64))), 0.0005)
    o = np.concatenate([world + n * normal_bias, np.ones(world.shape[:-1] + (1,))], axis=-1) @ m
    o = o[..., :3] / o[..., 3:4]
    s = scenes.pcf_factor(smap, o[..., 0] * 0.5 + 0.5, 1.0 - (o[..., 1] * 0.5 + 0.5), o[..., 2] - ab)
    return np.where(inside, s, 1.0)


def _assert_frame(out_rgba, lit, unlit, s, name):
    expect = unlit[..., :3].astype(np.float64) + s[..., None] * (lit[..., :3].astype(np.float64) - unlit[..., :3])
    err = np.abs(out_rgba[..., :3].astype(np.float64) - expect) / np.maximum(1.0, np.abs(expect))
    bad = err.max(axis=-1) >= RGB_TOL
    assert not bad.any(), f"{name}: {int(bad.sum())} pixels differ from the PCF model of the map read back, max |dRGB| = {float(err.max())}, first at {np.argwhere(bad)[0]}"


def test_pancaking_shadowed_ground_case(mirhi, scenes, oracle, device):
    w, h, msize = 160, 120, 128
    base = scenes.shadowed_ground_case(w, h, map_size=msize)
    light_dir = np.asarray(scenes.SHADOWED_GROUND_LIGHT, dtype=np.float64)
    to_light = -light_dir / np.linalg.norm(light_dir)
    ls = scenes.light_space_matrix(scenes.SHADOWED_GROUND_LIGHT, half_extent=scenes.SHADOWED_GROUND_EXTENT)
    box = base.shadow.casters[0]
    lift, _ = _lift_in_front_of_near(scenes, ls, light_dir, box.vertices)
    caster = dataclasses.replace(box, camera=scenes.shadow_constants_ubo(scenes.flip_clip_y(ls), lift))
    ground_only = lambda sc: dataclasses.replace(sc, draws=[sc.draws[0]], shadow=None)
    lit = oracle.render(ground_only(base), want_bgra8=False)
    unlit = oracle.render(ground_only(scenes.shadowed_ground_case(w, h, map_size=msize, intensity=0.0)), want_bgra8=False)["rgba"]
    ground = lit["prim"] != NONE
    hits = _ground_hits(scenes, w, h, (0.0, 4.5, 6.5))
    assert ground.sum() > 5000 and float(np.abs(lit["rgba"][..., :3] - unlit[..., :3])[ground].min()) > 0.05
    for clamp in (False, True):
        scene = dataclasses.replace(base, draws=[base.draws[0]], shadow=dataclasses.replace(base.shadow, casters=[caster], depth_clamp=clamp))
        res = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT, want_prim=True)
        res.render()
        out = res.read()
        smap = res.shadow_map.read().reshape(msize, msize).copy()
        res.destroy()
        assert np.array_equal(out["prim"], lit["prim"])
        under = smap == 0.0
        assert np.all(smap[~under] == 1.0)
        s = np.where(ground, _single_map_factor(scenes, smap, ls, hits, (0.0, 1.0, 0.0), to_light, 0.005, 0.02), 1.0)
        if clamp:
            assert under.sum() > 100, "with depth clamp the caster must be in the map at depth 0"
            assert (s[ground] == 0.0).sum() > 100 and (s[ground] == 1.0).sum() > 3000 and ((s[ground] > 0) & (s[ground] < 1)).sum() > 20
        else:
            assert not under.any(), "without depth clamp the caster is clipped away: the map stays cleared"
            assert np.all(s == 1.0)
        _assert_frame(out["color"], lit["rgba"], unlit, s, f"shadowed_ground_case clamp {clamp}")


def test_pancaking_in_one_cascade(mirhi, scenes, oracle, device):
    """cascaded_ground_case: cascade 1's own box, moved in front of that cascade's near plane, is the only caster of the four scopes.  CascadeSpec's
    depth_clamp goes to the pipelines of all four; the frame against scenes.csm_factor of the array read back, on every pixel."""
    w, h, msize, k = 160, 120, 256, 1
    base = scenes.cascaded_ground_case(w, h, map_size=msize)
    light_dir = np.asarray(scenes.CASCADED_GROUND_LIGHT, dtype=np.float64)
    to_light = -light_dir / np.linalg.norm(light_dir)
    view, proj, _ = scenes.default_camera(w, h, eye=scenes.CASCADED_GROUND_EYE, target=scenes.CASCADED_GROUND_TARGET)
    cas = scenes.csm_cascades(view, proj, scenes.CASCADED_GROUND_LIGHT, *scenes.CASCADED_GROUND_RANGE, lam=scenes.CASCADED_GROUND_LAM)
    box = base.cascades.casters[k][k]                   # (casters[layer] = every box in order, then the sphere)
    lift, _ = _lift_in_front_of_near(scenes, cas.matrices[k], light_dir, box.vertices)
    caster = dataclasses.replace(box, camera=scenes.shadow_constants_ubo(scenes.flip_clip_y(cas.matrices[k]), lift))
    ground_only = lambda sc: dataclasses.replace(sc, draws=[sc.draws[0]], cascades=None)
    lit = oracle.render(ground_only(base), want_bgra8=False)
    unlit = oracle.render(ground_only(scenes.cascaded_ground_case(w, h, map_size=msize, intensity=0.0)), want_bgra8=False)["rgba"]
    ground = lit["prim"] != NONE
    hits = _ground_hits(scenes, w, h, scenes.CASCADED_GROUND_EYE, scenes.CASCADED_GROUND_TARGET)
    assert ground.sum() > 5000
    for clamp in (False, True):
        layers_casters = [[caster] if j == k else [] for j in range(4)]
        scene = dataclasses.replace(base, draws=[base.draws[0]], cascades=dataclasses.replace(base.cascades, casters=layers_casters, depth_clamp=clamp))
        res = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT, want_prim=True, want_depth=True)
        res.render()
        out = res.read()
        layers = res.cascade_array.read().reshape(4, msize, msize).copy()
        res.destroy()
        assert np.array_equal(out["prim"], lit["prim"])
        for j in range(4):
            if j != k or not clamp:
                assert np.all(layers[j] == 1.0), f"layer {j} clamp {clamp}"
        s = scenes.csm_factor(layers, cas.matrices, cas.split_depths, hits, (0.0, 1.0, 0.0), to_light, out["depth"], 0.005, 0.01, float(msize))
        s = np.where(ground, s, 1.0)
        if clamp:
            under = layers[k] == 0.0
            assert under.sum() > 50 and np.all(layers[k][~under] == 1.0)
            assert (s[ground] == 0.0).sum() > 50 and (s[ground] == 1.0).sum() > 3000
        else:
            assert np.all(s == 1.0)
        _assert_frame(out["color"], lit["rgba"], unlit, s, f"cascade {k} clamp {clamp}")


# 10 --------------------------------------------------------------------------------------------------------------------------------------
LEFT = [(8, 8, 0.25), (40, 8, 0.375), (8, 72, 0.25)]              # dz/dx = 2^-8
RIGHT = [(48, 8, 0.25), (80, 8, 0.375), (48, 72, 0.25)]


def test_two_draws_with_different_factors_share_a_scope(mirhi, scenes, device):
    base = _render(mirhi, device, _scene(scenes, [_draw(scenes, LEFT), _draw(scenes, RIGHT)]))
    out = _render(mirhi, device, _scene(scenes, [_draw(scenes, LEFT, depth_bias=(0.0, 0.0, 4.0)), _draw(scenes, RIGHT, depth_bias=(1000.0, 0.0, -2.0))]))
    assert np.array_equal(out["prim"], base["prim"]) and set(np.unique(base["prim"])) == {0, 1, NONE}       # prim ids run on: no segment cut
    d = out["depth"].astype(np.float64) - base["depth"].astype(np.float64)
    assert np.all(d[base["prim"] == 0] == 4.0 * Q)
    assert np.all(d[base["prim"] == 1] == -2.0 * Q + 1000.0 * 2.0 ** -25)                                   # r = 2^-25 for depths in [0.25, 0.5)
    assert np.all(d[base["prim"] == NONE] == 0.0)


def test_rerecording_with_other_factors_is_another_frame(mirhi, scenes, device, sloped_base):
    """The same command buffer re-recorded with a pipeline that differs only in its factors (the plan cache compares the draw descriptors)."""
    scene = _scene(scenes, _draw(scenes, SLOPED, depth_bias=(0.0, 0.0, 4.0)))
    res = mirhi.SceneResources(device, scene, want_prim=True, want_depth=True)
    mk = lambda *f: (mirhi.GraphicsPipelineBuilder().vertex_shader(mirhi.Program.TRIANGLE).fragment_shader(mirhi.Program.TRIANGLE).vertex_binding(24)
                     .vertex_attributes(mirhi.TRIANGLE_VERTEX_OFFSETS).color_attachment_format(res.color_format).depth_attachment_format(mirhi.Format.D32_SFLOAT)
                     .cull_mode(scenes.CULL_NONE).depth_bias(*f).build(device))
    other, third = mk(0.0, 0.0, -4.0), mk(0.0, Q, 4.0)
    first_pipe = res.draw_state[0]["pipe"]
    try:
        for pipe, want in ((first_pipe, 4.0 * Q), (other, -4.0 * Q), (third, Q), (first_pipe, 4.0 * Q), (other, -4.0 * Q)):
            res.draw_state[0]["pipe"] = pipe
            res.record()
            res.render()
            _assert_offset(sloped_base, res.read(), want, f"re-recorded {want}")
    finally:
        res.draw_state[0]["pipe"] = first_pipe
        res.destroy(); other.destroy(); third.destroy()


def test_frames_in_flight_with_different_factors(mirhi, scenes, device, sloped_base):
    """two frames in flight on two lanes, three times over, then both command buffers in one submit (the batched form)"""
    factors = [(0.0, 0.0, 4.0), (0.0, 0.0, -4.0)]
    device.set_queue_lanes(2)
    try:
        frames = [mirhi.SceneResources(device, _scene(scenes, _draw(scenes, SLOPED, depth_bias=f)), want_prim=True, want_depth=True) for f in factors]
        for lane, f in enumerate(frames):
            f.cmd.set_queue_lane(lane)
        fences = [mirhi.Fence(device) for _ in frames]
        for step in range(3):
            for f, fe in zip(frames, fences):
                f.render(fe)
            for f, fe, fac in zip(frames, fences, factors):
                fe.wait(); fe.reset()
                _assert_offset(sloped_base, f.read(), fac[2] * Q, f"in flight, frame {step}, slope {fac[2]}")
        # one submit of both command buffers: scopes of equal shape whose draw descriptors differ keep their own
        for f in frames:
            f.cmd.set_queue_lane(0)
        device.submit([f.cmd for f in frames], fences[0])
        fences[0].wait(); fences[0].reset()
        for f, fac in zip(frames, factors):
            _assert_offset(sloped_base, f.read(), fac[2] * Q, f"one submit, slope {fac[2]}")
        for f, fe in zip(frames, fences):
            f.destroy(); fe.destroy()
    finally:
        device.wait_idle()
        device.set_queue_lanes(1)


def test_frame_loop_keeps_the_workspace_idle(mirhi, scenes, device, monkeypatch):
    """MIRHI_VERIFY_IDLE=1: every re-recording checks on the host that the frame before left the workspace re-armed.  Two frames in flight, each
    RE-RECORDED every frame (three frames) with the other pipeline for its first draw -- behind biased, clamped and clipped draws (bins, the big list,
    two segments)."""
    monkeypatch.setenv("MIRHI_VERIFY_IDLE", "1")
    factors = [(0.0, 0.0, 4.0), (1000.0, -Q, -4.0)]
    low = [(x, y + 80, z) for x, y, z in SLOPED]                  # below the other two draws: its depth is the frame's there
    mk_scene = lambda f: _scene(scenes, [_draw(scenes, low, depth_bias=f), _draw(scenes, GUARD, depth_bias=(3.0, 0.0, -4.0)),
                                         _draw(scenes, RAMP, depth_compare=scenes.CMP_LESS_OR_EQUAL, depth_clamp=True)], 160, 160)
    singles = [_render(mirhi, device, mk_scene(f)) for f in factors]
    assert not np.array_equal(singles[0]["depth"], singles[1]["depth"]) and set(np.unique(singles[0]["prim"])) >= {0, 1, 2}
    frames = [mirhi.SceneResources(device, mk_scene(factors[j]), want_prim=True, want_depth=True) for j in range(2)]
    pipes = [f.draw_state[0]["pipe"] for f in frames]          # (each frame owns one of the two; both outlive the loop)
    fences = [mirhi.Fence(device) for _ in frames]
    try:
        for step in range(3):
            for j, (f, fe) in enumerate(zip(frames, fences)):
                f.draw_state[0]["pipe"] = pipes[(step + j) % 2]
                f.record()
                f.render(fe)
            for j, (f, fe) in enumerate(zip(frames, fences)):
                fe.wait(); fe.reset()
                out = f.read()
                for key in ("color", "prim", "depth"):
                    assert np.array_equal(out[key].view(np.uint32), singles[(step + j) % 2][key].view(np.uint32)), (step, j, key)
    finally:
        device.wait_idle()
        for j, (f, fe) in enumerate(zip(frames, fences)):
            f.draw_state[0]["pipe"] = pipes[j]
            f.destroy(); fe.destroy()


@pytest.mark.parametrize("world, layout", [(2, "bands"), (2, "interleaved"), (4, "bands"), (4, "interleaved")])
def test_tile_split_assembles_the_unsplit_frame(mirhi, scenes, device, world, layout):
    scene = _scene(scenes, [_draw(scenes, BIG, depth_bias=(0.0, 0.0, 4.0)), _draw(scenes, RAMP, depth_compare=scenes.CMP_LESS_OR_EQUAL, depth_clamp=True),
                            _draw(scenes, GUARD, depth_bias=(3.0, 0.0, -4.0))], 160, 160)
    whole = _render(mirhi, device, scene)
    assert set(np.unique(whole["prim"])) >= {0, 1, 2}
    assembled = {k: np.zeros_like(v) for k, v in whole.items()}
    try:
        for rank in range(world):
            device.set_tile_split(rank, world, layout)
            part = _render(mirhi, device, scene)
            first, step, rows = device.split_rows(scene.height)
            for k in range(rows):
                r0 = (first + k * step) * 32
                for key in assembled:
                    assembled[key][r0:r0 + 32] = part[key][r0:r0 + 32]
    finally:
        device.set_tile_split(0, 1, "interleaved")
    for key in assembled:
        assert np.array_equal(assembled[key].view(np.uint32), whole[key].view(np.uint32)), key


# 11 --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(mirhi, scenes, device, sloped_base):
    M, R = mirhi, mirhi.RhiError
    tri = lambda: (M.GraphicsPipelineBuilder().vertex_shader(M.Program.TRIANGLE).fragment_shader(M.Program.TRIANGLE).vertex_binding(24)
                   .vertex_attributes(M.TRIANGLE_VERTEX_OFFSETS).color_attachment_format(M.Format.R32G32B32A32_SFLOAT).depth_attachment_format(M.Format.D32_SFLOAT))
    sky = lambda: (M.GraphicsPipelineBuilder().vertex_shader(M.Program.SKYBOX).fragment_shader(M.Program.SKYBOX).vertex_binding(0).vertex_attributes(())
                   .color_attachment_format(M.Format.R32G32B32A32_SFLOAT).depth_attachment_format(M.Format.D32_SFLOAT))

    def refused(text, build):
        with pytest.raises(R) as e:
            build().destroy()
        assert e.value.code == M.ERR_PIPELINE and "unsupported:" in str(e.value) and text in str(e.value), str(e.value)

    for bad in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, float("-inf"))):
        refused("finite", lambda: tri().depth_bias(*bad).build(device))
    refused("SKYBOX", lambda: sky().depth_bias(1.0, 0.0, 1.0).build(device))
    refused("SKYBOX", lambda: sky().depth_clamp_enable(True).build(device))

    def with_discard(b):
        b.desc.rasterizer_discard_enable = 1
        return b
    refused("rasterizer_discard_enable", lambda: with_discard(tri().depth_bias(1.0, 0.0, 1.0)).build(device))
    refused("rasterizer_discard_enable", lambda: with_discard(tri().depth_clamp_enable(True)).build(device))
    # a NULL bias through the C entry point
    import ctypes as C
    b, h = tri(), C.c_void_p()
    rc = M.lib().mirhi_pipeline_create_with_depth_bias(device.handle, C.byref(b.desc), None, C.byref(h))
    assert rc == M.ERR_PIPELINE and not h.value
    msg = M.lib().mirhi_last_error_message().decode()
    assert "unsupported:" in msg and "NULL depth bias" in msg, msg
    # a clamped draw under a viewport whose depth range is not [0, 1]
    pipe = tri().depth_clamp_enable(True).build(device)
    img, depth = M.Image(device, 64, 64, M.Format.R32G32B32A32_SFLOAT), M.Image(device, 64, 64, M.Format.D32_SFLOAT)
    vb = M.Buffer.new_with_data(device, M.BufferUsage.Vertex, scenes._tri_verts(_clip(FLAT)))
    cmd = M.CommandBuffer(device)
    try:
        cmd.begin()
        cmd.begin_rendering(img, depth=depth)
        cmd.set_scissor(0, 0, 64, 64)
        cmd.bind_pipeline(pipe)
        cmd.bind_vertex_buffers(0, [vb], [0])
        for rng in ((0.0, 0.5), (0.25, 1.0), (1.0, 0.0)):
            cmd.set_viewport(0.0, 0.0, 64.0, 64.0, *rng)
            with pytest.raises(R) as e:
                cmd.draw(3, 1, 0, 0)
            assert e.value.code == M.ERR_INVALID_HANDLE and "unsupported: depth clamp with a viewport depth range other than [0, 1]" in str(e.value)
        cmd.set_viewport(0.0, 0.0, 64.0, 64.0, 0.0, 1.0)
        cmd.draw(3, 1, 0, 0)
        cmd.end_rendering(); cmd.end()
    finally:
        device.wait_idle()
        cmd.destroy(); vb.destroy(); img.destroy(); depth.destroy(); pipe.destroy()
    # depth_bias_enable = 1 through the old entry point: factors (0, 0, 0), the unbiased frame bit for bit
    scene = _scene(scenes, _draw(scenes, SLOPED))
    res = mirhi.SceneResources(device, scene, want_prim=True, want_depth=True)
    b = tri().cull_mode(scenes.CULL_NONE)
    b.desc.depth_bias_enable = 1
    zero = b.build(device)                                        # (no factors: mirhi_pipeline_create)
    explicit = tri().cull_mode(scenes.CULL_NONE).depth_bias(0.0, 0.0, 0.0).build(device)
    keep = res.draw_state[0]["pipe"]
    try:
        for pipe in (zero, explicit):
            res.draw_state[0]["pipe"] = pipe
            res.record(); res.render()
            out = res.read()
            for k in ("color", "prim", "depth"):
                assert np.array_equal(out[k].view(np.uint32), sloped_base[k].view(np.uint32)), k
    finally:
        res.draw_state[0]["pipe"] = keep
        res.destroy(); zero.destroy(); explicit.destroy()
