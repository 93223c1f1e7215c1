"""Seamless cube filtering without a GPU (include/mirhi.h "The sampler"): the float64 model of renderer-rs_amd/ibl.py against closed
forms, the conditions the GPU cases of tests/test_gpu_seamless.py rest on (asserted on the model alone), planted errors the GPU comparison has to
notice, the device's edge table against the model's re-projection, and the names through every binding."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import seamless_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=np.float64)      # the centres of faces 0 .. 5


@pytest.fixture(scope="module")
def ibl(mirhi):
    return mirhi.ibl


def _six_colours():
    return np.random.default_rng(3).random((6, 1, 1, 3))


# ---- the model against closed forms ---------------------------------------------------------------------------------------------------------
def test_one_texel_faces_centres_edges_corners(ibl):
    cols = _six_colours()
    c = cols[:, 0, 0]
    assert np.array_equal(ibl.sample_cube([cols], AXES, seamless=True), c)                        # a face centre: that colour exactly
    for a, b in itertools.combinations(range(6), 2):
        if a // 2 == b // 2:
            continue                                                                                # (opposite faces share no edge)
        got = ibl.sample_cube([cols], (AXES[a] + AXES[b])[None], seamless=True)[0]
        assert np.allclose(got, (c[a] + c[b]) / 2.0, rtol=0, atol=1e-15), (a, b)                   # the midpoint of an edge: the mean of two
    for a, b, e in itertools.product((0, 1), (2, 3), (4, 5)):
        got = ibl.sample_cube([cols], (AXES[a] + AXES[b] + AXES[e])[None], seamless=True)[0]
        assert np.allclose(got, (c[a] + c[b] + c[e]) / 3.0, rtol=0, atol=1e-15), (a, b, e)        # a cube corner: the mean of three


@pytest.mark.parametrize("n", [1, 2, 4, 8, 64])
def test_constant_cube_and_in_face_equality(ibl, n):
    rng = np.random.default_rng(n)
    d = ibl._normalize(rng.standard_normal((4000, 3)))
    const = np.broadcast_to(np.array([0.25, 0.5, 0.75]), (6, n, n, 3))
    assert np.allclose(ibl.sample_cube([const], d, seamless=True), const[0, 0, 0], rtol=0, atol=1e-15)
    cube = rng.random((6, n, n, 3))
    edge, corner = sc.tap_classes(n, d)
    inside = ~(edge | corner)
    assert n == 1 or inside.sum() > 100
    assert not inside.any() or n > 1
    for t in (np.float64, np.float32):           # bit for bit wherever the four taps are in-face, in both precisions
        assert np.array_equal(ibl.sample_cube([cube], d[inside], dtype=t, seamless=True), ibl.sample_cube([cube], d[inside], dtype=t))
    # the defaults are today's arithmetic
    assert np.array_equal(ibl.sample_cube([cube], d), ibl.sample_cube([cube], d, seamless=False))


def _edge_pairs(count=40):
    """Direction pairs 1e-9 apart straddling each of the 12 edges: [12, count, 2, 3]."""
    rng = np.random.default_rng(5)
    out = []
    for a, b in itertools.combinations(range(6), 2):
        if a // 2 == b // 2:
            continue
        third = np.cross(AXES[a], AXES[b])
        along = rng.uniform(-0.98, 0.98, count)[:, None] * third[None, :]
        out.append(np.stack([AXES[a] * (1.0 + 5e-10) + AXES[b] + along, AXES[a] + AXES[b] * (1.0 + 5e-10) + along], axis=1))
    return np.array(out)


def _corner_pairs():
    """Pairs 1e-9 apart around each of the 8 corners, one pair per pair of the three faces that meet there: [8, 3, 2, 3]."""
    out = []
    for a, b, e in itertools.product((0, 1), (2, 3), (4, 5)):
        corner = AXES[a] + AXES[b] + AXES[e]
        out.append([np.stack([corner + 1e-9 * AXES[p], corner + 1e-9 * AXES[q]]) for p, q in ((a, b), (b, e), (a, e))])
    return np.array(out)


@pytest.mark.parametrize("n", [1, 2, 8])
def test_continuity_across_edges_and_around_corners(ibl, n):
    cube = np.random.default_rng(20 + n).random((6, n, n, 3))
    edges, corners = _edge_pairs(), _corner_pairs()
    assert edges.shape[0] == 12 and corners.shape[0] == 8
    for pairs in (edges.reshape(-1, 2, 3), corners.reshape(-1, 2, 3)):
        face_a, face_b = ibl.select_face(pairs[:, 0])[0], ibl.select_face(pairs[:, 1])[0]
        assert np.all(face_a != face_b)                                       # the pairs do straddle
        jump = np.abs(ibl.sample_cube([cube], pairs[:, 0], seamless=True) - ibl.sample_cube([cube], pairs[:, 1], seamless=True)).max()
        clamped = np.abs(ibl.sample_cube([cube], pairs[:, 0]) - ibl.sample_cube([cube], pairs[:, 1])).max()
        assert jump < 1e-6, (n, jump)
        assert clamped > 0.1, (n, clamped)                                    # the inputs can tell


@pytest.mark.parametrize("n", [1, 2, 4, 16])
def test_edge_neighbour_relation(ibl, n):
    """From the projection definition alone: the neighbour lies in another face's border, at the same position along the edge, and the relation is
    symmetric -- stepping back out of the neighbour across the same edge returns the texel one came from -- over all 24 (face, side) pairs."""
    seen = set()
    for face in range(6):
        for side, (i, j) in enumerate(((-1, None), (n, None), (None, -1), (None, n))):
            for p in range(n):
                ti, tj = (i, p) if i is not None else (p, j)
                f2, i2, j2 = (int(v) for v in ibl.edge_neighbour(n, face, ti, tj))
                assert f2 != face and f2 // 2 != face // 2                    # an adjacent face, not the opposite one
                on_border = [i2 == 0, i2 == n - 1, j2 == 0, j2 == n - 1]
                assert any(on_border)
                # the same position along the shared edge: the two texel centres, each pushed out to the shared edge, coincide
                here = ibl.cube_direction(face, np.array([(min(max(ti, -0.5), n - 0.5) + 0.5) / n, (min(max(tj, -0.5), n - 0.5) + 0.5) / n]))
                back = None
                for s2, (bi, bj) in enumerate(((-1, j2), (n, j2), (i2, -1), (i2, n))):
                    if not on_border[s2]:
                        continue
                    g = tuple(int(v) for v in ibl.edge_neighbour(n, f2, bi, bj))
                    if g[0] == face:
                        back = g
                        there = ibl.cube_direction(f2, np.array([(min(max(bi, -0.5), n - 0.5) + 0.5) / n, (min(max(bj, -0.5), n - 0.5) + 0.5) / n]))
                assert back == (face, min(max(ti, 0), n - 1), min(max(tj, 0), n - 1)), (face, side, p, back)
                assert np.allclose(here, there, rtol=0, atol=1e-12), (face, side, p)
                seen.add((face, side))
    assert len(seen) == 24


def test_device_edge_table_agrees_with_the_projection(mirhi, ibl):
    """The kernels use a table of neighbours (mirhi_ibl_sample.hip.h), the model re-projects; mirhi_debug_cube_edge_tap runs the table as host code."""
    lib = C.CDLL(mirhi.LIB_PATH)
    fn = lib.mirhi_debug_cube_edge_tap
    fn.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(C.c_uint32)]
    fn.restype = None
    out = (C.c_uint32 * 2)()
    for n in (1, 2, 4, 16):
        for face in range(6):
            for i in range(-1, n + 1):
                for j in range(-1, n + 1):
                    fn(n, face, i, j, out)
                    ox, oy = i < 0 or i > n - 1, j < 0 or j > n - 1
                    assert out[1] == (1 if ox and oy else 0)
                    assert out[0] < 6 * n * n
                    if ox and oy:
                        continue
                    f2, i2, j2 = ((face, i, j) if not (ox or oy) else tuple(int(v) for v in ibl.edge_neighbour(n, face, i, j)))
                    assert out[0] == (f2 * n + j2) * n + i2, (n, face, i, j)
    # whatever the indices hold, the offset stays inside the level
    for i, j in ((-2**31, 5), (2**31 - 1, -2**31), (7, 2**31 - 1)):
        fn(4, 3, i, j, out)
        assert out[0] < 6 * 16


def test_multi_level_lookup(ibl):
    levels = [np.random.default_rng(40 + l).random((6, 4 >> l, 4 >> l, 3)) for l in range(3)]      # 4^2, 2^2, 1^2
    d = ibl._normalize(np.random.default_rng(41).standard_normal((500, 3)))
    each = [ibl.sample_cube([l], d, seamless=True) for l in levels]
    assert np.allclose(ibl.sample_cube(levels, d, 0.25, seamless=True), 0.75 * each[0] + 0.25 * each[1], rtol=0, atol=1e-15)
    assert np.allclose(ibl.sample_cube(levels, d, 1.5, seamless=True), 0.5 * each[1] + 0.5 * each[2], rtol=0, atol=1e-15)
    for lod in (2.0, 9.0):                                                                        # the last, 1 x 1 level; the clamp
        assert np.allclose(ibl.sample_cube(levels, d, lod, seamless=True), each[2], rtol=0, atol=1e-15)
    assert np.array_equal(ibl.sample_cube(levels, d, 0.0, seamless=True), each[0])
    # the last level of a seamless chain is not one constant per face
    assert np.abs(each[2] - levels[2][ibl.select_face(d)[0], 0, 0]).max() > 0.05


def test_keywords_default_to_todays_arithmetic(ibl):
    env = sc.environment()
    small = [env[2], env[3], env[4]]                 # 4^2, 2^2, 1^2: quick
    assert np.array_equal(ibl.irradiance(small, 2), ibl.irradiance(small, 2, seamless=False))
    assert np.array_equal(ibl.prefilter(small, 2, 2, 8)[1], ibl.prefilter(small, 2, 2, 8, seamless=False)[1])
    assert np.abs(ibl.prefilter(small, 2, 2, 8, seamless=True)[1] - ibl.prefilter(small, 2, 2, 8)[1]).max() > 1e-3
    m = sc.sky_matrix("corner")
    assert np.array_equal(ibl.skybox(small, m, sc.VIEWPORT, 8, 8), ibl.skybox(small, m, sc.VIEWPORT, 8, 8, seamless=False))


# ---- the conditions of the GPU cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", sorted(sc.POSES))
def test_sky_frames_meet_their_conditions(ibl, pose):
    d = sc.sky_directions(pose).reshape(-1, 3)
    for n in (4, 16):
        edge, corner = sc.tap_classes(n, d)
        assert edge.sum() >= 200 and corner.sum() >= 8, (pose, n, int(edge.sum()), int(corner.sum()))
    edge, corner = sc.tap_classes(1, d)
    assert np.all(edge | corner)                     # cube size 1: every pixel qualifies
    for n in sc.SKY_SIZES:
        levels, m64, m32 = sc.sky_case(pose, n)
        assert 0.0 <= float(np.min(levels[0])) and float(np.max(levels[0])) <= 1.0
        assert sc.err(m32, m64) < 1e-4               # (the float32 run's own error is small: the bound stays below 1e-3, the planted errors are above 1e-2)


def test_lit_case_reaches_the_small_levels(mirhi):
    import ibl_shading_cases
    for r, want in ((1.0, {4}), (0.5, {3, 4}), (0.1, {0, 1})):
        scene = sc.facets_scene(r)
        prim = ibl_shading_cases.software_prim(scene)
        py, px, facet = ibl_shading_cases.facet_pixels(scene, prim)
        assert set(facet.tolist()) == set(range(12))
        lod = sc.prefiltered_lods(scene, facet)
        # (the irradiance lookups along the quads' normals cross edges and corners too: seamless_cases.FACET_NORMALS)
        edge, corner = sc.tap_classes(sc.IRR_SIZE, np.array([f["normal"] for f in scene.facets], dtype=np.float64))
        assert (edge & ~corner).sum() >= 4 and corner.sum() >= 2 and (~edge & ~corner).sum() >= 2, (edge, corner)
        used = set(np.floor(lod).astype(int).tolist()) | set(np.minimum(np.floor(lod).astype(int) + (lod > np.floor(lod)), sc.PRE_LEVELS - 1).tolist())
        assert used == want, (r, used)
    assert sc.PRE_SIZE >> 4 == 1 and sc.PRE_SIZE >> 3 == 2      # roughness 1 reads the 1 x 1 level alone, roughness 0.5 the 2^2 and the 1 x 1 level


# ---- planted errors ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant", sc.PLANTS)
@pytest.mark.parametrize("pose, n", [("corner", 4), ("edge", 16), ("corner", 1)])
def test_the_sky_comparison_notices_a_planted_error(plant, pose, n):
    levels, m64, m32 = sc.sky_case(pose, n)
    limit = sc.bound(sc.err(m32, m64))
    assert 1e-4 <= limit < 1e-3
    wrong = sc.planted_level(levels[0], sc.sky_directions(pose), plant)
    if plant == "mirrored" and n == 1:
        assert np.array_equal(wrong, m64)            # (one texel per face: there is no position along an edge to mirror)
        return
    assert sc.err(wrong, m64) > 10 * limit, (plant, pose, n, sc.err(wrong, m64), limit)
    # and the unplanted helper is the model
    assert np.allclose(sc.planted_level(levels[0], sc.sky_directions(pose), "none"), m64, rtol=0, atol=1e-15)


def test_the_comparison_notices_one_seamless_level_of_two(ibl):
    """The sixth planted error: a trilinear lookup (the prefiltered cube at roughness 0.5: lod 3.5, the 2^2 and the 1 x 1 level) whose second level is clamped."""
    pre = [l[..., :3] for l in sc.ibl_set().prefiltered]
    d = sc.sky_directions("corner")
    m64 = ibl.sample_cube(pre, d, 3.5, np.float64, seamless=True)
    m32 = ibl.sample_cube(pre, d, 3.5, np.float32, seamless=True)
    limit = sc.bound(sc.err(m32, m64))
    assert sc.err(sc.one_level_seamless(pre, d, 3.5), m64) > 10 * limit
    # ... and in the lit frame itself, through ibl.ambient
    import ibl_shading_cases
    scene = sc.facets_scene(0.5)
    py, px, facet = ibl_shading_cases.facet_pixels(scene, ibl_shading_cases.software_prim(scene))
    images = ibl_shading_cases.scene_images(scene)
    both, _ = sc.expected_ambient(scene, images, py, px, facet, np.float64, True, True)
    b32, _ = sc.expected_ambient(scene, images, py, px, facet, np.float32, True, True)
    for flags in ((False, False), (True, False), (False, True)):
        other, _ = sc.expected_ambient(scene, images, py, px, facet, np.float64, *flags)
        assert sc.err(other, both) > 10 * sc.bound(sc.err(b32, both)), flags


# ---- bindings -----------------------------------------------------------------------------------------------------------------------------------
def test_names_through_every_binding(mirhi):
    names = ("mirhi_image_set_cube_seamless", "mirhi_image_cube_seamless")
    header = open(os.path.join(ROOT, "include", "mirhi.h")).read()
    lib = C.CDLL(mirhi.LIB_PATH)
    rust_sys = open(os.path.join(ROOT, "bindings", "rust", "mirhi-sys", "src", "lib.rs")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", "image.rs")).read()
    hpp = open(os.path.join(ROOT, "renderer-rs_amd", "host", "mirhi.hpp")).read()
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", header) and hasattr(lib, name) and name in mirhi._SIGNATURES
        assert f"pub fn {name}(" in rust_sys and f"mirhi_sys::{name}(" in rust and name + "(h_" in hpp
    assert "pub fn set_cube_seamless(" in rust and "pub fn cube_seamless(" in rust
    assert hasattr(mirhi.Image, "set_cube_seamless") and isinstance(mirhi.Image.cube_seamless, property)
    import inspect
    assert inspect.signature(mirhi.Image.create_cube).parameters["seamless"].default is False
    assert mirhi.lib().mirhi_abi_version() == 5 == mirhi.ABI_VERSION
    assert "not seamless across faces unless the cube's seamless state is on" in header
    # NULL: an error, not a crash; the getter answers 0
    assert mirhi.lib().mirhi_image_set_cube_seamless(None, 1) == mirhi.ERR_INVALID_HANDLE
    assert mirhi.lib().mirhi_image_cube_seamless(None) == 0


def test_refusal_texts_are_in_the_library(mirhi):
    """The refusals need a device to be provoked (tests/test_gpu_seamless.py); their wording is checked here against the built library."""
    blob = open(mirhi.LIB_PATH, "rb").read()
    for text in (b"not a cube image", b"cube seamless state %u is neither 0 nor 1", b"two different IBL sets"):
        assert text in blob, text


def _choice(mirhi, programs, ibl_seamless, sky_seamless, **kw):
    lib = C.CDLL(mirhi.LIB_PATH)
    vals = dict(allow_wide=1, pred=0, zflip=0, zmask=0xFFFFFFFF, tp=64, teams=1, wide=0, alpha=0, xcd=1, ordered=0)
    vals.update(kw)
    arr = (C.c_uint32 * 12)(programs, vals["allow_wide"], vals["pred"], vals["zflip"], vals["zmask"], vals["tp"], vals["teams"], vals["wide"], vals["alpha"],
                            vals["xcd"], vals["ordered"], 0)
    name, gb = C.create_string_buffer(128), (C.c_uint32 * 4)()
    if ibl_seamless is None:
        assert lib.mirhi_debug_raster_choice(arr, name, 128, gb) == 0
    else:
        assert lib.mirhi_debug_raster_choice_seamless(arr, C.c_uint32(ibl_seamless), C.c_uint32(sky_seamless), name, 128, gb) == 0
    return name.value.decode(), tuple(gb)


def test_selector_picks_the_new_variants_only_under_a_latched_state(mirhi):
    PBR, SHADOWED, CASCADED, IBL, SKY, BLEND = 4, 8, 16, 32, 64, 256
    for shadow, s in ((0, 0), (SHADOWED, 1), (SHADOWED | CASCADED, 2), (SHADOWED | CASCADED | BLEND, 3)):
        for tp in (0, 64):
            for zflip, zmask, k in ((0, 0xFFFFFFFF, 0), (0xFFFFFFFF, 0xFFFFFFFF, 1)):
                progs = PBR | IBL | shadow
                old = _choice(mirhi, progs, None, 0, tp=tp, zflip=zflip, zmask=zmask)
                assert old == _choice(mirhi, progs, 0, 0, tp=tp, zflip=zflip, zmask=zmask) == _choice(mirhi, progs, 0, 1, tp=tp, zflip=zflip, zmask=zmask)
                assert old[0] == f"raster_kernel_ibl<{k}, {1 if tp else 0}, {s}>"
                for bits in (1, 2, 3):
                    new = _choice(mirhi, progs, bits, 0, tp=tp, zflip=zflip, zmask=zmask)
                    assert new == (f"raster_kernel_ibl_seamless<{k}, {1 if tp else 0}, {s}>", old[1])
    assert _choice(mirhi, SKY, None, 0) == _choice(mirhi, SKY, 0, 0) == _choice(mirhi, SKY, 3, 0)
    assert _choice(mirhi, SKY, 0, 0)[0] == "sky_kernel"
    assert _choice(mirhi, SKY, 0, 1) == ("sky_kernel_seamless", _choice(mirhi, SKY, 0, 0)[1])
    # every other program set answers what it answered, whatever the two words hold
    for progs in (0, 1, 2, 3, 4, PBR | SHADOWED, PBR | SHADOWED | CASCADED):
        assert _choice(mirhi, progs, None, 0) == _choice(mirhi, progs, 3, 1), progs
