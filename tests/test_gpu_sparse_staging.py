"""The split bin pass of the sparse pixel-parallel raster variants (raster_bins_split): the four waves of a tile build each staged record
together -- one edge each, and the pixel box -- at the record's own index, and AND their four block masks behind the pass's barrier.
Each case is one small frame of PROGRAM_TRIANGLE draws on a 500 x 250 target (16 x 8 tiles, the last column and row partial) against the
oracle, as test_gpu_fuzz.py checks a frame: winning primitive and depth bits exact, colour to its tolerance.  The shapes are the smallest at
which the split can go wrong: record counts around the 64-lane group, around the pass of RASTER_CHUNK = 192 records and beyond the tile's fixed
page; the corner of four tiles (records whose box touches a tile that no edge mask keeps; every quadrant, four role rotations); the partial
edge tile; a scissor that cuts the triangles (boxed records: the big list's one-wave staging beside the split pass); the flipped and the
predicate depth key; an exhausted bin pool (records of pages the pool could not supply contribute nothing from the bin pass).
Every scene stays below the triangle-parallel density, and the scope-plan report says which kernel it gets."""
import ctypes as C
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 500, 250
TILES = 16 * 8
INTERIOR = (5 * 32 + 16, 3 * 32 + 16)      # centre of tile (5, 3)
CORNER = (6 * 32, 4 * 32)                  # shared by tiles (5, 3), (6, 3), (5, 4), (6, 4)
EDGE_TILE = (15 * 32 + 12, 7 * 32 + 14)    # in the last tile: 20 x 26 pixels of it lie inside the target


def _triangles(scenes, n, centre, spread, seed, **state):
    """n random overlapping small triangles: centres within `spread` pixels of `centre`, radius 2 to 7 pixels, random depth and colour."""
    rng = np.random.default_rng(seed)
    c = np.array(centre, dtype=np.float64) + rng.uniform(-spread, spread, (n, 1, 2))
    ang = rng.uniform(0, 2 * np.pi, (n, 3, 1))
    p = c + rng.uniform(2.0, 7.0, (n, 1, 1)) * np.concatenate([np.cos(ang), np.sin(ang)], axis=2)
    ndc = p / np.array([W, H]) * 2.0 - 1.0
    z = np.repeat(rng.uniform(0.05, 0.95, (n, 1, 1)), 3, axis=1) if n % 2 else rng.uniform(0.05, 0.95, (n, 3, 1))
    verts = np.concatenate([ndc, z, rng.uniform(0, 1, (n, 3, 3))], axis=2).astype(np.float32).reshape(n * 3, 6)
    return scenes.DrawSpec(vertices=verts, stride=24, count=3 * n, program=scenes.PROGRAM_TRIANGLE, cull_mode=scenes.CULL_NONE, **state)


def _kernel(mirhi, draw, clear_depth, tris):
    """The raster kernel build_plan picks for a one-draw TRIANGLE scope of this target (mirhi_debug_scope_plan: tests/test_scope_plan_cpu.py)."""
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_scope_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32]
    words = [1, int(draw.depth_test), int(draw.depth_compare), int(draw.depth_write), 0, 0, struct.unpack("<I", struct.pack("<f", clear_depth))[0],
             0, TILES, tris, 0, 0, 1, 1, 1, 0, 0, 0]
    inp, out, name = (C.c_uint32 * 27)(*(words + [0] * (27 - len(words)))), (C.c_uint32 * 32)(), C.create_string_buffer(96)
    assert fn(inp, out, name, len(name)) == 0
    return name.value.decode()


def _check(mirhi, oracle, device, scenes, draw, kernel="raster_kernel<1, 0, 0, 1, false>", clear_depth=1.0, whole_depth=False):
    n = draw.count // 3
    assert _kernel(mirhi, draw, clear_depth, n) == kernel          # pixel-parallel, one team of four waves: the split bin pass
    scene = scenes.Scene(f"sparse-staging-{n}", W, H, [draw], clear_color=(0.2, 0.3, 0.1, 1.0), clear_depth=clear_depth)
    res = mirhi.SceneResources(device, scene, want_prim=True, want_depth=True)
    res.render()
    out = res.read()
    res.destroy()
    ref = oracle.render(scene, want_bgra8=False)
    diff = out["prim"] != ref["prim"]
    assert not diff.any(), f"{int(diff.sum())} pixels differ in winning primitive (first {np.argwhere(diff)[0]})"
    cov = ref["prim"] != 0xFFFFFFFF
    assert cov.sum() > 0
    if whole_depth:
        cov = np.ones_like(cov)
    assert np.array_equal(out["depth"].view(np.uint32)[cov], ref["depth"].view(np.uint32)[cov]), "depth bits differ"
    a, b = out["color"], ref["rgba"]
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert err.max() < 1e-4, f"max |dRGBA| {err.max()}"
    return ref


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 191, 192, 193, 257])
def test_record_counts_in_one_interior_tile(mirhi, oracle, device, scenes, n):
    ref = _check(mirhi, oracle, device, scenes, _triangles(scenes, n, INTERIOR, 8.0, 100 + n))
    ys, xs = np.nonzero(ref["prim"] != 0xFFFFFFFF)
    assert xs.min() >= 160 and xs.max() < 192 and ys.min() >= 96 and ys.max() < 128      # all in tile (5, 3)


@pytest.mark.parametrize("n", [3, 65, 193])
def test_tile_corner(mirhi, oracle, device, scenes, n):
    ref = _check(mirhi, oracle, device, scenes, _triangles(scenes, n, CORNER, 5.0, 200 + n))
    if n > 3:       # all four tiles hold covered pixels
        cov = ref["prim"] != 0xFFFFFFFF
        assert cov[:128, :192].any() and cov[:128, 192:].any() and cov[128:, :192].any() and cov[128:, 192:].any()


def test_partial_edge_tile(mirhi, oracle, device, scenes):
    ref = _check(mirhi, oracle, device, scenes, _triangles(scenes, 65, EDGE_TILE, 10.0, 300))
    cov = ref["prim"] != 0xFFFFFFFF
    assert cov[:, W - 1].any() and cov[H - 1, :].any()       # the triangles reach both borders of the target


def test_scissor_cuts_the_triangles(mirhi, oracle, device, scenes):
    d = _triangles(scenes, 65, CORNER, 5.0, 400)
    d.scissor = (CORNER[0] - 5, CORNER[1] - 3, 9, 11)
    ref = _check(mirhi, oracle, device, scenes, d)
    ys, xs = np.nonzero(ref["prim"] != 0xFFFFFFFF)
    assert xs.min() == CORNER[0] - 5 and xs.max() == CORNER[0] + 3 and ys.min() == CORNER[1] - 3 and ys.max() == CORNER[1] + 7


def test_depth_compare_greater(mirhi, oracle, device, scenes):
    d = _triangles(scenes, 65, CORNER, 5.0, 500, depth_compare=scenes.CMP_GREATER)
    _check(mirhi, oracle, device, scenes, d, kernel="raster_kernel<1, 1, 0, 1, false>", clear_depth=0.0)


def test_depth_test_without_write(mirhi, oracle, device, scenes):
    d = _triangles(scenes, 65, CORNER, 5.0, 600, depth_compare=scenes.CMP_LESS_OR_EQUAL, depth_write=False)
    _check(mirhi, oracle, device, scenes, d, kernel="raster_kernel<1, 2, 0, 1, false>", clear_depth=0.5, whole_depth=True)


def test_exhausted_pool(mirhi, oracle, device, scenes, monkeypatch):
    """No dynamic pages at all (MIRHI_POOL_PAGES, as test_bin_pool_exhaustion_spills_and_grows forces it) and one fixed page per tile: records
    64 ... of the interior tile have no page (PAGE_NONE in the tile's table row) and reach the tile through the big list."""
    monkeypatch.setenv("MIRHI_POOL_PAGES", "0")
    monkeypatch.setenv("MIRHI_FIXED_PAGES", "1")
    _check(mirhi, oracle, device, scenes, _triangles(scenes, 193, INTERIOR, 8.0, 700))
    st = device.stats()
    assert st.last_status & 4 and st.last_big_list > 0
