"""The geometry kernel's routing decisions against the exact integer model of tests/binning_cases.py.

The image tests see whether a pixel comes out right, not where the geometry kernel put the triangle: a triangle binned and spilled as well, binned into a
tile it does not touch, or sent to the big list by an over-cautious `fits` all resolve to the same frame.  Two exact observables do see it: the
fragment-count pass (Profile.FRAGMENTS), which walks the bins and the big list as they were laid out -- a record stored twice is counted twice -- and
DeviceStats.last_big_list / last_bin_pages / last_status.  Every case sits on, one sub-pixel inside or one sub-pixel outside one boundary of the routing
(tests/test_binning_cpu.py holds each case to the condition it was built for, and the model to the oracle); here the kernel's figures must EQUAL the model's."""
import ctypes as C
import struct

import numpy as np
import pytest

import binning_cases as bc

pytestmark = pytest.mark.gpu

NO_PRIM = 0xFFFFFFFF
_BASE = [c for c in bc.unsplit_cases() if not c.model]
CASES = {c.name: c for c in _BASE}
CASES.update({p.name: p for p in (bc.with_companion(c) for c in _BASE if bc.pairable(c))})
SPLITS = [(kind, world, layout) for kind in bc.SPLIT_KINDS for layout in ("bands", "interleaved") for world in (2, 4)]


def render_counted(mirhi, dev, scene):
    """One render of the scene under Profile.FRAGMENTS: the images, (shaded, covered, scopes) and the device's statistics of that scope."""
    res = mirhi.SceneResources(dev, scene, mirhi.Format.R32G32B32A32_SFLOAT, want_prim=True, want_depth=True)
    fence = mirhi.Fence(dev)
    dev.wait_idle()
    dev.reset_kernel_times()
    dev.set_profiling(mirhi.Profile.FRAGMENTS)
    res.render(fence)
    fence.wait()
    dev.set_profiling(0)
    got = res.read()
    counted, st = dev.fragment_stats(), dev.stats()
    res.destroy()
    fence.destroy()
    return got, counted, st


def oracle_fragments(c, oracle, scenes):
    """The sum of the oracle's single-triangle coverages (the clipped cases take their fragment sum from here)."""
    n = len(c.clip) // 3 if c.clipped else len(c.tris)
    return sum(int((oracle.render(bc.scene_of(c, scenes, only=k), want_bgra8=False)["prim"] != NO_PRIM).sum()) for k in range(n))


def check_frame(got, ref):
    assert np.array_equal(got["prim"], ref["prim"])
    hit = ref["prim"] != NO_PRIM
    assert np.array_equal(got["depth"].view(np.uint32)[hit], ref["depth"].view(np.uint32)[hit])


@pytest.mark.parametrize("name", list(CASES))
def test_case(name, mirhi, oracle, device, scenes, monkeypatch):
    c = CASES[name]
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    scene = bc.scene_of(c, scenes)
    ref = oracle.render(scene, want_bgra8=False)
    fig = bc.figures(c)
    want_covered = oracle_fragments(c, oracle, scenes) if c.clipped else fig["covered"]
    got, (shaded, covered, scopes), st = render_counted(mirhi, device, scene)
    print(f"{name}: covered {covered} (model {want_covered}), shaded {shaded}, big list {st.last_big_list} (model {fig['big']}), pages {st.last_bin_pages}, "
          f"status {st.last_status}, triangles per wave {bc.tris_per_wave(c)}")
    check_frame(got, ref)
    assert st.last_status == 0              # no list filled, no pool ran out: what makes the fragment equality exact
    assert st.last_big_list == fig["big"]   # a spilled triangle counts 1, a clipped one its pieces
    assert scopes == 1 and covered == want_covered
    assert shaded == int((ref["prim"] != NO_PRIM).sum())
    if c.pages is not None:
        assert st.last_bin_pages == c.pages


def _plan(mirhi, tris, tiles=64):
    """(teams, xcd_bins) mirhi_debug_scope_plan gives a one-draw MODEL scope with a LESS depth state (tests/test_scope_plan_cpu.py has the words)."""
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_scope_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32]
    words = [1, 1, 1, 1, 0, 0, struct.unpack("<I", struct.pack("<f", 1.0))[0], 0, tiles, tris, 0, 0, 1, 1, 1, 1, 0, 0]
    inp, out, name = (C.c_uint32 * 27)(*(words + [0] * (27 - len(words)))), (C.c_uint32 * 32)(), C.create_string_buffer(96)
    assert fn(inp, out, name, len(name)) == 0
    return out[16], out[18]


def test_per_xcd_lists(mirhi, oracle, device, scenes, monkeypatch):
    """The smallest scope raster_mode gives two teams and per-XCD bins: a MODEL-program draw of 4 triangles per tile.  The same frame with
    MIRHI_XCD_BINS=0 -- one list per tile -- has the same image, fragment sum and big list, and both have the model's."""
    monkeypatch.delenv("MIRHI_XCD_BINS", raising=False)
    assert _plan(mirhi, bc.XCD_TRIS) == (2, 1) and _plan(mirhi, bc.XCD_TRIS - 1) == (1, 0)
    c = bc.xcd_case()
    scene = bc.scene_of(c, scenes)
    ref = oracle.render(scene, want_bgra8=False)
    fig = bc.figures(c)
    runs = []
    for knob in (None, "0"):
        if knob is not None:
            monkeypatch.setenv("MIRHI_XCD_BINS", knob)
            assert _plan(mirhi, bc.XCD_TRIS) == (2, 0)
        got, counted, st = render_counted(mirhi, device, scene)
        print(f"xcd_bins {knob}: counted {counted} (model covered {fig['covered']}), big list {st.last_big_list} (model {fig['big']}), pages {st.last_bin_pages}")
        check_frame(got, ref)
        assert st.last_status == 0 and st.last_big_list == fig["big"]
        assert counted == (int((ref["prim"] != NO_PRIM).sum()), fig["covered"], 1)
        runs.append((got, counted, st.last_big_list))
    (a, ca, ba), (b, cb, bb) = runs
    assert (ca, ba) == (cb, bb)
    assert np.array_equal(a["prim"], b["prim"]) and np.array_equal(a["color"].view(np.uint32), b["color"].view(np.uint32))
    assert np.array_equal(a["depth"].view(np.uint32), b["depth"].view(np.uint32))


@pytest.mark.parametrize("kind, world, layout", SPLITS, ids=[f"{k}-{l}{w}" for k, w, l in SPLITS])
def test_row_split(kind, world, layout, mirhi, oracle, device, scenes):
    """One GPU as rank r of a world, rank after rank (as test_tile_row_split_rows_assemble): each rank's big list and fragment sum are the model's for
    that rank -- the statistics pass runs for a split rank's scope (scope_counted: it has tile rows), over its own rows -- and the ranks' rows assemble
    into the unsplit frame."""
    from renderer_rs_amd import multigpu
    c = bc.split_case(kind, world, layout)
    scene = bc.scene_of(c, scenes)
    ref = oracle.render(scene, want_bgra8=False)
    whole, _, _ = render_counted(mirhi, device, scene)
    check_frame(whole, ref)
    out = {k: np.zeros_like(v) for k, v in whole.items()}
    owners = np.zeros(c.height, dtype=np.int32)
    for rank in range(world):
        s = bc.split_of(rank, world, layout)
        fig = bc.figures(c, s)
        dev = mirhi.Device(0)
        try:
            dev.set_tile_split(rank, world, layout=layout)
            assert dev.split_rows(c.height) == (s.first, s.step, s.count)
            got, (_, covered, scopes), st = render_counted(mirhi, dev, scene)
        finally:
            dev.destroy()
        print(f"{c.name} rank {rank}: covered {covered} (model {fig['covered']}), big list {st.last_big_list} (model {fig['big']}), status {st.last_status}")
        assert st.last_status == 0
        assert st.last_big_list == fig["big"]
        assert scopes == 1 and covered == fig["covered"]
        mine = np.zeros(c.height, dtype=bool)
        for r0, r1 in multigpu.owned_pixel_rows(c.height, rank, world, layout):
            mine[r0:r1] = True
        for k in out:
            out[k][mine] = got[k][mine]
        owners += mine
    assert (owners == 1).all()
    for k in out:
        assert np.array_equal(out[k].view(np.uint32), whole[k].view(np.uint32)), k
