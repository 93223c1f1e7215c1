"""build_plan decides about a scope what the commit before mirhi_scope.h decided.  What kind of scope a recorded segment is (depth key, ordered,
alpha-masked, program set, own raster family), how it is rastered (triangle-parallel path, teams, per-XCD bins, wide variant, tile order) and how
its bins are sized shows in no image as long as the choice is a valid one: tests/golden/scope_plans.json holds what the text of the fixture's
"parent" -- cut out of its mirhi_api.hip and compiled as it stood by tools/make_scope_plans.py -- answers for every row of a grid of scopes, and
mirhi_debug_scope_plan says what the library under test answers.  No GPU: the export makes no HIP call."""
import ctypes as C
import itertools
import json
import os
import struct

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scope_plans.json")
N_IN, N_OUT = 27, 32
OUT_NAMES = ("clear_depth_bits pred zflip zmask idflip strict init_zk init_idk ordered masked_plain tri_prog shadowed ibl own_family programs tp_max_area teams "
             "wide_eligible xcd_bins wide xcd_swizzle bin_cap sub_cap fixed_per_tile fixed_pages pool_pages_lo pool_pages_hi big_cap grid_x grid_y grid_z block kernel").split()


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(FIXTURE))


@pytest.fixture(scope="module")
def plan(mirhi):
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_scope_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32]
    inp, out, name = (C.c_uint32 * N_IN)(), (C.c_uint32 * N_OUT)(), C.create_string_buffer(96)

    def plan(words):
        """The output words and the kernel name, as one tuple."""
        inp[:] = words
        assert fn(inp, out, name, len(name)) == 0
        return (*out, name.value.decode())
    return plan


ORDERING = (1, 3, 4, 6)       # LESS, LESS_OR_EQUAL, GREATER, GREATER_OR_EQUAL


def scopes_of(f):
    """[state index, mix index] of every scope, mixes slowest.  Every mix meets every depth state but those record_draw / pipeline creation refuse (the
    tool's docstring): "ordered key" (a shadow map, MODEL_PBR_IBL), "tested ordered key" (cascades, depth-only); the scope without draws has no key, and it alone."""
    out = []
    for mi, (_, _, needs, draws) in enumerate(f["mixes"]):
        for si, (k, t, op, w, d, b) in enumerate(f["states"]):
            if not draws or not k:
                ok = not draws and not k
            else:
                ok = needs == "" or (not d and not b and ((t and w and op in ORDERING) or (needs == "ordered key" and not t)))
            if ok:
                out.append([si, mi])
    return out


def answer(f, pair):
    """The 32 output words and the kernel name of a [scope part, plan part] pair of the fixture."""
    raster, bins = (f["raster_parts"][f["plan_parts"][pair[1]][0]], f["bins_parts"][f["plan_parts"][pair[1]][1]])
    return tuple(f["scope_parts"][pair[0]] + raster[:6] + bins + raster[6:])


def joined(lists, pieces, i):
    return [x for p in lists[i] for x in pieces[p]]


def words(state, mix, clear=1.0, tiles=20, tris=0, spread=0, wide=0, pool_scale=1, allow_wide=1):
    """The input words of mirhi_debug_scope_plan (tools/make_scope_plans.py: words)."""
    _, depth_only, _, draws = mix
    w = list(state) + [struct.unpack("<I", struct.pack("<f", clear))[0], depth_only, tiles, tris, spread, wide, pool_scale, allow_wide, len(draws)]
    for d in draws:
        w += d
    return w + [0] * (N_IN - len(w))


def set_knobs(monkeypatch, env):
    for name in [k for k in os.environ if k.startswith("MIRHI_")]:
        monkeypatch.delenv(name)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def differences(rows):
    """rows: (what, input words, wanted outcome, outcome); the first few that differ, with the differing words named."""
    wrong = [(what, w, {n: (a, b) for n, a, b in zip(OUT_NAMES, want, got) if a != b}) for what, w, want, got in rows if tuple(want) != got]
    return f"{len(wrong)} rows, first: {wrong[:3]}" if wrong else ""


def test_fixture_is_the_whole_grid(fixture):
    f = fixture
    states, mixes = f["states"], f["mixes"]
    assert sorted(states) == sorted([[1, t, op, w, d, b] for op in range(8) for t in (0, 1) for w in (0, 1) for d in (0, 1) for b in (0, 1)] + [[0] * 6])
    assert {m[0]: m[3] for m in mixes} == {
        "triangle": [[0, 0, 0]], "model": [[1, 0, 0]], "model_textured": [[1, 0, 1]], "model_full": [[2, 0, 0]], "triangle+model": [[0, 0, 0], [1, 0, 0]],
        "model+pbr": [[1, 0, 0], [3, 0, 0]], "pbr": [[3, 0, 0]], "pbr_map": [[3, 1, 0]], "pbr_cascades": [[3, 2, 0]], "ibl": [[5, 0, 0]], "ibl_map": [[5, 1, 0]],
        "ibl_cascades": [[5, 2, 0]], "ibl+pbr": [[5, 0, 0], [3, 0, 0]], "shadow_depth_only": [[4, 0, 0]], "no_draws": []}
    assert [m[0] for m in mixes if m[1]] == ["shadow_depth_only"]
    assert {m[0]: m[2] for m in mixes if m[2]} == {"pbr_map": "ordered key", "ibl": "ordered key", "ibl_map": "ordered key", "ibl+pbr": "ordered key", "no_draws": "no key",
                                                   "pbr_cascades": "tested ordered key", "ibl_cascades": "tested ordered key", "shadow_depth_only": "tested ordered key"}
    scopes = scopes_of(f)
    assert [sum(1 for _, m in scopes if m == mi) for mi in range(len(mixes))] == [128] * 7 + [20, 4, 20, 20, 4, 20, 4, 1] and len(scopes) == 989
    assert (f["tris_per_tile"], f["spread"], f["wide"], f["tiles"]) == ([0, 3, 4, 15, 16, 200], [0, 1], [0, 8, 16], 20)
    assert [env for _, env in f["knobs"]] == [
        {}, {"MIRHI_RASTER_TEAMS": "1"}, {"MIRHI_RASTER_TEAMS": "2"}, {"MIRHI_RASTER_WIDE": "0"}, {"MIRHI_RASTER_WIDE": "8"}, {"MIRHI_RASTER_WIDE": "16"},
        {"MIRHI_RASTER_TEAMS": "2", "MIRHI_RASTER_WIDE": "8"}, {"MIRHI_TP_MAX_AREA": "0"}, {"MIRHI_TP_DENSITY": "1"}, {"MIRHI_MASKED_ORDERED": "1"},
        {"MIRHI_XCD_BINS": "0"}, {"MIRHI_XCD_RUN": "2"}]
    assert set(f["main"]) == {k for k, _ in f["knobs"]}
    assert all(len(joined(f["vectors"], f["vector_pieces"], i)) == 989 for v in f["main"].values() for i in v)
    assert all(len(joined(f["patterns"], f["pattern_pieces"], i)) == 36 for i in range(len(f["patterns"])))
    assert all(len(o) == 15 for o in f["scope_parts"]) and all(len(o) == 11 for o in f["raster_parts"]) and all(len(o) == 7 for o in f["bins_parts"])
    assert f["clear"]["values"] == [0.0, 0.5, 1.0, 1.5] and len(f["clear"]["answers"]) == 129 * 4
    b = f["bins"]
    assert (b["tiles"], b["tris"], b["xcd_bins"], b["pool_scale"]) == ([1, 20, 2040], [0, 1, 100, 10000, 1000000], [0, 1], [1, 2])
    assert [env for _, env in b["knobs"]] == [{}, {"MIRHI_BIN_CAP": "100"}, {"MIRHI_BIN_CAP": "100000"}, {"MIRHI_FIXED_PAGES": "3"}, {"MIRHI_POOL_PAGES": "5"}]
    assert len(b["answers"]) == 5 * 2 * 3 * 5 * 2
    # not vacuous: every raster family and both resolves occur among the answers
    kernels = {o[-1].split("<")[0] for o in f["raster_parts"]}
    assert kernels == {"raster_kernel", "raster_kernel_wide", "raster_kernel_depth", "raster_kernel_shadow", "raster_kernel_csm", "raster_kernel_ibl", "ordered_kernel"}
    assert {o[1] for o in f["raster_parts"]} == {1, 2} and {o[4] for o in f["raster_parts"]} == {0, 8, 16} and {o[9] for o in f["scope_parts"]} == {0, 1}


@pytest.mark.parametrize("knob", range(12))
def test_class_and_raster_mode_are_the_parents(fixture, plan, monkeypatch, knob):
    f = fixture
    name, env = f["knobs"][knob]
    set_knobs(monkeypatch, env)
    inner = list(itertools.product(f["tris_per_tile"], f["spread"], f["wide"]))
    rows = []
    scope_parts, patterns = (joined(f["vectors"], f["vector_pieces"], i) for i in f["main"][name])
    for (si, mi), scope_part, pattern in zip(scopes_of(f), scope_parts, patterns):
        for (per_tile, spread, wide), plan_part in zip(inner, joined(f["patterns"], f["pattern_pieces"], pattern)):
            w = words(f["states"][si], f["mixes"][mi], tiles=f["tiles"], tris=per_tile * f["tiles"], spread=spread, wide=wide)
            rows.append((f["mixes"][mi][0], w, answer(f, (scope_part, plan_part)), plan(w)))
    assert len(rows) == 989 * 36
    assert not differences(rows)


def test_depth_key_is_the_parents_for_every_clear_depth(fixture, plan, monkeypatch):
    f = fixture
    set_knobs(monkeypatch, {})
    model, no_draws = next(m for m in f["mixes"] if m[0] == "model"), next(m for m in f["mixes"] if m[0] == "no_draws")
    rows = []
    for (state, clear), outcome in zip(itertools.product(f["states"], f["clear"]["values"]), f["clear"]["answers"]):
        w = words(state, model if state[0] else no_draws, clear=clear, tris=200 * 20)
        rows.append((clear, w, answer(f, outcome), plan(w)))
    assert len(rows) == 516 and len({r[2][0] for r in rows}) == 3          # (clear-depth bits: 0.0, 0.5, and 1.0 for both 1.0 and 1.5)
    assert not differences(rows)


def test_bin_geometry_is_the_parents(fixture, plan, monkeypatch):
    f, b = fixture, fixture["bins"]
    model = next(m for m in f["mixes"] if m[0] == "model")
    grid = itertools.product(b["knobs"], b["xcd_bins"], b["tiles"], b["tris"], b["pool_scale"])
    rows = []
    for ((_, env), xcd, tiles, tris, scale), outcome in zip(grid, b["answers"]):
        set_knobs(monkeypatch, dict(b["xcd_bins_env"][xcd], **env))
        w = words([1, 1, 1, 1, 0, 0], model, tiles=tiles, tris=tris, pool_scale=scale)
        rows.append((env, w, answer(f, outcome), plan(w)))
        assert rows[-1][2][18] == xcd
    assert len(rows) == 300
    assert not differences(rows)
