"""A submit goes out as the commit before mirhi_submit.h sent it.  Whether a submit is batched, goes out as AQL packets, what carries its fence, the memory
scopes of a scope's packets, its triangles per geometry wave, whether it may take a wide variant, is timed and counted, and what the busy-tile feedback
asks for show in no image when they are wrong -- a stale read now and then, a race between frames.  tests/golden/submit_paths.json holds what the text of the
fixture's "parent" -- cut out of its mirhi_api.hip and compiled as it stood by tools/make_submit_paths.py -- answers for every row of its grids, and
mirhi_debug_submit_path says what the library under test answers.  No GPU: the export makes no HIP or HSA call.  The input words of a row are stated
here (as tools/make_submit_paths.py states them), from the axes the fixture names; the fixture's "inputs" is the sha256 of every grid's input words."""
import ctypes as C
import hashlib
import itertools
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "submit_paths.json")
N_IN, N_OUT = 11 + 16 * 9, 8
OUT_NAMES = {"batch": "batched native_eligible native fence_carrier carrier_cmd carrier_scope".split(),
             "scope": "vertex_flags geometry_flags raster_flags tris_per_wave allow_wide timed counted parity_flips".split(), "feedback": ["wide_wanted"]}
OUT_NAMES.update(path=OUT_NAMES["batch"], flags=OUT_NAMES["scope"], tpw=OUT_NAMES["scope"], wide=OUT_NAMES["scope"], profile=OUT_NAMES["scope"])
NONE, STOP_EVENT, NATIVE_SIGNAL, EVENT_RECORD, NATIVE_DRAIN = range(5)
KINDS = ["plain", "ordered", "depth_only", "sky", "transfer"]


def cmd_words(ident, lane=0, scopes=1, ordered="none", tiles=1, variant="equal", load="none", color=None, depth=None, prim_out=None):
    """The 16 words of one command buffer: a frame of a frame loop (one PBR scope of 5 x 4 tiles with targets of its own), changed as asked.  ordered: "none", or
    the "first" or the "last" scope is an ordered one; tiles: the last scope has tile rows (a first of two always has)."""
    first_ordered = int(scopes >= 1 and (ordered == "first" or (ordered == "last" and scopes == 1)))
    return [ident, lane, scopes, int(scopes == 2 and ordered == "last"), int(scopes == 2 and tiles),
            5 if variant == "programs" else 4, 64 if variant == "kernel" else 0, 6 if variant == "grid" else 5, 4 if (scopes != 1 or tiles) else 0,
            8 if variant == "batched_form" else 0, first_ordered, int(load == "colour"), int(load == "depth"),
            1000 + ident if color is None else color, 2000 + ident if depth is None else depth, 3000 + ident if prim_out is None else prim_out]


def path_words(cmds, profiling=0, native=0, owns_stream=1, native_on_external=0, lanes=4, no_batch=0, fence_record=0, queue_opens=1, fence=1):
    return [0, profiling, native, owns_stream, native_on_external, lanes, no_batch, fence_record, queue_opens, fence, len(cmds)] + [w for c in cmds for w in c]


def batch_row(count, other_lane, variant, load, shared, scopes, profiling, no_batch):
    every = {}          # what the axis value says of every command buffer, not of the last alone
    if shared == "no_depth":
        every["depth"] = 0
    if shared == "no_prim_out":
        every["prim_out"] = 0
    if variant == "none_batched":
        every["variant"] = variant = "batched_form"
    cmds = [cmd_words(i + 1, **every) for i in range(count - 1)]
    if shared == "same" and count >= 2:
        cmds.append(list(cmds[0]))          # (the first once more: whatever the other axes say)
    else:
        last = dict(every, variant=variant, **{"colour": dict(color=1001), "depth": dict(depth=2001), "prim_out": dict(prim_out=3001)}.get(shared, {}))
        cmds.append(cmd_words(count, lane=other_lane, scopes=scopes, load=load, **last))
    return path_words(cmds, profiling=profiling, no_batch=no_batch)


def path_row(count, other_lane, batchable, scopes, ordered, tiles, profiling, native, owns_stream, native_on_external, lane0, lanes, queue_opens, fence, fence_record):
    cmds = [cmd_words(i + 1, lane=lane0, tiles=tiles) for i in range(count - 1)]
    cmds.append(cmd_words(count, lane=lane0 ^ other_lane, scopes=scopes, ordered=ordered, tiles=tiles, variant="equal" if batchable else "grid"))
    return path_words(cmds, profiling=profiling, native=native, owns_stream=owns_stream, native_on_external=native_on_external, lanes=lanes,
                      fence_record=fence_record, queue_opens=queue_opens, fence=fence)


def scope_words(system_scope=0, unseen_foreign=0, ws_foreign=0, vs_total_slots=64, kind="plain", total_slots=64, geom_tpw=0, in_flight=1, wide_set=0, profiling=0, lane=0, tile_rows=4, tiles_x=5):
    return [1, system_scope, unseen_foreign, ws_foreign, vs_total_slots, KINDS.index(kind), total_slots, geom_tpw, in_flight, wide_set, profiling, lane, tile_rows, tiles_x]


def feedback_words(busy_tiles, wide):
    return [2, busy_tiles, wide]


MAKE = {"batch": batch_row, "path": path_row, "flags": scope_words, "tpw": scope_words, "wide": scope_words, "profile": scope_words, "feedback": feedback_words}


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(FIXTURE))


@pytest.fixture(scope="module")
def ask(mirhi):
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_submit_path
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    inp, out = (C.c_uint32 * N_IN)(), (C.c_uint32 * N_OUT)()

    def ask(words, first, count):
        inp[:len(words)] = words
        assert fn(inp, out) == 0
        return tuple(out[first:first + count])
    return ask


def answers_of(g):
    """The answer of every row of a grid of the fixture, in row order."""
    return [g["answers"][a] for r in g["rows"] for a in g["pieces"][r]]


def replay(fixture, ask, grid):
    g = fixture["grids"][grid]
    names = [n for n, _ in g["axes"]]
    make = MAKE[grid]
    count = len(g["answers"][0])
    rows = []
    for values, want in zip(itertools.product(*[v for _, v in g["axes"]]), answers_of(g), strict=True):
        w = make(**dict(zip(names, values)))
        rows.append((dict(zip(names, values)), w, want, ask(w, g["first"], count)))
    # the rows mean what they meant when the parent answered them
    assert hashlib.sha256("".join(" ".join(map(str, w)) + "\n" for _, w, _, _ in rows).encode()).hexdigest() == g["inputs"]
    return rows


def differences(grid, first, rows):
    """rows: (axis values, input words, wanted outcome, outcome); the first few that differ, with the differing words named."""
    names = OUT_NAMES[grid][first:]
    wrong = [(what, w, {n: (a, b) for n, a, b in zip(names, want, got) if a != b}) for what, w, want, got in rows if tuple(want) != got]
    return f"{len(wrong)} rows, first: {wrong[:3]}" if wrong else ""


def test_fixture_is_the_whole_grid(fixture):
    f, g = fixture, fixture["grids"]
    assert f["max_batch"] == 8 and f["piece"] == 64
    counts, timing, fragments = [1, 2, 3, 8, 9], 1, 2
    assert g["batch"]["axes"] == [["count", counts], ["other_lane", [0, 1]], ["variant", ["equal", "kernel", "grid", "batched_form", "programs", "none_batched"]],
                                  ["load", ["none", "colour", "depth"]], ["shared", ["none", "colour", "depth", "prim_out", "same", "no_depth", "no_prim_out"]], ["scopes", [0, 1, 2]],
                                  ["profiling", [0, timing, fragments]], ["no_batch", [0, 1]]]
    assert g["path"]["axes"] == [["count", counts], ["other_lane", [0, 1]], ["batchable", [1, 0]], ["scopes", [0, 1, 2]], ["ordered", ["none", "last", "first"]], ["tiles", [1, 0]],
                                 ["profiling", [0, timing, fragments]], ["native", [0, 1]], ["owns_stream", [0, 1]], ["native_on_external", [0, 1]], ["lane0", [0, 1]],
                                 ["lanes", [1, 4]], ["queue_opens", [1, 0]], ["fence", [0, 1]], ["fence_record", [0, 1]]]
    assert g["flags"]["axes"] == [["system_scope", [0, 1, 2]], ["unseen_foreign", [0, 1]], ["ws_foreign", [0, 1]], ["vs_total_slots", [0, 64]], ["kind", ["plain", "sky", "transfer"]]]
    assert g["tpw"]["axes"] == [["total_slots", [0, 256 * 64, 257 * 64 - 1, 257 * 64, 512 * 64, 513 * 64 - 1, 513 * 64]], ["geom_tpw", [0, 16, 32, 64]]]
    assert g["wide"]["axes"] == [["in_flight", [1, 2, 3]], ["wide_set", [0, 1]]]
    assert g["profile"]["axes"] == [["profiling", [0, timing, fragments, timing | 1 << 8, timing | 2 << 8, timing | fragments]], ["lane", [0, 1]],
                                    ["kind", ["plain", "ordered", "depth_only", "sky", "transfer"]], ["tile_rows", [4, 0]], ["tiles_x", [5, 0]]]
    assert g["feedback"]["axes"] == [["busy_tiles", [0, 240, 241, 300, 301, 512, 513, 640, 641]], ["wide", [0, 8, 16]]]
    assert {k: len(answers_of(v)) for k, v in g.items()} == {"batch": 22680, "path": 276480, "flags": 72, "tpw": 28, "wide": 6, "profile": 240, "feedback": 27}
    assert {k: (v["first"], len(v["answers"][0])) for k, v in g.items()} == {"batch": (0, 6), "path": (0, 6), "flags": (0, 3), "tpw": (3, 1), "wide": (4, 1), "profile": (5, 3),
                                                                               "feedback": (0, 1)}
    # not vacuous: batched and not, native and not (eligible and in the end), all four carriers and no fence, a carrying scope that is not the first; both sides of every scope rule
    for grid in ("batch", "path"):
        assert {a[0] for a in g[grid]["answers"]} == {0, 1}
    path = g["path"]["answers"]
    assert {a[1] for a in path} == {0, 1} and {a[2] for a in path} == {0, 1} and {(a[1], a[2]) for a in path} == {(0, 0), (1, 0), (1, 1)}
    assert {a[3] for a in path} == {NONE, STOP_EVENT, NATIVE_SIGNAL, EVENT_RECORD, NATIVE_DRAIN}
    assert {a[5] for a in path} == {0, 1, 0xFFFFFFFF} and {a[4] for a in path} == {0, 1, 2, 7, 8, 0xFFFFFFFF}
    assert {tuple(a) for a in g["flags"]["answers"]} == {(0, 0, 2), (1, 0, 2), (1, 1, 2), (3, 3, 3), (1, 0, 3), (1, 1, 3)}
    assert sorted(a[0] for a in g["tpw"]["answers"]) == [16, 32, 64] and sorted(a[0] for a in g["wide"]["answers"]) == [0, 1]
    assert all({a[i] for a in g["profile"]["answers"]} == {0, 1} for i in range(3)) and sorted(a[0] for a in g["feedback"]["answers"]) == [0, 8, 16]


@pytest.mark.parametrize("grid", ["batch", "path", "flags", "tpw", "wide", "profile", "feedback"])
def test_submit_decisions_are_the_parents(fixture, ask, grid):
    rows = replay(fixture, ask, grid)
    assert not differences(grid, fixture["grids"][grid]["first"], rows)
