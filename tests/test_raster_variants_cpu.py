"""The raster launch chooses what the hand-written ladder chose.  Every raster variant produces the same pixels, so a wrong choice
shows in no image: tests/golden/raster_variants.json holds the kernel, grid and block that launch_raster / launch_raster_batch of the
commit before the selector (the fixture's "parent", recorded by tools/make_raster_variants.py) picked for every row of a grid of
scopes, and mirhi_debug_raster_choice says what the library under test picks.  No GPU: the export makes no HIP call."""
import ctypes as C
import itertools
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_variants.json")
NOT_BATCHABLE = "not batchable"


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(FIXTURE))


@pytest.fixture(scope="module")
def rows(fixture):
    """The twelve input words of every row, n_batch left 0 (row = index in the product of the axes, first axis slowest)."""
    out = []
    for programs, ks, tp, teams, wide, alpha, swz, ordered, allow in itertools.product(*(values for _, values in fixture["axes"])):
        k = fixture["key_states"][ks]
        out.append([programs, allow, k["pred"], k["zflip"], k["zmask"], tp, teams, wide, alpha, swz, ordered, 0])
    return out


@pytest.fixture(scope="module")
def choose(mirhi):
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_raster_choice
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]

    def choose(words, n_batch):
        """'<kernel> grid X Y Z block B', or NOT_BATCHABLE."""
        name, shape = C.create_string_buffer(96), (C.c_uint32 * 4)()
        rc = fn((C.c_uint32 * 12)(*words[:11], n_batch), name, len(name), shape)
        assert rc in (0, 1) and (rc == 0 or n_batch >= 2)
        return NOT_BATCHABLE if rc else f"{name.value.decode()} grid {shape[0]} {shape[1]} {shape[2]} block {shape[3]}"
    return choose


def by_row(groups, n):
    out = [None] * n
    for what, members in groups.items():
        for i in members:
            assert out[i] is None
            out[i] = what
    assert None not in out
    return out


def test_fixture_is_the_whole_grid(fixture, rows):
    assert [name for name, _ in fixture["axes"]] == ["programs", "key_state", "tp_max_area", "raster_teams", "raster_wide", "alpha_scope", "xcd_swizzle", "ordered", "allow_wide"]
    assert [values for _, values in fixture["axes"]] == [[0, 1, 2, 3, 4, 7, 12, 28], ["plain", "flipped", "predicate"], [0, 64], [1, 2], [0, 8, 16], [0, 1], [1, 2], [0, 1], [0, 1]]
    assert fixture["key_states"] == {"plain": {"zflip": 0, "zmask": 0xFFFFFFFF, "pred": 0}, "flipped": {"zflip": 0xFFFFFFFF, "zmask": 0xFFFFFFFF, "pred": 0},
                                     "predicate": {"zflip": 0, "zmask": 0xFFFFFFFF, "pred": 5}}
    assert len(rows) == 4608 and len(fixture["parent"]) == 40
    by_row(fixture["single"], len(rows)); by_row(fixture["batched"], len(rows))
    assert sorted(i for m in fixture["parent_keys"].values() for i in m) == list(range(0, len(rows), 2))


def test_single_launch_choice_is_the_parents(fixture, rows, choose):
    want = by_row(fixture["single"], len(rows))
    wrong = [(i, rows[i], want[i], got) for i in range(len(rows)) if (got := choose(rows[i], 0)) != want[i]]
    assert not wrong, f"{len(wrong)} of {len(rows)} rows, first: {wrong[:3]}"


def test_batched_launch_choice_is_the_parents(fixture, rows, choose):
    want = by_row(fixture["batched"], len(rows))
    wrong = [(i, rows[i], want[i], got) for i in range(len(rows)) if (got := choose(rows[i], 2)) != want[i]]
    assert not wrong, f"{len(wrong)} of {len(rows)} rows, first: {wrong[:3]}"
    assert sum(w != NOT_BATCHABLE for w in want) == 40          # (not vacuous)


def parent_key(fixture, n):
    key = [None] * n
    for k, members in fixture["parent_keys"].items():
        for i in members:
            key[i] = key[i + 1] = k         # (rows 2k and 2k + 1 differ in allow_wide alone, which the key does not see)
    return key


def test_rows_batch_together_exactly_where_the_parents_did(fixture, rows, choose):
    """New rule: two command buffers share a batched launch when their variant has a batched form and the variants are equal, grid
    included -- what the export reports for n_batch = 2.  Parent's rule: raster_batchable for both and equal raster_variant_key.
    Stated over partitions, which says the same about every pair of rows: the same rows are batchable, and they fall into the same classes."""
    n = len(rows)
    parent_batched, key = by_row(fixture["batched"], n), parent_key(fixture, n)
    new = [choose(r, 2) for r in rows]
    assert [c != NOT_BATCHABLE for c in new] == [c != NOT_BATCHABLE for c in parent_batched]
    batchable = [i for i in range(n) if new[i] != NOT_BATCHABLE]
    classes_new, classes_parent = {}, {}
    for i in batchable:
        classes_new.setdefault(new[i], set()).add(i)
        classes_parent.setdefault(key[i], set()).add(i)
    assert sorted(map(sorted, classes_new.values())) == sorted(map(sorted, classes_parent.values()))
    assert len(classes_new) >= 10


def test_parents_equal_keys_meant_equal_launches(fixture, rows):
    """The old comment's promise, "equal keys <=> the same raster_kernel instantiation and grid", for the rows the key was ever compared on: those
    raster_batchable let through.  (Over all rows it did not hold -- the key saw neither alpha_scope nor allow_wide, and folded the program sets
    12 and 28, raster_kernel_shadow and raster_kernel_csm, into one -- which is why the key alone never decided anything.)"""
    n = len(rows)
    single, batched, key = by_row(fixture["single"], n), by_row(fixture["batched"], n), parent_key(fixture, n)
    launches = {}
    for i in range(n):
        if batched[i] != NOT_BATCHABLE:
            launches.setdefault(key[i], set()).add((single[i], batched[i]))
    assert len(launches) >= 10 and all(len(v) == 1 for v in launches.values()), {k: v for k, v in launches.items() if len(v) != 1}
    # and, among those rows, different keys meant different launches
    assert len({next(iter(v)) for v in launches.values()}) == len(launches)
