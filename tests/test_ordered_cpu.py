"""The model of fragment order and blending (tests/ordered_cases.py) against the CPU oracle, every case against the condition it was built for, and
the planted errors the comparison must reject.  No GPU.

The layers come from the oracle's renders of each live triangle alone and opaque; the model's frame must EQUAL the oracle's render of the whole
scene: float colour bits, depth bits, primitive ids.  tests/test_gpu_ordered.py then holds ordered_kernel against the same model, with the layers the
GPU rendered."""
import numpy as np
import pytest

import binning_cases as bc
import ordered_cases as oc
import render_area_cases as rc

NO_PRIM = oc.NO_PRIM
CASES = {c.name: c for c in oc.float_cases() + oc.split_cases()}
ORDER_CASES = [c.name for c in oc.slot_cases() + oc.marker_cases() + oc.load_store_cases() + oc.block_cases() + oc.split_cases()]
SENT = rc.sentinels(oc.W, oc.H, seed=5)
PRIOR = oc.Frame(SENT["float"], SENT["depth"], SENT["prim"])


@pytest.fixture(scope="module")
def world(oracle, scenes):
    """The oracle's renders, each computed once: the single-layer sources by their key, and the whole scenes by case name."""
    groups, frames = {}, {}

    def render(scene, key=None):
        k = (scene.width, scene.height, key)
        if key is None or k not in groups:
            got = oracle.render(scene, want_bgra8=False)
            got = {"color": got["rgba"], "prim": got["prim"], "depth": got["depth"]}
            if key is None:
                return got
            groups[k] = got
        return groups[k]

    class World:
        def sources(self, c):
            return oc.sources_of(c, scenes, render)

        def frame(self, c):
            """The oracle's frame of the whole case (a render area: the scissors cut to it, over the prior contents -- render_area_cases E1)."""
            if c.name not in frames:
                scene = oc.scene_of(c, scenes, area=False)
                if c.render_area is not None:
                    got = render(rc.cut_to_area(scene, c.render_area))
                    got = {"color": rc.compose(got["color"], PRIOR.color, c.render_area), "depth": rc.compose(got["depth"], PRIOR.depth, c.render_area),
                           "prim": rc.compose(got["prim"], PRIOR.prim, c.render_area)}
                else:
                    got = render(scene)
                frames[c.name] = got
            return frames[c.name]

        def render(self, scene):
            return render(scene)
    return World()


def differences(frame: oc.Frame, ref) -> np.ndarray:
    """The pixels in which a model frame and a rendered one differ in any bit of colour, depth or primitive id."""
    return (np.any(frame.color.view(np.uint32) != ref["color"].view(np.uint32), axis=-1) | (frame.depth.view(np.uint32) != ref["depth"].view(np.uint32))
            | (frame.prim != ref["prim"]))


def model(c, world, rules=oc.EXACT, permute=None):
    return oc.model_frame(c, world.sources(c), rules, PRIOR if c.render_area is not None else None, permute)


@pytest.mark.parametrize("name", list(CASES))
def test_model_equals_the_oracle(name, world):
    c = CASES[name]
    bad = differences(model(c, world), world.frame(c))
    assert not bad.any(), f"{int(bad.sum())} pixels differ, the first at {tuple(np.argwhere(bad)[0][::-1])}"


def test_row_cases_equal_the_oracle(world):
    for row in oc.table_rows() + oc.mask_rows():
        c = oc.row_case(row)
        assert not differences(model(c, world), world.frame(c)).any(), row.name


# ---- the cases against their conditions ----
@pytest.mark.parametrize("name", [c.name for c in oc.slot_cases() + oc.marker_cases()])
def test_live_triangles_sit_at_their_slots(name):
    c = CASES[name]
    si = c.expect.get("segment", 0)
    state, dis = c.segments()[si]
    assert state.ordered and c.ordered_segments() == 1
    slots = c.segment_slots(si)
    if "slots" in c.expect:
        assert slots == c.expect["slots"]
    else:
        first = c.prim_base(dis[0])
        markers = [c.prim_base(di) + k - first for di in dis for k, s in enumerate(c.draws[di].slots) if isinstance(s, oc.Live) and s.clip is not None]
        assert markers == c.expect["markers"] and set(markers) <= set(slots)


def test_slot_cases_reach_what_they_name():
    by = {c.name: c for c in oc.slot_cases()}
    n = lambda name, si=0: sum(len(by[name].draws[di].slots) * by[name].draws[di].instances for di in by[name].segments()[si][1])
    assert [n("slots_1"), n("slots_256"), n("slots_257"), n("slots_513"), n("slots_768_skip"), n("slots_300_behind_100", 1)] == [1, 256, 257, 513, 768, 300]
    c = by["slots_768_skip"]
    slots = c.draws[0].slots
    assert all(s == oc.FILL for s in slots[256:512]) and not any(s == oc.FILL for s in slots[:256] + slots[512:])
    assert all(s // oc.CHUNK != 1 for s in c.segment_slots(0)) and {s // oc.CHUNK for s in c.segment_slots(0)} == {0, 2}
    c = by["slots_300_behind_100"]
    first = c.prim_base(c.segments()[1][1][0])
    assert first == 100 and first % oc.CHUNK != 0
    assert by["slots_two_draws_instanced"].draws[1].instances == 2 and len(by["slots_two_draws_instanced"].segments()) == 1
    c = {c.name: c for c in oc.marker_cases()}["marker_alone_in_chunk"]
    assert [k for k, s in enumerate(c.draws[0].slots) if k >= oc.CHUNK and s != oc.ZERO] == [300]


def test_fillers_keep_to_tile_b_and_live_triangles_reach_tile_a(world):
    c = CASES["slots_257"]
    src = world.sources(c)
    tile = lambda t: (slice(32 * t[1], 32 * t[1] + 32), slice(32 * t[0], 32 * t[0] + 32))
    for key, (cover, _, _) in src.items():
        if key[0] == oc.FILL_TRI:
            assert cover.any() and cover[tile(oc.TILE_B)].sum() == cover.sum()
        else:
            assert cover[tile(oc.TILE_A)].any()
    # the marker that misses tile A: all of it inside tile B
    c = CASES["marker_misses_tile"]
    cover = next(v[0] for k, v in world.sources(c).items() if k[0] == oc.CLIP_NEAR_B)
    assert cover.any() and cover[tile(oc.TILE_B)].sum() == cover.sum()


@pytest.mark.parametrize("which", ["near", "guard", "near_b"])
def test_clipped_triangles_have_pieces_that_do_not_overlap(which, world, scenes):
    lv = {"near": oc.CLIP_NEAR, "guard": oc.CLIP_GUARD, "near_b": oc.CLIP_NEAR_B}[which]
    pieces = bc.clip_pieces(list(lv.clip), oc.W, oc.H)
    assert len(pieces) >= 2
    hw, hh, cx, cy, gx, gy = bc.draw_constants(oc.W, oc.H)
    assert any(z < 0 or x > float(gx) for x, y, z in lv.clip)
    opaque = world.render(oc.scene_of(oc.Case("alone", [oc.Draw([lv], oc.OPAQUE)], clear_color=(0, 0, 0, 0)), scenes))
    additive = oc.State(False, False, oc.ALWAYS, (oc.ONE_F, oc.ONE_F, oc.ADD, oc.ONE_F, oc.ONE_F, oc.ADD, 0xF))
    summed = world.render(oc.scene_of(oc.Case("summed", [oc.Draw([lv], additive)], clear_color=(0, 0, 0, 0)), scenes))
    assert (opaque["prim"] == 0).sum() > 20
    assert np.array_equal(opaque["color"].view(np.uint32), summed["color"].view(np.uint32))      # a pixel under two pieces would hold twice the colour


def _swaps(c):
    """Every exchange of two live layers that follow each other in a segment (fillers between them stay where they are)."""
    live_prims = set()
    for di, d in enumerate(c.draws):
        for inst in range(d.instances):
            live_prims |= {c.prim_base(di) + inst * len(d.slots) + k for k in c.live_slots(di) if d.slots[k] != oc.FILL_TRI}
    out = []
    for si, (state, dis) in enumerate(c.segments()):
        prims = sorted(p for p in live_prims if c.prim_base(dis[0]) <= p < c.prim_base(dis[-1]) + len(c.draws[dis[-1]].slots) * c.draws[dis[-1]].instances)
        out += [(a, b) for a, b in zip(prims, prims[1:]) if state.ordered]
    return out


def _swap(a, b):
    def permute(layers):
        ids = [L.prim for L in layers]
        if a not in ids or b not in ids:
            return layers
        i, j = ids.index(a), ids.index(b)
        out = list(layers)
        out[i], out[j] = oc.Layer(a, layers[j].cover, layers[j].depth, layers[j].color), oc.Layer(b, layers[i].cover, layers[i].depth, layers[i].color)
        return out
    return permute


@pytest.mark.parametrize("name", ORDER_CASES)
def test_the_order_of_any_two_neighbours_shows(name, world):
    """Planted error 1 as well: the comparison with the oracle rejects the model with two adjacent layers exchanged (the ids stay in order, the
    triangles change places)."""
    c = CASES[name]
    swaps = _swaps(c)
    assert swaps or len([s for d in c.draws for s in d.slots if isinstance(s, oc.Live)]) == 1
    ref = world.frame(c)
    for a, b in swaps:
        assert differences(model(c, world, permute=_swap(a, b)), ref).any(), (a, b)


DEPTH = [c.name for c in oc.depth_cases()]


@pytest.mark.parametrize("name", DEPTH)
def test_running_depth_shows(name, world):
    """Planted error 2: the depth test against the depth the segment started from.  EQUAL (it rewrites what it found) and ALWAYS (it reads nothing)
    cannot tell the two rules apart, nor can a tie under LESS_OR_EQUAL (both rules take the second layer): there the frames are the same, and that is
    asserted too.  A tie under LESS does tell them apart: the running depth refuses the second layer, the clear depth would take it."""
    c = CASES[name]
    bad = differences(model(c, world, oc.Rules(initial_depth=True)), world.frame(c))
    assert bad.any() == c.expect["differs"]
    if name.startswith("depth_tie"):
        # the second layer of a tie: refused by LESS, taken by LESS_OR_EQUAL and EQUAL
        first, second = oc.layers_of(c, len(c.draws) - 1, world.sources(c))
        both = first.cover & second.cover
        assert both.any() and (world.frame(c)["prim"][both] == second.prim).all() == (c.expect["op"] != oc.LESS)
        assert (world.frame(c)["prim"][both] == first.prim).all() == (c.expect["op"] == oc.LESS)


def test_table_rows_are_told_apart(world):
    """Every two rows differ in some pixel of the oracle's frame -- but for two MIN rows or two MAX rows, which ignore their factors (table 28.2)
    and must give the SAME frame; the mask rows differ from one another."""
    rows = oc.table_rows()
    cell = lambda row: world.frame(oc.row_case(row))["color"][:oc.CELL, :oc.CELL].view(np.uint32)
    frames = [cell(r) for r in rows]
    same = [(a.name, b.name) for i, a in enumerate(rows) for j, b in enumerate(rows[:i]) if np.array_equal(frames[i], frames[j])]
    allowed = [(a, b) for a, b in same if a[:3] == b[:3] and a[:3] in ("op3", "op4")]
    assert same == allowed, [p for p in same if p not in allowed]
    assert len(allowed) == 2 * (11 * 10 // 2)
    masks = [cell(r) for r in oc.mask_rows()]
    assert all(not np.array_equal(a, b) for i, a in enumerate(masks) for b in masks[:i])
    # SRC_ALPHA_SATURATE lies on both sides of 1 - Ad: the first layer's alpha below the clear's 1 - 0.5, the second's above
    assert oc.TABLE_ALPHAS[0] < 1.0 - oc.TABLE_CLEAR[3] < oc.TABLE_ALPHAS[1]
    src = world.sources(oc.row_case(rows[0]))
    covers = [v[0] for v in src.values()]
    assert (covers[0] & ~covers[1]).any() and (covers[1] & ~covers[0]).any() and (covers[0] & covers[1]).any()
    assert sorted({float(v[2][v[0]][0, 3]) for v in src.values()}) == list(oc.TABLE_ALPHAS)


def test_table_covers_what_it_names():
    rows = oc.table_rows()
    add = [r.blend for r in rows if r.blend[2] == oc.ADD]
    assert len(rows) == 165 and {(b[0], b[1]) for b in add} == {(s, d) for s in oc.FACTORS for d in oc.FACTORS}
    for op in range(5):
        bl = [r.blend for r in rows if r.blend[2] == op]
        assert all(b[5] == op for b in bl)
        for pos in (0, 1, 3, 4):
            assert {b[pos] for b in bl} == set(oc.FACTORS), (op, pos)
        if op != oc.ADD:
            assert len(bl) == 11 and sorted(b[0] for b in bl) == sorted(oc.FACTORS) == sorted(b[1] for b in bl)
    assert [r.blend[6] for r in oc.mask_rows()] == list(range(16)) and all(r.blend[2] != r.blend[5] for r in oc.mask_rows())
    packed = oc.table_cases()
    assert [n for c in packed for n in c.expect["rows"]] == [r.name for r in rows + oc.mask_rows()]
    assert all(c.ordered_segments() == len(c.expect["rows"]) for c in packed)


# ---- planted errors in the blend table ----
def _rows_rejected(world, rules):
    """The rows of the packed table in whose cell the model under `rules` and the oracle differ; nothing may differ outside the cells."""
    out = []
    for c in oc.table_cases():
        bad = differences(model(c, world, rules), world.frame(c))
        for r, name in enumerate(c.expect["rows"]):
            if bad[oc.cell_of(c, r)].any():
                out.append(name)
    return out


def _uses(row, factor=None, positions=(0, 1, 3, 4)):
    return any(row.blend[p] == factor for p in positions)


def test_planted_blend_errors_are_rejected(world):
    rows = {r.name: r for r in oc.table_rows() + oc.mask_rows()}
    minmax = lambda r, colour: rows[r].blend[2 if colour else 5] in (oc.MIN, oc.MAX)
    # DST_ALPHA in place of ONE_MINUS_DST_ALPHA: rejected in every row that reads factor 9 (MIN and MAX read no factor) -- and in no other
    got = _rows_rejected(world, oc.Rules(dst_alpha_swapped=True))
    reads = [n for n, r in rows.items() if (_uses(r, 9, (0, 1)) and not minmax(n, True) and r.blend[6] & 7) or (_uses(r, 9, (3, 4)) and not minmax(n, False) and r.blend[6] & 8)]
    assert set(got) <= set(n for n, r in rows.items() if _uses(r, 9))
    colour = [n for n in reads if _uses(rows[n], 9, (0, 1)) and not minmax(n, True) and rows[n].blend[6] & 7]
    assert len(colour) == 25 and set(colour) <= set(got), sorted(set(colour) - set(got))      # (A_SHIFT: the first layer always leaves another alpha than 0.5)
    assert len(set(reads) & set(got)) >= len(reads) - 8, sorted(set(reads) - set(got))          # (read in an alpha position only: most, not all)
    # REVERSE_SUBTRACT as SUBTRACT
    got = _rows_rejected(world, oc.Rules(rsub_as_sub=True))
    rsub = [n for n, r in rows.items() if (r.blend[2] == oc.REVERSE_SUBTRACT and r.blend[6] & 7) or (r.blend[5] == oc.REVERSE_SUBTRACT and r.blend[6] & 8)]
    assert len(rsub) >= 11 and set(got) == set(rsub)
    # the write mask ignored: every mask row but the full mask
    got = _rows_rejected(world, oc.Rules(ignore_mask=True))
    assert set(got) == {f"mask_{m}" for m in range(15)}
    # SRC_ALPHA_SATURATE's alpha factor as `sat`
    got = _rows_rejected(world, oc.Rules(sat_alpha=True))
    sat = [n for n, r in rows.items() if _uses(r, oc.SRC_ALPHA_SATURATE, (3, 4)) and not minmax(n, False) and r.blend[6] & 8]
    assert len(sat) >= 20 and set(got) == set(sat), (sorted(set(sat) - set(got)), sorted(set(got) - set(sat)))


# ---- the model's own rules that no case above reaches ----
def _flat(h, w, prim, z, rgba, cover=None):
    return oc.Layer(prim, np.ones((h, w), dtype=bool) if cover is None else cover, np.full((h, w), z, dtype=np.float32), np.tile(np.asarray(rgba, dtype=np.float32), (h, w, 1)))


def test_same_primitive_under_always_with_write_keeps_the_nearer():
    c = oc.Case("x", [], width=4, height=2, clear_depth=0.0)
    start = oc.initial_frame(c)
    st = oc.State(True, True, oc.ALWAYS, oc.ORDER_BLEND)
    near, far = _flat(2, 4, 7, 0.25, (0.5, 0.5, 0.5, 1.0)), _flat(2, 4, 7, 0.75, (0.5, 0.5, 0.5, 1.0))
    a, b = oc.resolve(start, [near, far], st), oc.resolve(start, [far, near], st)
    assert (a.depth == 0.25).all() and (b.depth == 0.25).all() and (a.prim == 7).all()
    once = oc.resolve(start, [near], st)
    assert np.array_equal(a.color, once.color) and not np.array_equal(b.color, once.color)       # the farther one second: refused; first: both are blended
    other = oc.resolve(start, [near, _flat(2, 4, 8, 0.75, (0.5, 0.5, 0.5, 1.0))], st)
    assert (other.depth == 0.75).all() and (other.prim == 8).all()                                 # another primitive: ALWAYS takes it


def test_the_regression_scene_of_overlapping_pieces_runs_through_the_model(oracle, scenes):
    """tests/test_oracle_kats.overlapping_clip_pieces_scene: pixel (183, 38) holds two fragments of primitive 0.  Its two fragments as two layers of one
    id -- the nearer from a LESS render, the farther from a GREATER render -- under ALWAYS with write: the model stores the nearer depth whatever
    their order, as the oracle does."""
    from test_oracle_kats import overlapping_clip_pieces_scene
    get = lambda op, clear, **kw: oracle.render(overlapping_clip_pieces_scene(scenes, op, clear_depth=clear, **kw), want_bgra8=False)
    less, greater, always = get(scenes.CMP_LESS, 1.0), get(scenes.CMP_GREATER, 0.0), get(scenes.CMP_ALWAYS, 0.0)
    cover = less["prim"] == 0
    near, far = oc.Layer(0, cover, less["depth"], less["rgba"]), oc.Layer(0, cover, greater["depth"], greater["rgba"])
    c = oc.Case("kat", [], width=272, height=45, clear_color=(0.2, 0.3, 0.4, 0.5), clear_depth=0.0)
    for layers in ([near, far], [far, near]):
        out = oc.resolve(oc.initial_frame(c), layers, oc.State(True, True, oc.ALWAYS, None))
        assert np.array_equal(out.depth.view(np.uint32), always["depth"].view(np.uint32)) and np.array_equal(out.prim, always["prim"])


def test_discard_writes_nothing():
    c = oc.Case("x", [], width=4, height=2)
    start = oc.initial_frame(c)
    st = oc.State(True, True, oc.LESS, None, cutoff=0.5)
    out = oc.resolve(start, [_flat(2, 4, 1, 0.5, (1, 0, 0, 0.25)), _flat(2, 4, 2, 0.75, (0, 1, 0, 0.5))], st)
    assert (out.prim == 2).all() and (out.depth == 0.75).all() and np.array_equal(out.color[0, 0], np.asarray((0, 1, 0, 0.5), dtype=np.float32))


def test_srgb8_encoding():
    v = np.asarray([[[0.0, 0.0031308, 0.5, 0.25], [1.0, 2.0, -1.0, 1.0]]], dtype=np.float32)
    assert oc.srgb8_of(v).tolist() == [[[188, 10, 0, 64], [0, 255, 255, 255]]]


def test_case_counts():
    """What DESIGN.md 8s and the commit message report."""
    assert (len(oc.slot_cases()), len(oc.marker_cases()), len(oc.depth_cases()), len(oc.table_cases()), len(oc.load_store_cases()), len(oc.block_cases())) == (7, 10, 33, 2, 4, 1)
    assert sum(1 for c in oc.depth_cases() if c.expect["differs"]) == 21
    assert len(oc.float_cases()) == 57 and len(oc.srgb8_cases()) == 12 and len(oc.split_cases()) == 2
    assert all(len({s for d in c.draws for s in d.slots if isinstance(s, oc.Live) and s != oc.FILL_TRI}) <= 8 for c in oc.slot_cases() + oc.marker_cases() + oc.depth_cases() + oc.block_cases())
