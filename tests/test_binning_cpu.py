"""The integer model of the geometry kernel's routing (tests/binning_cases.py) against the CPU oracle, and every case against the condition it was
built for.  No GPU.

The model says where a triangle goes (rejected, binned into which tiles, big list) and which pixel centres each (triangle, tile) pair covers; the
oracle knows nothing of tiles and renders the triangle alone.  Covered set against covered set, pixel for pixel; the per-tile sums against the
oracle's count.  tests/test_gpu_binning.py then holds the kernel's fragment count and big-list length against the model's figures."""
import numpy as np
import pytest

import binning_cases as bc

NO_PRIM = 0xFFFFFFFF
UNSPLIT = bc.unsplit_cases()
BY_NAME = {c.name: c for c in UNSPLIT}
SPLITS = [(kind, world, layout) for kind in bc.SPLIT_KINDS for layout in ("bands", "interleaved") for world in (2, 4)]


@pytest.fixture(scope="module")
def single(oracle, scenes):
    """The oracle's render of triangle k of a case, alone: the covered pixels.  Computed once per distinct triangle."""
    cache = {}

    def single(c, k):
        key = (c.tris[k], c.width, c.height, c.scissor, c.model) if not c.clipped else (c.name, k)
        if key not in cache:
            cache[key] = oracle.render(bc.scene_of(c, scenes, only=k), want_bgra8=False)["prim"] != NO_PRIM
        return cache[key]
    return single


def failures(c, single, rules=bc.KERNEL, split=None, rows=None):
    """Every way the model under `rules` disagrees with the oracle or with the case's own condition.  rows: the pixel rows the split owns (bool)."""
    out = []
    if c.clipped:
        rs = bc.model_case(c, split, rules)
        if len(rs) != c.expect["pieces"]:
            out.append(f"pieces {len(rs)} != {c.expect['pieces']}")
        union = np.zeros((c.height, c.width), dtype=bool)
        for r in rs:
            if r.route != "big":
                out.append("a piece is not on the big list")
            union |= r.covered
        if not np.array_equal(union, single(c, 0)):
            out.append("union of the pieces != the oracle's triangle")
        return out
    rs = bc.model_case(c, split, rules)
    for k, (t, r) in enumerate(zip(c.tris, rs)):
        want = single(c, k)
        if rows is not None:
            want = want & rows[:, None]
        if not np.array_equal(r.covered, want):
            out.append(f"triangle {k}: covered set differs in {int((r.covered != want).sum())} pixels")
        if r.frags != int(want.sum()):
            out.append(f"triangle {k}: per-tile sums {r.frags} != oracle {int(want.sum())}")
        if (r.route == "rejected") != (not want.any()):
            out.append(f"triangle {k}: route {r.route} ({r.why}) but the oracle covers {int(want.sum())} pixels")
    for key, v in c.expect.items():
        if key == "union_once":
            union = np.zeros((c.height, c.width), dtype=bool)
            for r in rs:
                union |= r.covered
            if not (sum(r.frags for r in rs) == int(union.sum()) == v):
                out.append(f"union_once: sum {sum(r.frags for r in rs)}, union {int(union.sum())}, wanted {v}")
        elif len(c.tris) > 100:         # (the pages cases: the condition holds for every triangle)
            out += [f"triangle {k}: {key} = {r.facts.get(key)!r}, built for {v!r}" for k, r in enumerate(rs) if r.facts.get(key) != v]
        elif rs[0].facts.get(key) != v:
            out.append(f"{key} = {rs[0].facts.get(key)!r}, built for {v!r}")
    return out


@pytest.mark.parametrize("name", [c.name for c in UNSPLIT])
def test_round_trip(name):
    """X, Y -> binary32 clip coordinates -> the kernel's window transform and snap -> X, Y, inside the guard band and |xs| <= 16383, checked with the
    draw's own gx, gy.  The clipped cases are the ones named as leaving the band."""
    c = BY_NAME[name]
    if c.clipped:
        hw, hh, cx, cy, gx, gy = bc.draw_constants(c.width, c.height)
        assert any(z < 0 or x > float(gx) for x, y, z in c.clip)
        return
    assert all(bc.round_trip(t, c.width, c.height) for t in c.tris)
    bc.vertices(c)          # (raises for a triangle that does not come back)


def test_a_case_off_the_grid_is_refused():
    t = bc.Tri((1, 2 ** 24 + 1, 5), (0, 7, 900))        # 2^24 + 1 is no binary32
    assert not bc.round_trip(t, 256, 256)
    with pytest.raises(ValueError):
        bc.vertices(bc.Case("off_grid", [t]))
    assert not bc.round_trip(bc.Tri((0, 256 * 16384, 5), (0, 7, 900)), 256, 256)       # beyond |xs| <= 16383
    assert not bc.round_trip(bc.Tri((0, 256 * 16100, 5), (0, 7, 900)), 256, 256)       # beyond the guard band


@pytest.mark.parametrize("name", [c.name for c in UNSPLIT])
def test_model_equals_the_oracle_and_the_case_sits_on_its_boundary(name, single):
    assert failures(BY_NAME[name], single) == []


def test_zero_area_padding_is_rejected(single):
    c = BY_NAME["waves_tpw64"]
    assert bc.tris_per_wave(BY_NAME["waves_tpw16"]) == 16 and bc.tris_per_wave(BY_NAME["waves_tpw32"]) == 32 and bc.tris_per_wave(c) == 64
    v = bc.vertices(c)
    n = len(c.tris)
    pad = v[3 * (n - n // 2):3 * (n - n // 2) + 3 * c.pad, :3]
    assert (pad == pad[0]).all()                                         # one point three times: S == 0 whatever the snap
    assert v.shape[0] == 3 * (n + c.pad) and (n + c.pad + 63) // 64 > 512


def test_largest_box_value_of_a_compact_triangle():
    """box_x_286: no compact triangle shows a tile of its span a larger (xmax - 128) >> 8.  The first pixel column px0 lies in the first tile
    (px0 - 32 tx0 <= 31) or left of it clamped (then tx0 = 0 and xmin < 0); (xmin + 127) >> 8 = px0 bounds xmin <= 256 px0 + 128, and
    xmax <= xmin + 65535 gives (xmax - 128) >> 8 <= px0 + 255."""
    best = 0
    for xmin in range(bc.px(128) - 127, bc.px(160) - 127):          # every xmin whose first pixel lies in tile 4
        px0 = (xmin + 127) >> 8
        assert 128 <= px0 <= 159
        best = max(best, ((xmin + 65535 - 128) >> 8) - 128)
    assert best == 286 == BY_NAME["box_x_286"].expect["box_hi_x_first"]


@pytest.mark.parametrize("rules, caught_by", [
    (bc.Rules(lo=128), ["tie_vertices", "tie_tile_boundary_first", "tie_tile_boundary_last"]),
    (bc.Rules(tie_bias=False), ["tie_vertices", "tie_tile_boundary_first", "tie_tile_boundary_last"]),
    (bc.Rules(ntx_unclamped=True), ["reach_x_n1_on", "reach_x_n1_in", "box_x_128", "box_x_255", "box_x_286", "extent_x_on"]),
], ids=["plus_128", "no_tie_bias", "ntx_unclamped"])
def test_planted_errors_are_caught(rules, caught_by, single):
    """The model with one rule changed must disagree with the oracle, or with a case's condition, in the cases built for that rule."""
    for name in caught_by:
        assert failures(BY_NAME[name], single, rules) != [], name
    caught = [c.name for c in UNSPLIT if len(c.tris) <= 100 and failures(c, single, rules)]
    assert set(caught_by) <= set(caught)


# ---- tile-row split ----
def _rows(split, height):
    mine = np.zeros(height, dtype=bool)
    for row in split.rows():
        mine[row * bc.TILE:(row + 1) * bc.TILE] = True
    return mine


@pytest.mark.parametrize("kind, world, layout", SPLITS, ids=[f"{k}-{l}{w}" for k, w, l in SPLITS])
def test_split_model_equals_the_oracle(kind, world, layout, single, mirhi):
    from renderer_rs_amd import multigpu
    c = bc.split_case(kind, world, layout)
    total = np.zeros((c.height, c.width), dtype=np.int32)
    for rank in range(world):
        s = bc.split_of(rank, world, layout)
        assert (s.first, s.step, s.count) == multigpu.split_tile_rows(c.height, rank, world, layout)
        assert failures(c, single, split=s, rows=_rows(s, c.height)) == []
        rs = bc.model_case(c, s)
        for r in rs:
            total += r.covered
        # the condition the rank's own triangle (triangle `rank`) was built for
        f, own = rs[rank].facts, rs[rank]
        rows = s.rows()
        first = rows[0] if layout == "bands" else next(q for q in rows if q >= 4)
        last = rows[-1] if layout == "bands" else first
        if kind == "last_owned_row":
            assert own.route == "binned" and own.box[3] == (last + 1) * bc.TILE - 1
            if last + 1 < c.height // bc.TILE:
                assert c.tris[rank].Y[2] + 1 - 128 == (last + 1) * bc.TW       # one sub-pixel further and the box enters the next band
        elif kind == "next_band_first_pixel" and last + 1 < c.height // bc.TILE:
            assert own.route == "rejected" and own.why == "no owned row"
            keepers = [q for q in range(world) if bc.model_case(c, bc.split_of(q, world, layout))[rank].route != "rejected"]
            assert len(keepers) == 1 and keepers[0] != rank
        elif kind == "reach_from_above_on":
            assert own.route == "binned" and f["margin_lo_y"] == 0 and f["box_lo_y_last"] == -128
        elif kind == "reach_from_above_out":
            assert own.route == "big" and f["margin_lo_y"] == -1 and f["compact"]
        elif kind == "tall_255":
            assert f["rows_spanned"] >= 8 and f["nty"] <= f["rows_spanned"] and f["extent_y"] == 255 * 256
            if layout == "interleaved":
                assert f["nty"] < f["rows_spanned"]
        elif kind == "tall_5_rows" and layout == "interleaved":
            assert own.route == "binned" and f["rows_spanned"] == 5 > bc.MAX_BIN_SPAN >= f["nty"] and f["margin_lo_y"] == 0
        elif kind == "nothing_owned":
            assert own.route == "rejected" and own.why == "no owned row"
            # one pixel row from an owned row: the box ends on the row above the band's first, or starts on the row below its last
            unsplit = bc.route(c.tris[rank], c.width, c.height)
            assert unsplit.box[3] + 1 == first * bc.TILE or unsplit.box[2] - 1 == (last + 1) * bc.TILE - 1
    assert (total <= len(c.tris)).all()
    # every covered pixel of every triangle is some rank's, once
    want = sum(single(c, k).astype(np.int32) for k in range(len(c.tris)))
    assert np.array_equal(total, want)


def test_case_counts():
    """What DESIGN.md 8r and the commit message report."""
    on = [c for c in UNSPLIT if c.boundary == "on"]
    assert len(UNSPLIT) == 62 and len(on) == 23 and len([c for c in UNSPLIT if c.boundary]) == 47 and len([c for c in UNSPLIT if bc.pairable(c)]) == 35
    assert len(SPLITS) == 28
