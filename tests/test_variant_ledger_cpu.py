"""The ledger of tests/variant_cases.py against the launch tables (mirhi_debug_raster_table: no HIP call), and the conditions of its scenes on the
oracle alone, so that a GPU visit never discovers a badly chosen input: the twin condition of the generic-key rows, the small triangle, the
multi-tile triangle and the tile of more than 64 records of every rastered scene, the share the alpha-masked material discards, the covered pixels of
every case, the multisample condition -- and that the bit-for-bit comparison rejects the planted errors.  No GPU."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import msaa_cases
import render_area_cases as rc
import variant_cases as vc

NO_PRIM = vc.NO_PRIM
KINDS = ("tri", "model", "mixed", "pbr", "masked", "ibl")


@pytest.fixture(scope="module")
def lib(mirhi):
    return C.CDLL(mirhi.LIB_PATH)


@pytest.fixture(scope="module")
def tables(lib):
    fn = lib.mirhi_debug_raster_table
    fn.restype, fn.argtypes = C.c_int, [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32]
    out = []
    for table in range(3):
        names, buf = [], C.create_string_buffer(128)
        while fn(table, len(names), buf, len(buf)) == 0:
            names.append(buf.value.decode())
        assert fn(table, len(names) + 1000, buf, len(buf)) == 1
        out.append(names)
    assert fn(3, 0, C.create_string_buffer(8), 8) == 1          # no fourth table
    return out


def _row(kind, **kw):
    return dataclasses.replace(next(r for r in vc.ROWS if r.kind == kind), area=False, **kw)


@pytest.fixture(scope="module")
def frames(oracle):
    """oracle frames per (kind, variant, key), rendered once"""
    cache = {}

    def get(kind, variant, key="less"):
        if (kind, variant, key) not in cache:
            scene = vc.depth_oracle_scene(variant, key) if kind == "depth" else vc.oracle_scene(_row(kind), variant, key)
            cache[(kind, variant, key)] = oracle.render(scene, want_bgra8=False)
        return cache[(kind, variant, key)]
    return get


# ---- the ledger is the tables ---------------------------------------------------------------------------------------------------------------------
def test_ledger_keys_are_the_table_names(tables):
    assert [len(t) for t in tables] == [172, 10, 4]
    names = [n for t in tables for n in t]
    assert len(set(names)) == len(names) == 186, "a kernel name occurs twice in the tables"
    missing, extra = sorted(set(names) - set(vc.LEDGER)), sorted(set(vc.LEDGER) - set(names))
    assert not missing and not extra, f"table rows without a ledger entry: {missing}; ledger entries without a table row: {extra}"
    assert {r.name for r in vc.ROWS if r.route == "batch"} == set(tables[1]) and {r.name for r in vc.ROWS if r.route == "multiview"} == set(tables[2])


def test_unreachable_rows_are_none(tables):
    """An entry may be marked unreachable only with the line of raster_variant / mirhi_scope.h that excludes it; every row has an input that yields it."""
    unreachable = [r for r in vc.ROWS if r.unreachable]
    print(f"LEDGER unreachable rows: {len(unreachable)} of {len(vc.ROWS)}")
    assert all("mirhi_" in r.unreachable for r in unreachable)
    assert len(unreachable) == 0


def test_every_entry_states_its_case():
    for r in vc.ROWS:
        assert set(r.knobs) == {"MIRHI_TP_MAX_AREA", "MIRHI_TP_DENSITY", "MIRHI_RASTER_TEAMS", "MIRHI_RASTER_WIDE"} and r.yardstick and r.kind and r.key
        assert r.anchor in vc.LEDGER and len(r.seamless) == 3
        if r.teams == 2 or r.wide:          # two-team and wide rows: mesh scenes without a TRIANGLE draw, at program sets 2 and 4
            assert r.kind in ("model", "pbr", "masked") and vc.PROGRAM_SETS[r.kind] in (2, 4)
    anchors = {r.anchor for r in vc.ROWS if r.family not in ("predicate", "ordered", "sky", "transfer") and r.route != "multiview"}
    assert anchors == set(vc.ANCHOR_CHECKS), sorted(anchors ^ set(vc.ANCHOR_CHECKS))
    assert all(vc.LEDGER[a].key == "less" and not vc.LEDGER[a].area for a in anchors)


def test_the_launch_record_is_off_and_empty(lib):
    read = lib.mirhi_debug_raster_trace_read
    read.restype, read.argtypes = C.c_uint32, [C.c_char_p, C.c_uint32]
    buf = C.create_string_buffer(b"x" * 15, 16)
    assert read(buf, 16) == 0 and buf.value == b""
    assert read(None, 0) == 0


# ---- the scenes' conditions -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS + ("depth",))
def test_twin_condition(frames, kind):
    """The twin scene's primitive-id image is the same under LESS / clear 1 and GREATER / clear 0 (no pixel is covered by two primitives), its depth too
    where covered; the overdraw scene's is not, by hundreds of pixels."""
    less, greater = frames(kind, "twin", "less"), frames(kind, "twin", "greater")
    covered = less["prim"] != NO_PRIM
    assert np.array_equal(less["prim"], greater["prim"]) and covered.sum() > 1000
    assert np.array_equal(less["depth"].view(np.uint32)[covered], greater["depth"].view(np.uint32)[covered])
    if kind != "depth":
        assert np.array_equal(less["rgba"].view(np.uint32), greater["rgba"].view(np.uint32))
    over_l, over_g = frames(kind, "overdraw", "less"), frames(kind, "overdraw", "greater")
    assert (over_l["prim"] != over_g["prim"]).sum() > 300
    n_a = vc.layer_triangles("A")
    for f in (over_l, over_g):          # both layers win pixels under both states
        won = f["prim"][f["prim"] != NO_PRIM]
        assert (won < n_a).sum() > 300 and (won >= n_a).sum() > 300


def test_single_triangle_coverages(oracle, scenes):
    """From the oracle's coverage of every triangle drawn alone: the twin and the overdraw scene hold a triangle whose pixel box is at most 64 pixels,
    one that spans at least 2 x 2 tiles, and one tile in which more than 64 triangles cover pixels (more than 64 records: past one lane group)."""
    per_tile = np.zeros((4, 4), dtype=int)
    small = multi = 0
    for layer in "AB":
        big, tiny = vc.layer_points(layer)
        pts = big + tiny
        for t in range(len(pts) // 3):
            draw = scenes.DrawSpec(vertices=scenes._tri_verts(np.array(msaa_cases.clip_of(pts[3 * t:3 * t + 3]), dtype=np.float32)), stride=24, count=3,
                                   cull_mode=scenes.CULL_NONE, viewport=vc.VIEWPORT)
            ys, xs = np.nonzero(oracle.render(scenes.Scene("one", vc.W, vc.H, [draw]), want_bgra8=False)["prim"] != NO_PRIM)
            assert ys.size > 0, f"triangle {t} of layer {layer} covers no pixel centre"
            box = (xs.max() - xs.min() + 1) * (ys.max() - ys.min() + 1)
            cols, rows = xs.max() // 32 - xs.min() // 32 + 1, ys.max() // 32 - ys.min() // 32 + 1
            small += box <= 64
            multi += cols >= 2 and rows >= 2
            for ty, tx in {(int(y) // 32, int(x) // 32) for y, x in zip(ys, xs)}:
                per_tile[ty, tx] += 1
        if layer == "A":          # the twin scene alone already holds all three
            assert small >= 72 and multi >= 2 and per_tile[vc.BUSY_TILE[1], vc.BUSY_TILE[0]] > 64, (small, multi, per_tile)
    assert small >= 88 and multi >= 5 and per_tile.max() == per_tile[vc.BUSY_TILE[1], vc.BUSY_TILE[0]] > 64
    assert (per_tile[3] > 0).all() and (per_tile[1:, 3] > 0).all(), "the partial tiles at the right and the bottom edge hold records"


def test_masked_scene_discards_a_part_of_the_mesh(frames):
    for variant in ("twin", "overdraw", "B"):
        whole, cut = frames("pbr", variant)["prim"] != NO_PRIM, frames("masked", variant)["prim"] != NO_PRIM
        assert not (cut & ~whole).any()
        share = 1.0 - cut.sum() / whole.sum()
        print(f"LEDGER masked {variant}: {share:.1%} of the covered pixels discarded")
        assert 0.10 <= share <= 0.90


@pytest.mark.parametrize("kind", KINDS + ("depth",))
def test_every_case_covers_pixels(frames, kind):
    """A few hundred covered pixels in every scene a row renders, and inside the render area of the AREA rows; the area cuts through covered pixels."""
    size = vc.MAP if kind == "depth" else vc.W
    inside = rc.mask(vc.MAP_AREA if kind == "depth" else vc.AREA, size, size)
    for variant in ("overdraw", "twin", "B"):
        for key in ("less", "greater"):
            covered = frames(kind, variant, key)["prim"] != NO_PRIM
            assert covered.sum() >= 500, (variant, key, int(covered.sum()))
            if variant != "B":
                assert (covered & inside).sum() >= 300 and (covered & ~inside).sum() >= 300, (variant, key)
    if kind in ("tri", "model", "mixed", "pbr"):
        for key in ("predicate", "blend"):
            assert (frames(kind, "overdraw", key)["prim"] != NO_PRIM).sum() >= 500


def test_colour_depends_on_primitive_and_pixel_alone(frames):
    """The premise of the generic-key rows' colour yardstick, on the oracle: the overdraw scene's GREATER frame is, bit for bit, the frames of its two layers
    drawn alone, picked per pixel by the winning primitive."""
    for kind in KINDS:
        over = frames(kind, "overdraw", "greater")
        a, b = ({"prim": f["prim"], "color": f["rgba"]} for f in (frames(kind, "twin"), frames(kind, "B")))
        want = vc.compose_by_primitive(over["prim"], a, b, vc.CLEAR)
        assert np.array_equal(want.view(np.uint32), over["rgba"].view(np.uint32)), kind


def test_multisample_condition_holds(scenes):
    for p, kind in vc.KINDS.items():
        for variant in ("overdraw", "twin", "B"):
            checked, failed = msaa_cases.condition_holds(scenes, vc.scene_for(_row(kind), variant))
            assert checked >= 60 and failed == 0, (kind, variant, checked, failed)


def test_shadow_terms_shade_a_part_of_the_receivers(scenes):
    """The casters' footprints in every light matrix lie over a part of layer A's quad, and the splits select every cascade: the lit rows' frames depend on their
    shadow term.  (Window-space reasoning alone: light clip = scale * clip + scale - 1, depth = z.)"""
    big, _ = vc.layer_points("A")
    z = np.array([p[2] for p in big + vc.layer_points("B")[0]])
    splits = np.array(vc.CASCADE_SPLITS)
    assert z.min() < splits[0] and (z > splits[2]).any() and ((z > splits[0]) & (z < splits[1])).any()
    for s in vc.CASCADE_SCALES:
        win = np.array(vc.caster_points())[:, :2]
        texel = (s * ((win - 128.0) / 128.0) + s - 1.0 + 1.0) * 0.5 * vc.MAP
        assert texel.min() >= 0 and texel.max() <= vc.MAP, "a caster leaves the map"
    assert all(p[2] < z.min() for p in vc.caster_points())


# ---- planted errors -----------------------------------------------------------------------------------------------------------------------------------
def test_comparison_rejects_the_planted_errors(frames):
    ref = frames("pbr", "overdraw")
    good = {"color": ref["rgba"].copy(), "prim": ref["prim"].copy(), "depth": ref["depth"].copy()}
    sent = rc.sentinels(vc.W, vc.H)
    sentinel = {"color": sent["float"], "prim": sent["prim"], "depth": sent["depth"]}
    composed = {k: rc.compose(good[k], sentinel[k], vc.AREA) for k in good}
    assert vc.frame_differences(good, good) == [] and vc.frame_differences(composed, good, vc.AREA, sentinel) == []
    x, y = vc.AREA[0] + 5, vc.AREA[1] + 7          # a covered pixel inside the area
    assert good["prim"][y, x] != NO_PRIM

    def planted(frame, key, edit):
        out = {k: v.copy() for k, v in frame.items()}
        edit(out[key])
        return out

    def one_ulp(c):
        c.view(np.uint32)[y, x, 1] += 1

    def one_id(p):
        p[y, x] += 1

    def one_depth_bit(d):
        d.view(np.uint32)[y, x] ^= 1

    for key, edit in (("color", one_ulp), ("prim", one_id), ("depth", one_depth_bit)):
        for frame, args in ((good, ()), (composed, (vc.AREA, sentinel))):
            diffs = vc.frame_differences(planted(frame, key, edit), good, *args)
            assert len(diffs) == 1 and diffs[0].startswith(f"{key}: 1 words differ"), diffs
    # one sentinel pixel overwritten outside the area, in each attachment
    ox, oy = vc.AREA[0] - 1, vc.AREA[1] + 3
    for key, edit in (("color", lambda c: c.__setitem__((oy, ox), good["color"][oy, ox])), ("prim", lambda p: p.__setitem__((oy, ox), good["prim"][oy, ox])),
                      ("depth", lambda d: d.__setitem__((oy, ox), np.float32(0.5)))):
        diffs = vc.frame_differences(planted(composed, key, edit), good, vc.AREA, sentinel)
        assert len(diffs) == 1 and "0 pixels inside the area, 1 sentinel pixels outside it" in diffs[0], diffs
    # a frame that ignores the area altogether, and a missing attachment
    assert len(vc.frame_differences(good, good, vc.AREA, sentinel)) == 3
    assert vc.frame_differences({"color": good["color"]}, good) == ["prim: missing", "depth: missing"]
    # the twin expectation keeps the depth where a primitive won and takes the other clear value elsewhere
    twin = vc.twin_expectation(good)
    won = good["prim"] != NO_PRIM
    assert np.array_equal(twin["depth"][won], good["depth"][won]) and np.all(twin["depth"][~won] == 0.0) and (~won).sum() > 100
