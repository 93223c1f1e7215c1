"""Render areas on the GPU (include/mirhi.h, mirhi_rendering_info::render_area) against the two equivalences of
tests/render_area_cases.py: E1 -- an area scope with CLEAR equals, inside the area, the full-extent CLEAR scope whose scissors are cut to the area
(itself checked against the oracle) and leaves every pixel outside as it was -- and E2 -- with LOAD it equals the full-extent LOAD scope with the
cut scissors over the same prior contents, everywhere.  Bit for bit on colour (both formats), primitive ids and stored depth: both sides run the
same arithmetic on the same absolute pixel coordinates.  Attachments are prefilled from the host with a per-pixel sentinel."""
import dataclasses
import os

import numpy as np
import pytest

import render_area_cases as rc
from test_gpu_parity import _check
from test_gpu_sparse_staging import _triangles, W as SW, H as SH

pytestmark = pytest.mark.gpu
FORMATS = ("float", "srgb8")


def _fmt(mirhi, key):
    return mirhi.Format.R32G32B32A32_SFLOAT if key == "float" else mirhi.Format.B8G8R8A8_SRGB


def render_into(mirhi, device, scene, key, prior, color_load=None, depth_load=None, depth=True, **kw):
    """One frame of `scene` into attachments that hold `prior` (dict: float / srgb8, depth, prim) before: what they hold afterwards."""
    L = mirhi.LoadOp
    w, h = scene.width, scene.height
    color = mirhi.Image(device, w, h, _fmt(mirhi, key))
    prim = mirhi.Image(device, w, h, mirhi.Format.R32_UINT)
    dimg = mirhi.Image(device, w, h, mirhi.Format.D32_SFLOAT) if depth else None
    color.upload(np.ascontiguousarray(prior[key]))
    prim.upload(np.ascontiguousarray(prior["prim"]))
    if dimg is not None:
        dimg.upload(np.ascontiguousarray(prior["depth"]))
    res = mirhi.SceneResources(device, scene, _fmt(mirhi, key), color_image=color, prim_image=prim, depth_image=dimg,
                               color_load_op=L.CLEAR if color_load is None else color_load, depth_load_op=L.CLEAR if depth_load is None else depth_load, **kw)
    try:
        res.render()
        out = res.read()
    finally:
        res.destroy()
        prim.destroy()
        if dimg is not None:
            dimg.destroy()
    return out


def assert_same(got, want, what, keys=("color", "prim", "depth")):
    for k in keys:
        if k in want:
            diff = got[k].view(np.uint32 if got[k].dtype != np.uint8 else np.uint8) != want[k].view(np.uint32 if want[k].dtype != np.uint8 else np.uint8)
            assert not diff.any(), f"{what}: {k} differs at {int(diff.sum())} places, first {np.argwhere(diff)[0]}"


def e1(mirhi, device, scene, area, key, sent, depth=True, **kw):
    """The area scope, and what E1 expects of it: (got, expected, the yardstick frame)."""
    got = render_into(mirhi, device, rc.in_area(scene, area), key, sent, depth=depth, **kw)
    yard = render_into(mirhi, device, rc.cut_to_area(scene, area), key, sent, depth=depth, **kw)
    want = {"color": rc.compose(yard["color"], sent[key], area), "prim": rc.compose(yard["prim"], sent["prim"], area)}
    if depth:
        want["depth"] = rc.compose(yard["depth"], sent["depth"], area)
    return got, want, yard


def area_b(scene):
    return rc.areas(scene.width, scene.height)["b_unaligned"]


@pytest.fixture(scope="module")
def sent_for():
    cache = {}

    def get(scene):
        k = (scene.width, scene.height)
        if k not in cache:
            cache[k] = rc.sentinels(*k)
        return cache[k]
    return get


@pytest.fixture(scope="module")
def oracle_frames(oracle, scenes):
    """oracle(scene with the scissors cut to the area), once per (case, area): both colour formats compare with it."""
    cache = {}

    def get(case, name):
        if (case, name) not in cache:
            scene = scenes.SMALL_CASES[case]()
            cache[(case, name)] = oracle.render(rc.cut_to_area(scene, rc.areas(scene.width, scene.height)[name]), want_bgra8=True)
        return cache[(case, name)]
    return get


# 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", FORMATS)
@pytest.mark.parametrize("name", ["a_aligned", "b_unaligned", "c_in_one_tile", "d_corner_2x2", "e_one_pixel", "f_column", "g_bottom_right", "h_full"])
@pytest.mark.parametrize("case", ["random_small", "multi_draw", "sphere_small"])
def test_e1_clear_scope_over_the_areas(mirhi, device, scenes, oracle_frames, sent_for, case, name, key):
    scene = scenes.SMALL_CASES[case]()
    area = rc.areas(scene.width, scene.height)[name]
    sent = sent_for(scene)
    got, want, yard = e1(mirhi, device, scene, area, key, sent)
    _check(yard, oracle_frames(case, name), f"{case} cut to {name}", depth=any(d.depth_test for d in scene.draws))      # the yardstick against the oracle
    assert_same(got, want, f"{case} in {name} {area}")
    if name == "h_full":        # the explicit full extent is the scope without an area, bit for bit
        plain = render_into(mirhi, device, scene, key, sent)
        assert_same(got, plain, f"{case}: explicit full extent against render_area = 0")


def test_e1_partial_edge_tile_of_a_ragged_extent(mirhi, device, scenes, sent_for):
    """(g) where neither extent is a multiple of 32: the area ends in the attachment's own partial tile column and row."""
    scene = scenes.random_triangles(300, 333, 211, seed=43, rmin=2, rmax=40)
    area = rc.areas(333, 211)["g_bottom_right"]
    assert (area[0] + area[2], area[1] + area[3]) == (333, 211) and 333 % 32 and 211 % 32
    for key in FORMATS:
        got, want, yard = e1(mirhi, device, scene, area, key, sent_for(scene))
        assert (yard["prim"][rc.mask(area, 333, 211)] != rc.NO_PRIM).any()
        assert_same(got, want, f"ragged g {key}")


# 2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", FORMATS)
@pytest.mark.parametrize("transient_depth", [False, True])
def test_e2_load_scope_over_a_full_extent_frame(mirhi, device, scenes, sent_for, key, transient_depth):
    """Frame A full-extent; then scene B into area (b) with colour LOAD and depth LOAD + STORE -- or with a transient depth (no image, CLEAR)."""
    L = mirhi.LoadOp
    a = scenes.random_triangles(300, 320, 200, seed=42, rmin=2, rmax=40)
    b = scenes.random_triangles(200, 320, 200, seed=77, rmin=4, rmax=30)
    area = area_b(b)
    frame_a = render_into(mirhi, device, a, key, sent_for(a))
    prior = {key: frame_a["color"], "prim": frame_a["prim"], "depth": frame_a["depth"]}
    kw = dict(color_load=L.LOAD, depth_load=L.CLEAR if transient_depth else L.LOAD, depth=not transient_depth)
    got = render_into(mirhi, device, rc.in_area(b, area), key, prior, **kw)
    want = render_into(mirhi, device, rc.cut_to_area(b, area), key, prior, **kw)
    assert_same(got, want, "E2")
    m = rc.mask(area, 320, 200)
    assert (got["prim"][m] != frame_a["prim"][m]).any()                      # B shows inside ...
    assert_same({k: v[~m] for k, v in got.items()}, {k: v[~m] for k, v in frame_a.items() if k in got}, "E2 outside the area")      # ... and A is intact outside


# 3 ---------------------------------------------------------------------------------------------------------------------------------------
def _greater(scene):
    draws = [dataclasses.replace(d, depth_compare=6) for d in scene.draws]      # GREATER_OR_EQUAL: the flipped key
    return dataclasses.replace(scene, draws=draws, clear_depth=0.0)


def _predicate(scene):
    draws = [dataclasses.replace(d, depth_compare=3, depth_write=False) for d in scene.draws]      # LESS_OR_EQUAL without write: a predicate key
    return dataclasses.replace(scene, draws=draws, clear_depth=0.6)


def _blend_behind_opaque(scenes):
    s = scenes.random_triangles(120, 320, 200, seed=5, rmin=6, rmax=40)
    t = scenes.random_triangles(60, 320, 200, seed=6, rmin=10, rmax=50).draws[0]
    t = dataclasses.replace(t, depth_write=False, blend=scenes.ALPHA_BLEND)
    return dataclasses.replace(s, draws=[s.draws[0], t], name="opaque-then-blended")


ROUTES = {
    # name: (scene builder, environment, SceneResources keywords)
    "sparse": (lambda sc: sc.SMALL_CASES["random_small"](), {"MIRHI_TP_DENSITY": "1000000"}, {}),
    "dense": (lambda sc: sc.SMALL_CASES["random_small"](), {"MIRHI_TP_DENSITY": "0"}, {}),
    "dense_mesh": (lambda sc: sc.SMALL_CASES["sphere_small"](), {"MIRHI_TP_DENSITY": "0", "MIRHI_RASTER_TEAMS": "1"}, {}),
    "two_teams": (lambda sc: sc.SMALL_CASES["sphere_small"](), {"MIRHI_TP_DENSITY": "0", "MIRHI_RASTER_TEAMS": "2"}, {}),
    "two_teams_one_list": (lambda sc: sc.SMALL_CASES["sphere_small"](), {"MIRHI_TP_DENSITY": "0", "MIRHI_RASTER_TEAMS": "2", "MIRHI_XCD_BINS": "0"}, {}),
    "wide8": (lambda sc: sc.SMALL_CASES["sphere_small"](), {"MIRHI_TP_DENSITY": "0", "MIRHI_RASTER_WIDE": "8"}, {}),
    "wide16": (lambda sc: sc.SMALL_CASES["sphere_small"](), {"MIRHI_TP_DENSITY": "0", "MIRHI_RASTER_WIDE": "16"}, {}),
    "masked": (lambda sc: sc.SMALL_CASES["alpha_mask"](), {}, {}),
    "masked_ordered": (lambda sc: sc.SMALL_CASES["alpha_mask"](), {"MIRHI_MASKED_ORDERED": "1"}, {}),
    "blend_behind_opaque": (_blend_behind_opaque, {}, {}),
    "pbr": (lambda sc: sc.SMALL_CASES["pbr"](), {}, {}),
    "textured": (lambda sc: sc.SMALL_CASES["textured"](), {}, {}),
    "pbr_shadow_map": (lambda sc: sc.shadowed_ground_case(320, 240, 128), {}, {}),
    "pbr_cascades": (lambda sc: sc.cascaded_ground_case(320, 240, 128), {}, {}),
    "pbr_ibl": (lambda sc: sc.ibl_facets_case(128, 96, lit=True), {}, {}),
    "sky_behind_geometry": (lambda sc: dataclasses.replace(sc.ibl_facets_case(128, 96), sky=sc.skybox_case(128, 96, 0).sky), {}, {}),
    "sky_alone": (lambda sc: sc.skybox_case(128, 96, 1), {}, {}),
    "greater_key": (lambda sc: _greater(sc.SMALL_CASES["random_small"]()), {}, {}),
    "greater_key_mesh": (lambda sc: _greater(sc.SMALL_CASES["sphere_small"]()), {"MIRHI_TP_DENSITY": "0"}, {}),
    "predicate_key": (lambda sc: _predicate(sc.SMALL_CASES["random_small"]()), {}, {}),
    "xcd_run_knob": (lambda sc: sc.SMALL_CASES["random_small"](), {"MIRHI_XCD_RUN": "4"}, {}),
}


@pytest.mark.parametrize("key", FORMATS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_routes_in_an_unaligned_area(mirhi, device, scenes, sent_for, monkeypatch, route, key):
    build, env, kw = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene = build(scenes)
    area = area_b(scene)
    got, want, yard = e1(mirhi, device, scene, area, key, sent_for(scene), **kw)
    m = rc.mask(area, scene.width, scene.height)
    assert (yard["prim"][m] != rc.NO_PRIM).any()
    assert_same(got, want, f"{route} {key}")


@pytest.mark.parametrize("n", [63, 64, 65])
def test_record_counts_in_a_partial_tile(mirhi, device, scenes, sent_for, n):
    """n bin records in tile (14, 6) of a 500 x 250 frame, which area (b) cuts at x = 477: the sparse variants' split bin pass around its 64-lane group."""
    scene = scenes.Scene(f"area-records-{n}", SW, SH, [_triangles(scenes, n, (460, 208), 3.0, 900 + n)], clear_color=(0.2, 0.3, 0.1, 1.0))
    area = area_b(scene)
    assert area[0] + area[2] == 477 and 448 < 477 < 480
    got, want, yard = e1(mirhi, device, scene, area, "float", sent_for(scene))
    ys, xs = np.nonzero(yard["prim"] != rc.NO_PRIM)
    assert xs.min() >= 448 and xs.max() < 477 and ys.min() >= 192 and ys.max() < 224          # all in that tile, uncut: bin records
    assert_same(got, want, f"{n} records")


def test_depth_only_shadow_scope_in_an_area(mirhi, device, scenes):
    """A SHADOW scope into area (b) of a 160 x 160 D32 image: E1 on the depth image alone."""
    base = scenes.shadowed_ground_case(96, 96, 160)
    area = rc.areas(160, 160)["b_unaligned"]
    sent = rc.sentinels(160, 160)["depth"]
    frames = {}
    for name in ("area", "yard"):
        sh = base.shadow
        casters = sh.casters if name == "area" else [dataclasses.replace(c, scissor=rc.intersect(c.scissor, area, 160, 160)) for c in sh.casters]
        spec = dataclasses.replace(sh, casters=casters, render_area=area if name == "area" else None)
        smap = mirhi.Image(device, 160, 160, mirhi.Format.D32_SFLOAT)
        smap.upload(sent)
        res = mirhi.SceneResources(device, dataclasses.replace(base, shadow=spec), shadow_map=smap)
        res.render()
        device.wait_idle()
        frames[name] = smap.read()
        res.destroy(); smap.destroy()
    m = rc.mask(area, 160, 160)
    assert (frames["yard"][m] != np.float32(1.0)).any()
    assert rc.same_bits(frames["area"], rc.compose(frames["yard"], sent, area))


def test_fragment_statistics_equal_the_yardsticks(mirhi, device, scenes):
    scene = scenes.SMALL_CASES["random_small"]()
    area = area_b(scene)
    counts = []
    for s in (rc.in_area(scene, area), rc.cut_to_area(scene, area)):
        res = mirhi.SceneResources(device, s, want_prim=True, want_depth=True)
        device.wait_idle()
        device.reset_kernel_times()
        device.set_profiling(mirhi.Profile.FRAGMENTS)
        try:
            res.render()
            device.wait_idle()
        finally:
            device.set_profiling(0)
        counts.append(device.fragment_stats())
        res.destroy()
    assert counts[0] == counts[1] and counts[0][0] > 0 and counts[0][1] >= counts[0][0], counts


# 4 ---------------------------------------------------------------------------------------------------------------------------------------
def test_shadow_atlas_of_four_quadrants(mirhi, device, scenes):
    """Four SHADOW scopes, each CLEAR, into the four 64 x 64 quadrants of one 128 x 128 D32 image, each with a viewport equal to its quadrant:
    the composite of the four E1 yardsticks -- no scope disturbs another's quadrant."""
    bases = [scenes.shadowed_ground_case(96, 96, 64, light_dir=d) for d in ((-0.4, -1.0, -0.3), (0.5, -1.0, 0.2), (0.1, -1.0, 0.6), (-0.6, -1.0, 0.4))]
    quads = [(0, 0, 64, 64), (64, 0, 64, 64), (0, 64, 64, 64), (64, 64, 64, 64)]
    sent = rc.sentinels(128, 128, seed=4)["depth"]

    def spec_for(i, with_area):
        q = quads[i]
        vp = (float(q[0]), float(q[1]), 64.0, 64.0, 0.0, 1.0)
        casters = [dataclasses.replace(c, viewport=vp, scissor=None if with_area else q) for c in bases[i].shadow.casters]
        return dataclasses.replace(bases[i].shadow, casters=casters, size=(128, 128), render_area=q if with_area else None)

    atlas = mirhi.Image(device, 128, 128, mirhi.Format.D32_SFLOAT)
    atlas.upload(sent)
    for i in range(4):
        res = mirhi.SceneResources(device, dataclasses.replace(bases[i], shadow=spec_for(i, True)), shadow_map=atlas)
        res.render()
        device.wait_idle()
        res.destroy()
    got = atlas.read()
    want = sent.copy()
    for i in range(4):
        atlas.upload(sent)
        res = mirhi.SceneResources(device, dataclasses.replace(bases[i], shadow=spec_for(i, False)), shadow_map=atlas)
        res.render()
        device.wait_idle()
        res.destroy()
        yard = atlas.read()
        assert (yard[rc.mask(quads[i], 128, 128)] != np.float32(1.0)).any()
        want = rc.compose(yard, want, quads[i])
    atlas.destroy()
    assert rc.same_bits(got, want)
    assert not (got == sent).any()          # every pixel of the atlas belongs to a quadrant and was cleared or drawn


def test_a_quadrant_of_the_atlas_read_as_a_shadow_map(mirhi, device, scenes, oracle):
    """An area scope writes one 64 x 64 quadrant of a 128 x 128 D32 atlas (flat casters at depth 0.25 over the clear value 1: a two-valued map, as in
    test_gpu_shadow.py's PCF test); copy_image moves the quadrant into a map of its own, and a MODEL_PBR draw that samples it gives
    unlit + s (lit - unlit) with s the numpy PCF factor (scenes.pcf_factor) of the map read back -- the model and the bound of that test."""
    from test_gpu_shadow import _pattern_scene, assert_close
    m, size, strength = 64, 128, 1.0
    quad = (64, 0, 64, 64)
    tris = scenes.random_triangles(40, m, m, seed=21, rmin=3, rmax=12).draws[0]
    verts = np.array(np.ascontiguousarray(tris.vertices, dtype=np.float32).reshape(-1, 6))
    verts[:, 2] = 0.25
    eye = np.eye(4, dtype=np.float32)
    caster = scenes.DrawSpec(vertices=verts, stride=24, count=tris.count, program=scenes.PROGRAM_SHADOW, cull_mode=scenes.CULL_NONE,
                             camera=scenes.shadow_constants_ubo(eye, eye), viewport=(64.0, 0.0, 64.0, 64.0, 0.0, 1.0))
    sent = rc.sentinels(128, 128, seed=6)["depth"]
    atlas = mirhi.Image(device, 128, 128, mirhi.Format.D32_SFLOAT)
    smap = mirhi.Image(device, m, m, mirhi.Format.D32_SFLOAT)
    atlas.upload(sent)
    spec = scenes.ShadowSpec([caster], (128, 128), scenes.shadow_ubo(eye, size=(128, 128)), render_area=quad)
    res = mirhi.SceneResources(device, scenes.Scene("atlas-writer", 64, 64, [], shadow=spec), shadow_map=atlas)
    res.render()
    device.wait_idle()
    res.destroy()
    cmd = mirhi.CommandBuffer(device)
    cmd.begin()
    cmd.copy_image(atlas, smap, [(0, (quad[0], quad[1]), 0, (0, 0), (m, m))])
    cmd.end()
    device.submit([cmd])
    device.wait_idle()
    cmd.destroy()
    after = atlas.read()
    pattern = smap.read().reshape(m, m).copy()
    inside = rc.mask(quad, 128, 128)
    assert np.array_equal(after[~inside], sent[~inside]) and np.array_equal(after[inside].reshape(m, m), pattern)
    assert set(np.unique(pattern)) == {np.float32(0.25), np.float32(1.0)} and 0.05 < (pattern == np.float32(0.25)).mean() < 0.95
    scene = _pattern_scene(scenes, size, strength)
    res = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT, shadow_map=smap)      # (its shadow scope: LOAD, no draws -- the map stays)
    res.render()
    out = res.read()["color"]
    res.destroy(); smap.destroy(); atlas.destroy()
    lit = oracle.render(_pattern_scene(scenes, size, strength, shadow=False), want_bgra8=False)["rgba"]
    unlit = oracle.render(_pattern_scene(scenes, size, strength, intensity=0.0, shadow=False), want_bgra8=False)["rgba"]
    px, py = np.meshgrid(np.arange(size), np.arange(size), indexing="xy")
    u, v = (px + 0.5) / size, 1.0 - (py + 0.5) / size
    ls = scenes.light_space_matrix((0.0, -1.0, 0.0), half_extent=2.0, near=0.1, far=20.0)
    plane_depth = float((ls.T.astype(np.float64) @ np.array([0.0, 0.0, 0.0, 1.0]))[2])
    assert 0.25 < plane_depth - 0.0005 < 1.0
    s_ = scenes.pcf_factor(pattern, u, v, np.full(u.shape, plane_depth - 0.0005), strength=strength)
    assert (s_ < 1.0).mean() > 0.05 and (s_ > 0.0).mean() > 0.05          # the quadrant's casters shade the frame, partly
    assert_close(out, unlit[..., :3] + s_[..., None] * (lit[..., :3] - unlit[..., :3]), "PBR over a quadrant of the atlas")


# 5 ---------------------------------------------------------------------------------------------------------------------------------------
def _frame_sequence(scene):
    ar = rc.areas(scene.width, scene.height)
    return [ar["b_unaligned"], None, ar["c_in_one_tile"], ar["a_aligned"], None, ar["g_bottom_right"], ar["f_column"]]


def test_rerecorded_command_buffer_whose_area_changes_every_frame(mirhi, device, scenes, monkeypatch):
    """Two frames in flight under MIRHI_VERIFY_IDLE: every frame re-records with another area (a full-extent frame between area frames) into
    attachments that keep their contents -- colour and depth LOAD -- so a stale plan would show as a wrong rectangle."""
    monkeypatch.setenv("MIRHI_VERIFY_IDLE", "1")
    L = mirhi.LoadOp
    scene = scenes.SMALL_CASES["random_small"]()
    seq = _frame_sequence(scene)
    sent = rc.sentinels(scene.width, scene.height, seed=9)
    # what each step must leave: E2, chained from the sentinel
    want, prior = [], {"float": sent["float"], "prim": sent["prim"], "depth": sent["depth"]}
    for area in seq:
        s = rc.cut_to_area(scene, area) if area else scene
        out = render_into(mirhi, device, s, "float", prior, color_load=L.LOAD, depth_load=L.LOAD)
        want.append(out)
        prior = {"float": out["color"], "prim": out["prim"], "depth": out["depth"]}
    frames, fences, images = [], [], []
    for _ in range(2):
        color = mirhi.Image(device, scene.width, scene.height, mirhi.Format.R32G32B32A32_SFLOAT)
        prim = mirhi.Image(device, scene.width, scene.height, mirhi.Format.R32_UINT)
        dimg = mirhi.Image(device, scene.width, scene.height, mirhi.Format.D32_SFLOAT)
        color.upload(sent["float"]); prim.upload(sent["prim"]); dimg.upload(sent["depth"])
        frames.append(mirhi.SceneResources(device, scene, color_image=color, prim_image=prim, depth_image=dimg, color_load_op=L.LOAD, depth_load_op=L.LOAD))
        fences.append(mirhi.Fence(device))
        images += [prim, dimg]
    try:
        for step, area in enumerate(seq):
            for res, fence in zip(frames, fences):
                res.scene = rc.in_area(scene, area) if area else scene
                res.record()
                res.render(fence)
            for res, fence in zip(frames, fences):
                fence.wait(); fence.reset()
                assert_same(res.read(), want[step], f"step {step} area {area}")
    finally:
        device.wait_idle()
        for res, fence in zip(frames, fences):
            res.destroy(); fence.destroy()
        for im in images:
            im.destroy()


@pytest.mark.skipif(os.environ.get("MIRHI_NATIVE_DISPATCH") == "0", reason="native dispatch switched off for this run")
def test_both_dispatch_paths(mirhi, scenes):
    scene = scenes.SMALL_CASES["sphere_small"]()
    area = area_b(scene)
    sent = rc.sentinels(scene.width, scene.height)
    dev = mirhi.Device(0, stream=0)
    outs, used = [], []
    try:
        want = e1(mirhi, dev, scene, area, "float", sent)[1]
        for native in (False, True):
            dev.set_native_dispatch(native)
            before = dev.stats().native_dispatches
            outs.append(render_into(mirhi, dev, rc.in_area(scene, area), "float", sent))
            used.append((dev.dispatch_path(), dev.stats().native_dispatches - before))
    finally:
        dev.destroy()
    assert used[0][1] == 0 and used[1][1] > 0 and used[1][0].startswith("native:"), used
    for out in outs:
        assert_same(out, want, "dispatch path")


def test_a_submit_of_several_area_command_buffers(mirhi, device, scenes):
    """One mirhi_queue_submit of four command buffers -- two area scopes, a full-extent one, another area scope; each clears its own attachments:
    the shape a batched submit takes when its scopes are alike.  An area scope keeps out of a batch (mirhi_submit.h); the frames must be right."""
    scene = scenes.SMALL_CASES["random_small"]()
    ar = rc.areas(scene.width, scene.height)
    seq = [ar["b_unaligned"], ar["a_aligned"], None, ar["b_unaligned"]]
    sent = rc.sentinels(scene.width, scene.height, seed=3)
    want = [e1(mirhi, device, scene, a, "srgb8", sent, depth=False)[1] if a else render_into(mirhi, device, scene, "srgb8", sent, depth=False) for a in seq]
    slots, images = [], []
    for a in seq:
        color = mirhi.Image(device, scene.width, scene.height, mirhi.Format.B8G8R8A8_SRGB)
        prim = mirhi.Image(device, scene.width, scene.height, mirhi.Format.R32_UINT)
        color.upload(sent["srgb8"]); prim.upload(sent["prim"])
        res = mirhi.SceneResources(device, rc.in_area(scene, a) if a else scene, mirhi.Format.B8G8R8A8_SRGB, color_image=color, prim_image=prim)
        res.record()
        slots.append(res); images.append(prim)
    try:
        fence = mirhi.Fence(device)
        device.submit([r.cmd for r in slots], fence)
        fence.wait()
        for i, res in enumerate(slots):
            assert_same(res.read(), want[i], f"command buffer {i} of the submit", keys=("color", "prim"))
        fence.destroy()
    finally:
        device.wait_idle()
        for res in slots:
            res.destroy()
        for im in images:
            im.destroy()


# 6 ---------------------------------------------------------------------------------------------------------------------------------------
def _begin(mirhi, device, area, depth_only=False, w=320, h=200):
    color = None if depth_only else mirhi.Image(device, w, h, mirhi.Format.B8G8R8A8_SRGB)
    depth = mirhi.Image(device, w, h, mirhi.Format.D32_SFLOAT)
    cmd = mirhi.CommandBuffer(device)
    try:
        cmd.begin()
        cmd.begin_rendering(color, depth=depth, depth_store_op=mirhi.StoreOp.STORE, render_area=area)
        cmd.end_rendering()
        cmd.end()
    finally:
        cmd.destroy()
        depth.destroy()
        if color is not None:
            color.destroy()


@pytest.mark.parametrize("depth_only", [False, True])
def test_refusals_and_acceptance(mirhi, device, depth_only):
    for area in ((-1, 0, 10, 10), (0, -3, 10, 10), (300, 0, 21, 10), (0, 190, 10, 11), (2147483647, 0, 2147483647, 10)):
        with pytest.raises(mirhi.RhiError) as e:
            _begin(mirhi, device, area, depth_only)
        msg = str(e.value)
        assert "render area" in msg and all(str(v) in msg for v in area) and "320" in msg and "200" in msg, msg
    for area in ((19, 13, 278, 170), (0, 0, 320, 200), (319, 199, 1, 1), (5, 5, 0, 0)):      # a valid partial area is no longer refused
        _begin(mirhi, device, area, depth_only)


def test_partial_area_on_a_split_device_is_refused(mirhi, device):
    try:
        device.set_tile_split(0, 2, "bands")
        with pytest.raises(mirhi.RhiError, match="unsupported: a partial render area on a split device"):
            _begin(mirhi, device, (19, 13, 278, 170))
        _begin(mirhi, device, (0, 0, 320, 200))          # the full extent is what a split device renders
    finally:
        device.set_tile_split(0, 1, "interleaved")
