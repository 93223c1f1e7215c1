"""What a recording is, on the GPU (renderer-rs_amd/csrc/mirhi_api.hip, "command recording"; DESIGN.md "Plan cache").

(a) Every property of a recording is part of the plan's identity: a command buffer that records frame A twice keeps its plan (mirhi_debug_plan_builds
    stands still) and renders the same frame; recording B, which differs from A in ONE property, builds another plan, and the frame is, bit for bit,
    B recorded into a fresh command buffer.  A plan that survived such a change would not fail, it would draw the stale frame.
(b) A continued segment is the scope it continues: two draws of different depth states in one scope (the second draw cuts the scope into a second
    segment) render, bit for bit, what the same draws render as two scopes, the second with LOAD ops.

Frames are 64 x 64 (2 x 2 tiles: a cut or an area crosses a tile edge), cubes 8 x 8, depth arrays 32 x 32 x 2; one or two triangles (two quads for the
lit programs)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import multiview_cases as mc
import render_area_cases as rc

pytestmark = pytest.mark.gpu
W = H = 64
MV = 32                                  # a layer of the multiview rows' array
AREA = (10, 6, 40, 45)                   # off the tile grid on all four sides, in all four tiles
# two triangles in clip space (x, y, z, r, g, b): T0 in front (z 0.3), T1 behind it (z 0.6), overlapping in the middle of the frame
VERTS = np.array([[-0.8, -0.7, 0.3, 1.0, 0.2, 0.1], [0.7, -0.5, 0.3, 0.2, 1.0, 0.1], [-0.1, 0.8, 0.3, 0.1, 0.2, 1.0],
                  [-0.5, 0.6, 0.6, 0.9, 0.9, 0.1], [0.8, 0.1, 0.6, 0.1, 0.9, 0.9], [0.1, -0.8, 0.6, 0.9, 0.1, 0.9]], dtype=np.float32)
T0, T1 = 0, 3                            # first vertex of each


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


@dataclasses.dataclass
class Draw:
    first: int = T0
    compare: int = 1                     # CompareOp.Less
    scissor: tuple = (0, 0, W, H)


@dataclasses.dataclass
class Scope:
    """One colour scope of TRIANGLE draws as Kit.record_scope records it; None attachments are left out."""
    color: object = None
    clear_color: tuple = (0.1, 0.2, 0.3, 1.0)
    color_load: int = 1                  # LoadOp.CLEAR
    depth: object = None
    clear_depth: float = 1.0
    depth_load: int = 1
    depth_store: int = 0                 # StoreOp.STORE
    prim: object = None
    area: object = None
    resolve: bool = False                # a 4x scope that resolves into `color`
    draws: tuple = (Draw(T0), Draw(T1))


class Kit:
    """Attachments, the vertex buffer and pipelines shared by the rows; everything a row renders into is prefilled with sentinels before every submit."""

    def __init__(self, mirhi, scenes, dev):
        self.m, self.scenes, self.dev, self.objs, self.pipes = mirhi, scenes, dev, [], {}
        F = mirhi.Format
        self.color, self.color2 = (self.keep(mirhi.Image(dev, W, H, F.R32G32B32A32_SFLOAT)) for _ in range(2))
        self.depth = self.keep(mirhi.Image(dev, W, H, F.D32_SFLOAT))
        self.prim = self.keep(mirhi.Image(dev, W, H, F.R32_UINT))
        self.ms_color = self.keep(mirhi.Image.multisampled(dev, W, H, F.R32G32B32A32_SFLOAT, 4))
        self.vb = self.keep(mirhi.Buffer.new_with_data(dev, mirhi.BufferUsage.Vertex, VERTS))
        eye = np.eye(4, dtype=np.float32)
        self.mats = [mc.view_matrix(eye, v) for v in range(3)]
        self.cams = [self.keep(mirhi.Buffer.new_with_data(dev, mirhi.BufferUsage.Uniform, scenes.shadow_constants_ubo(m, eye))) for m in self.mats]
        self.sent = rc.sentinels(W, H)
        self.builds = C.CDLL(mirhi.LIB_PATH).mirhi_debug_plan_builds
        self.builds.restype = C.c_uint64

    def keep(self, obj):
        self.objs.append(obj)
        return obj

    def destroy(self):
        self.dev.wait_idle()
        for o in list(self.pipes.values()) + self.objs[::-1]:
            o.destroy()

    def pipe(self, compare, samples=1):
        m, key = self.m, ("triangle", compare, samples)
        if key not in self.pipes:
            self.pipes[key] = (m.GraphicsPipelineBuilder().vertex_shader(m.Program.TRIANGLE).fragment_shader(m.Program.TRIANGLE).vertex_binding(24)
                               .vertex_attributes(m.TRIANGLE_VERTEX_OFFSETS).color_attachment_format(m.Format.R32G32B32A32_SFLOAT)
                               .depth_attachment_format(m.Format.D32_SFLOAT).cull_mode(m.CullMode.NONE).depth_compare_op(compare)
                               .rasterization_samples(samples).build(self.dev))
        return self.pipes[key]

    def shadow_pipe(self, compare):
        m, key = self.m, ("shadow", compare)
        if key not in self.pipes:
            self.pipes[key] = (m.GraphicsPipelineBuilder().vertex_shader(m.Program.SHADOW).fragment_shader(m.Program.SHADOW).vertex_binding(24)
                               .vertex_attributes(m.SHADOW_VERTEX_OFFSETS).color_attachment_format(m.Format.UNDEFINED)
                               .depth_attachment_format(m.Format.D32_SFLOAT).cull_mode(m.CullMode.NONE).depth_compare_op(compare).build(self.dev))
        return self.pipes[key]

    def prefill(self):
        self.color.upload(self.sent["float"]); self.color2.upload(self.sent["float"])
        self.depth.upload(self.sent["depth"]); self.prim.upload(self.sent["prim"])

    def read(self):
        return [self.color.read(), self.color2.read(), self.depth.read(), self.prim.read()]

    def record_scope(self, cmd, s):
        if s.resolve:
            cmd.begin_rendering_resolve(self.ms_color, s.color, clear_color=s.clear_color)
        else:
            cmd.begin_rendering(s.color, clear_color=s.clear_color, color_load_op=s.color_load, depth=s.depth, clear_depth=s.clear_depth,
                                depth_load_op=s.depth_load, depth_store_op=s.depth_store, prim_id=s.prim, render_area=s.area)
        cmd.set_viewport(0.0, 0.0, float(W), float(H), 0.0, 1.0)
        cmd.bind_vertex_buffers(0, [self.vb], [0])
        for d in s.draws:
            cmd.set_scissor(*d.scissor)
            cmd.bind_pipeline(self.pipe(d.compare, 4 if s.resolve else 1))
            cmd.draw(3, 1, d.first, 0)
        cmd.end_rendering()

    def record_shadow_draws(self, cmd, size, draws, cam):
        """SHADOW draws (first vertex, compare op) of the two triangles into the depth-only scope that is open"""
        cmd.set_viewport(0.0, 0.0, float(size), float(size), 0.0, 1.0)
        cmd.set_scissor(0, 0, size, size)
        cmd.bind_vertex_buffers(0, [self.vb], [0])
        cmd.bind_uniform(self.m.Slot.CAMERA, cam)
        for first, compare in draws:
            cmd.bind_pipeline(self.shadow_pipe(compare))
            cmd.draw(3, 1, first, 0)

    def submit(self, cmd, record, prefill=None):
        """Prefills, records `record(cmd)` into the reusable command buffer, ends it; the plan builds counted so far; then submits and waits."""
        (prefill or self.prefill)()
        cmd.begin_reusable()
        record(cmd)
        cmd.end()
        n = self.builds()
        self.dev.submit([cmd])
        self.dev.wait_idle()
        return n

    def check_identity(self, rec_a, rec_b, read=None, prefill=None, rebuilds=1):
        """The three steps of (a): A, A again (the plan stands, the frame too), B (`rebuilds` more plans; the frame of a fresh command buffer)."""
        read = read or self.read
        cmd, fresh = self.m.CommandBuffer(self.dev), self.m.CommandBuffer(self.dev)
        try:
            self.submit(cmd, rec_a, prefill)
            first = self.builds()
            frame_a = read()
            assert self.submit(cmd, rec_a, prefill) == first, "recording A again built another plan"
            assert same(read(), frame_a), "recording A again changed the frame"
            assert self.submit(cmd, rec_b, prefill) == first + rebuilds, "plan builds after recording B"
            got = read()
            self.submit(fresh, rec_b, prefill)
            want = read()
            assert same(got, want), "B after A differs from B in a fresh command buffer"
            return frame_a, got
        finally:
            self.dev.wait_idle()
            cmd.destroy(); fresh.destroy()


@pytest.fixture(scope="module")
def kit(mirhi, scenes, device):
    k = Kit(mirhi, scenes, device)
    yield k
    k.destroy()


# ---- (a) the plan's identity --------------------------------------------------------------------------------------------------------------------
def _scope_rows(k):
    """name -> (A, B): scopes that differ in one property"""
    M = k.m
    LESS, LEQUAL, GREATER = M.CompareOp.Less, M.CompareOp.LessOrEqual, M.CompareOp.Greater
    full = Scope(color=k.color, depth=k.depth, prim=k.prim)
    bare = Scope(color=k.color, depth_store=M.StoreOp.DONT_CARE)
    two = dataclasses.replace(full, draws=(Draw(T0, LESS), Draw(T1, GREATER)))
    return {
        "clear_color": (full, dataclasses.replace(full, clear_color=(0.3, 0.2, 0.1, 0.5))),
        "clear_depth": (full, dataclasses.replace(full, clear_depth=0.5)),               # T1 (z 0.6) no longer passes
        "color_load_op": (full, dataclasses.replace(full, color_load=M.LoadOp.LOAD)),
        "depth_store_op": (full, dataclasses.replace(full, depth_store=M.StoreOp.DONT_CARE)),
        "render_area": (full, dataclasses.replace(full, area=AREA)),
        "depth_attachment": (dataclasses.replace(full, depth=None), full),
        "prim_id_image": (dataclasses.replace(full, prim=None), full),
        "resolve_scope": (bare, dataclasses.replace(bare, resolve=True)),
        "draw_scissor": (full, dataclasses.replace(full, draws=(Draw(T0), Draw(T1, scissor=(5, 5, 30, 40))))),
        "draw_compare_op": (dataclasses.replace(full, draws=(Draw(T0, LESS),)), dataclasses.replace(full, draws=(Draw(T0, GREATER),))),      # nothing passes
        "second_segment_state": (two, dataclasses.replace(two, draws=(Draw(T0, LESS), Draw(T1, LEQUAL)))),      # T1 shows beside T0, not on it
    }


SCOPE_ROWS = ["clear_color", "clear_depth", "color_load_op", "depth_store_op", "render_area", "depth_attachment", "prim_id_image", "resolve_scope",
              "draw_scissor", "draw_compare_op", "second_segment_state"]


@pytest.mark.parametrize("row", SCOPE_ROWS)
def test_a_changed_scope_property_builds_another_plan(kit, row):
    a, b = _scope_rows(kit)[row]
    frame_a, frame_b = kit.check_identity(lambda cmd: kit.record_scope(cmd, a), lambda cmd: kit.record_scope(cmd, b))
    assert not same(frame_a, frame_b), "the row's two frames are the same frame: it could not tell a stale plan"


def test_another_color_image_keeps_the_plan(kit):
    """The same frame into another colour image of the same extent and format (a swapchain that cycles): no plan is built, the frame lands in the new image."""
    a = Scope(color=kit.color, depth=kit.depth, prim=kit.prim)
    b = dataclasses.replace(a, color=kit.color2)
    frame_a, frame_b = kit.check_identity(lambda cmd: kit.record_scope(cmd, a), lambda cmd: kit.record_scope(cmd, b), rebuilds=0)
    assert same([frame_b[1]], [frame_a[0]]) and same([frame_b[0]], [kit.sent["float"]]) and same(frame_b[2:], frame_a[2:])


@pytest.mark.parametrize("row", ["view_mask", "view_offset"])
def test_a_changed_multiview_property_builds_another_plan(kit, row):
    m, dev = kit.m, kit.dev
    array = m.Image.array(dev, MV, MV, 2, m.Format.D32_SFLOAT)
    consts = m.Buffer.new_with_data(dev, m.BufferUsage.Uniform, mc.view_constants(kit.mats, 3, stride=80, offset=0))
    start = mc.sentinels(2, MV)
    mask_b, offset_b = (0b01, 0) if row == "view_mask" else (0b11, 80)

    def record(mask, offset):
        def rec(cmd):
            cmd.begin_rendering_multiview(array, mask, consts, offset, 80)
            kit.record_shadow_draws(cmd, MV, [(T0, m.CompareOp.Less), (T1, m.CompareOp.Less)], kit.cams[0])
            cmd.end_rendering()
        return rec
    try:
        frame_a, frame_b = kit.check_identity(record(0b11, 0), record(mask_b, offset_b), read=lambda: [array.read().copy()], prefill=lambda: array.upload(start))
        assert not same(frame_a, frame_b)
    finally:
        dev.wait_idle()
        consts.destroy(); array.destroy()


@pytest.mark.parametrize("row", ["ibl_lut", "ibl_prefiltered_seamless", "sky_environment"])
def test_a_changed_binding_builds_another_plan(kit, row):
    m, scenes, dev = kit.m, kit.scenes, kit.dev
    extra = []
    if row == "sky_environment":
        scene = scenes.skybox_case(W, H, 0, size=8, levels=4)
        res = m.SceneResources(dev, scene)
        other = dataclasses.replace(scene.sky, levels=[(0.5 * l).astype(np.float32) for l in scene.sky.levels]).create_image(dev, m.Image)
        extra, own = [other], res.sky_image

        def bind(b):
            res.sky_image = other if b else own
    else:
        scene = scenes.ibl_facets_case(W, H, lit=True, pre_size=8, pre_levels=4)
        scene = dataclasses.replace(scene, draws=scene.draws[:2])
        irr, pre, lut = extra = list(scene.ibl.create_images(dev, m.Image, m.Format.R32G32B32A32_SFLOAT))
        res = m.SceneResources(dev, scene, ibl_images=(irr, pre, lut))
        lut2 = m.Image(dev, lut.width, lut.height, m.Format.R32G32B32A32_SFLOAT)      # another image of the same size
        lut2.upload(np.ascontiguousarray(0.5 * scene.ibl.lut, dtype=np.float32))
        extra.append(lut2)

        def bind(b):
            if row == "ibl_lut":
                res.ibl_images = (irr, pre, lut2 if b else lut)
            else:
                pre.set_cube_seamless(bool(b))

    def record(b):
        def rec(cmd):
            bind(b)
            res.record_scopes(cmd)
        return rec
    try:
        frame_a, frame_b = kit.check_identity(record(False), record(True), read=lambda: [res.color.read()], prefill=lambda: None)
        if row != "ibl_prefiltered_seamless":      # (the two quads' lookups need not come near a face edge)
            assert not same(frame_a, frame_b)
    finally:
        kit.dev.wait_idle()
        bind(False)
        res.destroy()
        for o in extra:
            o.destroy()


# ---- (b) a continued segment is the scope it continues --------------------------------------------------------------------------------------------
def test_segments_under_a_partial_render_area(kit):
    M = kit.m
    one = Scope(color=kit.color, depth=kit.depth, area=AREA, draws=(Draw(T0, M.CompareOp.Less), Draw(T1, M.CompareOp.Greater)))
    first = dataclasses.replace(one, draws=one.draws[:1])
    second = dataclasses.replace(one, color_load=M.LoadOp.LOAD, depth_load=M.LoadOp.LOAD, draws=one.draws[1:])
    cmd = M.CommandBuffer(kit.dev)
    try:
        kit.submit(cmd, lambda c: kit.record_scope(c, one))
        got = kit.read()
        kit.submit(cmd, lambda c: kit.record_scope(c, first))
        only_first = kit.read()
        kit.submit(cmd, lambda c: (kit.record_scope(c, first), kit.record_scope(c, second)))
        want = kit.read()
    finally:
        kit.dev.wait_idle()
        cmd.destroy()
    assert same(got, want)
    assert not same(got, only_first), "the second draw shows nowhere"
    inside = rc.mask(AREA, W, H)
    assert same([got[0][~inside], got[2][~inside]], [kit.sent["float"][~inside], kit.sent["depth"][~inside]]), "written outside the area"


def test_segments_of_a_depth_only_scope(kit):
    M = kit.m
    S, L = M.StoreOp.STORE, M.LoadOp.LOAD
    draws = [(T0, M.CompareOp.Less), (T1, M.CompareOp.Greater)]

    def one(cmd):
        cmd.begin_rendering(None, depth=kit.depth, depth_store_op=S)
        kit.record_shadow_draws(cmd, W, draws, kit.cams[0])
        cmd.end_rendering()

    def two(cmd, n=2):
        for i in range(n):
            cmd.begin_rendering(None, depth=kit.depth, depth_store_op=S, depth_load_op=L if i else M.LoadOp.CLEAR)
            kit.record_shadow_draws(cmd, W, draws[i:i + 1], kit.cams[0])
            cmd.end_rendering()
    cmd = M.CommandBuffer(kit.dev)
    try:
        kit.submit(cmd, one)
        got = kit.depth.read()
        kit.submit(cmd, lambda c: two(c, 1))
        only_first = kit.depth.read()
        kit.submit(cmd, two)
        want = kit.depth.read()
    finally:
        kit.dev.wait_idle()
        cmd.destroy()
    assert same([got], [want])
    assert not same([got], [only_first]), "the second draw shows nowhere"


def test_segments_of_a_multiview_scope(kit):
    """mask 0b11: against the single-view scopes into the layer views, two per view (the second LOADs)"""
    m, dev = kit.m, kit.dev
    draws = [(T0, m.CompareOp.Less), (T1, m.CompareOp.Greater)]
    array = m.Image.array(dev, MV, MV, 2, m.Format.D32_SFLOAT)
    views = [array.layer_view(v) for v in range(2)]
    consts = m.Buffer.new_with_data(dev, m.BufferUsage.Uniform, mc.view_constants(kit.mats, 2, stride=80, offset=0))
    start = mc.sentinels(2, MV)

    def multi(cmd):
        cmd.begin_rendering_multiview(array, 0b11, consts, 0, 80)
        kit.record_shadow_draws(cmd, MV, draws, kit.cams[0])
        cmd.end_rendering()

    def single(cmd, n=2):
        for v in range(2):
            for i in range(n):
                cmd.begin_rendering(None, depth=views[v], depth_store_op=m.StoreOp.STORE, depth_load_op=m.LoadOp.LOAD if i else m.LoadOp.CLEAR)
                kit.record_shadow_draws(cmd, MV, draws[i:i + 1], kit.cams[v])
                cmd.end_rendering()
    cmd = m.CommandBuffer(dev)
    try:
        fill = lambda: array.upload(start)
        kit.submit(cmd, multi, fill)
        got = array.read().copy()
        kit.submit(cmd, lambda c: single(c, 1), fill)
        only_first = array.read().copy()
        kit.submit(cmd, single, fill)
        want = array.read().copy()
    finally:
        dev.wait_idle()
        cmd.destroy()
        for v in views:
            v.destroy()
        consts.destroy(); array.destroy()
    assert same([got], [want])
    assert all(not same([got[v]], [only_first[v]]) for v in range(2)), "the second draw shows nowhere"
    assert not same([got[0]], [got[1]])


@pytest.mark.parametrize("kind", ["model_pbr_ibl", "lit_then_skybox"])
def test_segments_of_lit_scopes(kit, kind):
    """Two MODEL_PBR_IBL quads of different depth states (LESS, LESS_OR_EQUAL); a lit scope whose last draw is the SKYBOX (always a segment of its own)."""
    m, scenes, dev = kit.m, kit.scenes, kit.dev
    L = m.LoadOp.LOAD
    base = scenes.ibl_facets_case(W, H, lit=True, pre_size=8, pre_levels=4)
    ibl = base.ibl.create_images(dev, m.Image, m.Format.R32G32B32A32_SFLOAT)
    if kind == "model_pbr_ibl":
        d0, d1 = base.draws[0], dataclasses.replace(base.draws[1], depth_compare=scenes.CMP_LESS_OR_EQUAL)
        whole = dataclasses.replace(base, draws=[d0, d1])
        parts = [dataclasses.replace(base, draws=[d0]), dataclasses.replace(base, draws=[d1])]
    else:
        sky = scenes.skybox_case(W, H, 0, size=8, levels=4).sky
        whole = dataclasses.replace(base, draws=base.draws[:2], sky=sky)
        parts = [dataclasses.replace(base, draws=base.draws[:2]), dataclasses.replace(base, draws=[], sky=sky)]
    sky_image = whole.sky.create_image(dev, m.Image) if whole.sky is not None else None
    F = m.Format
    images = [(m.Image(dev, W, H, F.R32G32B32A32_SFLOAT), m.Image(dev, W, H, F.D32_SFLOAT)) for _ in range(2)]
    made = []

    def render(scene, target, **kw):
        res = m.SceneResources(dev, scene, color_image=target[0], depth_image=target[1], ibl_images=ibl, sky_image=sky_image, **kw)
        made.append(res)
        res.render()
        dev.wait_idle()
    try:
        for c, d in images:
            c.upload(kit.sent["float"]); d.upload(kit.sent["depth"])
        render(whole, images[0])
        render(parts[0], images[1])
        only_first = [images[1][0].read(), images[1][1].read()]
        render(parts[1], images[1], color_load_op=L, depth_load_op=L)
        got, want = [images[0][0].read(), images[0][1].read()], [images[1][0].read(), images[1][1].read()]
    finally:
        dev.wait_idle()
        for res in made:
            res.destroy()
        for o in [i for pair in images for i in pair] + list(ibl) + ([sky_image] if sky_image is not None else []):
            o.destroy()
    assert same(got, want)
    assert not same(got, only_first), "the second segment shows nowhere"
