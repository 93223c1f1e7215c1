"""Shadow mapping on the GPU: the depth-only SHADOW pass (vertex/shadow.hlsl + pixel/shadow.hlsl) against the oracle's MODEL depth,
CalculateShadow's 3x3 PCF (shadow.hlsli:49-121) in the MODEL_PBR resolve against a numpy model, the ordering of a shadow scope and the
scope that samples its map, the tile split and the record-time refusals (include/mirhi.h MIRHI_PROGRAM_SHADOW, MIRHI_TEXTURE_SHADOW_MAP)."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4          # the PBR parity tests' bound (test_gpu_parity.py)


def assert_close(out_rgba, ref_rgba, name, mask=None):
    a, b = out_rgba[..., :3].astype(np.float64), ref_rgba[..., :3].astype(np.float64)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    if mask is not None:
        err = err[mask]
    worst = float(err.max()) if err.size else 0.0
    assert worst < RGB_TOL, f"{name}: max |dRGB| = {worst}"


# ---- casters: a sphere and a box, drawn with SHADOW into a map and with MODEL through the oracle ---------------------------
def _casters(scenes):
    sphere = scenes.displaced_sphere(24, 17, 64, 64, seed=5).draws[0]
    bv, bi = scenes._box_mesh((0.8, 0.2, -0.3), (0.5, 0.9, 0.4))
    ls = scenes.light_space_matrix((0.3, -1.0, 0.2), half_extent=2.5)
    m_sphere = scenes.trs((0.9, 0.9, 0.9), (0.0, 0.0, 0.0, 1.0), (-0.6, 0.4, 0.2))
    return ls, [(np.ascontiguousarray(sphere.vertices, dtype=np.float32).reshape(-1, 12), sphere.indices, m_sphere),
                (bv.astype(np.float32), bi, np.eye(4, dtype=np.float32))]


def _camera_from(scenes, vp, eye=(0.0, 10.0, 0.0)):
    """CameraData 208 B whose viewProjection (@128) is vp: what a MODEL draw needs to put its depth where a SHADOW draw does."""
    z = np.zeros((4, 4), dtype=np.float32)
    return z.tobytes() + z.tobytes() + vp.astype(np.float32).tobytes() + np.array([*eye, 0.0], dtype=np.float32).tobytes()


def _oracle_depth(scenes, oracle, ls, casters, size, compare, clear, cull):
    draws = [scenes.DrawSpec(vertices=v, stride=48, count=i.size, indices=i, program=scenes.PROGRAM_MODEL, cull_mode=cull,
                             depth_compare=compare, camera=_camera_from(scenes, ls), object=scenes.object_ubo(m))
             for v, i, m in casters]
    ref = oracle.render(scenes.Scene("shadow-ref", size, size, draws, clear_depth=clear), want_bgra8=False)
    return ref["depth"], ref["prim"] != 0xFFFFFFFF


def _render_map(mirhi, scenes, dev, ls, casters, size, compare, clear, cull, stride=48, load_map=None):
    objs = []
    img = mirhi.Image(dev, size, size, mirhi.Format.D32_SFLOAT)
    if load_map is not None:
        img.upload(load_map)
    pipe = (mirhi.GraphicsPipelineBuilder().vertex_shader(mirhi.Program.SHADOW).fragment_shader(mirhi.Program.SHADOW)
            .vertex_binding(stride).vertex_attributes(mirhi.SHADOW_VERTEX_OFFSETS)
            .color_attachment_format(mirhi.Format.UNDEFINED).depth_attachment_format(mirhi.Format.D32_SFLOAT)
            .cull_mode(cull).depth_compare_op(compare).build(dev))
    cmd = mirhi.CommandBuffer(dev)
    cmd.begin()
    cmd.begin_rendering(None, depth=img, clear_depth=clear, depth_store_op=mirhi.StoreOp.STORE,
                        depth_load_op=mirhi.LoadOp.LOAD if load_map is not None else mirhi.LoadOp.CLEAR)
    cmd.set_viewport(0.0, 0.0, float(size), float(size))
    cmd.set_scissor(0, 0, size, size)
    cmd.bind_pipeline(pipe)
    for v, i, m in casters:
        verts = v if stride == 48 else np.ascontiguousarray(v[:, 0:3])
        vb = mirhi.Buffer.new_with_data(dev, mirhi.BufferUsage.Vertex, verts)
        ib = mirhi.Buffer.new_with_data(dev, mirhi.BufferUsage.Index, i.astype(np.uint32))
        ub = mirhi.Buffer.new_with_data(dev, mirhi.BufferUsage.Uniform, np.frombuffer(scenes.shadow_constants_ubo(ls, m), dtype=np.uint8))
        objs += [vb, ib, ub]
        cmd.bind_vertex_buffers(0, [vb], [0])
        cmd.bind_index_buffer(ib, 0, mirhi.IndexType.UINT32)
        cmd.bind_uniform(mirhi.Slot.CAMERA, ub)
        cmd.draw_indexed(int(i.size))
    cmd.end_rendering()
    cmd.end()
    dev.submit([cmd])
    dev.wait_idle()
    out = img.read().reshape(size, size).copy()
    cmd.destroy(); pipe.destroy(); img.destroy()
    for o in objs:
        o.destroy()
    return out


DEPTH_CASES = {   # compare op, clear value, cull mode, vertex stride
    "less-48": ("CMP_LESS", 1.0, "CULL_NONE", 48),
    "less-12": ("CMP_LESS", 1.0, "CULL_NONE", 12),
    "lequal-48": ("CMP_LESS_OR_EQUAL", 1.0, "CULL_NONE", 48),
    "greater-48": ("CMP_GREATER", 0.0, "CULL_NONE", 48),
    "gequal-12": ("CMP_GREATER_OR_EQUAL", 0.0, "CULL_NONE", 12),
    "cull-front-48": ("CMP_LESS", 1.0, "CULL_FRONT", 48),
}


@pytest.mark.parametrize("case", list(DEPTH_CASES))
def test_depth_only_pass_matches_the_oracle_model_depth(mirhi, scenes, oracle, device, case):
    """A SHADOW draw and a MODEL draw with viewProjection = lightSpaceMatrix give the same depth bits; uncovered texels hold the clear value."""
    cmp_name, clear, cull_name, stride = DEPTH_CASES[case]
    compare, cull = getattr(scenes, cmp_name), getattr(scenes, cull_name)
    ls, casters = _casters(scenes)
    size = 160
    ref, covered = _oracle_depth(scenes, oracle, ls, casters, size, compare, clear, cull)
    out = _render_map(mirhi, scenes, device, ls, casters, size, compare, clear, cull, stride=stride)
    assert covered.sum() > 2000
    assert np.array_equal(out.view(np.uint32)[covered], ref.view(np.uint32)[covered]), f"{case}: depth bits differ"
    assert np.all(out[~covered] == np.float32(clear)), f"{case}: uncovered texels do not hold the clear value"


def test_depth_only_load_scope_and_hip_launch_path(mirhi, scenes, oracle, device):
    """LOAD: the scope starts from the image's depth (texels no caster reaches keep it); the HIP launch path (a timed submit) stores the
    same bits as the native one; one 2048 x 2048 map."""
    ls, casters = _casters(scenes)
    size = 2048
    ref, covered = _oracle_depth(scenes, oracle, ls, casters, size, scenes.CMP_LESS, 1.0, scenes.CULL_NONE)
    native = _render_map(mirhi, scenes, device, ls, casters, size, scenes.CMP_LESS, 1.0, scenes.CULL_NONE)
    assert np.array_equal(native.view(np.uint32)[covered], ref.view(np.uint32)[covered])
    device.set_profiling(mirhi.Profile.TIMING)           # timed dispatches go out as HIP launches
    try:
        hip = _render_map(mirhi, scenes, device, ls, casters, size, scenes.CMP_LESS, 1.0, scenes.CULL_NONE)
    finally:
        device.set_profiling(0)
        device.reset_kernel_times()
    assert np.array_equal(hip.view(np.uint32), native.view(np.uint32)), "native and HIP launch paths differ"
    start = np.full((size, size), 0.75, dtype=np.float32)
    loaded = _render_map(mirhi, scenes, device, ls, casters, size, scenes.CMP_LESS, 1.0, scenes.CULL_NONE, load_map=start)
    expect = np.where(covered & (ref < 0.75), ref, np.float32(0.75))
    assert np.array_equal(loaded.view(np.uint32), expect.view(np.uint32)), "LOAD scope differs from min(loaded, caster depth)"


# ---- the PCF term against a pattern uploaded into the map ------------------------------------------------------------------------
def _pattern_scene(scenes, size, strength, intensity=3.0, map_size=64, shadow=True):
    ls = scenes.light_space_matrix((0.0, -1.0, 0.0), half_extent=2.0, near=0.1, far=20.0)
    gv, gi = scenes._ground_quad(3.0, 4)
    light = scenes.light_ubo(direction=(0.0, -1.0, 0.0), intensity=intensity, color=(1.0, 0.9, 0.8))
    d = scenes.DrawSpec(vertices=gv, stride=48, count=gi.size, indices=gi, program=scenes.PROGRAM_MODEL_PBR, cull_mode=scenes.CULL_NONE,
                        camera=_camera_from(scenes, ls), object=scenes.object_ubo(np.eye(4, dtype=np.float32)), light=light,
                        material=scenes.pbr_material_ubo((0.7, 0.7, 0.7, 1.0), 0.0, 0.6))
    sh = None
    if shadow:
        sh = scenes.ShadowSpec([], (map_size, map_size), scenes.shadow_ubo(ls, 0.0, 0.0, (map_size, map_size), strength),
                               load_op=scenes.LOAD_OP_LOAD)
    return scenes.Scene("pcf-pattern", size, size, [d], shadow=sh)


@pytest.mark.parametrize("strength", [1.0, 0.6])
def test_pcf_factor_matches_the_numpy_model(mirhi, scenes, oracle, device, strength):
    """Orthographic light straight down on a plane that fills its frustum, NdotL = 1, NormalBias 0; the camera has the light's frustum at
    twice the map's resolution, so pixel centres sit at quarter-texel points.  The frame is unlit + s * (lit - unlit) with s the numpy PCF
    factor of the uploaded two-valued map -- border rows and columns (clamp-to-edge) included."""
    m, size = 64, 128
    rng = np.random.default_rng(1234)
    pattern = np.where(rng.random((m, m)) < 0.5, 0.25, 1.0).astype(np.float32)
    smap = mirhi.Image(device, m, m, mirhi.Format.D32_SFLOAT)
    smap.upload(pattern)
    scene = _pattern_scene(scenes, size, strength)
    res = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT, shadow_map=smap)
    res.render()
    out = res.read()["color"]
    kept = smap.read().reshape(m, m).copy()
    res.destroy(); smap.destroy()
    assert np.array_equal(kept, pattern), "a LOAD scope without draws changed the map"
    lit = oracle.render(_pattern_scene(scenes, size, strength, shadow=False), want_bgra8=False)["rgba"]
    unlit = oracle.render(_pattern_scene(scenes, size, strength, intensity=0.0, shadow=False), want_bgra8=False)["rgba"]
    px, py = np.meshgrid(np.arange(size), np.arange(size), indexing="xy")
    u, v = (px + 0.5) / size, 1.0 - (py + 0.5) / size
    ls = scenes.light_space_matrix((0.0, -1.0, 0.0), half_extent=2.0, near=0.1, far=20.0)
    plane_depth = float((ls.T.astype(np.float64) @ np.array([0.0, 0.0, 0.0, 1.0]))[2])
    s = scenes.pcf_factor(pattern, u, v, np.full(u.shape, plane_depth - 0.0005), strength=strength)
    assert (s < 1.0).mean() > 0.5 and (s > 1.0 - strength).mean() > 0.5      # the pattern shades the frame, partly
    expect = unlit[..., :3] + s[..., None] * (lit[..., :3] - unlit[..., :3])
    assert_close(out, expect, f"pcf strength {strength}")


@pytest.mark.parametrize("kind", ["strength0", "cleared1", "cleared0"])
def test_shadow_no_op_cases_equal_the_oracle_frames(mirhi, scenes, oracle, device, kind):
    """Strength 0, or a map cleared to 1 without casters, leave the oracle's PBR frame; a map cleared to 0 gives the frame with the
    directional light off."""
    scene = scenes.shadowed_ground_case(160, 120, map_size=128, strength=0.0 if kind == "strength0" else 1.0)
    plain = dataclasses.replace(scene, shadow=None)
    if kind != "strength0":
        scene = dataclasses.replace(scene, shadow=dataclasses.replace(scene.shadow, casters=[], clear_depth=1.0 if kind == "cleared1" else 0.0))
    res = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT)
    res.render()
    out = res.read()["color"]
    res.destroy()
    if kind == "cleared0":
        plain = scenes.shadowed_ground_case(160, 120, map_size=128, intensity=0.0)
        plain = dataclasses.replace(plain, shadow=None)
    assert_close(out, oracle.render(plain, want_bgra8=False)["rgba"], kind)


# ---- end to end: a shadow scope ahead of the lit scope -----------------------------------------------------------------------------
def _footprint_classes(scenes, oracle, scene, margin_texels=3.0):
    """(inside, outside) masks of the ground pixels more than margin_texels map texels inside / outside the box's analytic shadow
    footprint (its corners projected along the light onto y = 0)."""
    ref = oracle.render(dataclasses.replace(scene, shadow=None), want_bgra8=False)
    ground_tris = scene.draws[0].count // 3
    ground = ref["prim"] < ground_tris
    h, w = ground.shape
    view, proj, _ = scenes.default_camera(w, h, eye=(0.0, 4.5, 6.5))
    inv = np.linalg.inv(scenes.mat_mul(proj, view).T.astype(np.float64))
    px, py = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5, indexing="xy")
    nx, ny = px / w * 2 - 1, py / h * 2 - 1

    def unproject(z):
        p = np.stack([nx, ny, np.full_like(nx, z), np.ones_like(nx)], axis=-1) @ inv.T
        return p[..., :3] / p[..., 3:4]
    a, b = unproject(0.0), unproject(1.0)
    t = a[..., 1] / (a[..., 1] - b[..., 1])
    hit = a + (b - a) * t[..., None]
    d = np.array(scenes.SHADOWED_GROUND_LIGHT, dtype=np.float64)
    (cx, cy, cz), (hx, hy, hz) = scenes.SHADOWED_GROUND_BOX
    pts = []
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                p = np.array([cx + sx * hx, cy + sy * hy, cz + sz * hz])
                q = p - d * (p[1] / d[1])
                pts.append((q[0], q[2]))
    pts = sorted(set(pts))

    def cross(o, p, q):
        return (p[0] - o[0]) * (q[1] - o[1]) - (p[1] - o[1]) * (q[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    hull = np.array(lower[:-1] + upper[:-1])               # counter-clockwise in (x, z)
    x, z = hit[..., 0], hit[..., 2]
    inside_d = np.full(x.shape, np.inf)
    out_d = np.full(x.shape, np.inf)
    for k in range(len(hull)):
        p0, p1 = hull[k], hull[(k + 1) % len(hull)]
        e = p1 - p0
        n = np.array([-e[1], e[0]]) / np.linalg.norm(e)        # inward normal of a counter-clockwise hull
        inside_d = np.minimum(inside_d, (x - p0[0]) * n[0] + (z - p0[1]) * n[1])
        tt = np.clip(((x - p0[0]) * e[0] + (z - p0[1]) * e[1]) / (e @ e), 0.0, 1.0)
        out_d = np.minimum(out_d, np.hypot(x - (p0[0] + tt * e[0]), z - (p0[1] + tt * e[1])))
    texel = 2.0 * scenes.SHADOWED_GROUND_EXTENT / scene.shadow.size[0] * np.linalg.norm(d) / abs(d[1])
    margin = margin_texels * texel
    return ground & (inside_d > margin), ground & (inside_d < 0) & (out_d > margin)


def test_shadow_scope_then_lit_scope_end_to_end(mirhi, scenes, oracle):
    """shadowed_ground_case: ground pixels well inside the box's shadow equal the unlit frame, those well outside the lit one; the frame is
    the same bits from one command buffer, from two on two queue lanes in one submit, and from two separate submits."""
    scene = scenes.shadowed_ground_case()
    inside, outside = _footprint_classes(scenes, oracle, scene)
    assert inside.sum() >= 1000 and outside.sum() >= 1000, (int(inside.sum()), int(outside.sum()))
    lit = oracle.render(dataclasses.replace(scene, shadow=None), want_bgra8=False)["rgba"]
    unlit = oracle.render(dataclasses.replace(scenes.shadowed_ground_case(intensity=0.0), shadow=None), want_bgra8=False)["rgba"]
    dev = mirhi.Device(0)
    try:
        dev.set_queue_lanes(2)
        one = mirhi.SceneResources(dev, scene, mirhi.Format.R32G32B32A32_SFLOAT)
        one.render()
        frame = one.read()["color"]
        one.destroy()
        assert_close(frame, unlit, "inside the footprint", inside)
        assert_close(frame, lit, "outside the footprint", outside)
        two = mirhi.SceneResources(dev, scene, mirhi.Format.R32G32B32A32_SFLOAT, shadow_cmd=True)
        two.shadow_cmd.set_queue_lane(1)
        two.cmd.set_queue_lane(0)
        for _ in range(3):
            two.render()                                       # one submit, two lanes
            assert np.array_equal(two.read()["color"], frame), "two lanes in one submit differ from one command buffer"
        for _ in range(3):
            dev.submit([two.shadow_cmd])                       # two submits
            dev.submit([two.cmd])
            assert np.array_equal(two.read()["color"], frame), "two submits differ from one command buffer"
        two.destroy()
    finally:
        dev.destroy()


@pytest.mark.parametrize("shared", [False, True])
def test_frames_in_flight_with_alternating_lights(mirhi, scenes, oracle, shared):
    """Two frames in flight, fenced, the light alternating between two directions (each frame its own shadow map, or one map shared by
    both -- the next frame's shadow scope rewrites what the last frame's lit scope reads): every frame equals its single-shot frame."""
    dirs = [scenes.SHADOWED_GROUND_LIGHT, (-0.5, -1.0, 0.2)]
    cases = [scenes.shadowed_ground_case(160, 120, map_size=256, light_dir=d) for d in dirs]
    dev = mirhi.Device(0)
    try:
        dev.set_queue_lanes(2)
        single = []
        for c in cases:
            r = mirhi.SceneResources(dev, c, mirhi.Format.R32G32B32A32_SFLOAT)
            r.render()
            single.append(r.read()["color"])
            r.destroy()
        assert not np.array_equal(single[0], single[1])
        smap = mirhi.Image(dev, 256, 256, mirhi.Format.D32_SFLOAT) if shared else None
        res = [mirhi.SceneResources(dev, c, mirhi.Format.R32G32B32A32_SFLOAT, shadow_map=smap) for c in cases]
        assert res[0].cmd.handle != res[1].cmd.handle
        fences = [mirhi.Fence(dev, signaled=True) for _ in range(2)]
        for f in range(8):
            k = f % 2
            fences[k].wait()
            if f >= 2:
                assert np.array_equal(res[k].color.read(), single[k]), f"frame {f - 2} differs from its single-shot frame"
            fences[k].reset()
            res[k].render(fences[k])
        for k in range(2):
            fences[k].wait()
            assert np.array_equal(res[k].color.read(), single[k])
        for f in fences:
            f.destroy()
        for r in res:
            r.destroy()
        if smap is not None:
            smap.destroy()
    finally:
        dev.destroy()


@pytest.mark.parametrize("layout", ["bands", "interleaved"])
@pytest.mark.parametrize("world", [2, 4])
def test_tile_split_renders_the_whole_map_on_every_rank(mirhi, scenes, layout, world):
    """set_tile_split(r, world): the depth-only scope renders the unsplit map on every rank; each rank's rows of the lit frame equal the
    unsplit frame's."""
    scene = scenes.shadowed_ground_case(160, 120, map_size=256)
    dev = mirhi.Device(0)
    try:
        full = mirhi.SceneResources(dev, scene, mirhi.Format.R32G32B32A32_SFLOAT)
        full.render()
        frame, fmap = full.read()["color"], full.shadow_map.read().copy()
        full.destroy()
        for r in range(world):
            dev.set_tile_split(r, world, layout)
            res = mirhi.SceneResources(dev, scene, mirhi.Format.R32G32B32A32_SFLOAT)
            res.render()
            out = res.read()["color"]
            assert np.array_equal(res.shadow_map.read(), fmap), f"rank {r}/{world}: the shadow map is not the whole map"
            first, step, count = dev.split_rows(scene.height)
            for k in range(count):
                y0 = (first + k * step) * 32
                assert np.array_equal(out[y0:y0 + 32], frame[y0:y0 + 32]), f"rank {r}/{world}: tile row {first + k * step} differs"
            res.destroy()
        dev.set_tile_split(0, 1)
    finally:
        dev.destroy()


def test_shadow_refusals(mirhi, scenes, device):
    """Every refusal of the shadow path, with its result code and message; D32 in the albedo slot is still refused."""
    M = mirhi

    def shadow_builder():
        return (M.GraphicsPipelineBuilder().vertex_shader(M.Program.SHADOW).fragment_shader(M.Program.SHADOW).vertex_binding(12)
                .vertex_attributes(M.SHADOW_VERTEX_OFFSETS).depth_attachment_format(M.Format.D32_SFLOAT))

    def refused(fn, variant, text):
        with pytest.raises(M.RhiError) as e:
            fn()
        assert e.value.variant == variant and text in e.value.message, (e.value.variant, e.value.message)

    refused(lambda: shadow_builder().build(device), "PipelineError", "At least one color attachment format is required")
    refused(lambda: shadow_builder().color_attachment_format(M.Format.B8G8R8A8_SRGB).build(device), "PipelineError", "depth-only")
    refused(lambda: (M.GraphicsPipelineBuilder().vertex_shader(M.Program.MODEL).fragment_shader(M.Program.MODEL).vertex_binding(48)
                     .vertex_attributes(M.VERTEX_OFFSETS).color_attachment_format(M.Format.UNDEFINED)
                     .depth_attachment_format(M.Format.D32_SFLOAT).build(device)), "PipelineError", "UNDEFINED")
    for op in (scenes.CMP_EQUAL, scenes.CMP_ALWAYS, scenes.CMP_NOT_EQUAL):
        refused(lambda: shadow_builder().color_attachment_format(M.Format.UNDEFINED).depth_compare_op(op).build(device), "PipelineError", "unsupported")
    refused(lambda: shadow_builder().color_attachment_format(M.Format.UNDEFINED).depth_write_enable(False).build(device), "PipelineError", "unsupported")
    refused(lambda: shadow_builder().vertex_binding(8).color_attachment_format(M.Format.UNDEFINED).build(device), "PipelineError", "vertex stride")
    refused(lambda: (M.GraphicsPipelineBuilder().vertex_shader(M.Program.SHADOW).fragment_shader(M.Program.MODEL).vertex_binding(48)
                     .vertex_attributes(M.VERTEX_OFFSETS).color_attachment_format(M.Format.R32G32B32A32_SFLOAT)
                     .depth_attachment_format(M.Format.D32_SFLOAT).build(device)), "ShaderError", "does not produce the inputs")
    sp = shadow_builder().color_attachment_format(M.Format.UNDEFINED).build(device)
    mp = (M.GraphicsPipelineBuilder().vertex_shader(M.Program.MODEL).fragment_shader(M.Program.MODEL_PBR).vertex_binding(48)
          .vertex_attributes(M.VERTEX_OFFSETS).color_attachment_format(M.Format.R32G32B32A32_SFLOAT)
          .depth_attachment_format(M.Format.D32_SFLOAT).build(device))
    bp = (M.GraphicsPipelineBuilder().vertex_shader(M.Program.MODEL).fragment_shader(M.Program.MODEL_PBR).vertex_binding(48)
          .vertex_attributes(M.VERTEX_OFFSETS).color_attachment_format(M.Format.R32G32B32A32_SFLOAT)
          .depth_attachment_format(M.Format.D32_SFLOAT).alpha_blend().build(device))
    dimg = M.Image(device, 64, 64, M.Format.D32_SFLOAT)
    cimg = M.Image(device, 64, 64, M.Format.R32G32B32A32_SFLOAT)
    vb = M.Buffer.new_with_data(device, M.BufferUsage.Vertex, np.zeros(3 * 12, dtype=np.float32))
    ub = M.Buffer.new_with_data(device, M.BufferUsage.Uniform, np.zeros(208, dtype=np.uint8))
    small = M.Buffer.new_with_data(device, M.BufferUsage.Uniform, np.zeros(80, dtype=np.uint8))
    cmd = M.CommandBuffer(device)

    def scope(color, depth=None, **kw):
        cmd.begin()
        cmd.begin_rendering(color, depth=depth, **kw)
        cmd.set_viewport(0.0, 0.0, 64.0, 64.0)
        cmd.set_scissor(0, 0, 64, 64)
        cmd.bind_vertex_buffers(0, [vb], [0])
        for s in (M.Slot.CAMERA, M.Slot.OBJECT, M.Slot.LIGHTS, M.Slot.MATERIAL):
            cmd.bind_uniform(s, ub)

    refused(lambda: (cmd.begin(), cmd.begin_rendering(None)), "InvalidHandle", "color_image is null")
    cmd.reset()
    pimg = M.Image(device, 64, 64, M.Format.R32_UINT)
    refused(lambda: (cmd.begin(), cmd.begin_rendering(None, depth=dimg, depth_store_op=M.StoreOp.STORE, prim_id=pimg)),
            "InvalidHandle", "prim_id_image")
    cmd.reset()
    refused(lambda: (cmd.begin(), cmd.begin_rendering(None, depth=dimg)), "InvalidHandle", "must store its depth")
    cmd.reset()
    refused(lambda: (cmd.begin(), cmd.begin_rendering(None, depth=cimg, depth_store_op=M.StoreOp.STORE)), "InvalidHandle", "D32_SFLOAT")
    cmd.reset()
    scope(None, dimg, depth_store_op=M.StoreOp.STORE)
    cmd.bind_pipeline(mp)
    refused(lambda: cmd.draw(3), "InvalidHandle", "only SHADOW draws")
    cmd.reset()
    scope(cimg, dimg)
    cmd.bind_pipeline(sp)
    refused(lambda: cmd.draw(3), "InvalidHandle", "depth-only rendering scope")
    cmd.reset()
    scope(cimg, dimg)
    refused(lambda: cmd.bind_texture(M.TextureSlot.SHADOW_MAP, cimg), "InvalidHandle", "D32_SFLOAT")
    refused(lambda: cmd.bind_texture(M.TextureSlot.ALBEDO, dimg), "InvalidHandle", "R8G8B8A8")
    cmd.bind_pipeline(mp)
    cmd.bind_texture(M.TextureSlot.SHADOW_MAP, dimg)
    refused(lambda: cmd.draw(3), "InvalidHandle", "ShadowParams")
    cmd.bind_uniform(M.Slot.SHADOW_DATA, small)
    refused(lambda: cmd.draw(3), "InvalidHandle", "ShadowParams (SHADOW_DATA) range 80 smaller than 96")
    cmd.bind_uniform(M.Slot.SHADOW_DATA, ub)
    cmd.bind_pipeline(bp)
    refused(lambda: cmd.draw(3), "InvalidHandle", "unsupported: a shadow map with blending")
    cmd.bind_pipeline(mp)
    cmd.draw(3)
    cmd.bind_texture(M.TextureSlot.SHADOW_MAP, None)
    cmd.draw(3)                                              # a PBR draw without a map still records
    cmd.end_rendering()
    cmd.end()
    cmd.destroy()
    for o in (sp, mp, bp, dimg, cimg, pimg, vb, ub, small):
        o.destroy()
