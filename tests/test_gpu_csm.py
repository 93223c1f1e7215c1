"""Cascaded shadow maps on the GPU: layered D32 images and layer views, CalculateShadowCSM (shadow_csm.hlsli) in the MODEL_PBR resolve against
the numpy model with no excluded pixels, the no-op cases, four shadow scopes ahead of the lit scope on one or two queue lanes ("ordering is
by the parent"), frames in flight on one shared array, the tile split, a single layer as an ordinary shadow map, and the refusals."""
import dataclasses

import numpy as np
import pytest

import csm_cases
from test_gpu_shadow import RGB_TOL, _casters, _oracle_depth, _render_map, assert_close      # noqa: F401  (the bound of the PBR parity tests)

pytestmark = pytest.mark.gpu


# ---- 1. layer views --------------------------------------------------------------------------------------------------------------------
def _render_into_view(mirhi, scenes, dev, array, layer, ls, casters, size, load):
    view = array.layer_view(layer)
    objs = [view]
    pipe = (mirhi.GraphicsPipelineBuilder().vertex_shader(mirhi.Program.SHADOW).fragment_shader(mirhi.Program.SHADOW)
            .vertex_binding(48).vertex_attributes(mirhi.SHADOW_VERTEX_OFFSETS)
            .color_attachment_format(mirhi.Format.UNDEFINED).depth_attachment_format(mirhi.Format.D32_SFLOAT)
            .cull_mode(scenes.CULL_NONE).depth_compare_op(scenes.CMP_LESS).build(dev))
    cmd = mirhi.CommandBuffer(dev)
    cmd.begin()
    cmd.begin_rendering(None, depth=view, clear_depth=1.0, depth_store_op=mirhi.StoreOp.STORE,
                        depth_load_op=mirhi.LoadOp.LOAD if load else mirhi.LoadOp.CLEAR)
    cmd.set_viewport(0.0, 0.0, float(size), float(size))
    cmd.set_scissor(0, 0, size, size)
    cmd.bind_pipeline(pipe)
    for v, i, m in casters:
        vb = mirhi.Buffer.new_with_data(dev, mirhi.BufferUsage.Vertex, v)
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
    out_view = view.read().copy()
    cmd.destroy(); pipe.destroy()
    for o in objs:
        o.destroy()
    return out_view


@pytest.mark.parametrize("hip_launch", [False, True])
@pytest.mark.parametrize("load", [False, True])
@pytest.mark.parametrize("layer", [0, 3])
def test_shadow_scope_into_a_layer_view(mirhi, scenes, oracle, device, layer, load, hip_launch):
    """Layer k equals, bit for bit, the same scope rendered into a stand-alone D32 image (and the oracle's MODEL depth where covered); the
    other three layers keep their sentinels; read() of the array returns the layers in order, of a view its layer."""
    size = 96
    ls, casters = _casters(scenes)
    sentinels = np.stack([np.full((size, size), v, dtype=np.float32) for v in (0.9, 0.8, 0.7, 0.6)])
    sentinels[:, ::7, ::5] += np.float32(0.01)
    alone = _render_map(mirhi, scenes, device, ls, casters, size, scenes.CMP_LESS, 1.0, scenes.CULL_NONE, load_map=sentinels[layer] if load else None)
    ref, covered = _oracle_depth(scenes, oracle, ls, casters, size, scenes.CMP_LESS, 1.0, scenes.CULL_NONE)
    array = mirhi.Image.array(device, size, size, 4, mirhi.Format.D32_SFLOAT)
    assert array.layers == 4 and array.width == size and mirhi.lib().mirhi_image_size_bytes(array.handle) == 4 * size * size * 4
    array.upload(sentinels)
    if hip_launch:
        device.set_profiling(mirhi.Profile.TIMING)           # timed dispatches go out as HIP launches
    try:
        seen = _render_into_view(mirhi, scenes, device, array, layer, ls, casters, size, load)
    finally:
        if hip_launch:
            device.set_profiling(0)
            device.reset_kernel_times()
    out = array.read()
    array.destroy()
    assert out.shape == (4, size, size)
    assert np.array_equal(out[layer].view(np.uint32), alone.view(np.uint32)), "the layer differs from the stand-alone image"
    assert np.array_equal(seen.view(np.uint32), out[layer].view(np.uint32)), "reading the view does not return its layer"
    if not load:
        assert covered.sum() > 500 and np.array_equal(out[layer].view(np.uint32)[covered], ref.view(np.uint32)[covered])
    for k in range(4):
        if k != layer:
            assert np.array_equal(out[k].view(np.uint32), sentinels[k].view(np.uint32)), f"layer {k} lost its sentinel"


def test_view_upload_touches_its_layer_only(mirhi, device):
    array = mirhi.Image.array(device, 8, 4, 3, mirhi.Format.D32_SFLOAT)
    base = np.arange(3 * 4 * 8, dtype=np.float32).reshape(3, 4, 8)
    array.upload(base)
    v = array.layer_view(1)
    assert v.layers == 1 and v.read().shape == (4, 8) and np.array_equal(v.read(), base[1])
    v.upload(np.full((4, 8), -2.0, dtype=np.float32))
    want = base.copy(); want[1] = -2.0
    assert np.array_equal(array.read(), want)
    v.destroy(); array.destroy()


# ---- 2. the CSM term against the numpy model -------------------------------------------------------------------------------------------
def test_csm_factor_matches_the_numpy_model(mirhi, scenes, oracle, device):
    """csm_cases.pattern_scene: a receiver tilted about one horizontal axis under four lights that look straight down (half extents e, 1.5e,
    2e, 3e -- see csm_cases.pattern_matrices for why not e, 2e, 4e, 8e), four independent two-valued layers, splits between the oracle depths
    of neighbouring columns.  Expected: unlit + s * (lit - unlit), s = csm_factor fed with the oracle's depth.  NO pixel is excluded."""
    layers = csm_cases.pattern_layers()
    expect, splits, facts = csm_cases.pattern_expectation(scenes, oracle, layers)
    print("pattern facts:", facts)
    csm_cases.assert_pattern_conditions(facts)
    array = mirhi.Image.array(device, csm_cases.PATTERN_LAYER, csm_cases.PATTERN_LAYER, 4, mirhi.Format.D32_SFLOAT)
    array.upload(layers)
    scene = csm_cases.pattern_scene(scenes, cascades=csm_cases.pattern_spec(scenes, splits))
    res = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT, cascade_array=array, want_depth=True)
    res.render()
    got = res.read()
    kept = array.read().copy()
    res.destroy(); array.destroy()
    assert np.array_equal(kept, layers), "LOAD scopes without draws changed the layers"
    ref_depth = oracle.render(csm_cases.pattern_scene(scenes), want_bgra8=False)["depth"]
    assert np.array_equal(got["depth"].view(np.uint32), ref_depth.view(np.uint32)), "SV_Position.z: the depth bits differ from the oracle's"
    err = np.abs(got["color"][..., :3].astype(np.float64) - expect) / np.maximum(1.0, np.abs(expect))
    print("csm pattern: max |dRGB| =", float(err.max()))
    assert_close(got["color"], expect, "csm pattern")


# ---- 3. no-op cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cleared1", "cleared0", "out_of_bounds"])
def test_csm_no_op_cases_equal_the_oracle_frames(mirhi, scenes, oracle, device, kind):
    """All four layers cleared to 1.0 without casters: the plain PBR frame; cleared to 0.0: the frame with the directional light off (the
    cascades of this case span the view distances 1 .. 120, so that every fragment of the frame lies inside the cascade it selects -- outside a
    cascade's bounds the term is 1.0 by definition, which is the third case: lights that look elsewhere leave the plain frame)."""
    scene = scenes.cascaded_ground_case(160, 120, map_size=128)
    plain = dataclasses.replace(scene, cascades=None)
    view, proj, _ = scenes.default_camera(160, 120, eye=scenes.CASCADED_GROUND_EYE, target=scenes.CASCADED_GROUND_TARGET)
    cas = scenes.csm_cascades(view, proj, scenes.CASCADED_GROUND_LIGHT, 1.0, 120.0)
    spec = dataclasses.replace(scene.cascades, casters=[[], [], [], []], clear_depth=0.0 if kind == "cleared0" else 1.0,
                               params=scenes.csm_ubo(cas.matrices, cas.split_depths, 0.005, 0.01, 128.0))
    if kind == "out_of_bounds":           # lights that look at a place 500 units away: every fragment is outside every cascade -> 1.0, whatever the layers hold
        mats = [scenes.light_space_matrix(scenes.CASCADED_GROUND_LIGHT, center=(500.0, 0.0, 0.0), half_extent=2.0 + k) for k in range(4)]
        spec = dataclasses.replace(spec, clear_depth=0.0, params=scenes.csm_ubo(mats, [0.99, 0.995, 0.998], 0.005, 0.01, 128.0))
    res = mirhi.SceneResources(device, dataclasses.replace(scene, cascades=spec), mirhi.Format.R32G32B32A32_SFLOAT)
    res.render()
    out = res.read()["color"]
    res.destroy()
    if kind == "cleared0":
        plain = dataclasses.replace(scenes.cascaded_ground_case(160, 120, map_size=128, intensity=0.0), cascades=None)
    assert_close(out, oracle.render(plain, want_bgra8=False)["rgba"], kind)


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------
def test_cascade_scopes_then_lit_scope_end_to_end(mirhi, scenes, oracle):
    """cascaded_ground_case: ground pixels more than 3 texels (of the cascade the pixel selects) inside a box's footprint equal the unlit
    oracle frame, those more than 3 such texels outside every footprint the lit one, in every cascade; the frame is the same bits from one
    command buffer, from shadow scopes and lit scope on two queue lanes in one submit, and from two submits."""
    scene = scenes.cascaded_ground_case()
    c = csm_cases.ground_classes(scenes, oracle, scene)
    csm_cases.assert_ground_conditions(c)
    lit = c["ref"]["rgba"]
    unlit = oracle.render(dataclasses.replace(scenes.cascaded_ground_case(intensity=0.0), cascades=None), want_bgra8=False)["rgba"]
    dev = mirhi.Device(0)
    try:
        dev.set_queue_lanes(2)
        one = mirhi.SceneResources(dev, scene, mirhi.Format.R32G32B32A32_SFLOAT)
        one.render()
        frame = one.read()["color"]
        one.destroy()
        for k in range(4):
            sel = c["idx"] == k
            assert_close(frame, unlit, f"cascade {k}: inside the footprints", c["inside"] & sel)
            assert_close(frame, lit, f"cascade {k}: outside the footprints", c["outside"] & sel)
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


# ---- 5. frames in flight ---------------------------------------------------------------------------------------------------------
def test_frames_in_flight_share_one_cascade_array(mirhi, scenes):
    dirs = [scenes.CASCADED_GROUND_LIGHT, (-0.5, -1.0, 0.3)]
    cases = [scenes.cascaded_ground_case(160, 120, map_size=256, light_dir=d) for d in dirs]
    dev = mirhi.Device(0)
    try:
        dev.set_queue_lanes(2)
        single = []
        for cse in cases:
            r = mirhi.SceneResources(dev, cse, mirhi.Format.R32G32B32A32_SFLOAT)
            r.render()
            single.append(r.read()["color"])
            r.destroy()
        assert not np.array_equal(single[0], single[1])
        array = mirhi.Image.array(dev, 256, 256, 4, mirhi.Format.D32_SFLOAT)
        res = [mirhi.SceneResources(dev, cse, mirhi.Format.R32G32B32A32_SFLOAT, cascade_array=array) for cse in cases]
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
        array.destroy()
    finally:
        dev.destroy()


# ---- 6. tile split -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["bands", "interleaved"])
@pytest.mark.parametrize("world", [2, 4])
def test_tile_split_renders_every_layer_on_every_rank(mirhi, scenes, layout, world):
    scene = scenes.cascaded_ground_case(160, 120, map_size=256)
    dev = mirhi.Device(0)
    try:
        full = mirhi.SceneResources(dev, scene, mirhi.Format.R32G32B32A32_SFLOAT)
        full.render()
        frame, layers = full.read()["color"], full.cascade_array.read().copy()
        full.destroy()
        assert all((layers[k] < 1.0).any() for k in range(4)), "every layer holds casters"
        rows = np.zeros(scene.height, dtype=bool)
        for r in range(world):
            dev.set_tile_split(r, world, layout)
            res = mirhi.SceneResources(dev, scene, mirhi.Format.R32G32B32A32_SFLOAT)
            res.render()
            out = res.read()["color"]
            assert np.array_equal(res.cascade_array.read().view(np.uint32), layers.view(np.uint32)), f"rank {r}/{world}: the layers are not whole"
            first, step, count = dev.split_rows(scene.height)
            for k in range(count):
                y0 = (first + k * step) * 32
                assert np.array_equal(out[y0:y0 + 32], frame[y0:y0 + 32]), f"rank {r}/{world}: tile row {first + k * step} differs"
                rows[y0:y0 + 32] = True
            res.destroy()
        assert rows.all(), "the ranks' rows do not cover the frame"
        dev.set_tile_split(0, 1)
    finally:
        dev.destroy()


# ---- 7. a single layer as an ordinary shadow map ---------------------------------------------------------------------------------
def test_layer_view_as_an_ordinary_shadow_map(mirhi, scenes, device):
    scene = scenes.shadowed_ground_case(160, 120, map_size=128)
    alone = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT)
    alone.render()
    want = alone.read()["color"]
    alone.destroy()
    array = mirhi.Image.array(device, 128, 128, 4, mirhi.Format.D32_SFLOAT)
    array.upload(np.zeros((4, 128, 128), dtype=np.float32))
    view = array.layer_view(2)
    res = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT, shadow_map=view)
    res.render()
    got = res.read()["color"]
    res.destroy()
    layers = array.read()
    view.destroy(); array.destroy()
    assert np.array_equal(got, want), "a layer view at MIRHI_TEXTURE_SHADOW_MAP differs from a stand-alone map"
    assert (layers[2] > 0).any() and not layers[[0, 1, 3]].any()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_csm_refusals(mirhi, scenes, device):
    M = mirhi

    def refused(fn, variant, text):
        with pytest.raises(M.RhiError) as e:
            fn()
        assert e.value.variant == variant and text in e.value.message, (e.value.variant, e.value.message)

    refused(lambda: M.Image.array(device, 16, 16, 4, M.Format.R8G8B8A8_UNORM), "InvalidHandle", "D32_SFLOAT only")
    refused(lambda: M.Image.array(device, 16, 16, 0, M.Format.D32_SFLOAT), "InvalidHandle", "[1, 2048]")
    refused(lambda: M.Image.array(device, 16, 16, 2049, M.Format.D32_SFLOAT), "InvalidHandle", "[1, 2048]")
    refused(lambda: M.Image.array(device, 0, 16, 4, M.Format.D32_SFLOAT), "InvalidHandle", "greater than 0")
    arr = M.Image.array(device, 64, 64, 4, M.Format.D32_SFLOAT)
    arr3 = M.Image.array(device, 64, 64, 3, M.Format.D32_SFLOAT)
    dimg = M.Image(device, 64, 64, M.Format.D32_SFLOAT)
    cimg = M.Image(device, 64, 64, M.Format.R32G32B32A32_SFLOAT)
    assert dimg.layers == 1 and cimg.layers == 1
    refused(lambda: arr.layer_view(4), "InvalidHandle", "layer 4 out of range")
    refused(lambda: dimg.layer_view(0), "InvalidHandle", "array images")
    view = arr.layer_view(1)
    refused(lambda: view.layer_view(0), "InvalidHandle", "array images")
    refused(arr.destroy, "InvalidHandle", "live layer views")
    assert arr.handle                                       # (the failed destroy left the wrapper's handle alone)
    vb = M.Buffer.new_with_data(device, M.BufferUsage.Vertex, np.zeros(3 * 12, dtype=np.float32))
    ub = M.Buffer.new_with_data(device, M.BufferUsage.Uniform, np.zeros(336, dtype=np.uint8))
    small = M.Buffer.new_with_data(device, M.BufferUsage.Uniform, np.zeros(320, dtype=np.uint8))
    sb = M.Buffer(device, M.BufferUsage.Storage, 336)

    def pbr():
        return (M.GraphicsPipelineBuilder().vertex_shader(M.Program.MODEL).fragment_shader(M.Program.MODEL_PBR).vertex_binding(48)
                .vertex_attributes(M.VERTEX_OFFSETS).color_attachment_format(M.Format.R32G32B32A32_SFLOAT).depth_attachment_format(M.Format.D32_SFLOAT))
    mp, bp = pbr().build(device), pbr().alpha_blend().build(device)
    dp, pp = pbr().fragment_discard_enable(True).build(device), pbr().depth_write_enable(False).build(device)
    fp = (M.GraphicsPipelineBuilder().vertex_shader(M.Program.MODEL).fragment_shader(M.Program.MODEL_FULL).vertex_binding(48)
          .vertex_attributes(M.VERTEX_OFFSETS).color_attachment_format(M.Format.R32G32B32A32_SFLOAT).depth_attachment_format(M.Format.D32_SFLOAT).build(device))
    cmd = M.CommandBuffer(device)
    refused(lambda: (cmd.begin(), cmd.begin_rendering(arr)), "InvalidHandle", "an image array is not an attachment")
    cmd.reset()
    refused(lambda: (cmd.begin(), cmd.begin_rendering(None, depth=arr, depth_store_op=M.StoreOp.STORE)), "InvalidHandle", "an image array is not an attachment")
    cmd.reset()
    cmd.begin()
    cmd.begin_rendering(cimg, depth=dimg)
    cmd.set_viewport(0.0, 0.0, 64.0, 64.0)
    cmd.set_scissor(0, 0, 64, 64)
    cmd.bind_vertex_buffers(0, [vb], [0])
    big = M.Buffer.new_with_data(device, M.BufferUsage.Uniform, np.zeros(208, dtype=np.uint8))
    for s in (M.Slot.CAMERA, M.Slot.OBJECT, M.Slot.LIGHTS, M.Slot.MATERIAL, M.Slot.SHADOW_DATA):
        cmd.bind_uniform(s, big)
    refused(lambda: cmd.bind_shadow_cascades(dimg, ub), "InvalidHandle", "an image array (mirhi_image_create_array)")
    refused(lambda: cmd.bind_shadow_cascades(view, ub), "InvalidHandle", "not a layer view")
    refused(lambda: cmd.bind_shadow_cascades(arr3, ub), "InvalidHandle", "CASCADE_COUNT = 4 layers (got 3)")
    refused(lambda: cmd.bind_shadow_cascades(arr, small), "InvalidHandle", "CSMParams range 320 smaller than 336")
    refused(lambda: cmd.bind_shadow_cascades(arr, ub, 16, 0), "InvalidHandle", "CSMParams range 320 smaller than 336")
    refused(lambda: cmd.bind_shadow_cascades(arr, ub, 0, 400), "InvalidHandle", "exceeds buffer")
    refused(lambda: cmd.bind_shadow_cascades(arr, sb), "InvalidHandle", "uniform buffer")
    refused(lambda: cmd.bind_texture(M.TextureSlot.SHADOW_MAP, arr), "InvalidHandle", "must be a 2-D image")
    cmd.bind_shadow_cascades(arr, ub)
    cmd.bind_texture(M.TextureSlot.SHADOW_MAP, view)          # a view is an ordinary D32 image here
    cmd.bind_pipeline(mp)
    refused(lambda: cmd.draw(3), "InvalidHandle", "both a shadow map (MIRHI_TEXTURE_SHADOW_MAP) and shadow cascades")
    cmd.bind_texture(M.TextureSlot.SHADOW_MAP, None)
    for p in (bp, dp, pp):
        cmd.bind_pipeline(p)
        refused(lambda: cmd.draw(3), "InvalidHandle", "unsupported: shadow cascades with blending, fragment discard, a predicate depth state")
    cmd.bind_pipeline(fp)
    cmd.draw(3)                                               # MODEL_FULL ignores the binding
    cmd.bind_pipeline(mp)
    cmd.draw(3)
    cmd.bind_shadow_cascades(None)
    cmd.bind_texture(M.TextureSlot.SHADOW_MAP, dimg)
    refused(lambda: cmd.draw(3), "InvalidHandle", "a single shadow map and draws with shadow cascades in one rendering scope")
    cmd.bind_texture(M.TextureSlot.SHADOW_MAP, None)
    cmd.draw(3)                                               # a PBR draw with nothing bound still records
    cmd.end_rendering()
    cmd.end()
    cmd.destroy()
    view.destroy()
    for o in (arr, arr3, dimg, cimg, vb, ub, small, sb, big, mp, bp, dp, pp, fp):
        o.destroy()
