"""Cascade blending and stabilised cascades on the GPU: CalculateShadowCSMBlended (shadow_csm.hlsli:212-277) in the MODEL_PBR and MODEL_PBR_IBL
resolves against the float64 model with no excluded pixel and on both dispatch paths, threshold 0 through the new call, blended and unblended
draws in one scope, the stabilised ground case end to end, a camera that moves in a re-recorded frame loop, the tile split, a render area, and
the refusals.  Inputs and their conditions: tests/csm_blend_cases.py (asserted by tests/test_csm_blend_cpu.py)."""
import dataclasses

import numpy as np
import pytest

import csm_blend_cases as cases
import csm_cases
import render_area_cases as rc
from test_csm_blend_cpu import PROGS_CSM_BLEND, _scope_plan
from test_gpu_shadow import RGB_TOL, assert_close      # noqa: F401  (the bound of test_gpu_csm.py's assert_close: the PBR parity tests')

pytestmark = pytest.mark.gpu


def _pattern_array(mirhi, device):
    array = mirhi.Image.array(device, csm_cases.PATTERN_LAYER, csm_cases.PATTERN_LAYER, 4, mirhi.Format.D32_SFLOAT)
    array.upload(csm_cases.pattern_layers())
    return array


def _render_pattern(mirhi, device, scene, array, fmt=None, prepare=None):
    res = mirhi.SceneResources(device, scene, fmt or mirhi.Format.R32G32B32A32_SFLOAT, cascade_array=array, want_depth=True)
    if prepare is not None:
        prepare(res)
        res.record()
    res.render()
    out = res.read()
    res.destroy()
    return out


# ---- 1. the blended term against the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hip_launch", [False, True])
def test_blended_factor_matches_the_model(mirhi, scenes, oracle, device, hip_launch):
    """csm_cases.pattern_scene under threshold 0.5: expected = unlit + s (lit - unlit), s = csm_factor_blended fed with the oracle's depth.
    Every pixel is checked; the depth bits are the oracle's.  hip_launch: timed dispatches go out as HIP launches, the other dispatch path."""
    expect, plain, splits, facts, ref_depth = cases.pattern_expectation(scenes, oracle)
    cases.assert_blend_conditions(facts)
    array = _pattern_array(mirhi, device)
    scene = csm_cases.pattern_scene(scenes, cascades=cases.pattern_spec(scenes, splits))
    if hip_launch:
        device.set_profiling(mirhi.Profile.TIMING)
    try:
        got = _render_pattern(mirhi, device, scene, array)
    finally:
        if hip_launch:
            device.set_profiling(0)
            device.reset_kernel_times()
    kept = array.read().copy()
    array.destroy()
    assert np.array_equal(kept, csm_cases.pattern_layers()), "LOAD scopes without draws changed the layers"
    assert np.array_equal(got["depth"].view(np.uint32), ref_depth.view(np.uint32)), "SV_Position.z: the depth bits differ from the oracle's"
    err = np.abs(got["color"][..., :3].astype(np.float64) - expect) / np.maximum(1.0, np.abs(expect))
    off = np.abs(got["color"][..., :3].astype(np.float64) - plain) / np.maximum(1.0, np.abs(plain))
    print(f"blended csm pattern (hip_launch={hip_launch}): max |dRGB| = {float(err.max()):.3e}; against the unblended model: {float(off.max()):.3e}")
    assert_close(got["color"], expect, "blended csm pattern")
    assert float(off.max()) > 100 * RGB_TOL, "the blended frame is not the unblended one"


# ---- 2. threshold 0 through the new call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["R32G32B32A32_SFLOAT", "B8G8R8A8_SRGB"])
def test_threshold_zero_through_the_new_call_keeps_the_bits(mirhi, scenes, oracle, device, fmt):
    _, _, splits, _, _ = cases.pattern_expectation(scenes, oracle)
    array = _pattern_array(mirhi, device)
    scene = csm_cases.pattern_scene(scenes, cascades=csm_cases.pattern_spec(scenes, splits))
    f = getattr(mirhi.Format, fmt)
    old = _render_pattern(mirhi, device, scene, array, f)
    calls = []

    def through_the_new_call(res):
        def bind(arr, params=None, offset=0, range_=0, blend_threshold=0.0):
            calls.append(blend_threshold)
            res.cmd.bind_shadow_cascades_blended(arr, params, offset, range_, 0.0)
        res.cmd.bind_shadow_cascades = bind
    new = _render_pattern(mirhi, device, scene, array, f, prepare=through_the_new_call)
    array.destroy()
    assert calls == [0.0]
    for k in ("color", "depth"):
        assert rc.same_bits(old[k], new[k]), k
    assert len(np.unique(old["color"].reshape(-1, 4), axis=0)) > 4


# ---- 3. one scope, two draws ----------------------------------------------------------------------------------------------------------------
def test_blended_and_unblended_draws_share_a_scope(mirhi, scenes, oracle, device):
    """The receiver drawn twice in one scope: under a scissor over the left half with threshold 0.5, under one over the right half through
    bind_shadow_cascades.  Each half against its own model, and bit for bit against the one-draw frames; the scope's kernel is the blended one."""
    expect, plain, splits, _, _ = cases.pattern_expectation(scenes, oracle)
    size = 2 * csm_cases.PATTERN_LAYER
    half = size // 2
    array = _pattern_array(mirhi, device)
    one = csm_cases.pattern_scene(scenes, cascades=csm_cases.pattern_spec(scenes, splits))
    d = one.draws[0]
    both = dataclasses.replace(one, draws=[dataclasses.replace(d, scissor=(0, 0, half, size), csm_blend=cases.PATTERN_THRESHOLD),
                                           dataclasses.replace(d, scissor=(half, 0, half, size))])
    got = _render_pattern(mirhi, device, both, array)
    unblended = _render_pattern(mirhi, device, one, array)
    blended = _render_pattern(mirhi, device, dataclasses.replace(one, cascades=cases.pattern_spec(scenes, splits)), array)
    array.destroy()
    left = np.zeros((size, size), dtype=bool)
    left[:, :half] = True
    assert_close(got["color"], expect, "left half: blended", left)
    assert_close(got["color"], plain, "right half: unblended", ~left)
    assert rc.same_bits(got["color"][:, :half], blended["color"][:, :half]) and rc.same_bits(got["color"][:, half:], unblended["color"][:, half:])
    assert not rc.same_bits(blended["color"][:, half:], unblended["color"][:, half:])
    assert rc.same_bits(got["depth"], unblended["depth"])
    PBR = scenes.PROGRAM_MODEL_PBR
    shadowed, programs, kernel = _scope_plan(mirhi, [(PBR, 3), (PBR, 2)])
    assert (shadowed, programs) == (3, PROGS_CSM_BLEND) and kernel.startswith("raster_kernel_csm_blend<"), kernel


# ---- 4. MODEL_PBR_IBL with blended cascades -------------------------------------------------------------------------------------------------
def test_model_pbr_ibl_with_blended_cascades(mirhi, scenes, oracle, device):
    """The stabilised, blended ground case with metallic materials as MODEL_PBR (raster_kernel_csm_blend) and as MODEL_PBR_IBL under a zero
    environment (raster_kernel_ibl<.., 3>): the shadowed Cook-Torrance half agrees on every pixel and with the oracle's frames on the footprint
    classes; under a non-zero environment the ambient term is what it is without blending."""
    from test_gpu_ibl_shading import _ground_pair, _oracle_frames, _render
    base = cases.ground_scene(scenes, **cases.CLASS_SIZE)
    scene, out, ref = _ground_pair(mirhi, scenes, device, base, "blended cascades")
    lit, unlit = _oracle_frames(scenes, oracle, scene, cases.ground_scene(scenes, intensity=0.0, **cases.CLASS_SIZE), cascades=None)
    assert np.array_equal(out["prim"], lit["prim"])
    c = cases.ground_classes(scenes, oracle)
    assert_close(out["color"], unlit["rgba"], "zero IBL, blended cascades: inside the footprints", c["inside"])
    assert_close(out["color"], lit["rgba"], "zero IBL, blended cascades: outside the footprints", c["outside"])
    assert_close(out["color"], ref["color"], "zero IBL, blended cascades, against MODEL_PBR")
    # the blended frame is not the unblended one (the method has something to see) ...
    hard = dataclasses.replace(scene, cascades=dataclasses.replace(scene.cascades, blend_threshold=0.0))
    ref_hard = _render(mirhi, device, hard)
    assert float(np.abs(ref["color"][..., :3] - ref_hard["color"][..., :3]).max()) > 100 * RGB_TOL
    # ... and the ambient term is untouched: (environment - zero environment) is the same image with and without blending
    to_ibl = lambda sc, zero: dataclasses.replace(sc, draws=[dataclasses.replace(d, program=scenes.PROGRAM_MODEL_PBR_IBL) if d.program == scenes.PROGRAM_MODEL_PBR else d
                                                              for d in sc.draws], ibl=scenes.ibl_test_images(zero=zero))
    amb_blend = _render(mirhi, device, to_ibl(scene, False))["color"][..., :3].astype(np.float64) - out["color"][..., :3]
    amb_hard = _render(mirhi, device, to_ibl(hard, False))["color"][..., :3].astype(np.float64) - _render(mirhi, device, to_ibl(hard, True))["color"][..., :3]
    assert float(np.abs(amb_hard).max()) > 0.01
    assert_close(amb_blend, amb_hard, "the ambient term with and without blending")


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------------------
def test_stabilised_blended_ground_case_end_to_end(mirhi, scenes, oracle, device):
    """cascaded_ground_case(320, 240, map_size=256, stabilize=True, blend_threshold=0.1) -- 320 x 240, not 160 x 120: the smallest frame whose
    classes hold 300 pixels per cascade, csm_blend_cases.CLASS_SIZE --: four shadow scopes and the lit scope from one command buffer.  Ground pixels more than 3 texels -- of the coarser of the cascades the pixel samples -- inside a box's footprint equal the unlit oracle
    frame, those more than that outside every footprint the lit one, in every cascade."""
    scene = cases.ground_scene(scenes, **cases.CLASS_SIZE)
    c = cases.ground_classes(scenes, oracle)
    cases.assert_ground_conditions(c)
    lit = c["ref"]["rgba"]
    unlit = oracle.render(dataclasses.replace(cases.ground_scene(scenes, intensity=0.0, **cases.CLASS_SIZE), cascades=None), want_bgra8=False)["rgba"]
    res = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT)
    assert res.shadow_cmd is None
    res.render()
    frame = res.read()["color"]
    layers = res.cascade_array.read().copy()
    res.destroy()
    assert all((layers[k] < 1.0).any() for k in range(4)), "every layer holds casters"
    for k in range(4):
        sel = c["idx"] == k
        assert_close(frame, unlit, f"cascade {k}: inside the footprints", c["inside"] & sel)
        assert_close(frame, lit, f"cascade {k}: outside the footprints", c["outside"] & sel)


# ---- 6. a moving camera in a re-recorded frame loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("verify_idle", [False, True])
def test_moving_camera_in_a_rerecorded_frame_loop(mirhi, scenes, monkeypatch, verify_idle):
    """Six frames, two in flight: the camera moves a third of cascade 0's texel per frame along the light's x axis, every frame has its own
    uniform buffers (camera, casters' matrices, CSMParams), all share one cascade array, and every frame's command buffer is recorded again
    before it is submitted.  Every frame equals, bit for bit, a single-shot render of its pose."""
    if verify_idle:
        monkeypatch.setenv("MIRHI_VERIFY_IDLE", "1")
    a = cases.GROUND_ARGS
    view, proj, _, _ = cases.ground_view(scenes, a["width"], a["height"])
    texel0 = 2.0 * cases.stable_cascades(scenes, view, proj, a["map_size"]).half_extents[0] / a["map_size"]
    axis = cases.light_x_axis(scenes)
    poses = [cases.ground_view(scenes, a["width"], a["height"], offset=tuple(axis * (texel0 / 3.0 * f)))[2:] for f in range(6)]
    frames = [cases.ground_scene(scenes, eye=eye, target=target) for eye, target in poses]
    params = [f.cascades.params for f in frames]
    assert len({p[256:320] for p in params}) == 1, "cascade 3 does not move within two texels of cascade 0"
    assert 2 <= len({p[0:64] for p in params}) <= 3, "cascade 0 moves in whole texels: two texels in six frames"
    dev = mirhi.Device(0)
    try:
        dev.set_queue_lanes(2)
        single = []
        for sc in frames:
            r = mirhi.SceneResources(dev, sc, mirhi.Format.R32G32B32A32_SFLOAT)
            r.render()
            single.append(r.read()["color"])
            r.destroy()
        assert all(not np.array_equal(single[f], single[f + 1]) for f in range(5)), "the camera moves"
        array = mirhi.Image.array(dev, a["map_size"], a["map_size"], 4, mirhi.Format.D32_SFLOAT)
        res = [mirhi.SceneResources(dev, sc, mirhi.Format.R32G32B32A32_SFLOAT, cascade_array=array) for sc in frames]
        fences = [mirhi.Fence(dev, signaled=True) for _ in range(2)]
        for f in range(6):
            k = f % 2
            fences[k].wait()
            if f >= 2:
                assert np.array_equal(res[f - 2].color.read(), single[f - 2]), f"frame {f - 2} differs from its single-shot frame"
            fences[k].reset()
            res[f].record()
            res[f].render(fences[k])
        for f in (4, 5):
            fences[f % 2].wait()
            assert np.array_equal(res[f].color.read(), single[f]), f"frame {f} differs from its single-shot frame"
        for fe in fences:
            fe.destroy()
        for r in res:
            r.destroy()
        array.destroy()
    finally:
        dev.destroy()


# ---- 7. tile split ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["bands", "interleaved"])
def test_tile_split_of_the_blended_frame(mirhi, scenes, layout):
    scene, world = cases.ground_scene(scenes), 2
    dev = mirhi.Device(0)
    try:
        full = mirhi.SceneResources(dev, scene, mirhi.Format.R32G32B32A32_SFLOAT)
        full.render()
        frame, layers = full.read()["color"], full.cascade_array.read().copy()
        full.destroy()
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


# ---- 8. an area scope -----------------------------------------------------------------------------------------------------------------------------
def test_blended_pattern_inside_a_render_area(mirhi, scenes, oracle, device):
    """The pattern of test 1 inside an unaligned render area (the AREA instantiation of raster_kernel_csm_blend): the full-extent frame's bits inside
    the area, the sentinel outside -- colour, primitive ids and stored depth."""
    from test_gpu_render_area import assert_same, e1, render_into
    _, _, splits, _, _ = cases.pattern_expectation(scenes, oracle)
    scene = csm_cases.pattern_scene(scenes, cascades=cases.pattern_spec(scenes, splits))
    area = rc.areas(scene.width, scene.height)["b_unaligned"]
    assert area[0] % 32 and area[1] % 32 and (area[0] + area[2]) % 32 and (area[1] + area[3]) % 32
    sent = rc.sentinels(scene.width, scene.height)
    array = _pattern_array(mirhi, device)
    try:
        got, want, yard = e1(mirhi, device, scene, area, "float", sent, cascade_array=array)
        full = render_into(mirhi, device, scene, "float", sent, cascade_array=array)
    finally:
        device.wait_idle()
        array.destroy()
    assert_same(got, want, f"blended pattern in {area}")
    m = rc.mask(area, scene.width, scene.height)
    for k in ("color", "prim", "depth"):
        assert rc.same_bits(got[k][m], full[k][m]), f"{k}: the area scope differs from the full-extent frame inside the area"
        assert rc.same_bits(got[k][~m], sent["float" if k == "color" else k][~m]), f"{k}: a pixel outside the area was written"


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_blended_refusals(mirhi, scenes, device):
    M = mirhi

    def refused(fn, variant, text):
        with pytest.raises(M.RhiError) as e:
            fn()
        assert e.value.variant == variant and text in e.value.message, (e.value.variant, e.value.message)

    arr = M.Image.array(device, 64, 64, 4, M.Format.D32_SFLOAT)
    arr3 = M.Image.array(device, 64, 64, 3, M.Format.D32_SFLOAT)
    dimg = M.Image(device, 64, 64, M.Format.D32_SFLOAT)
    cimg = M.Image(device, 64, 64, M.Format.R32G32B32A32_SFLOAT)
    view = arr.layer_view(1)
    vb = M.Buffer.new_with_data(device, M.BufferUsage.Vertex, np.zeros(3 * 12, dtype=np.float32))
    ub = M.Buffer.new_with_data(device, M.BufferUsage.Uniform, np.zeros(336, dtype=np.uint8))
    small = M.Buffer.new_with_data(device, M.BufferUsage.Uniform, np.zeros(320, dtype=np.uint8))
    sb = M.Buffer(device, M.BufferUsage.Storage, 336)
    big = M.Buffer.new_with_data(device, M.BufferUsage.Uniform, np.zeros(208, dtype=np.uint8))

    def pbr():
        return (M.GraphicsPipelineBuilder().vertex_shader(M.Program.MODEL).fragment_shader(M.Program.MODEL_PBR).vertex_binding(48)
                .vertex_attributes(M.VERTEX_OFFSETS).color_attachment_format(M.Format.R32G32B32A32_SFLOAT).depth_attachment_format(M.Format.D32_SFLOAT))
    mp, bp = pbr().build(device), pbr().alpha_blend().build(device)
    dp, pp = pbr().fragment_discard_enable(True).build(device), pbr().depth_write_enable(False).build(device)
    cmd = M.CommandBuffer(device)

    def begin():
        cmd.begin()
        cmd.begin_rendering(cimg, depth=dimg)
        cmd.set_viewport(0.0, 0.0, 64.0, 64.0)
        cmd.set_scissor(0, 0, 64, 64)
        cmd.bind_vertex_buffers(0, [vb], [0])
        for s in (M.Slot.CAMERA, M.Slot.OBJECT, M.Slot.LIGHTS, M.Slot.MATERIAL, M.Slot.SHADOW_DATA):
            cmd.bind_uniform(s, big)
    begin()
    blend = cmd.bind_shadow_cascades_blended
    # the threshold
    for bad in (float("nan"), -0.1, 1.5, float("inf"), -float("inf")):
        refused(lambda: blend(arr, ub, 0, 0, bad), "InvalidHandle", "unsupported:")
        refused(lambda: cmd.bind_shadow_cascades(arr, ub, blend_threshold=bad), "InvalidHandle", "unsupported:")
    for good in (0.0, -0.0, 1.0, 0.5):
        blend(arr, ub, 0, 0, good)
    blend(None, None, 0, 0, float("nan"))                       # array == NULL unbinds, whatever else is passed
    # every refusal of a cascade binding
    refused(lambda: blend(dimg, ub, 0, 0, 0.5), "InvalidHandle", "an image array (mirhi_image_create_array)")
    refused(lambda: blend(view, ub, 0, 0, 0.5), "InvalidHandle", "not a layer view")
    refused(lambda: blend(arr3, ub, 0, 0, 0.5), "InvalidHandle", "CASCADE_COUNT = 4 layers (got 3)")
    refused(lambda: blend(arr, small, 0, 0, 0.5), "InvalidHandle", "CSMParams range 320 smaller than 336")
    refused(lambda: blend(arr, ub, 16, 0, 0.5), "InvalidHandle", "CSMParams range 320 smaller than 336")
    refused(lambda: blend(arr, ub, 0, 400, 0.5), "InvalidHandle", "exceeds buffer")
    refused(lambda: blend(arr, sb, 0, 0, 0.5), "InvalidHandle", "uniform buffer")
    # ... and of a cascaded draw
    blend(arr, ub, 0, 0, 0.5)
    cmd.bind_texture(M.TextureSlot.SHADOW_MAP, view)
    cmd.bind_pipeline(mp)
    refused(lambda: cmd.draw(3), "InvalidHandle", "both a shadow map (MIRHI_TEXTURE_SHADOW_MAP) and shadow cascades")
    cmd.bind_texture(M.TextureSlot.SHADOW_MAP, None)
    for p in (bp, dp, pp):
        cmd.bind_pipeline(p)
        refused(lambda: cmd.draw(3), "InvalidHandle", "unsupported: shadow cascades with blending, fragment discard, a predicate depth state")
    cmd.bind_pipeline(mp)
    cmd.draw(3)                                                 # a blended cascaded draw ...
    cmd.bind_shadow_cascades(arr, ub)
    cmd.draw(3)                                                 # ... and an unblended one share the scope
    blend(None)
    cmd.bind_texture(M.TextureSlot.SHADOW_MAP, dimg)
    refused(lambda: cmd.draw(3), "InvalidHandle", "a single shadow map and draws with shadow cascades in one rendering scope")
    cmd.bind_texture(M.TextureSlot.SHADOW_MAP, None)
    # begin and reset clear the binding with its threshold: a blending pipeline, refused under cascades, records again
    blend(arr, ub, 0, 0, 0.5)
    cmd.bind_pipeline(bp)
    refused(lambda: cmd.draw(3), "InvalidHandle", "unsupported: shadow cascades with blending")
    cmd.end_rendering()
    cmd.end()
    begin()
    cmd.bind_pipeline(bp)
    cmd.draw(3)
    blend(arr, ub, 0, 0, 0.5)
    refused(lambda: cmd.draw(3), "InvalidHandle", "unsupported: shadow cascades with blending")
    cmd.reset()
    begin()
    cmd.bind_pipeline(bp)
    cmd.draw(3)
    cmd.end_rendering()
    cmd.end()
    cmd.destroy()
    view.destroy()
    for o in (arr, arr3, dimg, cimg, vb, ub, small, sb, big, mp, bp, dp, pp):
        o.destroy()
