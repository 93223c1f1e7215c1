"""Multiview depth scopes on the GPU (include/mirhi.h "Multiview depth scopes"): one scope that renders its SHADOW draws into several
layers of a D32 array equals, bit for bit in every layer, the single-view scopes of the same build (multiview_cases states the equivalence) -- over masks,
load ops, depth states, the raster kernel's routes, six views, both dispatch paths, constants rewritten between submits, the cascaded-ground frame on one
and two lanes, a re-recorded frame loop -- and every refusal by its text."""
import numpy as np
import pytest

import multiview_cases as mc
from test_gpu_shadow import _casters, _oracle_depth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def base(mirhi, scenes, device):
    """The casters of test_gpu_shadow under four light matrices, uploaded once; the single-view CLEAR render of all four layers (the reference of several tests)."""
    ls, casters = _casters(scenes)
    bufs = mc.CasterBuffers(mirhi, device, casters)
    mats = mc.view_matrices(ls, 6)
    pipe = mc.shadow_pipeline(mirhi, scenes, device)
    single = mc.run_single(mirhi, scenes, device, bufs, mats, 0b1111, mc.sentinels(), pipe)
    single.setflags(write=False)
    yield dict(ls=ls, casters=casters, bufs=bufs, mats=mats, pipe=pipe, single=single)
    pipe.destroy()
    bufs.destroy()


# ---- 1. masks, against the single-view scopes and the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [0b1111, 0b0001, 0b1010])
def test_mask_equals_single_view_scopes_and_the_oracle(mirhi, scenes, oracle, device, base, mask):
    start = mc.sentinels()
    multi = mc.run_multiview(mirhi, scenes, device, base["bufs"], base["mats"], mask, start, base["pipe"])
    single = base["single"].copy()
    for v in range(mc.LAYERS):
        if not (mask >> v) & 1:
            single[v] = start[v]
    mc.assert_equivalent(multi, single, start, mask, f"mask {mask:#06b}")
    for v in range(mc.LAYERS):
        if (mask >> v) & 1:
            ref, covered = _oracle_depth(scenes, oracle, base["mats"][v], base["casters"], mc.SIZE, scenes.CMP_LESS, 1.0, scenes.CULL_NONE)
            assert covered.sum() >= 500, f"layer {v}: only {covered.sum()} covered pixels"
            assert np.array_equal(multi[v].view(np.uint32)[covered], ref.view(np.uint32)[covered]), f"layer {v} differs from the oracle's depth"
            assert np.all(multi[v][~covered] == np.float32(1.0))
    for v in range(mc.LAYERS):
        for u in range(v):
            assert not np.array_equal(base["single"][v], base["single"][u]), "two views render the same image: the test could not tell them apart"


# ---- 2. load ops ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("load", [False, True])
def test_load_ops(mirhi, scenes, device, base, load):
    start = mc.sentinels()
    args = (mirhi, scenes, device, base["bufs"], base["mats"], 0b1101, start, base["pipe"])
    multi, single = mc.run_multiview(*args, load=load), mc.run_single(*args, load=load)
    mc.assert_equivalent(multi, single, start, 0b1101, "LOAD" if load else "CLEAR")
    if load:      # texels no caster reaches (or reaches behind the loaded depth) keep what the layer held
        assert all((multi[v] == start[v]).any() and (multi[v] < start[v]).any() for v in (0, 2, 3))


# ---- 3. depth states: both KEYED instantiations, a biased pipeline ----------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["less", "greater", "lequal_biased"])
def test_depth_states(mirhi, scenes, device, base, state):
    compare, clear, bias = {"less": (scenes.CMP_LESS, 1.0, None), "greater": (scenes.CMP_GREATER, 0.0, None),
                            "lequal_biased": (scenes.CMP_LESS_OR_EQUAL, 1.0, (1.25, 0.0, 1.75))}[state]
    pipe = mc.shadow_pipeline(mirhi, scenes, device, compare=compare, bias=bias)
    start = mc.sentinels()
    try:
        args = (mirhi, scenes, device, base["bufs"], base["mats"], 0b1111, start, pipe)
        multi, single = mc.run_multiview(*args, clear=clear), mc.run_single(*args, clear=clear)
    finally:
        pipe.destroy()
    mc.assert_equivalent(multi, single, start, 0b1111, state)
    if state != "less":
        assert not np.array_equal(multi, base["single"]), f"{state}: the state changed nothing"


# ---- 4. the raster kernel's routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", mc.ROUTES)
def test_raster_routes(mirhi, scenes, device, base, route):
    casters, scissor = mc.route_casters(route)
    bufs = mc.CasterBuffers(mirhi, device, casters)
    mats = mc.view_matrices(np.eye(4, dtype=np.float32))
    start = mc.sentinels()
    try:
        args = (mirhi, scenes, device, bufs, mats, 0b1111, start, base["pipe"])
        multi, single = mc.run_multiview(*args, scissor=scissor), mc.run_single(*args, scissor=scissor)
    finally:
        bufs.destroy()
    mc.assert_equivalent(multi, single, start, 0b1111, route)
    assert device.stats().last_status == 0
    if scissor:
        x, y, w, h = scissor
        outside = np.ones((mc.SIZE, mc.SIZE), dtype=bool)
        outside[y:y + h, x:x + w] = False
        assert np.all(multi[:, outside] == np.float32(1.0)) and (multi[:, ~outside] < 1.0).any()


# ---- 5. six views ---------------------------------------------------------------------------------------------------------------------------------
def test_six_views(mirhi, scenes, device, base):
    start = mc.sentinels(6)
    args = (mirhi, scenes, device, base["bufs"], base["mats"], 0b111111, start, base["pipe"])
    multi, single = mc.run_multiview(*args, instances=2), mc.run_single(*args, instances=2)
    mc.assert_equivalent(multi, single, start, 0b111111, "six views")
    assert np.array_equal(multi[:4], base["single"]), "an instanced draw changes nothing a single instance does not draw"


# ---- 6. dispatch paths ------------------------------------------------------------------------------------------------------------------------
def test_one_launch_per_stage_on_both_dispatch_paths(mirhi, scenes, device, base):
    start = mc.sentinels()
    args = (mirhi, scenes, device, base["bufs"], base["mats"], 0b1111, start, base["pipe"])
    device.set_profiling(mirhi.Profile.TIMING)           # timed dispatches go out as HIP launches
    try:
        device.reset_kernel_times()
        hip = mc.run_multiview(*args)
        launches = {k: device.kernel_time(k)[1] for k in (mirhi.Kernel.VERTEX, mirhi.Kernel.GEOMETRY, mirhi.Kernel.RASTER)}
    finally:
        device.set_profiling(0)
        device.reset_kernel_times()
    assert launches == {mirhi.Kernel.VERTEX: 1, mirhi.Kernel.GEOMETRY: 1, mirhi.Kernel.RASTER: 1}, launches
    assert np.array_equal(hip.view(np.uint32), base["single"].view(np.uint32))
    before = device.stats()
    plain = mc.run_multiview(*args)
    after = device.stats()
    assert np.array_equal(plain.view(np.uint32), hip.view(np.uint32)), "the two dispatch paths differ"
    native = device.dispatch_path().startswith("native")
    assert after.native_dispatches - before.native_dispatches == (3 if native else 0), device.dispatch_path()
    assert after.frames_submitted - before.frames_submitted == 1, "the scope counts once"
    tris = sum(int(i.size) // 3 for _, i, _ in base["casters"])
    assert after.triangles_submitted - before.triangles_submitted == 4 * tris, "its triangles count once per view"


# ---- 7. the constants are read when the scope executes ------------------------------------------------------------------------------------------
def test_view_constants_are_read_at_execution(mirhi, scenes, device, base):
    start = mc.sentinels()
    array = mirhi.Image.array(device, mc.SIZE, mc.SIZE, mc.LAYERS, mirhi.Format.D32_SFLOAT)
    consts = mirhi.Buffer.new_with_data(device, mirhi.BufferUsage.Uniform, mc.view_constants(base["mats"], mc.LAYERS))
    objs = [consts]
    cmd = mirhi.CommandBuffer(device)
    cmd.begin_reusable()
    cmd.begin_rendering_multiview(array, 0b1111, consts, mc.OFFSET, mc.STRIDE)
    mc.record_draws(mirhi, scenes, cmd, device, base["pipe"], base["bufs"], mc.DECOY, mc.SIZE, None, objs)
    cmd.end_rendering()
    cmd.end()
    try:
        array.upload(start)
        device.submit([cmd]); device.wait_idle()
        first = array.read().copy()
        swapped = [base["mats"][v] for v in (2, 3, 0, 1)]
        consts.write_data(0, mc.view_constants(swapped, mc.LAYERS))
        device.submit([cmd]); device.wait_idle()
        second = array.read().copy()
    finally:
        cmd.destroy()
        for o in objs:
            o.destroy()
        array.destroy()
    assert np.array_equal(first.view(np.uint32), base["single"].view(np.uint32))
    want = mc.run_single(mirhi, scenes, device, base["bufs"], swapped, 0b1111, start, base["pipe"])
    assert np.array_equal(second.view(np.uint32), want.view(np.uint32)), "the second submit did not see the rewritten matrices"
    assert np.array_equal(want[0], base["single"][2]) and not np.array_equal(second, first)


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------------------------
def test_cascaded_ground_frame_equals_the_four_scope_form(mirhi, scenes):
    """cascaded_ground_case: the multiview scope feeding the lit MODEL_PBR scope -- in one command buffer, and in a command buffer of its own on another
    queue lane ("ordering is by the parent") -- gives the frame of the four-scope form, bit for bit, and the same four layers."""
    scene = scenes.cascaded_ground_case(160, 120, map_size=256)
    dev = mirhi.Device(0)
    try:
        dev.set_queue_lanes(2)
        four = mirhi.SceneResources(dev, scene, mirhi.Format.R32G32B32A32_SFLOAT)
        four.render()
        frame, layers = four.read()["color"], four.cascade_array.read().copy()
        four.destroy()
        assert all((layers[k] < 1.0).any() for k in range(4)), "every layer holds casters"
        one = mirhi.SceneResources(dev, scene, mirhi.Format.R32G32B32A32_SFLOAT, multiview=True)
        one.render()
        got, got_layers = one.read()["color"], one.cascade_array.read().copy()
        one.destroy()
        assert np.array_equal(got_layers.view(np.uint32), layers.view(np.uint32)), "one lane: the layers differ"
        assert np.array_equal(got, frame), "one lane: the frame differs from the four-scope form"
        two = mirhi.SceneResources(dev, scene, mirhi.Format.R32G32B32A32_SFLOAT, shadow_cmd=True, multiview=True)
        two.shadow_cmd.set_queue_lane(1)
        two.cmd.set_queue_lane(0)
        for _ in range(3):
            two.render()
            assert np.array_equal(two.read()["color"], frame), "two lanes: the frame differs from the four-scope form"
        two.destroy()
    finally:
        dev.destroy()


def test_rerecorded_frame_loop_under_verify_idle(mirhi, scenes, base, monkeypatch):
    """Two frames in flight, each command buffer reset and re-recorded every frame with another mask and another number of draws, under MIRHI_VERIFY_IDLE=1:
    every re-recording checks that the frame before left the view slots' counters and page tables re-armed."""
    monkeypatch.setenv("MIRHI_VERIFY_IDLE", "1")
    dev = mirhi.Device(0)
    objs = []
    try:
        dev.set_queue_lanes(2)
        pipe = mc.shadow_pipeline(mirhi, scenes, dev)
        sets = [mc.CasterBuffers(mirhi, dev, base["casters"][:n]) for n in (1, 2)]
        start = mc.sentinels()
        singles = [mc.run_single(mirhi, scenes, dev, b, base["mats"], 0b1111, start, pipe) for b in sets]
        assert not np.array_equal(singles[0], singles[1])
        consts = mirhi.Buffer.new_with_data(dev, mirhi.BufferUsage.Uniform, mc.view_constants(base["mats"], mc.LAYERS))
        arrays = [mirhi.Image.array(dev, mc.SIZE, mc.SIZE, mc.LAYERS, mirhi.Format.D32_SFLOAT) for _ in range(2)]
        expect = [start.copy(), start.copy()]
        for a in arrays:
            a.upload(start)
        cmds = [mirhi.CommandBuffer(dev) for _ in range(2)]
        fences = [mirhi.Fence(dev, signaled=True) for _ in range(2)]
        frames = [(0b1111, 1), (0b0101, 0), (0b0010, 1), (0b1011, 0), (0b1111, 0), (0b0001, 1), (0b1110, 1), (0b0110, 0)]
        for f, (mask, which) in enumerate(frames):
            k = f % 2
            fences[k].wait()
            if f >= 2:
                assert np.array_equal(arrays[k].read().view(np.uint32), expect[k].view(np.uint32)), f"frame {f - 2} differs"
            fences[k].reset()
            cmds[k].reset()
            cmds[k].begin()
            cmds[k].begin_rendering_multiview(arrays[k], mask, consts, mc.OFFSET, mc.STRIDE)
            mc.record_draws(mirhi, scenes, cmds[k], dev, pipe, sets[which], mc.DECOY, mc.SIZE, None, objs)
            cmds[k].end_rendering()
            cmds[k].end()
            dev.submit([cmds[k]], fences[k])
            for v in range(mc.LAYERS):
                if (mask >> v) & 1:
                    expect[k][v] = singles[which][v]
        for k in range(2):
            fences[k].wait()
            assert np.array_equal(arrays[k].read().view(np.uint32), expect[k].view(np.uint32)), f"the last frame of slot {k} differs"
        for o in fences + cmds + arrays + [consts, pipe] + objs:
            o.destroy()
        for b in sets:
            b.destroy()
    finally:
        dev.destroy()


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_multiview_refusals(mirhi, scenes, base):
    M = mirhi
    dev = M.Device(0)

    def refused(fn, text):
        with pytest.raises(M.RhiError) as e:
            fn()
        assert e.value.variant == "InvalidHandle" and "unsupported: " + text in e.value.message, (e.value.variant, e.value.message)

    try:
        arr = M.Image.array(dev, 64, 64, 4, M.Format.D32_SFLOAT)
        arr12 = M.Image.array(dev, 16, 16, 12, M.Format.D32_SFLOAT)
        dimg = M.Image(dev, 64, 64, M.Format.D32_SFLOAT)
        cimg = M.Image(dev, 64, 64, M.Format.R32G32B32A32_SFLOAT)
        pimg = M.Image(dev, 64, 64, M.Format.R32_UINT)
        msd = M.Image.multisampled(dev, 64, 64, M.Format.D32_SFLOAT, 4)
        view = arr.layer_view(1)
        ub = M.Buffer.new_with_data(dev, M.BufferUsage.Uniform, np.zeros(80 * 3 + 64, dtype=np.uint8))
        vb = M.Buffer.new_with_data(dev, M.BufferUsage.Vertex, np.zeros(3 * 12, dtype=np.float32))
        cam = M.Buffer.new_with_data(dev, M.BufferUsage.Uniform, np.zeros(208, dtype=np.uint8))
        cmd = M.CommandBuffer(dev)

        def begin(*a, **kw):
            cmd.reset()
            cmd.begin()
            cmd.begin_rendering_multiview(*a, **kw)

        refused(lambda: begin(arr, 0b1111, ub, 0, 80, color=cimg), "a multiview scope is depth-only")
        refused(lambda: begin(arr, 0b1111, ub, 0, 80, prim_id=pimg), "a multiview scope is depth-only")
        refused(lambda: begin(dimg, 0b1, ub, 0, 80), "a multiview scope renders into an image array")
        refused(lambda: begin(view, 0b1, ub, 0, 80), "a multiview scope renders into an image array")
        refused(lambda: begin(None, 0b1, ub, 0, 80), "a multiview scope renders into an image array")
        refused(lambda: begin(msd, 0b1, ub, 0, 80), "a multisampled depth image in a multiview scope")
        refused(lambda: begin(arr, 0b1111, ub, 0, 80, depth_load_op=M.LoadOp.DONT_CARE), "the depth load op of a multiview scope is CLEAR or LOAD")
        refused(lambda: begin(arr, 0b1111, ub, 0, 80, depth_store_op=M.StoreOp.DONT_CARE), "a multiview scope must store its depth")
        refused(lambda: begin(arr, 0, ub, 0, 80), "an empty view mask")
        refused(lambda: begin(arr12, 0b111111111, ub, 0, 16), "more than 8 views")
        refused(lambda: begin(arr, 0b10001, ub, 0, 64), "a view mask bit at or above the array's layer count")
        refused(lambda: begin(arr, 0b1111, None, 0, 80), "a multiview scope without view_constants")
        refused(lambda: begin(arr, 0b1111, ub, 0, 48), "view_stride must be at least 64 and a multiple of 16")
        refused(lambda: begin(arr, 0b1111, ub, 0, 72), "view_stride must be at least 64 and a multiple of 16")
        refused(lambda: begin(arr, 0b1111, ub, 8, 80), "view_offset must be a multiple of 16")
        refused(lambda: begin(arr, 0b1111, ub, 16, 80), "the view_constants buffer is too short")
        refused(lambda: begin(arr, 0b1111, ub, 1 << 40, 80), "the view_constants buffer is too short")
        refused(lambda: begin(arr, 0b1111, ub, 0, 80, render_area=(0, 0, 32, 64)), "a partial render area in a multiview scope")
        begin(arr, 0b0111, ub, 16, 80)                            # (three views fit behind the offset)
        cmd.set_viewport(0.0, 0.0, 64.0, 64.0)
        cmd.set_scissor(0, 0, 64, 64)
        cmd.bind_vertex_buffers(0, [vb], [0])
        cmd.bind_uniform(M.Slot.CAMERA, cam)
        cmd.bind_uniform(M.Slot.OBJECT, cam)
        model = (M.GraphicsPipelineBuilder().vertex_shader(M.Program.MODEL).fragment_shader(M.Program.MODEL).vertex_binding(48)
                 .vertex_attributes(M.VERTEX_OFFSETS).color_attachment_format(M.Format.R32G32B32A32_SFLOAT).depth_attachment_format(M.Format.D32_SFLOAT).build(dev))
        cmd.bind_pipeline(model)
        refused(lambda: cmd.draw(3), "only SHADOW draws may be recorded in a multiview scope")
        cmd.bind_pipeline(base_pipe := mc.shadow_pipeline(M, scenes, dev))
        cmd.draw(3)
        cmd.end_rendering()
        cmd.end()
        # the array is still no attachment of an ordinary scope
        with pytest.raises(M.RhiError) as e:
            cmd.reset(); cmd.begin(); cmd.begin_rendering(None, depth=arr, depth_store_op=M.StoreOp.STORE)
        assert "an image array is not an attachment" in e.value.message
        dev.set_profiling(M.Profile.FRAGMENTS)
        refused(lambda: begin(arr, 0b1111, ub, 0, 80), "fragment statistics of a multiview scope")
        dev.set_profiling(0)
        dev.set_tile_split(1, 2)
        refused(lambda: begin(arr, 0b1111, ub, 0, 80), "a multiview scope on a split device")
        dev.set_tile_split(0, 1)
        cmd.reset()
        cmd.destroy()
        view.destroy()
        for o in (arr, arr12, dimg, cimg, pimg, msd, ub, vb, cam, model, base_pipe):
            o.destroy()
    finally:
        dev.destroy()
