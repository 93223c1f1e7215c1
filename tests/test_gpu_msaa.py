"""4x MSAA on the GPU (include/mirhi.h "4x MSAA") against the yardstick of tests/msaa_cases.py: sample s of the multisampled frame is the
unchanged oracle's 1x frame under a viewport moved by (1/2 - sx, 1/2 - sy).  Visibility (the winner of every sample, the depth of sample 0) is compared
bit for bit at every texel of every case; colour is the stated recombination ((c0 + c1) + (c2 + c3)) * 0.25 of per-sample colours taken from the clear colour,
from the 1x GPU frame where the winner owns the centre, and otherwise from the extrapolating model (TRIANGLE: float64; MODEL_FULL / MODEL_PBR: the oracle's
frame of a coplanar carrier quad).  Targets are 64 x 64 and 96 x 80 (3 x 3 tiles, the last row partial)."""
import os

import numpy as np
import pytest

import msaa_cases as mc

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4            # tests/test_gpu_parity.py: linear float colour
CODE_TOL = 1              # ... and sRGB8, in codes
NONE = mc.NONE


def _render(mirhi, device, scene, samples=1, fmt=None, **kw):
    fmt = mirhi.Format.R32G32B32A32_SFLOAT if fmt is None else fmt
    res = mirhi.SceneResources(device, scene, fmt, want_prim=True, want_depth=True, samples=samples, **kw)
    res.render()
    out = res.read()
    res.destroy()
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def case_scenes(scenes):
    return mc.cases(scenes)


@pytest.fixture(scope="module")
def frames(mirhi, scenes, oracle, device, case_scenes):
    """per case, rendered once and left unchanged: the multisampled GPU frame and the 1x GPU frame (float target), the four moved-viewport oracle frames"""
    out = {}
    for name, scene in case_scenes.items():
        prim, depth, one = mc.oracle_samples(scenes, oracle, mc.oracle_scene(scenes, name, scene))
        out[name] = dict(ms=_render(mirhi, device, scene, samples=4), one=_render(mirhi, device, scene), oracle_prim=prim, oracle_depth=depth, oracle_one=one)
    return out


CASES = ["random-less", "random-lequal", "random-greater", "random-gequal", "slivers", "sample-edges", "tile-corner", "full-tile-65", "full-tile-193",
         "full-tile-300", "big-list", "near-clip", "scissor", "biased-clamped"]


def test_case_list_is_complete(case_scenes):
    assert list(case_scenes) == CASES


# 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_visibility(frames, case_scenes, name):
    """the 4 W x H id image and the SAMPLE_ZERO depth resolve: every texel, bit for bit"""
    fr, scene = frames[name], case_scenes[name]
    got, want = fr["ms"]["prim"], fr["oracle_prim"]
    assert got.shape == want.shape == (scene.height, scene.width, 4)
    assert (want != NONE).sum() > 0
    diff = got != want
    assert not diff.any(), f"{name}: {int(diff.sum())} sample winners differ; first (y, x, s) = {np.argwhere(diff)[0]}: got {got[diff][0]} want {want[diff][0]}"
    want_depth = mc.biased_depth(scene.width, scene.height)[:, :, 0] if name == "biased-clamped" else fr["oracle_depth"][:, :, 0]
    want_depth = np.where(want[:, :, 0] != NONE, want_depth, np.float32(scene.clear_depth))
    bad = _bits(fr["ms"]["depth"]) != _bits(want_depth)
    assert not bad.any(), f"{name}: {int(bad.sum())} sample-0 depths differ; first (y, x) = {np.argwhere(bad)[0]}: got {fr['ms']['depth'][bad][0]!r} want {want_depth[bad][0]!r}"


def test_slivers_are_invisible_at_1x_and_visible_at_4x(frames):
    fr = frames["slivers"]
    assert (fr["one"]["prim"] == NONE).all()
    lit = (fr["ms"]["prim"] != NONE).sum(axis=2)
    assert lit.max() == 1 and (lit == 1).sum() > 300
    clear = np.array(mc.CLEAR, dtype=np.float32)
    assert (np.abs(fr["ms"]["color"][lit == 1] - clear).max(axis=1) > 0.01).all()      # a quarter of the sliver's colour reached the resolved pixel


# 2 ---------------------------------------------------------------------------------------------------------------------------------------
def _expected_linear(scenes, scene, fr):
    """[H, W, 4] binary32 and the mask of pixels whose four samples share the 1x frame's winner"""
    prim, one = fr["oracle_prim"], fr["one"]
    same = (prim == one["prim"][:, :, None]).all(axis=2)
    cols = np.empty(prim.shape + (4,), dtype=np.float32)
    cols[:] = np.array(scene.clear_color, dtype=np.float32)
    cache = {}
    for s in range(4):
        owns = (prim[:, :, s] == one["prim"]) & (prim[:, :, s] != NONE)
        cols[:, :, s][owns] = one["color"][owns]
        other = (prim[:, :, s] != NONE) & ~owns
        for pid in np.unique(prim[:, :, s][other]):
            if int(pid) not in cache:
                cache[int(pid)] = scenes.msaa_triangle_colour(scene, int(pid)).astype(np.float32)
            m = other & (prim[:, :, s] == pid)
            cols[:, :, s][m] = cache[int(pid)][m]
    return scenes.msaa_resolve(cols[:, :, 0], cols[:, :, 1], cols[:, :, 2], cols[:, :, 3], np.float32), same


@pytest.mark.parametrize("name", CASES)
def test_colour_float(scenes, frames, case_scenes, name):
    fr, scene = frames[name], case_scenes[name]
    want, same = _expected_linear(scenes, scene, fr)
    got = fr["ms"]["color"]
    assert same.sum() > 0 and (~same).sum() > 0
    bad = (_bits(got) != _bits(fr["one"]["color"])).any(axis=2) & same
    assert not bad.any(), f"{name}: {int(bad.sum())} pixels whose four samples share the 1x winner differ from the 1x frame; first {np.argwhere(bad)[0]}"
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{name}: {int((~same).sum())} mixed pixels, max |dRGBA| = {float(err.max()):.3e}")
    assert float(err.max()) < RGB_TOL, f"{name}: max |dRGBA| = {float(err.max())} at {np.unravel_index(err.argmax(), err.shape)}"


def _identity_camera(scenes):
    eye = np.eye(4, dtype=np.float32)
    return scenes.camera_ubo(eye, eye, (0.0, 0.0, -2.0))


def _model_quad(scenes, rect, program, mips):
    """A MODEL_FULL / MODEL_PBR quad over the window rectangle `rect` under msaa_cases.VIEWPORT with an identity camera (clip = position, w = 1), whose
    attributes are AFFINE functions of the window position -- the same functions for every rectangle, so that a quad is a sub-rectangle of any larger one"""
    x0, y0, x1, y1 = rect
    win = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)
    pos = np.concatenate([(win - 128.0) / 128.0, np.full((4, 1), 0.5)], axis=1).astype(np.float32)
    uv = (win / 16.0).astype(np.float32)                                   # 16 px per repeat: minified, the chain's level 1 to 2
    nrm = np.tile(np.array([0, 0, -1], dtype=np.float32), (4, 1))
    tan = np.tile(np.array([1, 0, 0, 1], dtype=np.float32), (4, 1))
    rng = np.random.default_rng(0x5A4D0003)
    tex = scenes.Texture(rng.integers(0, 256, (64, 64, 4), dtype=np.uint8), mips=mips, srgb=mips)
    tex.rgba8[..., 3] = 255
    pbr = program == scenes.PROGRAM_MODEL_PBR
    material = scenes.pbr_material_ubo((0.9, 0.8, 0.7, 1.0), 0.2, 0.5, 0.9, has_base_color=True) if pbr else scenes.material_ubo((0.9, 0.8, 0.7, 1.0), 0.0, 0.4, 0.8)
    return scenes.DrawSpec(vertices=scenes._pack_vertex48(pos, nrm, uv, tan), stride=48, count=6, indices=np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32), program=program,
                           cull_mode=scenes.CULL_NONE, viewport=mc.VIEWPORT, camera=_identity_camera(scenes), object=scenes.object_ubo(np.eye(4, dtype=np.float32)),
                           light=scenes.light_ubo(direction=(0.3, 0.2, 1.0), intensity=0.8, color=(1.0, 0.95, 0.9), num_point=1),
                           point_lights=scenes.point_light((0.2, -0.1, -1.0), 6.0, (0.7, 0.8, 1.0), 3.0), material=material, albedo_map=tex)


FOREGROUND = (20.25, 14.375, 70.6875, 60.8125)       # on the 1/256 grid, off the pixel grid: partial coverage all along the silhouette
CARRIER = (4.0, 4.0, 92.0, 76.0)


@pytest.mark.parametrize("program, mips", [("PROGRAM_MODEL_FULL", False), ("PROGRAM_MODEL_PBR", True)])
def test_colour_model_programs_against_the_carrier_quad(mirhi, scenes, oracle, device, program, mips):
    """A foreground quad drawn as a sub-rectangle of a larger coplanar carrier quad with the same affine attributes: the oracle's 1x frame of the CARRIER is the
    fragment program's colour at every pixel centre near the silhouette, covered by the foreground or not.  PROGRAM_MODEL_PBR: an sRGB albedo with a mip chain."""
    prog = getattr(scenes, program)
    scene = mc._scene(scenes, "model-fg", 96, 80, _model_quad(scenes, FOREGROUND, prog, mips))
    carrier = mc._scene(scenes, "model-carrier", 96, 80, _model_quad(scenes, CARRIER, prog, mips))
    assert mc.condition_holds(scenes, scene) == (6, 0)
    prim, _, _ = mc.oracle_samples(scenes, oracle, scene)
    ref = oracle.render(carrier, want_bgra8=False)["rgba"]
    ms, one = _render(mirhi, device, scene, samples=4), _render(mirhi, device, scene)
    assert np.array_equal(ms["prim"], prim)
    cols = np.where((prim != NONE)[..., None], ref[:, :, None, :], np.array(scene.clear_color, dtype=np.float32))
    want = scenes.msaa_resolve(cols[:, :, 0], cols[:, :, 1], cols[:, :, 2], cols[:, :, 3], np.float32)
    same = (prim == one["prim"][:, :, None]).all(axis=2)
    partial = ~same
    assert partial.sum() > 150 and (same & (one["prim"] != NONE)).sum() > 1500
    bad = (_bits(ms["color"]) != _bits(one["color"])).any(axis=2) & same
    assert not bad.any(), f"{int(bad.sum())} fully covered pixels differ from the 1x frame"
    err = np.abs(ms["color"] - want) / np.maximum(1.0, np.abs(want))
    print(f"{program}: {int(partial.sum())} silhouette pixels, max |dRGBA| = {float(err.max()):.3e}")
    assert float(err.max()) < RGB_TOL, f"max |dRGBA| = {float(err.max())} at {np.unravel_index(err.argmax(), err.shape)}"
    # the same frame on the B8G8R8A8_SRGB target: the expected linear colour, encoded once
    got8 = _render(mirhi, device, scene, samples=4, fmt=mirhi.Format.B8G8R8A8_SRGB)
    assert np.array_equal(got8["prim"], prim)
    d = np.abs(got8["color"].astype(np.int32) - _encode(oracle, want).astype(np.int32))
    print(f"{program}: sRGB8 max code difference {int(d.max())}")
    assert d.max() <= CODE_TOL, f"sRGB8 differs by {int(d.max())} codes at {np.unravel_index(d.argmax(), d.shape)}"


# 3 ---------------------------------------------------------------------------------------------------------------------------------------
def _encode(oracle, linear):
    """[H, W, 4] linear RGBA -> B8G8R8A8_SRGB bytes: the oracle's OETF on R, G, B, alpha to UNORM8"""
    L = oracle.lib()
    lut = np.vectorize(lambda v: L.oracle_srgb8(float(v)), otypes=[np.uint8])
    rgb = lut(linear[..., :3])
    a = np.rint(np.clip(linear[..., 3], 0.0, 1.0) * 255.0).astype(np.uint8)
    return np.stack([rgb[..., 2], rgb[..., 1], rgb[..., 0], a], axis=2)


@pytest.mark.parametrize("name", CASES)
def test_colour_srgb8_encodes_the_average_once(mirhi, scenes, oracle, device, frames, case_scenes, name):
    fr, scene = frames[name], case_scenes[name]
    want, _ = _expected_linear(scenes, scene, fr)
    got = _render(mirhi, device, scene, samples=4, fmt=mirhi.Format.B8G8R8A8_SRGB)["color"]
    d = np.abs(got.astype(np.int32) - _encode(oracle, want).astype(np.int32))
    print(f"{name}: max code difference {int(d.max())}")
    assert d.max() <= CODE_TOL, f"{name}: sRGB8 differs by {int(d.max())} codes at {np.unravel_index(d.argmax(), d.shape)}"


def test_srgb8_averages_linear_values_not_bytes(mirhi, scenes, device):
    """a white quad on black whose vertical edge lies at x = k + 1/2: two samples of four.  Linear 0.5 encodes to 188; the average of the bytes 0 and 255 would be 127 or 128"""
    white = [[1.0, 1.0, 1.0]] * 6
    scene = mc._scene(scenes, "black-white", 64, 64, mc.draw(scenes, mc.quad(20.5, 8.0, 50.0, 56.0, 0.5), white), clear_color=(0.0, 0.0, 0.0, 1.0))
    out = _render(mirhi, device, scene, samples=4, fmt=mirhi.Format.B8G8R8A8_SRGB)
    assert list(out["prim"][30, 20] != NONE) == [False, True, False, True]
    assert list(out["color"][30, 19]) == [0, 0, 0, 255] and list(out["color"][30, 21]) == [255, 255, 255, 255]
    edge = out["color"][8:56, 20]
    assert (np.abs(edge[:, :3].astype(np.int32) - 188) <= CODE_TOL).all() and (edge[:, 3] == 255).all(), edge[0]


# 4 ---------------------------------------------------------------------------------------------------------------------------------------
def _loop_scene(scenes, dx):
    return mc._scene(scenes, "loop", 96, 80, [_model_quad(scenes, (FOREGROUND[0] + dx, FOREGROUND[1], FOREGROUND[2] + dx, FOREGROUND[3]), scenes.PROGRAM_MODEL_FULL, False)])


def _loop_object(scenes, step):
    m = np.eye(4, dtype=np.float32)
    m[3, 0] = np.float32(step * 3.0 / 128.0)          # [col, row]: a translation in clip x by 3 px a frame
    return scenes.object_ubo(m)


@pytest.mark.parametrize("submit_thread", [False, True])
def test_rerecorded_frame_loop(mirhi, scenes, device, monkeypatch, submit_thread):
    """two frames in flight, each re-recorded every frame, under MIRHI_VERIFY_IDLE=1 (every re-recording checks that the frame before left the workspace re-armed),
    a uniform (the object matrix) that changes every frame: every frame equals its single-shot render"""
    monkeypatch.setenv("MIRHI_VERIFY_IDLE", "1")
    steps = 6
    singles = []
    for step in range(steps):
        sc = _loop_scene(scenes, 0.0)
        sc.draws[0].object = _loop_object(scenes, step)
        singles.append(_render(mirhi, device, sc, samples=4))
    assert not np.array_equal(singles[0]["prim"], singles[1]["prim"])
    device.set_submit_thread(submit_thread)
    frames_ = [mirhi.SceneResources(device, _loop_scene(scenes, 0.0), want_prim=True, want_depth=True, samples=4) for _ in range(2)]
    fences = [mirhi.Fence(device) for _ in frames_]
    try:
        for step in range(0, steps, 2):
            for j, (f, fe) in enumerate(zip(frames_, fences)):
                f.draw_state[0]["object"].write_data(0, _loop_object(scenes, step + j))
                f.record()
                f.render(fe)
            for j, (f, fe) in enumerate(zip(frames_, fences)):
                fe.wait(); fe.reset()
                out = f.read()
                for key in ("color", "prim", "depth"):
                    assert np.array_equal(out[key].view(np.uint32), singles[step + j][key].view(np.uint32)), (step + j, key)
    finally:
        device.wait_idle()
        device.set_submit_thread(False)
        for f, fe in zip(frames_, fences):
            f.destroy(); fe.destroy()


# 5 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(os.environ.get("MIRHI_NATIVE_DISPATCH") == "0", reason="native dispatch switched off for this run")
def test_both_dispatch_paths(mirhi, scenes, frames, case_scenes):
    dev = mirhi.Device(0, stream=0)
    outs, used = [], []
    try:
        res = mirhi.SceneResources(dev, case_scenes["random-less"], want_prim=True, want_depth=True, samples=4)
        fence = mirhi.Fence(dev)
        for native in (False, True):
            dev.set_native_dispatch(native)
            before = dev.stats().native_dispatches
            res.render(fence)
            fence.wait(); fence.reset()
            used.append((dev.dispatch_path(), dev.stats().native_dispatches - before))
            outs.append(res.read())
        res.destroy(); fence.destroy()
    finally:
        dev.destroy()
    assert used[0][1] == 0 and used[1][1] > 0 and used[1][0].startswith("native:"), used
    for out in outs:
        for key in ("color", "prim", "depth"):
            assert np.array_equal(out[key].view(np.uint32), frames["random-less"]["ms"][key].view(np.uint32)), key


# 6 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2])
def test_three_scopes_in_one_command_buffer(mirhi, scenes, device, frames, case_scenes, lanes):
    """a 1x sky scope (a SKYBOX segment) into image A, a multisampled scope resolving into image B with a depth resolve, a 1x overlay scope that LOADs B and the resolved depth: the
    overlay sees what the multisampled scope resolved (ordering goes by the resolve images).  lanes = 2: the overlay is a command buffer of its own on the other lane."""
    scene = case_scenes["random-less"]
    back = scenes.skybox_case(96, 80)
    sky_alone = _render(mirhi, device, back)
    assert np.abs(sky_alone["color"][..., :3] - np.array(back.clear_color[:3], dtype=np.float32)).max() > 0.05      # the sky draws something
    # the overlay: a quad at depth 0.4375 over the left half, LESS against the resolved sample-0 depth
    overlay = mc._scene(scenes, "overlay", 96, 80, mc.draw(scenes, mc.quad(0.0, 0.0, 48.0, 80.0, 0.4375), [[1.0, 0.0, 1.0]] * 6))
    fmt = mirhi.Format.R32G32B32A32_SFLOAT
    alone = _render(mirhi, device, overlay)          # the overlay's own colours (a flat triangle's interpolated colour need not be its vertex colour to the bit)
    device.set_queue_lanes(lanes)
    try:
        a = mirhi.SceneResources(device, back, fmt)
        b = mirhi.SceneResources(device, scene, fmt, want_depth=True, samples=4)
        c = mirhi.SceneResources(device, overlay, fmt, color_image=b.color, depth_image=b.depth, color_load_op=mirhi.LoadOp.LOAD, depth_load_op=mirhi.LoadOp.LOAD)
        cmds = [mirhi.CommandBuffer(device) for _ in range(lanes)]
        for lane, cmd in enumerate(cmds):
            cmd.set_queue_lane(lane)
        recorders = [(a, cmds[0]), (b, cmds[0]), (c, cmds[-1])]
        for cmd in cmds:
            cmd.begin_reusable()
        for res, cmd in recorders:       # each helper records its one scope into the shared command buffer
            res.record_scopes(cmd)
        for cmd in cmds:
            cmd.end()
        fence = mirhi.Fence(device)
        for rep in range(2):
            if lanes == 1:
                device.submit(cmds, fence)
            else:
                device.submit([cmds[0]]); device.submit([cmds[1]], fence)
            fence.wait(); fence.reset()
            device.wait_idle()
            got_a, got_b, got_depth = a.color.read(), b.color.read(), b.depth.read()
            ms = frames["random-less"]["ms"]
            wins = (np.arange(96)[None, :] < 48) & (np.float32(0.4375) < ms["depth"])
            assert wins.sum() > 500 and (~wins[:, :48]).sum() > 100
            want_b = np.where(wins[..., None], alone["color"], ms["color"])
            want_depth = np.where(wins, np.float32(0.4375), ms["depth"])
            assert np.array_equal(_bits(got_b), _bits(want_b)), rep
            assert np.array_equal(_bits(got_depth), _bits(want_depth)), rep
            assert np.array_equal(_bits(got_a), _bits(sky_alone["color"])), rep
        fence.destroy()
        for cmd in cmds:
            cmd.destroy()
        c.destroy(); b.destroy(); a.destroy()
    finally:
        device.wait_idle()
        device.set_queue_lanes(1)


# 7 ---------------------------------------------------------------------------------------------------------------------------------------
def _refused(mirhi, phrase, fn, *args, **kw):
    with pytest.raises(mirhi.RhiError) as e:
        fn(*args, **kw)
    assert phrase in str(e.value), (phrase, str(e.value))


def test_refusals(mirhi, scenes, device):
    F, S = mirhi.Format, scenes
    for n, phrase in ((1, "use mirhi_image_create"), (2, "unsupported: sample count"), (8, "unsupported: sample count"), (0, "unsupported: sample count")):
        _refused(mirhi, phrase, mirhi.Image.multisampled, device, 64, 64, F.R32G32B32A32_SFLOAT, n)
    _refused(mirhi, "unsupported: multisampled images of format", mirhi.Image.multisampled, device, 64, 64, F.R8G8B8A8_UNORM, 4)
    ms, msd, ms8 = (mirhi.Image.multisampled(device, 64, 64, f) for f in (F.R32G32B32A32_SFLOAT, F.D32_SFLOAT, F.B8G8R8A8_SRGB))
    one, oned, prim, small = mirhi.Image(device, 64, 64, F.R32G32B32A32_SFLOAT), mirhi.Image(device, 64, 64, F.D32_SFLOAT), mirhi.Image(device, 256, 64, F.R32_UINT), mirhi.Image(device, 32, 64, F.R32G32B32A32_SFLOAT)
    buf = mirhi.Buffer(device, mirhi.BufferUsage.Storage, 64 * 64 * 16)
    ubo = mirhi.Buffer(device, mirhi.BufferUsage.Uniform, 512)
    cmd = mirhi.CommandBuffer(device)
    objs = [ms, msd, ms8, one, oned, prim, small, buf, ubo]
    try:
        assert ms.samples == 4 and one.samples == 1 and mirhi.lib().mirhi_image_size_bytes(ms.handle) == 0 and not mirhi.lib().mirhi_image_device_ptr(ms.handle)
        # the image is an attachment and nothing else
        M = "multisampled"
        _refused(mirhi, M, ms.upload, np.zeros((64, 64, 4), dtype=np.float32))
        with pytest.raises(mirhi.RhiError) as e:
            mirhi.check(mirhi.lib().mirhi_image_read(ms.handle, np.zeros(16, dtype=np.uint8).ctypes.data, 16))
        assert M in str(e.value)
        _refused(mirhi, M, ms.layer_view, 0)
        _refused(mirhi, M, ms8.generate_mips)
        _refused(mirhi, M, ms8.set_max_anisotropy, 4)
        _refused(mirhi, M, ms8.set_sampler, address_u=mirhi.AddressMode.CLAMP_TO_EDGE)
        cmd.begin()
        for slot in range(5):
            _refused(mirhi, M, cmd.bind_texture, slot, ms8)
        _refused(mirhi, M, cmd.bind_texture, mirhi.TextureSlot.SHADOW_MAP, msd)
        _refused(mirhi, M, cmd.bind_shadow_cascades, msd, ubo)
        _refused(mirhi, M, cmd.bind_ibl, ms, ms, ms)
        _refused(mirhi, M, cmd.bind_skybox, ms)
        _refused(mirhi, M, cmd.copy_image_to_buffer, ms, buf, [(0, 0, 0, 0, (0, 0), (64, 64))])
        _refused(mirhi, M, cmd.copy_buffer_to_image, buf, ms, [(0, 0, 0, 0, (0, 0), (64, 64))])
        _refused(mirhi, M, cmd.copy_image, ms, one, [(0, (0, 0), 0, (0, 0), (64, 64))])
        _refused(mirhi, M, cmd.copy_image, one, ms, [(0, (0, 0), 0, (0, 0), (64, 64))])
        blit = [(0, ((0, 0), (64, 64)), 0, ((0, 0), (64, 64)))]
        _refused(mirhi, M, cmd.blit_image, ms, one, blit)
        _refused(mirhi, M, cmd.blit_image, one, ms, blit)
        _refused(mirhi, M, cmd.clear_color_image, ms, (0.0, 0.0, 0.0, 1.0))
        _refused(mirhi, M, cmd.clear_depth_stencil_image, msd, 1.0)
        # the scope
        _refused(mirhi, "mirhi_cmd_begin_rendering_resolve", cmd.begin_rendering, ms)
        _refused(mirhi, "needs a multisampled color_image", cmd.begin_rendering_resolve, one, one)
        T = "unsupported: multisampled attachments are transient"
        _refused(mirhi, T, cmd.begin_rendering_resolve, ms, one, color_load_op=mirhi.LoadOp.LOAD)
        _refused(mirhi, T, cmd.begin_rendering_resolve, ms, one, color_store_op=mirhi.StoreOp.STORE)
        _refused(mirhi, T, cmd.begin_rendering_resolve, ms, one, depth=msd, depth_load_op=mirhi.LoadOp.LOAD)
        _refused(mirhi, T, cmd.begin_rendering_resolve, ms, one, depth=msd, depth_store_op=mirhi.StoreOp.STORE)
        _refused(mirhi, "needs a color_resolve_image", cmd.begin_rendering_resolve, ms, None)
        _refused(mirhi, "MIRHI_RESOLVE_AVERAGE", cmd.begin_rendering_resolve, ms, one, color_mode=mirhi.ResolveMode.SAMPLE_ZERO)
        _refused(mirhi, "format and extent", cmd.begin_rendering_resolve, ms, small)
        _refused(mirhi, "format and extent", cmd.begin_rendering_resolve, ms8, one)
        _refused(mirhi, "multisampled itself", cmd.begin_rendering_resolve, ms, ms)
        _refused(mirhi, "single-sampled depth attachment", cmd.begin_rendering_resolve, ms, one, depth=oned)
        _refused(mirhi, "MIRHI_RESOLVE_SAMPLE_ZERO", cmd.begin_rendering_resolve, ms, one, depth=msd, depth_resolve=oned, depth_mode=mirhi.ResolveMode.AVERAGE)
        _refused(mirhi, "must be D32_SFLOAT", cmd.begin_rendering_resolve, ms, one, depth=msd, depth_resolve=one)
        _refused(mirhi, "4 * width x height", cmd.begin_rendering_resolve, ms, one, prim_id=small)
        _refused(mirhi, "unsupported: a partial render area", cmd.begin_rendering_resolve, ms, one, render_area=(0, 0, 32, 64))
        device.set_profiling(mirhi.Profile.FRAGMENTS)
        try:
            _refused(mirhi, "unsupported: fragment statistics", cmd.begin_rendering_resolve, ms, one)
        finally:
            device.set_profiling(0)
        device.set_tile_split(0, 2)
        try:
            _refused(mirhi, "unsupported: a multisampled scope on a split device", cmd.begin_rendering_resolve, ms, one)
        finally:
            device.set_tile_split(0, 1)

        # pipelines and draws
        def pipe(samples=4, program=mirhi.Program.TRIANGLE, **kw):
            model = program != mirhi.Program.TRIANGLE
            b = (mirhi.GraphicsPipelineBuilder().vertex_shader(mirhi.Program.MODEL if model and program != mirhi.Program.SKYBOX else program).fragment_shader(program)
                 .vertex_binding(48 if model else 24).vertex_attributes(mirhi.VERTEX_OFFSETS if model else mirhi.TRIANGLE_VERTEX_OFFSETS)
                 .color_attachment_format(F.R32G32B32A32_SFLOAT).depth_attachment_format(F.D32_SFLOAT).cull_mode(mirhi.CullMode.NONE).rasterization_samples(samples))
            if program == mirhi.Program.SKYBOX:
                b.vertex_binding(0).vertex_attributes(())
            for k, v in kw.items():
                getattr(b, k)(*v) if isinstance(v, tuple) else getattr(b, k)(v)
            p = b.build(device)
            objs.append(p)
            return p
        _refused(mirhi, "unsupported sample count 2", pipe, 2)
        _refused(mirhi, "unsupported sample count 8", pipe, 8)
        vb = mirhi.Buffer.new_with_data(device, mirhi.BufferUsage.Vertex, np.zeros((6, 12), dtype=np.float32))
        objs.append(vb)

        def draw_with(p, scope_samples=4):
            if scope_samples == 4:
                cmd.begin_rendering_resolve(ms, one, depth=msd, depth_resolve=oned, prim_id=prim)
            else:
                cmd.begin_rendering(one, depth=oned)
            try:
                cmd.set_viewport(0.0, 0.0, 64.0, 64.0); cmd.set_scissor(0, 0, 64, 64)
                cmd.bind_pipeline(p); cmd.bind_vertex_buffers(0, [vb], [0])
                cmd.draw(3, 1, 0, 0)
            finally:
                cmd.end_rendering()
        draw_with(pipe(4))
        with pytest.raises(mirhi.RhiError) as e:
            draw_with(pipe(1), 4)
        assert "rasterization_samples 1" in str(e.value) and "sample count 4" in str(e.value)
        with pytest.raises(mirhi.RhiError) as e:
            draw_with(pipe(4), 1)
        assert "rasterization_samples 4" in str(e.value) and "sample count 1" in str(e.value)
        _refused(mirhi, "unsupported: blending", draw_with, pipe(4, alpha_blend=()))
        _refused(mirhi, "unsupported: fragment_discard_enable", draw_with, pipe(4, fragment_discard_enable=True))
        for kw in (dict(depth_write_enable=False), dict(depth_test_enable=False), dict(depth_compare_op=mirhi.CompareOp.Equal), dict(depth_compare_op=mirhi.CompareOp.Always),
                   dict(depth_compare_op=mirhi.CompareOp.Never)):
            _refused(mirhi, "unsupported: a predicate depth state", draw_with, pipe(4, **kw))
        _refused(mirhi, "unsupported: a SKYBOX draw", draw_with, pipe(4, program=mirhi.Program.SKYBOX, depth_write_enable=False, depth_compare_op=mirhi.CompareOp.LessOrEqual))
        shadow_pipe = (mirhi.GraphicsPipelineBuilder().vertex_shader(mirhi.Program.SHADOW).fragment_shader(mirhi.Program.SHADOW).vertex_binding(48)
                       .vertex_attributes(mirhi.SHADOW_VERTEX_OFFSETS).color_attachment_format(F.UNDEFINED).depth_attachment_format(F.D32_SFLOAT)
                       .rasterization_samples(4).build(device))
        objs.append(shadow_pipe)
        _refused(mirhi, "unsupported: a SHADOW draw in a multisampled scope", draw_with, shadow_pipe)
        # a second depth state inside the scope
        cmd.begin_rendering_resolve(ms, one)
        cmd.set_viewport(0.0, 0.0, 64.0, 64.0); cmd.set_scissor(0, 0, 64, 64)
        cmd.bind_vertex_buffers(0, [vb], [0])
        cmd.bind_pipeline(pipe(4)); cmd.draw(3, 1, 0, 0)
        cmd.bind_pipeline(pipe(4, depth_compare_op=mirhi.CompareOp.LessOrEqual))
        _refused(mirhi, "unsupported: a depth state change", cmd.draw, 3, 1, 0, 0)
        cmd.end_rendering()
        cmd.end()
    finally:
        device.wait_idle()
        cmd.destroy()
        for o in reversed(objs):
            o.destroy()


def test_program_and_shadow_refusals(mirhi, scenes, device):
    """a shadowed draw, a cascaded draw and a MODEL_PBR_IBL draw in a multisampled scope, through the scene helper (whose constructor records the scene)"""
    for scene, phrase in ((scenes.shadowed_ground_case(96, 80, map_size=64), "unsupported: a shadowed or cascaded draw in a multisampled scope"),
                          (scenes.cascaded_ground_case(96, 80, map_size=64), "unsupported: a shadowed or cascaded draw in a multisampled scope"),
                          (scenes.ibl_facets_case(96, 80), "unsupported: a MODEL_PBR_IBL draw in a multisampled scope")):
        res = mirhi.SceneResources.__new__(mirhi.SceneResources)
        try:
            with pytest.raises(mirhi.RhiError) as e:
                res.__init__(device, scene, samples=4)
            assert phrase in str(e.value), str(e.value)
        finally:
            res.destroy()
