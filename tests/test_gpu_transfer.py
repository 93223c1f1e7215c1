"""The recorded transfer commands on the GPU (include/mirhi.h "Transfer commands"): copies byte for byte against numpy slicing, the
blit against the numpy model of tests/transfer_cases.py (exact index choice; float32 error against the float64 model; 8-bit bytes within one LSB and
equal wherever the model decides), clears, and how the commands behave in a command buffer: order, both dispatch paths, the plan cache, a frame loop
under MIRHI_VERIFY_IDLE, queue lanes, mirhi_buffer_write, the tile split, the submit thread, the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import transfer_cases as tc

pytestmark = pytest.mark.gpu
W, H = 37, 29                          # the copy cases' image: odd, no multiple of a tile, rows of 148 / 592 bytes
ALL_FORMATS = (tc.BGRA8_SRGB, tc.RGBA32F, tc.D32, tc.RGBA8_UNORM, tc.R32_UINT, tc.RGBA8_SRGB)


class Rig:
    """Images and buffers that live as long as one test, and command buffers recorded by a function."""

    def __init__(self, mirhi, device):
        self.m, self.dev, self.objs = mirhi, device, []

    def image(self, w, h, fmt, data=None):
        img = self.m.Image(self.dev, w, h, fmt)
        self.objs.append(img)
        if data is not None:
            img.upload(data)
        return img

    def buffer(self, size, data=None):
        buf = self.m.Buffer(self.dev, self.m.BufferUsage.Staging, size)
        self.objs.append(buf)
        if data is not None:
            buf.upload(data)
        return buf

    def keep(self, obj):
        self.objs.append(obj)
        return obj

    def run(self, record, fence=None, cmd=None, lane=None):
        """Records a one-time command buffer with `record(cmd)`, submits it and waits."""
        own = cmd is None
        cmd = cmd or self.m.CommandBuffer(self.dev)
        if lane is not None:
            cmd.set_queue_lane(lane)
        cmd.begin()
        record(cmd)
        cmd.end()
        self.dev.submit([cmd], fence)
        if fence is not None:
            fence.wait(); fence.reset()
        self.dev.wait_idle()
        if own:
            cmd.destroy()

    def destroy(self):
        self.dev.wait_idle()
        for o in reversed(self.objs):
            o.destroy()


@pytest.fixture
def rig(mirhi, device):
    r = Rig(mirhi, device)
    yield r
    r.destroy()


def level_bytes(img_array):
    return tc.as_bytes(img_array)


# ---- copies: buffers --------------------------------------------------------------------------------------------------------------------------
def test_copy_buffer_sizes_and_offsets(rig):
    """Head, body and tail of the vector path: sizes 1 .. 4099 at co-aligned and not co-aligned offsets; bytes outside the range stay."""
    rng = np.random.default_rng(5)
    n = 4099 + 64
    src_bytes = rng.integers(0, 256, n, dtype=np.uint8)
    src = rig.buffer(n, src_bytes)
    cases = [(size, so, do) for size in (1, 3, 15, 16, 17, 255, 4099) for so, do in ((0, 0), (1, 2), (16, 4), (3, 3))]
    dsts = [rig.buffer(n, np.full(n, 0xA5, dtype=np.uint8)) for _ in cases]
    # (one command buffer: every case is a command of its own)
    rig.run(lambda cmd: [cmd.copy_buffer(src, d, [(so, do, size)]) for d, (size, so, do) in zip(dsts, cases)])
    for d, (size, so, do) in zip(dsts, cases):
        want = np.full(n, 0xA5, dtype=np.uint8)
        want[do:do + size] = src_bytes[so:so + size]
        assert np.array_equal(d.read(0, n), want), (size, so, do)


def test_copy_buffer_regions_and_one_buffer(rig):
    rng = np.random.default_rng(6)
    a = rng.integers(0, 256, 2048, dtype=np.uint8)
    src, dst = rig.buffer(2048, a), rig.buffer(2048, np.zeros(2048, dtype=np.uint8))
    rig.run(lambda cmd: cmd.copy_buffer(src, dst, [(0, 100, 50), (64, 1024, 512), (700, 3, 17)]))
    want = np.zeros(2048, dtype=np.uint8)
    want[100:150], want[1024:1536], want[3:20] = a[0:50], a[64:576], a[700:717]
    assert np.array_equal(dst.read(0, 2048), want)
    rig.run(lambda cmd: cmd.copy_buffer(src, src, [(0, 1024, 1000), (1000, 2030, 10)]))      # disjoint ranges of one buffer
    want = a.copy()
    want[1024:2024], want[2030:2040] = a[0:1000], a[1000:1010]
    assert np.array_equal(src.read(0, 2048), want)


# ---- copies: buffer <-> image -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ALL_FORMATS)
def test_buffer_image_copies(rig, fmt):
    bpp = tc.texel_bytes(fmt)
    texels = tc.raw_texels(fmt, W, H)
    stored = level_bytes(texels).reshape(H, W, bpp)
    img = rig.image(W, H, fmt, texels)
    # image -> buffer: whole and tight; a region with row length 40 / image height 31 at an unaligned offset
    tight, pitched = rig.buffer(W * H * bpp), rig.buffer(bpp + 40 * 31 * bpp, np.full(bpp + 40 * 31 * bpp, 0x5A, dtype=np.uint8))
    rig.run(lambda cmd: (cmd.copy_image_to_buffer(img, tight, [(0, 0, 0, 0, (0, 0), (W, H))]),
                         cmd.copy_image_to_buffer(img, pitched, [(bpp, 40, 31, 0, (5, 3), (13, 11))])))
    assert np.array_equal(tight.read(0, W * H * bpp).reshape(H, W, bpp), stored)
    got = pitched.read(0, bpp + 40 * 31 * bpp)
    want = np.full((40 * 31 + 1, bpp), 0x5A, dtype=np.uint8)
    rows = want[1:].reshape(31, 40, bpp)
    rows[:11, :13] = stored[3:14, 5:18]
    assert np.array_equal(got.reshape(-1, bpp), want)
    # buffer -> another image: the whole image back (round trip), then a region from the pitched buffer over it
    back = rig.image(W, H, fmt, np.zeros_like(texels))
    rig.run(lambda cmd: (cmd.copy_buffer_to_image(tight, back, [(0, 0, 0, 0, (0, 0), (W, H))]),
                         cmd.copy_buffer_to_image(pitched, back, [(bpp, 40, 31, 0, (20, 10), (13, 11))])))
    want_img = stored.copy()
    want_img[10:21, 20:33] = stored[3:14, 5:18]
    assert np.array_equal(level_bytes(back.read()).reshape(H, W, bpp), want_img)


def test_layers_and_levels(rig, mirhi):
    m = mirhi
    array = rig.keep(m.Image.array(rig.dev, 16, 16, 4, tc.D32))
    layers = np.random.default_rng(8).random((4, 16, 16)).astype(np.float32)
    array.upload(layers)
    v1, v3 = array.layer_view(1), array.layer_view(3)
    try:
        rig.run(lambda cmd: cmd.copy_image(v1, v3, [(0, (0, 0), 0, (0, 0), (16, 16))]))
        want = layers.copy()
        want[3] = layers[1]
        assert np.array_equal(array.read(), want)
    finally:
        rig.dev.wait_idle()
        v1.destroy(); v3.destroy()
    # level 1 of a 37 x 29 chain to a buffer and back into level 1 of another image
    texels = tc.raw_texels(tc.RGBA8_UNORM, W, H, seed=3)
    a, b = rig.image(W, H, tc.RGBA8_UNORM, texels), rig.image(W, H, tc.RGBA8_UNORM, np.zeros_like(texels))
    a.generate_mips(); b.generate_mips()
    lw, lh = W >> 1, H >> 1
    buf, check = rig.buffer(lw * lh * 4), rig.buffer(lw * lh * 4)
    rig.run(lambda cmd: (cmd.copy_image_to_buffer(a, buf, [(0, 0, 0, 1, (0, 0), (lw, lh))]),
                         cmd.copy_buffer_to_image(buf, b, [(0, 0, 0, 1, (0, 0), (lw, lh))]),
                         cmd.copy_image_to_buffer(b, check, [(0, 0, 0, 1, (0, 0), (lw, lh))])))
    want = tc.mip_level(texels, 1)
    assert np.array_equal(buf.read(0, lw * lh * 4).reshape(lh, lw, 4), want)
    assert np.array_equal(check.read(0, lw * lh * 4).reshape(lh, lw, 4), want)
    assert not b.read().any()                                                # level 0 of the second image was not touched


@pytest.mark.parametrize("sf, df", [(tc.BGRA8_SRGB, tc.RGBA8_UNORM), (tc.D32, tc.D32), (tc.RGBA32F, tc.RGBA32F)])
def test_copy_image_with_offsets(rig, sf, df):
    bpp = tc.texel_bytes(sf)
    src_t, dst_t = tc.raw_texels(sf, W, H, seed=1), tc.raw_texels(df, 48, 40, seed=2)
    src, dst = rig.image(W, H, sf, src_t), rig.image(48, 40, df, dst_t)
    rig.run(lambda cmd: cmd.copy_image(src, dst, [(0, (5, 3), 0, (9, 7), (13, 11)), (0, (0, 0), 0, (30, 25), (18, 15))]))
    want = level_bytes(dst_t).reshape(40, 48, bpp).copy()
    s = level_bytes(src_t).reshape(H, W, bpp)
    want[7:18, 9:22] = s[3:14, 5:18]
    want[25:40, 30:48] = s[0:15, 0:18]
    assert np.array_equal(level_bytes(dst.read()).reshape(40, 48, bpp), want)


# ---- blit -------------------------------------------------------------------------------------------------------------------------------------
def _blit(rig, sf, df, srect, drect, linear, dw=tc.DST_W, dh=tc.DST_H, seed=0):
    """(stored destination texels after the blit, the decoded source in float64, in float32)"""
    texels = tc.source(sf, seed)
    src = rig.image(tc.SRC_W, tc.SRC_H, sf, texels)
    init = np.full((dh, dw, 4), 0.125 if df == tc.RGBA32F else 0x33, dtype=np.float32 if df == tc.RGBA32F else np.uint8)
    dst = rig.image(dw, dh, df, init)
    rig.run(lambda cmd: cmd.blit_image(src, dst, [(0, srect, 0, drect)], rig.m.Filter.LINEAR if linear else rig.m.Filter.NEAREST))
    out = dst.read()
    x0, x1 = sorted((drect[0][0], drect[1][0])); y0, y1 = sorted((drect[0][1], drect[1][1]))
    outside = np.ones((dh, dw), dtype=bool)
    outside[y0:y1, x0:x1] = False
    assert np.array_equal(out[outside], init[outside])                      # texels outside the destination rectangle stay
    return out[y0:y1, x0:x1], tc.decode(texels, sf), tc.decode(texels, sf, np.float32)


WHOLE_SRC = ((0, 0), (tc.SRC_W, tc.SRC_H))
WHOLE_DST = ((0, 0), (tc.DST_W, tc.DST_H))


def _check_8bit(out, m64, df, what):
    want = tc.encode(m64, df)
    skip = tc.undecided(m64, df)
    share = skip.mean()
    off = np.abs(out.astype(np.int32) - want.astype(np.int32))
    print(f"BLIT8 {what}: {100 * share:.2f} % undecided, {int((off[~skip] != 0).sum())} decided channels differ, max |LSB| {int(off.max())}")
    assert share <= 0.02, what
    assert off.max() <= 1, what
    assert np.array_equal(out[~skip], want[~skip]), what


@pytest.mark.parametrize("fmt", tc.BLIT_FORMATS)
def test_nearest_one_to_one_same_format_and_flips(rig, fmt):
    texels = tc.source(fmt)
    same = ((0, 0), (tc.SRC_W, tc.SRC_H))
    out, _, _ = _blit(rig, fmt, fmt, same, same, False, tc.SRC_W, tc.SRC_H)
    assert np.array_equal(out, texels)
    for drect, want in ((((tc.SRC_W, 0), (0, tc.SRC_H)), texels[:, ::-1]), (((0, tc.SRC_H), (tc.SRC_W, 0)), texels[::-1]),
                        (((tc.SRC_W, tc.SRC_H), (0, 0)), texels[::-1, ::-1])):
        out, _, _ = _blit(rig, fmt, fmt, same, drect, False, tc.SRC_W, tc.SRC_H)
        assert np.array_equal(out, want), drect


@pytest.mark.parametrize("dw, dh", [(48, 40), (37, 29)])
def test_nearest_rescale_takes_the_models_texels(rig, dw, dh):
    """Exact: the index is formed in integers on both sides, no arithmetic touches the values."""
    for fmt in (tc.RGBA32F, tc.RGBA8_UNORM):
        out, s64, _ = _blit(rig, fmt, fmt, WHOLE_SRC, ((0, 0), (dw, dh)), False, dw, dh)
        assert np.array_equal(out, tc.encode(tc.blit(s64, WHOLE_SRC, ((0, 0), (dw, dh)), False), fmt)), fmt
        _, ix, _, _, _ = tc.axis_taps(0, dw, 0, tc.SRC_W, tc.SRC_W, False)
        _, iy, _, _, _ = tc.axis_taps(0, dh, 0, tc.SRC_H, tc.SRC_H, False)
        assert np.array_equal(out, tc.source(fmt)[iy[:, None], ix[None, :]]), fmt


@pytest.mark.parametrize("sf", tc.BLIT_FORMATS)
@pytest.mark.parametrize("df", tc.BLIT_FORMATS)
def test_nearest_one_to_one_every_format_pair(rig, sf, df):
    same = ((0, 0), (tc.SRC_W, tc.SRC_H))
    out, s64, _ = _blit(rig, sf, df, same, same, False, tc.SRC_W, tc.SRC_H)
    if df == tc.RGBA32F:
        assert np.array_equal(out, tc.decode(tc.source(sf), sf, np.float32))      # decode alone: a table entry or byte / 255 (float32: x * (1 / 255))
    else:
        _check_8bit(out, s64, df, f"nearest {sf} -> {df}")


@pytest.mark.parametrize("name, srect, drect", [("37x29", WHOLE_SRC, WHOLE_DST), ("flipped 37x29", WHOLE_SRC, ((tc.DST_W, tc.DST_H), (0, 0))),
                                                ("sub-region (3, 2)-(16, 13)", WHOLE_SRC, ((3, 2), (16, 13)))])
def test_linear_into_a_float_destination(rig, name, srect, drect):
    """BLIT <case>: E32 / bound / GPU are printed for DESIGN.md 8g."""
    out, s64, s32 = _blit(rig, tc.RGBA32F, tc.RGBA32F, srect, drect, True)
    m64, m32 = tc.blit(s64, srect, drect, True), tc.blit(s32, srect, drect, True, np.float32)
    e32, gpu = tc.rel_err(m32, m64), tc.rel_err(out, m64)
    print(f"BLIT linear float {name}: E32 {e32:.3e} bound {tc.bound_for(e32):.3e} GPU {gpu:.3e}")
    assert gpu <= tc.bound_for(e32)


@pytest.mark.parametrize("sf", [tc.RGBA8_SRGB, tc.BGRA8_SRGB, tc.RGBA8_UNORM, tc.RGBA32F])
@pytest.mark.parametrize("df", [tc.RGBA8_UNORM, tc.BGRA8_SRGB, tc.RGBA8_SRGB])
def test_linear_into_8_bit_destinations(rig, sf, df):
    for name, drect in (("37x29", WHOLE_DST), ("13x11", ((3, 2), (16, 13)))):      # (non-integer ratios only: a 1:2 ratio makes exact ties)
        out, s64, _ = _blit(rig, sf, df, WHOLE_SRC, drect, True)
        _check_8bit(out, tc.blit(s64, WHOLE_SRC, drect, True), df, f"linear {sf} -> {df} {name}")


def _scope(cmd, res, color, clear, load=None):
    """One rendering scope of res.scene's draws (TRIANGLE program, no uniforms) into `color`."""
    m, s = res.m, res.scene
    cmd.begin_rendering(color, clear_color=clear, color_load_op=m.LoadOp.CLEAR if load is None else load)
    for st in res.draw_state:
        cmd.set_viewport(0.0, 0.0, float(s.width), float(s.height)); cmd.set_scissor(0, 0, s.width, s.height)
        cmd.bind_pipeline(st["pipe"]); cmd.bind_vertex_buffers(0, [st["vb"]], [0])
        cmd.draw(st["draw"].count, 1, st["draw"].first, 0)
    cmd.end_rendering()


@pytest.fixture
def triangle(mirhi, scenes, device):
    """hello_triangle at 100 x 75 on both colour formats: the resources (pipelines, vertex buffer, targets) and the frames rendered directly."""
    scene = scenes.hello_triangle(100, 75)
    res = {fmt: mirhi.SceneResources(device, scene, fmt) for fmt in (tc.RGBA32F, tc.BGRA8_SRGB)}
    frames = {}
    for fmt, r in res.items():
        r.m = mirhi
        r.render()
        frames[fmt] = r.read()["color"]
    yield scene, res, frames
    for r in res.values():
        r.destroy()


def test_float_frame_blitted_to_srgb8_equals_the_direct_frame(rig, triangle):
    scene, res, frames = triangle
    out8 = rig.image(100, 75, tc.BGRA8_SRGB, np.zeros((75, 100, 4), dtype=np.uint8))
    f = res[tc.RGBA32F]
    whole = ((0, 0), (100, 75))
    rig.run(lambda cmd: (_scope(cmd, f, f.color, scene.clear_color), cmd.blit_image(f.color, out8, [(0, whole, 0, whole)], rig.m.Filter.NEAREST)))
    assert np.array_equal(out8.read(), frames[tc.BGRA8_SRGB])


# ---- clears -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", tc.BLIT_FORMATS)
def test_clear_color_image(rig, fmt):
    color = (1.75, -0.25, 0.31, 0.6)                                        # a value above 1 and a negative one; none with x * 255 on a tie (0.3: 76.5 in float32)
    img = rig.image(W, H, fmt, tc.raw_texels(fmt, W, H))
    rig.run(lambda cmd: cmd.clear_color_image(img, color))
    want = tc.encode(np.broadcast_to(np.array(color, dtype=np.float32), (H, W, 4)), fmt)
    assert np.array_equal(img.read(), want)
    if fmt in (tc.RGBA8_UNORM, tc.RGBA8_SRGB):                              # an image with a chain: every level
        img.generate_mips()
        other = (0.2, 0.52, 0.91, 1.0)
        sizes = [(max(1, W >> l), max(1, H >> l)) for l in range(img.mip_levels)]
        bufs = [rig.buffer(w * h * 4) for w, h in sizes]
        rig.run(lambda cmd: (cmd.clear_color_image(img, other),
                             [cmd.copy_image_to_buffer(img, b, [(0, 0, 0, l, (0, 0), s)]) for l, (b, s) in enumerate(zip(bufs, sizes))]))
        texel = tc.encode(np.array(other, dtype=np.float32), fmt)
        for b, (w, h) in zip(bufs, sizes):
            assert (b.read(0, w * h * 4).reshape(-1, 4) == texel).all(), (w, h)


def test_clear_depth_stencil_image(rig, mirhi):
    img = rig.image(W, H, tc.D32, tc.raw_texels(tc.D32, W, H))
    rig.run(lambda cmd: cmd.clear_depth_stencil_image(img, 0.625))
    assert (img.read() == np.float32(0.625)).all()
    array = rig.keep(mirhi.Image.array(rig.dev, 15, 13, 4, tc.D32))         # (a layer of 780 bytes: layer 1 starts 12 bytes past a 16-byte boundary)
    layers = np.random.default_rng(9).random((4, 13, 15)).astype(np.float32)
    array.upload(layers)
    view = array.layer_view(1)
    try:
        rig.run(lambda cmd: cmd.clear_depth_stencil_image(view, 2.5))
        want = layers.copy()
        want[1] = 2.5
        assert np.array_equal(array.read(), want)                           # the other layers are untouched
    finally:
        rig.dev.wait_idle()
        view.destroy()


@pytest.mark.parametrize("fmt", [tc.BGRA8_SRGB, tc.RGBA32F])
def test_clear_then_load_scope_equals_the_clear_scope(rig, triangle, fmt):
    scene, res, frames = triangle
    r = res[fmt]
    target = rig.image(100, 75, fmt, tc.raw_texels(fmt, 100, 75))
    rig.run(lambda cmd: (cmd.clear_color_image(target, scene.clear_color), _scope(cmd, r, target, scene.clear_color, rig.m.LoadOp.LOAD)))
    assert np.array_equal(target.read(), frames[fmt])


# ---- API behaviour ----------------------------------------------------------------------------------------------------------------------------
CLEAR_A, CLEAR_B = (0.8, 0.1, 0.1, 1.0), (0.1, 0.1, 0.8, 1.0)


def _frame_with_clear(mirhi, device, res, clear):
    x = mirhi.Image(device, 100, 75, tc.RGBA32F)
    cmd = mirhi.CommandBuffer(device)
    cmd.begin(); _scope(cmd, res, x, clear); cmd.end()
    device.submit([cmd]); device.wait_idle()
    out = x.read()
    cmd.destroy(); x.destroy()
    return out


def test_order_inside_a_command_buffer(rig, mirhi, triangle):
    scene, res, frames = triangle
    r = res[tc.RGBA32F]
    x, y = rig.image(100, 75, tc.RGBA32F), rig.image(100, 75, tc.RGBA32F, np.zeros((75, 100, 4), dtype=np.float32))
    rig.run(lambda cmd: (_scope(cmd, r, x, CLEAR_A), cmd.copy_image(x, y, [(0, (0, 0), 0, (0, 0), (100, 75))]), _scope(cmd, r, x, CLEAR_B)))
    assert np.array_equal(y.read(), _frame_with_clear(mirhi, rig.dev, r, CLEAR_A))
    assert np.array_equal(x.read(), _frame_with_clear(mirhi, rig.dev, r, CLEAR_B))


@pytest.mark.skipif(os.environ.get("MIRHI_NATIVE_DISPATCH") == "0", reason="native dispatch switched off for this run")
def test_both_dispatch_paths_with_the_transfer_last(mirhi, scenes):
    """A device on the caller's (null) stream keeps lane 0 on HIP launches until mirhi_device_set_native_dispatch(1): both paths in one process."""
    dev = mirhi.Device(0, stream=0)
    outs, used = [], []
    try:
        res = mirhi.SceneResources(dev, scenes.hello_triangle(100, 75), tc.RGBA32F)
        res.m = mirhi
        y = mirhi.Image(dev, 100, 75, tc.BGRA8_SRGB)
        fence, cmd = mirhi.Fence(dev), mirhi.CommandBuffer(dev)
        whole = ((0, 0), (100, 75))
        cmd.begin_reusable()
        _scope(cmd, res, res.color, res.scene.clear_color)
        cmd.blit_image(res.color, y, [(0, whole, 0, whole)])
        cmd.end()
        for native in (False, True):
            y.upload(np.zeros((75, 100, 4), dtype=np.uint8))
            dev.set_native_dispatch(native)
            before = dev.stats().native_dispatches
            dev.submit([cmd], fence)       # the transfer is the submit's last launch: the fence rides on it
            fence.wait(); fence.reset()
            used.append((dev.dispatch_path(), dev.stats().native_dispatches - before))
            outs.append(y.read())
        direct = mirhi.SceneResources(dev, res.scene, tc.BGRA8_SRGB)
        direct.render()
        want = direct.read()["color"]
        direct.destroy(); cmd.destroy(); fence.destroy(); y.destroy(); res.destroy()
    finally:
        dev.destroy()
    assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want)
    assert used[0][1] == 0 and (used[0][0].startswith("hip:") or "lane 0 stays on the caller's HIP stream" in used[0][0]), used
    assert used[1][0].startswith("native:") and "lane 0 stays" not in used[1][0], used
    assert used[1][1] == 3, used          # geometry and raster of the triangle scope, the blit


def test_plan_cache_takes_unchanged_transfers_and_sees_a_changed_region(rig, mirhi):
    builds = C.CDLL(mirhi.LIB_PATH).mirhi_debug_plan_builds
    builds.restype = C.c_uint64
    texels = tc.raw_texels(tc.RGBA8_UNORM, W, H, seed=4)
    src = rig.image(W, H, tc.RGBA8_UNORM, texels)
    dst = rig.image(W, H, tc.RGBA8_UNORM)
    buf = rig.buffer(W * H * 4)
    cmd = rig.keep(mirhi.CommandBuffer(rig.dev))

    def record(ox):
        cmd.begin_reusable()
        cmd.clear_color_image(dst, (0.0, 0.0, 0.0, 0.0))
        cmd.copy_image(src, dst, [(0, (0, 0), 0, (ox, 2), (10, 9))])
        cmd.copy_image_to_buffer(dst, buf, [(0, 0, 0, 0, (0, 0), (W, H))])
        cmd.end()

    def run():
        rig.dev.submit([cmd]); rig.dev.wait_idle()
        return buf.read(0, W * H * 4).reshape(H, W, 4)

    def want(ox):
        a = np.zeros((H, W, 4), dtype=np.uint8)
        a[2:11, ox:ox + 10] = texels[0:9, 0:10]
        return a

    record(4)
    first = builds()
    assert np.array_equal(run(), want(4))
    record(4)                                                               # the same transfers again: end()'s fast path
    assert builds() == first
    assert np.array_equal(run(), want(4))
    record(5)                                                               # one region offset changed: another plan, the new result
    assert builds() == first + 1
    assert np.array_equal(run(), want(5))


def test_frame_loop_with_readback_copies_keeps_the_workspace_idle(rig, mirhi, triangle, monkeypatch):
    """Two frames in flight under MIRHI_VERIFY_IDLE: scope -> copy_image_to_buffer into the frame's own buffer, mixed with frames that hold no
    transfer -- a transfer entry flips no workspace parity and touches no counter."""
    monkeypatch.setenv("MIRHI_VERIFY_IDLE", "1")
    scene, res, frames = triangle
    r = res[tc.RGBA32F]
    n = 100 * 75 * 16
    slots = [(rig.keep(mirhi.CommandBuffer(rig.dev)), rig.keep(mirhi.Fence(rig.dev)), rig.image(100, 75, tc.RGBA32F), rig.buffer(n)) for _ in range(2)]
    want = {c: _frame_with_clear(mirhi, rig.dev, r, c) for c in (CLEAR_A, CLEAR_B)}
    for step, (clear, with_copy) in enumerate(((CLEAR_A, True), (CLEAR_B, True), (CLEAR_A, False), (CLEAR_B, True), (CLEAR_B, True), (CLEAR_A, False), (CLEAR_A, True))):
        for cmd, fence, x, buf in slots:
            if with_copy:
                buf.upload(np.zeros(n, dtype=np.uint8))
            cmd.begin_reusable()
            _scope(cmd, r, x, clear)
            if with_copy:
                cmd.copy_image_to_buffer(x, buf, [(0, 0, 0, 0, (0, 0), (100, 75))])
            cmd.end()
            rig.dev.submit([cmd], fence)
        for cmd, fence, x, buf in slots:
            fence.wait(); fence.reset()
            if with_copy:
                assert np.array_equal(buf.read(0, n).view(np.float32).reshape(75, 100, 4), want[clear]), step
            else:
                assert np.array_equal(x.read(), want[clear]), step


def test_a_blit_on_another_lane_waits_for_the_scope(rig, mirhi, triangle):
    scene, res, frames = triangle
    r = res[tc.RGBA32F]
    rig.dev.set_queue_lanes(2)
    try:
        x = rig.image(100, 75, tc.RGBA32F, np.zeros((75, 100, 4), dtype=np.float32))
        y = rig.image(100, 75, tc.BGRA8_SRGB, np.zeros((75, 100, 4), dtype=np.uint8))
        a, b = rig.keep(mirhi.CommandBuffer(rig.dev)), rig.keep(mirhi.CommandBuffer(rig.dev))
        a.set_queue_lane(0); b.set_queue_lane(1)
        whole = ((0, 0), (100, 75))
        a.begin(); _scope(a, r, x, scene.clear_color); a.end()
        b.begin(); b.blit_image(x, y, [(0, whole, 0, whole)]); b.end()
        rig.dev.submit([a]); rig.dev.submit([b])                            # no fence in between: the image orders them
        rig.dev.wait_idle()
        assert np.array_equal(y.read(), frames[tc.BGRA8_SRGB])
    finally:
        rig.dev.wait_idle()
        rig.dev.set_queue_lanes(1)


def test_buffer_write_waits_for_a_transfer_that_reads_the_buffer(rig):
    n = 1 << 20
    old = np.random.default_rng(11).integers(0, 256, n, dtype=np.uint8)
    src, dst = rig.buffer(n, old), rig.buffer(n, np.zeros(n, dtype=np.uint8))
    cmd = rig.keep(rig.m.CommandBuffer(rig.dev))
    cmd.begin(); cmd.copy_buffer(src, dst, [(0, 0, n)]); cmd.end()
    rig.dev.submit([cmd])
    src.write_data(0, np.full(n, 0xEE, dtype=np.uint8))                     # right behind the submit: the copy still saw the old bytes
    rig.dev.wait_idle()
    assert np.array_equal(dst.read(0, n), old)
    assert (src.read(0, n) == 0xEE).all()


def test_tile_split_copies_the_whole_range_on_each_rank(rig):
    n = 70000
    data = np.random.default_rng(12).integers(0, 256, n, dtype=np.uint8)
    src = rig.buffer(n, data)
    try:
        for rank in range(2):
            rig.dev.set_tile_split(rank, 2, "interleaved")
            dst = rig.buffer(n, np.zeros(n, dtype=np.uint8))
            rig.run(lambda cmd: cmd.copy_buffer(src, dst, [(0, 0, n)]))
            assert np.array_equal(dst.read(0, n), data), rank
    finally:
        rig.dev.set_tile_split(0, 1, "interleaved")


def test_with_the_submit_thread(rig, mirhi, triangle):
    scene, res, frames = triangle
    r = res[tc.RGBA32F]
    rig.dev.set_submit_thread(True)
    try:
        y = rig.image(100, 75, tc.BGRA8_SRGB)
        fence = rig.keep(mirhi.Fence(rig.dev))
        whole = ((0, 0), (100, 75))
        for _ in range(3):
            y.upload(np.zeros((75, 100, 4), dtype=np.uint8))
            rig.run(lambda cmd: (_scope(cmd, r, r.color, scene.clear_color), cmd.blit_image(r.color, y, [(0, whole, 0, whole)])), fence=fence)
            assert np.array_equal(y.read(), frames[tc.BGRA8_SRGB])
    finally:
        rig.dev.wait_idle()
        rig.dev.set_submit_thread(False)


def test_refusals(rig, mirhi):
    m, R = mirhi, mirhi.RhiError
    other_dev = m.Device(0)
    foreign_img, foreign_buf = m.Image(other_dev, 8, 8, tc.RGBA8_UNORM), m.Buffer(other_dev, m.BufferUsage.Staging, 256)
    a, b = rig.buffer(1024), rig.buffer(1024)
    u8, u8b, f32 = rig.image(W, H, tc.RGBA8_UNORM), rig.image(W, H, tc.RGBA8_UNORM), rig.image(W, H, tc.RGBA32F)
    d32, ids = rig.image(W, H, tc.D32), rig.image(W, H, tc.R32_UINT)
    array = rig.keep(m.Image.array(rig.dev, 16, 16, 2, tc.D32))
    cube = rig.keep(m.Image.create_cube(rig.dev, 8, 1))
    cmd = rig.keep(m.CommandBuffer(rig.dev))
    whole = ((0, 0), (W, H))

    def refused(text, fn, *args, code=m.ERR_INVALID_HANDLE):
        with pytest.raises(R) as e:
            fn(*args)
        assert e.value.code == code and text in e.value.message, e.value.message

    try:
        cmd.begin()
        # a region outside its resource
        refused("outside its buffer", cmd.copy_buffer, a, b, [(1000, 0, 100)])
        refused("outside its buffer", cmd.copy_buffer, a, b, [(0, 1000, 100)])
        refused("outside its image", cmd.copy_image_to_buffer, u8, a, [(0, 0, 0, 0, (30, 0), (8, 4))])
        refused("outside its image", cmd.copy_buffer_to_image, a, u8, [(0, 0, 0, 0, (-1, 0), (4, 4))])
        refused("outside its buffer", cmd.copy_image_to_buffer, u8, a, [(0, 0, 0, 0, (0, 0), (W, H))])       # 4292 bytes into 1024
        refused("outside its source image", cmd.copy_image, u8, u8b, [(0, (30, 0), 0, (0, 0), (8, 4))])
        refused("outside its destination image", cmd.copy_image, u8, u8b, [(0, (0, 0), 0, (0, 26), (8, 4))])
        refused("outside its image", cmd.blit_image, u8, f32, [(0, ((0, 0), (W + 1, H)), 0, whole)])
        refused("mip level 1", cmd.copy_image_to_buffer, u8, a, [(0, 0, 0, 1, (0, 0), (4, 4))])
        # overflowing offsets
        refused("overflows", cmd.copy_buffer, a, b, [(2 ** 64 - 8, 0, 16)])
        refused("overflows", cmd.copy_image_to_buffer, u8, a, [(2 ** 64 - 8, 0, 0, 0, (0, 0), (4, 4))])
        # region_count 0 or above 16
        refused("region_count 0", cmd.copy_buffer, a, b, [])
        refused("region_count 17", cmd.copy_buffer, a, b, [(i, i, 1) for i in range(17)])
        refused("region_count 0", cmd.blit_image, u8, f32, [])
        refused("region_count 17", cmd.copy_image, u8, u8b, [(0, (0, 0), 0, (0, 0), (1, 1))] * 17)
        # overlapping source and destination ranges of one resource
        refused("overlapping", cmd.copy_buffer, a, a, [(0, 50, 100)])
        refused("overlapping", cmd.copy_buffer, a, a, [(0, 512, 100), (600, 50, 100)])
        refused("overlapping", cmd.copy_image, u8, u8, [(0, (0, 0), 0, (4, 4), (8, 8))])
        cmd.copy_image(u8, u8, [(0, (0, 0), 0, (8, 8), (8, 8))])                                     # (disjoint rectangles of one image are fine)
        # a buffer_offset that is not a multiple of the texel size; a row length or image height below the extent
        refused("not a multiple of the texel size", cmd.copy_image_to_buffer, u8, a, [(2, 0, 0, 0, (0, 0), (4, 4))])
        refused("not a multiple of the texel size", cmd.copy_buffer_to_image, a, f32, [(4, 0, 0, 0, (0, 0), (2, 2))])
        refused("at least the extent", cmd.copy_image_to_buffer, u8, a, [(0, 3, 0, 0, (0, 0), (4, 4))])
        refused("at least the extent", cmd.copy_image_to_buffer, u8, a, [(0, 0, 3, 0, (0, 0), (4, 4))])
        refused("zero extent", cmd.copy_image_to_buffer, u8, a, [(0, 0, 0, 0, (0, 0), (0, 4))])
        refused("size 0", cmd.copy_buffer, a, b, [(0, 0, 0)])
        # resources of another device
        refused("another device", cmd.copy_buffer, foreign_buf, b, [(0, 0, 16)])
        refused("another device", cmd.copy_buffer, a, foreign_buf, [(0, 0, 16)])
        refused("another device", cmd.copy_image_to_buffer, foreign_img, a, [(0, 0, 0, 0, (0, 0), (4, 4))])
        refused("another device", cmd.blit_image, u8, foreign_img, [(0, ((0, 0), (8, 8)), 0, ((0, 0), (8, 8)))])
        refused("another device", cmd.clear_color_image, foreign_img, (0, 0, 0, 0))
        # array objects and cubes as the handle
        refused("use a layer view", cmd.copy_image_to_buffer, array, a, [(0, 0, 0, 0, (0, 0), (4, 4))])
        refused("use a layer view", cmd.clear_depth_stencil_image, array, 1.0)
        refused("cube", cmd.copy_buffer_to_image, a, cube, [(0, 0, 0, 0, (0, 0), (2, 2))])
        refused("cube", cmd.clear_color_image, cube, (0, 0, 0, 0))
        # copy_image: equal texel size, both colour or both D32
        refused("not copy-compatible", cmd.copy_image, u8, f32, [(0, (0, 0), 0, (0, 0), (4, 4))])
        refused("not copy-compatible", cmd.copy_image, d32, u8, [(0, (0, 0), 0, (0, 0), (4, 4))])
        # blit: formats, source = destination, zero area, the filter
        refused("unsupported: formats", cmd.blit_image, d32, f32, [(0, whole, 0, whole)])
        refused("unsupported: formats", cmd.blit_image, u8, ids, [(0, whole, 0, whole)])
        refused("must differ", cmd.blit_image, u8, u8, [(0, ((0, 0), (8, 8)), 0, ((16, 16), (24, 24)))])
        refused("zero area", cmd.blit_image, u8, f32, [(0, ((3, 0), (3, H)), 0, whole)])
        refused("zero area", cmd.blit_image, u8, f32, [(0, whole, 0, ((0, 5), (W, 5)))])
        refused("unknown filter", cmd.blit_image, u8, f32, [(0, whole, 0, whole)], 2)
        # clears: formats
        refused("unsupported: format", cmd.clear_color_image, d32, (0, 0, 0, 0))
        refused("unsupported: format", cmd.clear_color_image, ids, (0, 0, 0, 0))
        refused("not D32_SFLOAT", cmd.clear_depth_stencil_image, f32, 1.0)
        # inside a rendering scope: every one of the seven
        cmd.begin_rendering(f32)
        for fn, args in ((cmd.copy_buffer, (a, b, [(0, 0, 16)])), (cmd.copy_buffer_to_image, (a, u8, [(0, 0, 0, 0, (0, 0), (4, 4))])),
                         (cmd.copy_image_to_buffer, (u8, a, [(0, 0, 0, 0, (0, 0), (4, 4))])), (cmd.copy_image, (u8, u8b, [(0, (0, 0), 0, (0, 0), (4, 4))])),
                         (cmd.blit_image, (u8, u8b, [(0, whole, 0, whole)])), (cmd.clear_color_image, (u8, (0, 0, 0, 0))), (cmd.clear_depth_stencil_image, (d32, 1.0))):
            refused("inside an active rendering scope", fn, *args, code=m.ERR_DEVICE)
        cmd.end_rendering()
        cmd.reset()
    finally:
        rig.dev.wait_idle()
        foreign_img.destroy(); foreign_buf.destroy(); other_dev.destroy()
