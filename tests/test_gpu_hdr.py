"""Radiance RGBE on the device (mirhi_image_expand_rgbe, mirhi_ibl_equirect_to_cube_rgbe).  The expansion is exact, so it is
compared bit for bit with the host's mires_hdr_to_float; the fused pass is compared bit for bit with the same build's float path (they share
their body and differ in how a tap is fetched) and, by the rule of test_gpu_ibl.py, with the float64 model.  Inputs: hdr_cases.py."""
import dataclasses

import numpy as np
import pytest

import hdr_cases as cases
import ibl_cases

pytestmark = pytest.mark.gpu


def check(name, gpu, m64, m32):
    """The rule of test_gpu_ibl.check: err(GPU) <= max(8 * E32, 1e-4), E32 the float32 model's own error on the same inputs."""
    e32, e = ibl_cases.err(m32, m64), ibl_cases.err(gpu, m64)
    b = ibl_cases.bound(e32)
    print(f"IBL {name}: E32 {e32:.3e} bound {b:.3e} GPU {e:.3e}")
    assert np.all(np.isfinite(np.asarray(gpu)))
    assert e <= b, f"{name}: err(GPU) {e:.3e} > max(8 * E32, 1e-4) = {b:.3e} (E32 {e32:.3e})"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _images(mirhi):
    import __graft_entry__ as ge
    ge.load_package()
    from renderer_rs_amd import images
    images.build()
    return images


@pytest.fixture(scope="module")
def images(mirhi):
    return _images(mirhi)


def upload_rgbe(mirhi, images, device, rgbe):
    return mirhi.Image.from_hdr(device, images.HdrImage(np.ascontiguousarray(rgbe)))


# ---- expand_rgbe ---------------------------------------------------------------------------------------------------------------------
def _expand_case(mirhi, images, device, rgbe):
    """The destination is prefilled with a sentinel; a second image allocated behind it must stay untouched."""
    F32 = mirhi.Format.R32G32B32A32_SFLOAT
    h, w = rgbe.shape[:2]
    src = upload_rgbe(mirhi, images, device, rgbe)
    dst, behind = mirhi.Image(device, w, h, F32), mirhi.Image(device, w, h, F32)
    try:
        sentinel = np.full((h, w, 4), -7.0, dtype=np.float32)
        dst.upload(sentinel)
        behind.upload(sentinel)
        dst.expand_rgbe(src)
        got, want = dst.read(), images.HdrImage(rgbe).to_float()
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), f"{w}x{h}: {int(np.sum(bits(got) != bits(want)))} values differ"
        assert np.all(behind.read() == -7.0)
        assert np.array_equal(src.read(), rgbe)                          # the source is read, not written
    finally:
        for o in (src, dst, behind):
            o.destroy()


def test_expand_every_mantissa_and_exponent(mirhi, images, device):
    """All 2^16 (m, E) pairs, the denormals of E < 10 included: the build must not flush them."""
    x = cases.all_pairs()
    f = cases.decode_float(x)
    assert np.count_nonzero((f[..., :3] != 0.0) & (np.abs(f[..., :3]) < np.finfo(np.float32).tiny)) > 1000      # (the case does hold denormals)
    _expand_case(mirhi, images, device, x)


@pytest.mark.parametrize("w,h", ((1, 1), (3, 5), (64, 1), (65, 1), (256, 1), (257, 3), (1023, 2), (1024, 1), (1025, 1)))
def test_expand_extents(mirhi, images, device, w, h):
    """One lane, a partial wave, a wave, a wave plus one, a 256-thread row, odd widths, and one workgroup's 1024 texels exactly and plus one."""
    _expand_case(mirhi, images, device, cases.random_rgbe(w, h, 1000 * w + h))


# ---- the fused pass against the same build's float path --------------------------------------------------------------------------------
def _pair(mirhi, images, dev, rgbe, sizes):
    """For each cube size: level 0 of ibl_equirect_to_cube_rgbe and of expand_rgbe + ibl_equirect_to_cube, and level 1 of the fused cube."""
    F32 = mirhi.Format.R32G32B32A32_SFLOAT
    h, w = rgbe.shape[:2]
    src, flt = upload_rgbe(mirhi, images, dev, rgbe), mirhi.Image(dev, w, h, F32)
    out = {}
    try:
        flt.expand_rgbe(src)
        for n in sizes:
            levels = 2 if n > 1 else 1
            fused, plain = mirhi.Image.create_cube(dev, n, levels), mirhi.Image.create_cube(dev, n, levels)
            try:
                sentinel = np.full((mirhi.ibl.cube_texels(n, levels), 4), -7.0, dtype=np.float32)
                fused.upload(sentinel)
                plain.upload(sentinel)
                fused.ibl_equirect_to_cube_rgbe(src)
                plain.ibl_equirect_to_cube(flt)
                f, p = fused.cube_levels(), plain.cube_levels()
                out[n] = (f[0].copy(), p[0].copy(), f[1].copy() if levels > 1 else None)
            finally:
                fused.destroy(); plain.destroy()
    finally:
        src.destroy(); flt.destroy()
    return out


def _assert_pairs_equal(name, out):
    for n, (fused, plain, level1) in out.items():
        assert np.all(np.isfinite(fused)) and np.all(fused[..., 3] == 1.0)
        assert np.array_equal(bits(fused), bits(plain)), f"{name} -> {n}^2: {int(np.sum(bits(fused) != bits(plain)))} values differ from the float path"
        assert level1 is None or np.all(level1 == -7.0)                  # level 0 only


SIZES = (1, 2, 16, 64)


@pytest.fixture(scope="module")
def equirect_pairs(mirhi, images, device):
    return _pair(mirhi, images, device, cases.equirect_rgbe(), SIZES)


def test_fused_pass_equals_the_float_path(equirect_pairs):
    assert np.any(equirect_pairs[64][0][..., :3] > 0.0)
    _assert_pairs_equal("256x128", equirect_pairs)


@pytest.mark.parametrize("w,h", ((8, 4), (1, 1)))
def test_fused_pass_equals_the_float_path_from_a_tiny_source(mirhi, images, device, w, h):
    """8 x 4, and 1 x 1 where u wraps onto the texel itself and v clamps onto it: every output texel is that texel."""
    rgbe = cases.rgbe_from_float(np.random.default_rng(w).uniform(0.0, 40.0, size=(h, w, 3)))
    out = _pair(mirhi, images, device, rgbe, SIZES)
    _assert_pairs_equal(f"{w}x{h}", out)
    if (w, h) == (1, 1):
        texel = cases.decode_float(rgbe)[0, 0]
        for n in SIZES:
            assert np.array_equal(bits(out[n][0]), bits(np.broadcast_to(texel, out[n][0].shape)))


def test_fused_pass_with_every_exponent(mirhi, images, device):
    """all_pairs() as a source: denormal and huge taps go through the same blend in both paths (2 x 255 x 2^119 stays finite)."""
    _assert_pairs_equal("all pairs", _pair(mirhi, images, device, cases.all_pairs(), (16,)))


def test_fused_pass_reads_level_0_of_a_source_with_a_mip_chain(mirhi, images, device):
    rgbe = cases.equirect_rgbe()
    src, cube = upload_rgbe(mirhi, images, device, rgbe), mirhi.Image.create_cube(device, 16, 1)
    flt = mirhi.Image(device, rgbe.shape[1], rgbe.shape[0], mirhi.Format.R32G32B32A32_SFLOAT)
    try:
        cube.ibl_equirect_to_cube_rgbe(src)
        before = cube.read()
        src.generate_mips()
        assert src.mip_levels == 9
        cube.upload(np.zeros_like(before))
        cube.ibl_equirect_to_cube_rgbe(src)
        assert np.array_equal(bits(cube.read()), bits(before))
        flt.expand_rgbe(src)
        assert np.array_equal(bits(flt.read()), bits(images.HdrImage(rgbe).to_float()))
    finally:
        for o in (src, cube, flt):
            o.destroy()


# ---- the fused pass against the float64 model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ibl_cases.EQUIRECT_CUBE_SIZES)
def test_fused_pass_against_the_model(mirhi, images, device, size):
    decoded = images.HdrImage(cases.equirect_rgbe()).to_float()
    src = upload_rgbe(mirhi, images, device, cases.equirect_rgbe())
    cube = mirhi.Image.create_cube(device, size, 2)
    try:
        cube.upload(np.full((mirhi.ibl.cube_texels(size, 2), 4), -7.0, dtype=np.float32))
        cube.ibl_equirect_to_cube_rgbe(src)
        levels = cube.cube_levels()
        m64, m32 = ibl_cases.both(mirhi.ibl.equirect_to_cube, decoded, size)
        check(f"equirect rgbe 256x128 -> {size}^2", levels[0], m64, m32)
        assert np.all(levels[1] == -7.0)
    finally:
        src.destroy(); cube.destroy()


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
def _sky_frame(mirhi, scenes, device, env):
    spec = dataclasses.replace(scenes.skybox_case(64, 48, 0, 16, 1).sky, levels=None, image=env)
    res = mirhi.SceneResources(device, scenes.Scene("hdr-sky", 64, 48, [], sky=spec), mirhi.Format.R32G32B32A32_SFLOAT, want_prim=True, want_depth=True)
    res.render()
    out = res.read()
    res.destroy()
    return out


def test_load_environment_equals_the_chain_built_by_hand(mirhi, scenes, oracle, images, device):
    """load_environment from the file's bytes, then the same chain by hand from the float upload: all four images and a SKYBOX frame of each
    environment are equal bit for bit; an ordinary frame straight behind the passes matches the oracle, as test_gpu_ibl's chain test has it."""
    M, F32 = mirhi, mirhi.Format.R32G32B32A32_SFLOAT
    rgbe = cases.equirect_rgbe()
    data = images.encode_hdr(rgbe)
    scene = scenes.displaced_sphere(24, 17, 128, 96, seed=3)
    res = M.SceneResources(device, scene, F32, want_prim=True)
    res.render()                                     # a frame before: the device's lanes have seen work the passes must wait for
    made = list(M.load_environment(device, data, 32, irradiance_size=8, prefiltered_size=16, prefilter_samples=64, lut_size=32))
    res.render()                                     # straight behind the passes, before anything is read back
    out = res.read()
    try:
        env, irr, pre, lut = made
        assert (env.width, env.mip_levels, irr.width, irr.mip_levels, pre.width, pre.mip_levels) == (32, 6, 8, 1, 16, 5)
        assert (lut.width, lut.height, lut.is_cube) == (32, 32, False)
        h, w = rgbe.shape[:2]
        src = M.Image(device, w, h, F32)
        made.append(src)
        src.upload(images.decode_hdr(data).to_float())
        hand = [M.Image.create_cube(device, 32, 6), M.Image.create_cube(device, 8, 1), M.Image.create_cube(device, 16, 5), M.Image(device, 32, 32, F32)]
        made += hand
        hand[0].ibl_equirect_to_cube(src)
        hand[0].ibl_cube_generate_mips()
        hand[1].ibl_irradiance(hand[0])
        hand[2].ibl_prefilter(hand[0], 64)
        hand[3].ibl_brdf_lut()
        for name, a, b in zip(("environment", "irradiance", "prefiltered", "brdf lut"), (env, irr, pre, lut), hand):
            ra, rb = a.read(), b.read()
            assert np.all(np.isfinite(ra)) and np.array_equal(bits(ra), bits(rb)), name
        assert np.any(env.read()[:, :3] > 0.0)
        fa, fb = _sky_frame(M, scenes, device, env), _sky_frame(M, scenes, device, hand[0])
        for k in ("color", "prim", "depth"):
            assert np.array_equal(fa[k], fb[k]), k
        assert np.any(fa["color"][..., :3] > 0.0)
        ref = oracle.render(scene, want_bgra8=False)
        assert np.array_equal(out["prim"], ref["prim"])
        assert float(np.max(np.abs(out["color"][..., :3] - ref["rgba"][..., :3]))) < 1e-4
    finally:
        device.wait_idle()
        for o in made:
            o.destroy()
        res.destroy()


def test_load_environment_from_a_path_and_seamless(mirhi, images, device, tmp_path):
    p = tmp_path / "env.hdr"
    p.write_bytes(images.encode_hdr(cases.equirect_rgbe(), rle=False))
    made = mirhi.load_environment(device, str(p), 16, irradiance_size=4, prefiltered_size=8, prefilter_samples=16, lut_size=16, seamless=True)
    try:
        assert [i.cube_seamless for i in made[:3]] == [True, True, True]
        assert all(np.all(np.isfinite(i.read())) for i in made)
    finally:
        for o in made:
            o.destroy()
    with pytest.raises(images.ImageDecodeError):
        mirhi.load_environment(device, cases.FILE_8X2[:-1], 16)


# ---- dispatch ------------------------------------------------------------------------------------------------------------------------------
def test_pair_on_the_other_dispatch_path(mirhi, scenes, images, device, equirect_pairs):
    """A device on the caller's (null) stream, put with set_native_dispatch on the path the default device does not take: the immediate passes
    coexist with it, and give the bits they give on the default device."""
    default_native = device.dispatch_path().startswith("native")
    dev = mirhi.Device(0, stream=0)
    try:
        dev.set_native_dispatch(not default_native)
        print(f"dispatch: default {device.dispatch_path()!r}, this device {dev.dispatch_path()!r}")
        res = mirhi.SceneResources(dev, scenes.displaced_sphere(24, 17, 128, 96, seed=3), mirhi.Format.R32G32B32A32_SFLOAT, want_prim=True)
        before = dev.stats().native_dispatches
        res.render()                                 # work on that path ahead of the passes
        out = _pair(mirhi, images, dev, cases.equirect_rgbe(), (16, 64))
        res.render()
        frame = res.read()
        used = dev.stats().native_dispatches - before
        res.destroy()
    finally:
        dev.destroy()
    assert (used > 0) == (not default_native), used      # (this device's lane 0 launched through the path the default device does not take)
    _assert_pairs_equal("other path", out)
    for n in (16, 64):
        assert np.array_equal(bits(out[n][0]), bits(equirect_pairs[n][0]))
    assert np.all(np.isfinite(frame["color"]))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(mirhi, device):
    M, F = mirhi, mirhi.Format

    def refused(fn, text, variant="InvalidHandle"):
        with pytest.raises(M.RhiError) as e:
            fn()
        assert e.value.variant == variant and text in e.value.message, (e.value.variant, e.value.message)

    rgbe = M.Image(device, 32, 16, F.R8G8B8A8_UNORM)
    srgb = M.Image(device, 32, 16, F.R8G8B8A8_SRGB)
    bgra = M.Image(device, 32, 16, F.B8G8R8A8_SRGB)
    flt = M.Image(device, 32, 16, F.R32G32B32A32_SFLOAT)
    flt_other = M.Image(device, 16, 32, F.R32G32B32A32_SFLOAT)
    dimg = M.Image(device, 32, 16, F.D32_SFLOAT)
    uimg = M.Image(device, 32, 16, F.R32_UINT)
    arr = M.Image.array(device, 32, 16, 4, F.D32_SFLOAT)
    view = arr.layer_view(1)
    ms = M.Image.multisampled(device, 32, 16, F.R32G32B32A32_SFLOAT)
    cube, cube2 = M.Image.create_cube(device, 16, 5), M.Image.create_cube(device, 8, 1)
    objs = [rgbe, srgb, bgra, flt, flt_other, dimg, uimg, view, arr, ms, cube, cube2]
    try:
        for call in (lambda s: flt.expand_rgbe(s), lambda s: cube.ibl_equirect_to_cube_rgbe(s)):
            for src in (cube2, arr, view, ms):
                refused(lambda: call(src), "the RGBE source must be a 2-D image")
            for src in (srgb, bgra, flt_other, dimg, uimg):
                refused(lambda: call(src), "the RGBE source must be R8G8B8A8_UNORM")
        # the destination of the expansion: a 2-D R32G32B32A32_SFLOAT image of the source's extent
        refused(lambda: cube.expand_rgbe(rgbe), "the destination must be a 2-D image")
        refused(lambda: arr.expand_rgbe(rgbe), "the destination must be a 2-D image")
        refused(lambda: view.expand_rgbe(rgbe), "the destination must be a 2-D image")
        refused(lambda: ms.expand_rgbe(rgbe), "a multisampled image is a transient attachment")
        refused(lambda: dimg.expand_rgbe(rgbe), "the destination must be R32G32B32A32_SFLOAT")
        refused(lambda: srgb.expand_rgbe(rgbe), "the destination must be R32G32B32A32_SFLOAT")
        refused(lambda: rgbe.expand_rgbe(rgbe), "the destination must be R32G32B32A32_SFLOAT")
        refused(lambda: flt_other.expand_rgbe(rgbe), "the destination must have the source's extent")
        # the destination of the fused pass: a cube
        refused(lambda: flt.ibl_equirect_to_cube_rgbe(rgbe), "the destination must be a cube image")
        refused(lambda: rgbe.ibl_equirect_to_cube_rgbe(rgbe), "the destination must be a cube image")
        refused(lambda: ms.ibl_equirect_to_cube_rgbe(rgbe), "a multisampled image is a transient attachment")
        # NULL, as the helpers word it
        L = M.lib()
        for fn, dst in ((L.mirhi_image_expand_rgbe, flt), (L.mirhi_ibl_equirect_to_cube_rgbe, cube)):
            assert fn(None, dst.handle) == M.ERR_INVALID_HANDLE and b"the RGBE source is null" in L.mirhi_last_error_message()
            assert fn(rgbe.handle, None) == M.ERR_INVALID_HANDLE and b"the destination is null" in L.mirhi_last_error_message()
        # the float pass goes on refusing RGBA8
        refused(lambda: cube.ibl_equirect_to_cube(rgbe), "must be R32G32B32A32_SFLOAT")
        other = M.Device(0)
        try:
            foreign_cube, foreign_flt = M.Image.create_cube(other, 8, 1), M.Image(other, 32, 16, F.R32G32B32A32_SFLOAT)
            refused(lambda: foreign_cube.ibl_equirect_to_cube_rgbe(rgbe), "different devices")
            refused(lambda: foreign_flt.expand_rgbe(rgbe), "different devices")
            foreign_cube.destroy(); foreign_flt.destroy()
        finally:
            other.destroy()
        # nothing above ran: the accepted calls still do
        rgbe.upload(np.full((16, 32, 4), 128, dtype=np.uint8))
        flt.expand_rgbe(rgbe)
        assert np.all(flt.read() == np.array([2.0 ** -1, 2.0 ** -1, 2.0 ** -1, 1.0], dtype=np.float32))
        cube.ibl_equirect_to_cube_rgbe(rgbe)
        assert np.all(cube.cube_levels()[0] == np.array([0.5, 0.5, 0.5, 1.0], dtype=np.float32))
    finally:
        for o in objs:
            o.destroy()
