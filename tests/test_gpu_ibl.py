"""The IBL precompute passes on the GPU (mirhi_ibl_* of include/mirhi.h) against the float64 numpy model, every texel and
channel of every output.  Bound per output: err(GPU) <= max(8 * E32, 1e-4) with E32 the float32 model's own error on the same
inputs (tests/ibl_cases.py says where the numbers come from).  Every comparison prints its figures before it asserts."""
import numpy as np
import pytest

import ibl_cases as cases

pytestmark = pytest.mark.gpu


def check(name, gpu, m64, m32):
    e32, e = cases.err(m32, m64), cases.err(gpu, m64)
    b = cases.bound(e32)
    print(f"IBL {name}: E32 {e32:.3e} bound {b:.3e} GPU {e:.3e}")
    assert np.all(np.isfinite(np.asarray(gpu)))
    assert e <= b, f"{name}: err(GPU) {e:.3e} > max(8 * E32, 1e-4) = {b:.3e} (E32 {e32:.3e})"


@pytest.fixture(scope="module")
def env_image(mirhi, device):
    """analytic_environment(64) with its full chain, uploaded whole (the chain is cube_mips in float32, what the device builds too)."""
    img = mirhi.Image.create_cube(device, cases.ENV_SIZE, cases.ENV_LEVELS)
    img.upload(cases.packed(cases.environment()).astype(np.float32))
    yield img
    img.destroy()


# ---- the images ------------------------------------------------------------------------------------------------------------------
def test_cube_accessors_and_round_trip(mirhi, device):
    M = mirhi
    cube = M.Image.create_cube(device, 16, 5)
    texels = 6 * (256 + 64 + 16 + 4 + 1)
    assert cube.layers == 6 and cube.mip_levels == 5 and cube.width == 16 and cube.height == 16
    assert M.lib().mirhi_image_size_bytes(cube.handle) == texels * 16 == M.ibl.cube_texels(16, 5) * 16
    assert M.lib().mirhi_image_format(cube.handle) == M.Format.R32G32B32A32_SFLOAT
    data = np.random.default_rng(5).uniform(-4.0, 4.0, size=(texels, 4)).astype(np.float32)
    cube.upload(data)
    back = cube.read()
    assert back.shape == (texels, 4) and np.array_equal(back, data)
    levels = cube.cube_levels(back)
    assert [l.shape for l in levels] == [(6, 16 >> l, 16 >> l, 4) for l in range(5)]
    assert np.array_equal(levels[1][2], data[6 * 256 + 2 * 64:6 * 256 + 3 * 64].reshape(8, 8, 4))     # level-major, then face-major, then rows
    assert np.array_equal(cube.cube_face(1, 2, back), levels[1][2])
    with pytest.raises(M.RhiError):
        cube.upload(data[:-1])
    one = M.Image.create_cube(device, 1, 1)
    assert one.layers == 6 and one.mip_levels == 1 and M.lib().mirhi_image_size_bytes(one.handle) == 96
    big = M.Image.create_cube(device, 64)
    assert big.mip_levels == 1 and M.lib().mirhi_image_size_bytes(big.handle) == 6 * 64 * 64 * 16
    for o in (cube, one, big):
        o.destroy()


def test_refusals(mirhi, device):
    M = mirhi

    def refused(fn, text, variant="InvalidHandle"):
        with pytest.raises(M.RhiError) as e:
            fn()
        assert e.value.variant == variant and text in e.value.message, (e.value.variant, e.value.message)

    F = M.Format
    # creation
    for fmt in (F.R8G8B8A8_UNORM, F.D32_SFLOAT, F.B8G8R8A8_SRGB, F.R32_UINT, F.UNDEFINED):
        refused(lambda: M.Image.create_cube(device, 16, 1, fmt), "R32G32B32A32_SFLOAT only")
    for size in (0, 3, 48, 8192):
        refused(lambda: M.Image.create_cube(device, size, 1), "power of two in [1, 4096]")
    refused(lambda: M.Image.create_cube(device, 16, 0), "1 to 5 mip levels")
    refused(lambda: M.Image.create_cube(device, 16, 6), "1 to 5 mip levels")
    cube = M.Image.create_cube(device, 16, 5)
    cube2 = M.Image.create_cube(device, 8, 4)
    img2d = M.Image(device, 32, 16, F.R32G32B32A32_SFLOAT)
    sq = M.Image(device, 16, 16, F.R32G32B32A32_SFLOAT)
    rgba8 = M.Image(device, 16, 16, F.R8G8B8A8_UNORM)
    dimg = M.Image(device, 16, 16, F.D32_SFLOAT)
    arr = M.Image.array(device, 16, 16, 4, F.D32_SFLOAT)
    ub = M.Buffer.new_with_data(device, M.BufferUsage.Uniform, np.zeros(336, dtype=np.uint8))
    # a cube where a 2-D image or an array is due
    cmd = M.CommandBuffer(device)
    refused(lambda: (cmd.begin(), cmd.begin_rendering(cube)), "a cube image is not an attachment")
    cmd.reset()
    refused(lambda: (cmd.begin(), cmd.begin_rendering(sq, depth=cube)), "a cube image is not an attachment")
    cmd.reset()
    refused(lambda: (cmd.begin(), cmd.begin_rendering(None, depth=cube, depth_store_op=M.StoreOp.STORE)), "a cube image is not an attachment")
    cmd.reset()
    cmd.begin()
    for slot in range(6):          # every mirhi_texture_slot
        refused(lambda: cmd.bind_texture(slot, cube), "a cube image cannot be bound at a texture slot")
    refused(lambda: cmd.bind_shadow_cascades(cube, ub), "not a cube image")
    cmd.end()
    cmd.destroy()
    refused(lambda: cube.layer_view(0), "a cube image has no layer views")
    refused(cube.generate_mips, "mirhi_ibl_cube_generate_mips")
    refused(lambda: cube.set_max_anisotropy(4), "a cube image has no anisotropic sampler")
    assert not hasattr(M.lib(), "mirhi_image_wrap_device_memory_cube")       # there is no wrapped cube
    # the passes
    refused(lambda: cube.ibl_equirect_to_cube(cube2), "the equirectangular source must be a 2-D image")
    refused(lambda: cube.ibl_equirect_to_cube(rgba8), "must be R32G32B32A32_SFLOAT")
    refused(lambda: cube.ibl_equirect_to_cube(arr), "must be a 2-D image")
    refused(lambda: sq.ibl_equirect_to_cube(img2d), "the destination must be a cube image")
    refused(lambda: sq.ibl_cube_generate_mips(), "must be a cube image")
    refused(lambda: cube.ibl_irradiance(cube), "cannot read and write the same image")
    refused(lambda: cube.ibl_irradiance(sq), "the environment must be a cube image")
    refused(lambda: sq.ibl_irradiance(cube), "the destination must be a cube image")
    refused(lambda: cube.ibl_prefilter(cube, 64), "cannot read and write the same image")
    refused(lambda: cube.ibl_prefilter(img2d, 64), "the environment must be a cube image")
    refused(lambda: dimg.ibl_prefilter(cube, 64), "the destination must be a cube image")
    refused(lambda: cube.ibl_prefilter(cube2, 0), "sample_count must be in [1, 4096]")
    refused(lambda: cube.ibl_prefilter(cube2, 4097), "sample_count must be in [1, 4096]")
    refused(cube.ibl_brdf_lut, "the destination must be a 2-D image")
    refused(img2d.ibl_brdf_lut, "must be square")
    refused(rgba8.ibl_brdf_lut, "must be R32G32B32A32_SFLOAT")
    refused(dimg.ibl_brdf_lut, "must be R32G32B32A32_SFLOAT")
    L = M.lib()
    assert L.mirhi_ibl_irradiance(None, cube.handle) == M.ERR_INVALID_HANDLE and b"null" in L.mirhi_last_error_message()
    assert L.mirhi_ibl_brdf_lut(None) == M.ERR_INVALID_HANDLE
    other = M.Device(0)
    try:
        foreign = M.Image.create_cube(other, 8, 1)
        foreign2d = M.Image(other, 32, 16, F.R32G32B32A32_SFLOAT)
        refused(lambda: cube.ibl_irradiance(foreign), "different devices")
        refused(lambda: cube.ibl_prefilter(foreign, 16), "different devices")
        refused(lambda: cube.ibl_equirect_to_cube(foreign2d), "different devices")
        foreign.destroy()
        foreign2d.destroy()
    finally:
        other.destroy()
    for o in (cube, cube2, img2d, sq, rgba8, dimg, arr, ub):
        o.destroy()


# ---- each pass against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cases.EQUIRECT_CUBE_SIZES)
def test_equirect_to_cube(mirhi, device, size):
    w, h = cases.EQUIRECT_EXTENT
    src = mirhi.Image(device, w, h, mirhi.Format.R32G32B32A32_SFLOAT)
    src.upload(cases.equirect())
    cube = mirhi.Image.create_cube(device, size, 2)
    sentinel = np.full((mirhi.ibl.cube_texels(size, 2), 4), -7.0, dtype=np.float32)
    cube.upload(sentinel)
    cube.ibl_equirect_to_cube(src)
    levels = cube.cube_levels()
    m64, m32 = cases.equirect_models(size)
    check(f"equirect 256x128 -> {size}^2", levels[0], m64, m32)
    assert np.all(levels[1] == -7.0)                 # level 0 only
    src.destroy()
    cube.destroy()


def test_cube_mips_are_bit_exact(mirhi, device, env_image):
    cube = mirhi.Image.create_cube(device, cases.ENV_SIZE, cases.ENV_LEVELS)
    data = np.full((mirhi.ibl.cube_texels(cases.ENV_SIZE, cases.ENV_LEVELS), 4), np.nan, dtype=np.float32)
    data[:6 * cases.ENV_SIZE ** 2] = cases.environment()[0].reshape(-1, 4)
    cube.upload(data)
    cube.ibl_cube_generate_mips()
    got = cube.cube_levels()
    want = mirhi.ibl.cube_mips(cases.environment()[0], cases.ENV_LEVELS, dtype=np.float32)
    for l, (g, w) in enumerate(zip(got, want)):
        assert w.dtype == np.float32 and np.array_equal(g.view(np.uint32), w.view(np.uint32)), f"level {l} differs from cube_mips(float32)"
    cube.destroy()


@pytest.mark.parametrize("size", cases.IRRADIANCE_SIZES)
def test_irradiance(mirhi, device, env_image, size):
    out = mirhi.Image.create_cube(device, size, 1)
    out.ibl_irradiance(env_image)
    m64, m32 = cases.irradiance_models(size)
    check(f"irradiance {size}^2", out.cube_levels()[0], m64, m32)
    out.destroy()


@pytest.mark.parametrize("size,levels,samples", cases.PREFILTER_CASES)
def test_prefilter(mirhi, device, env_image, size, levels, samples):
    out = mirhi.Image.create_cube(device, size, levels)
    out.ibl_prefilter(env_image, samples)
    got = out.cube_levels()
    m64, m32 = cases.prefilter_models(size, levels, samples)
    failures = []
    for l in range(levels):
        try:
            check(f"prefilter {size}^2 x {levels} levels x {samples} samples, level {l}", got[l], m64[l], m32[l])
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    out.destroy()


def test_prefilter_level_0_is_the_environment(mirhi, device, env_image):
    """Roughness < 0.01 (prefilter_map.hlsl:168-173): one lookup at R; with `out` the size of `env` that is env's own texel."""
    out = mirhi.Image.create_cube(device, cases.ENV_SIZE, 2)
    out.ibl_prefilter(env_image, 16)
    got = out.cube_levels()[0]
    want = cases.environment()[0].astype(np.float64).copy()
    want[..., 3] = 1.0
    m32 = mirhi.ibl.prefilter(cases.environment(), cases.ENV_SIZE, 2, 16, dtype=np.float32)[0]
    check("prefilter level 0 against env level 0", got, want, m32)
    out.destroy()


def test_prefilter_with_the_largest_sample_count(mirhi, device, env_image):
    """4096 samples: the largest table a workgroup keeps."""
    out = mirhi.Image.create_cube(device, 4, 2)
    out.ibl_prefilter(env_image, 4096)
    got = out.cube_levels()
    m64, m32 = cases.both(mirhi.ibl.prefilter, cases.environment(), 4, 2, 4096)
    check("prefilter 4^2 x 2 levels x 4096 samples, level 1", got[1], m64[1], m32[1])
    out.destroy()


@pytest.mark.parametrize("size", cases.LUT_SIZES)
def test_brdf_lut(mirhi, device, size):
    lut = mirhi.Image(device, size, size, mirhi.Format.R32G32B32A32_SFLOAT)
    lut.ibl_brdf_lut()
    got = lut.read()
    m64, m32 = cases.lut_models(size)
    check(f"brdf lut {size}^2 A", got[..., 0], m64[..., 0], m32[..., 0])
    check(f"brdf lut {size}^2 B", got[..., 1], m64[..., 1], m32[..., 1])
    assert np.all(got[..., 2] == 0.0) and np.all(got[..., 3] == 1.0)
    lut.destroy()


def test_constant_environment_identities(mirhi, device):
    c = np.array([0.25, 1.5, 12.0, 1.0], dtype=np.float32)
    env = mirhi.Image.create_cube(device, 16, 5)
    env.upload(np.broadcast_to(c, (mirhi.ibl.cube_texels(16, 5), 4)).copy())
    env.ibl_cube_generate_mips()
    assert np.array_equal(env.read(), np.broadcast_to(c, (mirhi.ibl.cube_texels(16, 5), 4)))
    pre = mirhi.Image.create_cube(device, 8, 4)
    pre.ibl_prefilter(env, 256)
    got = pre.read()
    assert np.allclose(got[:, :3], c[:3], rtol=1e-5, atol=0) and np.all(got[:, 3] == 1.0)
    irr = mirhi.Image.create_cube(device, 4, 1)
    irr.ibl_irradiance(env)
    _, thetas = mirhi.ibl.irradiance_angles()
    th = thetas.astype(np.float64)
    want = c[:3].astype(np.float64) * mirhi.ibl.PI * np.mean(np.cos(th) * np.sin(th))
    got = irr.read()
    assert np.allclose(got[:, :3], want, rtol=1e-5, atol=0) and np.all(got[:, 3] == 1.0)
    for o in (env, pre, irr):
        o.destroy()


def test_chain_in_one_sequence_then_an_ordinary_frame(mirhi, scenes, oracle, device):
    """equirect -> cube -> mips -> irradiance + prefilter with nothing but the passes in between, against the model chained the
    same way (the environment is stored as float32 between the stages, as the image stores it); then an ordinary frame on
    the same device, compared with the oracle as the smoke test does: the passes left the queue lanes and the caches in order."""
    M, ibl = mirhi, mirhi.ibl
    # a frame before, so that the device's lanes have seen work the passes must wait for
    scene = scenes.displaced_sphere(24, 17, 128, 96, seed=3)
    res = M.SceneResources(device, scene, M.Format.R32G32B32A32_SFLOAT, want_prim=True)
    res.render()
    w, h = cases.EQUIRECT_EXTENT
    src = M.Image(device, w, h, M.Format.R32G32B32A32_SFLOAT)
    src.upload(cases.equirect())
    env = M.Image.create_cube(device, 32, 6)
    irr = M.Image.create_cube(device, 8, 1)
    pre = M.Image.create_cube(device, 16, 5)
    env.ibl_equirect_to_cube(src)
    env.ibl_cube_generate_mips()
    irr.ibl_irradiance(env)
    pre.ibl_prefilter(env, 64)
    res.render()                                     # straight behind the passes, before anything is read back
    out = res.read()
    got_env, got_irr, got_pre = env.cube_levels(), irr.cube_levels()[0], pre.cube_levels()

    def chain(dtype):
        e0 = ibl.equirect_to_cube(cases.equirect(), 32, dtype=dtype).astype(np.float32)
        chain_env = ibl.cube_mips(e0, 6, dtype=np.float32)
        return e0, ibl.irradiance(chain_env, 8, dtype=dtype), ibl.prefilter(chain_env, 16, 5, 64, dtype=dtype)
    e64, i64, p64 = chain(np.float64)
    e32, i32, p32 = chain(np.float32)
    check("chain: environment level 0", got_env[0], e64, e32)
    gpu_chain = [np.asarray(l, dtype=np.float32) for l in got_env]
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(gpu_chain, ibl.cube_mips(gpu_chain[0], 6, dtype=np.float32)))
    check("chain: irradiance 8^2", got_irr, i64, i32)
    for l in range(5):
        check(f"chain: prefilter level {l}", got_pre[l], p64[l], p32[l])
    ref = oracle.render(scene, want_bgra8=False)
    assert np.array_equal(out["prim"], ref["prim"])
    assert float(np.max(np.abs(out["color"][..., :3] - ref["rgba"][..., :3]))) < 1e-4
    for o in (src, env, irr, pre):
        o.destroy()
    res.destroy()
