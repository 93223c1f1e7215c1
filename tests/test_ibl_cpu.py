"""The numpy model of the IBL precompute passes (renderer_rs_amd.ibl) against closed forms, and the cube sampler's orientation.
No GPU: these pin the yardstick the GPU tests (test_gpu_ibl.py) measure the kernels with."""
import math

import numpy as np
import pytest

import ibl_cases as cases


@pytest.fixture(scope="module")
def ibl(mirhi):
    return mirhi.ibl


def test_binding_covers_the_new_entry_points(mirhi):
    names = {"mirhi_image_create_cube", "mirhi_ibl_equirect_to_cube", "mirhi_ibl_cube_generate_mips", "mirhi_ibl_irradiance",
             "mirhi_ibl_prefilter", "mirhi_ibl_brdf_lut"}
    assert names <= set(mirhi._SIGNATURES)
    header = open(mirhi.INCLUDE).read()
    for n in names:
        assert n + "(" in header
        assert hasattr(mirhi.lib(), n)
    assert mirhi.ABI_VERSION == 5 == mirhi.lib().mirhi_abi_version()


@pytest.mark.parametrize("n", range(1, 17))
def test_sampling_a_texel_centre_returns_that_texel(ibl, n):
    """sample_cube(cube_direction(face, uv)) is that face's texel at every texel centre: pins the orientation of all six faces in
    both tables (GetCubemapDirection and the face selection are inverses of each other)."""
    rng = np.random.default_rng(n)
    level = rng.uniform(0.0, 4.0, size=(6, n, n, 4))
    c = (np.arange(n) + 0.5) / n
    for face in range(6):
        uv = np.stack(np.broadcast_arrays(c[None, :], c[:, None]), axis=-1)
        got = ibl.sample_cube([level], ibl.cube_direction(face, uv))
        assert np.allclose(got, level[face], rtol=0, atol=1e-12), (n, face)
        f, s, t = ibl.select_face(ibl.cube_direction(face, uv))
        assert np.all(f == face)
        assert np.allclose(s, uv[..., 0], atol=1e-15) and np.allclose(t, uv[..., 1], atol=1e-15)


def test_face_selection_ties_prefer_z_then_y_then_x(ibl):
    d = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 0.5], [-1.0, 0.5, -1.0], [1.0, -1.0, 0.0], [-1.0, 0.0, 0.0]])
    f, _, _ = ibl.select_face(d)
    assert f.tolist() == [4, 2, 5, 3, 1]


def test_lod_is_clamped_and_lerped(ibl):
    levels = [np.full((6, 4, 4, 1), 1.0), np.full((6, 2, 2, 1), 3.0), np.full((6, 1, 1, 1), 7.0)]
    d = np.array([[0.2, -0.3, 1.0]])
    for lod, want in ((-2.0, 1.0), (0.0, 1.0), (0.25, 1.5), (1.0, 3.0), (1.5, 5.0), (2.0, 7.0), (9.0, 7.0)):
        assert ibl.sample_cube(levels, d, lod)[0, 0] == pytest.approx(want, abs=1e-12), lod


def test_equirect_lookup_wraps_u_and_clamps_v(ibl):
    src = np.arange(4 * 8, dtype=np.float64).reshape(4, 8, 1)
    # u = 0 lies between the last and the first column; v = 0 is above the first row's centre
    assert ibl.sample_equirect(src, np.array([[0.0, 0.0]]))[0, 0] == pytest.approx(0.5 * (src[0, 7, 0] + src[0, 0, 0]))
    assert ibl.sample_equirect(src, np.array([[1.0, 1.0]]))[0, 0] == pytest.approx(0.5 * (src[3, 7, 0] + src[3, 0, 0]))
    assert ibl.sample_equirect(src, np.array([[2.5 / 8, 1.5 / 4]]))[0, 0] == src[1, 2, 0]


def test_layout_offsets(ibl):
    assert [ibl.level_offset(8, l) for l in range(5)] == [0, 384, 480, 504, 510]
    levels = [np.full((6, 4 >> l, 4 >> l, 4), float(l)) for l in range(3)]
    flat = ibl.pack_cube(levels)
    assert flat.shape == (ibl.cube_texels(4, 3), 4) == (126, 4)
    back = ibl.unpack_cube(flat, 4, 3)
    assert all(np.array_equal(a, b) for a, b in zip(back, levels))


# ---- closed forms, float64 ------------------------------------------------------------------------------------------------------
CONSTANT = np.array([0.25, 1.5, 12.0, 1.0])


def constant_cube(size, levels):
    return [np.broadcast_to(CONSTANT, (6, size >> l, size >> l, 4)).copy() for l in range(levels)]


def test_mips_of_a_constant_are_that_constant(ibl):
    for level in ibl.cube_mips(constant_cube(16, 1)[0], 5):
        assert np.array_equal(level, np.broadcast_to(CONSTANT, level.shape))
    assert [l.shape[1] for l in ibl.cube_mips(constant_cube(16, 1)[0], 5)] == [16, 8, 4, 2, 1]


def test_prefilter_of_a_constant_environment_is_that_constant(ibl):
    out = ibl.prefilter(constant_cube(8, 4), 8, 4, 32)
    assert [l.shape for l in out] == [(6, 8, 8, 4), (6, 4, 4, 4), (6, 2, 2, 4), (6, 1, 1, 4)]
    for level in out:
        assert np.allclose(level[..., :3], CONSTANT[:3], rtol=1e-13, atol=0)
        assert np.all(level[..., 3] == 1.0)


def test_irradiance_of_a_constant_environment(ibl):
    """c * PI * mean(cos theta sin theta) over the 252 x 63 grid the shader's float32 loops make."""
    phis, thetas = ibl.irradiance_angles()
    assert len(phis) == 252 and len(thetas) == 63
    assert phis.dtype == np.float32 and float(phis[1]) == float(np.float32(0.025))
    th = thetas.astype(np.float64)
    want = CONSTANT[:3] * ibl.PI * np.mean(np.cos(th) * np.sin(th))
    out = ibl.irradiance(constant_cube(4, 1), 4)
    assert out.shape == (6, 4, 4, 4)
    assert np.allclose(out[..., :3], want, rtol=1e-12, atol=0)
    assert np.all(out[..., 3] == 1.0)


def lut_cell(ndv, roughness):
    """brdf_lut.hlsl:116-177 (IntegrateBRDF) in plain float64 Python, written from the shader, sharing nothing with the model."""
    pi = 3.14159265359
    vx, vz = math.sqrt(1.0 - ndv * ndv), ndv
    k = roughness * roughness / 2.0
    a = roughness * roughness
    A = B = 0.0
    for i in range(1024):
        bits = int("{:032b}".format(i)[::-1], 2)
        x, y = i / 1024.0, bits * 2.3283064365386963e-10
        phi = 2.0 * pi * x
        ct = math.sqrt((1.0 - y) / (1.0 + (a * a - 1.0) * y))
        st = math.sqrt(1.0 - ct * ct)
        h_t = (math.cos(phi) * st, math.sin(phi) * st, ct)
        # N = (0, 0, 1): up = (1, 0, 0), tangent = normalize(cross(up, N)) = (0, -1, 0), bitangent = cross(N, tangent) = (1, 0, 0)
        h = (h_t[1], -h_t[0], h_t[2])
        hl = math.sqrt(h[0] ** 2 + h[1] ** 2 + h[2] ** 2)
        h = tuple(c / hl for c in h)
        vdh = vx * h[0] + vz * h[2]
        l = (2.0 * vdh * h[0] - vx, 2.0 * vdh * h[1], 2.0 * vdh * h[2] - vz)
        ll = math.sqrt(l[0] ** 2 + l[1] ** 2 + l[2] ** 2)
        ndl = max(l[2] / ll, 0.0)
        ndh = max(h[2], 0.0)
        vdh = max(vdh, 0.0)
        if ndl > 0.0:
            g = (ndl / max(ndl * (1.0 - k) + k, 0.0001)) * (ndv / max(ndv * (1.0 - k) + k, 0.0001))
            g_vis = g * vdh / max(ndh * ndv, 0.0001)
            fc = (1.0 - vdh) ** 5
            A += (1.0 - fc) * g_vis
            B += fc * g_vis
    return A / 1024.0, B / 1024.0


def test_brdf_lut_known_answers(ibl):
    n = 8
    lut = ibl.brdf_lut(n)
    assert lut.shape == (n, n, 4) and np.all(lut[..., 2] == 0.0) and np.all(lut[..., 3] == 1.0)
    for col, row in ((0, 0), (5, 2), (7, 7)):
        a, b = lut_cell(max((col + 0.5) / n, 0.001), (row + 0.5) / n)
        assert lut[row, col, 0] == pytest.approx(a, rel=1e-10) and lut[row, col, 1] == pytest.approx(b, rel=1e-10, abs=1e-14)
    # a smooth surface seen head on reflects F0 unchanged: scale -> 1, bias -> 0
    assert lut[0, n - 1, 0] == pytest.approx(1.0, abs=2e-2) and lut[0, n - 1, 1] < 1e-2


def test_equirect_of_an_analytic_function_reproduces_it(ibl):
    """The equirectangular image stores analytic_radiance at its pixel centres; the cube made from it must equal analytic_radiance
    at the cube's texel centres up to the bilinear interpolation error, bounded here from the function's derivatives:
    |error| <= (dphi^2 + dtheta^2) / 8 * max |second derivative along phi or theta|, and along a great-circle parameter the second
    derivative of f(d(t)) is at most |Hessian f| |d'|^2 + |grad f| |d''| <= M2 + M1 with |d'|, |d''| <= 1.
    analytic_radiance: the lobe P exp(-k (1 - a.d)) has |grad| <= P k and |Hessian| <= P k^2 (channel scale <= 1); the polynomial
    parts have |grad| <= 1.0 and |Hessian| <= 0.5."""
    w, h = cases.EQUIRECT_EXTENT
    m1 = ibl.LOBE_PEAK * ibl.LOBE_SHARPNESS + 1.0
    m2 = ibl.LOBE_PEAK * ibl.LOBE_SHARPNESS ** 2 + 0.5
    dphi, dtheta = 2.0 * math.pi / w, math.pi / h
    tol = (dphi ** 2 + dtheta ** 2) / 8.0 * (m1 + m2)
    src = ibl.analytic_equirect(w, h)
    for size in cases.EQUIRECT_CUBE_SIZES:
        d = ibl.texel_directions(size)
        # every texel centre lies between two rows' centres, so the lookup interpolates (the bound does not cover the clamped border)
        assert np.max(np.abs(np.arcsin(d[..., 1]))) <= math.pi / 2 - dtheta / 2
        got = ibl.equirect_to_cube(src, size)
        want = ibl.analytic_environment(size)
        worst = float(np.max(np.abs(got - want)))
        print(f"equirect -> {size}^2: max |error| {worst:.4f}, bound {tol:.4f}")
        assert worst <= tol
        assert worst > 0.0


def test_analytic_environment_is_smooth_hdr(ibl):
    env = ibl.analytic_environment(16)
    assert env.shape == (6, 16, 16, 4) and np.all(env[..., :3] > 0.0) and np.all(env[..., 3] == 1.0)
    assert 15.0 < env[..., 0].max() <= 1.75 + ibl.LOBE_PEAK
    assert abs(np.linalg.norm(ibl.LOBE_AXIS) - 1.0) < 1e-12


def test_up_vector_branches_are_not_on_a_knife_edge(ibl):
    """No texel centre of any size the tests use has | |N.z| - 0.999 | (prefilter_map.hlsl:74) or | |N.y| - 0.999 |
    (irradiance_map.hlsl:84) below 1e-5, so float32 and float64 take the same branch.  Sizes >= 32 take the alternate up vector
    somewhere (as does size 1, whose only texel centre is the axis itself), sizes 2 to 16 nowhere."""
    for n in cases.N_SIZES:
        d = ibl.texel_directions(n)
        for axis in (1, 2):
            margin = float(np.min(np.abs(np.abs(d[..., axis]) - 0.999)))
            assert margin >= 1e-5, (n, axis, margin)
            assert bool(np.any(np.abs(d[..., axis]) >= 0.999)) == (n >= 32 or n == 1), (n, axis)
        d32 = ibl.texel_directions(n, np.float32)
        assert np.array_equal(np.abs(d32[..., 1:]) < np.float32(0.999), np.abs(d[..., 1:]) < 0.999)


def test_float32_model_follows_the_float64_model(ibl):
    """The same operations in float32: close to float64, and float32 throughout (no silent promotion)."""
    env = cases.environment()
    assert all(l.dtype == np.float32 for l in env)
    m64, m32 = cases.irradiance_models(8)
    assert m32.dtype == np.float32 and m64.dtype == np.float64
    assert 0.0 < cases.err(m32, m64) < 1e-4
    p64, p32 = cases.prefilter_models(16, 5, 1024)
    assert all(l.dtype == np.float32 for l in p32)
    l64, l32 = cases.lut_models(32)
    assert l32.dtype == np.float32 and 0.0 < cases.err(l32, l64) < 1e-2
