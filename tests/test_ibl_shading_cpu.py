"""MODEL_PBR_IBL without a GPU: the numpy model of the ambient term (renderer-rs_amd/ibl.py) against closed forms, the header / Python / Rust
agreement on the new enum value and function, the raster variant a scope with a MODEL_PBR_IBL draw gets (mirhi_debug_raster_choice makes no HIP
call), and the camera of scenes.ibl_facets_case: the share of pixels the GPU test may leave out, from the float64 model alone."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import ibl_shading_cases as ibl_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGS_IBL = 32


@pytest.fixture(scope="module")
def ibl(mirhi):
    return mirhi.ibl


def _dirs(n, seed=3):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _constant_set(c, A, B, levels=5):
    irr = [np.broadcast_to(np.array(c + (1.0,)), (6, 8, 8, 4)).copy()]
    pre = [np.broadcast_to(np.array(c + (1.0,)), (6, 16 >> l, 16 >> l, 4)).copy() for l in range(levels)]
    lut = np.broadcast_to(np.array([A, B, 0.0, 1.0]), (16, 16, 4)).copy()
    return irr, pre, lut


@pytest.mark.parametrize("dtype, tol", [(np.float64, 1e-13), (np.float32, 2e-6)])
def test_ambient_closed_form_for_a_constant_environment(ibl, dtype, tol):
    """constant environment c, constant LUT (A, B): ambient = (kD c albedo + c (F0 A + B)) ao."""
    c, A, B = (0.7, 1.3, 2.1), 0.6, 0.15
    irr, pre, lut = _constant_set(c, A, B)
    N, V = _dirs(200, 1), _dirs(200, 2)
    rng = np.random.default_rng(5)
    albedo, metallic, rough, ao = rng.uniform(0.1, 1.0, (200, 3)), rng.uniform(0, 1, 200), rng.uniform(0, 1, 200), rng.uniform(0.2, 1, 200)
    got = ibl.ambient(irr, pre, lut, N, V, albedo, metallic, rough, ao, dtype)
    assert got.dtype == dtype
    r = np.maximum(rough, 0.04)
    F0 = 0.04 + (albedo - 0.04) * metallic[:, None]
    ndv = np.maximum(np.sum(N * V, axis=1), 0.0)
    F = F0 + (np.maximum((1.0 - r)[:, None], F0) - F0) * ((1.0 - ndv) ** 5)[:, None]
    kD = (1.0 - F) * (1.0 - metallic)[:, None]
    cc = np.array(c)
    want = (kD * cc * albedo + cc * (F0 * A + B)) * ao[:, None]
    assert np.max(np.abs(got - want) / np.abs(want)) < tol


def test_fresnel_is_f0_at_normal_incidence(ibl):
    F0 = np.array([[0.04, 0.5, 0.9]])
    for rough in (0.04, 0.3, 1.0):
        assert np.array_equal(ibl.fresnel_schlick_roughness(np.array([1.0]), F0, np.array([rough])), F0)
        # grazing: F90 = max(1 - roughness, F0)
        assert np.allclose(ibl.fresnel_schlick_roughness(np.array([0.0]), F0, np.array([rough])), np.maximum(1.0 - rough, F0), rtol=0, atol=1e-15)
    # cosTheta is saturated
    assert np.array_equal(ibl.fresnel_schlick_roughness(np.array([1.7]), F0, np.array([0.5])), F0)


def test_prefiltered_lod_clamps_at_the_last_level(ibl):
    """roughness * 7 beyond levels - 1 reads the last level alone: a 5-level cube saturates at roughness 4/7; an 8-level one does not."""
    N = _dirs(64, 7)
    V = N.copy()                                  # R = N, NdotV = 1: F = F0
    zero_irr = [np.zeros((6, 8, 8, 4))]
    lut = np.broadcast_to(np.array([1.0, 0.0, 0.0, 1.0]), (16, 16, 4))
    albedo, metallic = np.ones((64, 3)), np.ones(64)     # F0 = 1: ambient = prefiltered
    for levels, size in ((5, 16), (8, 128)):
        pre = [np.full((6, size >> l, size >> l, 4), float(l + 1)) for l in range(levels)]
        for rough in (4.0 / 7.0, 0.8, 1.0):
            got = ibl.ambient(zero_irr, pre, lut, N, V, albedo, metallic, rough, 1.0)
            lod = min(rough * 7.0, levels - 1)
            want = (1 - (lod - np.floor(lod))) * (np.floor(lod) + 1) + (lod - np.floor(lod)) * (min(np.floor(lod) + 1, levels - 1) + 1)
            assert np.allclose(got, want, rtol=1e-12), (levels, rough)
        if levels == 5:
            a = ibl.ambient(zero_irr, pre, lut, N, V, albedo, metallic, 4.0 / 7.0 + 1e-9, 1.0)
            assert np.allclose(a, 5.0, rtol=1e-12) and np.allclose(ibl.ambient(zero_irr, pre, lut, N, V, albedo, metallic, 1.0, 1.0), 5.0, rtol=1e-12)


def test_lut_lookup_clamps_to_the_edge(ibl):
    n = 16
    lut = np.zeros((n, n, 2))
    lut[..., 0] = np.arange(n)[None, :]           # column index: the NdotV axis
    lut[..., 1] = np.arange(n)[:, None]           # row index: the roughness axis
    got = ibl.sample_lut(lut, np.array([0.0, 1.0, 0.0, 1.0]), np.array([0.0, 0.0, 1.0, 1.0]))
    assert np.array_equal(got, np.array([[0.0, 0.0], [n - 1.0, 0.0], [0.0, n - 1.0], [n - 1.0, n - 1.0]]))
    # texel centres are exact, and u runs along a row
    c = (np.arange(n) + 0.5) / n
    assert np.allclose(ibl.sample_lut(lut, c, np.full(n, c[3]))[:, 0], np.arange(n), atol=1e-12)
    assert np.allclose(ibl.sample_lut(lut, c, np.full(n, c[3]))[:, 1], 3.0, atol=1e-12)
    # NdotV = 0 and roughness = 1 inside ambient: the edge texels, no texel from outside
    N = np.array([[0.0, 0.0, 1.0]]); V = np.array([[1.0, 0.0, 0.0]])
    pre = [np.ones((6, 4, 4, 4))]
    a = ibl.ambient([np.zeros((6, 2, 2, 4))], pre, np.dstack([lut, np.zeros((n, n, 2))]), N, V, np.ones((1, 3)), 1.0, 1.0, 1.0)
    assert np.allclose(a, 0.0 * 1.0 + (n - 1.0))              # F0 = 1: brdf.x + brdf.y = 0 + (n - 1)


def test_header_python_and_rust_agree_on_the_new_names(mirhi):
    header = open(os.path.join(ROOT, "include", "mirhi.h")).read()
    assert re.search(r"MIRHI_PROGRAM_MODEL_PBR_IBL = 5\b", header)
    assert mirhi.Program.MODEL_PBR_IBL == 5 == mirhi.scenes.PROGRAM_MODEL_PBR_IBL
    assert re.search(r"mirhi_result mirhi_cmd_bind_ibl\(mirhi_cmd\* cmd, mirhi_image\* irradiance, mirhi_image\* prefiltered, mirhi_image\* brdf_lut\);", header)
    assert "#define MIRHI_ABI_VERSION 5u" in header and re.search(r"MIRHI_TEXTURE_COUNT = 6\b", header)
    res, args = mirhi._SIGNATURES["mirhi_cmd_bind_ibl"]
    assert res is C.c_int32 and args == [C.c_void_p] * 4
    assert hasattr(C.CDLL(mirhi.LIB_PATH), "mirhi_cmd_bind_ibl")
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "mirhi-sys", "src", "lib.rs")).read()
    assert "pub const MIRHI_PROGRAM_MODEL_PBR_IBL: mirhi_program = 5;" in sys_rs
    assert "pub fn mirhi_cmd_bind_ibl(cmd: *mut mirhi_cmd, irradiance: *mut mirhi_image, prefiltered: *mut mirhi_image, brdf_lut: *mut mirhi_image) -> mirhi_result;" in sys_rs
    safe = open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", "command.rs")).read()
    assert "mirhi_sys::mirhi_cmd_bind_ibl(" in safe
    assert "ModelPbrIbl = 5" in open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", "pipeline.rs")).read()
    hpp = open(os.path.join(ROOT, "renderer-rs_amd", "host", "mirhi.hpp")).read()
    assert "ModelPbrIbl = 5" in hpp and "mirhi_cmd_bind_ibl(" in hpp


# ---- the raster variant of a scope with a MODEL_PBR_IBL draw -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def choose(mirhi):
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_raster_choice
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]

    def choose(programs, zflip=0, tp=0, teams=1, wide=0, swz=1, allow=1, n_batch=0):
        name, shape = C.create_string_buffer(96), (C.c_uint32 * 4)()
        rc = fn((C.c_uint32 * 12)(programs, allow, 0, zflip, 0xFFFFFFFF, tp, teams, wide, 0, swz, 0, n_batch), name, len(name), shape)
        return rc, name.value.decode(), tuple(shape)
    return choose


def test_ibl_scopes_select_the_ibl_family(choose):
    names = set()
    for shadow_bits, sv in ((0, 0), (8, 1), (24, 2)):
        for zflip, tp, teams, wide, allow in itertools.product((0, 0xFFFFFFFF), (0, 64), (1, 2), (0, 8, 16), (0, 1)):
            progs = 4 | PROGS_IBL | shadow_bits
            rc, name, shape = choose(progs, zflip, tp, teams, wide, 1, allow)
            assert rc == 0 and name == f"raster_kernel_ibl<{1 if zflip else 0}, {1 if tp else 0}, {sv}>", (progs, name)
            # never wide, never two teams: four waves per tile on the 2-D grid -- the launch shape of the shadowed families for the same parameters
            assert shape == (5, 4, 1, 256)
            for other in (12, 28):
                assert choose(other, zflip, tp, teams, wide, 1, allow)[2] == shape
            # never batched
            assert choose(progs, zflip, tp, teams, wide, 1, allow, n_batch=2)[0] == 1
            names.add(name)
    assert len(names) == 12           # 2 keys x 2 paths x 3 shadow terms: the shadow variants are distinct kernels


def test_program_sets_without_the_bit_keep_their_kernels(choose):
    for progs in (0, 1, 2, 3, 4, 7, 12, 28):
        for zflip, tp in itertools.product((0, 0xFFFFFFFF), (0, 64)):
            assert "raster_kernel_ibl" not in choose(progs, zflip, tp)[1]
    assert choose(12)[1].startswith("raster_kernel_shadow<") and choose(28)[1].startswith("raster_kernel_csm<") and choose(0)[1].startswith("raster_kernel_depth<")


# ---- scenes.ibl_facets_case ---------------------------------------------------------------------------------------------------------------
def test_facets_case_shape_and_left_out_share(scenes, ibl):
    """The properties the GPU test relies on, and the cap on the pixels it may leave out (R within 1e-4 of a face tie), from the float64 model."""
    for size, levels in ((16, 5), (128, 8)):
        sc = scenes.ibl_facets_case(pre_size=size, pre_levels=levels)
        assert 96 <= sc.width <= 160 and 64 <= sc.height <= 120 and len(sc.draws) == 12
        assert sc.ibl.irradiance.shape == (6, 8, 8, 4) and len(sc.ibl.prefiltered) == levels and sc.ibl.prefiltered[0].shape == (6, size, size, 4) and sc.ibl.lut.shape == (16, 16, 4)
        normals = np.array([f["normal"] for f in sc.facets], dtype=np.float64)
        a = np.sort(np.abs(normals), axis=1)
        assert np.all(a[:, 2] - a[:, 1] > 1e-3)
        assert set(ibl.select_face(normals)[0].tolist()) == {0, 1, 2, 3, 4, 5}
        assert {round(f["roughness"], 4) for f in sc.facets} == {0.0, 0.3, round(4 / 7, 4), 0.8, 1.0}
        assert {f["metallic"] for f in sc.facets} == {0.0, 0.5, 1.0}
        assert len({f["ao"] for f in sc.facets}) > 3 and sum(bool(np.any(f["emissive"] > 0)) for f in sc.facets) == 1
        for d in sc.draws:
            v = np.asarray(d.vertices)
            assert np.all(v[:, 3:6] == v[0, 3:6])
    prim = ibl_cases.software_prim(sc)
    py, px, facet = ibl_cases.facet_pixels(sc, prim)
    assert py.size > 0.25 * sc.width * sc.height and set(facet.tolist()) == set(range(12))
    keep = ibl_cases.keep_mask(sc, py, px, facet)
    left_out = 1.0 - keep.mean()
    print(f"ibl_facets_case: {py.size} covered pixels, left out {left_out:.5%}")
    assert left_out <= 1e-3
    # E32 of the model on this frame, what the GPU bound is made of
    for size, levels in ((16, 5), (128, 8)):
        sc = scenes.ibl_facets_case(pre_size=size, pre_levels=levels)
        m64, _ = ibl_cases.expected_ambient(sc, ibl_cases.scene_images(sc), py[keep], px[keep], facet[keep], np.float64)
        m32, _ = ibl_cases.expected_ambient(sc, ibl_cases.scene_images(sc), py[keep], px[keep], facet[keep], np.float32)
        e32 = ibl_cases.rel_err(m32, m64)
        print(f"ibl_facets_case {size}^2 x {levels}: E32 {e32:.3e} bound {ibl_cases.bound_for(e32):.3e}")
        assert np.all(np.isfinite(m64)) and e32 < 1e-3
