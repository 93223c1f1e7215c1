"""SKYBOX without a GPU: the numpy model of the sky (renderer-rs_amd/ibl.py skybox_*) against closed forms, the header / Python / C++ / Rust
agreement on the new enum value and function, the class, variant and launch shape a SKYBOX segment gets (mirhi_debug_scope_plan and
mirhi_debug_raster_choice make no HIP call), and the share of pixels the GPU test may leave out, from the float64 model alone."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import sky_cases as sky

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGS_SKY, PROGRAM_SKYBOX = 64, 6


@pytest.fixture(scope="module")
def ibl(mirhi):
    return mirhi.ibl


def _inv_vp(scenes, yaw, pitch, w, h, fov=60.0):
    return scenes.inverse_view_projection(scenes.sky_rotation(yaw, pitch), scenes.perspective_rh(math.radians(fov), w / h, 0.1, 100.0))


# ---- the model against closed forms -------------------------------------------------------------------------------------------------------
def test_centre_of_an_unrotated_symmetric_camera_looks_down_minus_z(ibl, scenes):
    w, h = 64, 48
    d = ibl.skybox_directions(_inv_vp(scenes, 0.0, 0.0, w, h), (0, 0, w, h), w, h)
    centre = d[h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 1].mean(axis=(0, 1))      # the four pixels around the frame's centre
    assert np.allclose(centre / np.linalg.norm(centre), (0.0, 0.0, -1.0), atol=1e-6)
    assert np.allclose(np.linalg.norm(d, axis=-1), 1.0, atol=1e-12)
    # the top row looks up (vertex/skybox.hlsl:40 flips y), the right column to +x, and the vertical field of view is the projection's
    assert d[0, w // 2, 1] > 0 > d[-1, w // 2, 1] and d[h // 2, -1, 0] > 0 > d[h // 2, 0, 0]
    top = ibl.skybox_local_pos(_inv_vp(scenes, 0.0, 0.0, w, h), (0.5, 0.5, w - 1, h), w, 1)[0, w // 2]      # (a pixel centre ON the viewport's top edge, on its vertical centre line)
    assert math.isclose(math.degrees(math.atan2(top[1], -top[2])), 30.0, abs_tol=1e-4)


def test_a_constant_environment_gives_a_constant_frame(ibl, scenes):
    c = np.array([0.3, 1.7, 6.0, 0.5])
    env = [np.broadcast_to(c, (6, 8, 8, 4)).copy()]
    for dtype, tol in ((np.float64, 1e-14), (np.float32, 1e-6)):
        f = ibl.skybox(env, _inv_vp(scenes, 0.9, -0.4, 40, 24), (0, 0, 40, 24), 40, 24, dtype)
        assert f.shape == (24, 40, 4) and np.allclose(f, c, rtol=tol, atol=0)


def test_analytic_environment_through_the_sky_is_the_analytic_radiance(ibl, scenes):
    """Bilinear error of an n^2 cube: |f''| h^2 / 8 per axis with h = 2 / n in face coordinates; analytic_radiance's second derivatives stay below
    ~900 (the lobe: 20 k^2 + 20 k with k = 6), and the not-seamless clamp adds a first-order h / 2 |f'| <= 0.5 / n * 140 in the half texel beside an
    edge.  Checked away from face edges with the second-order bound, everywhere with the first-order one."""
    n, w, h = 64, 96, 64
    M = _inv_vp(scenes, 0.6, 0.3, w, h)
    d = ibl.skybox_directions(M, (0, 0, w, h), w, h)
    f = ibl.skybox([ibl.analytic_environment(n)], M, (0, 0, w, h), w, h)
    ref = ibl.analytic_radiance(d)
    _, s, t = ibl.select_face(d)
    inner = (np.abs(s - 0.5) < 0.5 - 1.0 / n) & (np.abs(t - 0.5) < 0.5 - 1.0 / n)
    assert inner.mean() > 0.9
    assert np.abs(f - ref)[inner].max() < 2 * 900.0 * (2.0 / n) ** 2 / 8.0
    assert np.abs(f - ref).max() < 140.0 * 1.0 / n


def test_the_affine_rule_is_not_the_per_pixel_divide(ibl, scenes):
    """An inverse whose last row has x in it: the shaders divide at the three vertices and interpolate, which is not M clip / w per pixel."""
    w, h = 32, 24
    M = _inv_vp(scenes, 0.2, 0.1, w, h).astype(np.float64)      # [col, row]
    M[0, 3] = 0.35                                               # column 0 (x), row 3 (w)
    L = ibl.skybox_local_pos(M, (0, 0, w, h), w, h)
    xn = (np.arange(w) + 0.5) / (w / 2) - 1.0
    yn = (np.arange(h) + 0.5) / (h / 2) - 1.0
    clip = np.stack(np.broadcast_arrays(xn[None, :], -yn[:, None], 1.0, 1.0), axis=-1)
    wpos = clip @ M            # maths M = M.T: (M.T @ clip) = clip @ M
    per_pixel = wpos[..., :3] / wpos[..., 3:]
    assert np.abs(L - per_pixel).max() > 0.05 * np.abs(L).max()
    # ... and it IS the plane through the three vertex values
    v = [np.array([x, -y, 1.0, 1.0]) @ M for x, y in ibl.SKY_CLIP]
    v = [p[:3] / p[3] for p in v]
    a, b = (xn + 1.0) / 4.0, (yn + 1.0) / 4.0
    plane = v[0] + (v[1] - v[0]) * a[None, :, None] + (v[2] - v[0]) * b[:, None, None]
    assert np.allclose(L, plane, rtol=1e-13, atol=1e-13)
    # without x or y in the last row the two coincide
    M0 = _inv_vp(scenes, 0.2, 0.1, w, h).astype(np.float64)
    w0 = clip @ M0
    pp0 = w0[..., :3] / w0[..., 3:]
    assert np.abs(ibl.skybox_local_pos(M0, (0, 0, w, h), w, h) - pp0).max() < 1e-4 * np.abs(pp0).max()      # (the float32 inverse leaves 1e-8 in the last row beside w = 0.01)


def test_coverage_of_the_sky_triangle(ibl):
    full = ibl.skybox_coverage((0, 0, sky.W, sky.H), None, sky.W, sky.H)
    assert full.all()
    # an offset viewport: the triangle starts at its corner and reaches past its far edges (nothing clips it to the viewport), up to the hypotenuse
    c = ibl.skybox_coverage((40, 24, 32, 32), None, sky.W, sky.H)
    ys, xs = np.nonzero(c)
    assert xs.min() == 40 and ys.min() == 24 and c[24, 40 + 62] and not c[24, 40 + 63] and c[24 + 31, 40 + 31] and not c[24 + 31, 40 + 32]      # (a centre ON the hypotenuse is out: no top or left edge)
    assert (ibl.skybox_coverage((40, 24, 32, 32), (40, 24, 32, 32), sky.W, sky.H) == (c & (np.arange(sky.W)[None, :] < 72) & (np.arange(sky.H)[:, None] < 56))).all()
    # winding: positive height is clockwise on the screen (back-facing under COUNTER_CLOCKWISE), a negative height flips it
    assert not ibl.skybox_coverage((0, 0, sky.W, sky.H), None, sky.W, sky.H, cull_mode=2, front_face=0).any()
    assert ibl.skybox_coverage((0, 0, sky.W, sky.H), None, sky.W, sky.H, cull_mode=1, front_face=0).all()
    assert ibl.skybox_coverage((0, sky.H, sky.W, -sky.H), None, sky.W, sky.H, cull_mode=2, front_face=0).all()
    assert not ibl.skybox_coverage((0, sky.H, sky.W, -sky.H), None, sky.W, sky.H, cull_mode=2, front_face=1).any()
    assert not ibl.skybox_coverage((0, 0, sky.W, sky.H), None, sky.W, sky.H, cull_mode=3).any()


@pytest.mark.parametrize("camera, ties", [(0, 1), (1, 2)])
def test_the_gpu_cases_see_three_faces_and_leave_out_at_most_a_thousandth(mirhi, camera, ties):
    _, frame, dirs = sky.model(mirhi, camera, 16, 5)
    assert len(np.unique(mirhi.ibl.select_face(dirs)[0])) == 3
    assert int(mirhi.ibl.tie_mask(dirs).sum()) == ties <= 1e-3 * sky.W * sky.H
    assert frame.shape == (sky.H, sky.W, 4)


def test_lod_zero_only(mirhi):
    """The chain's further levels of skybox_case are scaled: a model (or kernel) that reads them shows."""
    scene, frame, _ = sky.model(mirhi, 0, 16, 5)
    one = mirhi.ibl.skybox(scene.sky.levels[:1], scene.sky.inv_view_proj, (0, 0, sky.W, sky.H), sky.W, sky.H)
    assert np.array_equal(one, frame)
    assert not np.allclose(scene.sky.levels[1], mirhi.ibl.cube_mips(scene.sky.levels[0], 2)[1])


# ---- agreement ------------------------------------------------------------------------------------------------------------------------------
def test_header_python_cpp_and_rust_agree_on_the_new_names(mirhi):
    header = open(os.path.join(ROOT, "include", "mirhi.h")).read()
    assert re.search(r"MIRHI_PROGRAM_SKYBOX = 6\b", header)
    assert mirhi.Program.SKYBOX == 6 == mirhi.scenes.PROGRAM_SKYBOX
    assert re.search(r"mirhi_result mirhi_cmd_bind_skybox\(mirhi_cmd\* cmd, mirhi_image\* environment\);", header)
    assert "#define MIRHI_ABI_VERSION 5u" in header and re.search(r"MIRHI_TEXTURE_COUNT = 6\b", header)
    res, args = mirhi._SIGNATURES["mirhi_cmd_bind_skybox"]
    assert res is C.c_int32 and args == [C.c_void_p] * 2
    assert hasattr(C.CDLL(mirhi.LIB_PATH), "mirhi_cmd_bind_skybox") and mirhi.lib().mirhi_abi_version() == 5
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "mirhi-sys", "src", "lib.rs")).read()
    assert "pub const MIRHI_PROGRAM_SKYBOX: mirhi_program = 6;" in sys_rs
    assert "pub fn mirhi_cmd_bind_skybox(cmd: *mut mirhi_cmd, environment: *mut mirhi_image) -> mirhi_result;" in sys_rs
    assert "mirhi_sys::mirhi_cmd_bind_skybox(" in open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", "command.rs")).read()
    assert "Skybox = 6" in open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", "pipeline.rs")).read()
    hpp = open(os.path.join(ROOT, "renderer-rs_amd", "host", "mirhi.hpp")).read()
    assert "Skybox = 6" in hpp and "mirhi_cmd_bind_skybox(" in hpp


# ---- the plan of a SKYBOX segment -----------------------------------------------------------------------------------------------------------
def _raster_choice(mirhi, programs, zflip=0, zmask=0xFFFFFFFF, pred=0, tp=0, teams=1, wide=0, swz=1, allow=1, n_batch=0):
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_raster_choice
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    name, shape = C.create_string_buffer(96), (C.c_uint32 * 4)()
    rc = fn((C.c_uint32 * 12)(programs, allow, pred, zflip, zmask, tp, teams, wide, 0, swz, 0, n_batch), name, len(name), shape)
    return rc, name.value.decode(), tuple(shape)


def test_a_sky_segment_launches_the_sky_kernel_whatever_the_selectors_say(mirhi):
    for zflip in (0, 0xFFFFFFFF):
        for pred in (0, 3, 7):
            for tp, teams, wide, swz, allow in ((0, 1, 0, 1, 1), (64, 2, 16, 4, 1), (64, 1, 8, 1, 0)):
                rc, name, shape = _raster_choice(mirhi, PROGS_SKY, zflip=zflip, pred=pred, tp=tp, teams=teams, wide=wide, swz=swz, allow=allow)
                assert (rc, name, shape) == (0, "sky_kernel", (5, 4, 1, 256))
    assert _raster_choice(mirhi, PROGS_SKY, n_batch=2)[0] == 1           # no batched form
    assert _raster_choice(mirhi, 4 | 32)[1].startswith("raster_kernel_ibl<")      # the family before it keeps its kernels


def test_scope_plan_of_a_sky_segment(mirhi, monkeypatch):
    for k in list(os.environ):
        if k.startswith("MIRHI_"):
            monkeypatch.delenv(k)
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_scope_plan
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32]
    one = np.float32(1.0).view(np.uint32)
    for test, compare, write in ((1, 3, 0), (1, 1, 1), (0, 7, 0), (1, 5, 1), (1, 4, 0)):
        for tris, spread, wide in ((0, 0, 0), (1, 1, 16)):
            words = [1, test, compare, write, 0, 0, int(one), 0, 20, tris, spread, wide, 1, 1, 1, PROGRAM_SKYBOX, 0, 0]
            out, name = (C.c_uint32 * 32)(), C.create_string_buffer(96)
            assert fn((C.c_uint32 * len(words))(*words), out, name, len(name)) == 0
            ordered, masked, tri_prog, shadowed, is_ibl, own_family, programs = out[8:15]
            tp, teams, wide_eligible, xcd_bins, wide_out, swz = out[15:21]
            assert (ordered, masked, tri_prog, shadowed, is_ibl, own_family, programs) == (0, 0, 0, 0, 0, 1, PROGS_SKY)
            assert (tp, teams, wide_eligible, xcd_bins, wide_out, swz) == (0, 1, 0, 0, 0, 1)
            assert name.value.decode() == "sky_kernel" and tuple(out[28:32]) == (5, 4, 1, 256)
