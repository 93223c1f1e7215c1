"""The recorded transfer commands without a GPU: the numpy model of tests/transfer_cases.py against closed forms, the share of channels the 8-bit
GPU cases may leave out (from the float64 model alone), the agreement of header, ctypes, the Rust crates and mirhi.hpp on the seven functions and
four structs, and the kernel a transfer entry selects (mirhi_debug_raster_choice makes no HIP call)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import transfer_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("copy_buffer", "copy_buffer_to_image", "copy_image_to_buffer", "copy_image", "blit_image", "clear_color_image", "clear_depth_stencil_image")
STRUCTS = {"mirhi_buffer_copy": "BufferCopy", "mirhi_buffer_image_copy": "BufferImageCopy", "mirhi_image_copy": "ImageCopy", "mirhi_image_blit": "ImageBlit"}
PROGS_TRANSFER = 128
XFER_COPY, XFER_BLIT_NEAREST, XFER_BLIT_LINEAR, XFER_FILL = 1, 2, 3, 4


# ---- the model against closed forms -------------------------------------------------------------------------------------------------------
def _whole(w, h):
    return ((0, 0), (w, h))


def test_nearest_one_to_one_is_the_identity():
    src = tc.decode(tc.source(tc.RGBA32F), tc.RGBA32F)
    assert np.array_equal(tc.blit(src, _whole(24, 20), _whole(24, 20), False), src)
    assert np.array_equal(tc.blit(src, ((3, 2), (16, 13)), ((5, 1), (18, 12)), False), src[2:13, 3:16])


def test_nearest_two_times_upscale_repeats_texels():
    src = tc.decode(tc.source(tc.RGBA8_UNORM), tc.RGBA8_UNORM)
    assert np.array_equal(tc.blit(src, _whole(24, 20), _whole(48, 40), False), src.repeat(2, axis=0).repeat(2, axis=1))


def test_linear_reproduces_a_horizontal_ramp_away_from_the_clamped_edge():
    w, h, dw = 24, 4, 37
    ramp = np.broadcast_to((np.arange(w, dtype=np.float64) * 0.25 + 1.0)[None, :, None], (h, w, 4))
    out = tc.blit(ramp, _whole(w, h), ((0, 0), (dw, h)), True)
    u = (np.arange(dw) + 0.5) * w / dw                       # the ramp is 0.25 (u - 1/2) + 1 where both taps exist
    inner = (u - 0.5 >= 0) & (u - 0.5 <= w - 1)
    assert inner.sum() >= dw - 2
    assert np.allclose(out[:, inner, 0], (0.25 * (u[inner] - 0.5) + 1.0)[None, :], rtol=1e-14)
    assert np.allclose(out[:, 0], ramp[:, 0]) and np.allclose(out[:, -1], ramp[:, -1])      # edge clamp: the end values, not an extrapolation


def test_reversed_offsets_flip():
    src = tc.decode(tc.source(tc.RGBA32F), tc.RGBA32F)
    for linear in (False, True):
        plain = tc.blit(src, _whole(24, 20), _whole(37, 29), linear)
        assert np.allclose(tc.blit(src, _whole(24, 20), ((37, 0), (0, 29)), linear), plain[:, ::-1], rtol=1e-14)
        assert np.allclose(tc.blit(src, ((0, 20), (24, 0)), _whole(37, 29), linear), plain[::-1], rtol=1e-14)
        assert np.allclose(tc.blit(src, ((24, 20), (0, 0)), _whole(37, 29), linear), plain[::-1, ::-1], rtol=1e-14)
    assert np.array_equal(tc.blit(src, _whole(24, 20), ((24, 0), (0, 20)), False), src[:, ::-1])


def test_edge_clamp_of_the_index_choice():
    i, lo, hi, num, den = tc.axis_taps(0, 8, 0, 4, 4, True)      # a 2x upscale: u - 1/2 = (i + 1/2) / 2 - 1/2
    assert lo.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and hi.tolist() == [0, 1, 1, 2, 2, 3, 3, 3]
    assert (num / den).tolist() == [0.75, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.25]
    _, lo, _, _, _ = tc.axis_taps(0, 37, 0, 24, 24, False)
    assert lo[18] == 12                                          # (18 + 1/2) 24 / 37 is 12 exactly: floor is formed in integers, no rounding decides it
    assert lo.min() == 0 and lo.max() == 23


def test_srgb_decode_then_encode_of_every_byte_is_the_identity(oracle):
    L = oracle.lib()
    assert [L.oracle_srgb8(float(v)) for v in tc.SRGB_LUT] == list(range(256))
    bytes_ = np.arange(256, dtype=np.uint8)
    texels = np.stack([bytes_, bytes_[::-1], bytes_, bytes_], axis=-1)[None]
    for fmt in (tc.BGRA8_SRGB, tc.RGBA8_SRGB, tc.RGBA8_UNORM):
        assert np.array_equal(tc.encode(tc.decode(texels, fmt), fmt), texels)
        assert np.array_equal(tc.encode(tc.decode(texels, fmt, np.float32), fmt), texels)
    # the model's encoder is the oracle's on values all over [0, 1] and beyond
    vals = np.concatenate([np.linspace(-0.25, 1.25, 1531), tc.SRGB_LUT.astype(np.float64), [0.0031308, 0.003, 0.0032]]).astype(np.float32)
    mine = tc.encode(np.stack([vals, vals, vals, vals], axis=-1), tc.RGBA8_SRGB)[:, 0]
    assert mine.tolist() == [L.oracle_srgb8(float(v)) for v in vals]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_8_bit_gpu_cases_leave_out_under_two_percent(seed):
    """From the float64 model alone: the undecided share of the LINEAR 24 x 20 -> 37 x 29 cases and of the 13 x 11 sub-region."""
    for sf in (tc.RGBA8_SRGB, tc.RGBA32F):
        src = tc.decode(tc.source(sf, seed), sf)
        for df in (tc.RGBA8_UNORM, tc.BGRA8_SRGB, tc.RGBA8_SRGB):
            for srect, drect in ((_whole(24, 20), _whole(37, 29)), (_whole(24, 20), ((3, 2), (16, 13)))):
                share = tc.undecided(tc.blit(src, srect, drect, True), df).mean()
                assert share < 0.02, (sf, df, drect, share)


# ---- agreement ------------------------------------------------------------------------------------------------------------------------------
def test_header_ctypes_and_rust_agree_on_functions_and_structs(mirhi):
    header = open(os.path.join(ROOT, "include", "mirhi.h")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "mirhi-sys", "src", "lib.rs")).read()
    cmd_rs = open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", "command.rs")).read()
    hpp = open(os.path.join(ROOT, "renderer-rs_amd", "host", "mirhi.hpp")).read()
    assert "#define MIRHI_ABI_VERSION 5u" in header and mirhi.lib().mirhi_abi_version() == 5
    so = C.CDLL(mirhi.LIB_PATH)
    for f in FUNCTIONS:
        decl = re.search(r"mirhi_result mirhi_cmd_%s\(([^;]*)\);" % f, header)
        assert decl, f
        arity = len(decl.group(1).split(","))
        res, args = mirhi._SIGNATURES["mirhi_cmd_" + f]
        assert res is C.c_int32 and len(args) == arity, f
        assert hasattr(so, "mirhi_cmd_" + f)
        rust = re.search(r"pub fn mirhi_cmd_%s\(([^;]*)\) -> mirhi_result;" % f, sys_rs)
        assert rust and len(rust.group(1).split(",")) == arity, f
        assert re.search(r"pub fn %s\(&self" % f, cmd_rs) and ("mirhi_sys::mirhi_cmd_%s(" % f) in cmd_rs, f
        assert re.search(r"void %s\(" % f, hpp) and ("mirhi_cmd_%s(h_" % f) in hpp, f
        assert callable(getattr(mirhi.CommandBuffer, f))
    for c_name, py_name in STRUCTS.items():
        assert re.search(r"\}\s*%s;" % c_name, header) and ("pub struct %s {" % c_name) in sys_rs and c_name in cmd_rs
        assert issubclass(getattr(mirhi, py_name), C.Structure)
    assert re.search(r"MIRHI_FILTER_NEAREST = 0, MIRHI_FILTER_LINEAR = 1", header) and (mirhi.Filter.NEAREST, mirhi.Filter.LINEAR) == (0, 1)
    assert "pub const MIRHI_FILTER_LINEAR: mirhi_filter = 1;" in sys_rs and "Linear = 1" in cmd_rs
    assert subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True).returncode == 0


def test_struct_layouts_in_ctypes_equal_the_headers(mirhi, tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler builds the oracle: it is there"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mirhi.h"', 'int main(void) {']
    for c_name, py_name in STRUCTS.items():
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (c_name, c_name))
        for field, _ in getattr(mirhi, py_name)._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (c_name, field, c_name, field))
    lines += ["return 0; }"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split("\n")
    seen = {tuple(l.split()[:2]): int(l.split()[2]) for l in out if l}
    for c_name, py_name in STRUCTS.items():
        cls = getattr(mirhi, py_name)
        assert seen[(c_name, "sizeof")] == C.sizeof(cls), c_name
        for field, _ in cls._fields_:
            assert seen[(c_name, field)] == getattr(cls, field).offset, (c_name, field)
    assert {n: seen[(n, "sizeof")] for n in STRUCTS} == {"mirhi_buffer_copy": 24, "mirhi_buffer_image_copy": 40, "mirhi_image_copy": 32, "mirhi_image_blit": 40}


def test_a_translation_unit_that_calls_each_new_hpp_method_compiles(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx
    (tmp_path / "calls.cpp").write_text('''#include "mirhi.hpp"
void record(const mirhi::CommandBuffer& cmd, const mirhi::Buffer& a, const mirhi::Buffer& b, const mirhi::Image& x, const mirhi::Image& y) {
    cmd.copy_buffer(a, b, {mirhi_buffer_copy{0, 16, 64}});
    cmd.copy_buffer_to_image(a, x, {mirhi_buffer_image_copy{0, 0, 0, 0, {0, 0}, {4, 4}}});
    cmd.copy_image_to_buffer(x, b, {mirhi_buffer_image_copy{0, 8, 8, 0, {1, 1}, {2, 2}}});
    cmd.copy_image(x, y, {mirhi_image_copy{0, {0, 0}, 0, {0, 0}, {4, 4}}});
    cmd.blit_image(x, y, {mirhi_image_blit{0, {{0, 0}, {4, 4}}, 0, {{8, 8}, {0, 0}}}}, MIRHI_FILTER_LINEAR);
    const float red[4] = {1.0f, 0.0f, 0.0f, 1.0f};
    cmd.clear_color_image(x, red);
    cmd.clear_depth_stencil_image(y, 1.0f);
}
''')
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "renderer-rs_amd", "host"),
                           str(tmp_path / "calls.cpp")])


# ---- the kernel a transfer entry selects ------------------------------------------------------------------------------------------------------
def _raster_choice(mirhi, programs, kind=0, groups=0, zflip=0, zmask=0xFFFFFFFF, tp=0, teams=1, wide=0, swz=1, allow=1, n_batch=0):
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_raster_choice
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    name, shape = C.create_string_buffer(96), (C.c_uint32 * 4)()
    rc = fn((C.c_uint32 * 12)(programs, allow, kind, groups if programs == PROGS_TRANSFER else zflip, zmask, tp, teams, wide, 0, swz, 0, n_batch), name, len(name), shape)
    return rc, name.value.decode(), tuple(shape)


def test_a_transfer_entry_launches_its_kernel_whatever_the_selectors_say(mirhi):
    names = {XFER_COPY: "transfer_copy_kernel", XFER_BLIT_NEAREST: "transfer_blit_kernel<0>", XFER_BLIT_LINEAR: "transfer_blit_kernel<1>", XFER_FILL: "transfer_fill_kernel"}
    for kind, name in names.items():
        for groups in (1, 7, 2048):
            for tp, teams, wide, swz, allow in ((0, 1, 0, 1, 1), (64, 2, 16, 4, 1), (64, 1, 8, 1, 0)):
                assert _raster_choice(mirhi, PROGS_TRANSFER, kind, groups, tp=tp, teams=teams, wide=wide, swz=swz, allow=allow) == (0, name, (groups, 1, 1, 256))
        assert _raster_choice(mirhi, PROGS_TRANSFER, kind, 4, n_batch=2)[0] == 1            # no batched form
    assert _raster_choice(mirhi, 64)[1] == "sky_kernel"                                       # the family before it keeps its kernel
    assert _raster_choice(mirhi, 1)[1].startswith("raster_kernel<")
