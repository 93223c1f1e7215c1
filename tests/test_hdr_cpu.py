"""Radiance .hdr decode on the host (renderer-rs_amd/host/image_decode.hpp through include/miresources.h), and the
bindings of the two device operations on RGBE bytes.  No GPU.  The inputs and their expected texels are in hdr_cases.py; decoded
values are exact in binary32, so they are compared bit for bit."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as _ge  # noqa: E402

_ge.load_package()
from renderer_rs_amd import images  # noqa: E402

import hdr_cases as cases  # noqa: E402

MIRES_OK, MIRES_ERR_DECODE = 0, 1


@pytest.fixture(scope="module", autouse=True)
def _built():
    images.build()


def c_decode(data: bytes):
    """Through the C ABI itself: (rc, message, rgbe or None, exposure)."""
    L = images.lib()
    img = images._MiresHdr()
    rc = L.mires_hdr_decode(data, len(data), C.byref(img))
    if rc != MIRES_OK:
        assert not img.rgbe and img.width == 0 and img.height == 0      # nothing is handed over on failure
        return rc, L.mires_last_error_message().decode(), None, None
    try:
        n = img.width * img.height * 4
        return rc, "", np.ctypeslib.as_array(img.rgbe, shape=(n,)).copy().reshape(img.height, img.width, 4), float(img.exposure)
    finally:
        L.mires_hdr_free(C.byref(img))
        assert not img.rgbe and img.width == 0                          # zeroed
        L.mires_hdr_free(C.byref(img))                                  # and freeing it again is harmless
        L.mires_hdr_free(None)


@pytest.mark.parametrize("name,data,want,exposure", cases.GOOD_FILES, ids=[c[0] for c in cases.GOOD_FILES])
def test_hand_written_files(name, data, want, exposure):
    rc, msg, got, exp = c_decode(data)
    assert rc == MIRES_OK, msg
    assert got.shape == want.shape and np.array_equal(got, want)
    assert exp == exposure
    img = images.decode_hdr(data)
    assert (img.width, img.height) == (want.shape[1], want.shape[0]) and img.rgbe.dtype == np.uint8
    assert np.array_equal(img.rgbe, want) and img.exposure == exposure
    f = img.to_float()
    assert f.dtype == np.float32 and np.array_equal(f.view(np.uint32), cases.decode_float(want).view(np.uint32))


def test_the_1x1_file_in_floats_and_load_hdr(tmp_path):
    assert np.array_equal(images.decode_hdr(cases.FILE_1X1).to_float(), cases.WANT_1X1_FLOAT)
    assert np.array_equal(cases.decode_float(cases.WANT_8X2)[1, 0], [0.0, 0.0, 0.0, 1.0])      # E = 0 under a non-zero mantissa
    p = tmp_path / "env.hdr"
    p.write_bytes(cases.FILE_8X2)
    img = images.load_hdr(str(p))
    assert np.array_equal(img.rgbe, cases.WANT_8X2)
    with pytest.raises(images.ImageDecodeError) as e:
        images.load_hdr(str(tmp_path / "missing.hdr"))
    assert e.value.code == 2
    (tmp_path / "bad.hdr").write_bytes(cases.FILE_8X2[:-1])
    with pytest.raises(images.ImageDecodeError) as e:
        images.load_hdr(str(tmp_path / "bad.hdr"))
    assert e.value.code == MIRES_ERR_DECODE and "bad.hdr" in str(e.value) and "truncated" in str(e.value)


def test_to_float_of_every_mantissa_and_exponent():
    x = cases.all_pairs()
    got = images.HdrImage(x).to_float()
    m, e = x[..., :3].astype(np.float32), x[..., 3].astype(np.int32)
    want = np.ones((256, 256, 4), dtype=np.float32)
    want[..., :3] = np.ldexp(m, (e - 136)[..., None])
    want[0, :, :3] = 0.0                                                # E = 0 rows
    assert want.dtype == np.float32 and np.all(np.isfinite(want))
    assert want[1, 1, 0] == np.float32(2.0) ** -135 and want[255, 255, 0] == np.float32(255.0) * np.float32(2.0) ** 119
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(cases.decode_float(x).view(np.uint32), want.view(np.uint32))


_ROUND_TRIPS = cases.round_trip_images()


@pytest.mark.parametrize("rle", (True, False), ids=("rle", "flat"))
@pytest.mark.parametrize("name,x", _ROUND_TRIPS, ids=[c[0] for c in _ROUND_TRIPS])
def test_encode_decode_round_trip(name, x, rle):
    data = images.encode_hdr(x, rle=rle)
    back = images.decode_hdr(data)
    assert back.rgbe.shape == x.shape and np.array_equal(back.rgbe, x) and back.exposure == 1.0
    w = x.shape[1]
    if rle and 8 <= w <= 32767:
        assert len(data) < 64 + x.size + 2 * (x.size // 128 + 8 * x.shape[0])      # literals cost at most one count byte per 128
        if name.startswith("one repeated"):
            assert len(data) < 64 + x.shape[0] * (4 + 4 * 2 * (w // 127 + 2))       # ... and a repeated texel is runs
    else:
        assert data.endswith(x.tobytes())


def test_encode_hdr_is_deterministic_and_refuses_what_it_cannot_write():
    x = cases.random_rgbe(64, 2, 9)
    assert images.encode_hdr(x) == images.encode_hdr(x.copy())
    # the rule of the docstring on one plane: 5 x 7 -> a run; (1, 2) literal; 130 x 9 -> runs of 127 and 3; 2 x 4 literal
    plane = np.array([7] * 5 + [1, 2] + [9] * 130 + [4, 4], dtype=np.uint8)
    assert images._encode_plane(plane) == bytes([133, 7, 2, 1, 2, 255, 9, 131, 9, 2, 4, 4])
    # 128 equal bytes: a run of 127 and one byte left, which is a literal
    assert images._encode_plane(np.full(128, 3, dtype=np.uint8)) == bytes([255, 3, 1, 3])
    marker = np.zeros((1, 16, 4), dtype=np.uint8)
    marker[0, 5] = (1, 1, 1, 9)
    with pytest.raises(ValueError):
        images.encode_hdr(marker, rle=False)
    assert np.array_equal(images.decode_hdr(images.encode_hdr(marker)).rgbe, marker)
    first = np.zeros((1, 16, 4), dtype=np.uint8)
    first[0, 0] = (2, 2, 0, 16)
    with pytest.raises(ValueError):
        images.encode_hdr(first, rle=False)
    with pytest.raises(ValueError):
        images.encode_hdr(np.zeros((4, 4, 3), dtype=np.uint8))


def test_every_proper_prefix_of_the_8x2_file_is_a_decode_error():
    for n in range(len(cases.FILE_8X2)):
        rc, msg, _, _ = c_decode(cases.FILE_8X2[:n])
        assert rc == MIRES_ERR_DECODE and msg, (n, rc, msg)
        with pytest.raises(images.ImageDecodeError) as e:
            images.decode_hdr(cases.FILE_8X2[:n])
        assert e.value.code == MIRES_ERR_DECODE


@pytest.mark.parametrize("name,data,text", cases.BAD_FILES, ids=[c[0] for c in cases.BAD_FILES])
def test_refusals_name_their_cause(name, data, text):
    t0 = time.perf_counter()
    rc, msg, _, _ = c_decode(data)
    dt = time.perf_counter() - t0
    print(f"{name}: {msg!r} in {dt * 1e3:.2f} ms")
    assert rc == MIRES_ERR_DECODE and text in msg, (rc, msg)
    assert dt < 1.0                                                     # (a header's claim drives no large allocation)
    with pytest.raises(images.ImageDecodeError) as e:
        images.decode_hdr(data)
    assert e.value.code == MIRES_ERR_DECODE and text in str(e.value)


def test_null_arguments_and_the_png_jpeg_path():
    L = images.lib()
    img = images._MiresHdr()
    assert L.mires_hdr_decode(None, 0, C.byref(img)) == 3 and L.mires_hdr_decode(b"x", 1, None) == 3
    assert L.mires_hdr_to_float(None, None) == 3
    # mires_image_decode goes on refusing .hdr bytes; the decoder of .hdr refuses a PNG
    for data in (cases.FILE_1X1, cases.FILE_8X2, cases.FILE_RGBE_SIGNATURE):
        with pytest.raises(images.ImageDecodeError) as e:
            images.decode_image(data)
        assert e.value.code == MIRES_ERR_DECODE and "PNG and JPEG" in str(e.value)
    png = open(os.path.join(ROOT, "tests", "golden", "textures", "Metal049A.png"), "rb").read()
    assert images.decode_image(png).rgba.shape[2] == 4
    with pytest.raises(images.ImageDecodeError) as e:
        images.decode_hdr(png)
    assert e.value.code == MIRES_ERR_DECODE and "signature" in str(e.value)


# ---- bindings ------------------------------------------------------------------------------------------------------------------------
NEW_MIRHI = ("mirhi_image_expand_rgbe", "mirhi_ibl_equirect_to_cube_rgbe")
NEW_MIRES = ("mires_hdr_decode", "mires_hdr_load", "mires_hdr_free", "mires_hdr_to_float")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_new_names_are_in_every_mirror(mirhi):
    header, res_header = _read("include", "mirhi.h"), _read("include", "miresources.h")
    for name in NEW_MIRHI:
        assert re.search(r"mirhi_result\s+%s\(mirhi_image\* rgbe8, mirhi_image\* \w+\);" % name, header), name
        assert "pub fn %s(" % name in _read("bindings", "rust", "mirhi-sys", "src", "lib.rs"), name
        assert name in mirhi._SIGNATURES
    assert "still 5 (new functions only): mirhi_image_expand_rgbe, mirhi_ibl_equirect_to_cube_rgbe" in header
    for name in NEW_MIRES:
        assert re.search(r"^(int32_t|void)\s+\(%s\)\(" % name, res_header, re.M), name       # (declared; the declarator is parenthesised)
        assert hasattr(images.lib(), name), name
    assert ".hdr -> RGBE8 rows" in res_header and "mires_hdr;" in res_header
    image_rs, hpp = _read("bindings", "rust", "renderer-rhi-hip", "src", "image.rs"), _read("renderer-rs_amd", "host", "mirhi.hpp")
    for method, c_name in (("expand_rgbe", "mirhi_image_expand_rgbe"), ("ibl_equirect_to_cube_rgbe", "mirhi_ibl_equirect_to_cube_rgbe")):
        assert "pub fn %s(&self, rgbe8: &Image)" % method in image_rs and "mirhi_sys::%s(rgbe8.raw, self.raw)" % c_name in image_rs
        assert "void %s(const Image& rgbe8) const { check(%s(rgbe8.h_, h_)); }" % (method, c_name) in hpp
        assert callable(getattr(mirhi.Image, method))
    assert callable(mirhi.Image.from_hdr) and callable(mirhi.load_environment)
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py"), "--check"], capture_output=True).returncode == 0
    assert mirhi.ABI_VERSION == 5 and "#define MIRHI_ABI_VERSION 5u" in header


def test_the_library_exports_them_and_the_abi_is_5(mirhi):
    L = mirhi.lib()
    assert L.mirhi_abi_version() == 5
    for name in NEW_MIRHI:
        assert hasattr(L, name)
    # NULL is refused before anything touches a device
    assert L.mirhi_image_expand_rgbe(None, None) == mirhi.ERR_INVALID_HANDLE and b"the RGBE source is null" in L.mirhi_last_error_message()
    assert L.mirhi_ibl_equirect_to_cube_rgbe(None, None) == mirhi.ERR_INVALID_HANDLE and b"the RGBE source is null" in L.mirhi_last_error_message()


def test_the_ctypes_mires_hdr_is_the_headers(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler builds the oracle: it is there"
    fields = [f for f, _ in images._MiresHdr._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "miresources.h"', 'int main(void) {', 'printf("sizeof %zu\\n", sizeof(mires_hdr));']
    lines += ['printf("%s %%zu\\n", offsetof(mires_hdr, %s));' % (f, f) for f in fields] + ["return 0; }"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    out = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split("\n")
    seen = {l.split()[0]: int(l.split()[1]) for l in out if l}
    assert seen["sizeof"] == C.sizeof(images._MiresHdr) == 24
    for f in fields:
        assert seen[f] == getattr(images._MiresHdr, f).offset, f


def test_a_translation_unit_that_calls_the_new_hpp_methods_compiles(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx
    (tmp_path / "calls.cpp").write_text('''
#include "mirhi.hpp"
#include "image_decode.hpp"
void calls(std::shared_ptr<mirhi::Device> dev, const uint8_t* bytes, size_t n) {
    mirhi::resources::HdrData hdr = mirhi::resources::decode_hdr(bytes, n);
    mirhi::Image rgbe = mirhi::Image::from_rgbe(dev, hdr.width, hdr.height, hdr.rgbe.data());
    mirhi::Image flt(dev, hdr.width, hdr.height, mirhi::Format::R32G32B32A32_SFLOAT);
    flt.expand_rgbe(rgbe);
    mirhi::Image cube = mirhi::Image::cube(dev, 64, 7);
    cube.ibl_equirect_to_cube_rgbe(rgbe);
    cube.ibl_cube_generate_mips();
}
''')
    subprocess.check_call([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "renderer-rs_amd", "host"),
                           str(tmp_path / "calls.cpp")])
