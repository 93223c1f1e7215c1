"""PNG / JPEG -> RGBA8 and Radiance .hdr -> RGBE8 through libmiresources.so (include/miresources.h; C++ in host/image_decode.hpp).

The texture-decode half of SURVEY.md section 8f rank 1.  The reference gets decoded images from `gltf::import` and drops
them (crates/resources/src/model.rs:120); this is the piece a caller needs to turn `assets/textures/*` or a glTF's
`images[]` into the RGBA8 texels `Image.write` / `scenes.Texture` take.  Host-only: no GPU is touched here, and there is
no Python fallback decoder -- a missing library is an error.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libmiresources.so")
SOURCES = [os.path.join(HERE, "host", "resources_capi.cpp"), os.path.join(HERE, "host", "image_decode.hpp"),
           os.path.join(HERE, "..", "include", "miresources.h")]


class ImageDecodeError(RuntimeError):
    """`.code` is the MIRES_ERR_* value."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


class _MiresImage(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("source_channels", C.c_uint32), ("reserved", C.c_uint32),
                ("rgba", C.POINTER(C.c_uint8))]


class _MiresHdr(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("exposure", C.c_float), ("reserved", C.c_uint32),
                ("rgbe", C.POINTER(C.c_uint8))]


def build(force: bool = False) -> str:
    """g++ -> renderer-rs_amd/libmiresources.so (host code only)."""
    if not force and os.path.exists(LIB) and all(os.path.getmtime(s) <= os.path.getmtime(LIB) for s in SOURCES):
        return LIB
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-shared", "-fPIC", "-o", LIB, SOURCES[0]])
    return LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise ImageDecodeError(2, f"{LIB} is missing: run `python -m renderer-rs_amd.build` / __graft_entry__.build()")
        l = C.CDLL(LIB)
        l.mires_image_decode.restype = C.c_int32
        l.mires_image_decode.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(_MiresImage)]
        l.mires_image_load.restype = C.c_int32
        l.mires_image_load.argtypes = [C.c_char_p, C.POINTER(_MiresImage)]
        l.mires_image_free.restype = None
        l.mires_image_free.argtypes = [C.POINTER(_MiresImage)]
        l.mires_hdr_decode.restype = C.c_int32
        l.mires_hdr_decode.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(_MiresHdr)]
        l.mires_hdr_load.restype = C.c_int32
        l.mires_hdr_load.argtypes = [C.c_char_p, C.POINTER(_MiresHdr)]
        l.mires_hdr_free.restype = None
        l.mires_hdr_free.argtypes = [C.POINTER(_MiresHdr)]
        l.mires_hdr_to_float.restype = C.c_int32
        l.mires_hdr_to_float.argtypes = [C.POINTER(_MiresHdr), C.c_void_p]
        l.mires_last_error_message.restype = C.c_char_p
        l.mires_last_error_message.argtypes = []
        _lib = l
    return _lib


class DecodedImage:
    """`rgba`: (h, w, 4) uint8, top row first; `source_channels`: what the file stored (1, 2, 3 or 4)."""

    def __init__(self, rgba: np.ndarray, source_channels: int):
        self.rgba, self.source_channels = rgba, source_channels

    @property
    def width(self) -> int:
        return int(self.rgba.shape[1])

    @property
    def height(self) -> int:
        return int(self.rgba.shape[0])


def _take(rc: int, img: _MiresImage) -> DecodedImage:
    l = lib()
    if rc != 0:
        raise ImageDecodeError(rc, (l.mires_last_error_message() or b"").decode("utf-8", "replace"))
    try:
        n = img.width * img.height * 4
        arr = np.ctypeslib.as_array(img.rgba, shape=(n,)).copy().reshape(img.height, img.width, 4)
        return DecodedImage(arr, int(img.source_channels))
    finally:
        l.mires_image_free(C.byref(img))


def decode_image(data: bytes) -> DecodedImage:
    img = _MiresImage()
    return _take(lib().mires_image_decode(bytes(data), len(data), C.byref(img)), img)


def load_image(path: str) -> DecodedImage:
    img = _MiresImage()
    return _take(lib().mires_image_load(os.fsencode(path), C.byref(img)), img)


# ---- Radiance .hdr ---------------------------------------------------------------------------------------------------
class HdrImage:
    """`rgbe`: (h, w, 4) uint8 (R, G, B, E), top row first -- the file's own texel form, what `Image.from_hdr` uploads;
    `exposure`: the product of the header's EXPOSURE= lines (1.0 without one), reported and never applied."""

    def __init__(self, rgbe: np.ndarray, exposure: float = 1.0):
        self.rgbe, self.exposure = rgbe, float(exposure)

    @property
    def width(self) -> int:
        return int(self.rgbe.shape[1])

    @property
    def height(self) -> int:
        return int(self.rgbe.shape[0])

    def to_float(self) -> np.ndarray:
        """(h, w, 4) float32 through mires_hdr_to_float: E = 0 -> (0, 0, 0), else m * 2^(E - 136) (exact); alpha 1."""
        rgbe = np.ascontiguousarray(self.rgbe, dtype=np.uint8)
        img = _MiresHdr(self.width, self.height, self.exposure, 0, rgbe.ctypes.data_as(C.POINTER(C.c_uint8)))
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        l = lib()
        rc = l.mires_hdr_to_float(C.byref(img), out.ctypes.data)
        if rc != 0:
            raise ImageDecodeError(rc, (l.mires_last_error_message() or b"").decode("utf-8", "replace"))
        return out


def _take_hdr(rc: int, img: _MiresHdr) -> HdrImage:
    l = lib()
    if rc != 0:
        raise ImageDecodeError(rc, (l.mires_last_error_message() or b"").decode("utf-8", "replace"))
    try:
        n = img.width * img.height * 4
        arr = np.ctypeslib.as_array(img.rgbe, shape=(n,)).copy().reshape(img.height, img.width, 4)
        return HdrImage(arr, float(img.exposure))
    finally:
        l.mires_hdr_free(C.byref(img))


def decode_hdr(data: bytes) -> HdrImage:
    img = _MiresHdr()
    return _take_hdr(lib().mires_hdr_decode(bytes(data), len(data), C.byref(img)), img)


def load_hdr(path: str) -> HdrImage:
    img = _MiresHdr()
    return _take_hdr(lib().mires_hdr_load(os.fsencode(path), C.byref(img)), img)


def _encode_plane(b: np.ndarray) -> bytes:
    """One component plane of a new-style scanline (the rule is in encode_hdr's docstring)."""
    edges = np.flatnonzero(np.diff(b)) + 1
    starts = np.concatenate(([0], edges))
    lengths = np.diff(np.concatenate((starts, [b.size])))
    out, lit = bytearray(), bytearray()

    def flush():
        for i in range(0, len(lit), 128):
            out.append(min(128, len(lit) - i))
            out.extend(lit[i:i + 128])
        lit.clear()

    for s, n in zip(starts.tolist(), lengths.tolist()):
        v = int(b[s])
        while n >= 3:
            k = min(n, 127)
            flush()
            out.append(128 + k)
            out.append(v)
            n -= k
        lit.extend(bytes([v]) * n)
    flush()
    return bytes(out)


def encode_hdr(rgbe, rle: bool = True) -> bytes:
    """A Radiance file (#?RADIANCE, FORMAT=32-bit_rle_rgbe, -Y h +X w) of the (h, w, 4) uint8 array `rgbe`; decode_hdr gives it back.

    rle=True writes new-style RLE scanlines where the format has them (8 <= w <= 32767; flat pixels otherwise).  Each of a line's four
    component planes is cut into its maximal stretches of one repeated byte, left to right.  A stretch of 3 or more becomes runs: 127 at
    a time while 3 or more remain; what is left of it (0, 1 or 2 bytes) and every shorter stretch are literal bytes.  Literal bytes
    collect until the next run or the plane's end and are written 128 at a time, the last group shorter.
    rle=False writes flat pixels.  For 8 <= w <= 32767 a reader takes such a line for old-style RLE, so a line that holds a pixel
    (1, 1, 1, n), or begins with (2, 2, <128, n), cannot be written flat: ValueError."""
    a = np.ascontiguousarray(rgbe, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"encode_hdr takes an (h, w, 4) uint8 array, got shape {a.shape}")
    h, w = a.shape[:2]
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + f"-Y {h} +X {w}\n".encode()
    if w < 8 or w > 32767:
        return head + a.tobytes()
    if not rle:
        marker = np.all(a[..., :3] == 1, axis=2)
        first = (a[:, 0, 0] == 2) & (a[:, 0, 1] == 2) & (a[:, 0, 2] < 128)
        if marker.any() or first.any():
            raise ValueError("encode_hdr(rle=False): a line holds a pixel a reader would take for an RLE marker; write it with rle=True")
        return head + a.tobytes()
    rows, done = [], {}
    for y in range(h):
        key = a[y].tobytes()
        if key not in done:
            done[key] = bytes([2, 2, w >> 8, w & 255]) + b"".join(_encode_plane(a[y, :, c]) for c in range(4))
        rows.append(done[key])
    return head + b"".join(rows)
