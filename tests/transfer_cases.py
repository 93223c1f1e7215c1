"""Shared by tests/test_transfer_cpu.py and tests/test_gpu_transfer.py: the numpy model of the recorded transfer commands (include/mirhi.h
"Transfer commands") in float64 and in float32 -- the blit's exact index choice, the per-texel decode, the filter, the 8-bit encoding -- the
error measure of DESIGN.md 8d, and the seeded sources the GPU cases use (computed once, left unchanged)."""
import numpy as np

BGRA8_SRGB, RGBA32F, D32, RGBA8_UNORM, R32_UINT, RGBA8_SRGB = 1, 2, 3, 4, 5, 6      # mirhi_format
BLIT_FORMATS = (BGRA8_SRGB, RGBA8_UNORM, RGBA8_SRGB, RGBA32F)
NEAREST, LINEAR = 0, 1
EPS = 4e-6          # "undecided": about ten float32 roundings of 6e-8 each on the blit's path, with a 6x margin
SRC_W, SRC_H = 24, 20
DST_W, DST_H = 37, 29

# the 256-entry table the samplers use: the sRGB EOTF per byte, evaluated in double and rounded to float32 once
_c = np.arange(256, dtype=np.float64) / 255.0
SRGB_LUT = np.where(_c <= 0.04045, _c / 12.92, ((_c + 0.055) / 1.055) ** 2.4).astype(np.float32)
SRGB_LUT.setflags(write=False)


def texel_bytes(fmt):
    return 16 if fmt == RGBA32F else 4


def decode(texels, fmt, dtype=np.float64):
    """Linear RGBA [.., 4] in dtype of stored texels: float32 [.., 4] (R32G32B32A32_SFLOAT) or bytes [.., 4] in the format's byte order."""
    if fmt == RGBA32F:
        return np.asarray(texels, dtype=np.float32).astype(dtype)
    b = np.asarray(texels, dtype=np.uint8)
    if fmt == BGRA8_SRGB:
        b = b[..., [2, 1, 0, 3]]
    alpha = b[..., 3].astype(dtype) / dtype(255.0) if dtype is np.float64 else b[..., 3].astype(np.float32) * np.float32(1.0 / 255.0)
    if fmt == RGBA8_UNORM:
        rgb = b[..., :3].astype(dtype) / dtype(255.0) if dtype is np.float64 else b[..., :3].astype(np.float32) * np.float32(1.0 / 255.0)
    else:
        rgb = SRGB_LUT[b[..., :3]].astype(dtype)
    return np.concatenate([rgb, alpha[..., None]], axis=-1)


def encode(rgba, fmt):
    """Stored texels of linear RGBA: float32 for a float destination (unclamped); bytes in the format's order for an 8-bit one -- saturate, the sRGB
    OETF on RGB of an _SRGB format, round-to-nearest-even of x * 255 -- evaluated in float64 on the values given."""
    if fmt == RGBA32F:
        return np.asarray(rgba, dtype=np.float32)
    c = np.clip(np.asarray(rgba, dtype=np.float64), 0.0, 1.0)
    rgb = c[..., :3]
    if fmt != RGBA8_UNORM:
        rgb = np.clip(np.where(rgb <= 0.0031308, 12.92 * rgb, 1.055 * rgb ** (1.0 / 2.4) - 0.055), 0.0, 1.0)
    out = np.rint(np.concatenate([rgb, c[..., 3:]], axis=-1) * 255.0).astype(np.uint8)
    return out[..., [2, 1, 0, 3]] if fmt == BGRA8_SRGB else out


def undecided(m64, fmt):
    """Channels of an 8-bit destination whose byte the float64 model does not decide: a value EPS below and one EPS above encode differently."""
    lo = encode((m64 * (1.0 - EPS)).astype(np.float32), fmt)
    hi = encode((m64 * (1.0 + EPS)).astype(np.float32), fmt)
    return lo != hi


def axis_taps(d0, d1, s0, s1, n, linear):
    """One axis of a blit region, exact: for the destination texels i = min(d0, d1) .. max(d0, d1) - 1 the source index floor(u) (NEAREST), or floor(u - 1/2),
    that plus one and frac(u - 1/2) as numerator / denominator (LINEAR), u = (i + 1/2 - d0) (s1 - s0) / (d1 - d0) + s0; indices clamped to [0, n - 1]."""
    i = np.arange(min(d0, d1), max(d0, d1), dtype=np.int64)
    sgn, mag = (1, d1 - d0) if d1 > d0 else (-1, d0 - d1)
    num = sgn * (2 * (i - d0) + 1) * (s1 - s0) - (mag if linear else 0)
    den = 2 * mag
    q = num // den                       # (floor division: exact)
    lo = np.clip(s0 + q, 0, n - 1)
    hi = np.clip(s0 + q + 1, 0, n - 1)
    return i, lo, hi, num - q * den, den


def blit(src_linear, src_rect, dst_rect, linear, dtype=np.float64):
    """The destination rectangle [rows, columns, 4] of one blit region, linear RGBA in dtype, rows / columns in ascending destination order.
    src_linear: the decoded source level; rects: ((x0, y0), (x1, y1))."""
    s = np.asarray(src_linear, dtype=dtype)
    h, w = s.shape[:2]
    _, x0, x1, rx, dx = axis_taps(dst_rect[0][0], dst_rect[1][0], src_rect[0][0], src_rect[1][0], w, linear)
    _, y0, y1, ry, dy = axis_taps(dst_rect[0][1], dst_rect[1][1], src_rect[0][1], src_rect[1][1], h, linear)
    if not linear:
        return s[y0[:, None], x0[None, :]]
    fx = (rx.astype(dtype) / dtype(dx))[None, :, None]
    fy = (ry.astype(dtype) / dtype(dy))[:, None, None]
    gx, gy = dtype(1.0) - fx, dtype(1.0) - fy
    t00, t10, t01, t11 = s[y0[:, None], x0[None, :]], s[y0[:, None], x1[None, :]], s[y1[:, None], x0[None, :]], s[y1[:, None], x1[None, :]]
    return ((t00 * gx + t10 * fx) * gy + (t01 * gx + t11 * fx) * fy).astype(dtype)


def rel_err(x, m64):
    """max |X - M64| / max(|M64|, 1e-3 max |M64|)"""
    m64 = np.asarray(m64, dtype=np.float64)
    return float((np.abs(np.asarray(x, dtype=np.float64) - m64) / np.maximum(np.abs(m64), 1e-3 * np.abs(m64).max())).max())


def bound_for(e32):
    return max(8.0 * e32, 1e-4)


def mip_level(level0, level):
    """Level `level` of mirhi_image_generate_mips' chain of bytes [h, w, 4]: 2 x 2 box on the stored bytes, round half up, edge clamp."""
    a = np.asarray(level0, dtype=np.uint32)
    for _ in range(level):
        h, w = a.shape[:2]
        dh, dw = max(1, h >> 1), max(1, w >> 1)
        ys0, ys1 = np.minimum(2 * np.arange(dh), h - 1), np.minimum(2 * np.arange(dh) + 1, h - 1)
        xs0, xs1 = np.minimum(2 * np.arange(dw), w - 1), np.minimum(2 * np.arange(dw) + 1, w - 1)
        a = (a[ys0[:, None], xs0[None, :]] + a[ys0[:, None], xs1[None, :]] + a[ys1[:, None], xs0[None, :]] + a[ys1[:, None], xs1[None, :]] + 2) >> 2
    return a.astype(np.uint8)


_sources = {}


def source(fmt, seed=0, w=SRC_W, h=SRC_H):
    """Seeded random texels of a w x h image of `fmt`: float32 [h, w, 4] in [0, 2) for the float format (values above 1 included; of one sign, so that the error
    measure sees the filter's rounding and not a cancellation), random bytes otherwise.  Computed once per key and left unchanged."""
    key = (fmt, seed, w, h)
    if key not in _sources:
        rng = np.random.default_rng(1000 * seed + fmt)
        a = (rng.random((h, w, 4)) * 2.0).astype(np.float32) if fmt == RGBA32F else rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        a.setflags(write=False)
        _sources[key] = a
    return _sources[key]


def np_dtype(fmt):
    return np.float32 if fmt in (RGBA32F, D32) else (np.uint32 if fmt == R32_UINT else np.uint8)


def raw_texels(fmt, w, h, seed=0):
    """Random texels of ANY format as the array Image.upload takes and Image.read gives back ([h, w, 4] bytes or floats, [h, w] for D32 / R32_UINT)."""
    rng = np.random.default_rng(77 * seed + fmt + 13 * w)
    if fmt == RGBA32F:
        return rng.random((h, w, 4)).astype(np.float32)
    if fmt == D32:
        return rng.random((h, w)).astype(np.float32)
    if fmt == R32_UINT:
        return rng.integers(0, 2 ** 32, (h, w), dtype=np.uint32)
    return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


def as_bytes(a):
    """The stored bytes of a texel array, [h, w * texel size]."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1)
