"""Shared by test_hdr_cpu.py and test_gpu_hdr.py: Radiance .hdr inputs with their expected texels, and the conditions on them that
are checked on the CPU.

The value of a texel (R, G, B, E) is (0, 0, 0) for E = 0 and m * 2^(E - 136) per channel otherwise, alpha 1: exact in binary32 for
every (m, E), so every comparison of decoded values is bit for bit (`decode_float` below is the numpy statement of it).

A mistake in the plan of these cases, kept visible: an 8-wide component plane holds 8 bytes, so the run of 127, the run of 1 and the
literal of 128 that one plane was to hold need a 256-wide line.  FILE_8X2 therefore carries what fits (a run, a run of 1 and literals
in one plane; it is also the file whose every proper prefix must be refused), and FILE_256X1 carries exactly the planned plane."""
import functools

import numpy as np


def ibl():
    import __graft_entry__ as ge
    return ge.load_package().ibl


def decode_float(rgbe) -> np.ndarray:
    """(h, w, 4) float32 of (h, w, 4) uint8 RGBE by the definition: np.ldexp(m, E - 136), E = 0 rows zero, alpha 1."""
    rgbe = np.asarray(rgbe, dtype=np.uint8)
    e = rgbe[..., 3].astype(np.int32)
    out = np.ones(rgbe.shape, dtype=np.float32)
    out[..., :3] = np.ldexp(rgbe[..., :3].astype(np.float32), (e - 136)[..., None])
    out[..., :3][e == 0] = 0.0
    return out


def rgbe_from_float(rgb) -> np.ndarray:
    """The test's own encoder: frexp of the largest channel, mantissas truncated, negatives clamped to 0.  (..., 3 or 4) -> (..., 4) uint8."""
    rgb = np.maximum(np.asarray(rgb, dtype=np.float64)[..., :3], 0.0)
    v = np.max(rgb, axis=-1)
    _, ex = np.frexp(v)                                 # v = m * 2^ex, m in [0.5, 1)
    out = np.zeros(rgb.shape[:-1] + (4,), dtype=np.uint8)
    live = v >= 1e-32
    scale = np.ldexp(256.0, -ex)                        # m * 256 / v
    out[..., :3] = np.where(live[..., None], np.floor(rgb * scale[..., None]), 0.0).astype(np.uint8)
    out[..., 3] = np.where(live, ex + 128, 0).astype(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def all_pairs() -> np.ndarray:
    """256 x 256 RGBE: E = row, R = column, G = 255 - column, B = (7 * column) & 255: every (m, E) pair occurs."""
    col = np.arange(256, dtype=np.uint32)
    img = np.empty((256, 256, 4), dtype=np.uint8)
    img[..., 0] = col[None, :]
    img[..., 1] = 255 - col[None, :]
    img[..., 2] = (7 * col[None, :]) & 255
    img[..., 3] = col[:, None]
    pairs = {(int(m), int(e)) for c in range(3) for m, e in zip(img[..., c].ravel(), img[..., 3].ravel())}
    assert len(pairs) == 65536
    img.setflags(write=False)
    return img


EQUIRECT_EXTENT = (256, 128)                    # width, height


@functools.lru_cache(maxsize=None)
def equirect_rgbe() -> np.ndarray:
    """rgbe_from_float(max(analytic_equirect(256, 128), 0)); checked here: every decoded value finite, at least 99 % of the texels non-zero
    (a comparison against the model cannot pass on a black image), exponents in a moderate range."""
    w, h = EQUIRECT_EXTENT
    img = rgbe_from_float(np.maximum(ibl().analytic_equirect(w, h), 0.0))
    f = decode_float(img)
    assert np.all(np.isfinite(f))
    assert np.count_nonzero(np.any(f[..., :3] != 0.0, axis=-1)) >= 0.99 * w * h
    e = img[..., 3][img[..., 3] != 0]
    assert 96 <= int(e.min()) and int(e.max()) <= 160
    img.setflags(write=False)
    return img


def random_rgbe(w: int, h: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 4), dtype=np.uint8)


# ---- hand-written files --------------------------------------------------------------------------------------------------------------
HEAD = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"


def _px(*rows):
    return np.array(rows, dtype=np.uint8)


# 1 x 1, flat (W < 8): the texel (128, 64, 32, 129) = (128, 64, 32) * 2^-7 = (1.0, 0.5, 0.25)
FILE_1X1 = HEAD + b"-Y 1 +X 1\n" + bytes([128, 64, 32, 129])
WANT_1X1 = _px([[128, 64, 32, 129]])
WANT_1X1_FLOAT = np.array([[[1.0, 0.5, 0.25, 1.0]]], dtype=np.float32)

# 8 x 2, new-style RLE: each line is (2, 2, 0, 8) and then the planes R, G, B, E of 8 bytes each
FILE_8X2 = HEAD + b"-Y 2 +X 8\n" + bytes(
    [2, 2, 0, 8,
     133, 10, 129, 20, 2, 30, 31,               # R: run of 5 x 10, run of 1 x 20, literal (30, 31)      -> 10 10 10 10 10 20 30 31
     8, 1, 2, 3, 4, 5, 6, 7, 8,                 # G: literal of 8                                        -> 1 2 3 4 5 6 7 8
     136, 7,                                    # B: run of 8 x 7                                        -> 7 x 8
     136, 128,                                  # E: run of 8 x 128                                      -> 128 x 8
     2, 2, 0, 8,
     3, 9, 8, 7, 133, 0,                        # R: literal (9, 8, 7), run of 5 x 0                     -> 9 8 7 0 0 0 0 0
     132, 255, 132, 1,                          # G: run of 4 x 255, run of 4 x 1                        -> 255 x 4, 1 x 4
     8, 0, 1, 1, 1, 2, 2, 0, 128,               # B: literal of 8 (markers of the old style are bytes here) -> 0 1 1 1 2 2 0 128
     1, 0, 135, 130])                           # E: literal (0), run of 7 x 130                         -> 0 130 x 7
WANT_8X2 = np.stack([
    np.stack([_px(10, 10, 10, 10, 10, 20, 30, 31), _px(1, 2, 3, 4, 5, 6, 7, 8), _px(*[7] * 8), _px(*[128] * 8)], axis=-1),
    np.stack([_px(9, 8, 7, 0, 0, 0, 0, 0), _px(255, 255, 255, 255, 1, 1, 1, 1), _px(0, 1, 1, 1, 2, 2, 0, 128), _px(0, *[130] * 7)], axis=-1)])

# 256 x 1, new-style RLE, the R plane = a run of 127, then a run of 1, then a literal of 128 (the longest run, the shortest, the longest literal)
FILE_256X1 = HEAD + b"-Y 1 +X 256\n" + bytes(
    [2, 2, 1, 0,
     255, 200, 129, 201, 128, *range(128),      # R: 127 x 200, 1 x 201, then 0 .. 127
     255, 1, 255, 2, 130, 3,                    # G: 127 x 1, 127 x 2, 2 x 3
     128, *range(128, 256), 128, *range(128),   # B: two literals of 128: 128 .. 255, 0 .. 127
     255, 128, 255, 128, 130, 128])             # E: 256 x 128 as runs of 127, 127 and 2
WANT_256X1 = np.stack([_px(*[200] * 127, 201, *range(128)), _px(*[1] * 127, *[2] * 127, 3, 3), _px(*range(128, 256), *range(128)),
                       _px(*[128] * 256)], axis=-1)[None]

# 9 x 1, old-style RLE (the first pixel is not (2, 2, <128, n)): A, repeat 2 << 0, repeat 0 << 8 (a second consecutive marker: shift 8),
# B (shift back to 0), repeat 3 << 0, C, D  ->  A A A B B B B C D
_A, _B, _C, _D = (50, 60, 70, 128), (1, 2, 3, 130), (2, 2, 200, 9), (255, 255, 255, 255)
FILE_9X1_OLD = HEAD + b"-Y 1 +X 9\n" + bytes([*_A, 1, 1, 1, 2, 1, 1, 1, 0, *_B, 1, 1, 1, 3, *_C, *_D])
WANT_9X1_OLD = _px([_A, _A, _A, _B, _B, _B, _B, _C, _D])

# 601 x 1, old-style RLE where the shift counts: A, repeat 88 << 0, repeat 2 << 8 = 512  ->  601 x A
FILE_601X1_OLD = HEAD + b"-Y 1 +X 601\n" + bytes([*_A, 1, 1, 1, 88, 1, 1, 1, 2])
WANT_601X1_OLD = _px([_A] * 601)

# the other signature, no FORMAT line, two EXPOSURE lines (the product is reported: 2.0 * 0.25 = 0.5), an unknown line that is ignored
FILE_RGBE_SIGNATURE = b"#?RGBE\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 1\n" + bytes([128, 64, 32, 129])
FILE_NO_FORMAT = b"#?RADIANCE\nSOFTWARE=none\n\n-Y 1 +X 2\n" + bytes([1, 2, 3, 4, 5, 6, 7, 8])
WANT_NO_FORMAT = _px([[1, 2, 3, 4], [5, 6, 7, 8]])
FILE_TWO_EXPOSURES = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=2.0\n# a comment\nEXPOSURE=0.25\n\n-Y 1 +X 1\n" + bytes([128, 64, 32, 129])

# (name, file, expected rgbe, expected exposure)
GOOD_FILES = (
    ("1x1 flat", FILE_1X1, WANT_1X1, 1.0),
    ("8x2 new RLE", FILE_8X2, WANT_8X2, 1.0),
    ("256x1 new RLE: run 127, run 1, literal 128", FILE_256X1, WANT_256X1, 1.0),
    ("9x1 old RLE, consecutive markers", FILE_9X1_OLD, WANT_9X1_OLD, 1.0),
    ("601x1 old RLE, shift 8", FILE_601X1_OLD, WANT_601X1_OLD, 1.0),
    ("#?RGBE", FILE_RGBE_SIGNATURE, WANT_1X1, 1.0),
    ("no FORMAT line", FILE_NO_FORMAT, WANT_NO_FORMAT, 1.0),
    ("two EXPOSURE lines", FILE_TWO_EXPOSURES, WANT_1X1, 0.5),
    ("bytes behind the last scanline", FILE_1X1 + b"trailing", WANT_1X1, 1.0),
)

_LINE8 = bytes([2, 2, 0, 8])
_REST8 = bytes([136, 1, 136, 2, 136, 3])        # three whole planes
# (name, file, a piece of the message that names the cause)
BAD_FILES = (
    ("bad signature", b"#?RADIANCF\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 1\n" + bytes(4), "signature"),
    ("no signature at all", b"", "signature"),
    ("XYZE", b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n-Y 1 +X 1\n" + bytes(4), "32-bit_rle_xyze"),
    ("+Y 2 +X 8", HEAD + b"+Y 2 +X 8\n" + bytes(64), "orientation '+Y 2 +X 8'"),
    ("-Y 2 -X 8", HEAD + b"-Y 2 -X 8\n" + bytes(64), "orientation '-Y 2 -X 8'"),
    ("+X 8 -Y 2", HEAD + b"+X 8 -Y 2\n" + bytes(64), "orientation '+X 8 -Y 2'"),
    ("missing resolution line: the data ends", HEAD, "resolution line"),
    ("missing resolution line: scanlines follow the header", HEAD + FILE_8X2[len(HEAD) + len(b"-Y 2 +X 8\n"):], "resolution line"),
    ("the data ends inside the header", b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n", "resolution line"),
    ("W = 0", HEAD + b"-Y 2 +X 0\n" + bytes(64), "width 0"),
    ("H = 0", HEAD + b"-Y 0 +X 2\n" + bytes(64), "height 0"),
    ("W = 65537", HEAD + b"-Y 1 +X 65537\n" + bytes(64), "width 65537"),
    ("W * H > 2^28 in front of a short body", HEAD + b"-Y 16385 +X 16384\n" + bytes(100), "2^28"),
    ("W * H = 2^28 in front of a short body", HEAD + b"-Y 16384 +X 16384\n" + bytes([7] * 100), "truncated"),
    ("run count 0", HEAD + b"-Y 1 +X 8\n" + _LINE8 + bytes([4, 1, 2, 3, 4, 0, 9]) + _REST8, "count 0"),
    ("a run past the plane's end", HEAD + b"-Y 1 +X 8\n" + _LINE8 + bytes([4, 1, 2, 3, 4, 133, 9]) + _REST8, "run passes the end"),
    ("a literal past the plane's end", HEAD + b"-Y 1 +X 8\n" + _LINE8 + bytes([132, 9, 5, 1, 2, 3, 4, 5]) + _REST8, "literal passes the end"),
    ("a scanline header whose length is not W", HEAD + b"-Y 1 +X 8\n" + bytes([2, 2, 0, 9, 137, 1, 137, 2, 137, 3, 137, 4]), "declares length 9"),
    ("an old-style repeat as the first pixel", HEAD + b"-Y 1 +X 9\n" + bytes([1, 1, 1, 2, *_A * 7]), "no pixel before"),
    ("an old-style repeat past the line's end", HEAD + b"-Y 1 +X 9\n" + bytes([*_A, 1, 1, 1, 9]), "repeat passes the end"),
    ("an old-style repeat past the line's end through its shift", HEAD + b"-Y 1 +X 9\n" + bytes([*_A, 1, 1, 1, 2, 1, 1, 1, 1, *_B * 6]), "repeat passes the end"),
    ("truncated flat data", HEAD + b"-Y 2 +X 2\n" + bytes(15), "truncated"),
)

ROUND_TRIP_WIDTHS = (1, 7, 8, 9, 127, 128, 129, 255, 32767, 32768)      # height 1 for the last two


def round_trip_images():
    """(name, rgbe) for decode_hdr(encode_hdr(x)) == x: random texels at every width, and rows of one repeated texel, rows with no repeats
    (no two neighbouring bytes of a plane equal) and rows that alternate between runs of 2 and 3."""
    out = []
    for i, w in enumerate(ROUND_TRIP_WIDTHS):
        h = 1 if w > 255 else 3
        out.append((f"random {w}x{h}", random_rgbe(w, h, 100 + i)))
    for w in (8, 129, 255):
        rng = np.random.default_rng(w)
        one = np.broadcast_to(rng.integers(0, 256, size=(2, 1, 4), dtype=np.uint8), (2, w, 4)).copy()
        out.append((f"one repeated texel {w}x2", one))
        step = np.arange(w, dtype=np.uint32)
        none = np.stack([(step * k + o) & 255 for k, o in ((1, 0), (3, 7), (5, 100), (7, 128))], axis=-1).astype(np.uint8)[None]
        assert np.all(np.diff(none.astype(np.int32), axis=1) != 0)
        out.append((f"no repeats {w}x1", none))
        lengths = np.tile([2, 3], w)[:w]
        runs = np.repeat(np.arange(w, dtype=np.uint32), lengths)[:w]         # 0 0 1 1 1 2 2 3 3 3 ...
        alt = np.stack([(runs * k + o) & 255 for k, o in ((1, 0), (3, 7), (5, 100), (7, 128))], axis=-1).astype(np.uint8)[None]
        out.append((f"runs of 2 and 3 {w}x1", alt))
    return out
