"""An exact integer model of the geometry kernel's routing decisions, and the cases that sit on their boundaries.

Plain Python and numpy, integers only (fractions.Fraction in the clipper); no GPU call.  A triangle is given in integer 1/256-pixel
coordinates X, Y and drawn with the TRIANGLE program (w = 1) on a target whose width and height are powers of two: the clip coordinate
X / (128 W) - 1 is then exact in binary32 and so is the viewport transform back (round_trip checks that for every case, and refuses one that
does not come back).

The rules, with the lines of renderer-rs_amd/csrc they mirror:
  setup      mirhi_geometry.hip.h:85-91   signed area S, S == 0 rejects, cull mode
             mirhi_geometry.hip.h:92-96   orientation normalised (S < 0: vertices 1 and 2 swapped)
             mirhi_geometry.hip.h:123-131 pixel box: (min + 127) >> 8 .. (max - 128) >> 8, `cut` by a partial scissor, clamp, empty box rejects
             mirhi_geometry.hip.h:56-62   owned_rows (tile_row_begin / _end / _step); :133-137 no owned row rejects
             mirhi_geometry.hip.h:141     compact: not cut and both extents <= 65535
  route      mirhi_geometry.hip.h:407-416 tx0, ntx, nty (owned rows only), fits, spill (MAX_BIN_SPAN = 4, mirhi_device.h:25)
             mirhi_geometry.hip.h:382-387 store_bin_rec: the record relative to its tile, 16 bits (what `fits` promises)
  coverage   mirhi_raster.hip.h:61-72     tile_edge: A, B, top-left tie bias, Q = floor((E + bias) / 256) at the tile origin's pixel centre
             mirhi_raster.hip.h:150-158   tile_tri_from_bin: the box recomputed from the vertices, relative to the tile; :47-52 clamp_box
             mirhi_raster.hip.h:161-171   tile_tri_from_big: the record's (scissor-clamped) box against the tile
             mirhi_stats.hip.h:15-35      count_tile_tri: a pixel counts when all three Q + A ix + B iy are >= 0
  clipping   mirhi_geometry.hip.h:152-171 planes and outcodes; :188-217 Sutherland-Hodgman in plane order, a fan from vertex 0, every piece to the big list
             mirhi_api.hip:2316-2332      the draw's hw, hh, cx, cy, gx, gy (GUARD_PX = 16000)
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from fractions import Fraction
from typing import Dict, List, Optional, Tuple

import numpy as np

TILE = 32
TILE_LOG2 = 5
TW = TILE * 256                 # a tile in 1/256 px
MAX_BIN_SPAN = 4                # mirhi_device.h:25
GUARD_PX = 16000.0
NO_PRIM = 0xFFFFFFFF
f32 = np.float32


@dataclass(frozen=True)
class Tri:
    X: Tuple[int, int, int]
    Y: Tuple[int, int, int]
    z: float = 0.5              # the same depth at the three vertices: the depth plane is z exactly (zx = zy = 0)

    def transposed(self) -> "Tri":
        return Tri(self.Y, self.X, self.z)


@dataclass(frozen=True)
class Split:
    """PassParams::tile_row_begin, tile_row_step and the number of owned rows (tile_row_end = first + count)."""
    first: int
    step: int
    count: int

    def rows(self) -> List[int]:
        return [self.first + k * max(self.step, 1) for k in range(self.count)]


@dataclass(frozen=True)
class Rules:
    """The model's rules; the defaults are the kernel's.  The other values are the planted errors tests/test_binning_cpu.py must catch."""
    lo: int = 127               # mirhi_geometry.hip.h:126
    tie_bias: bool = True       # mirhi_raster.hip.h:65-67
    ntx_unclamped: bool = False  # mirhi_geometry.hip.h:407-409 take the span from the clamped box


KERNEL = Rules()


@dataclass
class Case:
    name: str
    tris: List[Tri]
    width: int = 256
    height: int = 256
    scissor: Optional[Tuple[int, int, int, int]] = None     # (x, y, w, h)
    expect: Dict[str, object] = field(default_factory=dict)   # the condition the case was built for, on the facts of triangle 0
    boundary: str = ""          # "on" / "in" / "out": where the case sits against its boundary ("" = no boundary variant)
    clipped: bool = False       # the named clipped cases: vertices are clip coordinates (x, y, z) in `clip`, not X / Y
    clip: Optional[List[Tuple[Fraction, Fraction, Fraction]]] = None
    pad: int = 0                # zero-area triangles in the scene (rejected at S == 0), around the real ones
    env: Dict[str, str] = field(default_factory=dict)
    pages: Optional[int] = None  # DeviceStats::last_bin_pages the case must report
    model: bool = False         # drawn with the MODEL program under identity matrices (a mesh-program scope: the per-XCD lists), w = 1 all the same

    def full_split(self) -> Split:
        return Split(0, 1, (self.height + TILE - 1) // TILE)


# ------------------------------------------------------------------------------------------------
# exact inputs
# ------------------------------------------------------------------------------------------------
def clip_xy(X: int, Y: int, width: int, height: int):
    """The binary32 clip coordinates that snap back to (X, Y)."""
    return f32(f32(X) / f32(128 * width) - f32(1.0)), f32(f32(Y) / f32(128 * height) - f32(1.0))


def draw_constants(width: int, height: int):
    """record_draw (mirhi_api.hip:2316-2332) for the full-extent viewport: hw, hh, cx, cy, gx, gy in binary32."""
    hw, hh = f32(0.5) * f32(width), f32(0.5) * f32(height)
    cx, cy = f32(0.0) + hw, f32(0.0) + hh
    gx, gy = (f32(GUARD_PX) - abs(cx)) / hw, (f32(GUARD_PX) - abs(cy)) / hh
    return hw, hh, cx, cy, f32(gx), f32(gy)


def round_trip(t: Tri, width: int, height: int) -> bool:
    """setup_triangle's window transform and snap (mirhi_geometry.hip.h:75-82) of the case's clip coordinates, in binary32, give X, Y again; every
    vertex has w = 1 > 0, lies inside the guard band (outcode_clip, :163-172, with the draw's own gx, gy), inside |xs| <= 16383 and in 0 <= z <= 1."""
    hw, hh, cx, cy, gx, gy = draw_constants(width, height)
    w = f32(1.0)
    for X, Y in zip(t.X, t.Y):
        x, y = clip_xy(X, Y, width, height)
        z = f32(t.z)
        if z < 0 or w - z < 0 or x + gx * w < 0 or gx * w - x < 0 or y + gy * w < 0 or gy * w - y < 0:
            return False
        iw = f32(1.0) / w
        xs, ys = f32(f32(x * iw) * hw) + cx, f32(f32(y * iw) * hh) + cy
        if not (abs(xs) <= f32(16383.0)) or not (abs(ys) <= f32(16383.0)):
            return False
        if int(np.rint(f32(xs * f32(256.0)))) != X or int(np.rint(f32(ys * f32(256.0)))) != Y:
            return False
        # and the exact value agrees with the binary32 one
        if Fraction(float(x)) != Fraction(X, 128 * width) - 1 or Fraction(float(y)) != Fraction(Y, 128 * height) - 1:
            return False
    return True


def vertices(c: Case) -> np.ndarray:
    """The case's vertex buffer: 24-byte TRIANGLE vertices (position, colour), the zero-area padding around the real triangles (half of them in
    front: the first waves; the rest behind: the last)."""
    if c.clipped:
        rows = [[float(x), float(y), float(z)] for (x, y, z) in c.clip]
        n_real = len(rows) // 3
    else:
        rows = []
        for t in c.tris:
            if not round_trip(t, c.width, c.height):
                raise ValueError(f"{c.name}: {t} does not round-trip")
            for X, Y in zip(t.X, t.Y):
                x, y = clip_xy(X, Y, c.width, c.height)
                rows.append([x, y, f32(t.z)])
        n_real = len(c.tris)
    head = n_real - n_real // 2
    pos = np.asarray(rows, dtype=f32).reshape(-1, 3)
    if c.pad:
        # a zero-area triangle: three times the same point inside the target
        p = np.tile(np.array([[0.25, 0.25, 0.5]], dtype=f32), (3 * c.pad, 1))
        pos = np.concatenate([pos[:3 * head], p, pos[3 * head:]], axis=0)
    col = np.empty_like(pos)
    k = np.arange(pos.shape[0]) // 3
    col[:, 0] = ((k * 37) % 101 + 20) / 128.0
    col[:, 1] = ((k * 53) % 89 + 20) / 128.0
    col[:, 2] = ((k * 71) % 97 + 20) / 128.0
    return np.concatenate([pos, col.astype(f32)], axis=1)


def scene_of(c: Case, scenes, only: Optional[int] = None):
    """A scenes.Scene of the case (only: triangle `only` alone, without padding)."""
    if only is not None:
        one = replace(c, pad=0, tris=[c.tris[only]]) if not c.clipped else replace(c, pad=0, clip=c.clip[3 * only:3 * only + 3])
        v = vertices(one)
    else:
        v = vertices(c)
    if c.model:
        # 48-byte MODEL vertices; model, view and projection the identity: every product of the two matrix multiplications is the coordinate or a zero
        n = v.shape[0]
        eye = np.eye(4, dtype=f32)
        v48 = np.zeros((n, 12), dtype=f32)
        v48[:, 0:3] = v[:, 0:3]
        v48[:, 5] = 1.0
        v48[:, 8] = 1.0
        v48[:, 11] = 1.0
        d = scenes.DrawSpec(vertices=v48, stride=48, count=n, program=scenes.PROGRAM_MODEL, cull_mode=scenes.CULL_NONE, scissor=c.scissor,
                            camera=scenes.camera_ubo(eye, eye, (0.0, 0.0, 1.0)), object=scenes.object_ubo(eye),
                            light=scenes.light_ubo(direction=(0.0, 0.0, -1.0), intensity=1.0), material=scenes.material_ubo((0.7, 0.7, 0.7, 1.0), 0.0, 0.5, 1.0),
                            albedo_map=scenes.WHITE_1X1, normal_map=scenes.WHITE_1X1)
        return scenes.Scene(c.name, c.width, c.height, [d])
    d = scenes.DrawSpec(vertices=v, stride=24, count=v.shape[0], cull_mode=scenes.CULL_NONE, scissor=c.scissor)
    return scenes.Scene(c.name, c.width, c.height, [d])


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
def owned_rows(s: Split, ty0: int, ty1: int):
    """mirhi_geometry.hip.h:56-62."""
    a, b = ty0 - s.first, ty1 - s.first
    if s.step <= 1:
        return max(a, 0), min(b, s.count - 1)
    k0 = 0 if a <= 0 else (a + s.step - 1) // s.step
    k1 = -1 if b < 0 else min(b // s.step, s.count - 1)
    return k0, k1


@dataclass
class Routed:
    route: str                                  # "rejected" / "binned" / "big"
    why: str = ""
    X: Tuple[int, ...] = ()
    Y: Tuple[int, ...] = ()
    box: Tuple[int, int, int, int] = (0, -1, 0, -1)     # px0, px1, py0, py1 (clamped, inclusive)
    cut: bool = False
    compact: bool = False
    pairs: List[Tuple[int, int]] = field(default_factory=list)      # binned: (tile column, tile row); big: the owned tiles its box touches
    tile_sums: List[int] = field(default_factory=list)              # covered pixel centres per pair
    covered: Optional[np.ndarray] = None                            # (height, width) bool
    facts: Dict[str, object] = field(default_factory=dict)

    @property
    def frags(self) -> int:
        return int(sum(self.tile_sums))


def setup(X, Y, width, height, scissor, split: Split, rules: Rules = KERNEL, cull_mode: int = 0):
    """setup_triangle, mirhi_geometry.hip.h:85-141 (cull NONE: every case draws with it).  None: rejected (with the reason), else the facts."""
    X, Y = list(X), list(Y)
    S = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])       # :85
    if S == 0:
        return None, "S == 0"                                               # :87
    if S < 0:                                                               # :92-96
        X[1], X[2] = X[2], X[1]
        Y[1], Y[2] = Y[2], Y[1]
    xmin, xmax, ymin, ymax = min(X), max(X), min(Y), max(Y)
    px0u, px1u = (xmin + rules.lo) >> 8, (xmax - 128) >> 8                  # :127
    py0u, py1u = (ymin + rules.lo) >> 8, (ymax - 128) >> 8                  # :128
    if scissor is None:
        sx0, sy0, sx1, sy1, partial = 0, 0, width - 1, height - 1, False
    else:
        sx0, sy0 = max(scissor[0], 0), max(scissor[1], 0)
        sx1, sy1 = min(scissor[0] + scissor[2], width) - 1, min(scissor[1] + scissor[3], height) - 1
        partial = sx0 > 0 or sy0 > 0 or sx1 < width - 1 or sy1 < height - 1      # mirhi_api.hip:2336
    cut = partial and (px0u < sx0 or px1u > sx1 or py0u < sy0 or py1u > sy1)    # :129
    px0, px1, py0, py1 = max(px0u, sx0), min(px1u, sx1), max(py0u, sy0), min(py1u, sy1)     # :130
    if px0 > px1 or py0 > py1:
        return None, "empty box"                                            # :131
    k0, k1 = owned_rows(split, py0 >> TILE_LOG2, py1 >> TILE_LOG2)          # :135
    if k1 < k0:
        return None, "no owned row"                                         # :136
    compact = (not cut) and xmax - xmin <= 65535 and ymax - ymin <= 65535   # :141
    return dict(X=tuple(X), Y=tuple(Y), S=S, box=(px0, px1, py0, py1), ubox=(px0u, px1u, py0u, py1u), cut=cut, compact=compact,
                vminx=xmin, vminy=ymin, xmax=xmax, ymax=ymax, k0=k0, k1=k1), ""


def _edges(X, Y, ox, oy, rules: Rules):
    """tile_edge (mirhi_raster.hip.h:61-72) of the three edges, the tile's origin at (ox, oy) 1/256 px: (A, B, Q)."""
    out = []
    for i in range(3):
        xa, ya, xb, yb = X[i] - ox, Y[i] - oy, X[(i + 1) % 3] - ox, Y[(i + 1) % 3] - oy
        dx, dy = xb - xa, yb - ya
        A, B = -dy, dx
        topleft = dy < 0 or (dy == 0 and dx > 0)
        bias = 0 if (topleft or not rules.tie_bias) else -1
        q = (A * (128 - xa) + B * (128 - ya) + bias) >> 8
        q = min(max(q, -(1 << 30)), 1 << 30)
        out.append((A, B, q))
    return out


def _clamp_box(bx0, bx1, by0, by1):
    """clamp_box, mirhi_raster.hip.h:47-52."""
    bx0, by0 = min(max(bx0, 0), TILE), min(max(by0, 0), TILE)
    bx1, by1 = max(min(bx1, TILE - 1), -1), max(min(by1, TILE - 1), -1)
    return bx0, bx1, by0, by1


def tile_cover(s, col, row, width, height, binned: bool, rules: Rules = KERNEL) -> np.ndarray:
    """The pixel centres of tile (col, row) the statistics pass counts for the record (count_tile_tri), as a TILE x TILE bool array [iy, ix]."""
    ox, oy = col * TW, row * TW
    X, Y = s["X"], s["Y"]
    if binned:
        # the 16-bit record (store_bin_rec) and its decode: the smallest coordinates relative to the tile must fit int16, the others uint16 above them
        rx, ry = s["vminx"] - ox, s["vminy"] - oy
        assert -32768 <= rx <= 32767 and -32768 <= ry <= 32767, "fits promised a 16-bit origin"
        assert all(0 <= x - s["vminx"] <= 65535 for x in X) and all(0 <= y - s["vminy"] <= 65535 for y in Y)
        bx0, bx1 = (rx + rules.lo) >> 8, (s["xmax"] - ox - 128) >> 8        # tile_tri_from_bin, mirhi_raster.hip.h:156
        by0, by1 = (ry + rules.lo) >> 8, (s["ymax"] - oy - 128) >> 8
    else:
        px0, px1, py0, py1 = s["box"]                                       # tile_tri_from_big, mirhi_raster.hip.h:163-165
        bx0, bx1, by0, by1 = px0 - col * TILE, px1 - col * TILE, py0 - row * TILE, py1 - row * TILE
    out = np.zeros((TILE, TILE), dtype=bool)
    if not binned and (bx1 < 0 or bx0 > TILE - 1 or by1 < 0 or by0 > TILE - 1):
        return out
    bx0, bx1, by0, by1 = _clamp_box(bx0, bx1, by0, by1)
    bx1, by1 = min(bx1, width - 1 - col * TILE), min(by1, height - 1 - row * TILE)      # lim_x, lim_y (mirhi_stats.hip.h:47)
    if bx0 > bx1 or by0 > by1:
        return out
    ix = np.arange(TILE, dtype=np.int64)[None, :]
    iy = np.arange(TILE, dtype=np.int64)[:, None]
    ok = (ix >= bx0) & (ix <= bx1) & (iy >= by0) & (iy <= by1)
    for A, B, q in _edges(X, Y, ox, oy, rules):
        ok &= (q + A * ix + B * iy) >= 0
    return ok


def route(t: Tri, width: int, height: int, scissor=None, split: Optional[Split] = None, rules: Rules = KERNEL, force_big: bool = False) -> Routed:
    """The head of bin_triangle_pairs (mirhi_geometry.hip.h:403-419) behind setup_triangle, and the coverage the statistics pass counts.
    force_big: a clipper's piece (emit_big, :215)."""
    split = split or Split(0, 1, (height + TILE - 1) // TILE)
    s, why = setup(t.X, t.Y, width, height, scissor, split, rules)
    if s is None:
        return Routed("rejected", why, covered=np.zeros((height, width), dtype=bool), facts={"route": "rejected", "why": why})
    px0, px1, py0, py1 = s["box"]
    step = max(split.step, 1)
    tx0 = px0 >> TILE_LOG2                                                  # :407
    k0, k1 = s["k0"], s["k1"]                                               # :408
    ntx = (px1 >> TILE_LOG2) - tx0 + 1                                      # :409
    if rules.ntx_unclamped:
        ntx = (s["ubox"][1] >> TILE_LOG2) - (s["ubox"][0] >> TILE_LOG2) + 1
    nty = k1 - k0 + 1                                                       # :410
    row_lo, row_hi = split.first + k0 * step, split.first + k1 * step
    m = dict(hi_x=32767 - (s["vminx"] - tx0 * TW), lo_x=s["vminx"] - (tx0 + ntx - 1) * TW + 32768,
             hi_y=32767 - (s["vminy"] - row_lo * TW), lo_y=s["vminy"] - row_hi * TW + 32768)         # the four margins of `fits`, >= 0: inside (:414-415)
    fits = s["compact"] and min(m.values()) >= 0
    spill = ntx > MAX_BIN_SPAN or nty > MAX_BIN_SPAN or not fits or force_big   # :416
    r = Routed("big" if spill else "binned", X=s["X"], Y=s["Y"], box=s["box"], cut=s["cut"], compact=s["compact"])
    if spill:
        # the big list is walked by every owned tile; the record's box decides (tile_tri_from_big)
        r.pairs = [(c, row) for row in split.rows() for c in range(px0 >> TILE_LOG2, (px1 >> TILE_LOG2) + 1)
                   if (py0 >> TILE_LOG2) <= row <= (py1 >> TILE_LOG2)]
    else:
        r.pairs = [(tx0 + i, split.first + (k0 + j) * step) for j in range(nty) for i in range(ntx)]
    r.covered = np.zeros((height, width), dtype=bool)
    for c, row in r.pairs:
        tc = tile_cover(s, c, row, width, height, not spill, rules)
        r.tile_sums.append(int(tc.sum()))
        h, w = min(TILE, height - row * TILE), min(TILE, width - c * TILE)
        if h > 0 and w > 0:
            r.covered[row * TILE:row * TILE + h, c * TILE:c * TILE + w] |= tc[:h, :w]
    last_c, first_c = tx0 + ntx - 1, tx0
    r.facts = dict(route=r.route, ntx=ntx, nty=nty, nb=0 if spill else ntx * nty, cut=s["cut"], compact=s["compact"], fits=bool(fits),
                   extent_x=s["xmax"] - s["vminx"], extent_y=s["ymax"] - s["vminy"], margin_lo_x=m["lo_x"], margin_lo_y=m["lo_y"],
                   margin_hi_x=m["hi_x"], margin_hi_y=m["hi_y"], rows_spanned=(py1 >> TILE_LOG2) - (py0 >> TILE_LOG2) + 1,
                   # the tile-relative box values tile_tri_from_bin computes, seen from the first and the last tile of the span
                   box_hi_x_first=(s["xmax"] - first_c * TW - 128) >> 8, box_hi_x_last=(s["xmax"] - last_c * TW - 128) >> 8,
                   box_hi_y_first=(s["ymax"] - row_lo * TW - 128) >> 8, box_hi_y_last=(s["ymax"] - row_hi * TW - 128) >> 8,
                   box_lo_x_last=(s["vminx"] - last_c * TW + 127) >> 8, box_lo_y_last=(s["vminy"] - row_hi * TW + 127) >> 8,
                   box=s["box"], boxed=s["cut"])
    return r


# ------------------------------------------------------------------------------------------------
# the clipper on exact rationals (mirhi_geometry.hip.h:152-217)
# ------------------------------------------------------------------------------------------------
def _round_half_even(q: Fraction) -> int:
    f = q.numerator // q.denominator
    r = q - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2 == 1):
        return f + 1
    return f


def clip_pieces(clip, width: int, height: int) -> List[Tri]:
    """Sutherland-Hodgman of one triangle of clip coordinates (x, y, z; w = 1) against near, far and the four guard-band planes, in the kernel's
    plane order, only the planes some vertex is outside of; then the fan from vertex 0, snapped.  The cases are built so that every intersection is a
    dyadic rational the kernel's binary32 arithmetic computes exactly."""
    hw, hh, cx, cy, gx, gy = (Fraction(float(v)) for v in draw_constants(width, height))

    def dist(plane, v):
        x, y, z, w = v
        return {1: z, 2: w - z, 4: x + gx * w, 8: gx * w - x, 16: y + gy * w, 32: gy * w - y}[plane]

    poly = [(Fraction(x), Fraction(y), Fraction(z), Fraction(1)) for (x, y, z) in clip]
    planes = [p for p in (1, 2, 4, 8, 16, 32) if any(dist(p, v) < 0 for v in poly)]
    for plane in planes:
        if len(poly) < 3:
            break
        out = []
        for i, a in enumerate(poly):
            b = poly[(i + 1) % len(poly)]
            da, db = dist(plane, a), dist(plane, b)
            ina, inb = da >= 0, db >= 0
            if ina:
                out.append(a)
            if ina != inb:
                p, q, dp, dq = (a, b, da, db) if ina else (b, a, db, da)
                tt = dp / (dp - dq)
                out.append(tuple(p[k] + tt * (q[k] - p[k]) for k in range(4)))
        poly = out
    pieces = []
    for i in range(1, len(poly) - 1):
        tri = (poly[0], poly[i], poly[i + 1])
        X = tuple(_round_half_even(((v[0] / v[3]) * hw + cx) * 256) for v in tri)
        Y = tuple(_round_half_even(((v[1] / v[3]) * hh + cy) * 256) for v in tri)
        pieces.append(Tri(X, Y))
    return pieces


def model_case(c: Case, split: Optional[Split] = None, rules: Rules = KERNEL) -> List[Routed]:
    """One Routed per big-list record or binned / rejected triangle of the case (a clipped triangle: one per piece that passes setup)."""
    split = split or c.full_split()
    if c.clipped:
        out = []
        for k in range(len(c.clip) // 3):
            for p in clip_pieces(c.clip[3 * k:3 * k + 3], c.width, c.height):
                r = route(p, c.width, c.height, c.scissor, split, rules, force_big=True)
                if r.route != "rejected":
                    out.append(r)
        return out
    return [route(t, c.width, c.height, c.scissor, split, rules) for t in c.tris]


def figures(c: Case, split: Optional[Split] = None) -> Dict[str, int]:
    """What the GPU must report for the case: the fragment sum over all (record, tile) pairs and the big-list length."""
    rs = model_case(c, split)
    return {"covered": sum(r.frags for r in rs), "big": sum(1 for r in rs if r.route == "big"), "binned": sum(1 for r in rs if r.route == "binned")}


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def px(p: float) -> int:
    """pixels -> 1/256 px (the argument is a multiple of 1/256)."""
    v = p * 256
    assert v == int(v)
    return int(v)


VARIANTS = (("on", 0), ("in", 1), ("out", -1))      # the value on the boundary, one sub-pixel inside it, one outside


def _maybe_t(t: Tri, axis: str) -> Tri:
    return t if axis == "x" else t.transposed()


def _k(axis, name):
    return name.replace("_x", "_" + axis)


def _reach_cases() -> List[Case]:
    out = []
    for axis in "xy":
        for n in (1, 2, 3, 4):
            limit = -32768 + (n - 1) * TW
            xr = ((n - 1) * TILE + 20) * 256 + 77
            for v, d in VARIANTS:
                t = _maybe_t(Tri((limit + d, xr, xr), (px(108) + 13, px(100) + 40, px(118) + 200), 0.25 + 0.03125 * n), axis)
                exp = {"route": "big" if d < 0 else "binned", "n" + "t" + axis: n, "margin_lo_" + axis: d, "compact": True}
                if d == 0:
                    exp["box_lo_" + axis + "_last"] = -128
                out.append(Case(f"reach_{axis}_n{n}_{v}", [t], expect=exp, boundary=v))
    return out


def _extent_cases() -> List[Case]:
    out = []
    for axis in "xy":
        for v, d in VARIANTS:
            x0 = px(160)
            t = _maybe_t(Tri((x0, x0 + 65535 - d, x0 + 300), (px(108) + 13, px(100) + 40, px(118) + 200), 0.375), axis)
            exp = {"route": "big" if d < 0 else "binned", "extent_" + axis: 65535 - d, "compact": d >= 0, "n" + "t" + axis: 3}
            out.append(Case(f"extent_{axis}_{v}", [t], expect=exp, boundary=v))
    return out


def _span_cases() -> List[Case]:
    out = []
    for axis in "xy":
        for v, d in VARIANTS:
            # first tile 1; (xmax - 128) >> 8 = 32 + 127 for xmax up to 160 * 256 + 127: the largest value with ntx = 4
            t = _maybe_t(Tri((px(37) + 10, px(160) + 127 - d, px(60)), (px(108) + 13, px(100) + 40, px(118) + 200), 0.4375), axis)
            exp = {"route": "big" if d < 0 else "binned", "n" + "t" + axis: 5 if d < 0 else 4, "compact": True, "fits": True}
            out.append(Case(f"span_{axis}_{v}", [t], expect=exp, boundary=v))
    t = Tri((px(37) + 10, px(160) + 127, px(40)), (px(40) + 3, px(37) + 9, px(160) + 127), 0.46875)
    out.append(Case("span_pair_max", [t], expect={"route": "binned", "ntx": 4, "nty": 4, "nb": 16}, boundary="on"))
    return out


def _box_cases() -> List[Case]:
    """tile_tri_from_bin's tile-relative (xmax - 128) >> 8, seen from the first tile of the span (column 4 of 8: the triangle overhangs the target's
    edge, the clamp keeps the span at 4).  127 / 128 straddle a signed byte, 255 / 286 an unsigned one; 286 is the largest value a compact triangle can
    have from a tile of its span (its first pixel in the tile's last column, its extent 65535) -- the 383 of a 9-bit field is out of reach: extent <=
    65535 keeps the box within 256 pixels of its first, and the first lies in the tile."""
    out = []
    for axis in "xy":
        for v in (127, 128, 255):
            t = _maybe_t(Tri((px(131) + 50, px(128 + v) + 228, px(140)), (px(108) + 13, px(100) + 40, px(118) + 200), 0.53125), axis)
            exp = {"route": "binned", "n" + "t" + axis: 4, f"box_hi_{axis}_first": v, f"box_hi_{axis}_last": v - 96}
            out.append(Case(f"box_{axis}_{v}", [t], expect=exp, boundary="on"))
        x0 = px(159) + 128
        t = _maybe_t(Tri((x0, x0 + 65535, x0 + 300), (px(108) + 13, px(100) + 40, px(118) + 200), 0.5625), axis)
        exp = {"route": "binned", "n" + "t" + axis: 4, f"box_hi_{axis}_first": 286, f"box_hi_{axis}_last": 190, "extent_" + axis: 65535}
        out.append(Case(f"box_{axis}_286", [t], expect=exp, boundary="on"))
        # (ox + 127) >> 8 = -128 from the last tile of a four-tile span
        t = _maybe_t(Tri((-32768 + 3 * TW, px(96 + 20) + 77, px(96 + 25)), (px(108) + 13, px(100) + 40, px(118) + 200), 0.59375), axis)
        exp = {"route": "binned", "n" + "t" + axis: 4, f"box_lo_{axis}_last": -128, "margin_lo_" + axis: 0}
        out.append(Case(f"box_{axis}_lo_m128", [t], expect=exp, boundary="on"))
    return out


def _quad(x0, y0, x1, y1, z):
    return [Tri((px(x0), px(x1), px(x0)), (px(y0), px(y0), px(y1)), z), Tri((px(x1), px(x1), px(x0)), (px(y0), px(y1), px(y1)), z)]


def _tie_cases() -> List[Case]:
    out = [Case("tie_vertices", _quad(10.5, 10.5, 50.5, 50.5, 0.625), expect={"route": "binned", "ntx": 2, "nty": 2, "union_once": 40 * 40})]
    # a shared vertical and a shared horizontal edge through the pixel centres of a tile's last / first column and row
    for name, e in (("last", 63.5), ("first", 64.5)):
        tris = _quad(20.5, 20.5, e, e, 0.65625) + _quad(e, 20.5, 100.5, e, 0.6875) + _quad(20.5, e, e, 100.5, 0.71875) + _quad(e, e, 100.5, 100.5, 0.75)
        out.append(Case(f"tie_tile_boundary_{name}", tris, expect={"route": "binned", "union_once": 80 * 80}))
    return out


def _scissor_cases() -> List[Case]:
    sc = (64, 64, 128, 128)
    cutting = Tri((px(50) + 10, px(100) + 127, px(60)), (px(108) + 13, px(100) + 40, px(118) + 200), 0.78125)
    clear = Tri((px(70) + 10, px(100) + 127, px(80)), (px(108) + 13, px(100) + 40, px(118) + 200), 0.78125)
    return [Case("scissor_cut", [cutting], scissor=sc, expect={"route": "big", "cut": True, "boxed": True, "compact": False, "ntx": 2}),
            Case("scissor_clear", [clear], scissor=sc, expect={"route": "binned", "cut": False, "ntx": 2})]


def _clipped_cases() -> List[Case]:
    F = Fraction
    # near plane: one vertex at z = -1/2, the other two at z = 1/2: both crossings at t = 1/2
    near = [(F(-1, 2), F(-1, 2), F(1, 2)), (F(1, 2), F(-1, 4), F(1, 2)), (F(0), F(3, 4), F(-1, 2))]
    # a guard-band plane: gx = 124 on a 256-wide target; vertices at x = -1/2 and one at 124 + 124.5: both crossings at t = 1/2, x = 124 (16000 px)
    guard = [(F(-1, 2), F(-1, 2), F(1, 2)), (F(-1, 2), F(1, 2), F(1, 2)), (F(497, 2), F(0), F(1, 2))]
    return [Case("clipped_near", [], clipped=True, clip=near, expect={"pieces": 2}),
            Case("clipped_guard", [], clipped=True, clip=guard, expect={"pieces": 2})]


COMPANION = Tri((px(200) + 77, px(240) + 179, px(215) + 51), (px(200) + 51, px(203) + 26, px(215) + 230), 0.875)     # two tiles: nb = 2, the pair path


def _pages_cases() -> List[Case]:
    out = []
    for n, pages in ((65, 1), (128, 1), (129, 2)):
        tris = [Tri((px(70) + 3 * k, px(80) + 5 * k, px(72) + k), (px(70) + k, px(74) + 2 * k, px(85) + 3 * k), 0.125 + k / 256.0) for k in range(n)]
        out.append(Case(f"pages_{n}", tris, env={"MIRHI_FIXED_PAGES": "1"}, pages=pages, expect={"route": "binned", "nb": 1}))
    return out


def _wave_cases(base: List[Case]) -> List[Case]:
    tris = [c.tris[0] for c in base if c.name.startswith(("reach_", "extent_", "span_"))]
    out = [Case("waves_tpw16", tris)]
    # total_slots / 64 > 256: 32 triangles per wave; > 512: 64 (tris_per_wave, mirhi_submit.h:160-163); a draw's slots are its triangles rounded up to 64
    out.append(Case("waves_tpw32", tris, pad=256 * 64 + 1 - len(tris)))
    out.append(Case("waves_tpw64", tris, pad=512 * 64 + 1 - len(tris)))
    return out


XCD_TRIS = 256      # 64 tiles x 4: the fewest triangles at which raster_mode (mirhi_scope.h:310-321) finds a MODEL scope of a 256 x 256 target dense


def xcd_case(n: int = XCD_TRIS) -> Case:
    """The reach, extent and span triangles and small single-tile ones on a grid, n in all, as one MODEL-program draw."""
    base = _reach_cases() + _extent_cases() + _span_cases()
    tris = [c.tris[0] for c in base]
    k = 0
    while len(tris) < n:
        i, j = k % 15, k // 15
        x, y = px(8 + 16 * i) + 7 * k % 256, px(8 + 16 * j) + 11 * k % 256
        tris.append(Tri((x, x + px(6) + 31, x + px(1)), (y, y + px(2) + 9, y + px(7) + 77), 0.0625 + k / 1024.0))
        k += 1
    return Case(f"xcd_lists_{n}", tris, model=True)


def tris_per_wave(c: Case) -> int:
    slots = (len(c.tris) + c.pad + 63) // 64 * 64
    waves = slots // 64
    return 16 if waves <= 256 else (32 if waves <= 512 else 64)


def unsplit_cases() -> List[Case]:
    base = _reach_cases() + _extent_cases() + _span_cases() + _box_cases() + _tie_cases() + _scissor_cases()
    return base + [Case("companion", [COMPANION], expect={"route": "binned", "nb": 2})] + _clipped_cases() + _pages_cases() + _wave_cases(base) + [xcd_case()]


def with_companion(c: Case) -> Case:
    """The case with a two-tile triangle behind it, in the same wave: __ballot(nb > 1) then takes the pair path of bin_triangle_pairs."""
    return replace(c, name=c.name + "+pair", tris=list(c.tris) + [COMPANION])


def pairable(c: Case) -> bool:
    """A binned boundary case: run alone and again with the companion."""
    return bool(c.boundary) and not c.clipped and c.expect.get("route") == "binned" and len(c.tris) == 1


# ---- tile-row split (256 x 512: 16 tile rows) ----
SPLIT_W, SPLIT_H = 256, 512
SPLIT_KINDS = ("last_owned_row", "next_band_first_pixel", "reach_from_above_on", "reach_from_above_out", "tall_255", "tall_5_rows", "nothing_owned")


def split_of(rank: int, world: int, layout: str) -> Split:
    """multigpu.split_tile_rows for the 512-row target."""
    ty = SPLIT_H // TILE
    if layout == "bands":
        per = (ty + world - 1) // world
        b = min(rank * per, ty)
        return Split(b, 1, min(b + per, ty) - b)
    return Split(rank, world, (ty - rank + world - 1) // world if rank < ty else 0)


def split_case(kind: str, world: int, layout: str) -> Case:
    """One triangle per rank, built against that rank's rows; every rank renders them all."""
    tris = []
    for r in range(world):
        s = split_of(r, world, layout)
        rows = s.rows()
        x = (px(20 + 40 * r) + 10, px(50 + 40 * r) + 127, px(30 + 40 * r))
        z = 0.25 + 0.125 * r
        # the band under test: the rank's band, or under the interleaved layout its first single row with four tile rows above it
        band_first = rows[0] if layout == "bands" else next(q for q in rows if q >= 4)
        band_last = rows[-1] if layout == "bands" else band_first
        if kind == "last_owned_row":            # the box ends on the band's last pixel row
            y1 = (band_last + 1) * TW - 1 + 128             # (ymax - 128) >> 8 = the last pixel row, largest such ymax
            tris.append(Tri(x, (y1 - px(9), y1 - px(5), y1), z))
        elif kind == "next_band_first_pixel":   # the box starts on the first pixel row below the band: this rank rejects it, the owner of that row keeps it
            y0 = (band_last + 1) * TW - 127                 # (ymin + 127) >> 8 = the next band's first pixel row, smallest such ymin
            if band_last + 1 >= SPLIT_H // TILE:
                y0 = band_first * TW - 127                  # (the last band has no next one: its own first pixel row)
            tris.append(Tri(x, (y0, y0 + px(5), y0 + px(9)), z))
        elif kind in ("reach_from_above_on", "reach_from_above_out"):
            if band_first < 4:                              # (rank 0's band starts at the target's top: nothing above it; the reach of the target's edge)
                y0 = -32768 - (1 if kind.endswith("out") else 0)
                tris.append(Tri(x, (y0, px(10), px(20) + 77), z))
            else:
                y0 = (band_first - 4) * TW - (1 if kind.endswith("out") else 0)
                tris.append(Tri(x, (y0, y0 + px(60), band_first * TW + px(20) + 77), z))
        elif kind == "tall_255":
            y0 = band_first * TW + px(3)
            # (the tip in the rank's own rows, the base in another's: a band that gets only a few rows of it still gets pixels)
            if y0 + px(255) > px(SPLIT_H - 1):
                y1 = px(SPLIT_H - 4)
                tris.append(Tri(x, (y1 - px(255), y1 - px(255), y1), z))
            else:
                tris.append(Tri(x, (y0 + px(255), y0 + px(255), y0), z))
        elif kind == "tall_5_rows":             # rows band_first - 4 .. band_first, from the first row's very top: an interleaved rank bins it, its owned rows are <= 3
            y0 = max(band_first - 4, 0) * TW
            tris.append(Tri(x, (y0, y0 + px(60), y0 + 4 * TW + px(20) + 77), z))
        elif kind == "nothing_owned":           # ends one pixel row above the band's first owned row (rank 0 at the top: starts one pixel row below its band)
            if band_first == 0:
                y0 = (band_last + 1) * TW - 127
                tris.append(Tri(x, (y0, y0 + px(5), y0 + px(9)), z))
            else:
                y1 = band_first * TW - 1 + 128
                tris.append(Tri(x, (y1 - px(9), y1 - px(5), y1), z))
        else:
            raise KeyError(kind)
    return Case(f"split_{kind}_{layout}{world}", tris, width=SPLIT_W, height=SPLIT_H)
