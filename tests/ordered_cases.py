"""A model of fragment order and blending for the ordered resolve, and the cases placed on its machinery's boundaries.

Plain numpy and Python integers; no GPU call, no rasterisation, no shading.  resolve(initial, layers, state) takes what a segment starts from, the
segment's primitives in primitive order -- each one a cover mask, a per-pixel depth and a per-pixel source colour, taken from a render of that
triangle ALONE and OPAQUE -- and the segment's depth / blend state, and gives the frame the segment must leave: colour, depth, last writer.  What it
holds is exactly the part nothing independent held before: order, running depth, blend factors and ops, write mask, load and store.

The rules and where they come from:
  order      Vulkan 1.3 section 7.1 (rasterization order = primitive order); a clipped triangle is ONE primitive, hence one layer
  depth      Vulkan 1.3 section 29.7: the fragment's depth against the attachment's CURRENT value, written when the test passes and write is on
  blend      Vulkan 1.3 section 28.1, tables 28.1 (factors) and 28.2 (ops); pipeline.rs:411-531 (BlendFactor 0-9 and 14, BlendOp 0-4,
             ColorBlendAttachment: colour pair + op, alpha pair + op, write mask).  binary32, one rounding per operation, s*sf (+/-) d*df
  write mask Vulkan 1.3 section 28.1, the colour write mask: a masked-out component keeps the destination's value (blended segments)
  same id    DESIGN.md section 2 item 7: of two fragments of ONE primitive under ALWAYS with depth write the nearer is kept (a layer whose id is
             the pixel's last writer passes only when it is nearer)
  discard    pixel/model_pbr.hlsl:176-179: a fragment whose alpha is below the cutoff writes nothing
  area       include/mirhi.h render_area / the draw's scissor: nothing outside is read or written

A case is a list of draws; a draw is a list of SLOTS -- a live triangle, a zero-area filler (the geometry kernel leaves its slot empty) or a small
filler inside tile B -- and a state.  Only a handful of slots are live, so a case needs a handful of single-triangle renders however long it is.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from fractions import Fraction
from typing import Dict, List, Optional, Tuple

import numpy as np

import binning_cases as bc
from binning_cases import Tri, px

f32 = np.float32
NO_PRIM = 0xFFFFFFFF
W, H = 128, 64                  # 4 x 2 tiles
TILE = 32
CHUNK = 256                     # ORDERED_THREADS: slots per chunk
TILE_A, TILE_B = (1, 0), (3, 1)

(NEVER, LESS, EQUAL, LESS_OR_EQUAL, GREATER, NOT_EQUAL, GREATER_OR_EQUAL, ALWAYS) = range(8)
(ZERO_F, ONE_F, SRC_COLOR, ONE_MINUS_SRC_COLOR, DST_COLOR, ONE_MINUS_DST_COLOR, SRC_ALPHA, ONE_MINUS_SRC_ALPHA, DST_ALPHA, ONE_MINUS_DST_ALPHA) = range(10)
SRC_ALPHA_SATURATE = 14
FACTORS = tuple(range(10)) + (SRC_ALPHA_SATURATE,)      # what the pipeline accepts (the four constant-colour factors are refused)
(ADD, SUBTRACT, REVERSE_SUBTRACT, MIN, MAX) = range(5)


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class State:
    test: bool = True
    write: bool = True
    compare: int = LESS
    blend: Optional[Tuple[int, ...]] = None         # DrawSpec.blend: (src colour, dst colour, colour op, src alpha, dst alpha, alpha op, write mask)
    cutoff: Optional[float] = None                  # discard below this alpha
    area: Optional[Tuple[int, int, int, int]] = None  # (x, y, w, h): render area or scissor

    @property
    def ordered(self) -> bool:
        """mirhi_scope.h classify_scope: blended, or a depth state whose stored depth depends on the order of all fragments."""
        return self.blend is not None or (self.test and self.write and self.compare == NOT_EQUAL)


@dataclass(frozen=True)
class Rules:
    """The model's rules; the defaults are the specification's.  The others are the planted errors tests/test_ordered_cpu.py must reject."""
    initial_depth: bool = False         # the depth test reads the depth the segment started from
    dst_alpha_swapped: bool = False     # ONE_MINUS_DST_ALPHA gives DST_ALPHA
    rsub_as_sub: bool = False           # REVERSE_SUBTRACT computes SUBTRACT
    ignore_mask: bool = False           # every component is written
    sat_alpha: bool = False             # SRC_ALPHA_SATURATE's alpha factor is min(As, 1 - Ad) instead of 1


EXACT = Rules()


@dataclass
class Frame:
    color: np.ndarray       # (h, w, 4) float32
    depth: np.ndarray       # (h, w) float32 in [0, 1]
    prim: np.ndarray        # (h, w) uint32, NO_PRIM = nobody

    def copy(self) -> "Frame":
        return Frame(self.color.copy(), self.depth.copy(), self.prim.copy())


@dataclass
class Layer:
    prim: int
    cover: np.ndarray       # (h, w) bool
    depth: np.ndarray       # (h, w) float32
    color: np.ndarray       # (h, w, 4) float32


def _factor(f: int, s: np.ndarray, d: np.ndarray, rules: Rules):
    """Table 28.1: (rgb factor (..., 3), alpha factor (...,)) of blend factor f for source s and destination d (..., 4)."""
    one = f32(1.0)
    As, Ad = s[..., 3], d[..., 3]
    rep = lambda a: np.repeat(a[..., None], 3, axis=-1)
    if f == ZERO_F:
        return np.zeros_like(s[..., :3]), np.zeros_like(As)
    if f == ONE_F:
        return np.ones_like(s[..., :3]), np.ones_like(As)
    if f == SRC_COLOR:
        return s[..., :3], As
    if f == ONE_MINUS_SRC_COLOR:
        return one - s[..., :3], one - As
    if f == DST_COLOR:
        return d[..., :3], Ad
    if f == ONE_MINUS_DST_COLOR:
        return one - d[..., :3], one - Ad
    if f == SRC_ALPHA:
        return rep(As), As
    if f == ONE_MINUS_SRC_ALPHA:
        return rep(one - As), one - As
    if f == DST_ALPHA or (f == ONE_MINUS_DST_ALPHA and rules.dst_alpha_swapped):
        return rep(Ad), Ad
    if f == ONE_MINUS_DST_ALPHA:
        return rep(one - Ad), one - Ad
    if f == SRC_ALPHA_SATURATE:
        sat = np.where(As < one - Ad, As, one - Ad)
        return rep(sat), (sat if rules.sat_alpha else np.ones_like(As))
    raise ValueError(f"blend factor {f}")


def _op(op: int, s, sf, d, df, rules: Rules):
    """Table 28.2 in binary32: every product and the sum or difference rounded once (numpy float32 arithmetic does not contract)."""
    if op == ADD:
        return s * sf + d * df
    if op == SUBTRACT or (op == REVERSE_SUBTRACT and rules.rsub_as_sub):
        return s * sf - d * df
    if op == REVERSE_SUBTRACT:
        return d * df - s * sf
    if op == MIN:
        return np.where(s < d, s, d)
    if op == MAX:
        return np.where(s > d, s, d)
    raise ValueError(f"blend op {op}")


def blend(s: np.ndarray, d: np.ndarray, b: Optional[Tuple[int, ...]], rules: Rules = EXACT) -> np.ndarray:
    """The colour a fragment of source colour s leaves over destination d (both (..., 4) float32)."""
    if b is None:
        return s.copy()
    sc, dc, cop, sa, da, aop, mask = b
    assert s.dtype == np.float32 and d.dtype == np.float32
    with np.errstate(all="ignore"):
        sfc, dfc = _factor(sc, s, d, rules)[0], _factor(dc, s, d, rules)[0]
        sfa, dfa = _factor(sa, s, d, rules)[1], _factor(da, s, d, rules)[1]
        rgb = _op(cop, s[..., :3], sfc, d[..., :3], dfc, rules)
        a = _op(aop, s[..., 3], sfa, d[..., 3], dfa, rules)
    out = np.concatenate([rgb, a[..., None]], axis=-1).astype(np.float32)
    if not rules.ignore_mask:
        for k in range(4):
            if not (mask >> k) & 1:
                out[..., k] = d[..., k]
    return out


def _compare(op: int, z: np.ndarray, stored: np.ndarray) -> np.ndarray:
    return {NEVER: lambda: np.zeros(z.shape, dtype=bool), LESS: lambda: z < stored, EQUAL: lambda: z == stored, LESS_OR_EQUAL: lambda: z <= stored,
            GREATER: lambda: z > stored, NOT_EQUAL: lambda: z != stored, GREATER_OR_EQUAL: lambda: z >= stored, ALWAYS: lambda: np.ones(z.shape, dtype=bool)}[op]()


def resolve(initial: Frame, layers: List[Layer], state: State, rules: Rules = EXACT) -> Frame:
    """The frame a segment of `layers` (primitive order) under `state` leaves over `initial`.  Per layer and covered pixel: depth test against the
    running depth, discard, blend, write mask, depth write, last writer."""
    out = initial.copy()
    h, w = out.prim.shape
    inside = np.ones((h, w), dtype=bool)
    if state.area is not None:
        x, y, aw, ah = state.area
        inside[:] = False
        inside[max(y, 0):max(y + ah, 0), max(x, 0):max(x + aw, 0)] = True
    for L in layers:
        ys, xs = np.nonzero(L.cover & inside)
        if ys.size == 0:
            continue
        sl = (slice(ys.min(), ys.max() + 1), slice(xs.min(), xs.max() + 1))      # (the layer's box: a long segment of small triangles stays cheap)
        m = (L.cover & inside)[sl]
        z = L.depth[sl]
        if state.test:
            stored = (initial.depth if rules.initial_depth else out.depth)[sl]
            m = m & _compare(state.compare, z, stored)
            if state.write and state.compare == ALWAYS:
                m = m & ~((out.prim[sl] == np.uint32(L.prim)) & ~(z < stored))
        if state.cutoff is not None:
            m = m & ~(L.color[sl][..., 3] < f32(state.cutoff))
        if not m.any():
            continue
        blended = blend(L.color[sl], out.color[sl], state.blend, rules)
        out.color[sl][m] = blended[m]
        if state.test and state.write:
            out.depth[sl][m] = z[m]
        out.prim[sl][m] = np.uint32(L.prim)
    return out


def srgb8_of(color: np.ndarray) -> np.ndarray:
    """(h, w, 4) float32 RGBA -> (h, w, 4) uint8 BGRA as a B8G8R8A8_SRGB store holds it: the sRGB OETF (IEC 61966-2-1) in float64, rounded to nearest."""
    c = np.clip(np.nan_to_num(color.astype(np.float64), nan=0.0), 0.0, 1.0)
    enc = np.where(c <= 0.0031308, 12.92 * c, 1.055 * np.power(c, 1.0 / 2.4) - 0.055)
    enc[..., 3] = c[..., 3]
    q = np.floor(enc * 255.0 + 0.5).astype(np.uint8)
    return q[..., [2, 1, 0, 3]]


# ------------------------------------------------------------------------------------------------
# slots, draws, cases
# ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Live:
    tri: Optional[Tri] = None
    clip: Optional[Tuple[Tuple[Fraction, Fraction, Fraction], ...]] = None      # a clipped triangle: three clip-space vertices (w = 1)
    color: Tuple[float, float, float] = (0.5, 0.5, 0.5)                          # TRIANGLE program: the flat vertex colour (dyadic)


ZERO = "zero"           # three times one point: S == 0, the slot stays empty
FILL = "fill"           # a small triangle wholly inside tile B
FILL_TRI = Live(Tri((px(100) + 40, px(112) + 9, px(103) + 77), (px(40) + 13, px(45) + 200, px(55) + 31), 0.625), color=(0.25, 0.125, 0.375))

OPAQUE = State(True, True, LESS, None)
ORDER_BLEND = (ONE_F, SRC_COLOR, ADD, ONE_F, ZERO_F, ADD, 0xF)     # d' = s + d * s: not commutative, independent of alpha
PLAIN = State(True, False, LESS_OR_EQUAL, ORDER_BLEND)              # every fragment passes against the clear depth 1, nothing is written


@dataclass
class Draw:
    slots: List[object]
    state: State
    alpha: Optional[float] = None       # None: the TRIANGLE program (source alpha 1).  Else MODEL_FULL under identity matrices, unlit: the source colour
    base: Tuple[float, float, float] = (0.5, 0.5, 0.5)     # is RN(RN(base * 0.03) * 32) whatever the pixel, its alpha the material's
    instances: int = 1
    scissor: Optional[Tuple[int, int, int, int]] = None


@dataclass
class Case:
    name: str
    draws: List[Draw]
    width: int = W
    height: int = H
    clear_color: Tuple[float, float, float, float] = (0.125, 0.375, 0.625, 0.5)
    clear_depth: float = 1.0
    render_area: Optional[Tuple[int, int, int, int]] = None
    want_depth: bool = True             # False: a scope without a depth attachment (the segments hand depth over in the transient buffer)
    pack: bool = False                  # the blend table: the k-th live slots of all states are disjoint and come from ONE opaque render
    expect: Dict[str, object] = field(default_factory=dict)

    def prim_base(self, di: int) -> int:
        return sum(len(d.slots) * d.instances for d in self.draws[:di])

    def segments(self) -> List[Tuple[State, List[int]]]:
        """The scope's segments: maximal runs of draws of one state (mirhi_api.hip record_draw cuts where the state changes)."""
        out: List[Tuple[State, List[int]]] = []
        for di, d in enumerate(self.draws):
            if out and out[-1][0] == d.state:
                out[-1][1].append(di)
            else:
                out.append((d.state, [di]))
        return out

    def ordered_segments(self) -> int:
        return sum(1 for s, _ in self.segments() if s.ordered)

    def live_slots(self, di: int) -> List[int]:
        return [k for k, s in enumerate(self.draws[di].slots) if isinstance(s, Live)]

    def segment_slots(self, si: int) -> List[int]:
        """prim - ordered_first of every live primitive of segment si."""
        _, dis = self.segments()[si]
        first = self.prim_base(dis[0])
        out = []
        for di in dis:
            d = self.draws[di]
            for inst in range(d.instances):
                out += [self.prim_base(di) + inst * len(d.slots) + k - first for k in self.live_slots(di)]
        return out


# ---- vertex streams ----
def _positions(slot, width, height) -> List[List[float]]:
    if slot == ZERO:
        return [[0.25, 0.25, 0.5]] * 3
    if slot == FILL:
        slot = FILL_TRI
    if slot.clip is not None:
        return [[float(x), float(y), float(z)] for (x, y, z) in slot.clip]
    t = slot.tri
    if not bc.round_trip(t, width, height):
        raise ValueError(f"{t} does not round-trip on {width} x {height}")
    return [[*bc.clip_xy(X, Y, width, height), f32(t.z)] for X, Y in zip(t.X, t.Y)]


def _color(slot) -> Tuple[float, float, float]:
    return (0.0, 0.0, 0.0) if slot == ZERO else (FILL_TRI.color if slot == FILL else slot.color)


def draw_spec(scenes, d: Draw, slots, state: State, width: int, height: int, instances: int = 1):
    pos = np.asarray([p for s in slots for p in _positions(s, width, height)], dtype=f32).reshape(-1, 3)
    n = pos.shape[0]
    kw = dict(count=n, cull_mode=scenes.CULL_NONE, depth_test=state.test, depth_write=state.write, depth_compare=state.compare, blend=state.blend,
              scissor=d.scissor, instances=instances)
    if d.alpha is None:
        col = np.asarray([_color(s) for s in slots for _ in range(3)], dtype=f32).reshape(-1, 3)
        return scenes.DrawSpec(vertices=np.concatenate([pos, col], axis=1), stride=24, program=scenes.PROGRAM_TRIANGLE, **kw)
    eye = np.eye(4, dtype=f32)
    v48 = np.zeros((n, 12), dtype=f32)
    v48[:, 0:3] = pos
    v48[:, 5] = 1.0
    v48[:, 8] = 1.0
    v48[:, 11] = 1.0
    return scenes.DrawSpec(vertices=v48, stride=48, program=scenes.PROGRAM_MODEL_FULL, camera=scenes.camera_ubo(eye, eye, (0.0, 0.0, 1.0)),
                           object=scenes.object_ubo(eye), light=scenes.light_ubo(direction=(0.0, 0.0, -1.0), intensity=0.0),
                           material=scenes.material_ubo(tuple(d.base) + (d.alpha,), 0.0, 0.5, 32.0), albedo_map=scenes.WHITE_1X1, normal_map=scenes.WHITE_1X1, **kw)


def scene_of(c: Case, scenes, draws: Optional[List[int]] = None, area: bool = True):
    """The case's scope (draws: only these draws of it, their primitive ids then count from 0)."""
    use = range(len(c.draws)) if draws is None else draws
    specs = [draw_spec(scenes, c.draws[di], c.draws[di].slots, c.draws[di].state, c.width, c.height, c.draws[di].instances) for di in use]
    return scenes.Scene(c.name, c.width, c.height, specs, clear_color=c.clear_color, clear_depth=c.clear_depth, render_area=c.render_area if area else None)


# ---- single-layer renders ----
def _source_key(c: Case, di: int, k: int):
    d = c.draws[di]
    slot = d.slots[k]
    return (FILL_TRI if slot == FILL else slot, d.alpha, tuple(d.base) if d.alpha is not None else None, d.scissor)


def source_groups(c: Case) -> List[List[tuple]]:
    """The opaque renders the case's layers come from: each group a list of source keys drawn in ONE scope, one draw of one triangle each (a group of
    more than one key: the packed table, whose k-th live triangles lie in cells of their own)."""
    if c.pack:
        ranks: Dict[int, List[tuple]] = {}
        for s, dis in c.segments():
            keys = [_source_key(c, di, k) for di in dis for k in c.live_slots(di)]
            for r, key in enumerate(keys):
                ranks.setdefault(r, []).append(key)
        return [ranks[r] for r in sorted(ranks)]
    seen, out = set(), []
    for di, d in enumerate(c.draws):
        for k, slot in enumerate(d.slots):
            if slot == ZERO:
                continue
            key = _source_key(c, di, k)
            if key not in seen:
                seen.add(key)
                out.append([key])
    return out


def group_scene(c: Case, scenes, group: List[tuple]):
    """One group as a scope of its own: every triangle alone in its draw, opaque, LESS with write over the far clear."""
    specs = []
    for slot, alpha, base, scissor in group:
        d = Draw([slot], OPAQUE, alpha=alpha, base=base or (0.5, 0.5, 0.5), scissor=scissor)
        specs.append(draw_spec(scenes, d, d.slots, OPAQUE, c.width, c.height))
    return scenes.Scene(c.name + "-layer", c.width, c.height, specs, clear_color=(0.0, 0.0, 0.0, 0.0), clear_depth=1.0)


def sources_of(c: Case, scenes, render) -> Dict[tuple, Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """key -> (cover, depth, colour) through render(scene) -> dict(color, prim, depth), the renderer under test or the oracle."""
    out = {}
    for group in source_groups(c):
        got = render(group_scene(c, scenes, group), tuple(group))
        for i, key in enumerate(group):
            out[key] = (got["prim"] == np.uint32(i), got["depth"], got["color"])
    return out


def initial_frame(c: Case, prior: Optional[Frame] = None) -> Frame:
    """What the scope's first segment starts from: the clear values -- inside the render area, over `prior` (what the attachments held), when it has one."""
    h, w = c.height, c.width
    clear = Frame(np.tile(np.asarray(c.clear_color, dtype=f32), (h, w, 1)), np.full((h, w), f32(min(max(c.clear_depth, 0.0), 1.0)), dtype=f32),
                  np.full((h, w), NO_PRIM, dtype=np.uint32))
    if c.render_area is None:
        return clear
    x, y, aw, ah = c.render_area
    out = prior.copy()
    for a, b in ((out.color, clear.color), (out.depth, clear.depth), (out.prim, clear.prim)):
        a[y:y + ah, x:x + aw] = b[y:y + ah, x:x + aw]
    return out


def layers_of(c: Case, di: int, sources) -> List[Layer]:
    d = c.draws[di]
    out = []
    for inst in range(d.instances):
        for k, slot in enumerate(d.slots):
            if slot == ZERO:
                continue
            cover, depth, color = sources[_source_key(c, di, k)]
            out.append(Layer(c.prim_base(di) + inst * len(d.slots) + k, cover, depth, color))
    return out


def model_frame(c: Case, sources, rules: Rules = EXACT, prior: Optional[Frame] = None, permute=None) -> Frame:
    """The case's frame by the model: segment after segment, each from what the one before left.  permute(layers) -> layers: a planted reordering."""
    frame = initial_frame(c, prior)
    for state, dis in c.segments():
        layers = [L for di in dis for L in layers_of(c, di, sources)]
        if permute is not None:
            layers = permute(layers)
        st = state
        scissors = {c.draws[di].scissor for di in dis}
        area = c.render_area
        if scissors != {None}:
            assert len(scissors) == 1 and area is None
            area = next(iter(scissors))
        if area is not None:
            st = replace(state, area=area)
        frame = resolve(frame, layers, st, rules)
    return frame


# ------------------------------------------------------------------------------------------------
# the live triangles: eight that share the pixels around (50, 22) of tile A, each with corners of its own; dyadic colours, one depth each
# ------------------------------------------------------------------------------------------------
_CORNERS = [((41, 15), (60, 18), (48, 30)), ((43, 13), (58, 27), (44, 28)), ((40, 22), (57, 13), (56, 30)), ((45, 12), (61, 24), (42, 27)),
            ((39, 18), (59, 16), (52, 31)), ((47, 11), (60, 29), (41, 24)), ((42, 14), (62, 21), (46, 31)), ((44, 16), (58, 12), (53, 30))]


def live(k: int, z: Optional[float] = None, dy: int = 0, color=None) -> Live:
    """Live triangle k (dy: moved down by dy pixels -- across the tile-row boundary for the split cases)."""
    p = _CORNERS[k]
    X = tuple(px(p[j][0]) + (17 * k + 61 * j + 5) % 256 for j in range(3))
    Y = tuple(px(p[j][1] + dy) + (29 * k + 83 * j + 3) % 256 for j in range(3))
    col = color or ((k + 1) / 16.0, (2 * k + 3) / 32.0, (15 - k) / 16.0)
    return Live(Tri(X, Y, 0.25 + k / 32.0 if z is None else z), color=col)


F = Fraction
NEAR = tuple(bc._clipped_cases()[0].clip)      # two vertices at z = 1/2, one at -1/2: both crossings at t = 1/2; on 128 x 64 the visible quad is
#                                                (32, 16) (96, 24) (80, 40) (48, 36) and its fan's shared edge runs through the live triangles
NEAR_B = ((F(1, 2), F(1, 4), F(1, 2)), (F(15, 16), F(3, 8), F(1, 2)), (F(3, 4), F(7, 8), F(-1, 2)))      # the same construction inside tile B


def guard(width: int):
    """binning_cases' guard-band construction for a target of `width`: two vertices at x = -1/2 and one at 2 gx + 1/2, both crossings at t = 1/2, x = gx."""
    gx = Fraction(float(bc.draw_constants(width, 64)[4]))
    return ((F(-1, 2), F(-1, 2), F(1, 2)), (F(-1, 2), F(1, 2), F(1, 2)), (2 * gx + F(1, 2), F(0), F(1, 2)))


CLIP_NEAR = Live(clip=NEAR, color=(0.3125, 0.6875, 0.1875))
CLIP_GUARD = Live(clip=guard(W), color=(0.8125, 0.21875, 0.4375))
CLIP_NEAR_B = Live(clip=NEAR_B, color=(0.5625, 0.3125, 0.9375))


def _segment(n: int, lives: Dict[int, Live], fill=lambda i: FILL if i % 4 == 1 else ZERO) -> List[object]:
    return [lives[i] if i in lives else fill(i) for i in range(n)]


# ---- a. slot positions ----
def slot_cases(dy: int = 0) -> List[Case]:
    L = lambda k: live(k, dy=dy)
    out = [Case("slots_1", [Draw([L(0)], PLAIN)], expect={"slots": [0]}),
           Case("slots_256", [Draw(_segment(256, {0: L(0), 255: L(1)}), PLAIN)], expect={"slots": [0, 255]}),
           Case("slots_257", [Draw(_segment(257, {255: L(0), 256: L(1)}), PLAIN)], expect={"slots": [255, 256]}),
           Case("slots_513", [Draw(_segment(513, {0: L(0), 255: L(1), 256: L(2), 511: L(3), 512: L(4)}), PLAIN)], expect={"slots": [0, 255, 256, 511, 512]})]
    # chunk 1 holds tile-B fillers only, chunks 0 and 2 none: each of the two tiles skips the other's chunks
    lives = {3: L(0), 200: L(1), 255: L(2), 512: L(3), 600: L(4), 767: L(5)}
    out.append(Case("slots_768_skip", [Draw(_segment(768, lives, fill=lambda i: FILL if 256 <= i < 512 else ZERO), PLAIN)], expect={"slots": sorted(lives)}))
    # ordered_first = 100: the chunks are counted from the segment's first primitive, not from the scope's
    under = Live(Tri((px(36), px(62), px(40)), (px(8), px(14), px(30)), 0.9375), color=(0.5, 0.25, 0.75))
    opaque = Draw(_segment(100, {7: under, 64: FILL_TRI}, fill=lambda i: ZERO), OPAQUE)
    lives = {0: L(0), 155: L(1), 156: L(2), 255: L(3), 256: L(4), 299: L(5)}
    out.append(Case("slots_300_behind_100", [opaque, Draw(_segment(300, lives), State(True, False, LESS, ORDER_BLEND))], expect={"slots": sorted(lives), "segment": 1}))
    # two draws of one blend state, the second instanced: find_draw with num_draws > 1, an instance's primitives again
    out.append(Case("slots_two_draws_instanced", [Draw([L(0), ZERO, L(1)], PLAIN), Draw([L(2), FILL, L(3)], PLAIN, instances=2)],
                    expect={"slots": [0, 2, 3, 5, 6, 8]}))
    return out


# ---- b. markers ----
def marker_cases(dy: int = 0) -> List[Case]:
    L = lambda k: live(k, dy=dy)
    seg = lambda n, lives, **kw: [Draw(_segment(n, lives, **kw), PLAIN)]
    return [Case("marker_at_0", seg(300, {0: CLIP_NEAR, 100: L(0), 280: L(1)}), expect={"markers": [0]}),
            Case("marker_at_255", seg(300, {100: L(0), 255: CLIP_GUARD, 280: L(1)}), expect={"markers": [255]}),
            Case("marker_at_256", seg(300, {100: L(0), 256: CLIP_NEAR, 280: L(1)}), expect={"markers": [256]}),
            Case("markers_adjacent", seg(200, {129: L(0), 130: CLIP_NEAR, 131: CLIP_GUARD, 132: L(1)}), expect={"markers": [130, 131]}),
            Case("marker_between", seg(200, {63: L(0), 64: CLIP_NEAR, 65: L(1)}), expect={"markers": [64]}),
            Case("marker_between_guard", seg(200, {30: L(2), 31: CLIP_GUARD, 32: L(3)}), expect={"markers": [31]}),
            # chunk 1: the marker is all tile A gets (zero-area fillers around it)
            Case("marker_alone_in_chunk", seg(512, {10: L(0), 250: L(1), 300: CLIP_NEAR}, fill=lambda i: ZERO if i >= 256 else (FILL if i % 4 == 1 else ZERO)),
                 expect={"markers": [300]}),
            # the marker's pieces lie in tile B; the chunk's ordinary slots hit tile A, before and behind it
            Case("marker_misses_tile", seg(200, {40: L(0), 41: CLIP_NEAR_B, 42: L(1), 150: L(2)}), expect={"markers": [41]}),
            Case("marker_only_near", seg(1, {0: CLIP_NEAR}), expect={"markers": [0]}),
            Case("marker_only_guard", seg(1, {0: CLIP_GUARD}), expect={"markers": [0]})]


# ---- c. running depth ----
# op -> (clear depth, the layers' depths in primitive order, depth of the opaque segment underneath).  The order is chosen so that a layer passes against
# the depth the segment started from and fails against what an earlier layer wrote (or the reverse): LESS 0.5, then 0.75 (passes against the clear 1.0
# only), then 0.25.  EQUAL can only rewrite the value it found and ALWAYS reads nothing: there the two rules cannot differ, and the CPU test asserts
# that they do not.  Of the ties, LESS tells the rules apart (the second layer fails against the first, passes against the clear depth).
DEPTH_ORDERS = {LESS: (1.0, (0.5, 0.75, 0.25, 0.375), 0.875), LESS_OR_EQUAL: (1.0, (0.5, 0.75, 0.5, 0.25), 0.875),
                GREATER: (0.0, (0.5, 0.25, 0.75, 0.625), 0.125), GREATER_OR_EQUAL: (0.0, (0.5, 0.25, 0.5, 0.75), 0.125),
                EQUAL: (0.5, (0.5, 0.25, 0.5, 0.75), 0.5), NOT_EQUAL: (0.5, (0.25, 0.25, 0.5, 0.25), 0.75), ALWAYS: (0.5, (0.5, 0.75, 0.25, 0.5), 0.75)}
TIES = {LESS: (1.0, (0.5, 0.5), 0.875), LESS_OR_EQUAL: (1.0, (0.5, 0.5), 0.875), EQUAL: (0.5, (0.5, 0.5), 0.5)}
DEPTH_RUNS = ("first", "behind_opaque", "behind_opaque_transient")
OP_NAMES = {LESS: "less", LESS_OR_EQUAL: "less_or_equal", GREATER: "greater", GREATER_OR_EQUAL: "greater_or_equal", EQUAL: "equal", NOT_EQUAL: "not_equal", ALWAYS: "always"}


def depth_cases() -> List[Case]:
    out = []
    rows = [(f"depth_blend_{OP_NAMES[op]}", op, ORDER_BLEND, v) for op, v in DEPTH_ORDERS.items()]
    rows.append(("depth_not_equal_opaque", NOT_EQUAL, None, DEPTH_ORDERS[NOT_EQUAL]))
    rows += [(f"depth_tie_{OP_NAMES[op]}", op, ORDER_BLEND, v) for op, v in TIES.items()]
    for name, op, bl, (clear, zs, under_z) in rows:
        lives = [live(k, z=z) for k, z in enumerate(zs)]
        seg = Draw([lives[0], ZERO] + lives[1:], State(True, True, op, bl))
        for run in DEPTH_RUNS:
            draws = [seg]
            if run != "first":
                # an opaque triangle under half of the live pixels: ALWAYS with write stores its depth whatever the clear depth is
                under = Live(Tri((px(30), px(52), px(34)), (px(6), px(20), px(31)), under_z), color=(0.5, 0.25, 0.75))
                draws = [Draw([under, FILL], State(True, True, ALWAYS, None)), seg]
            out.append(Case(f"{name}-{run}", draws, clear_depth=clear, want_depth=run != "behind_opaque_transient",
                            expect={"op": op, "differs": op not in (EQUAL, ALWAYS) and not (name.startswith("depth_tie") and op != LESS), "segment": len(draws) - 1}))
    return out


# ---- d. the blend table ----
@dataclass(frozen=True)
class Row:
    name: str
    blend: Tuple[int, ...]


# Over the clear alpha 0.5 the FIRST layer cannot tell DST_ALPHA from ONE_MINUS_DST_ALPHA (both 0.5): the second layer does, where it lies over the first,
# if the first left another alpha.  The shift pairs a colour source factor 9 with the alpha source factor SRC_ALPHA (0.0625 + 0.5 * any factor value is
# not 0.5) and a colour destination factor 9 with the alpha destination factor ZERO (0.25 * any factor value is not 0.5).
A_SHIFT = (8, 2)


def table_rows() -> List[Row]:
    """121 colour-factor pairs under ADD; under each other op eleven pairs in which every factor is once source and once destination; the alpha pair
    is the colour pair shifted by A_SHIFT places of FACTORS, so every factor occurs in both alpha positions under every op; the alpha op is the colour op."""
    n = len(FACTORS)
    rows = []
    for i in range(n):
        for j in range(n):
            rows.append(Row(f"add_{FACTORS[i]}_{FACTORS[j]}", (FACTORS[i], FACTORS[j], ADD, FACTORS[(i + A_SHIFT[0]) % n], FACTORS[(j + A_SHIFT[1]) % n], ADD, 0xF)))
    for op, shift in ((SUBTRACT, 1), (REVERSE_SUBTRACT, 4), (MIN, 6), (MAX, 9)):
        for i in range(n):
            j = (i + shift) % n
            rows.append(Row(f"op{op}_{FACTORS[i]}_{FACTORS[j]}", (FACTORS[i], FACTORS[j], op, FACTORS[(i + A_SHIFT[0]) % n], FACTORS[(j + A_SHIFT[1]) % n], op, 0xF)))
    return rows


def mask_rows() -> List[Row]:
    """All sixteen write masks (0 included: the pipeline accepts it), each under a colour op and an alpha op that differ (alpha: MIN or MAX)."""
    return [Row(f"mask_{m}", (SRC_ALPHA, ONE_MINUS_SRC_ALPHA, m % 3, ONE_MINUS_DST_ALPHA, SRC_ALPHA_SATURATE, MIN + m % 2, m)) for m in range(16)]


TABLE_CLEAR = (0.125, 0.375, 0.625, 0.5)
TABLE_ALPHAS = (0.25, 0.75)         # SRC_ALPHA_SATURATE: 0.25 < 1 - 0.5 < 0.75
TABLE_BASES = ((0.75, 0.5, 0.25), (0.25, 0.625, 0.875))
CELL = 8


def _cell_tris(cx: int, cy: int):
    """Two triangles inside the 8 x 8 pixel cell (cx, cy): pixels of the first only, of the second only and of both."""
    ox, oy = CELL * cx, CELL * cy
    a = Tri((px(ox + 0.5), px(ox + 6.5), px(ox + 2.5)), (px(oy + 0.5), px(oy + 1.5), px(oy + 6.5)), 0.5)
    b = Tri((px(ox + 7.5), px(ox + 6.5), px(ox + 1.5)), (px(oy + 2.5), px(oy + 7.5), px(oy + 4.5)), 0.5)
    return a, b


def table_case(name: str, rows: List[Row], width: int = W, height: int = H, cells: Optional[List[Tuple[int, int]]] = None) -> Case:
    """One scope: row r is a segment of two one-triangle draws (source alpha 0.25, then 0.75) in cell r.  Every other tile of the target is one no
    record of the segment reaches (may_skip), and every segment starts from what the one before stored."""
    per_row = width // CELL
    draws = []
    for r, row in enumerate(rows):
        cx, cy = cells[r] if cells else (r % per_row, r // per_row)
        assert cy < height // CELL
        st = State(True, False, LESS_OR_EQUAL, row.blend)
        for t, alpha, base in zip(_cell_tris(cx, cy), TABLE_ALPHAS, TABLE_BASES):
            draws.append(Draw([Live(t)], st, alpha=alpha, base=base))
    return Case(name, draws, width=width, height=height, clear_color=TABLE_CLEAR, pack=True, expect={"rows": [r.name for r in rows]})


def table_cases() -> List[Case]:
    rows = table_rows()
    return [table_case("table_add", rows[:121]), table_case("table_ops_and_masks", rows[121:] + mask_rows())]


def row_case(row: Row) -> Case:
    """One row alone in cell (0, 0) of a 64 x 64 target: what the rows are told apart on."""
    return table_case("row_" + row.name, [row], width=64, height=64)


def cell_of(c: Case, r: int):
    per_row = c.width // CELL
    return (slice(CELL * (r // per_row), CELL * (r // per_row) + CELL), slice(CELL * (r % per_row), CELL * (r % per_row) + CELL))


# ---- e. tiles nobody reaches, load and store ----
def _recognisable() -> Draw:
    """An opaque segment that leaves every tile with pixels of several primitives and of the clear colour."""
    tris = [Live(Tri((px(2), px(126), px(6)), (px(3), px(9), px(60)), 0.9375), color=(0.75, 0.5, 0.25)),
            Live(Tri((px(125), px(122), px(20)), (px(12), px(62), px(58)), 0.90625), color=(0.25, 0.75, 0.5)),
            Live(Tri((px(34), px(63), px(40)), (px(2), px(10), px(31)), 0.875), color=(0.5, 0.125, 0.875))]
    return Draw(tris, OPAQUE)


def load_store_cases() -> List[Case]:
    blended = Draw([live(0), ZERO, live(1), live(2)], State(True, False, LESS, ORDER_BLEND))
    return [Case("untouched_behind_opaque", [_recognisable(), blended], expect={"segment": 1, "base_draws": [0]}),
            Case("untouched_first_segment_clear", [Draw([live(0), ZERO, live(1)], PLAIN)]),
            # a partial scissor across the edge between tile A and its right neighbour: the records are `boxed`
            Case("scissor_across_tiles", [Draw([Live(Tri((px(40) + 9, px(90) + 77, px(52) + 130), (px(4) + 5, px(12) + 200, px(30) + 19), 0.5), color=(0.375, 0.5, 0.8125)),
                                                live(1)], PLAIN, scissor=(45, 7, 33, 18))], expect={"boxed": True}),
            # a render area off the tile grid on all four sides, over prefilled attachments
            Case("area_unaligned", [Draw([live(0), live(1), Live(Tri((px(10), px(120), px(60)), (px(5), px(30), px(62)), 0.5), color=(0.625, 0.25, 0.5))], PLAIN)],
                 render_area=(37, 9, 70, 41))]


# ---- f. blocks and quadrants ----
def block_cases() -> List[Case]:
    """64 x 64: one large triangle over all four tiles; in tile (1, 1) three thin triangles along the rows 8, 16, 24 of the tile and three along its
    columns 8, 16, 24: together they cross every 8 x 8 block boundary and both wave-quadrant boundaries."""
    ox, oy = 32, 32
    big = Live(Tri((px(-20), px(150), px(-10)), (px(-15), px(-5), px(140)), 0.75), color=(0.5, 0.75, 0.25))
    thin = []
    for k, b in enumerate((8, 16, 24)):
        thin.append(Live(Tri((px(ox + 1) + 7 * k, px(ox + 31) - 5 * k, px(ox + 17) + 11 * k), (px(oy + b - 2) + 9, px(oy + b - 1) + 130, px(oy + b + 2) + 77), 0.5 - k / 16.0),
                         color=((k + 2) / 8.0, (5 - k) / 16.0, (2 * k + 1) / 8.0)))
        thin.append(Live(Tri((px(ox + b - 2) + 21, px(ox + b + 2) + 99, px(ox + b - 1) + 140), (px(oy + 1) + 5 * k, px(oy + 15) + 3 * k, px(oy + 31) - 7 * k), 0.4375 - k / 16.0),
                         color=((6 - k) / 8.0, (k + 3) / 16.0, (7 - 2 * k) / 8.0)))
    return [Case("blocks_and_quadrants", [Draw([big] + thin, PLAIN)], width=64, height=64)]


# ---- g. the 8-bit target: single ordered segments ----
def srgb8_cases() -> List[Case]:
    by = {c.name: c for c in slot_cases() + marker_cases()}
    rows = {r.name: r for r in table_rows() + mask_rows()}
    picked = [by[n] for n in ("slots_1", "slots_257", "slots_513", "marker_between", "marker_at_255", "marker_only_near")]
    picked += [row_case(rows[n]) for n in ("add_6_7", "add_14_9", "add_5_3", "op2_2_6", "op4_3_1", "mask_5")]
    return [replace(c, name="srgb8_" + c.name) for c in picked]


# ---- h. tile-row split: the live triangles lie across the boundary between the two tile rows ----
def split_cases() -> List[Case]:
    a = next(c for c in slot_cases(dy=10) if c.name == "slots_257")
    b = next(c for c in marker_cases(dy=10) if c.name == "marker_between")
    return [replace(a, name="split_slots_257"), replace(b, name="split_marker_between")]


def float_cases() -> List[Case]:
    """Every case rendered on an R32G32B32A32_SFLOAT target."""
    return slot_cases() + marker_cases() + depth_cases() + table_cases() + load_store_cases() + block_cases()


def clipped_lives(c: Case) -> List[Live]:
    return [s for d in c.draws for s in d.slots if isinstance(s, Live) and s.clip is not None]
