"""Shared builders of the sampler-state tests (tests/test_sampler_cpu.py, tests/test_gpu_sampler.py).

The yardstick of a texture's sampler state (include/mirhi.h mirhi_image_set_sampler) is the oracle under the only sampler it has, REPEAT /
LINEAR, fed a transformed scene: every new mode equals the old sampler on a rebuilt texture with rescaled texture coordinates.

  MIRRORED_REPEAT on T (w x h)  ==  REPEAT on the 2w x 2h tile [[T, T[:, ::-1]], [T[::-1], T[::-1, ::-1]]] with every uv halved
  CLAMP_TO_EDGE on T (w, h even) ==  REPEAT on the 2w x 2h texture whose extra half is w/2 copies of the last texel followed by w/2 copies
                                     of the first (per axis), uv halved and inside (-1/2 + 1/w, 3/2 - 1/w)
  NEAREST magnified k times at pixel centres k does not put on a texel edge == LINEAR on T with every texel replicated k x k, same uv
  NEAREST at texel fraction 3/4 == LINEAR on T with uv shifted by -1/4 texel (the LINEAR weights are then 1 and 0)

Halving a uv and doubling an extent are exact in binary floating point, through the interpolation and through u * (float)w, so the two sides
compute the same texel coordinates.  `sample` below is the float64 model of one level that test_sampler_cpu.py checks these statements with
before any GPU sees them; the GPU tests build their transformed textures with the same helpers.
"""
import numpy as np

REPEAT, MIRRORED_REPEAT, CLAMP_TO_EDGE = range(3)       # mirhi_address_mode
LINEAR, NEAREST = range(2)                              # mirhi_sampler_filter
MIP_LINEAR, MIP_NEAREST, MIP_BASE = range(3)            # mirhi_mip_mode


def address(i, n, mode):
    """Texel index i (an integer array) under an address mode with the level's extent n: the Vulkan specification's wrapping operation."""
    i = np.asarray(i, dtype=np.int64)
    if mode == CLAMP_TO_EDGE:
        return np.clip(i, 0, n - 1)
    if mode == MIRRORED_REPEAT:
        a = np.mod(i, 2 * n) - n
        return (n - 1) - np.where(a >= 0, a, -(1 + a))
    return np.mod(i, n)


def sample(tex, u, v, address_u=REPEAT, address_v=REPEAT, nearest=False):
    """One level of an (h, w, 4) uint8 texture at (u, v), float64, channels in [0, 1]: NEAREST reads floor(u w), floor(v h); LINEAR the four
    texels around u w - 1/2, v h - 1/2; each index then goes through its address mode."""
    t = np.asarray(tex, dtype=np.float64) / 255.0
    h, w = t.shape[:2]
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if nearest:
        return t[address(np.floor(v * h), h, address_v), address(np.floor(u * w), w, address_u)]
    fx, fy = u * w - 0.5, v * h - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0)[..., None], (fy - y0)[..., None]
    xa, xb = address(x0, w, address_u), address(x0 + 1, w, address_u)
    ya, yb = address(y0, h, address_v), address(y0 + 1, h, address_v)
    top = t[ya, xa] + (t[ya, xb] - t[ya, xa]) * ax
    bot = t[yb, xa] + (t[yb, xb] - t[yb, xa]) * ax
    return top + (bot - top) * ay


def extend_axis(tex, axis, mode):
    """Doubles an (h, w, 4) texture along `axis` (0: rows / v, 1: columns / u) so that REPEAT on the result, with that coordinate halved, is
    `mode` on the original: its mirror image behind it (MIRRORED_REPEAT), or n/2 copies of the last texel and n/2 of the first (CLAMP_TO_EDGE,
    n even), or itself again (REPEAT)."""
    tex = np.asarray(tex)
    n = tex.shape[axis]
    if mode == MIRRORED_REPEAT:
        extra = np.flip(tex, axis=axis)
    elif mode == CLAMP_TO_EDGE:
        assert n % 2 == 0, "the clamp tile needs an even extent"
        last, first = np.take(tex, [n - 1], axis=axis), np.take(tex, [0], axis=axis)
        extra = np.concatenate([np.repeat(last, n // 2, axis=axis), np.repeat(first, n // 2, axis=axis)], axis=axis)
    else:
        extra = tex
    return np.ascontiguousarray(np.concatenate([tex, extra], axis=axis))


def extended(tex, address_u, address_v):
    """The 2w x 2h texture on which REPEAT with every uv halved is (address_u, address_v) on `tex`."""
    return extend_axis(extend_axis(tex, 1, address_u), 0, address_v)


def replicated(tex, k):
    """Every texel k x k times: LINEAR on this, at pixel centres that sit on its texel centres, is NEAREST on `tex`."""
    return np.ascontiguousarray(np.repeat(np.repeat(np.asarray(tex), k, axis=0), k, axis=1))


def noise_texture(w, h, seed):
    """Independent random bytes per texel and channel: any two texels differ, so a wrong index shows."""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def banded_texture(n, seed):
    """n x n noise whose outer quarter bands are constant (the inner half, edge-replicated): box-filtering it and replicating its edge commute
    up to the level whose texels are n/4 wide, so CLAMP_TO_EDGE with a mip chain has an oracle equivalent while lambda < log2(n / 4) - 1."""
    assert n % 4 == 0
    core = noise_texture(n // 2, n // 2, seed)
    return np.ascontiguousarray(np.pad(core, ((n // 4, n // 4), (n // 4, n // 4), (0, 0)), mode="edge"))


def quad_vertices(uv0, uv1, rect=(-1.0, -1.0, 1.0, 1.0), split=None):
    """A screen-aligned quad in clip space (identity camera) as 48-byte vertices, uv running from uv0 at the rect's (x0, y0) corner to uv1 at
    (x1, y1).  `split`: (uv0b, uv1b) -- the second triangle gets vertices and a uv range of its own (six vertices, no shared ones)."""
    x0, y0, x1, y1 = rect

    def four(a, b):
        v = np.zeros((4, 12), dtype=np.float32)
        v[:, 0:3] = [[x0, y0, 0], [x1, y0, 0], [x1, y1, 0], [x0, y1, 0]]
        v[:, 3:6] = [0, 0, 1]
        v[:, 6:8] = [[a[0], a[1]], [b[0], a[1]], [b[0], b[1]], [a[0], b[1]]]
        v[:, 8:12] = [1, 0, 0, 1]
        return v
    if split is None:
        return four(uv0, uv1), np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32)
    return np.concatenate([four(uv0, uv1), four(*split)]), np.array([0, 1, 2, 4, 6, 7], dtype=np.uint32)


def quad_draw(scenes, tex, uv0, uv1, rect=(-1.0, -1.0, 1.0, 1.0), split=None, pbr=False, normal_map=None, first=0, count=6, alpha_cutoff=0.0, **extra):
    """One draw of the quad above, lit head-on by a directional light of intensity 1 (the albedo reaches the colour at full scale).  MODEL_FULL:
    the albedo texture is the only input that varies; pbr: MODEL_PBR with the texture as base colour (its alpha against `alpha_cutoff`: a pipeline with alpha_test=True) and
    `normal_map` as its normal map."""
    verts, idx = quad_vertices(uv0, uv1, rect, split)
    ident = np.eye(4, dtype=np.float32)
    if pbr:
        material = scenes.pbr_material_ubo((1.0, 1.0, 1.0, 1.0), 0.0, 0.6, 1.0, alpha_cutoff=alpha_cutoff, has_base_color=True, has_normal=normal_map is not None)
    else:
        material = scenes.material_ubo((1.0, 1.0, 1.0, 1.0), 0.0, 1.0, 1.0)
    fields = dict(vertices=verts, stride=48, count=count, first=first, indices=idx, program=scenes.PROGRAM_MODEL_PBR if pbr else scenes.PROGRAM_MODEL_FULL,
                  cull_mode=scenes.CULL_NONE, depth_test=False, depth_write=False,
                  camera=scenes.camera_ubo(ident, ident, (0.0, 0.0, 1.0)), object=scenes.object_ubo(ident),
                  light=scenes.light_ubo(direction=(0.0, 0.0, -1.0), intensity=1.0), material=material,
                  albedo_map=tex, normal_map=normal_map if normal_map is not None else scenes.WHITE_1X1)
    fields.update(extra)
    return scenes.DrawSpec(**fields)


def quad_scene(scenes, tex, W, H, uv0, uv1, name="sampler", **kw):
    return scenes.Scene(name, W, H, [quad_draw(scenes, tex, uv0, uv1, **kw)])


def halved(uv):
    return (uv[0] * 0.5, uv[1] * 0.5)


def texture(scenes, rgba8, **state):
    """scenes.Texture with sampler state by field name (address_u, address_v, mag_filter, min_filter, mip_mode) and mips / srgb / max_anisotropy"""
    return scenes.Texture(np.ascontiguousarray(rgba8), **state)


def pair(scenes, rgba8, W, H, uv0, uv1, address_u, address_v, mips=False, max_anisotropy=1, srgb=False, **kw):
    """(product scene, oracle scene) of equivalences 1 and 2: the quad under (address_u, address_v) on `rgba8`, and under the default sampler on
    the extended texture with halved uv."""
    tex = texture(scenes, rgba8, mips=mips, max_anisotropy=max_anisotropy, srgb=srgb, address_u=address_u, address_v=address_v)
    ref = texture(scenes, extended(rgba8, address_u, address_v), mips=mips, max_anisotropy=max_anisotropy, srgb=srgb)
    split = kw.pop("split", None)
    ref_split = None if split is None else (halved(split[0]), halved(split[1]))
    return (quad_scene(scenes, tex, W, H, uv0, uv1, split=split, **kw),
            quad_scene(scenes, ref, W, H, halved(uv0), halved(uv1), split=ref_split, **kw))
