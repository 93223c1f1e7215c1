"""Numpy model of the IBL precompute passes (mirhi_ibl_* of include/mirhi.h): the reference's four compute shaders
(shaders/hlsl/compute/{equirect_to_cubemap,irradiance_map,prefilter_map,brdf_lut}.hlsl) restated operation by operation, with
the cube and equirect samplers this build states in the header.  There is no oracle for these passes: this model, run in float64,
is the yardstick the GPU kernels are measured against; run in float32 (`dtype=np.float32`, same operation order, serial sums) it
gives the error a float32 evaluation of the same formulas has, which is what the GPU tolerance is derived from.  The last section is the
consumer of those images: the ambient term of pixel/model_pbr_ibl.hlsl (MODEL_PBR_IBL, mirhi_cmd_bind_ibl) over the same samplers.

A cube is a list of levels, level l an array [6, n >> l, n >> l, C] (faces +X, -X, +Y, -Y, +Z, -Z; rows top first).  pack_cube /
unpack_cube convert to and from the one-allocation layout of mirhi_image_create_cube (level-major, face-major, row-major)."""
from __future__ import annotations

import numpy as np

PI = 3.14159265359          # the shaders' #define, not math.pi
SAMPLE_DELTA = 0.025        # irradiance_map.hlsl:97
PREFILTER_RESOLUTION = 512.0   # prefilter_map.hlsl:204, hard-coded there
LUT_SAMPLES = 1024          # brdf_lut.hlsl:133


# ---- layout -------------------------------------------------------------------------------------------------------------------
def level_offset(size: int, level: int) -> int:
    """First texel of `level` in the packed chain: 6 * sum over k < level of (size >> k)^2."""
    return 6 * sum((size >> k) ** 2 for k in range(level))


def cube_texels(size: int, levels: int) -> int:
    return level_offset(size, levels)


def unpack_cube(flat, size: int, levels: int):
    """Views of a packed chain ([texels, C] or flat) as a list of [6, m, m, C] levels."""
    flat = np.asarray(flat)
    flat = flat.reshape(cube_texels(size, levels), -1)
    out = []
    for l in range(levels):
        m = size >> l
        o = level_offset(size, l)
        out.append(flat[o:o + 6 * m * m].reshape(6, m, m, flat.shape[1]))
    return out


def pack_cube(levels) -> np.ndarray:
    return np.concatenate([np.asarray(l, dtype=np.float32).reshape(-1, l.shape[-1]) for l in levels], axis=0)


# ---- directions ---------------------------------------------------------------------------------------------------------------
def _normalize(v):
    return v / np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])[..., None]


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def cube_direction(face, uv, dtype=np.float64):
    """GetCubemapDirection (equirect_to_cubemap.hlsl:22-56): face index (scalar or array) and uv [..., 2] in [0, 1] -> unit vector."""
    T = np.dtype(dtype).type
    uv = np.asarray(uv, dtype=dtype)
    u = uv[..., 0] * T(2.0) - T(1.0)
    v = uv[..., 1] * T(2.0) - T(1.0)
    face = np.broadcast_to(np.asarray(face), u.shape)
    one = np.ones_like(u)
    table = [(one, -v, -u), (-one, -v, u), (u, one, v), (u, -one, -v), (u, -v, one), (-u, -v, -one)]
    d = np.zeros(u.shape + (3,), dtype=dtype)
    for f, comps in enumerate(table):
        sel = face == f
        for k in range(3):
            d[..., k] = np.where(sel, comps[k], d[..., k])
    return _normalize(d)


def texel_directions(n: int, dtype=np.float64):
    """Directions of the texel centres of an n^2 cube: [6, n, n, 3] (uv = (pixel + 0.5) / n, as every pass computes it)."""
    T = np.dtype(dtype).type
    c = (np.arange(n, dtype=dtype) + T(0.5)) / T(n)
    uv = np.stack(np.broadcast_arrays(c[None, None, :], c[None, :, None]), axis=-1)
    uv = np.broadcast_to(uv, (6, n, n, 2))
    face = np.arange(6)[:, None, None]
    return cube_direction(face, uv, dtype)


# ---- samplers (include/mirhi.h, "IBL precompute": the build's own reading, sampler.rs is empty) ----------------------------------
def select_face(d, dtype=np.float64):
    """The Vulkan specification's cube-map face selection: major axis = largest magnitude, ties prefer z, then y, then x;
    returns (face, s, t) with s = 0.5 * (sc / |ma|) + 0.5."""
    T = np.dtype(dtype).type
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    isz = (az >= ax) & (az >= ay)
    isy = ~isz & (ay >= ax)
    face = np.where(isz, np.where(z < 0, 5, 4), np.where(isy, np.where(y < 0, 3, 2), np.where(x < 0, 1, 0)))
    sc = np.where(isz, np.where(z < 0, -x, x), np.where(isy, x, np.where(x < 0, z, -z)))
    tc = np.where(isz, -y, np.where(isy, np.where(y < 0, -z, z), -y))
    ma = np.where(isz, az, np.where(isy, ay, ax))
    s = T(0.5) * (sc / ma) + T(0.5)
    t = T(0.5) * (tc / ma) + T(0.5)
    return face, s, t


def _bilinear_face(level, face, s, t, dtype):
    """Bilinear inside the selected face, clamp to edge (not seamless): x = s n - 1/2, floor, fraction, four clamped texels."""
    T = np.dtype(dtype).type
    n = level.shape[1]
    flat = level.reshape(-1, level.shape[-1])          # (six faces of a cube level, or the one "face" of a 2-D image: sample_lut)
    x = s * T(n) - T(0.5)
    y = t * T(n) - T(0.5)
    x0 = np.floor(x)
    y0 = np.floor(y)
    fx = (x - x0)[..., None]
    fy = (y - y0)[..., None]
    i0 = np.clip(x0.astype(np.int64), 0, n - 1)
    i1 = np.clip(x0.astype(np.int64) + 1, 0, n - 1)
    j0 = np.clip(y0.astype(np.int64), 0, n - 1)
    j1 = np.clip(y0.astype(np.int64) + 1, 0, n - 1)
    row0 = (face * n + j0) * n
    row1 = (face * n + j1) * n
    one = T(1.0)
    top = flat[row0 + i0] * (one - fx) + flat[row0 + i1] * fx
    bot = flat[row1 + i0] * (one - fx) + flat[row1 + i1] * fx
    return top * (one - fy) + bot * fy


def edge_neighbour(n: int, face, i, j):
    """The texel an edge tap stands for (include/mirhi.h "The sampler", seamless cubes): tap (i, j) of `face` at a level of n x n texels, exactly
    one of i, j outside [0, n - 1].  By projection, with no table of neighbours: the face plane is extended to the tap's centre ((i + 1/2) / n,
    (j + 1/2) / n), that point's direction (GetCubemapDirection's table with |u| or |v| > 1) goes through the face selection, and the texel is
    (floor(s' n), floor(t' n)) clamped to [0, n - 1].  Always in float64, whatever the dtype of the lookup: s' n stays 1 / (n + 1) away from an
    integer, which float64 resolves for every n up to 4096 and float32 would not -- and a float32 run of the model has to read the same texels.
    Returns (face', i', j')."""
    i = np.asarray(i, dtype=np.int64)
    j = np.asarray(j, dtype=np.int64)
    uv = np.stack([(i.astype(np.float64) + 0.5) / float(n), (j.astype(np.float64) + 0.5) / float(n)], axis=-1)
    f2, s2, t2 = select_face(cube_direction(face, uv, np.float64), np.float64)
    i2 = np.clip(np.floor(s2 * float(n)).astype(np.int64), 0, n - 1)
    j2 = np.clip(np.floor(t2 * float(n)).astype(np.int64), 0, n - 1)
    return f2, i2, j2


def seamless_taps(n: int, face, s, t, dtype=np.float64):
    """The four taps of a seamless lookup: texel indices into the flattened level [6 n n] (order (i0, j0), (i0 + 1, j0), (i0, j0 + 1),
    (i0 + 1, j0 + 1)), a bool per tap "corner tap" (both indices outside: no texel, index of the clamped texel as a placeholder), a bool per tap
    "edge tap", and the fractions fx, fy."""
    T = np.dtype(dtype).type
    x = np.asarray(s * T(n) - T(0.5))
    y = np.asarray(t * T(n) - T(0.5))
    face = np.broadcast_to(np.asarray(face), x.shape)
    x0 = np.floor(x)
    y0 = np.floor(y)
    fx = x - x0
    fy = y - y0
    i0 = x0.astype(np.int64)
    j0 = y0.astype(np.int64)
    idx, corner, edge = [], [], []
    for dj in (0, 1):
        for di in (0, 1):
            i, j = i0 + di, j0 + dj
            ox = (i < 0) | (i > n - 1)
            oy = (j < 0) | (j > n - 1)
            ic, jc = np.clip(i, 0, n - 1), np.clip(j, 0, n - 1)
            is_edge = ox ^ oy
            # (an in-face tap is its texel; a corner tap gets the clamped texel as a placeholder and is replaced by the mean of the other three)
            k = np.array((face * n + jc) * n + ic, dtype=np.int64)
            if is_edge.any():
                f2, i2, j2 = edge_neighbour(n, face[is_edge], i[is_edge], j[is_edge])
                k[is_edge] = (f2 * n + j2) * n + i2
            idx.append(k)
            corner.append(ox & oy)
            edge.append(is_edge)
    return idx, corner, edge, fx, fy


def _bilinear_face_seamless(level, face, s, t, dtype):
    """Bilinear across faces (seamless_taps): the four unclamped taps, a corner tap = the mean of the other three ((a + b + c) / 3 in tap
    order), weighted by the fractions exactly as _bilinear_face does."""
    T = np.dtype(dtype).type
    n = level.shape[1]
    flat = level.reshape(-1, level.shape[-1])
    idx, corner, _, fx, fy = seamless_taps(n, face, s, t, dtype)
    v = [flat[k] for k in idx]
    for c in range(4):
        o = [v[k] for k in range(4) if k != c]
        v[c] = np.where(corner[c][..., None], ((o[0] + o[1]) + o[2]) / T(3.0), v[c])
    fx, fy = fx[..., None], fy[..., None]
    one = T(1.0)
    top = v[0] * (one - fx) + v[1] * fx
    bot = v[2] * (one - fx) + v[3] * fx
    return top * (one - fy) + bot * fy


def sample_cube(levels, d, lod=0.0, dtype=np.float64, seamless=False):
    """TextureCube.SampleLevel(LinearSampler, d, lod): lod clamped to [0, levels - 1], the levels floor(lod) and floor(lod) + 1
    (clamped) each filtered bilinearly in the selected face and lerped by the fraction.  seamless: the cube's seamless state
    (mirhi_image_set_cube_seamless) -- each level is filtered across face edges and corners instead (_bilinear_face_seamless); level
    selection and the lerp between levels are the same."""
    T = np.dtype(dtype).type
    levels = [np.asarray(l, dtype=dtype) for l in levels]
    d = np.asarray(d, dtype=dtype)
    face, s, t = select_face(d, dtype)
    bilinear = _bilinear_face_seamless if seamless else _bilinear_face
    if len(levels) == 1:                     # lod clamps to 0: the one level, weight exactly 1
        return bilinear(levels[0], face, s, t, dtype)
    lod = np.clip(np.broadcast_to(np.asarray(lod, dtype=dtype), s.shape), T(0.0), T(len(levels) - 1))
    l0 = np.floor(lod)
    f = (lod - l0)[..., None]
    l0 = l0.astype(np.int64)
    l1 = np.minimum(l0 + 1, len(levels) - 1)
    out = np.zeros(s.shape + (levels[0].shape[-1],), dtype=dtype)
    for k in range(len(levels)):
        use0 = l0 == k
        use1 = (l1 == k) & (f[..., 0] > 0)
        need = use0 | use1
        if not need.any():
            continue
        c = bilinear(levels[k], face[need], s[need], t[need], dtype)
        w = np.where(use0[need][..., None], T(1.0) - f[need], T(0.0)) + np.where((l1 == k)[need][..., None], f[need], T(0.0))
        # (l0 == l1 at the last level: the two weights add up to 1 there, as lerp(a, a, f) does up to rounding)
        out[need] += c * w
    return out


def direction_to_equirect_uv(d, dtype=np.float64):
    """DirectionToEquirectUV (equirect_to_cubemap.hlsl:59-75)."""
    T = np.dtype(dtype).type
    pi = T(PI)
    phi = np.arctan2(d[..., 2], d[..., 0])
    theta = np.arcsin(np.clip(d[..., 1], T(-1.0), T(1.0)))
    u = (phi + pi) / (T(2.0) * pi)
    v = (theta + pi * T(0.5)) / pi
    return np.stack([u, v], axis=-1)


def equirect_direction(uv, dtype=np.float64):
    """Inverse of direction_to_equirect_uv: what direction an equirectangular pixel centre stands for."""
    T = np.dtype(dtype).type
    uv = np.asarray(uv, dtype=dtype)
    phi = uv[..., 0] * (T(2.0) * T(PI)) - T(PI)
    theta = uv[..., 1] * T(PI) - T(PI) * T(0.5)
    return np.stack([np.cos(theta) * np.cos(phi), np.sin(theta), np.cos(theta) * np.sin(phi)], axis=-1)


def sample_equirect(src, uv, dtype=np.float64):
    """Texture2D.SampleLevel(LinearSampler, uv, 0) on the equirectangular source [H, W, C]: bilinear, u repeats, v clamps."""
    T = np.dtype(dtype).type
    src = np.asarray(src, dtype=dtype)
    h, w = src.shape[:2]
    flat = src.reshape(h * w, src.shape[-1])
    uv = np.asarray(uv, dtype=dtype)
    x = uv[..., 0] * T(w) - T(0.5)
    y = uv[..., 1] * T(h) - T(0.5)
    x0 = np.floor(x)
    y0 = np.floor(y)
    fx = (x - x0)[..., None]
    fy = (y - y0)[..., None]
    i0 = np.mod(x0.astype(np.int64), w)
    i1 = np.mod(x0.astype(np.int64) + 1, w)
    j0 = np.clip(y0.astype(np.int64), 0, h - 1)
    j1 = np.clip(y0.astype(np.int64) + 1, 0, h - 1)
    one = T(1.0)
    top = flat[j0 * w + i0] * (one - fx) + flat[j0 * w + i1] * fx
    bot = flat[j1 * w + i0] * (one - fx) + flat[j1 * w + i1] * fx
    return top * (one - fy) + bot * fy


# ---- the passes ---------------------------------------------------------------------------------------------------------------
def equirect_to_cube(src, size: int, dtype=np.float64):
    """equirect_to_cubemap.hlsl:78-105: level 0 of a size^2 cube, all channels."""
    d = texel_directions(size, dtype)
    return sample_equirect(src, direction_to_equirect_uv(d, dtype), dtype)


def cube_mips(level0, levels: int, dtype=np.float64):
    """mirhi_ibl_cube_generate_mips: each face by a 2 x 2 box filter, ((a + b) + (c + d)) * 0.25."""
    T = np.dtype(dtype).type
    out = [np.asarray(level0, dtype=dtype)]
    for _ in range(1, levels):
        p = out[-1]
        a, b = p[:, 0::2, 0::2], p[:, 0::2, 1::2]
        c, d = p[:, 1::2, 0::2], p[:, 1::2, 1::2]
        out.append(((a + b) + (c + d)) * T(0.25))
    return out


def irradiance_angles():
    """The phi and theta values of irradiance_map.hlsl:101-103 as its float32 loops produce them (the loop variable is
    accumulated in float32 and compared with the float32 bound): 252 phi and 63 theta steps."""
    delta = np.float32(SAMPLE_DELTA)

    def steps(limit):
        vals, a = [], np.float32(0.0)
        while a < limit:
            vals.append(a)
            a = np.float32(a + delta)
        return np.array(vals, dtype=np.float32)
    return steps(np.float32(2.0) * np.float32(PI)), steps(np.float32(0.5) * np.float32(PI))


def _serial_add(acc, terms):
    """acc + terms[:, 0] + terms[:, 1] + ... in that order, in the arrays' dtype (cumsum adds sequentially)."""
    return np.cumsum(np.concatenate([acc[:, None], terms], axis=1), axis=1)[:, -1]


def irradiance(env_levels, size: int, dtype=np.float64, seamless=False):
    """irradiance_map.hlsl:63-143: [6, size, size, 4] = (rgb, 1); lookups at level 0 of env (seamless: env's seamless state)."""
    T = np.dtype(dtype).type
    env0 = [np.asarray(env_levels[0], dtype=dtype)[..., :3]]
    N = texel_directions(size, dtype).reshape(-1, 3)
    up = np.where((np.abs(N[:, 1]) < T(0.999))[:, None], np.array([0.0, 1.0, 0.0], dtype=dtype), np.array([1.0, 0.0, 0.0], dtype=dtype))
    right = _normalize(_cross(up, N))
    up = _normalize(_cross(N, right))
    phis, thetas = irradiance_angles()
    phis, thetas = phis.astype(dtype), thetas.astype(dtype)
    sin_t, cos_t = np.sin(thetas), np.cos(thetas)
    acc = np.zeros((N.shape[0], 3), dtype=dtype)
    for phi in phis:
        tx = sin_t * np.cos(phi)
        ty = sin_t * np.sin(phi)
        vec = tx[None, :, None] * right[:, None, :] + ty[None, :, None] * up[:, None, :] + cos_t[None, :, None] * N[:, None, :]
        col = sample_cube(env0, vec, 0.0, dtype, seamless)
        acc = _serial_add(acc, col * cos_t[None, :, None] * sin_t[None, :, None])
    count = T(len(phis) * len(thetas))
    out = np.ones((N.shape[0], 4), dtype=dtype)
    out[:, :3] = T(PI) * acc / count
    return out.reshape(6, size, size, 4)


def radical_inverse(i, dtype=np.float64):
    """RadicalInverse_VdC (prefilter_map.hlsl:31-39)."""
    bits = np.asarray(i, dtype=np.uint32)
    bits = (bits << np.uint32(16)) | (bits >> np.uint32(16))
    bits = ((bits & np.uint32(0x55555555)) << np.uint32(1)) | ((bits & np.uint32(0xAAAAAAAA)) >> np.uint32(1))
    bits = ((bits & np.uint32(0x33333333)) << np.uint32(2)) | ((bits & np.uint32(0xCCCCCCCC)) >> np.uint32(2))
    bits = ((bits & np.uint32(0x0F0F0F0F)) << np.uint32(4)) | ((bits & np.uint32(0xF0F0F0F0)) >> np.uint32(4))
    bits = ((bits & np.uint32(0x00FF00FF)) << np.uint32(8)) | ((bits & np.uint32(0xFF00FF00)) >> np.uint32(8))
    return bits.astype(dtype) * np.dtype(dtype).type(2.3283064365386963e-10)


def hammersley(count: int, dtype=np.float64):
    i = np.arange(count, dtype=np.uint32)
    return i.astype(dtype) / np.dtype(dtype).type(count), radical_inverse(i, dtype)


def importance_sample_ggx(xi_x, xi_y, N, roughness, dtype=np.float64):
    """ImportanceSampleGGX (prefilter_map.hlsl:54-81): xi [S], N [T, 3] -> H [T, S, 3] in world space."""
    T = np.dtype(dtype).type
    a = roughness * roughness
    phi = T(2.0) * T(PI) * xi_x
    cos_t = np.sqrt((T(1.0) - xi_y) / (T(1.0) + (a * a - T(1.0)) * xi_y))
    sin_t = np.sqrt(T(1.0) - cos_t * cos_t)
    hx, hy, hz = np.cos(phi) * sin_t, np.sin(phi) * sin_t, cos_t
    up = np.where((np.abs(N[:, 2]) < T(0.999))[:, None], np.array([0.0, 0.0, 1.0], dtype=dtype), np.array([1.0, 0.0, 0.0], dtype=dtype))
    tangent = _normalize(_cross(up, N))
    bitangent = _cross(N, tangent)
    vec = tangent[:, None, :] * hx[..., None] + bitangent[:, None, :] * hy[..., None] + N[:, None, :] * hz[..., None]
    return _normalize(vec)


def _prefilter_level(env_rgb, m: int, roughness, sample_count: int, dtype, seamless=False):
    T = np.dtype(dtype).type
    R = texel_directions(m, dtype).reshape(-1, 3)
    out = np.ones((R.shape[0], 4), dtype=dtype)
    if roughness < T(0.01):                                # prefilter_map.hlsl:168-173
        out[:, :3] = sample_cube(env_rgb, R, 0.0, dtype, seamless)
        return out.reshape(6, m, m, 4)
    xs, ys = hammersley(sample_count, dtype)
    acc = np.zeros((R.shape[0], 3), dtype=dtype)
    wsum = np.zeros(R.shape[0], dtype=dtype)
    chunk = max(1, 400000 // R.shape[0])
    a = roughness * roughness
    a2 = a * a
    sa_texel = T(4.0) * T(PI) / (T(6.0) * T(PREFILTER_RESOLUTION) * T(PREFILTER_RESOLUTION))
    for s0 in range(0, sample_count, chunk):
        H = importance_sample_ggx(xs[None, s0:s0 + chunk], ys[None, s0:s0 + chunk], R, roughness, dtype)
        V = R[:, None, :]
        L = _normalize(T(2.0) * _dot(V, H)[..., None] * H - V)
        ndl = _dot(V, L)
        ndh = np.maximum(_dot(V, H), T(0.0))
        hdv = ndh
        denom = ndh * ndh * (a2 - T(1.0)) + T(1.0)
        denom = T(PI) * denom * denom
        D = a2 / np.maximum(denom, T(0.0001))
        with np.errstate(divide="ignore", invalid="ignore"):
            pdf = (D * ndh) / (T(4.0) * hdv) + T(0.0001)
            sa_sample = T(1.0) / (T(sample_count) * pdf + T(0.0001))
            mip = np.maximum(T(0.0), T(0.5) * np.log2(sa_sample / sa_texel))
        keep = ndl > 0
        mip = np.where(keep, mip, T(0.0))
        col = sample_cube(env_rgb, L, mip, dtype, seamless)
        w = np.where(keep, ndl, T(0.0))
        acc = _serial_add(acc, col * w[..., None])
        wsum = _serial_add(wsum, w)
    ok = wsum > 0
    out[:, :3] = np.where(ok[:, None], acc / np.where(ok, wsum, T(1.0))[:, None], acc)
    return out.reshape(6, m, m, 4)


def prefilter(env_levels, size: int, levels: int, sample_count: int = 1024, dtype=np.float64, seamless=False):
    """prefilter_map.hlsl:134-229 run once per level: MipSize = size >> l, Roughness = l / (levels - 1) (0 for one level); the
    lookups use the whole chain of env (trilinear at mipLevel; seamless: env's seamless state).  Returns the list of levels, each (rgb, 1)."""
    T = np.dtype(dtype).type
    env_rgb = [np.asarray(l, dtype=dtype)[..., :3] for l in env_levels]
    out = []
    for l in range(levels):
        rough = T(l) / T(levels - 1) if levels > 1 else T(0.0)
        out.append(_prefilter_level(env_rgb, size >> l, rough, sample_count, dtype, seamless))
    return out


def _g_schlick_ggx(ndx, roughness, T):
    k = (roughness * roughness) / T(2.0)
    return ndx / np.maximum(ndx * (T(1.0) - k) + k, T(0.0001))


def brdf_lut(size: int, dtype=np.float64):
    """brdf_lut.hlsl:116-206: [size, size, 4] = (A, B, 0, 1); column = NdotV, row = roughness.  Float storage: the reference's
    rg16f rounding is not applied."""
    T = np.dtype(dtype).type
    c = (np.arange(size, dtype=dtype) + T(0.5)) / T(size)
    ndv = np.broadcast_to(np.maximum(c, T(0.001))[None, :], (size, size)).reshape(-1)
    rough = np.broadcast_to(c[:, None], (size, size)).reshape(-1)
    V = np.stack([np.sqrt(T(1.0) - ndv * ndv), np.zeros_like(ndv), ndv], axis=-1)
    N = np.zeros_like(V)
    N[:, 2] = T(1.0)
    xs, ys = hammersley(LUT_SAMPLES, dtype)
    A = np.zeros_like(ndv)
    B = np.zeros_like(ndv)
    for i in range(LUT_SAMPLES):
        H = importance_sample_ggx(xs[i:i + 1][None, :], ys[i:i + 1][None, :], N, rough[:, None], dtype)[:, 0, :]
        vdh_raw = _dot(V, H)
        L = _normalize(T(2.0) * vdh_raw[:, None] * H - V)
        ndl = np.maximum(L[:, 2], T(0.0))
        ndh = np.maximum(H[:, 2], T(0.0))
        vdh = np.maximum(vdh_raw, T(0.0))
        G = _g_schlick_ggx(ndl, rough, T) * _g_schlick_ggx(np.maximum(V[:, 2], T(0.0)), rough, T)
        g_vis = (G * vdh) / np.maximum(ndh * ndv, T(0.0001))
        fc = np.power(T(1.0) - vdh, T(5.0))
        keep = ndl > 0
        A = A + np.where(keep, (T(1.0) - fc) * g_vis, T(0.0))
        B = B + np.where(keep, fc * g_vis, T(0.0))
    out = np.zeros((size * size, 4), dtype=dtype)
    out[:, 0] = A / T(LUT_SAMPLES)
    out[:, 1] = B / T(LUT_SAMPLES)
    out[:, 3] = T(1.0)
    return out.reshape(size, size, 4)


# ---- the consumer: the ambient term of pixel/model_pbr_ibl.hlsl:355-384 (MIRHI_PROGRAM_MODEL_PBR_IBL, include/mirhi.h mirhi_cmd_bind_ibl) --------
MAX_REFLECTION_LOD = 7.0    # pbr.hlsli:373, hard-coded there
MIN_ROUGHNESS = 0.04        # ClampRoughness, pbr.hlsli:476-479


def sample_lut(lut, u, v, dtype=np.float64):
    """brdfLUT.Sample(LinearSampler, float2(u, v)) on the square image [n, n, C]: bilinear at level 0, clamp to edge on both axes -- the
    filter of one cube face (u along a row, v down the rows)."""
    lut = np.asarray(lut, dtype=dtype)
    u = np.asarray(u, dtype=dtype)
    v = np.broadcast_to(np.asarray(v, dtype=dtype), u.shape)
    return _bilinear_face(lut[None], np.zeros(u.shape, dtype=np.int64), u, v, dtype)


def fresnel_schlick_roughness(cos_theta, F0, roughness, dtype=np.float64):
    """FresnelSchlickRoughness (pbr.hlsli:147-152): cos_theta [...], F0 [..., 3], roughness [...] -> [..., 3]."""
    T = np.dtype(dtype).type
    ct = np.clip(np.asarray(cos_theta, dtype=dtype), T(0.0), T(1.0))
    F0 = np.asarray(F0, dtype=dtype)
    F90 = np.maximum((T(1.0) - np.asarray(roughness, dtype=dtype))[..., None], F0)
    o = T(1.0) - ct
    return F0 + (F90 - F0) * (o * o * o * o * o)[..., None]


def reflect(V, N):
    """reflect(-V, N) = 2 dot(N, V) N - V (model_pbr_ibl.hlsl:259)."""
    return np.asarray(2.0, dtype=N.dtype) * _dot(N, V)[..., None] * N - V


def ambient(irradiance_levels, prefiltered_levels, lut, N, V, albedo, metallic, roughness, ao, dtype=np.float64, irradiance_seamless=False, prefiltered_seamless=False):
    """model_pbr_ibl.hlsl:355-384: (kD * irradiance * albedo + prefiltered * (F0 * brdf.x + brdf.y)) * ao for unit vectors N, V [..., 3],
    albedo [..., 3] and metallic, roughness, ao [...]; `roughness` is the material's, ClampRoughness (:262) is applied here.  The cubes
    are lists of levels [6, n, n, C >= 3] (level 0 of the irradiance cube is the one sampled), lut [n, n, C >= 2].  Each cube carries its
    own seamless state (mirhi_cmd_bind_ibl latches both); the LUT is 2-D and has none."""
    T = np.dtype(dtype).type
    N, V, albedo = (np.asarray(a, dtype=dtype) for a in (N, V, albedo))
    metallic, ao = (np.broadcast_to(np.asarray(a, dtype=dtype), N.shape[:-1]) for a in (metallic, ao))
    rough = np.maximum(np.broadcast_to(np.asarray(roughness, dtype=dtype), N.shape[:-1]), T(MIN_ROUGHNESS))
    F0 = T(0.04) + (albedo - T(0.04)) * metallic[..., None]                                    # :356
    ndv = np.maximum(_dot(N, V), T(0.0))                                                        # :359
    F = fresnel_schlick_roughness(ndv, F0, rough, dtype)                                        # :362
    kD = (T(1.0) - F) * (T(1.0) - metallic)[..., None]                                          # :365-366
    irr = sample_cube([np.asarray(irradiance_levels[0], dtype=dtype)[..., :3]], N, 0.0, dtype, irradiance_seamless)  # :369
    pre = sample_cube([np.asarray(l, dtype=dtype)[..., :3] for l in prefiltered_levels], reflect(V, N), rough * T(MAX_REFLECTION_LOD), dtype, prefiltered_seamless)   # :373-377
    brdf = sample_lut(np.asarray(lut, dtype=dtype)[..., :2], ndv, rough, dtype)                 # :380
    spec = pre * (F0 * brdf[..., 0:1] + brdf[..., 1:2])                                         # :381
    return (kD * (irr * albedo) + spec) * ao[..., None]                                         # :370, :384


def tie_mask(d, rel=1e-4):
    """True where the two largest |components| of d [..., 3] are within `rel` of each other (relative to the largest): the cube lookup may
    select either face there, and the stated sampler is not seamless."""
    a = np.sort(np.abs(np.asarray(d, dtype=np.float64)), axis=-1)
    return (a[..., 2] - a[..., 1]) <= rel * a[..., 2]



# ---- SKYBOX (vertex/skybox.hlsl + pixel/skybox.hlsl; include/mirhi.h "SKYBOX") -----------------------------------------------------
SKY_CLIP = ((-1.0, -1.0), (3.0, -1.0), (-1.0, 3.0))      # vertex/skybox.hlsl:20-24, SV_VertexID 0, 1, 2


def skybox_local_pos(inv_view_proj, viewport, width: int, height: int, dtype=np.float64):
    """LocalPos at every pixel centre, [height, width, 3], as the shaders compute it: at each of the three vertices w = M (x, -y, 1, 1) and
    LocalPos = w.xyz / w.w (vertex/skybox.hlsl:40-42), then the affine interpolation of the three vertex values over the viewport
    (x, y, width, height, ...): all clip w are 1.  inv_view_proj: [col, row] (4, 4) or the 16 floats in memory order (the convention of
    CameraData.viewProjection)."""
    T = np.dtype(dtype).type
    M = np.asarray(inv_view_proj, dtype=dtype).reshape(4, 4).T        # maths matrix
    L = []
    for x, y in SKY_CLIP:
        w = M @ np.array([x, -y, 1.0, 1.0], dtype=dtype)
        L.append(w[:3] / w[3])
    vx, vy, vw, vh = (T(v) for v in viewport[:4])
    hw, hh = vw * T(0.5), vh * T(0.5)
    xn = ((np.arange(width, dtype=dtype) + T(0.5)) - (vx + hw)) / hw
    yn = ((np.arange(height, dtype=dtype) + T(0.5)) - (vy + hh)) / hh
    a = ((xn + T(1.0)) * T(0.25))[None, :, None]
    b = ((yn + T(1.0)) * T(0.25))[:, None, None]
    return (L[0] + (L[1] - L[0]) * a + (L[2] - L[0]) * b).astype(dtype)


def skybox_directions(inv_view_proj, viewport, width: int, height: int, dtype=np.float64):
    """normalize(LocalPos) per pixel (pixel/skybox.hlsl:24): [height, width, 3]."""
    return _normalize(skybox_local_pos(inv_view_proj, viewport, width, height, dtype)).astype(dtype)


def skybox(levels, inv_view_proj, viewport, width: int, height: int, dtype=np.float64, seamless=False):
    """The sky frame [height, width, 4]: the cube lookup at lod 0 along skybox_directions (the stated deviation: `Sample` without derivatives)."""
    return sample_cube(levels[:1], skybox_directions(inv_view_proj, viewport, width, height, dtype), 0.0, dtype, seamless)


def skybox_coverage(viewport, scissor, width: int, height: int, cull_mode: int = 0, front_face: int = 0):
    """Pixels the sky triangle covers, bool [height, width]: the three vertices through the viewport in float32, snapped to 1 / 256 pixel,
    culled under the geometry kernel's winding rule (front_face 0 = counter-clockwise: front <=> S < 0), integer edge functions at the pixel
    centres with the top-left rule, cut by the scissor (x, y, width, height; None = the frame)."""
    f = np.float32
    vx, vy, vw, vh = (f(v) for v in viewport[:4])
    hw, hh = f(0.5) * vw, f(0.5) * vh
    cx, cy = vx + hw, vy + hh
    X = [int(np.rint(f(f(f(x) * hw + cx) * f(256.0)))) for x, _ in SKY_CLIP]
    Y = [int(np.rint(f(f(f(y) * hh + cy) * f(256.0)))) for _, y in SKY_CLIP]
    S = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
    front = S < 0 if front_face == 0 else S > 0
    out = np.zeros((height, width), dtype=bool)
    if S == 0 or cull_mode == 3 or (cull_mode == 2 and not front) or (cull_mode == 1 and front):
        return out
    if S < 0:
        X[1], X[2], Y[1], Y[2] = X[2], X[1], Y[2], Y[1]
    px = 256 * np.arange(width, dtype=np.int64)[None, :] + 128
    py = 256 * np.arange(height, dtype=np.int64)[:, None] + 128
    inside = np.ones((height, width), dtype=bool)
    for i in range(3):
        j = (i + 1) % 3
        dx, dy = X[j] - X[i], Y[j] - Y[i]
        bias = 0 if (dy < 0 or (dy == 0 and dx > 0)) else -1
        inside &= (-dy * (px - X[i]) + dx * (py - Y[i]) + bias) >= 0
    if scissor is not None:
        sx, sy, sw, sh = scissor
        cut = np.zeros_like(inside)
        cut[max(sy, 0):max(sy + sh, 0), max(sx, 0):max(sx + sw, 0)] = True
        inside &= cut
    return inside


# ---- test environment ---------------------------------------------------------------------------------------------------------
LOBE_AXIS = (0.48, 0.64, 0.6)      # unit vector
LOBE_PEAK = 20.0
LOBE_SHARPNESS = 6.0               # exp(-k (1 - cos)): falls to half its peak 27 degrees off axis


def analytic_radiance(d, dtype=np.float64):
    """A smooth HDR function of direction: a low-order polynomial in the components plus one broad Gaussian lobe of peak 20.
    d [..., 3] unit vectors -> [..., 4] (rgb, 1); positive everywhere."""
    T = np.dtype(dtype).type
    d = np.asarray(d, dtype=dtype)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    lobe = T(LOBE_PEAK) * np.exp(-T(LOBE_SHARPNESS) * (T(1.0) - (x * T(LOBE_AXIS[0]) + y * T(LOBE_AXIS[1]) + z * T(LOBE_AXIS[2]))))
    r = T(1.0) + T(0.5) * x + T(0.25) * y * y + lobe
    g = T(0.8) + T(0.4) * y + T(0.2) * x * z + T(0.8) * lobe
    b = T(0.6) - T(0.3) * z + T(0.2) * x * x + T(0.5) * lobe
    return np.stack([r, g, b, np.ones_like(r)], axis=-1)


def analytic_environment(size: int, dtype=np.float64):
    """analytic_radiance at the texel centres of a size^2 cube: level 0, [6, size, size, 4]."""
    return analytic_radiance(texel_directions(size, dtype), dtype)


def analytic_equirect(width: int, height: int, dtype=np.float64):
    """analytic_radiance at the pixel centres of a width x height equirectangular image: [height, width, 4]."""
    T = np.dtype(dtype).type
    u = (np.arange(width, dtype=dtype) + T(0.5)) / T(width)
    v = (np.arange(height, dtype=dtype) + T(0.5)) / T(height)
    uv = np.stack(np.broadcast_arrays(u[None, :], v[:, None]), axis=-1)
    return analytic_radiance(equirect_direction(uv, dtype), dtype)
