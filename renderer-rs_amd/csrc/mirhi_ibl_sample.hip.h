// Cube and 2-D lookups of the IBL images (include/mirhi.h, "The sampler"): layout of a cube chain, face selection, bilinear filtering inside a face,
// the trilinear cube lookup, and the seamless form of both (a cube whose seamless state is on: DESIGN.md 8o).  Shared by the precompute kernels (mirhi_ibl.hip.h, in mirhi_api.hip's unit) and the MODEL_PBR_IBL fragment program
// (mirhi_shading.hip.h, in mirhi_kernels.hip's unit, inside namespace mirhi): one statement of the sampler for both.  Needs <hip/hip_runtime.h>.
//
// Every index that reaches memory is an integer clamped to [0, n - 1] after the float -> int conversion, so a NaN or infinite direction reads a valid texel.
#pragma once

struct IblCube { const float4* texels; uint32_t size, levels; };

__host__ __device__ inline uint32_t ibl_level_offset(uint32_t size, uint32_t level) {      // 6 * sum_{k < level} (size >> k)^2; size a power of two, size >> level >= 1
    const uint32_t m = size >> level;
    return 8u * (size * size - m * m);
}
__host__ __device__ inline uint32_t ibl_chain_texels(uint32_t size, uint32_t levels) {     // texels of a chain of `levels` >= 1 levels
    const uint32_t m = size >> (levels - 1u);
    return ibl_level_offset(size, levels - 1u) + 6u * m * m;
}

struct IblFaceUV { uint32_t face; float s, t; };
// the Vulkan specification's cube-map face selection (major axis = largest magnitude, ties prefer z, then y, then x): the inverse of GetCubemapDirection
__device__ inline IblFaceUV ibl_select_face(float x, float y, float z) {
    #pragma clang fp contract(fast)
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    IblFaceUV r; float sc, tc, ma;
    if (az >= ax && az >= ay) { r.face = z < 0.0f ? 5u : 4u; sc = z < 0.0f ? -x : x; tc = -y; ma = az; }
    else if (ay >= ax)        { r.face = y < 0.0f ? 3u : 2u; sc = x; tc = y < 0.0f ? -z : z; ma = ay; }
    else                      { r.face = x < 0.0f ? 1u : 0u; sc = x < 0.0f ? z : -z; tc = -y; ma = ax; }
    const float h = 0.5f * __builtin_amdgcn_rcpf(ma);
    r.s = sc * h + 0.5f; r.t = tc * h + 0.5f;
    return r;
}
__device__ inline float4 ibl_lerp4(float4 a, float4 b, float f) {
    #pragma clang fp contract(fast)
    return make_float4(a.x + (b.x - a.x) * f, a.y + (b.y - a.y) * f, a.z + (b.z - a.z) * f, a.w + (b.w - a.w) * f);
}
// bilinear inside one face of n x n texels, clamp to edge: x = s n - 1/2, floor, fraction, four clamped texels.  In two halves, so that a caller with
// several lookups (the MODEL_PBR_IBL fragment program: sixteen) can compute every address and issue every load before it filters the first one:
// ibl_bilinear_taps gives the four texel offsets within the face and the two fractions, ibl_bilinear_filter weighs the four texels.
struct IblTaps { uint32_t o00, o10, o01, o11; float fx, fy; };
__device__ inline IblTaps ibl_bilinear_taps(uint32_t n, float s, float t) {
    #pragma clang fp contract(fast)
    const float x = s * (float)n - 0.5f, y = t * (float)n - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    const int hi = (int)n - 1;
    const int i0 = min(max((int)x0, 0), hi), i1 = min(max((int)x0 + 1, 0), hi);
    const int j0 = min(max((int)y0, 0), hi), j1 = min(max((int)y0 + 1, 0), hi);
    IblTaps r;
    r.o00 = (uint32_t)j0 * n + (uint32_t)i0; r.o10 = (uint32_t)j0 * n + (uint32_t)i1;
    r.o01 = (uint32_t)j1 * n + (uint32_t)i0; r.o11 = (uint32_t)j1 * n + (uint32_t)i1;
    r.fx = x - x0; r.fy = y - y0;
    return r;
}
__device__ inline float4 ibl_bilinear_filter(const IblTaps& k, float4 a, float4 b, float4 c, float4 d) {
    return ibl_lerp4(ibl_lerp4(a, b, k.fx), ibl_lerp4(c, d, k.fx), k.fy);
}
__device__ inline float4 ibl_bilinear(const float4* __restrict__ face, uint32_t n, float s, float t) {
    const IblTaps k = ibl_bilinear_taps(n, s, t);
    return ibl_bilinear_filter(k, face[k.o00], face[k.o10], face[k.o01], face[k.o11]);
}
__device__ inline float4 ibl_sample_cube_level(const IblCube& c, uint32_t level, const IblFaceUV& f) {
    const uint32_t n = c.size >> level;
    return ibl_bilinear(c.texels + ibl_level_offset(c.size, level) + f.face * n * n, n, f.s, f.t);
}
// TextureCube.SampleLevel(LinearSampler, dir, lod): lod clamped to [0, levels - 1], levels floor(lod) and floor(lod) + 1 (clamped) lerped by the fraction
__device__ inline float4 ibl_sample_cube(const IblCube& c, float x, float y, float z, float lod) {
    const IblFaceUV f = ibl_select_face(x, y, z);
    lod = fminf(fmaxf(lod, 0.0f), (float)(c.levels - 1u));
    const float l0f = floorf(lod), frac = lod - l0f;
    const uint32_t l0 = min((uint32_t)(int)l0f, c.levels - 1u);
    float4 r = ibl_sample_cube_level(c, l0, f);
    if (frac > 0.0f) r = ibl_lerp4(r, ibl_sample_cube_level(c, min(l0 + 1u, c.levels - 1u), f), frac);
    return r;
}

// ---- seamless cube filtering (include/mirhi.h "The sampler"): the state of a cube image, mirhi_image_set_cube_seamless ---------------------
// The four taps (i0 + di, j0 + dj) are NOT clamped.  A tap with one index outside the face (-1 or n) is the texel across that edge: in the neighbour
// face's border row or column, at the same position along the shared edge.  A tap with both indices outside (at most one of the four) has no texel: its
// value is the mean of the other three.  Which face lies across which edge, and how the position along the edge maps, is a table of 24 six-bit entries,
// one word per face, selected by compares (no memory access ahead of the gathers):
//   bits 0-2  the neighbour face
//   bit  3    1: the position along the edge becomes the neighbour's column (its row is the border), 0: it becomes the row (the column is the border)
//   bit  4    1: the position runs the other way (n - 1 - p)
//   bit  5    1: the border is row / column n - 1, 0: row / column 0
// side 0: i = -1 (left), 1: i = n (right), 2: j = -1 (top), 3: j = n (bottom).  Derived from GetCubemapDirection's table (ibl_texel_direction); the
// float64 model (renderer-rs_amd/ibl.py) re-projects instead and shares nothing with this table -- mirhi_debug_cube_edge_tap lets a test compare the two.
#define IBL_EDGE(nf, col, flip, hi) ((uint32_t)(nf) | (uint32_t)(col) << 3 | (uint32_t)(flip) << 4 | (uint32_t)(hi) << 5)
#define IBL_EDGE_ROW(l, r, t, b) ((l) | (r) << 6 | (t) << 12 | (b) << 18)
__host__ __device__ inline uint32_t ibl_edge_row(uint32_t face) {
    const uint32_t r0 = IBL_EDGE_ROW(IBL_EDGE(4, 0, 0, 1), IBL_EDGE(5, 0, 0, 0), IBL_EDGE(2, 0, 1, 1), IBL_EDGE(3, 0, 0, 1));      // +X
    const uint32_t r1 = IBL_EDGE_ROW(IBL_EDGE(5, 0, 0, 1), IBL_EDGE(4, 0, 0, 0), IBL_EDGE(2, 0, 0, 0), IBL_EDGE(3, 0, 1, 0));      // -X
    const uint32_t r2 = IBL_EDGE_ROW(IBL_EDGE(1, 1, 0, 0), IBL_EDGE(0, 1, 1, 0), IBL_EDGE(5, 1, 1, 0), IBL_EDGE(4, 1, 0, 0));      // +Y
    const uint32_t r3 = IBL_EDGE_ROW(IBL_EDGE(1, 1, 1, 1), IBL_EDGE(0, 1, 0, 1), IBL_EDGE(4, 1, 0, 1), IBL_EDGE(5, 1, 1, 1));      // -Y
    const uint32_t r4 = IBL_EDGE_ROW(IBL_EDGE(1, 0, 0, 1), IBL_EDGE(0, 0, 0, 0), IBL_EDGE(2, 1, 0, 1), IBL_EDGE(3, 1, 0, 0));      // +Z
    const uint32_t r5 = IBL_EDGE_ROW(IBL_EDGE(0, 0, 0, 1), IBL_EDGE(1, 0, 0, 0), IBL_EDGE(2, 1, 1, 0), IBL_EDGE(3, 1, 1, 1));      // -Z
    return face == 0u ? r0 : (face == 1u ? r1 : (face == 2u ? r2 : (face == 3u ? r3 : (face == 4u ? r4 : r5))));
}
#undef IBL_EDGE
#undef IBL_EDGE_ROW
// One tap (i, j) of face `face` (row = ibl_edge_row(face)) of a level of n x n texels, seamless: its texel offset from the level's first texel (the
// face included), and whether it is a corner tap (then the offset is the clamped in-face texel: read, never used).  Whatever i and j hold, the
// offset is below 6 n^2: both are clamped, the neighbour face is one of six, and the position along the edge stays in [0, n - 1].
__host__ __device__ inline uint32_t ibl_seamless_tap(uint32_t n, uint32_t face, uint32_t row, int i, int j, bool on, bool& corner) {
    const int hi = (int)n - 1;
    const bool ox = on && (i < 0 || i > hi), oy = on && (j < 0 || j > hi);
    const uint32_t ic = (uint32_t)(i < 0 ? 0 : (i > hi ? hi : i)), jc = (uint32_t)(j < 0 ? 0 : (j > hi ? hi : j));
    uint32_t f = face, ii = ic, jj = jc;
    if (ox != oy) {      // an edge tap
        const uint32_t side = ox ? (i < 0 ? 0u : 1u) : (j < 0 ? 2u : 3u);
        const uint32_t e = (row >> (6u * side)) & 63u;
        const uint32_t p = ox ? jc : ic;
        const uint32_t q = (e & 16u) ? (uint32_t)hi - p : p, c = (e & 32u) ? (uint32_t)hi : 0u;
        f = e & 7u; ii = (e & 8u) ? q : c; jj = (e & 8u) ? c : q;
    }
    corner = ox && oy;
    return (f * n + jj) * n + ii;
}
// The two halves of the seamless lookup, as ibl_bilinear_taps / ibl_bilinear_filter are of the clamped one: offsets from the LEVEL's first texel, the
// fractions, and which of the four taps is the corner tap (4: none).  on = false (a cube whose own state is off, in a scope whose other cube's is
// on): the clamped sampler's texels and arithmetic.
struct IblSeamTaps { uint32_t o00, o10, o01, o11; float fx, fy; uint32_t corner; };
__device__ inline IblSeamTaps ibl_seamless_taps(uint32_t n, uint32_t face, float s, float t, bool on) {
    #pragma clang fp contract(fast)
    const float x = s * (float)n - 0.5f, y = t * (float)n - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    const int hi = (int)n - 1;
    const int i0 = min(max((int)x0, -1), hi), j0 = min(max((int)y0, -1), hi);      // (clamped after the conversion: NaN and infinities read valid texels)
    const uint32_t row = ibl_edge_row(face);
    bool c00, c10, c01, c11;
    IblSeamTaps r;
    r.o00 = ibl_seamless_tap(n, face, row, i0, j0, on, c00); r.o10 = ibl_seamless_tap(n, face, row, i0 + 1, j0, on, c10);
    r.o01 = ibl_seamless_tap(n, face, row, i0, j0 + 1, on, c01); r.o11 = ibl_seamless_tap(n, face, row, i0 + 1, j0 + 1, on, c11);
    r.corner = c00 ? 0u : (c10 ? 1u : (c01 ? 2u : (c11 ? 3u : 4u)));
    r.fx = x - x0; r.fy = y - y0;
    return r;
}
__device__ inline float4 ibl_mean3(float4 a, float4 b, float4 c) {
    return make_float4(((a.x + b.x) + c.x) / 3.0f, ((a.y + b.y) + c.y) / 3.0f, ((a.z + b.z) + c.z) / 3.0f, ((a.w + b.w) + c.w) / 3.0f);
}
__device__ inline float4 ibl_seamless_filter(const IblSeamTaps& k, float4 a, float4 b, float4 c, float4 d) {
    if (k.corner == 0u) a = ibl_mean3(b, c, d);
    else if (k.corner == 1u) b = ibl_mean3(a, c, d);
    else if (k.corner == 2u) c = ibl_mean3(a, b, d);
    else if (k.corner == 3u) d = ibl_mean3(a, b, c);
    return ibl_lerp4(ibl_lerp4(a, b, k.fx), ibl_lerp4(c, d, k.fx), k.fy);
}
__device__ inline float4 ibl_sample_cube_level_seamless(const IblCube& c, uint32_t level, const IblFaceUV& f) {
    const uint32_t n = c.size >> level;
    const float4* const base = c.texels + ibl_level_offset(c.size, level);
    const IblSeamTaps k = ibl_seamless_taps(n, f.face, f.s, f.t, true);
    return ibl_seamless_filter(k, base[k.o00], base[k.o10], base[k.o01], base[k.o11]);
}
// ibl_sample_cube of a seamless cube: level selection and the lerp between levels are the clamped lookup's
__device__ inline float4 ibl_sample_cube_seamless(const IblCube& c, float x, float y, float z, float lod) {
    const IblFaceUV f = ibl_select_face(x, y, z);
    lod = fminf(fmaxf(lod, 0.0f), (float)(c.levels - 1u));
    const float l0f = floorf(lod), frac = lod - l0f;
    const uint32_t l0 = min((uint32_t)(int)l0f, c.levels - 1u);
    float4 r = ibl_sample_cube_level_seamless(c, l0, f);
    if (frac > 0.0f) r = ibl_lerp4(r, ibl_sample_cube_level_seamless(c, min(l0 + 1u, c.levels - 1u), f), frac);
    return r;
}
template <bool SEAMLESS>
__device__ inline float4 ibl_sample_cube_as(const IblCube& c, float x, float y, float z, float lod) {
    if constexpr (SEAMLESS) return ibl_sample_cube_seamless(c, x, y, z, lod);
    else return ibl_sample_cube(c, x, y, z, lod);
}
