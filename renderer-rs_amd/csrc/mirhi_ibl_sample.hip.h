// Cube and 2-D lookups of the IBL images (include/mirhi.h, "The sampler"): layout of a cube chain, face selection, bilinear filtering inside a face,
// the trilinear cube lookup.  Shared by the precompute kernels (mirhi_ibl.hip.h, in mirhi_api.hip's unit) and the MODEL_PBR_IBL fragment program
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
