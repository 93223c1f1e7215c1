// IBL precompute (include/mirhi.h "IBL precompute"): the reference's four compute shaders, shaders/hlsl/compute/
// {equirect_to_cubemap, irradiance_map, prefilter_map, brdf_lut}.hlsl, as gfx950 kernels, plus the cube mip chain the prefilter samples.
//
// Numeric policy: these passes are NOT on the bit-exact oracle path (there is no oracle for them; the float64 numpy model of
// renderer-rs_amd/ibl.py is the yardstick and the tests bound the error).  So, unlike the rest of the build, the kernels here contract
// (a local fp contract pragma per function; the global -ffp-contract=off stays), use the hardware's v_rcp / v_rsq / v_sqrt / v_log, and
// sum in another order than the shaders' serial loops.  The sample tables are built with the precise sinf / cosf: they are computed once
// per workgroup and cost nothing beside the lookups.  cube_mip_kernel is three exact operations in a fixed order and is bit-exact.
//
// Shapes: a cube is level-major, face-major, row-major float4 texels (ibl_level_offset).  Every index that reaches memory is an integer
// clamped to [0, n - 1] after the float -> int conversion, so a NaN or infinite direction reads a valid texel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define IBL_PI 3.14159265359f          // the shaders' #define PI

#include "mirhi_ibl_sample.hip.h"      // IblCube, ibl_level_offset, ibl_select_face, ibl_bilinear, ibl_sample_cube

// GetCubemapDirection (equirect_to_cubemap.hlsl:22-56) at the centre of texel (px, py) of an n x n face
__device__ inline float3 ibl_texel_direction(uint32_t face, uint32_t px, uint32_t py, uint32_t n) {
    #pragma clang fp contract(fast)
    const float u = ((float)px + 0.5f) / (float)n * 2.0f - 1.0f, v = ((float)py + 0.5f) / (float)n * 2.0f - 1.0f;
    float3 d;
    switch (face) {
        case 0: d = make_float3(1.0f, -v, -u); break;
        case 1: d = make_float3(-1.0f, -v, u); break;
        case 2: d = make_float3(u, 1.0f, v); break;
        case 3: d = make_float3(u, -1.0f, -v); break;
        case 4: d = make_float3(u, -v, 1.0f); break;
        default: d = make_float3(-u, -v, -1.0f); break;
    }
    const float inv = 1.0f / sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);       // (once per texel: the exact division)
    return make_float3(d.x * inv, d.y * inv, d.z * inv);
}
__device__ inline float3 ibl_cross(float3 a, float3 b) {
    return make_float3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ inline float3 ibl_normalize(float3 v) {
    const float inv = 1.0f / sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    return make_float3(v.x * inv, v.y * inv, v.z * inv);
}
__device__ inline float ibl_radical_inverse(uint32_t bits) {               // RadicalInverse_VdC (prefilter_map.hlsl:31-39) = bit reversal
    return (float)__brev(bits) * 2.3283064365386963e-10f;
}
// sum over the `width` (power of two <= 64) consecutive lanes that hold one texel's partial sums
__device__ inline float ibl_lane_sum(float v, uint32_t width) {
    for (uint32_t o = width >> 1; o > 0u; o >>= 1) v += __shfl_xor(v, (int)o, 64);
    return v;
}

// ---- equirect_to_cubemap.hlsl:78-105: one thread per texel of level 0 --------------------------------------------------------------------
// Everything of a texel but its four fetches: the direction, DirectionToEquirectUV, the tap indices and the blend weights.  Shared by the float
// source (ibl_equirect_kernel) and the RGBE source (ibl_equirect_rgbe_kernel), which differ in how a tap is fetched and in nothing else.
struct IblEquirectTaps { uint32_t i00, i01, i10, i11; float fx, fy; };      // texel indices of (j0, i0), (j0, i1), (j1, i0), (j1, i1); x - x0, y - y0
__device__ __forceinline__ IblEquirectTaps ibl_equirect_taps(uint32_t t, uint32_t n, uint32_t sw, uint32_t sh) {
    #pragma clang fp contract(fast)
    const uint32_t face = t / (n * n), py = (t / n) % n, px = t % n;
    const float3 d = ibl_texel_direction(face, px, py, n);
    const float phi = atan2f(d.z, d.x), theta = asinf(fminf(fmaxf(d.y, -1.0f), 1.0f));        // DirectionToEquirectUV :59-75
    const float u = (phi + IBL_PI) / (2.0f * IBL_PI), v = (theta + IBL_PI * 0.5f) / IBL_PI;
    // Texture2D.SampleLevel(LinearSampler, uv, 0): bilinear, u repeats (longitude wraps), v clamps to the edge
    const float x = u * (float)sw - 0.5f, y = v * (float)sh - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    int i0 = (int)x0 % (int)sw; if (i0 < 0) i0 += (int)sw;
    i0 = min(max(i0, 0), (int)sw - 1);
    const int i1 = i0 + 1 == (int)sw ? 0 : i0 + 1;
    const int j0 = min(max((int)y0, 0), (int)sh - 1), j1 = min(max((int)y0 + 1, 0), (int)sh - 1);
    return IblEquirectTaps{(uint32_t)j0 * sw + (uint32_t)i0, (uint32_t)j0 * sw + (uint32_t)i1, (uint32_t)j1 * sw + (uint32_t)i0, (uint32_t)j1 * sw + (uint32_t)i1,
                           x - x0, y - y0};
}
__global__ void __launch_bounds__(256) ibl_equirect_kernel(const float4* __restrict__ src, uint32_t sw, uint32_t sh, float4* __restrict__ cube, uint32_t n) {
    #pragma clang fp contract(fast)
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= 6u * n * n) return;
    const IblEquirectTaps k = ibl_equirect_taps(t, n, sw, sh);
    const float4 a = src[k.i00], b = src[k.i01];
    const float4 c = src[k.i10], e = src[k.i11];
    cube[t] = ibl_lerp4(ibl_lerp4(a, b, k.fx), ibl_lerp4(c, e, k.fx), k.fy);
}

// ---- Radiance RGBE texels: an R8G8B8A8_UNORM image whose four bytes are (R, G, B, E), read as little-endian words ----------------
// m * 2^(E - 136), built from integer operations alone, so that the result does not depend on the wave's denormal mode: with p the position of m's
// top bit the value is 1.xxx * 2^(p + E - 136), biased exponent p + E - 9; below 1 the result is a denormal whose bits are m * 2^(E - 136) / 2^-149
// = m << (E + 13).  Exact for all 2^16 (m, E) pairs: m has 8 significant bits, the largest value is 255 * 2^119, the smallest 2^-135.
__device__ __forceinline__ float rgbe_channel(uint32_t m, uint32_t e) {
    if (m == 0u) return 0.0f;
    const uint32_t p = 31u - (uint32_t)__clz((int)m);
    const int be = (int)(p + e) - 9;
    const uint32_t bits = be >= 1 ? ((uint32_t)(be - 1) << 23) + (m << (23u - p))      // (m's top bit lands on bit 23 and carries into the exponent)
                                  : m << (e + 13u);
    return __uint_as_float(bits);
}
__device__ __forceinline__ float4 rgbe_decode(uint32_t w) {
    const uint32_t e = w >> 24;
    if (e == 0u) return make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    return make_float4(rgbe_channel(w & 0xFFu, e), rgbe_channel((w >> 8) & 0xFFu, e), rgbe_channel((w >> 16) & 0xFFu, e), 1.0f);
}
// mirhi_image_expand_rgbe: a pure stream, 4 bytes in and 16 bytes out per texel.  A lane works on one texel at a time, so that a wave's accesses are
// whole lines (256 B loaded, 1 KiB stored per instruction: the stores are four fifths of the traffic and are as wide as a lane's store gets), and on
// four texels 256 apart, whose loads are issued together before the first store.
#define RGBE_EXPAND_PER_BLOCK 1024u
__global__ void __launch_bounds__(256) rgbe_expand_kernel(const uint32_t* __restrict__ src, float4* __restrict__ dst, uint32_t texels) {
    const uint32_t base = blockIdx.x * RGBE_EXPAND_PER_BLOCK + threadIdx.x;
    uint32_t w[4];
    #pragma unroll
    for (uint32_t k = 0; k < 4u; k++) { const uint32_t t = base + k * 256u; w[k] = t < texels ? src[t] : 0u; }
    #pragma unroll
    for (uint32_t k = 0; k < 4u; k++) { const uint32_t t = base + k * 256u; if (t < texels) dst[t] = rgbe_decode(w[k]); }
}
// mirhi_ibl_equirect_to_cube_rgbe: ibl_equirect_kernel with each of the four taps decoded from its RGBE word before the blend
__global__ void __launch_bounds__(256) ibl_equirect_rgbe_kernel(const uint32_t* __restrict__ src, uint32_t sw, uint32_t sh, float4* __restrict__ cube, uint32_t n) {
    #pragma clang fp contract(fast)
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= 6u * n * n) return;
    const IblEquirectTaps k = ibl_equirect_taps(t, n, sw, sh);
    const float4 a = rgbe_decode(src[k.i00]), b = rgbe_decode(src[k.i01]);
    const float4 c = rgbe_decode(src[k.i10]), e = rgbe_decode(src[k.i11]);
    cube[t] = ibl_lerp4(ibl_lerp4(a, b, k.fx), ibl_lerp4(c, e, k.fx), k.fy);
}

// ---- cube mip chain: one thread per texel of the destination level, 2 x 2 box filter per face, ((a + b) + (c + d)) * 0.25 (bit-exact) --------
__global__ void __launch_bounds__(256) ibl_cube_mip_kernel(const float4* __restrict__ src, float4* __restrict__ dst, uint32_t dn) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= 6u * dn * dn) return;
    const uint32_t face = t / (dn * dn), y = (t / dn) % dn, x = t % dn, sn = 2u * dn;
    const float4* s = src + face * sn * sn + (2u * y) * sn + 2u * x;
    const float4 a = s[0], b = s[1], c = s[sn], d = s[sn + 1u];
    dst[t] = make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f,
                         ((a.z + b.z) + (c.z + d.z)) * 0.25f, ((a.w + b.w) + (c.w + d.w)) * 0.25f);
}

// ---- irradiance_map.hlsl:63-143 ---------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads per output texel: the 252 x 63 hemisphere samples are split over the lanes (62 or 63 lookups each, neighbouring
// lanes = neighbouring theta of one phi, so a wave's lookups fall on neighbouring texels), the 252 + 63 sines and cosines are computed once
// into LDS, and the partial sums meet through lane shuffles and four LDS slots.  One thread per texel would be 96 waves of 15,876 dependent
// lookups each for a 32^2 map.
#define IBL_IRR_PHI 252u
#define IBL_IRR_THETA 63u
__global__ void __launch_bounds__(256) ibl_irradiance_kernel(IblCube env, float4* __restrict__ out, uint32_t n) {
    #pragma clang fp contract(fast)
    __shared__ float2 sc_phi[IBL_IRR_PHI], sc_theta[IBL_IRR_THETA];
    __shared__ float part[4][3];
    const uint32_t tid = threadIdx.x, t = blockIdx.x;            // (grid = 6 n^2 exactly)
    // the shader's float loops: phi += 0.025f while phi < 2 PI, theta += 0.025f while theta < PI / 2 (252 and 63 steps)
    if (tid == 0u) { float a = 0.0f; for (uint32_t i = 0; i < IBL_IRR_PHI; i++) { sc_phi[i].x = a; a += 0.025f; } }
    if (tid == 64u) { float a = 0.0f; for (uint32_t i = 0; i < IBL_IRR_THETA; i++) { sc_theta[i].x = a; a += 0.025f; } }
    __syncthreads();
    if (tid < IBL_IRR_PHI) { const float a = sc_phi[tid].x; sc_phi[tid] = make_float2(sinf(a), cosf(a)); }
    if (tid < IBL_IRR_THETA) { const float a = sc_theta[tid].x; sc_theta[tid] = make_float2(sinf(a), cosf(a)); }
    __syncthreads();
    const uint32_t face = t / (n * n), py = (t / n) % n, px = t % n;
    const float3 N = ibl_texel_direction(face, px, py, n);
    float3 up = fabsf(N.y) < 0.999f ? make_float3(0.0f, 1.0f, 0.0f) : make_float3(1.0f, 0.0f, 0.0f);
    const float3 right = ibl_normalize(ibl_cross(up, N));
    up = ibl_normalize(ibl_cross(N, right));
    IblCube env0 = env; env0.levels = 1u;
    float r = 0.0f, g = 0.0f, b = 0.0f;
    for (uint32_t s = tid; s < IBL_IRR_PHI * IBL_IRR_THETA; s += 256u) {
        const float2 p = sc_phi[s / IBL_IRR_THETA], th = sc_theta[s % IBL_IRR_THETA];
        const float tx = th.x * p.y, ty = th.x * p.x, tz = th.y;
        const float4 c = ibl_sample_cube(env0, tx * right.x + ty * up.x + tz * N.x, tx * right.y + ty * up.y + tz * N.y,
                                         tx * right.z + ty * up.z + tz * N.z, 0.0f);
        const float w = th.y * th.x;
        r += c.x * w; g += c.y * w; b += c.z * w;
    }
    r = ibl_lane_sum(r, 64u); g = ibl_lane_sum(g, 64u); b = ibl_lane_sum(b, 64u);
    if ((tid & 63u) == 0u) { part[tid >> 6][0] = r; part[tid >> 6][1] = g; part[tid >> 6][2] = b; }
    __syncthreads();
    if (tid == 0u) {
        const float k = IBL_PI / (float)(IBL_IRR_PHI * IBL_IRR_THETA);
        out[t] = make_float4(((part[0][0] + part[1][0]) + (part[2][0] + part[3][0])) * k, ((part[0][1] + part[1][1]) + (part[2][1] + part[3][1])) * k,
                             ((part[0][2] + part[1][2]) + (part[2][2] + part[3][2])) * k, 1.0f);
    }
}
// ... reading a seamless environment (the state of env, the cube being READ: mirhi_image_set_cube_seamless).  The same kernel with the seamless lookup, as a copy:
// a body shared through a template parameter moved ibl_irradiance_kernel's SGPR count (28 -> 29), and the kernels of a cube whose state is off stay what they were.
__global__ void __launch_bounds__(256) ibl_irradiance_kernel_seamless(IblCube env, float4* __restrict__ out, uint32_t n) {
    #pragma clang fp contract(fast)
    __shared__ float2 sc_phi[IBL_IRR_PHI], sc_theta[IBL_IRR_THETA];
    __shared__ float part[4][3];
    const uint32_t tid = threadIdx.x, t = blockIdx.x;            // (grid = 6 n^2 exactly)
    // the shader's float loops: phi += 0.025f while phi < 2 PI, theta += 0.025f while theta < PI / 2 (252 and 63 steps)
    if (tid == 0u) { float a = 0.0f; for (uint32_t i = 0; i < IBL_IRR_PHI; i++) { sc_phi[i].x = a; a += 0.025f; } }
    if (tid == 64u) { float a = 0.0f; for (uint32_t i = 0; i < IBL_IRR_THETA; i++) { sc_theta[i].x = a; a += 0.025f; } }
    __syncthreads();
    if (tid < IBL_IRR_PHI) { const float a = sc_phi[tid].x; sc_phi[tid] = make_float2(sinf(a), cosf(a)); }
    if (tid < IBL_IRR_THETA) { const float a = sc_theta[tid].x; sc_theta[tid] = make_float2(sinf(a), cosf(a)); }
    __syncthreads();
    const uint32_t face = t / (n * n), py = (t / n) % n, px = t % n;
    const float3 N = ibl_texel_direction(face, px, py, n);
    float3 up = fabsf(N.y) < 0.999f ? make_float3(0.0f, 1.0f, 0.0f) : make_float3(1.0f, 0.0f, 0.0f);
    const float3 right = ibl_normalize(ibl_cross(up, N));
    up = ibl_normalize(ibl_cross(N, right));
    IblCube env0 = env; env0.levels = 1u;
    float r = 0.0f, g = 0.0f, b = 0.0f;
    for (uint32_t s = tid; s < IBL_IRR_PHI * IBL_IRR_THETA; s += 256u) {
        const float2 p = sc_phi[s / IBL_IRR_THETA], th = sc_theta[s % IBL_IRR_THETA];
        const float tx = th.x * p.y, ty = th.x * p.x, tz = th.y;
        const float4 c = ibl_sample_cube_seamless(env0, tx * right.x + ty * up.x + tz * N.x, tx * right.y + ty * up.y + tz * N.y,
                                         tx * right.z + ty * up.z + tz * N.z, 0.0f);
        const float w = th.y * th.x;
        r += c.x * w; g += c.y * w; b += c.z * w;
    }
    r = ibl_lane_sum(r, 64u); g = ibl_lane_sum(g, 64u); b = ibl_lane_sum(b, 64u);
    if ((tid & 63u) == 0u) { part[tid >> 6][0] = r; part[tid >> 6][1] = g; part[tid >> 6][2] = b; }
    __syncthreads();
    if (tid == 0u) {
        const float k = IBL_PI / (float)(IBL_IRR_PHI * IBL_IRR_THETA);
        out[t] = make_float4(((part[0][0] + part[1][0]) + (part[2][0] + part[3][0])) * k, ((part[0][1] + part[1][1]) + (part[2][1] + part[3][1])) * k,
                             ((part[0][2] + part[1][2]) + (part[2][2] + part[3][2])) * k, 1.0f);
    }
}

// ---- prefilter_map.hlsl:134-229, every level in one grid -----------------------------------------------------------------------------------
// N = V = R, so in tangent space everything of a sample but the lookup is the same for every texel of a level: H, NdotH = HdotV = H.z,
// L = 2 H.z H - (0, 0, 1), NdotL = L.z, D, pdf and so mipLevel.  A workgroup builds that table for its level once in LDS -- float4 (L, mipLevel),
// the samples with NdotL <= 0 dropped, order kept -- and then does, per texel and kept sample, one 3 x 3 basis change and one trilinear lookup.
// `lanes` (1, 4, 16 or 64) lanes share a texel and split its samples, chosen per level on the host so that the small levels still fill the chip.
// Levels with Roughness < 0.01 are one lookup per texel, one thread each.
#define IBL_MAX_LEVELS 13u
struct IblPrefilterPlan {
    uint32_t levels, sample_count, size;
    uint32_t first_block[IBL_MAX_LEVELS + 1u];      // blocks [first_block[l], first_block[l + 1]) work on level l
    uint32_t lanes[IBL_MAX_LEVELS];                 // lanes per texel
};
// SEAMLESS: the state of env (every lookup, the single one of a level with Roughness < 0.01 included; ibl_prefilter_kernel_seamless below)
template <bool SEAMLESS>
__device__ __forceinline__ void ibl_prefilter_body(const IblCube& env, float4* __restrict__ out, const IblPrefilterPlan& plan) {
    #pragma clang fp contract(fast)
    extern __shared__ float4 table[];               // sample_count entries
    __shared__ uint32_t wave_kept[4];
    const uint32_t tid = threadIdx.x;
    uint32_t level = 0;
    while (level + 1u < plan.levels && blockIdx.x >= plan.first_block[level + 1u]) level++;
    const uint32_t m = plan.size >> level, texels = 6u * m * m;
    const uint32_t lanes = plan.lanes[level], per_block = 256u / lanes;
    const uint32_t t = (blockIdx.x - plan.first_block[level]) * per_block + tid / lanes, sub = tid % lanes;
    const bool live = t < texels;
    const uint32_t tc = live ? t : texels - 1u;
    const uint32_t face = tc / (m * m), py = (tc / m) % m, px = tc % m;
    const float3 N = ibl_texel_direction(face, px, py, m);
    float4* dst = out + ibl_level_offset(plan.size, level) + tc;
    const float roughness = plan.levels > 1u ? (float)level / (float)(plan.levels - 1u) : 0.0f;
    if (roughness < 0.01f) {                         // :168-173 (block-uniform; lanes == 1 here)
        const float4 c = ibl_sample_cube_as<SEAMLESS>(env, N.x, N.y, N.z, 0.0f);
        if (live) *dst = make_float4(c.x, c.y, c.z, 1.0f);
        return;
    }
    // the table: Hammersley + ImportanceSampleGGX in tangent space, in sample order, compacted
    const uint32_t S = plan.sample_count;
    const float a = roughness * roughness, a2 = a * a;
    const float sa_texel = 4.0f * IBL_PI / (6.0f * 512.0f * 512.0f);
    uint32_t kept = 0;
    for (uint32_t base = 0; base < S; base += 256u) {
        const uint32_t i = base + tid;
        float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        bool keep = false;
        if (i < S) {
            const float xi_x = (float)i / (float)S, xi_y = ibl_radical_inverse(i);
            const float phi = 2.0f * IBL_PI * xi_x;
            const float cos_t = sqrtf((1.0f - xi_y) / (1.0f + (a2 - 1.0f) * xi_y));
            const float sin_t = sqrtf(fmaxf(1.0f - cos_t * cos_t, 0.0f));
            const float hx = cosf(phi) * sin_t, hy = sinf(phi) * sin_t, hz = cos_t;
            const float lx = 2.0f * hz * hx, ly = 2.0f * hz * hy, lz = 2.0f * hz * hz - 1.0f;
            const float inv = 1.0f / sqrtf(lx * lx + ly * ly + lz * lz);       // normalize(2 dot(V, H) H - V)
            float denom = hz * hz * (a2 - 1.0f) + 1.0f;
            denom = IBL_PI * denom * denom;
            const float D = a2 / fmaxf(denom, 0.0001f);
            const float pdf = (D * hz) / (4.0f * hz) + 0.0001f;
            const float sa_sample = 1.0f / ((float)S * pdf + 0.0001f);
            const float mip = fmaxf(0.0f, 0.5f * __log2f(sa_sample / sa_texel));
            e = make_float4(lx * inv, ly * inv, lz * inv, mip);
            keep = e.z > 0.0f;
        }
        const unsigned long long ballot = __ballot(keep);
        if ((tid & 63u) == 0u) wave_kept[tid >> 6] = (uint32_t)__popcll(ballot);
        __syncthreads();
        uint32_t slot = kept + (uint32_t)__popcll(ballot & ((1ull << (tid & 63u)) - 1ull));
        for (uint32_t w = 0; w < (tid >> 6); w++) slot += wave_kept[w];
        if (keep) table[slot] = e;                   // slot < S: at most one entry per sample
        kept += wave_kept[0] + wave_kept[1] + wave_kept[2] + wave_kept[3];
        __syncthreads();
    }
    const uint32_t count = kept;                     // (the same in every thread)
    float3 up = fabsf(N.z) < 0.999f ? make_float3(0.0f, 0.0f, 1.0f) : make_float3(1.0f, 0.0f, 0.0f);
    const float3 T = ibl_normalize(ibl_cross(up, N));
    const float3 B = ibl_cross(N, T);
    float r = 0.0f, g = 0.0f, b = 0.0f, wsum = 0.0f;
    for (uint32_t k = sub; k < count; k += lanes) {
        const float4 e = table[k];
        const float4 c = ibl_sample_cube_as<SEAMLESS>(env, T.x * e.x + B.x * e.y + N.x * e.z, T.y * e.x + B.y * e.y + N.y * e.z,
                                         T.z * e.x + B.z * e.y + N.z * e.z, e.w);
        r += c.x * e.z; g += c.y * e.z; b += c.z * e.z; wsum += e.z;
    }
    r = ibl_lane_sum(r, lanes); g = ibl_lane_sum(g, lanes); b = ibl_lane_sum(b, lanes); wsum = ibl_lane_sum(wsum, lanes);
    if (live && sub == 0u) {
        const float inv = wsum > 0.0f ? 1.0f / wsum : 1.0f;
        *dst = make_float4(r * inv, g * inv, b * inv, 1.0f);
    }
}
__global__ void __launch_bounds__(256) ibl_prefilter_kernel(IblCube env, float4* __restrict__ out, IblPrefilterPlan plan) { ibl_prefilter_body<false>(env, out, plan); }
__global__ void __launch_bounds__(256) ibl_prefilter_kernel_seamless(IblCube env, float4* __restrict__ out, IblPrefilterPlan plan) { ibl_prefilter_body<true>(env, out, plan); }

// ---- brdf_lut.hlsl:116-206 ---------------------------------------------------------------------------------------------------------------
// A workgroup works on 256 texels of one row (one roughness): the 1024 half vectors of ImportanceSampleGGX depend on the row alone and are built
// once in LDS; N = (0, 0, 1) takes the shader's |N.z| >= 0.999 branch, whose basis turns the tangent-space H = (x, y, z) into (y, -x, z).
#define IBL_LUT_SAMPLES 1024u
__global__ void __launch_bounds__(256) ibl_brdf_lut_kernel(float4* __restrict__ out, uint32_t n) {
    #pragma clang fp contract(fast)
    __shared__ float4 hs[IBL_LUT_SAMPLES];
    const uint32_t tid = threadIdx.x, row = blockIdx.y, col = blockIdx.x * 256u + tid;
    const float roughness = ((float)row + 0.5f) / (float)n;
    const float a = roughness * roughness, a2 = a * a;
    for (uint32_t i = tid; i < IBL_LUT_SAMPLES; i += 256u) {
        const float xi_x = (float)i / (float)IBL_LUT_SAMPLES, xi_y = ibl_radical_inverse(i);
        const float phi = 2.0f * IBL_PI * xi_x;
        const float cos_t = sqrtf((1.0f - xi_y) / (1.0f + (a2 - 1.0f) * xi_y));
        const float sin_t = sqrtf(fmaxf(1.0f - cos_t * cos_t, 0.0f));
        hs[i] = make_float4(sinf(phi) * sin_t, -(cosf(phi) * sin_t), cos_t, 0.0f);
    }
    __syncthreads();
    if (col >= n) return;
    const float ndv = fmaxf(((float)col + 0.5f) / (float)n, 0.001f);
    const float vx = sqrtf(1.0f - ndv * ndv), vz = ndv;
    const float k = (roughness * roughness) * 0.5f, omk = 1.0f - k;
    const float g_v = ndv * __builtin_amdgcn_rcpf(fmaxf(ndv * omk + k, 0.0001f));
    float A = 0.0f, Bsum = 0.0f;
    for (uint32_t i = 0; i < IBL_LUT_SAMPLES; i++) {
        const float4 h = hs[i];
        const float vdh_raw = vx * h.x + vz * h.z;
        const float lx = 2.0f * vdh_raw * h.x - vx, ly = 2.0f * vdh_raw * h.y, lz = 2.0f * vdh_raw * h.z - vz;
        const float ndl = lz * __builtin_amdgcn_rsqf(lx * lx + ly * ly + lz * lz);
        if (ndl > 0.0f) {
            const float ndh = fmaxf(h.z, 0.0f), vdh = fmaxf(vdh_raw, 0.0f);
            const float G = ndl * __builtin_amdgcn_rcpf(fmaxf(ndl * omk + k, 0.0001f)) * g_v;
            const float g_vis = (G * vdh) * __builtin_amdgcn_rcpf(fmaxf(ndh * ndv, 0.0001f));
            const float o = 1.0f - vdh, o2 = o * o, fc = o2 * o2 * o;
            A += (1.0f - fc) * g_vis; Bsum += fc * g_vis;
        }
    }
    out[row * n + col] = make_float4(A * (1.0f / (float)IBL_LUT_SAMPLES), Bsum * (1.0f / (float)IBL_LUT_SAMPLES), 0.0f, 1.0f);
}
