// mirhi_shading.hip.h -- fragment programs: TRIANGLE, MODEL, MODEL_FULL, MODEL_PBR, MODEL_PBR_IBL; texture sampling; sRGB pack (rows a8, a9)
// Part of the single device translation unit mirhi_kernels.hip (included inside namespace mirhi).
#ifndef MIRHI_SHADING_HIP_H
#define MIRHI_SHADING_HIP_H

// ------------------------------------------------------------------------------------------------
// a8: fragment programs.  Colour is tolerance-checked (|dRGB| < 1e-4 vs the oracle), not bit-exact, so
// this part may contract to FMA and use the 1-ulp hardware rcp / rsq / exp2 / log2.
// ------------------------------------------------------------------------------------------------
#pragma clang fp contract(fast)

__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float frsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
// pow(x, y) for x >= 0 as exp2(y * log2(x)) (HLSL pow lowering); pow(0, y>0) = 0
// log2 near 1 comes from the series of ln(1+t) (t = x-1 is exact there): the hardware v_log_f32 has an absolute
// error of ~2^-22 around 1, which a Blinn-Phong exponent of up to 2048 would amplify past the 1e-4 colour bound.
__device__ __forceinline__ float flog2(float x) {
    const float t = x - 1.0f;
    const float p = t * (1.0f + t * (-0.5f + t * (0.33333334f + t * (-0.25f + t * 0.2f))));
    return fabsf(t) < 0.015625f ? p * 1.44269504089f : __builtin_amdgcn_logf(x);
}
__device__ __forceinline__ float fpow(float x, float y) { return __builtin_amdgcn_exp2f(y * flog2(x)); }
__device__ __forceinline__ f3 fnormalize3(f3 a) { const float r = frsq(dot3(a, a)); return {a.x * r, a.y * r, a.z * r}; }
#pragma clang fp contract(off)

// IEEE quotients, like the oracle's: a 1-ulp reciprocal here looks harmless (it only scales the light's colour) but a blended draw on
// top can feed the lit colour back through (1 - dst) factors and a reverse subtract -- the round-2 soak found one such scene in 160,000
// (seed 2018940 of tools/soak_fuzz.py: one pixel at 1.01e-4) while these two lines used v_rcp_f32.
__device__ __forceinline__ float attenuation(float distance, float radius) {          // lights.hlsli:63-73
    const float att = rcp_rn_nb(distance * distance + 1.0f);
    float falloff = saturatef(1.0f - div_rn_nb(distance, radius));
    falloff = falloff * falloff;
    return att * falloff;
}
__device__ __forceinline__ float roughness_to_shininess(float roughness) {             // lights.hlsli:152-159
    const float r = roughness < 0.0f ? 0.0f : (roughness > 1.0f ? 1.0f : roughness);
    return 2048.0f + (2.0f - 2048.0f) * r;
}
__device__ __forceinline__ f3 blinn_phong(f3 L, f3 V, f3 N, f3 lightColor, f3 albedo, float shininess) {  // :95-117
    float NdotL = dot3(N, L);
    if (!(NdotL > 0.0f)) NdotL = 0.0f;
    const f3 diffuse = mul3(scale3(lightColor, NdotL), albedo);
    if (NdotL <= 0.0f) return diffuse;
    const f3 H = normalize3(add3(L, V));
    float NdotH = dot3(N, H);
    if (!(NdotH > 0.0f)) NdotH = 0.0f;
    const float sp = fpow(NdotH, shininess);
    return add3(diffuse, scale3(lightColor, sp));
}

// sRGB byte -> linear, uploaded once per device (mirhi_api.hip builds it in double; the oracle builds the same table)
__device__ float g_srgb_lut[256];

__device__ __forceinline__ f4 unpack_rgba8(uint32_t p, bool srgb) {
    const float s = 1.0f / 255.0f;
    if (srgb) return {g_srgb_lut[p & 0xFF], g_srgb_lut[(p >> 8) & 0xFF], g_srgb_lut[(p >> 16) & 0xFF], (float)(p >> 24) * s};
    return {(float)(p & 0xFF) * s, (float)((p >> 8) & 0xFF) * s, (float)((p >> 16) & 0xFF) * s, (float)(p >> 24) * s};
}
// repeat addressing of one coordinate: c mod n into [0, n); a mask when n is a power of two (the usual case),
// one division otherwise.  The +1 neighbour wraps by comparison, so a bilinear tap costs two of these, not eight.
__device__ __forceinline__ int32_t wrap_coord(int32_t c, int32_t n) {
    if ((n & (n - 1)) == 0) return c & (n - 1);          // n is wave-uniform: a scalar branch
    c %= n;
    return c < 0 ? c + n : c;
}
// bilinear tap of one mip level, repeat addressing (see oracle sample_level)
__device__ __forceinline__ f4 sample_level(const uint32_t* texels, uint32_t w, uint32_t h, float u, float v, bool srgb) {
    if (w == 1 && h == 1) return unpack_rgba8(texels[0], srgb);
    const float fx = u * (float)w - 0.5f, fy = v * (float)h - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float ax = fx - x0f, ay = fy - y0f;
    const int32_t x0 = wrap_coord((int32_t)x0f, (int32_t)w), y0 = wrap_coord((int32_t)y0f, (int32_t)h);
    const int32_t x1 = x0 + 1 == (int32_t)w ? 0 : x0 + 1, y1 = y0 + 1 == (int32_t)h ? 0 : y0 + 1;
    const uint32_t r0 = (uint32_t)y0 * w, r1 = (uint32_t)y1 * w;
    const f4 c00 = unpack_rgba8(texels[r0 + (uint32_t)x0], srgb), c10 = unpack_rgba8(texels[r0 + (uint32_t)x1], srgb);
    const f4 c01 = unpack_rgba8(texels[r1 + (uint32_t)x0], srgb), c11 = unpack_rgba8(texels[r1 + (uint32_t)x1], srgb);
    f4 r;
#define MIRHI_LERP2(f) { const float top = c00.f + (c10.f - c00.f) * ax; const float bot = c01.f + (c11.f - c01.f) * ax; r.f = top + (bot - top) * ay; }
    MIRHI_LERP2(x) MIRHI_LERP2(y) MIRHI_LERP2(z) MIRHI_LERP2(w)
#undef MIRHI_LERP2
    return r;
}
// screen-space derivatives of the texture coordinates: (u, v) one pixel to the right and one pixel down, minus (u, v)
struct UvGrad { float dudx, dvdx, dudy, dvdy; };
// trilinear tap at level-of-detail lam (clamped to [0, levels - 1]) -- see oracle sample_trilinear
__device__ __forceinline__ f4 sample_trilinear(const uint32_t* texels, uint32_t w, uint32_t h, uint32_t levels, float u, float v, float lam, bool srgb) {
    if (!(lam > 0.0f)) lam = 0.0f;                                        // magnification, zero footprint, NaN
    const float top = (float)(levels - 1u);
    if (lam > top) lam = top;
    const float l0f = floorf(lam), f = lam - l0f;
    const uint32_t l0 = (uint32_t)l0f;
    uint32_t lw = w, lh = h;
    for (uint32_t l = 0; l < l0; l++) { texels += (size_t)lw * lh; lw = lw > 1u ? lw >> 1 : 1u; lh = lh > 1u ? lh >> 1 : 1u; }
    const f4 c0 = sample_level(texels, lw, lh, u, v, srgb);
    if (l0 + 1u >= levels) return c0;
    const uint32_t* next = texels + (size_t)lw * lh;
    const f4 c1 = sample_level(next, lw > 1u ? lw >> 1 : 1u, lh > 1u ? lh >> 1 : 1u, u, v, srgb);
    return {c0.x + (c1.x - c0.x) * f, c0.y + (c1.y - c0.y) * f, c0.z + (c1.z - c0.z) * f, c0.w + (c1.w - c0.w) * f};
}
// ---- sampler state (mirhi_image_set_sampler, include/mirhi.h) ----
// The state of a slot is wave-uniform (scalar loads of DrawDesc::tex_sampler / tex_aniso), so everything that depends on the state alone is a scalar
// branch; what depends on lambda (mag or min filter) is the lane's own.  A slot whose state is all zero never gets here: sample_texture keeps the
// sequence it had before the state existed.
// One coordinate under an address mode (the Vulkan specification, "Wrapping Operation"), with the level's extent n:
//   REPEAT i mod n; MIRRORED_REPEAT (n - 1) - mirror((i mod 2n) - n), mirror(a) = a >= 0 ? a : -(1 + a), which is m = i mod 2n folded at n;
//   CLAMP_TO_EDGE clamp(i, 0, n - 1)
__device__ __forceinline__ int32_t address_coord(int32_t c, int32_t n, uint32_t mode) {
    if (mode == 2u) return c < 0 ? 0 : (c > n - 1 ? n - 1 : c);
    if (mode == 1u) { const int32_t m = wrap_coord(c, 2 * n); return m < n ? m : 2 * n - 1 - m; }
    return wrap_coord(c, n);
}
// adds weight * texel to the accumulator: the texel stays packed until here, so that the four corners of a tap are four registers, not sixteen
__device__ __forceinline__ void accumulate_texel(f4& acc, uint32_t p, float weight, bool srgb) {
    const f4 c = unpack_rgba8(p, srgb);
    acc.x += c.x * weight; acc.y += c.y * weight; acc.z += c.z * weight; acc.w += c.w * weight;
}
// A texture under a sampler state `st` = address_u | address_v << 2 | mag_filter << 4 | min_filter << 5 | mip_mode << 6 that is not all zero.
// lambda is the level of detail sample_texture computes, before clamping: the mag filter where lambda <= 0 (also a zero footprint and NaN, which
// sample_trilinear treats as magnification too), the min filter where lambda > 0.  Levels: MIP_LINEAR as sample_trilinear; MIP_NEAREST the level
// ceil(lambda + 1/2) - 1 clamped to [0, levels - 1]; MIP_BASE, or no chain: level 0.  max_aniso > 1 (record_draw sets it only for LINEAR
// minification with MIP_LINEAR): the taps of sample_texture's anisotropic filter, each through this state, lambda being the filter's own.
// NEAREST reads the one texel at floor(u w), floor(v h), LINEAR the four around u w - 1/2, v h - 1/2, each coordinate through its address mode.
// (The +1 neighbour is formed as a float: a coordinate beyond the int32 range saturates in the conversion instead of overflowing, and every
// mode brings whatever comes out into [0, n).)
// The result is ONE weighted sum over every texel read -- weight = level weight x column weight x row weight, the sum over N -- in loops that are not
// unrolled (taps, levels), not the nested lerps of sample_level: the fragment programs sit at their register ceiling, and this form keeps an
// accumulator and four packed texels live where the other keeps sixteen floats per level.  The two forms differ by roundings of 2^-24.
__device__ __forceinline__ f4 sample_texture_state(const uint32_t* texels, uint32_t w, uint32_t h, uint32_t levels, float u, float v, const UvGrad& g, bool srgb,
                                                   uint32_t st, uint32_t max_aniso) {
    const uint32_t au = st & 3u, av = (st >> 2) & 3u, mip = st >> 6;
    float lam, nf = 1.0f;
    bool major_x = false;
    {
        const float ax = g.dudx * (float)w, bx = g.dvdx * (float)h, ay = g.dudy * (float)w, by = g.dvdy * (float)h;
        const float rx = ax * ax + bx * bx, ry = ay * ay + by * by;
        lam = 0.5f * __builtin_amdgcn_logf(rx > ry ? rx : ry);
        if (max_aniso > 1u) {                                        // (sample_texture's arithmetic: N has to be the oracle's integer)
            major_x = rx > ry;
            const float pmax = __builtin_sqrtf(major_x ? rx : ry), pmin = __builtin_sqrtf(major_x ? ry : rx);
            nf = __builtin_ceilf(pmax / pmin);
            if (!(nf <= (float)max_aniso)) nf = (float)max_aniso;
            if (!(nf >= 1.0f)) nf = 1.0f;
            lam = __builtin_amdgcn_logf(pmax / nf);
        }
    }
    const bool nearest = ((st >> (lam > 0.0f ? 5 : 4)) & 1u) != 0u;
    // the first level and the weight of the one behind it (0: that level is not read -- with a weight of exactly 0 it would add exactly nothing)
    float f = 0.0f;
    uint32_t l0 = 0u;
    if (levels > 1u && mip != 2u) {
        const float top = (float)(levels - 1u);
        if (mip == 1u) {
            float d = __builtin_ceilf(lam + 0.5f) - 1.0f;
            if (!(d > 0.0f)) d = 0.0f;
            if (d > top) d = top;
            l0 = (uint32_t)d;
        } else {
            if (!(lam > 0.0f)) lam = 0.0f;
            if (lam > top) lam = top;
            const float l0f = floorf(lam);
            f = lam - l0f; l0 = (uint32_t)l0f;             // (lam <= top: f > 0 only where level l0 + 1 exists)
        }
    }
    f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (float fi = 1.0f; fi <= nf; fi += 1.0f) {
        float tu = u, tv = v;
        if (max_aniso > 1u) {
            const float ti = fi / (nf + 1.0f) - 0.5f;
            tu = u + (major_x ? g.dudx : g.dudy) * ti; tv = v + (major_x ? g.dvdx : g.dvdy) * ti;
        }
#pragma unroll 1
        for (uint32_t k = 0; k < (f > 0.0f ? 2u : 1u); k++) {
            uint32_t off = 0u, lw = w, lh = h;              // the level's first texel (a chain of a 16384 x 16384 texture is under 2^29 texels) and its extent
#pragma unroll 1
            for (uint32_t l = 0; l < l0 + k; l++) { off += lw * lh; lw = lw > 1u ? lw >> 1 : 1u; lh = lh > 1u ? lh >> 1 : 1u; }
            const float wl = k == 0u ? 1.0f - f : f;
            if (nearest) {
                const int32_t x = address_coord((int32_t)floorf(tu * (float)lw), (int32_t)lw, au), y = address_coord((int32_t)floorf(tv * (float)lh), (int32_t)lh, av);
                accumulate_texel(acc, texels[off + (uint32_t)y * lw + (uint32_t)x], wl, srgb);
            } else {
                const float fx = tu * (float)lw - 0.5f, fy = tv * (float)lh - 0.5f;
                const float x0f = floorf(fx), y0f = floorf(fy);
                const uint32_t x0 = (uint32_t)address_coord((int32_t)x0f, (int32_t)lw, au), x1 = (uint32_t)address_coord((int32_t)(x0f + 1.0f), (int32_t)lw, au);
                const uint32_t r0 = off + (uint32_t)address_coord((int32_t)y0f, (int32_t)lh, av) * lw, r1 = off + (uint32_t)address_coord((int32_t)(y0f + 1.0f), (int32_t)lh, av) * lw;
                const uint32_t p00 = texels[r0 + x0], p10 = texels[r0 + x1], p01 = texels[r1 + x0], p11 = texels[r1 + x1];
                const float ax = fx - x0f, ay = fy - y0f;
                const float wt = wl * (1.0f - ay), wb = wl * ay;
                accumulate_texel(acc, p00, wt * (1.0f - ax), srgb);
                accumulate_texel(acc, p10, wt * ax, srgb);
                accumulate_texel(acc, p01, wb * (1.0f - ax), srgb);
                accumulate_texel(acc, p11, wb * ax, srgb);
            }
        }
    }
    if (max_aniso > 1u) { const float inv_n = 1.0f / nf; acc.x *= inv_n; acc.y *= inv_n; acc.z *= inv_n; acc.w *= inv_n; }
    return acc;
}
// Texture slot `slot` of the draw at (u, v).  The default sampler (the reference never creates one -- sampler.rs is a stub -- so REPEAT addressing and
// LINEAR filters are what a texture has until mirhi_image_set_sampler says otherwise).  Without a mip chain: bilinear.  With a chain
// (mirhi_image_generate_mips): trilinear, LOD = log2 of the longer screen-space footprint axis in texels,
// lambda = 0.5 * log2(max(|d(uv*size)/dx|^2, |d(uv*size)/dy|^2)) clamped to [0, levels - 1].
// With a chain and max_anisotropy > 1 (mirhi_image_set_max_anisotropy; device.rs:161-165 enables the feature): the Vulkan
// specification's example filter -- N = min(ceil(Pmax / Pmin), max_anisotropy) trilinear taps along the longer footprint axis at
// lambda = log2(Pmax / N), averaged (oracle sample_texture).  N has to be the oracle's integer, so the square roots and the
// quotient that decide it are the compiler's IEEE expansions (the path is taken by whole draws, rarely: instructions do not matter).
// A slot with sampler state (any bit of its share of tex_sampler / tex_aniso's mip modes; only the full-featured variant sees such draws) leaves
// through sample_texture_state on one scalar branch; every other slot runs the sequence below unchanged.
// STATE false: the caller's draws never carry sampler state on the slot it reads (pbr_base_alpha, slot 0: classify_scope keeps such draws out of the
// masked raster variants).
template <bool MIPS, bool STATE = MIPS>
__device__ __forceinline__ f4 sample_texture(DrawRef D, int slot, float u, float v, const UvGrad& g) {
    const uint32_t w = D.tex_w[slot], h = D.tex_h[slot], levels = D.tex_levels[slot];
    const uint32_t* texels = reinterpret_cast<const uint32_t*>(D.tex[slot]);
    if (!texels || w == 0 || h == 0) return {1.0f, 1.0f, 1.0f, 1.0f};
    const bool srgb = MIPS && ((D.tex_srgb >> slot) & 1u);      // (sRGB and mip-mapped textures live in the full-featured variant)
    if constexpr (STATE) {
        const uint32_t st = ((D.tex_sampler >> (6 * slot)) & 63u) | (((D.tex_aniso >> (TEX_MIP_MODE_SHIFT + 2 * slot)) & 3u) << 6);      // wave-uniform
        if (st != 0u) return sample_texture_state(texels, w, h, levels, u, v, g, srgb, st, ((D.tex_aniso >> (4 * slot)) & 15u) + 1u);
    }
    if (!MIPS || levels <= 1u) return sample_level(texels, w, h, u, v, srgb);
    const float ax = g.dudx * (float)w, bx = g.dvdx * (float)h, ay = g.dudy * (float)w, by = g.dvdy * (float)h;
    const float rx = ax * ax + bx * bx, ry = ay * ay + by * by;
    const uint32_t max_aniso = ((D.tex_aniso >> (4 * slot)) & 15u) + 1u;          // wave-uniform (scalar loads)
    if (max_aniso <= 1u) return sample_trilinear(texels, w, h, levels, u, v, 0.5f * __builtin_amdgcn_logf(rx > ry ? rx : ry), srgb);   // v_log_f32 is log2
    const bool major_x = rx > ry;
    const float pmax = __builtin_sqrtf(major_x ? rx : ry), pmin = __builtin_sqrtf(major_x ? ry : rx);
    float nf = __builtin_ceilf(pmax / pmin);
    if (!(nf <= (float)max_aniso)) nf = (float)max_aniso;      // also a zero short axis (inf) and a zero footprint (NaN)
    if (!(nf >= 1.0f)) nf = 1.0f;
    const float lam = __builtin_amdgcn_logf(pmax / nf);
    const float du = major_x ? g.dudx : g.dudy, dv = major_x ? g.dvdx : g.dvdy;
    f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    const float np1 = nf + 1.0f;
    // lanes run their own tap counts (at most 16)
#pragma unroll 1
    for (float fi = 1.0f; fi <= nf; fi += 1.0f) {
        const float ti = fi / np1 - 0.5f;
        const f4 sm = sample_trilinear(texels, w, h, levels, u + du * ti, v + dv * ti, lam, srgb);
        acc.x += sm.x; acc.y += sm.y; acc.z += sm.z; acc.w += sm.w;
    }
    return {acc.x / nf, acc.y / nf, acc.z / nf, acc.w / nf};
}

#pragma clang fp contract(off)
// Everything that feeds pow(NdotH, shininess) must match the oracle bit for bit: an exponent of up to 2048
// turns a 1-ulp difference in NdotH into a 1e-4 relative difference of the specular term.
// Shaded vertices are interpolated as they are fetched: ((b0 * a0 + b1 * a1) + b2 * a2) accumulated vertex by vertex -- the oracle's
// operation order -- so that one vertex's attributes are live at a time, not three (3 x 14 floats held 42 VGPRs and, together with
// the exact IEEE sequences, pushed the MODEL variants past their 96 registers).
__device__ __forceinline__ void acc1(float& a, float bk, float v, uint32_t k) { const float t = bk * v; a = k == 0u ? t : a + t; }
__device__ __forceinline__ void acc3(f3& a, float bk, f3 v, uint32_t k) { acc1(a.x, bk, v.x, k); acc1(a.y, bk, v.y, k); acc1(a.z, bk, v.z, k); }
// tangent and bitangent of the three shaded vertices (MODEL_FULL / MODEL_PBR layout, words 3 and 4), interpolated on demand: only
// pixels under a real normal map need them
__device__ __forceinline__ void interp_tangent_frame(DrawRef D, const uint32_t vi[3], const float b[3], f3& T, f3& Bt) {
    T = {0.0f, 0.0f, 0.0f}; Bt = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        const uint4* sv = reinterpret_cast<const uint4*>(D.vs_attr) + (size_t)vi[k] * (D.vs_words - 1u) - 1;     // (sv[1..]: the attribute words)
        const uint4 w3 = sv[3], w4 = sv[4];
        acc3(T, b[k], {__uint_as_float(w3.x), __uint_as_float(w3.y), __uint_as_float(w3.z)}, k);
        acc3(Bt, b[k], {__uint_as_float(w3.w), __uint_as_float(w4.x), __uint_as_float(w4.y)}, k);
    }
}

__device__ __forceinline__ f3 interp3(const float b[3], f3 a0, f3 a1, f3 a2) {
    return {(b[0] * a0.x + b[1] * a1.x) + b[2] * a2.x, (b[0] * a0.y + b[1] * a1.y) + b[2] * a2.y,
            (b[0] * a0.z + b[1] * a1.z) + b[2] * a2.z};
}

// perspective-correct barycentrics of the pixel centre from the original clip-space triangle
// (2-D homogeneous form relative to the pixel: valid for w <= 0 vertices, no clipped attributes needed)
template <bool FAST>
__device__ __forceinline__ void barycentrics(DrawRef D, const f4 c[3], float pxc, float pyc, float b[3]) {
    float ax[3], ay[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        ax[k] = (c[k].x * D.hw + c[k].w * D.cx) - pxc * c[k].w;
        ay[k] = (c[k].y * D.hh + c[k].w * D.cy) - pyc * c[k].w;
    }
    const float l0 = ax[1] * ay[2] - ax[2] * ay[1];
    const float l1 = ax[2] * ay[0] - ax[0] * ay[2];
    const float l2 = ax[0] * ay[1] - ax[1] * ay[0];
    const float inv = FAST ? __builtin_amdgcn_rcpf((l0 + l1) + l2) : rcp_rn_nb((l0 + l1) + l2);
    b[0] = l0 * inv; b[1] = l1 * inv; b[2] = l2 * inv;
}

// vertex/triangle.hlsl + pixel/triangle.hlsl: clip = (pos, 1), colour pass-through.  Strict arithmetic in the oracle's
// operation order: for a sliver triangle the three lambdas nearly cancel, and a contracted FMA or the 1-ulp rcp then shows
// up as 1e-3 in the interpolated colour (found by the 60000-scene soak of tools/soak_fuzz.py; one pixel in ~3000 scenes).
// With w = 1 the homogeneous form is ax_k = (x_k * W/2 + cx) - px.  Flat-coloured triangles never get here (flat_color).
// vin: the triangle's three vertex indices (fetch_triangle_indices), which a caller that shades the same triangle several times
// fetches once
__device__ __forceinline__ f4 shade_triangle_program(DrawRef D, const uint32_t vin[3], float pxc, float pyc) {
    float ax[3], ay[3]; f3 col[3];
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        const uint8_t* v = D.vb + (size_t)vin[k] * D.stride;
        ax[k] = (ldf(v, 0) * D.hw + D.cx) - pxc;                             // vertex/triangle.hlsl:19-20
        ay[k] = (ldf(v, 4) * D.hh + D.cy) - pyc;
        col[k] = {ldf(v, 12), ldf(v, 16), ldf(v, 20)};
    }
    const float l0 = ax[1] * ay[2] - ax[2] * ay[1];
    const float l1 = ax[2] * ay[0] - ax[0] * ay[2];
    const float l2 = ax[0] * ay[1] - ax[1] * ay[0];
    const float inv = rcp_rn_nb((l0 + l1) + l2);
    const float b[3] = {l0 * inv, l1 * inv, l2 * inv};
    const f3 o = interp3(b, col[0], col[1], col[2]);                         // pixel/triangle.hlsl:10-13
    return {o.x, o.y, o.z, 1.0f};
}
__device__ __forceinline__ void fetch_triangle_indices(DrawRef D, uint32_t tri, uint32_t vin[3]) {
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) vin[k] = fetch_index(D, 3u * tri + k);
}
__device__ __forceinline__ f4 shade_triangle_program(DrawRef D, uint32_t tri, float pxc, float pyc) {
    uint32_t vin[3];
    fetch_triangle_indices(D, tri, vin);
    return shade_triangle_program(D, vin, pxc, pyc);
}

// a8: Cook-Torrance GGX, shaders/hlsl/pbr.hlsli; the directional light's shadow term in its own raster variant (shade_pbr<true>)
#define PBR_PI 3.14159265358979323846f
#define PBR_EPSILON 0.0001f
__device__ __forceinline__ float max0(float x) { return x > 0.0f ? x : 0.0f; }
__device__ __forceinline__ float distribution_ggx(float NdotH, float roughness) {       // pbr.hlsli:55-69
    const float a = roughness * roughness, a2 = a * a;
    const float NdotH2 = NdotH * NdotH;
    float denom = NdotH2 * (a2 - 1.0f) + 1.0f;
    denom = (PBR_PI * denom) * denom;
    return div_rn_nb(a2, denom > PBR_EPSILON ? denom : PBR_EPSILON);
}
__device__ __forceinline__ float geometry_schlick_ggx(float NdotV, float roughness) {   // pbr.hlsli:83-93
    const float r = roughness + 1.0f;
    const float k = (r * r) * 0.125f;              // (exact: a power of two)
    const float denom = NdotV * (1.0f - k) + k;
    return div_rn_nb(NdotV, denom > PBR_EPSILON ? denom : PBR_EPSILON);
}
struct PbrMaterial { f3 albedo; float metallic, roughness; };
__device__ __forceinline__ f3 pbr_direct(f3 N, f3 V, f3 L, f3 radiance, const PbrMaterial& m) {   // pbr.hlsli:292-333
    const f3 H = normalize3(add3(V, L));
    const f3 F0 = {0.04f + (m.albedo.x - 0.04f) * m.metallic, 0.04f + (m.albedo.y - 0.04f) * m.metallic,
                   0.04f + (m.albedo.z - 0.04f) * m.metallic};
    const float NDF = distribution_ggx(max0(dot3(N, H)), m.roughness);
    const float NdotV = max0(dot3(N, V)), NdotL = max0(dot3(N, L));
    const float G = geometry_schlick_ggx(NdotV, m.roughness) * geometry_schlick_ggx(NdotL, m.roughness);
    const float ct = saturatef(max0(dot3(H, V)));
    const float p5 = fpow(1.0f - ct, 5.0f);                                             // FresnelSchlick :131-136
    const f3 F = {F0.x + (1.0f - F0.x) * p5, F0.y + (1.0f - F0.y) * p5, F0.z + (1.0f - F0.z) * p5};
    const float om = 1.0f - m.metallic;
    const f3 kD = {(1.0f - F.x) * om, (1.0f - F.y) * om, (1.0f - F.z) * om};
    const float ndg = NDF * G;
    const float denominator = (4.0f * NdotV) * NdotL + PBR_EPSILON;
    const f3 specular = {div_rn_nb(ndg * F.x, denominator), div_rn_nb(ndg * F.y, denominator), div_rn_nb(ndg * F.z, denominator)};
    return {((div_rn_nb(kD.x * m.albedo.x, PBR_PI) + specular.x) * radiance.x) * NdotL,
            ((div_rn_nb(kD.y * m.albedo.y, PBR_PI) + specular.y) * radiance.y) * NdotL,
            ((div_rn_nb(kD.z * m.albedo.z, PBR_PI) + specular.z) * radiance.z) * NdotL};
}

// alpha the Cook-Torrance program compares with alphaCutoff (pixel/model_pbr.hlsl:166-179) at one pixel of a draw with a base colour
// texture: the same barycentrics, (u, v), footprint and lookup as shade_model_program / shade_pbr, so the same bits (default sampler only: a scope
// with a draw under another sampler is resolved by the ordered kernel, classify_scope)
__device__ __forceinline__ float pbr_base_alpha(DrawRef D, const f4 c[3], const float uvk[3][2], float pxc, float pyc) {
    float b[3];
    barycentrics<false>(D, c, pxc, pyc, b);
    float u = 0.0f, v = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) { acc1(u, b[k], uvk[k][0], k); acc1(v, b[k], uvk[k][1], k); }
    UvGrad grad = {0.0f, 0.0f, 0.0f, 0.0f};
    if (D.tex_any_mips) {
        float bx[3], by[3];
        barycentrics<false>(D, c, pxc + 1.0f, pyc, bx);
        barycentrics<false>(D, c, pxc, pyc + 1.0f, by);
        grad.dudx = ((bx[0] * uvk[0][0] + bx[1] * uvk[1][0]) + bx[2] * uvk[2][0]) - u;
        grad.dvdx = ((bx[0] * uvk[0][1] + bx[1] * uvk[1][1]) + bx[2] * uvk[2][1]) - v;
        grad.dudy = ((by[0] * uvk[0][0] + by[1] * uvk[1][0]) + by[2] * uvk[2][0]) - u;
        grad.dvdy = ((by[0] * uvk[0][1] + by[1] * uvk[1][1]) + by[2] * uvk[2][1]) - v;
    }
    return sample_texture<true, false>(D, 0, u, v, grad).w * ldcf(cb(D.material), 12);
}
// true if the draw's fragments have to be alpha-tested one by one: MODEL_PBR with a base colour texture whose texel alpha (in [0, 1]
// times baseColorFactor.a) can fall on both sides of alphaCutoff -- the decision geometry_body takes per draw otherwise
__device__ __forceinline__ bool draw_needs_alpha_test(DrawRef D) {
    if (D.program != 3u) return false;      // (MODEL_PBR_IBL, program 5, has the same discard but its pipelines refuse fragment_discard_enable: no masked
                                            // scope holds one.  A masked IBL form would have to be let through here, as geometry_body's per-draw decision is.)
    const CBytePtr M = cb(D.material);
    const float fa = ldcf(M, 12), cutoff = ldcf(M, 44);
    if (ldcu(M, 48) == 0u) return false;
    const float lo = fa < 0.0f ? fa : 0.0f, hi = fa > 0.0f ? fa : 0.0f;
    return !(hi < cutoff) && !(lo >= cutoff);
}

// CalculateShadow (shaders/hlsl/shadow.hlsli:49-121), line for line.  ShadowParams (shadow.hlsli:20-30) at D.shadow_data: LightSpaceMatrix @0,
// ShadowBias @64, NormalBias @68, ShadowMapSize @72, ShadowStrength @80 -- wave-uniform, scalar loads once per draw.  The comparison sampler is
// this build's (sampler.rs is empty, include/mirhi.h MIRHI_TEXTURE_SHADOW_MAP): LESS_OR_EQUAL against the reference depth clamped to [0, 1],
// nearest texel, clamp-to-edge.
__device__ __forceinline__ float shadow_tap(DrawRef D, float u, float v, float dref, float fw, float fh) {
    const float fi = fminf(fmaxf(floorf(u * fw), 0.0f), fw - 1.0f);          // (fmaxf(NaN, 0) = 0)
    const float fj = fminf(fmaxf(floorf(v * fh), 0.0f), fh - 1.0f);
    const float texel = D.shadow_map[(size_t)(uint32_t)fj * D.shadow_w + (uint32_t)fi];
    return dref <= texel ? 1.0f : 0.0f;
}
__device__ __forceinline__ float calculate_shadow(DrawRef D, f3 worldPos, f3 normal, f3 lightDir) {
    const CBytePtr S = cb(D.shadow_data);
    const CFloatPtr lsm = reinterpret_cast<CFloatPtr>(S);
    const f4 ls = mat4_mul(lsm, {worldPos.x, worldPos.y, worldPos.z, 1.0f});                     // :58
    float px = div_rn_nb(ls.x, ls.w), py = div_rn_nb(ls.y, ls.w);                               // :61
    const float pz = div_rn_nb(ls.z, ls.w);
    px = px * 0.5f + 0.5f; py = py * 0.5f + 0.5f;                                               // :65
    py = 1.0f - py;                                                                             // :66
    if (px < 0.0f || px > 1.0f || py < 0.0f || py > 1.0f || pz < 0.0f || pz > 1.0f) return 1.0f;   // :70-75
    const float NdotL = dot3(normal, lightDir);                                                 // :79
    const float b0 = ldcf(S, 64) * (1.0f - NdotL);                                              // :80
    const float bias = b0 > 0.0005f ? b0 : 0.0005f;
    const f3 offsetPos = add3(worldPos, scale3(normal, ldcf(S, 68)));                           // :84
    const f4 ols = mat4_mul(lsm, {offsetPos.x, offsetPos.y, offsetPos.z, 1.0f});                // :85
    float ox = div_rn_nb(ols.x, ols.w), oy = div_rn_nb(ols.y, ols.w);                           // :86
    const float oz = div_rn_nb(ols.z, ols.w);
    ox = ox * 0.5f + 0.5f; oy = oy * 0.5f + 0.5f;                                               // :87
    oy = 1.0f - oy;                                                                             // :88
    const float currentDepth = oz - bias;                                                       // :92
    const float dref = fminf(fmaxf(currentDepth, 0.0f), 1.0f);                                  // (the sampler clamps D_ref)
    const float tx = rcp_rn_nb(ldcf(S, 72)), ty = rcp_rn_nb(ldcf(S, 76));                       // :98
    const float fw = (float)D.shadow_w, fh = (float)D.shadow_h;
    float shadow = 0.0f;
#pragma unroll
    for (int x = -1; x <= 1; ++x)
#pragma unroll
        for (int y = -1; y <= 1; ++y)                                                           // :101-113
            shadow += shadow_tap(D, ox + (float)x * tx, oy + (float)y * ty, dref, fw, fh);
    shadow = div_rn_nb(shadow, 9.0f);                                                           // :116
    return 1.0f + (shadow - 1.0f) * ldcf(S, 80);                                                // :120 lerp(1, shadow, ShadowStrength)
}

// CalculateShadowCSM (shaders/hlsl/shadow_csm.hlsli:163-194) with SelectCascade (:55-71) and SampleCascadePCF (:90-146), line for line.  CSMParams
// (:23-39, 336 B) at D.shadow_data: Cascades[k].ViewProjection @80k, Cascades[k].SplitDepth @80k + 64, ShadowBias @320, NormalBias @324,
// ShadowMapSize @328.  D.shadow_map is the base of the four tightly packed layers of D.shadow_w x D.shadow_h texels; the sampler is the one of
// MIRHI_TEXTURE_SHADOW_MAP, within the selected layer (clamp-to-edge never leaves it: the texel index is clamped before the layer offset is added).
// clipSpaceDepth = SV_Position.z: the depth the raster kernel resolved for the pixel (the bits a D32 attachment stores).
// The cascade index differs from lane to lane, so the selected matrix is fetched with per-lane vector loads (four 16-byte loads from a block
// every wave of the scope keeps in cache); splits, biases and the map size stay wave-uniform scalar loads.
// SampleCascadePCF (:90-146) of one cascade, written once: CalculateShadowCSM samples the selected cascade with it, CalculateShadowCSMBlended that
// one and, in a blend region, the next.
__device__ __forceinline__ float sample_cascade_pcf(DrawRef D, CBytePtr S, uint32_t cascadeIndex, f3 worldPos, f3 normal, f3 lightDir) {
    const float4* const mp = reinterpret_cast<const float4*>(D.shadow_data + 80u * cascadeIndex);   // :176 Cascades[cascadeIndex].ViewProjection
    const float4 c0 = mp[0], c1 = mp[1], c2 = mp[2], c3 = mp[3];                                // (columns: the matrix convention of mat4_mul)
    const float texelSize = rcp_rn_nb(ldcf(S, 328));                                            // :179
    const f3 offsetPos = add3(worldPos, scale3(normal, ldcf(S, 324)));                          // :103
    const float lx = ((c0.x * offsetPos.x + c1.x * offsetPos.y) + c2.x * offsetPos.z) + c3.x * 1.0f;   // :106 (mat4_mul's operation order)
    const float ly = ((c0.y * offsetPos.x + c1.y * offsetPos.y) + c2.y * offsetPos.z) + c3.y * 1.0f;
    const float lz = ((c0.z * offsetPos.x + c1.z * offsetPos.y) + c2.z * offsetPos.z) + c3.z * 1.0f;
    const float lw = ((c0.w * offsetPos.x + c1.w * offsetPos.y) + c2.w * offsetPos.z) + c3.w * 1.0f;
    float px = div_rn_nb(lx, lw), py = div_rn_nb(ly, lw);                                       // :107
    const float pz = div_rn_nb(lz, lw);
    px = px * 0.5f + 0.5f; py = py * 0.5f + 0.5f;                                               // :110
    py = 1.0f - py;                                                                             // :111
    if (px < 0.0f || px > 1.0f || py < 0.0f || py > 1.0f || pz < 0.0f || pz > 1.0f) return 1.0f;   // :114-119
    const float NdotL = dot3(normal, lightDir);                                                 // :122
    const float b0 = ldcf(S, 320) * (1.0f - NdotL);                                             // :123
    const float adaptiveBias = b0 > 0.0005f ? b0 : 0.0005f;
    const float currentDepth = pz - adaptiveBias;                                               // :124
    const float dref = fminf(fmaxf(currentDepth, 0.0f), 1.0f);                                  // (the sampler clamps D_ref)
    const float fw = (float)D.shadow_w, fh = (float)D.shadow_h;
    const float* const layer = D.shadow_map + (size_t)cascadeIndex * D.shadow_w * D.shadow_h;   // :136 sampleUVW.z
    float shadow = 0.0f;
#pragma unroll
    for (int x = -1; x <= 1; ++x)
#pragma unroll
        for (int y = -1; y <= 1; ++y) {                                                         // :130-143
            const float u = px + (float)x * texelSize, v = py + (float)y * texelSize;
            const float fi = fminf(fmaxf(floorf(u * fw), 0.0f), fw - 1.0f);                     // (shadow_tap's addressing, within the layer)
            const float fj = fminf(fmaxf(floorf(v * fh), 0.0f), fh - 1.0f);
            shadow += dref <= layer[(uint32_t)fj * D.shadow_w + (uint32_t)fi] ? 1.0f : 0.0f;
        }
    return div_rn_nb(shadow, 9.0f);                                                             // :145
}
__device__ __forceinline__ uint32_t select_cascade(CBytePtr S, float clipSpaceDepth) {
    uint32_t cascadeIndex = 0;                                                                  // :57
#pragma unroll
    for (uint32_t i = 0; i < 3u; ++i)                                                           // :62-68 (the last split passed, not the first)
        if (clipSpaceDepth > ldcf(S, 80u * i + 64u)) cascadeIndex = i + 1u;
    return cascadeIndex;
}
__device__ __forceinline__ float calculate_shadow_csm(DrawRef D, f3 worldPos, f3 normal, f3 lightDir, float clipSpaceDepth) {
    const CBytePtr S = cb(D.shadow_data);
    return sample_cascade_pcf(D, S, select_cascade(S, clipSpaceDepth), worldPos, normal, lightDir);
}
// CalculateShadowCSMBlended (shadow_csm.hlsli:212-277), line for line: the primary cascade's PCF and, for a lane within blendThreshold of its
// cascade's range in front of the split, the next cascade's, blended by the distance to the split.  Cascade index and blend region are per
// lane, so the second sample is a divergent branch with a second per-lane matrix fetch.  One PCF body walked at most twice (the first trip's result
// is carried in one register), not two inlined copies: the kernel keeps the registers of raster_kernel_csm.  blendThreshold 0 (an
// unblended draw in a blended scope): blendRegion = 0, no lane takes the second trip, the bits of calculate_shadow_csm.
__device__ __forceinline__ float calculate_shadow_csm_blended(DrawRef D, f3 worldPos, f3 normal, f3 lightDir, float clipSpaceDepth, float blendThreshold) {
    const CBytePtr S = cb(D.shadow_data);
    const uint32_t cascadeIndex = select_cascade(S, clipSpaceDepth);                            // :223
    const float s0 = ldcf(S, 64u), s1 = ldcf(S, 144u), s2 = ldcf(S, 224u);
    const float splitDepth = cascadeIndex == 0u ? s0 : (cascadeIndex == 1u ? s1 : s2);          // :244 (read under cascadeIndex < 3 only)
    const float prevSplit = cascadeIndex == 0u ? 0.0f : (cascadeIndex == 1u ? s0 : s1);         // :245-246
    const float cascadeRange = splitDepth - prevSplit;                                          // :247
    const float blendRegion = cascadeRange * blendThreshold;                                    // :248
    const float distanceToEdge = splitDepth - clipSpaceDepth;                                   // :251
    const bool blend = cascadeIndex < 3u && distanceToEdge < blendRegion && distanceToEdge > 0.0f;   // :242, :253
    float shadow = 0.0f;
    uint32_t index = cascadeIndex;
#pragma nounroll
    for (uint32_t trip = 0u;; ++trip) {
        const float s = sample_cascade_pcf(D, S, index, worldPos, normal, lightDir);            // :228-239, :258-269
        if (trip != 0u) {
            const float blendFactor = div_rn_nb(distanceToEdge, blendRegion);                   // :255
            shadow = s + blendFactor * (shadow - s);                                            // :272 lerp(nextShadow, shadow, blendFactor)
            break;
        }
        shadow = s;
        if (!blend) break;
        index = cascadeIndex + 1u;
    }
    return shadow;                                                                              // :276
}

// The Cook-Torrance programs, pixel/model_pbr.hlsl:159-320 and pixel/model_pbr_ibl.hlsl:199-396 / model_pbr_ibl_csm.hlsl, after the shared varying
// interpolation.  The two files share their front half (material factors and the five textures, GetWorldNormal, ClampRoughness: pbr_surface) and
// the three light loops with the directional light's shadow term (pbr_direct_lighting); they differ in the ambient term and the final sum
// (shade_pbr / shade_pbr_ibl).
struct PbrSurface { PbrMaterial m; f3 N, emissive; float ao, alpha; };
// model_pbr.hlsl:159-236 = model_pbr_ibl.hlsl:205-262: N comes in as the normalised vertex normal and leaves as GetWorldNormal's
__device__ __forceinline__ PbrSurface pbr_surface(DrawRef D, const float b[3], const uint32_t vi[3], float u, float v, f3 N, const UvGrad& grad) {
    const CBytePtr M = cb(D.material);                                                  // MaterialData :36-59 (80 B)
    f4 baseColor = {ldcf(M, 0), ldcf(M, 4), ldcf(M, 8), ldcf(M, 12)};
    float metallic = ldcf(M, 16), roughness = ldcf(M, 20), ao = ldcf(M, 24);
    const float normalScale = ldcf(M, 28);
    f3 emissive = {ldcf(M, 32), ldcf(M, 36), ldcf(M, 40)};
    if (ldcu(M, 48) != 0u) {
        const f4 t = sample_texture<true>(D, 0, u, v, grad);
        baseColor = {t.x * baseColor.x, t.y * baseColor.y, t.z * baseColor.z, t.w * baseColor.w};
    }
    if (ldcu(M, 56) != 0u) {
        const f4 t = sample_texture<true>(D, 2, u, v, grad);
        roughness = roughness * t.y; metallic = metallic * t.z;
    }
    if (ldcu(M, 60) != 0u) ao = ao * sample_texture<true>(D, 3, u, v, grad).x;
    if (ldcu(M, 64) != 0u) {
        const f4 t = sample_texture<true>(D, 4, u, v, grad);
        emissive = {emissive.x * t.x, emissive.y * t.y, emissive.z * t.z};
    }
    if (ldcu(M, 52) != 0u) {                                                            // GetWorldNormal :124-151
        const f4 nc = sample_texture<true>(D, 1, u, v, grad);
        const f3 ncm1 = {nc.x - 1.0f, nc.y - 1.0f, nc.z - 1.0f};
        if (!(length3(ncm1) < 0.01f)) {
            const f3 ns = normalize3({(nc.x * 2.0f - 1.0f) * normalScale, (nc.y * 2.0f - 1.0f) * normalScale, nc.z * 2.0f - 1.0f});
            f3 Ti, Bi;
            interp_tangent_frame(D, vi, b, Ti, Bi);
            const f3 T = normalize3(Ti), Bt = normalize3(Bi);
            N = normalize3(add3(add3(scale3(T, ns.x), scale3(Bt, ns.y)), scale3(N, ns.z)));
        }
    }
    PbrSurface s;
    s.m.albedo = {baseColor.x, baseColor.y, baseColor.z};
    s.m.metallic = metallic;
    s.m.roughness = roughness > 0.04f ? roughness : 0.04f;                              // ClampRoughness :476-479
    s.N = N; s.emissive = emissive; s.ao = ao; s.alpha = baseColor.w;
    return s;
}
// Lo of model_pbr.hlsl:229-305 = model_pbr_ibl.hlsl:275-346 (model_pbr_ibl_csm.hlsl:275-347).  SHADOW 1: the directional light's shadow term
// (model_pbr.hlsl:238-251) for draws with a shadow map bound; 2: CalculateShadowCSM instead (pixel/model_pbr_ibl_csm.hlsl:280-298) for draws with
// cascades bound, clipz = SV_Position.z; 3: CalculateShadowCSMBlended for scopes with a blended cascaded draw (DrawDesc::csm_blend)
template <int SHADOW>
__device__ __forceinline__ f3 pbr_direct_lighting(DrawRef D, f3 worldPos, f3 V, f3 N, const PbrMaterial& m, float clipz) {
    f3 lighting = {0.0f, 0.0f, 0.0f};
    {
        const f3 dir = {ldcf(cb(D.lights), 0), ldcf(cb(D.lights), 4), ldcf(cb(D.lights), 8)};
        const float intensity = ldcf(cb(D.lights), 12);
        const f3 color = {ldcf(cb(D.lights), 16), ldcf(cb(D.lights), 20), ldcf(cb(D.lights), 24)};
        if (!SHADOW || !D.shadow_map) {
            if (intensity != 0.0f) lighting = add3(lighting, pbr_direct(N, V, normalize3({-dir.x, -dir.y, -dir.z}), scale3(color, intensity), m));
        } else if (intensity != 0.0f) {                                                  // (intensity 0: exact zeros, shadow or not)
            const f3 L = normalize3({-dir.x, -dir.y, -dir.z});
            const float shadow = SHADOW == 3 ? calculate_shadow_csm_blended(D, worldPos, N, L, clipz, D.csm_blend)      // (:212-277 in the place of :163-194)
                               : SHADOW == 2 ? calculate_shadow_csm(D, worldPos, N, L, clipz)      // model_pbr_ibl_csm.hlsl:285-293
                                             : calculate_shadow(D, worldPos, N, L);                // model_pbr.hlsl:238-245
            lighting = add3(lighting, scale3(pbr_direct(N, V, L, scale3(color, intensity), m), shadow));   // :251
        }
    }
    const uint32_t numPoint = D.point_lights ? ldcu(cb(D.lights), 32) : 0u;
    const uint32_t numSpot = D.spot_lights ? ldcu(cb(D.lights), 36) : 0u;
    for (uint32_t i = 0; i < numPoint; i++) {
        const CBytePtr Lp = cb(D.point_lights) + 32u * i;
        const f3 pos = {ldcf(Lp, 0), ldcf(Lp, 4), ldcf(Lp, 8)};
        const float radius = ldcf(Lp, 12);
        const f3 color = {ldcf(Lp, 16), ldcf(Lp, 20), ldcf(Lp, 24)};
        const float intensity = ldcf(Lp, 28);
        const f3 lv = sub3(pos, worldPos);
        const float dist = length3(lv);
        const float att = attenuation(dist, radius);
        if (__ballot(att > 0.0f) == 0ull) continue;                          // out of the light's reach: exact zeros (see model_full)
        const f3 L = scale3(lv, rcp_rn_nb(dist));
        lighting = add3(lighting, pbr_direct(N, V, L, scale3(scale3(color, intensity), att), m));
    }
    for (uint32_t j = 0; j < numSpot; j++) {
        const CBytePtr Ls = cb(D.spot_lights) + 48u * j;
        const f3 pos = {ldcf(Ls, 0), ldcf(Ls, 4), ldcf(Ls, 8)};
        const float innerCos = ldcf(Ls, 12);
        const f3 sdir = {ldcf(Ls, 16), ldcf(Ls, 20), ldcf(Ls, 24)};
        const float outerCos = ldcf(Ls, 28);
        const f3 color = {ldcf(Ls, 32), ldcf(Ls, 36), ldcf(Ls, 40)};
        const float intensity = ldcf(Ls, 44);
        const f3 lv = sub3(pos, worldPos);
        const float dist = length3(lv);
        const f3 L = scale3(lv, rcp_rn_nb(dist));
        const float datt = attenuation(dist, 50.0f);
        const f3 sd = normalize3(sdir);
        const float cosAngle = dot3({-L.x, -L.y, -L.z}, sd);
        const float satt = saturatef(div_rn_nb(cosAngle - outerCos, innerCos - outerCos));
        if (__ballot(datt * satt > 0.0f) == 0ull) continue;
        lighting = add3(lighting, pbr_direct(N, V, L, scale3(scale3(scale3(color, intensity), datt), satt), m));
    }
    return lighting;
}
template <int SHADOW = 0>
__device__ __forceinline__ f4 shade_pbr(DrawRef D, const float b[3], const uint32_t vi[3], float u, float v, f3 worldPos, f3 V, f3 N, const UvGrad& grad, float clipz = 0.0f) {
    const PbrSurface s = pbr_surface(D, b, vi, u, v, N, grad);
    const PbrMaterial& m = s.m;
    N = s.N;
    const float ao = s.ao;
    f3 lighting = pbr_direct_lighting<SHADOW>(D, worldPos, V, N, m, clipz);
    const float up = N.y * 0.5f + 0.5f;                                                 // CalculateHemisphereAmbient pbr.hlsli:483-492
    const f3 amb = {0.08f + (0.15f - 0.08f) * up, 0.06f + (0.18f - 0.06f) * up, 0.04f + (0.25f - 0.04f) * up};
    const float om = 1.0f - m.metallic;
    const f3 ambient = scale3(scale3(mul3(amb, m.albedo), ao), om);
    lighting = scale3(lighting, 1.0f + (ao - 1.0f) * 0.5f);                             // lerp(1, ao, 0.5) :311
    const f3 col = add3(add3(ambient, lighting), s.emissive);
    return {col.x, col.y, col.z, s.alpha};
}

// The ambient term of pixel/model_pbr_ibl.hlsl:355-384 (include/mirhi.h, "MODEL_PBR_IBL"): irradianceMap.Sample(N), prefilteredMap.SampleLevel(R,
// roughness * MAX_REFLECTION_LOD) and brdfLUT.Sample((NdotV, roughness)) with the sampler of mirhi_ibl_sample.hip.h -- the lookups are the precompute
// kernels' own functions.  The set is per scope: base pointers, sizes and the level count come from the parameter block through scalar loads.
// Sixteen 16-byte gathers per pixel (4 irradiance, 2 x 4 prefiltered, 4 LUT): every address is computed and every load issued before the first
// texel is used, so the sixteen are in flight together; both prefiltered levels are always fetched (floor(lod) and the next, clamped to the last:
// a fraction of 0 returns the first one unchanged), which keeps the sequence free of branches.  Tolerance-checked against the float64 model of
// renderer-rs_amd/ibl.py like the precompute passes, not on the oracle's bit-exact path: this function contracts.
__device__ __forceinline__ f3 ibl_ambient(ParamsPtr R, f3 N, f3 V, const PbrMaterial& m, float ao) {
    #pragma clang fp contract(fast)
    const float4* const irr = reinterpret_cast<const float4*>(R->ibl_irradiance);
    const float4* const pre = reinterpret_cast<const float4*>(R->ibl_prefiltered);
    const float4* const lut = reinterpret_cast<const float4*>(R->ibl_lut);
    const uint32_t irr_n = R->ibl_irr_size, pre_n = R->ibl_pre_size, pre_levels = R->ibl_pre_levels, lut_n = R->ibl_lut_size;
    const float ndv_raw = dot3(N, V);
    const float NdotV = max0(ndv_raw);                                                  // :359
    const f3 Rv = {2.0f * ndv_raw * N.x - V.x, 2.0f * ndv_raw * N.y - V.y, 2.0f * ndv_raw * N.z - V.z};      // :259 reflect(-V, N)
    // addresses
    const IblFaceUV fn = ibl_select_face(N.x, N.y, N.z);                               // :369 (lod 0: the one level)
    const IblTaps ki = ibl_bilinear_taps(irr_n, fn.s, fn.t);
    const float4* const pi = irr + fn.face * irr_n * irr_n;
    const IblFaceUV fr = ibl_select_face(Rv.x, Rv.y, Rv.z);                            // :373-377
    const float lod = fminf(fmaxf(m.roughness * 7.0f, 0.0f), (float)(pre_levels - 1u));    // MAX_REFLECTION_LOD pbr.hlsli:373; the sampler's clamp
    const float l0f = floorf(lod), frac = lod - l0f;
    const uint32_t l0 = min((uint32_t)(int)l0f, pre_levels - 1u), l1 = min(l0 + 1u, pre_levels - 1u);
    const uint32_t n0 = pre_n >> l0, n1 = pre_n >> l1;
    const IblTaps k0 = ibl_bilinear_taps(n0, fr.s, fr.t), k1 = ibl_bilinear_taps(n1, fr.s, fr.t);
    const float4* const p0 = pre + ibl_level_offset(pre_n, l0) + fr.face * n0 * n0;
    const float4* const p1 = pre + ibl_level_offset(pre_n, l1) + fr.face * n1 * n1;
    const IblTaps kl = ibl_bilinear_taps(lut_n, NdotV, m.roughness);                   // :380 (u = NdotV: column, v = roughness: row)
    // the sixteen loads
    const float4 ia = pi[ki.o00], ib = pi[ki.o10], ic = pi[ki.o01], id = pi[ki.o11];
    const float4 pa = p0[k0.o00], pb = p0[k0.o10], pc = p0[k0.o01], pd = p0[k0.o11];
    const float4 qa = p1[k1.o00], qb = p1[k1.o10], qc = p1[k1.o01], qd = p1[k1.o11];
    const float4 la = lut[kl.o00], lb = lut[kl.o10], lc = lut[kl.o01], ld = lut[kl.o11];
    // filters
    const float4 irradiance = ibl_bilinear_filter(ki, ia, ib, ic, id);
    const float4 prefiltered = ibl_lerp4(ibl_bilinear_filter(k0, pa, pb, pc, pd), ibl_bilinear_filter(k1, qa, qb, qc, qd), frac);
    const float4 brdf = ibl_bilinear_filter(kl, la, lb, lc, ld);
    const f3 F0 = {0.04f + (m.albedo.x - 0.04f) * m.metallic, 0.04f + (m.albedo.y - 0.04f) * m.metallic, 0.04f + (m.albedo.z - 0.04f) * m.metallic};   // :356
    const float o = 1.0f - saturatef(NdotV), o2 = o * o, p5 = o2 * o2 * o;              // FresnelSchlickRoughness pbr.hlsli:147-152
    const float r1 = 1.0f - m.roughness, om = 1.0f - m.metallic;
    const f3 F = {F0.x + (fmaxf(r1, F0.x) - F0.x) * p5, F0.y + (fmaxf(r1, F0.y) - F0.y) * p5, F0.z + (fmaxf(r1, F0.z) - F0.z) * p5};
    const f3 kD = {(1.0f - F.x) * om, (1.0f - F.y) * om, (1.0f - F.z) * om};           // :365-366
    return {(kD.x * (irradiance.x * m.albedo.x) + prefiltered.x * (F0.x * brdf.x + brdf.y)) * ao,      // :370, :381, :384
            (kD.y * (irradiance.y * m.albedo.y) + prefiltered.y * (F0.y * brdf.x + brdf.y)) * ao,
            (kD.z * (irradiance.z * m.albedo.z) + prefiltered.z * (F0.z * brdf.x + brdf.y)) * ao};
}
// ... in a scope whose IBL set has a seamless cube (PassParams::ibl_seamless != 0, raster_kernel_ibl_seamless): the same sequence -- every
// address, then the sixteen loads, then the filters -- with the seamless taps of mirhi_ibl_sample.hip.h for the two cubes.  A function of its own, so that
// ibl_ambient above stays, instruction for instruction, what the non-seamless kernels ran before.
__device__ __forceinline__ f3 ibl_ambient_seamless(ParamsPtr R, f3 N, f3 V, const PbrMaterial& m, float ao) {
    #pragma clang fp contract(fast)
    const float4* const irr = reinterpret_cast<const float4*>(R->ibl_irradiance);
    const float4* const pre = reinterpret_cast<const float4*>(R->ibl_prefiltered);
    const float4* const lut = reinterpret_cast<const float4*>(R->ibl_lut);
    const uint32_t irr_n = R->ibl_irr_size, pre_n = R->ibl_pre_size, pre_levels = R->ibl_pre_levels, lut_n = R->ibl_lut_size;
    const uint32_t seam = R->ibl_seamless;      // (wave-uniform: bit 0 the irradiance cube's state, bit 1 the prefiltered cube's)
    const float ndv_raw = dot3(N, V);
    const float NdotV = max0(ndv_raw);                                                  // :359
    const f3 Rv = {2.0f * ndv_raw * N.x - V.x, 2.0f * ndv_raw * N.y - V.y, 2.0f * ndv_raw * N.z - V.z};      // :259 reflect(-V, N)
    // addresses
    const IblFaceUV fn = ibl_select_face(N.x, N.y, N.z);                               // :369 (lod 0: the one level)
    const IblSeamTaps ki = ibl_seamless_taps(irr_n, fn.face, fn.s, fn.t, (seam & 1u) != 0u);
    const float4* const pi = irr;      // (a seamless tap's offset counts from the level's first texel: it may lie in another face)
    const IblFaceUV fr = ibl_select_face(Rv.x, Rv.y, Rv.z);                            // :373-377
    const float lod = fminf(fmaxf(m.roughness * 7.0f, 0.0f), (float)(pre_levels - 1u));    // MAX_REFLECTION_LOD pbr.hlsli:373; the sampler's clamp
    const float l0f = floorf(lod), frac = lod - l0f;
    const uint32_t l0 = min((uint32_t)(int)l0f, pre_levels - 1u), l1 = min(l0 + 1u, pre_levels - 1u);
    const uint32_t n0 = pre_n >> l0, n1 = pre_n >> l1;
    const IblSeamTaps k0 = ibl_seamless_taps(n0, fr.face, fr.s, fr.t, (seam & 2u) != 0u), k1 = ibl_seamless_taps(n1, fr.face, fr.s, fr.t, (seam & 2u) != 0u);
    const float4* const p0 = pre + ibl_level_offset(pre_n, l0);
    const float4* const p1 = pre + ibl_level_offset(pre_n, l1);
    const IblTaps kl = ibl_bilinear_taps(lut_n, NdotV, m.roughness);                   // :380 (u = NdotV: column, v = roughness: row)
    // the sixteen loads
    const float4 ia = pi[ki.o00], ib = pi[ki.o10], ic = pi[ki.o01], id = pi[ki.o11];
    const float4 pa = p0[k0.o00], pb = p0[k0.o10], pc = p0[k0.o01], pd = p0[k0.o11];
    const float4 qa = p1[k1.o00], qb = p1[k1.o10], qc = p1[k1.o01], qd = p1[k1.o11];
    const float4 la = lut[kl.o00], lb = lut[kl.o10], lc = lut[kl.o01], ld = lut[kl.o11];
    // filters
    const float4 irradiance = ibl_seamless_filter(ki, ia, ib, ic, id);
    const float4 prefiltered = ibl_lerp4(ibl_seamless_filter(k0, pa, pb, pc, pd), ibl_seamless_filter(k1, qa, qb, qc, qd), frac);
    const float4 brdf = ibl_bilinear_filter(kl, la, lb, lc, ld);
    const f3 F0 = {0.04f + (m.albedo.x - 0.04f) * m.metallic, 0.04f + (m.albedo.y - 0.04f) * m.metallic, 0.04f + (m.albedo.z - 0.04f) * m.metallic};   // :356
    const float o = 1.0f - saturatef(NdotV), o2 = o * o, p5 = o2 * o2 * o;              // FresnelSchlickRoughness pbr.hlsli:147-152
    const float r1 = 1.0f - m.roughness, om = 1.0f - m.metallic;
    const f3 F = {F0.x + (fmaxf(r1, F0.x) - F0.x) * p5, F0.y + (fmaxf(r1, F0.y) - F0.y) * p5, F0.z + (fmaxf(r1, F0.z) - F0.z) * p5};
    const f3 kD = {(1.0f - F.x) * om, (1.0f - F.y) * om, (1.0f - F.z) * om};           // :365-366
    return {(kD.x * (irradiance.x * m.albedo.x) + prefiltered.x * (F0.x * brdf.x + brdf.y)) * ao,      // :370, :381, :384
            (kD.y * (irradiance.y * m.albedo.y) + prefiltered.y * (F0.y * brdf.x + brdf.y)) * ao,
            (kD.z * (irradiance.z * m.albedo.z) + prefiltered.z * (F0.z * brdf.x + brdf.y)) * ao};
}
// pixel/model_pbr_ibl.hlsl:199-396 (SHADOW 0 / 1) and pixel/model_pbr_ibl_csm.hlsl (SHADOW 2): color = ambient + Lo + emissive (:393) -- no hemisphere
// ambient, and Lo is NOT scaled by lerp(1, ao, 0.5), which is model_pbr.hlsl's alone
template <int SHADOW, bool SEAMLESS = false>
__device__ __forceinline__ f4 shade_pbr_ibl(DrawRef D, ParamsPtr R, const float b[3], const uint32_t vi[3], float u, float v, f3 worldPos, f3 V, f3 N, const UvGrad& grad, float clipz) {
    const PbrSurface s = pbr_surface(D, b, vi, u, v, N, grad);
    const f3 Lo = pbr_direct_lighting<SHADOW>(D, worldPos, V, s.N, s.m, clipz);
    f3 ambient;
    if constexpr (SEAMLESS) ambient = ibl_ambient_seamless(R, s.N, V, s.m, s.ao);
    else ambient = ibl_ambient(R, s.N, V, s.m, s.ao);
    const f3 col = add3(add3(ambient, Lo), s.emissive);
    return {col.x, col.y, col.z, s.alpha};
}

// FULL: the variant that also carries the Cook-Torrance program and mip-mapped (trilinear) sampling; SHADOW: and the shadow term (shade_pbr); IBL: and MODEL_PBR_IBL (shade_pbr_ibl,
// R = the scope's parameter block, where the IBL set lives; IBL = 2: with the seamless cube lookups, ibl_ambient_seamless)
template <bool FULL, int SHADOW = 0, int IBL = 0>
__device__ __forceinline__ f4 shade_model_program(DrawRef D, const uint32_t vi[3], float pxc, float pyc, float clipz = 0.0f, ParamsPtr R = nullptr) {
    f4 c[3];
    const bool full = D.program >= 2;
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        // vertex/model.hlsl outputs, computed once per vertex by vertex_kernel: the clip position first
        const uint4 w0 = reinterpret_cast<const uint4*>(D.vs_out)[vi[k]];
        c[k] = {__uint_as_float(w0.x), __uint_as_float(w0.y), __uint_as_float(w0.z), __uint_as_float(w0.w)};
    }
    float b[3];
    barycentrics<false>(D, c, pxc, pyc, b);
    f3 worldPos = {0.0f, 0.0f, 0.0f}, Nv = {0.0f, 0.0f, 0.0f};
    float u = 0.0f, v = 0.0f, uvk[3][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
        const uint4* sv = reinterpret_cast<const uint4*>(D.vs_attr) + (size_t)vi[k] * (D.vs_words - 1u) - 1;     // (sv[1..]: the attribute words)
        const uint4 w1 = sv[1], w2 = sv[2];
        acc3(worldPos, b[k], {__uint_as_float(w1.x), __uint_as_float(w1.y), __uint_as_float(w1.z)}, k);
        acc3(Nv, b[k], {__uint_as_float(w1.w), __uint_as_float(w2.x), __uint_as_float(w2.y)}, k);
        if (full) {
            uvk[k][0] = __uint_as_float(w2.z); uvk[k][1] = __uint_as_float(w2.w);
            acc1(u, b[k], uvk[k][0], k); acc1(v, b[k], uvk[k][1], k);
        }
    }
    const CFloatPtr cam = cf(D.camera);
    const f3 camPos = {cam[48], cam[49], cam[50]};          // cameraPosition @192 B
    const f3 V = normalize3(sub3(camPos, worldPos));
    f3 N = normalize3(Nv);

    if (!full) {                                                             // pixel/model.hlsl:29-82
        const f3 albedo = {0.7f, 0.7f, 0.7f};
        const f3 one = {1.0f, 1.0f, 1.0f};
        // normalize((1, 1, 1)) is a constant: RN(1 / RN(sqrt(3))) = 0x1.279a740000000p-1 (the oracle's two roundings), not recomputed per pixel
        const float inv_len = 0x1.279a740000000p-1f;
        const f3 L = {1.0f * inv_len, 1.0f * inv_len, 1.0f * inv_len};
        const f3 ambient = scale3(scale3(albedo, 0.03f), 1.0f);
        const f3 lighting = blinn_phong(L, V, N, one, albedo, roughness_to_shininess(0.5f));
        const f3 col = add3(ambient, lighting);
        return {col.x, col.y, col.z, 1.0f};
    }
    // Mip-mapped textures need the screen-space footprint of (u, v): the same perspective-correct interpolation one pixel
    // to the right and one pixel down (exact for a planar triangle; no quad, no neighbour lane needed)
    UvGrad grad = {0.0f, 0.0f, 0.0f, 0.0f};
    if (FULL && D.tex_any_mips) {
        float bx[3], by[3];
        barycentrics<false>(D, c, pxc + 1.0f, pyc, bx);
        barycentrics<false>(D, c, pxc, pyc + 1.0f, by);
        grad.dudx = ((bx[0] * uvk[0][0] + bx[1] * uvk[1][0]) + bx[2] * uvk[2][0]) - u;
        grad.dvdx = ((bx[0] * uvk[0][1] + bx[1] * uvk[1][1]) + bx[2] * uvk[2][1]) - v;
        grad.dudy = ((by[0] * uvk[0][0] + by[1] * uvk[1][0]) + by[2] * uvk[2][0]) - u;
        grad.dvdy = ((by[0] * uvk[0][1] + by[1] * uvk[1][1]) + by[2] * uvk[2][1]) - v;
    }
    if constexpr (IBL != 0) { if (D.program == 5) return shade_pbr_ibl<SHADOW, IBL == 2>(D, R, b, vi, u, v, worldPos, V, N, grad, clipz); }
    if (FULL && D.program == 3) return shade_pbr<SHADOW>(D, b, vi, u, v, worldPos, V, N, grad, clipz);
    // pixel/model_full.hlsl:85-150
    const f4 baseColor = {ldcf(cb(D.material), 0), ldcf(cb(D.material), 4), ldcf(cb(D.material), 8), ldcf(cb(D.material), 12)};
    const float roughness = ldcf(cb(D.material), 20), ao = ldcf(cb(D.material), 24);
    const f4 albedoSample = sample_texture<FULL>(D, 0, u, v, grad);
    const f3 albedo = {albedoSample.x * baseColor.x, albedoSample.y * baseColor.y, albedoSample.z * baseColor.z};
    const f4 nc = sample_texture<FULL>(D, 1, u, v, grad);
    const f3 ncm1 = {nc.x - 1.0f, nc.y - 1.0f, nc.z - 1.0f};
    const bool hasNormalMap = length3(ncm1) > 0.01f;                          // :94-95
    if (hasNormalMap) {                                                      // GetWorldNormal :63-83
        const f3 ns = {nc.x * 2.0f - 1.0f, nc.y * 2.0f - 1.0f, nc.z * 2.0f - 1.0f};
        f3 Ti, Bi;
        interp_tangent_frame(D, vi, b, Ti, Bi);
        const f3 T = normalize3(Ti), Bt = normalize3(Bi);
        N = normalize3(add3(add3(scale3(T, ns.x), scale3(Bt, ns.y)), scale3(N, ns.z)));
    }
    const f3 ambient = scale3(scale3(albedo, 0.03f), ao);
    f3 lighting = {0.0f, 0.0f, 0.0f};
    const float shininess = roughness_to_shininess(roughness);
    {   // CalculateDirectionalLight lights.hlsli:166-179 (HLSL DirectionalLight layout :17-23)
        const f3 dir = {ldcf(cb(D.lights), 0), ldcf(cb(D.lights), 4), ldcf(cb(D.lights), 8)};
        const float intensity = ldcf(cb(D.lights), 12);
        const f3 color = {ldcf(cb(D.lights), 16), ldcf(cb(D.lights), 20), ldcf(cb(D.lights), 24)};
        // (a light of intensity 0 adds exactly +0 to every channel: skipped, wave-uniformly -- BASELINE's Phong configs run without
        // a directional light)
        if (intensity != 0.0f) {
            const f3 L = normalize3({-dir.x, -dir.y, -dir.z});
            lighting = add3(lighting, blinn_phong(L, V, N, scale3(color, intensity), albedo, shininess));
        }
    }
    const uint32_t numPoint = D.point_lights ? ldcu(cb(D.lights), 32) : 0u;
    const uint32_t numSpot = D.spot_lights ? ldcu(cb(D.lights), 36) : 0u;
    for (uint32_t i = 0; i < numPoint; i++) {                                // CalculatePointLight :182-199
        const CBytePtr Lp = cb(D.point_lights) + 32u * i;
        const f3 pos = {ldcf(Lp, 0), ldcf(Lp, 4), ldcf(Lp, 8)};
        const float radius = ldcf(Lp, 12);
        const f3 color = {ldcf(Lp, 16), ldcf(Lp, 20), ldcf(Lp, 24)};
        const float intensity = ldcf(Lp, 28);
        const f3 lv = sub3(pos, worldPos);
        const float dist = length3(lv);
        // beyond its radius the light's falloff is exactly 0, and so is everything it adds: a wave none of whose pixels the light
        // reaches skips the rest of the iteration (the other lanes of a wave that goes on add their exact zeros)
        const float att = attenuation(dist, radius);
        if (__ballot(att > 0.0f) == 0ull) continue;
        const f3 L = scale3(lv, rcp_rn_nb(dist));
        const f3 lc = scale3(scale3(color, intensity), att);
        lighting = add3(lighting, blinn_phong(L, V, N, lc, albedo, shininess));
    }
    for (uint32_t j = 0; j < numSpot; j++) {                                 // CalculateSpotLight :202-231
        const CBytePtr Ls = cb(D.spot_lights) + 48u * j;
        const f3 pos = {ldcf(Ls, 0), ldcf(Ls, 4), ldcf(Ls, 8)};
        const float innerCos = ldcf(Ls, 12);
        const f3 sdir = {ldcf(Ls, 16), ldcf(Ls, 20), ldcf(Ls, 24)};
        const float outerCos = ldcf(Ls, 28);
        const f3 color = {ldcf(Ls, 32), ldcf(Ls, 36), ldcf(Ls, 40)};
        const float intensity = ldcf(Ls, 44);
        const f3 lv = sub3(pos, worldPos);
        const float dist = length3(lv);
        const f3 L = scale3(lv, rcp_rn_nb(dist));
        const float datt = attenuation(dist, 50.0f);
        const f3 sd = normalize3(sdir);
        const float cosAngle = dot3({-L.x, -L.y, -L.z}, sd);                // CalculateSpotAttenuation :77-81
        const float satt = saturatef(div_rn_nb(cosAngle - outerCos, innerCos - outerCos));
        if (__ballot(datt * satt > 0.0f) == 0ull) continue;                  // outside the cone or the range: exact zeros, as above
        const f3 lc = scale3(scale3(scale3(color, intensity), datt), satt);
        lighting = add3(lighting, blinn_phong(L, V, N, lc, albedo, shininess));
    }
    const f3 col = add3(ambient, lighting);
    return {col.x, col.y, col.z, albedoSample.w * baseColor.w};
}

template <bool FULL, int SHADOW = 0, int IBL = 0>
__device__ __forceinline__ f4 shade_model_program(DrawRef D, uint32_t tri, float pxc, float pyc, float clipz = 0.0f, ParamsPtr R = nullptr) {
    uint32_t vin[3];
    fetch_triangle_indices(D, tri, vin);
    return shade_model_program<FULL, SHADOW, IBL>(D, vin, pxc, pyc, clipz, R);
}

#pragma clang fp contract(fast)
// a9: sRGB OETF + UNORM8, BGRA byte order (swapchain.rs:561-570)
__device__ __forceinline__ uint32_t srgb8(float c) {
    c = saturatef(c);
    float e = (c <= 0.0031308f) ? 12.92f * c : 1.055f * __builtin_amdgcn_exp2f((1.0f / 2.4f) * __builtin_amdgcn_logf(c)) - 0.055f;
    e = saturatef(e);
    return (uint32_t)rintf(e * 255.0f);
}
__device__ __forceinline__ uint32_t pack_bgra8_srgb(f4 c) {
    return srgb8(c.z) | (srgb8(c.y) << 8) | (srgb8(c.x) << 16) | ((uint32_t)rintf(saturatef(c.w) * 255.0f) << 24);
}

#endif  // MIRHI_SHADING_HIP_H
