// mirhi_transfer.hip.h -- the kernels of the recorded transfer commands (include/mirhi.h "Transfer commands"): copies, blit, clears.
// Part of mirhi_kernels.hip's translation unit, inside namespace mirhi, behind mirhi_shading.hip.h (g_srgb_lut, unpack_rgba8, srgb8, pack_bgra8_srgb),
// mirhi_raster.hip.h (store_target) and mirhi_ordered.hip.h (unpack_bgra8_srgb).
//
// One launch per command; its regions (PassParams::xfer_regions, at most 16) are inside the launch: the work units of all regions are numbered
// through (XferRegion::first), a workgroup finds the region of its unit by comparing against these -- wave-uniform, scalar loads.
// Nothing of the workspace is touched: no counter, no page table, no status word (DESIGN.md 8g "Workspace parity").
// Every address is formed from a region the host has checked against its resource (record_transfer): lanes beyond a row, a rectangle or a range
// form no address at all.
#pragma once

typedef const MIRHI_CONST XferRegion* XferPtr;
typedef const MIRHI_CONST XferRegion& XferRef;
typedef uint32_t xfer_u32x4 __attribute__((ext_vector_type(4)));

// The colour / depth targets of a transfer are written once and not read back by the kernel: streaming stores, as the resolve's (store_target).
__device__ __forceinline__ void xfer_store16(uint8_t* p, xfer_u32x4 v) {
#ifndef MIRHI_PLAIN_TARGET_STORES
    __builtin_nontemporal_store(v, reinterpret_cast<xfer_u32x4*>(p));
#else
    *reinterpret_cast<xfer_u32x4*>(p) = v;
#endif
}

// the region that holds work unit `unit` (firsts ascend; the launch has no unit beyond the last region's)
__device__ __forceinline__ uint32_t xfer_region_of(XferPtr R, uint32_t n, uint32_t unit) {
    uint32_t r = 0u;
    for (uint32_t k = 1u; k < n; k++) r = unit >= R[k].first ? k : r;
    return r;
}

// ---- copies: raw bytes, no conversion ------------------------------------------------------------------------------------------------------
// A work unit is four steps of 256 accesses of one row: lane t of step k moves access (chunk * 4 + k) * 256 + t of the row's body -- a wave's
// 64 accesses of a step are one run of 1024 bytes (unit 16: whole 256-byte runs from a 16-byte aligned start).  The body starts where the
// destination is aligned for the unit (the source is then too: the host chose the unit so); the bytes before it and behind the last whole access
// are the first unit's lanes' to move one by one.  All loads of a lane are issued before its stores.
__global__ __launch_bounds__(RASTER_THREADS) void transfer_copy_kernel(const PassParams* __restrict__ params, const RasterHead H) {
    ParamsRef P = *(ParamsPtr)(uintptr_t)params;
    const XferPtr R = (XferPtr)(uintptr_t)P.xfer_regions;
    const uint32_t n = P.xfer_count, total = P.xfer_groups, tid = threadIdx.x;
    for (uint32_t g = blockIdx.x; g < total; g += gridDim.x) {
        XferRef G = R[xfer_region_of(R, n, g)];
        const uint32_t t = g - G.first, row = t / G.chunks, chunk = t - row * G.chunks;
        const uint8_t* const s = G.src + (uint64_t)row * G.src_pitch;
        uint8_t* const d = G.dst + (uint64_t)row * G.dst_pitch;
        const uint64_t L = G.row_bytes;
        const uint32_t U = G.unit;
        uint64_t head = (uint64_t)((0u - (uint32_t)(uintptr_t)d) & (U - 1u));
        head = head < L ? head : L;
        const uint64_t nb = (L - head) / U;
        const uint64_t i0 = (uint64_t)chunk * 1024u + tid;
        if (U == 16u) {
            xfer_u32x4 v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) { const uint64_t i = i0 + 256u * (uint32_t)k; if (i < nb) v[k] = *reinterpret_cast<const xfer_u32x4*>(s + head + i * 16u); }
#pragma unroll
            for (int k = 0; k < 4; k++) { const uint64_t i = i0 + 256u * (uint32_t)k; if (i < nb) xfer_store16(d + head + i * 16u, v[k]); }
        } else if (U == 4u) {
            uint32_t v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) { const uint64_t i = i0 + 256u * (uint32_t)k; if (i < nb) v[k] = *reinterpret_cast<const uint32_t*>(s + head + i * 4u); }
#pragma unroll
            for (int k = 0; k < 4; k++) { const uint64_t i = i0 + 256u * (uint32_t)k; if (i < nb) store_target(reinterpret_cast<uint32_t*>(d + head + i * 4u), v[k]); }
        } else {
            uint8_t v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) { const uint64_t i = i0 + 256u * (uint32_t)k; if (i < nb) v[k] = s[i]; }
#pragma unroll
            for (int k = 0; k < 4; k++) { const uint64_t i = i0 + 256u * (uint32_t)k; if (i < nb) d[i] = v[k]; }
        }
        if (chunk == 0u) {
            const uint64_t toff = head + nb * U, tail = L - toff;
            if (tid < head) d[tid] = s[tid];
            if (tid < tail) d[toff + tid] = s[toff + tid];
        }
    }
}

// ---- format conversion of blits and clears: the samplers' decode, the resolve's encode -----------------------------------------------------------
// (formats: 1 B8G8R8A8_SRGB, 2 R32G32B32A32_SFLOAT, 3 D32_SFLOAT, 4 R8G8B8A8_UNORM, 6 R8G8B8A8_SRGB; wave-uniform branches)
__device__ __forceinline__ f4 xfer_decode8(uint32_t format, uint32_t p) {
    if (format == 1u) return unpack_bgra8_srgb(p);
    return unpack_rgba8(p, format == 6u);
}
__device__ __forceinline__ uint32_t xfer_encode8(uint32_t format, f4 c) {
    if (format == 1u) return pack_bgra8_srgb(c);
    const uint32_t a = (uint32_t)rintf(saturatef(c.w) * 255.0f) << 24;
    if (format == 6u) return srgb8(c.x) | (srgb8(c.y) << 8) | (srgb8(c.z) << 16) | a;
    return (uint32_t)rintf(saturatef(c.x) * 255.0f) | ((uint32_t)rintf(saturatef(c.y) * 255.0f) << 8) | ((uint32_t)rintf(saturatef(c.z) * 255.0f) << 16) | a;
}
__device__ __forceinline__ int32_t xfer_floordiv(int32_t num, int32_t den) {      // den > 0
    const int32_t q = num / den;
    return (num - q * den) < 0 ? q - 1 : q;
}
__device__ __forceinline__ int32_t xfer_clamp(int32_t v, int32_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---- blit: destination-pixel-parallel ------------------------------------------------------------------------------------------------------------
// One 256-thread workgroup per 32 x 32 tile of the destination level that the region's rectangle touches (tiles aligned to the level's origin).  Lane t
// owns column t & 31 of rows (t >> 5) + 8 b, b = 0 .. 3 -- the sky kernel's mapping: a wave stores two whole rows of the tile per step, 128-byte
// segments of an 8-bit target, 512-byte ones of a float target.  All taps of a lane's four pixels (four of NEAREST, sixteen of LINEAR) are issued
// before any is decoded or filtered.  Source indices are clamped to the level's edge whatever the lane holds.
template <int FILTER>
__global__ __launch_bounds__(RASTER_THREADS, 4) void transfer_blit_kernel(const PassParams* __restrict__ params, const RasterHead H) {
    constexpr int TAPS = FILTER ? 4 : 1;
    ParamsRef P = *(ParamsPtr)(uintptr_t)params;
    const XferPtr R = (XferPtr)(uintptr_t)P.xfer_regions;
    const uint32_t tid = threadIdx.x, unit = blockIdx.x;
    if (unit >= P.xfer_groups) return;
    XferRef G = R[xfer_region_of(R, P.xfer_count, unit)];
    const uint32_t t = unit - G.first, ty = t / G.tiles_x, tx = t - ty * G.tiles_x;
    const int32_t x = (G.dx0 & ~31) + (int32_t)(tx * 32u + (tid & 31u));
    const int32_t y0 = (G.dy0 & ~31) + (int32_t)(ty * 32u + (tid >> 5));
    const bool in_x = x >= G.dx0 && x < G.dx1;
    const bool src_float = P.xfer_src_format == 2u, dst_float = P.xfer_dst_format == 2u;
    const int32_t wmax = (int32_t)G.src_w - 1, hmax = (int32_t)G.src_h - 1;

    // the column's source index (and weight) once, the four rows' each
    const int32_t xd = G.xd, yd = G.yd;
    const int32_t nx = G.xn0 + G.xns * (x - G.dx0), qx = xfer_floordiv(nx, xd);
    const uint32_t cx0 = (uint32_t)xfer_clamp(G.sx0 + qx, wmax), cx1 = (uint32_t)xfer_clamp(G.sx0 + qx + 1, wmax);
    const float fx = FILTER ? (float)(nx - qx * xd) / (float)xd : 0.0f;
    bool in[4];
    uint32_t off[4][TAPS];
    float fy[4];
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int32_t y = y0 + 8 * b;
        in[b] = in_x && y >= G.dy0 && y < G.dy1;
        const int32_t ny = G.yn0 + G.yns * (y - G.dy0), qy = xfer_floordiv(ny, yd);
        const uint32_t cy0 = (uint32_t)xfer_clamp(G.sy0 + qy, hmax), cy1 = (uint32_t)xfer_clamp(G.sy0 + qy + 1, hmax);
        fy[b] = FILTER ? (float)(ny - qy * yd) / (float)yd : 0.0f;
        off[b][0] = cy0 * G.src_w + cx0;
        if (FILTER) { off[b][1] = cy0 * G.src_w + cx1; off[b][2] = cy1 * G.src_w + cx0; off[b][3] = cy1 * G.src_w + cx1; }
    }
    f4 tap[4][TAPS];
    if (src_float) {
        const float4* const src = reinterpret_cast<const float4*>(G.src);
        float4 v[4][TAPS];
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int k = 0; k < TAPS; k++) v[b][k] = in[b] ? src[off[b][k]] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int k = 0; k < TAPS; k++) tap[b][k] = {v[b][k].x, v[b][k].y, v[b][k].z, v[b][k].w};
    } else {
        const uint32_t* const src = reinterpret_cast<const uint32_t*>(G.src);
        uint32_t v[4][TAPS];
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int k = 0; k < TAPS; k++) v[b][k] = in[b] ? src[off[b][k]] : 0u;
        const uint32_t sf = P.xfer_src_format;
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int k = 0; k < TAPS; k++) tap[b][k] = xfer_decode8(sf, v[b][k]);      // sRGB sources are decoded per texel, before the filter
    }
    const uint32_t df = P.xfer_dst_format;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        if (!in[b]) continue;
        f4 c = tap[b][0];
        if (FILTER) {
            const f4 a = tap[b][0], e = tap[b][1], f = tap[b][2], g = tap[b][3];
            const float gx = 1.0f - fx, gy = 1.0f - fy[b];
            c.x = (a.x * gx + e.x * fx) * gy + (f.x * gx + g.x * fx) * fy[b];
            c.y = (a.y * gx + e.y * fx) * gy + (f.y * gx + g.y * fx) * fy[b];
            c.z = (a.z * gx + e.z * fx) * gy + (f.z * gx + g.z * fx) * fy[b];
            c.w = (a.w * gx + e.w * fx) * gy + (f.w * gx + g.w * fx) * fy[b];
        }
        const size_t pix = (size_t)(uint32_t)(y0 + 8 * b) * G.dst_w + (uint32_t)x;
        if (dst_float) xfer_store16(G.dst + pix * 16u, xfer_u32x4{__float_as_uint(c.x), __float_as_uint(c.y), __float_as_uint(c.z), __float_as_uint(c.w)});
        else store_target(reinterpret_cast<uint32_t*>(G.dst) + pix, xfer_encode8(df, c));
    }
}

// ---- clears: a blit store of one value to every texel -------------------------------------------------------------------------------------------
// The value is encoded once per lane by the blit's encoder, then stored 16 bytes at a time: a work unit is four steps of 256 stores.  A range that
// does not start on a 16-byte boundary (a layer view, wrapped memory) has up to three words before the first whole store and behind the last.
__global__ __launch_bounds__(RASTER_THREADS) void transfer_fill_kernel(const PassParams* __restrict__ params, const RasterHead H) {
    ParamsRef P = *(ParamsPtr)(uintptr_t)params;
    const XferPtr R = (XferPtr)(uintptr_t)P.xfer_regions;
    const uint32_t n = P.xfer_count, total = P.xfer_groups, tid = threadIdx.x, df = P.xfer_dst_format;
    const f4 c = {P.xfer_color[0], P.xfer_color[1], P.xfer_color[2], P.xfer_color[3]};
    uint32_t p0, p1, p2, p3;
    if (df == 2u) { p0 = __float_as_uint(c.x); p1 = __float_as_uint(c.y); p2 = __float_as_uint(c.z); p3 = __float_as_uint(c.w); }
    else p0 = p1 = p2 = p3 = df == 3u ? __float_as_uint(c.x) : xfer_encode8(df, c);
    auto pat = [&](uint32_t j) { j &= 3u; return j == 0u ? p0 : (j == 1u ? p1 : (j == 2u ? p2 : p3)); };      // (selects: no indexed register array)
    for (uint32_t g = blockIdx.x; g < total; g += gridDim.x) {
        XferRef G = R[xfer_region_of(R, n, g)];
        const uint32_t chunk = g - G.first;
        uint8_t* const d = G.dst;
        const uint64_t words = G.row_bytes >> 2;
        uint64_t head = (uint64_t)(((0u - (uint32_t)(uintptr_t)d) & 15u) >> 2);
        head = head < words ? head : words;
        const uint64_t nv = (words - head) >> 2;
        // word j of the range holds pat(j): the whole stores behind `head` words hold the pattern rotated by it
        const uint32_t h = (uint32_t)head;
        const xfer_u32x4 v = {pat(h), pat(h + 1u), pat(h + 2u), pat(h + 3u)};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint64_t i = (uint64_t)chunk * 1024u + 256u * (uint32_t)k + tid;
            if (i < nv) xfer_store16(d + (head + i * 4u) * 4u, v);
        }
        if (chunk == 0u) {
            const uint64_t toff = head + nv * 4u, tail = words - toff;
            if (tid < head) reinterpret_cast<uint32_t*>(d)[tid] = pat(tid);
            if (tid < tail) reinterpret_cast<uint32_t*>(d)[toff + tid] = pat((uint32_t)(toff + tid));
        }
    }
}
