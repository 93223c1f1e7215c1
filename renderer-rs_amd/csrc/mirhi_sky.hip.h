// mirhi_sky.hip.h -- the SKYBOX segment's kernel (vertex/skybox.hlsl + pixel/skybox.hlsl; include/mirhi.h "SKYBOX").
// Part of mirhi_kernels.hip's translation unit, inside namespace mirhi, behind mirhi_ibl_sample.hip.h, mirhi_shading.hip.h (pack_bgra8_srgb) and
// mirhi_raster.hip.h (store_target).
//
// One 256-thread workgroup per 32 x 32 tile of the rows this device owns (grid row k = tile row tile_row_begin + k * tile_row_step, as in
// raster_body).  Lane t owns column t & 31 of rows (t >> 5) + 8 b, b = 0 .. 3: a wave writes two whole rows of the tile per step -- 128-byte
// row segments of an 8-bit target, 512-byte ones of a float target.  There is one fragment per pixel, so nothing is staged, binned or keyed:
// per pixel the coverage test (the host's integer edge functions), the scissor, the depth compare against the loaded or cleared depth, then for
// the pixels that pass the direction, the face, all four texel loads, and the filter.  The lookup is under per-lane conditions: a wave whose pixels
// all fail branches around it (no address formed, no texel fetched), in a mixed wave the failing lanes and pixels are masked off.
// Nothing of the workspace is touched: no counter, no page table, no status word (DESIGN.md 8f "Workspace parity").
#pragma once

template <bool SEAMLESS> struct SkyTaps { typedef IblTaps type; };
template <> struct SkyTaps<true> { typedef IblSeamTaps type; };

__device__ __forceinline__ bool sky_depth_passes(uint32_t op, float frag, float stored) {
    switch (op) {      // mirhi_compare_op; wave-uniform
        case 1u: return frag < stored;
        case 2u: return frag == stored;
        case 3u: return frag <= stored;
        case 4u: return frag > stored;
        case 5u: return frag != stored;
        case 6u: return frag >= stored;
        case 7u: return true;
        default: return false;
    }
}

// Four workgroups per CU are asked for: sixteen float4 texels in flight (four pixels x four taps) beside the addresses and fractions must fit, and the
// kernel waits on gathers, not on arithmetic.  What the compiler makes of it (VGPRs, occupancy; no spill, scratch or LDS) is DESIGN.md 8f's table.
// SEAMLESS: the environment's seamless state was on when the draw was recorded (PassParams::sky_seamless, sky_kernel_seamless): the four
// taps cross face edges (ibl_seamless_taps: offsets from level 0's first texel) and a corner tap is the mean of the other three.  The shape stays:
// every address, then the sixteen loads, then the filters.  SEAMLESS = false is sky_kernel as it was.
template <bool SEAMLESS>
__device__ __forceinline__ void sky_body(const PassParams* __restrict__ params, const RasterHead& H) {
    ParamsRef P = *(ParamsPtr)(uintptr_t)params;
    const uint32_t tid = threadIdx.x;
    const uint32_t tx = blockIdx.x + (H.tile_origin >> 16), ty = (H.tile_origin & 0xFFFFu) + blockIdx.y * H.tile_row_step;      // (the render area's tile columns)
    const uint32_t px = tx * TILE + (tid & 31u), py0 = ty * TILE + (tid >> 5);
    const uint32_t width = P.width;
    // the render area: the pixels this segment loads, fills and stores (the attachment itself in a full-extent scope; the scissor lies inside it)
    const uint32_t ax0 = P.area_x0, ay0 = P.area_y0, aw = P.area_w, ah = P.area_h;
    const bool load_depth = P.depth_load && P.depth;
    const float frag_depth = __uint_as_float(P.sky_depth_bits);
    const uint32_t visible = P.sky_visible, op = P.sky_compare;
    const bool in_x = px - ax0 < aw && (int32_t)px >= P.sky_scissor[0] && (int32_t)px <= P.sky_scissor[2];

    bool inb[4], won[4];
    uint32_t zorig[4];
    // every depth load of the lane first: the four latencies overlap
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const uint32_t py = py0 + 8u * (uint32_t)b;
        inb[b] = px - ax0 < aw && py - ay0 < ah;
        zorig[b] = P.clear_depth_bits;
        if (load_depth && inb[b]) zorig[b] = __float_as_uint(P.depth[(size_t)py * width + px]);
    }
    bool any = false;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const uint32_t py = py0 + 8u * (uint32_t)b;
        bool w = visible && in_x && py - ay0 < ah && (int32_t)py >= P.sky_scissor[1] && (int32_t)py <= P.sky_scissor[3];
        if (w) {
            const long long e0 = P.sky_e0[0] + 256ll * ((long long)P.sky_a[0] * (int32_t)px + (long long)P.sky_b[0] * (int32_t)py);
            const long long e1 = P.sky_e0[1] + 256ll * ((long long)P.sky_a[1] * (int32_t)px + (long long)P.sky_b[1] * (int32_t)py);
            const long long e2 = P.sky_e0[2] + 256ll * ((long long)P.sky_a[2] * (int32_t)px + (long long)P.sky_b[2] * (int32_t)py);
            w = (e0 | e1 | e2) >= 0 && sky_depth_passes(op, frag_depth, __uint_as_float(zorig[b]));
        }
        won[b] = w;
        any |= w;
    }

    f4 col[4];
    if (any) {      // (per lane: a wave without a passing pixel branches around the lookup)
        const uint32_t n = P.sky_size;
        const float4* const env = reinterpret_cast<const float4*>(P.sky_env);
        const float fx = (float)px + 0.5f;
        typename SkyTaps<SEAMLESS>::type taps[4];
        const float4* face[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            taps[b] = {}; face[b] = env;
            if (!won[b]) continue;      // (behind geometry most pixels fail: their direction arithmetic is skipped, not only their loads)
            const float fy = (float)(py0 + 8u * (uint32_t)b) + 0.5f;
            // LocalPos: affine in the pixel centre (pixel/skybox.hlsl:11 takes the interpolated vertex output), then normalize (:24)
            const float lx = __builtin_fmaf(P.sky_posy[0], fy, __builtin_fmaf(P.sky_posx[0], fx, P.sky_pos0[0]));
            const float ly = __builtin_fmaf(P.sky_posy[1], fy, __builtin_fmaf(P.sky_posx[1], fx, P.sky_pos0[1]));
            const float lz = __builtin_fmaf(P.sky_posy[2], fy, __builtin_fmaf(P.sky_posx[2], fx, P.sky_pos0[2]));
            const float inv = __builtin_amdgcn_rsqf(__builtin_fmaf(lz, lz, __builtin_fmaf(ly, ly, lx * lx)));
            const IblFaceUV f = ibl_select_face(lx * inv, ly * inv, lz * inv);
            if constexpr (SEAMLESS) taps[b] = ibl_seamless_taps(n, f.face, f.s, f.t, true);      // (face[b] stays the level's base: every tap offset < 6 n * n)
            else {
                taps[b] = ibl_bilinear_taps(n, f.s, f.t);
                face[b] = env + f.face * n * n;      // (level 0 starts the chain; face < 6 and every tap offset < n * n whatever the direction holds)
            }
        }
        float4 t[4][4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            if (won[b]) { t[b][0] = face[b][taps[b].o00]; t[b][1] = face[b][taps[b].o10]; t[b][2] = face[b][taps[b].o01]; t[b][3] = face[b][taps[b].o11]; }
            else t[b][0] = t[b][1] = t[b][2] = t[b][3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int b = 0; b < 4; b++) {
            float4 c;
            if constexpr (SEAMLESS) c = ibl_seamless_filter(taps[b], t[b][0], t[b][1], t[b][2], t[b][3]);
            else c = ibl_bilinear_filter(taps[b], t[b][0], t[b][1], t[b][2], t[b][3]);
            col[b] = {c.x, c.y, c.z, c.w};
        }
    }

    const bool keep_color = P.color_load != 0u;
    const bool store_depth = P.depth && P.depth_store;
    const bool write_depth = P.sky_write != 0u;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        if (!inb[b]) continue;
        const size_t pix = (size_t)(py0 + 8u * (uint32_t)b) * width + px;
        if (won[b] || !keep_color) {      // LOAD keeps what an earlier scope / segment wrote where the sky does not show
            const f4 c = won[b] ? col[b] : f4{P.clear_color[0], P.clear_color[1], P.clear_color[2], P.clear_color[3]};
            if (P.color_format == 2u) reinterpret_cast<float4*>(P.color)[pix] = make_float4(c.x, c.y, c.z, c.w);
            else store_target(reinterpret_cast<uint32_t*>(P.color) + pix, won[b] ? pack_bgra8_srgb(c) : P.clear_packed);
            if (P.prim_out) P.prim_out[pix] = won[b] ? P.sky_prim : NO_PRIM;
        }
        // a loaded depth that the sky leaves as it is needs no store; a cleared one is the scope's to write
        if (store_depth && ((won[b] && write_depth) || !load_depth)) P.depth[pix] = __uint_as_float((won[b] && write_depth) ? P.sky_depth_bits : zorig[b]);
    }
}

__global__ __launch_bounds__(RASTER_THREADS, 4) void sky_kernel(const PassParams* __restrict__ params, const RasterHead H) { sky_body<false>(params, H); }
// the SKYBOX segment of a seamless environment cube
__global__ __launch_bounds__(RASTER_THREADS, 4) void sky_kernel_seamless(const PassParams* __restrict__ params, const RasterHead H) { sky_body<true>(params, H); }
