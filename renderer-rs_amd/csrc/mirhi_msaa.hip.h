// mirhi_msaa.hip.h -- raster_kernel_msaa: a 4x multisampled scope whose samples never leave the chip
// Part of the single device translation unit mirhi_kernels.hip (included inside namespace mirhi, behind mirhi_raster.hip.h).
//
// The rasterizer is visibility-first: a tile resolves a (depth key, primitive id) minimum per pixel and only then shades.  Here a tile resolves FOUR
// such minima per pixel, one per sample of Vulkan's standard 4x pattern, shades every distinct winner of a pixel ONCE at the pixel centre, averages
// the four samples' colours and writes the resolved pixel -- the tiler idiom of a transient multisampled attachment with a resolve target.
//
//   coverage   a sample's coverage is the 1x centre test with the tile origin moved from the pixel centre (128, 128) to the sample position: the tile records
//              are built per sample (tile_rec_core with another origin), and everything behind them -- block masks, the pixel loops of raster_record, the
//              scissor's per-pixel box -- is the 1x code.  One pass of the staging and pixel loops per sample; a pass's keys go to LDS (32 KB for the
//              tile: 1024 pixels x 4 samples x 8 bytes), so the register allocation of a pass is the 1x kernel's.
//   depth      the triangle's depth plane at the sample position: the record's (tile origin - vertex 0) term carries the sample's offset, exactly.
//   shading    once per pixel and distinct winner, at (px + 1/2, py + 1/2), whether or not the winner covers the centre (the programs extrapolate).
//   resolve    colour ((c0 + c1) + (c2 + c3)) * 0.25f per channel, each operation rounded, nothing fused; an sRGB8 target encodes the average once.
//              Depth: sample 0.  prim_out: the four winners of pixel (px, py) at texels 4 px .. 4 px + 3 of row py.
// One team of four waves per tile, single-list bins, plain tile order, an ordered depth key, no triangle-parallel path (mirhi_scope.h keeps the scopes so).
#ifndef MIRHI_MSAA_HIP_H
#define MIRHI_MSAA_HIP_H

#pragma clang fp contract(off)

// sample s of the standard 4x pattern inside its pixel, in 1/256 px: (96, 32), (224, 96), (32, 160), (160, 224) -- exact in the 8 sub-pixel bits
__device__ __forceinline__ int32_t msaa_sample_x(uint32_t s) { return 96 + 128 * (int32_t)(s & 1u) - 64 * (int32_t)(s >> 1); }
__device__ __forceinline__ int32_t msaa_sample_y(uint32_t s) { return 32 + 64 * (int32_t)s; }

// One pass of one list for one sample: raster_list's staging (one record per lane, ballot compaction) with the record's origin at the sample, then the
// 1x pixel loops (raster_chunk).  (spx, spy): the sample position in 1/256 px, wave-uniform.
template <int KEYED, bool BINS>
__device__ __forceinline__ void msaa_list(const uint4* __restrict__ list, uint32_t n_total, uint32_t tile, uint32_t fixed_recs, const uint32_t* pages, uint4* lds_rec,
                                          uint32_t* lds_box, uint32_t* lds_count, uint32_t& flip, uint32_t tx, uint32_t ty, int32_t spx, int32_t spy, uint32_t qmask,
                                          int32_t ix0, int32_t iy0, float fix0, float fiy0, ParamsRef P, PixelState& st, uint32_t qbit0, uint32_t tid, uint32_t lane) {
    // the staging wave rotates with the tile, as in raster_list
    const uint32_t fq = (uint32_t)__builtin_amdgcn_readfirstlane((int)(((tid >> 6) + ((tx + ty) & 3u)) & 3u));
    const uint32_t ftid = fq * 64u + lane;
    // (exact: multiples of 2^-8; the sample's offset from the pixel centre, which tile_box adds 0.5 to)
    const float fsx = (float)(spx - 128) * (1.0f / 256.0f), fsy = (float)(spy - 128) * (1.0f / 256.0f);
    for (uint32_t base = 0; base < n_total; base += (uint32_t)RASTER_CHUNK) {
        __syncthreads();                                  // every wave has left the previous pass's records and read its count
        uint32_t* const cnt = lds_count + flip;
        if (tid == 0) lds_count[flip ^ 1u] = 0;           // (two counters used alternately: see raster_list)
        uint32_t txl = tx, tyl = ty;
        asm volatile("" : "+s"(txl), "+s"(tyl));
        const uint32_t i = base + ftid;
        bool hit = false;
        uint4 rec[4]; uint32_t box = 0;
        if (ftid < (uint32_t)RASTER_CHUNK && i < n_total) {
            int32_t X[3], Y[3], opx = 0, opy = 0;
            uint32_t z0 = 0, zx = 0, zy = 0, idk = 0, boxed = 0;
            if (BINS) {
                const uint32_t page = i < fixed_recs ? (tile * fixed_recs + i) >> BIN_PAGE_LOG2 : pages[i >> BIN_PAGE_LOG2];
                hit = page < PAGE_NONE;                   // (a page the exhausted pool could not supply: its records are in the big list)
                if (hit) {
                    const uint32_t ri = (page * (uint32_t)BIN_PAGE_RECS + (i & (BIN_PAGE_RECS - 1u))) * 2u;
                    const uint4 w0 = list[ri], w1 = list[ri + 1u];
                    const int32_t ox = (int32_t)(w0.x << 16) >> 16, oy = (int32_t)w0.x >> 16;
                    const uint32_t x0 = w0.y & 0xFFFFu, x1 = w0.z & 0xFFFFu, x2 = w0.w & 0xFFFFu, y0 = w0.y >> 16, y1 = w0.z >> 16, y2 = w0.w >> 16;
                    X[0] = ox + (int32_t)x0; X[1] = ox + (int32_t)x1; X[2] = ox + (int32_t)x2;
                    Y[0] = oy + (int32_t)y0; Y[1] = oy + (int32_t)y1; Y[2] = oy + (int32_t)y2;
                    const int32_t xmax = ox + (int32_t)max(x0, max(x1, x2)), ymax = oy + (int32_t)max(y0, max(y1, y2));
                    // every pixel with a sample inside the vertex bounds (as setup_triangle<true>), in tile-relative pixels
                    box = clamp_box((ox + 31) >> 8, (xmax - 32) >> 8, (oy + 31) >> 8, (ymax - 32) >> 8);
                    z0 = w1.x; zx = w1.y; zy = w1.z; idk = w1.w;
                }
            } else {
                const uint4 w0 = list[(size_t)i * 3u], w1 = list[(size_t)i * 3u + 1u], w2 = list[(size_t)i * 3u + 2u];
                opx = (int32_t)txl * TILE; opy = (int32_t)tyl * TILE;
                const int32_t bx0 = (int32_t)(w2.z & 0x7FFFu) - opx, bx1 = (int32_t)((w2.z >> 16) & 0x7FFFu) - opx;
                const int32_t by0 = (int32_t)(w2.w & 0xFFFFu) - opy, by1 = (int32_t)(w2.w >> 16) - opy;
                hit = !(bx1 < 0 || bx0 > TILE - 1 || by1 < 0 || by0 > TILE - 1);
                box = clamp_box(bx0, bx1, by0, by1);
                X[0] = (int32_t)w0.x; Y[0] = (int32_t)w0.y; X[1] = (int32_t)w0.z; Y[1] = (int32_t)w0.w; X[2] = (int32_t)w1.x; Y[2] = (int32_t)w1.y;
                z0 = w1.z; zx = w1.w; zy = w2.x; idk = w2.y; boxed = w2.z & 0x80000000u;
            }
            if (hit) {
                const int32_t bx0 = (int32_t)(box & 0xFFu), bx1 = (int32_t)(int8_t)((box >> 8) & 0xFFu);
                const int32_t by0 = (int32_t)((box >> 16) & 0xFFu), by1 = (int32_t)box >> 24;
                // the record of this sample: edge functions and block masks from the sample of the tile's first pixel, the depth term from the same point
                hit = tile_rec_core(rec, X, Y, 256 * opx + spx, 256 * opy + spy, bx0, bx1, by0, by1, (float)opx + fsx, (float)opy + fsy, z0, zx, zy, idk, boxed);
            }
        }
        const uint64_t ball = __ballot(hit);
        uint32_t wbase = 0;
        if (lane == 0 && ball) wbase = atomicAdd(cnt, (uint32_t)__popcll(ball));
        wbase = __builtin_amdgcn_readfirstlane(wbase);
        if (hit) {
            const uint32_t slot = wbase + (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
            lds_rec[slot * 4u + 0] = rec[0]; lds_rec[slot * 4u + 1] = rec[1];
            lds_rec[slot * 4u + 2] = rec[2]; lds_rec[slot * 4u + 3] = rec[3];
            lds_box[slot] = box;
        }
        __syncthreads();
        const uint32_t n = *cnt;
        flip ^= 1u;
        if (n) raster_chunk<KEYED, 0, false, 4>(lds_rec, lds_box, n, qmask, ix0, iy0, fix0, fiy0, P, st, qbit0, lane, txl, tyl);
    }
}

// (a value of a four-element set by a run-time index, without indexing registers through memory)
template <typename T>
__device__ __forceinline__ T msaa_pick(uint32_t s, T a, T b, T c, T d) { return s == 0u ? a : (s == 1u ? b : (s == 2u ? c : d)); }

// PROGS as raster_body: 1 TRIANGLE, 2 MODEL / MODEL_FULL, 3 both, 4 any mix with MODEL_PBR or mip-mapped / sRGB textures.  KEYED: 0 the plain key (LESS /
// LESS_OR_EQUAL), 1 the generic one (GREATER / GREATER_OR_EQUAL).
template <int PROGS, int KEYED>
__device__ __forceinline__ void raster_body_msaa(const PassParams* __restrict__ params, const RasterHead& H) {
    ParamsRef P = *(ParamsPtr)(uintptr_t)params;
    __shared__ uint4 lds_rec[RASTER_CHUNK * 4];
    __shared__ uint32_t lds_box[RASTER_CHUNK];
    __shared__ uint32_t lds_count[2];
    __shared__ uint32_t lds_pages[BIN_TABLE_ROW];
    __shared__ unsigned long long lds_keys[4][TILE * TILE];      // the four samples' keys of every pixel of the tile
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t q = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t tx = blockIdx.x, tyr = blockIdx.y;
    const uint32_t tile = tyr * H.tiles_x + tx, ty = H.tile_origin + tyr * H.tile_row_step;
    // wave q owns the 16x16 quadrant q, lane (x = lane & 7, y = lane >> 3) one pixel of each of its four 8x8 blocks
    const int32_t ix0 = (int32_t)((q & 1u) * 16u + (lane & 7u)), iy0 = (int32_t)((q >> 1) * 16u + (lane >> 3));
    const float fix0 = (float)ix0, fiy0 = (float)iy0;
    const uint32_t qbit0 = 1u << ((q >> 1) * 8u + (q & 1u) * 2u), qmask = qbit0 * 0x33u;

    uint32_t count_raw = H.bin_count[tile * BIN_COUNT_STRIDE];
    const uint32_t nbig_raw = *H.big_count;
    const uint32_t count = count_raw < H.bin_cap ? count_raw : H.bin_cap;
    const uint32_t nbig = nbig_raw < H.big_cap ? nbig_raw : H.big_cap;
    const bool need_pages = count > H.fixed_recs;
    if (need_pages && tid < (uint32_t)BIN_TABLE_ROW) lds_pages[tid] = P.bin_table[tile * (uint32_t)BIN_TABLE_ROW + tid];
    // the workspace is left re-armed for the next scope, as raster_body leaves it
    if (tid == 0 && tile == 0u) {
        *P.big_count_next = 0;
        P.status[1] = nbig_raw;
        uint32_t pages_used = 0;
        for (uint32_t x = 0; x < 8u; x++) {
            const uint32_t c = P.pool_next[x * (uint32_t)POOL_COUNTER_STRIDE];
            pages_used += c < P.pool_dyn_pages ? c : P.pool_dyn_pages;
            P.pool_next[x * (uint32_t)POOL_COUNTER_STRIDE] = 0;
        }
        P.status[2] = pages_used;
        uint32_t busy = 0;
        for (uint32_t x = 0; x < 8u; x++) { busy += P.active_prev[x * 32u]; P.active_prev[x * 32u] = 0; }
        P.status[3] = busy | 0x80000000u;
    }
    const uint32_t px0 = tx * TILE + (uint32_t)ix0, py0 = ty * TILE + (uint32_t)iy0;

    if (count == 0u && nbig == 0u) {
        // Empty tile: every sample of every pixel has the clear colour, whose average is the clear colour
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t px = px0 + (uint32_t)(b & 1) * BLOCK, py = py0 + (uint32_t)(b >> 1) * BLOCK;
            if (!(px < P.width && py < P.height)) continue;
            const size_t pix = (size_t)py * P.width + px;
            if (P.color_format == 2) reinterpret_cast<float4*>(P.color)[pix] = make_float4(P.clear_color[0], P.clear_color[1], P.clear_color[2], P.clear_color[3]);
            else reinterpret_cast<uint32_t*>(P.color)[pix] = P.clear_packed;
            if (P.prim_out) reinterpret_cast<uint4*>(P.prim_out)[pix] = make_uint4(NO_PRIM, NO_PRIM, NO_PRIM, NO_PRIM);
            if (P.depth && P.depth_store) P.depth[pix] = __uint_as_float(P.clear_depth_bits);
        }
        return;
    }

    if (tid == 0) { lds_count[0] = 0; lds_count[1] = 0; }      // (ordered by msaa_list's first barrier)
    if (PROGS >= 2 && tid == 0) __hip_atomic_fetch_add(&P.active[(tile & 7u) * 32u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a busy tile, as raster_body counts them)
    uint32_t flip = 0;
#pragma unroll 1
    for (uint32_t s = 0; s < 4u; s++) {
        const int32_t spx = msaa_sample_x(s), spy = msaa_sample_y(s);
        PixelState st;
#pragma unroll
        for (int b = 0; b < 4; b++) { st.zk[b] = P.init_zk; st.idk[b] = P.init_idk; }
        if (count) msaa_list<KEYED, true>(reinterpret_cast<const uint4*>(H.bin_pool), count, tile, H.fixed_recs, lds_pages, lds_rec, lds_box, lds_count, flip, tx, ty, spx, spy, qmask,
                                          ix0, iy0, fix0, fiy0, P, st, qbit0, tid, lane);
        if (nbig) msaa_list<KEYED, false>(reinterpret_cast<const uint4*>(launder_params((ParamsPtr)(uintptr_t)params)->big_recs), nbig, tile, 0u, lds_pages, lds_rec, lds_box, lds_count, flip,
                                           tx, ty, spx, spy, qmask, ix0, iy0, fix0, fiy0, P, st, qbit0, tid, lane);
        // (a lane writes and later reads its own pixels only: no barrier between here and the resolve)
#pragma unroll
        for (int b = 0; b < 4; b++)
            lds_keys[s][(iy0 + (b >> 1) * BLOCK) * TILE + ix0 + (b & 1) * BLOCK] = ((unsigned long long)st.zk[b] << 32) | st.idk[b];
    }
    // ready for the next scope that uses this workspace (every wave read the counter and the table row in front of the first pass's barrier)
    if (count && tid == 0) H.bin_count[tile * BIN_COUNT_STRIDE] = 0;
    if (need_pages && tid < (uint32_t)BIN_TABLE_ROW) launder_params((ParamsPtr)(uintptr_t)params)->bin_table[tile * (uint32_t)BIN_TABLE_ROW + tid] = PAGE_EMPTY;

    // ---- resolve: shade each pixel's distinct winners once at the pixel centre, average the four samples, store once ----
    const ParamsPtr R = launder_params((ParamsPtr)(uintptr_t)params);
    const uint32_t init_zk = R->init_zk, init_idk = R->init_idk;
    uint32_t held = 0;
    bool held_all = false;
#pragma unroll 1
    for (int b = 0; b < 4; b++) {
        const uint32_t px = px0 + (uint32_t)(b & 1) * BLOCK, py = py0 + (uint32_t)(b >> 1) * BLOCK;
        const bool inb = px < P.width && py < P.height;
        const size_t pix = (size_t)py * P.width + px;
        const uint32_t kofs = (uint32_t)((iy0 + (b >> 1) * BLOCK) * TILE + ix0 + (b & 1) * BLOCK);
        const unsigned long long k0 = lds_keys[0][kofs], k1 = lds_keys[1][kofs], k2 = lds_keys[2][kofs], k3 = lds_keys[3][kofs];
        const unsigned long long kinit = ((unsigned long long)init_zk << 32) | init_idk;
        // a sample is covered iff its key moved off the initial one (no primitive carries NO_PRIM, and the "nothing can pass" state is never replaced)
        const bool n0 = !inb || k0 == kinit, n1 = !inb || k1 == kinit, n2 = !inb || k2 == kinit, n3 = !inb || k3 == kinit;
        const uint32_t idflip = P.idflip;
        const uint32_t p0 = n0 ? NO_PRIM : (idflip ? MAX_PRIM_ID - (uint32_t)k0 : (uint32_t)k0), p1 = n1 ? NO_PRIM : (idflip ? MAX_PRIM_ID - (uint32_t)k1 : (uint32_t)k1);
        const uint32_t p2 = n2 ? NO_PRIM : (idflip ? MAX_PRIM_ID - (uint32_t)k2 : (uint32_t)k2), p3 = n3 ? NO_PRIM : (idflip ? MAX_PRIM_ID - (uint32_t)k3 : (uint32_t)k3);
        const f4 clear = {P.clear_color[0], P.clear_color[1], P.clear_color[2], P.clear_color[3]};
        f4 c0 = clear, c1 = clear, c2 = clear, c3 = clear;
        const float pxc = (float)px + 0.5f, pyc = (float)py + 0.5f;
        // Sample by sample: a winner an earlier sample of the pixel already shaded takes that colour (the usual pixel has one winner: one shading pass
        // for the whole wave, the other three find nothing to do); the others are shaded under the waterfall over the wave's draws, as in raster_body.
#pragma unroll 1
        for (uint32_t s = 0; s < 4u; s++) {
            const uint32_t prim = msaa_pick(s, p0, p1, p2, p3);
            const bool none = prim == NO_PRIM;
            f4 col = clear;
            bool need = !none;
            if (s > 2u && need && prim == p2) { col = c2; need = false; }
            if (s > 1u && need && prim == p1) { col = c1; need = false; }
            if (s > 0u && need && prim == p0) { col = c0; need = false; }
            const uint32_t mydraw = need ? (P.num_draws > 1 ? find_draw(P, prim) : 0u) : 0xFFFFFFFFu;
            uint64_t todo = __ballot(need);
            while (todo) {
                const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)mydraw, __ffsll((long long)todo) - 1);
                const bool mine = need && mydraw == d;
                if (mine) {
                    DrawRef D = const_draws(P.draws)[__builtin_amdgcn_readfirstlane(mydraw)];
                    const uint32_t tri = prim - D.prim_base;
                    if (PROGS == 1) col = shade_triangle_program(D, tri, pxc, pyc);
                    else if (PROGS == 2) col = shade_model_program<false>(D, tri, pxc, pyc);
                    else col = (D.program == 0) ? shade_triangle_program(D, tri, pxc, pyc) : shade_model_program<PROGS == 4, 0>(D, tri, pxc, pyc);
                }
                todo &= ~__ballot(mine);
            }
            if (s == 0u) c0 = col; else if (s == 1u) c1 = col; else if (s == 2u) c2 = col; else c3 = col;
        }
        // AVERAGE: in this order, each operation rounded (fp contract is off for this file); alpha like the colour channels
        f4 avg;
        avg.x = ((c0.x + c1.x) + (c2.x + c3.x)) * 0.25f; avg.y = ((c0.y + c1.y) + (c2.y + c3.y)) * 0.25f;
        avg.z = ((c0.z + c1.z) + (c2.z + c3.z)) * 0.25f; avg.w = ((c0.w + c1.w) + (c2.w + c3.w)) * 0.25f;
        if (P.color_format != 2) {
            // 8-bit target: the linear average is encoded once; a pixel none of whose samples was reached takes the host's packed clear colour, as at 1x.
            // The wave's two side-by-side blocks leave as one 8-byte store per lane (store_pair) when every lane of both writes its pixel.
            const uint32_t packed = (n0 && n1 && n2 && n3) ? P.clear_packed : pack_bgra8_srgb(avg);
            const bool all = __ballot(inb) == ~0ull;
            if ((b & 1) == 0) { held = packed; held_all = all; if (!all && inb) reinterpret_cast<uint32_t*>(P.color)[pix] = packed; }
            else if (all && held_all) store_pair(reinterpret_cast<uint32_t*>(P.color), py * P.width + (px - (uint32_t)BLOCK) - (lane & 7u), held, packed, lane);
            else {
                if (held_all) reinterpret_cast<uint32_t*>(P.color)[pix - (size_t)BLOCK] = held;
                if (inb) reinterpret_cast<uint32_t*>(P.color)[pix] = packed;
            }
        }
        if (!inb) continue;
        if (P.color_format == 2) reinterpret_cast<float4*>(P.color)[pix] = make_float4(avg.x, avg.y, avg.z, avg.w);
        if (P.prim_out) reinterpret_cast<uint4*>(P.prim_out)[pix] = make_uint4(p0, p1, p2, p3);
        // SAMPLE_ZERO: the depth bits of sample 0, the clear depth where no primitive reached it
        if (P.depth && P.depth_store) P.depth[pix] = __uint_as_float(n0 ? P.clear_depth_bits : ((uint32_t)(k0 >> 32) ^ P.zflip));
    }
}

// one 4x multisampled rendering scope: grid (tiles_x, tile rows)
template <int PROGS, int KEYED>
__global__ __launch_bounds__(RASTER_THREADS, (PROGS == 1 ? 3 : 2)) void raster_kernel_msaa(const PassParams* __restrict__ params, const RasterHead H) {
    raster_body_msaa<PROGS, KEYED>(params, H);
}

#endif  // MIRHI_MSAA_HIP_H
