// mirhi_kernels.hip -- gfx950 (CDNA4) kernels of the compute rasterizer.
//
// Two kernels per rendering scope (DESIGN.md "Kernels"; a SKYBOX segment runs sky_kernel alone, mirhi_sky.hip.h; a recorded transfer command one
// kernel of mirhi_transfer.hip.h):
//   geometry_kernel  one lane per input triangle: index + vertex fetch, vertex-shader position,
//                    clip / divide / viewport / snap / cull / depth-plane setup, then tile binning.
//                    Restates SURVEY 8a rows a1, a2, a4, a5 (crates/rhi/src/vertex.rs:20-61,88-170;
//                    command.rs:583-628; shaders/hlsl/vertex/{triangle,model}.hlsl;
//                    pipeline.rs:645-698,976-986; renderer.rs:504-518).
//   raster_kernel    one 256-lane workgroup per 32x32 tile: stages the tile's triangle records
//                    through LDS, resolves coverage (integer edge functions, top-left rule) and
//                    depth (64-bit key, registers only -- depth never leaves the CU unless a depth
//                    image is attached), then runs the fragment programs on the winning primitive
//                    of each pixel and stores the colour once.  Rows a6-a9 (pipeline.rs:976-1025;
//                    rendering.rs:102-115,356-370; depth_buffer.rs:48; shaders/hlsl/pixel/*.hlsl;
//                    lights.hlsli; swapchain.rs:561-570).
//
// Everything that decides coverage, depth or the winning primitive is integer arithmetic or IEEE
// binary32 {+,-,*,/} in the order fixed by DESIGN.md "Pipeline specification"; this file is
// compiled with -ffp-contract=off so results are bit-identical to the CPU oracle.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdio>
#include <cstdlib>
#include <stdint.h>
#include <atomic>
#include <mutex>
#include <string>

#include "mirhi_device.h"
#include "mirhi_launch.h"
#include "mirhi_variant.h"

namespace mirhi {

#include "mirhi_exact.hip.h"
#include "mirhi_common.hip.h"
#include "mirhi_geometry.hip.h"
#include "mirhi_ibl_sample.hip.h"
#include "mirhi_shading.hip.h"
#include "mirhi_raster.hip.h"
#include "mirhi_msaa.hip.h"
#include "mirhi_sky.hip.h"
#include "mirhi_stats.hip.h"
#include "mirhi_ordered.hip.h"
#include "mirhi_transfer.hip.h"
#include "mirhi_multiview.hip.h"

// the build this code object belongs to (build.py passes the source hash to both translation units; native_device_open compares)
#ifndef MIRHI_SOURCE_HASH
#define MIRHI_SOURCE_HASH "unknown"
#endif
__device__ __attribute__((used)) char g_build_id[17] = MIRHI_SOURCE_HASH;       // (not const: a const at namespace scope is a local symbol, the loader would not find it)
// measurement only (mirhi_device_measure_roundtrip): one wave that does nothing
__global__ __launch_bounds__(64) void noop_kernel(uint32_t) {}
// behind a natively dispatched frame of a tile split: tells the band-exchange stream (hipStreamWaitValue64 on signal memory) that the frame is rendered
__global__ __launch_bounds__(64) void seq_store_kernel(uint64_t* word, uint64_t value) {
    if (threadIdx.x == 0) __hip_atomic_store(word, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------------------------------------
// launch wrappers (host side of this translation unit)
// ------------------------------------------------------------------------------------------------
hipError_t upload_srgb_lut(const float* lut, hipStream_t stream) {
    return hipMemcpyToSymbolAsync(HIP_SYMBOL(g_srgb_lut), lut, 256 * sizeof(float), 0, hipMemcpyHostToDevice, stream);
}

// failure of a native dispatch inside the launch wrappers below (they report it with their return value)
static thread_local hipError_t t_native_err = hipSuccess;
static inline hipError_t launch_result() { const hipError_t e = t_native_err; t_native_err = hipSuccess; return e != hipSuccess ? e : hipGetLastError(); }
// A plain launch, or -- when the caller wants the dispatch timed -- one with an event pair attached to the dispatch itself, or a native dispatch.
#define MIRHI_LAUNCH(kernel, grid, block, stream, t, ...)                                                               \
    do {                                                                                                                \
        if ((t).native) {                                                                                               \
            const hipError_t ne__ = native_launch((t).native, reinterpret_cast<const void*>(+kernel), grid, block, (t).native_signal, (t).native_flags, __VA_ARGS__); \
            if (ne__ != hipSuccess) t_native_err = ne__;                                                                \
        }                                                                                                               \
        else if ((t).start || (t).stop) hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, (t).start, (t).stop, 0, __VA_ARGS__);     \
        else hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);                                           \
    } while (0)

hipError_t launch_noop(NativeQueue* q, uint64_t signal) {
    return native_launch(q, reinterpret_cast<const void*>(+noop_kernel), dim3(1), dim3(64), signal, NATIVE_RELEASE_SYSTEM, (uint32_t)0);
}

hipError_t launch_seq_store(NativeQueue* q, uint64_t* word, uint64_t value) {
    return native_launch(q, reinterpret_cast<const void*>(+seq_store_kernel), dim3(1), dim3(64), 0, NATIVE_RELEASE_SYSTEM, word, value);
}

hipError_t launch_vertex(const PassParams& P, const PassParams* dev_params, hipStream_t stream, LaunchTiming t) {
    if (P.vs_total_slots == 0) return hipSuccess;
    if (P.depth_only) MIRHI_LAUNCH(vertex_kernel_shadow, dim3(P.vs_total_slots / GEOM_THREADS), dim3(GEOM_THREADS), stream, t, dev_params);   // (clip stream only)
    else MIRHI_LAUNCH(vertex_kernel, dim3(P.vs_total_slots / GEOM_THREADS), dim3(GEOM_THREADS), stream, t, dev_params);
    return launch_result();
}

hipError_t launch_geometry(const PassParams& P, const PassParams* dev_params, hipStream_t stream, LaunchTiming t) {
    if (P.total_slots == 0) return hipSuccess;
    const uint32_t tpw = (t.tris_per_wave == 16u || t.tris_per_wave == 32u) ? t.tris_per_wave : (uint32_t)GEOM_THREADS;
    const uint32_t blocks = P.total_slots / tpw;
    GeometryHead H = {P.draws, P.num_draws, tpw, nullptr, 0u, 0u, 0u};
    if (t.head_draw && P.num_draws == 1u && t.head_draw->index_type == 0u && t.head_draw->program == 0u && t.head_draw->vs_words == 0u && t.head_draw->stride >= 24u) {
        H.vb0 = t.head_draw->vb; H.stride0 = t.head_draw->stride; H.first0 = t.head_draw->first; H.tris0 = t.head_draw->tri_count;
    }
    // (more waves than the chip holds at five per SIMD: the occupancy-oriented variant)
    if (P.samples == 4u) {      // a 4x multisampled scope: the sample-conservative pixel box (setup_triangle<true>)
        if (blocks > 5u * 1024u) MIRHI_LAUNCH(geometry_kernel_msaa<7>, dim3(blocks), dim3(GEOM_THREADS), stream, t, dev_params, H);
        else MIRHI_LAUNCH(geometry_kernel_msaa<5>, dim3(blocks), dim3(GEOM_THREADS), stream, t, dev_params, H);
        return launch_result();
    }
    if (blocks > 5u * 1024u) MIRHI_LAUNCH(geometry_kernel<7>, dim3(blocks), dim3(GEOM_THREADS), stream, t, dev_params, H);
    else MIRHI_LAUNCH(geometry_kernel<5>, dim3(blocks), dim3(GEOM_THREADS), stream, t, dev_params, H);
    return launch_result();
}

// ---- the raster launch: raster_variant (mirhi_variant.h) chooses, the two tables below turn the choice into a kernel entry --------
// Each table names every instantiation of its kernels exactly once (nothing else in this file refers to them): the set of raster kernels in the code object
// is the set of rows, and the code object holds them in the order of the rows.
// A record of what the three raster launchers launched (mirhi_debug_raster_trace below; tests/test_gpu_variant_ledger.py): the chosen entry's name, appended
// after the entry is found and before the launch, on either dispatch path.  Off: one relaxed load per raster launch; the mutex is taken only when on (the
// submit thread launches too).
static std::atomic<uint32_t> g_raster_trace_on{0u};
static std::mutex g_raster_trace_mutex;
static std::string g_raster_trace;          // the names, each followed by '\n'
static uint32_t g_raster_trace_count = 0u;
static inline void raster_trace(const char* name) {
    if (!g_raster_trace_on.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> lock(g_raster_trace_mutex);
    g_raster_trace += name; g_raster_trace += '\n'; g_raster_trace_count++;
}

struct RasterEntry { uint32_t id; const char* name; void (*kernel)(const PassParams*, const RasterHead); };      // id: RasterVariant::kernel_id
#define ORDERED(P) {raster_kernel_id(RASTER_ORDERED, P, 0, 0, 1, 0, 4), "ordered_kernel<" #P ">", ordered_kernel<P>}
#define OWN(FAMILY, KERNEL, K, T) {raster_kernel_id(FAMILY, 0, K, T, 1, 0, 4), #KERNEL "<" #K ", " #T ">", KERNEL<K, T>}
#define IBL(K, T, S) {raster_kernel_id(RASTER_IBL, S, K, T, 1, 0, 4), "raster_kernel_ibl<" #K ", " #T ", " #S ">", raster_kernel_ibl<K, T, S>}
#define WIDE(P, K, W) {raster_kernel_id(RASTER_WIDE, P, K, 1, 1, 0, W), "raster_kernel_wide<" #P ", " #K ", " #W ">", raster_kernel_wide<P, K, W>}
#define PLAIN(P, K, T, TEAMS, M) {raster_kernel_id(RASTER_PLAIN, P, K, T, TEAMS, M, 4 * TEAMS), "raster_kernel<" #P ", " #K ", " #T ", " #TEAMS ", " #M ">", raster_kernel<P, K, T, TEAMS, M>}
// ... and the AREA instantiations (a partial render area: RasterVariant::area), one team of four waves
#define OWN_A(FAMILY, KERNEL, K, T) {raster_kernel_id(FAMILY, 0, K, T, 1, 0, 4, 1), #KERNEL "<" #K ", " #T ", true>", KERNEL<K, T, true>}
#define IBL_A(K, T, S) {raster_kernel_id(RASTER_IBL, S, K, T, 1, 0, 4, 1), "raster_kernel_ibl<" #K ", " #T ", " #S ", true>", raster_kernel_ibl<K, T, S, true>}
#define PLAIN_A(P, K, T, M) {raster_kernel_id(RASTER_PLAIN, P, K, T, 1, M, 4, 1), "raster_kernel<" #P ", " #K ", " #T ", 1, " #M ", true>", raster_kernel<P, K, T, 1, M, true>}
// ... and the seamless instantiations of the IBL family (RasterVariant::seamless), full-extent and AREA
#define IBL_S(K, T, S) {raster_kernel_id(RASTER_IBL, S, K, T, 1, 0, 4, 0, 1), "raster_kernel_ibl_seamless<" #K ", " #T ", " #S ">", raster_kernel_ibl_seamless<K, T, S>}
#define IBL_SA(K, T, S) {raster_kernel_id(RASTER_IBL, S, K, T, 1, 0, 4, 1, 1), "raster_kernel_ibl_seamless<" #K ", " #T ", " #S ", true>", raster_kernel_ibl_seamless<K, T, S, true>}
#define MSAA(P, K) {raster_kernel_id(RASTER_MSAA, P, K, 0, 1, 0, 4), "raster_kernel_msaa<" #P ", " #K ">", raster_kernel_msaa<P, K>}
static const RasterEntry k_raster_entries[] = {
    ORDERED(2), ORDERED(3), ORDERED(4), ORDERED(1),
    OWN(RASTER_DEPTH, raster_kernel_depth, 0, 1), OWN(RASTER_DEPTH, raster_kernel_depth, 1, 1), OWN(RASTER_DEPTH, raster_kernel_depth, 0, 0), OWN(RASTER_DEPTH, raster_kernel_depth, 1, 0),
    OWN(RASTER_CSM, raster_kernel_csm, 0, 1), OWN(RASTER_CSM, raster_kernel_csm, 1, 1), OWN(RASTER_CSM, raster_kernel_csm, 0, 0), OWN(RASTER_CSM, raster_kernel_csm, 1, 0),
    OWN(RASTER_SHADOW, raster_kernel_shadow, 0, 1), OWN(RASTER_SHADOW, raster_kernel_shadow, 1, 1), OWN(RASTER_SHADOW, raster_kernel_shadow, 0, 0), OWN(RASTER_SHADOW, raster_kernel_shadow, 1, 0),
    WIDE(2, 0, 16), WIDE(2, 0, 8), WIDE(2, 1, 16), WIDE(2, 1, 8), WIDE(4, 0, 16), WIDE(4, 0, 8), WIDE(4, 1, 16), WIDE(4, 1, 8),
    // predicate mode: pixel-parallel only
    PLAIN(2, 2, 0, 1, false), PLAIN(4, 2, 0, 1, false), PLAIN(3, 2, 0, 1, false), PLAIN(1, 2, 0, 1, false),
    // with the triangle-parallel path: two teams (alpha-masked, mesh), one team; per key
    PLAIN(4, 0, 1, 2, true), PLAIN(2, 0, 1, 2, false), PLAIN(4, 0, 1, 2, false), PLAIN(2, 0, 1, 1, false), PLAIN(3, 0, 1, 1, false), PLAIN(4, 0, 1, 1, false), PLAIN(1, 0, 1, 1, false),
    PLAIN(4, 1, 1, 2, true), PLAIN(2, 1, 1, 2, false), PLAIN(4, 1, 1, 2, false), PLAIN(2, 1, 1, 1, false), PLAIN(3, 1, 1, 1, false), PLAIN(4, 1, 1, 1, false), PLAIN(1, 1, 1, 1, false),
    PLAIN(4, 0, 1, 1, true), PLAIN(4, 1, 1, 1, true),
    // pixel-parallel only
    PLAIN(2, 0, 0, 1, false), PLAIN(4, 0, 0, 1, false), PLAIN(3, 0, 0, 1, false), PLAIN(1, 0, 0, 1, false),
    PLAIN(2, 1, 0, 1, false), PLAIN(4, 1, 0, 1, false), PLAIN(3, 1, 0, 1, false), PLAIN(1, 1, 0, 1, false),
    // MODEL_PBR_IBL scopes: per key, with and without the triangle-parallel path, per shadow term (none, single map, cascades, blended cascades)
    IBL(0, 1, 0), IBL(1, 1, 0), IBL(0, 0, 0), IBL(1, 0, 0), IBL(0, 1, 1), IBL(1, 1, 1), IBL(0, 0, 1), IBL(1, 0, 1), IBL(0, 1, 2), IBL(1, 1, 2), IBL(0, 0, 2), IBL(1, 0, 2),
    // the AREA instantiations, in the order of the rows above
    OWN_A(RASTER_DEPTH, raster_kernel_depth, 0, 1), OWN_A(RASTER_DEPTH, raster_kernel_depth, 1, 1), OWN_A(RASTER_DEPTH, raster_kernel_depth, 0, 0), OWN_A(RASTER_DEPTH, raster_kernel_depth, 1, 0),
    OWN_A(RASTER_CSM, raster_kernel_csm, 0, 1), OWN_A(RASTER_CSM, raster_kernel_csm, 1, 1), OWN_A(RASTER_CSM, raster_kernel_csm, 0, 0), OWN_A(RASTER_CSM, raster_kernel_csm, 1, 0),
    OWN_A(RASTER_SHADOW, raster_kernel_shadow, 0, 1), OWN_A(RASTER_SHADOW, raster_kernel_shadow, 1, 1), OWN_A(RASTER_SHADOW, raster_kernel_shadow, 0, 0), OWN_A(RASTER_SHADOW, raster_kernel_shadow, 1, 0),
    PLAIN_A(2, 2, 0, false), PLAIN_A(4, 2, 0, false), PLAIN_A(3, 2, 0, false), PLAIN_A(1, 2, 0, false),
    PLAIN_A(2, 0, 1, false), PLAIN_A(3, 0, 1, false), PLAIN_A(4, 0, 1, false), PLAIN_A(1, 0, 1, false),
    PLAIN_A(2, 1, 1, false), PLAIN_A(3, 1, 1, false), PLAIN_A(4, 1, 1, false), PLAIN_A(1, 1, 1, false),
    PLAIN_A(4, 0, 1, true), PLAIN_A(4, 1, 1, true),
    PLAIN_A(2, 0, 0, false), PLAIN_A(4, 0, 0, false), PLAIN_A(3, 0, 0, false), PLAIN_A(1, 0, 0, false),
    PLAIN_A(2, 1, 0, false), PLAIN_A(4, 1, 0, false), PLAIN_A(3, 1, 0, false), PLAIN_A(1, 1, 0, false),
    IBL_A(0, 1, 0), IBL_A(1, 1, 0), IBL_A(0, 0, 0), IBL_A(1, 0, 0), IBL_A(0, 1, 1), IBL_A(1, 1, 1), IBL_A(0, 0, 1), IBL_A(1, 0, 1), IBL_A(0, 1, 2), IBL_A(1, 1, 2), IBL_A(0, 0, 2), IBL_A(1, 0, 2),
    // scopes with a blended cascaded draw, behind every older row so that the code object keeps those in their order: MODEL_PBR, MODEL_PBR_IBL, their AREA forms
    OWN(RASTER_CSM_BLEND, raster_kernel_csm_blend, 0, 1), OWN(RASTER_CSM_BLEND, raster_kernel_csm_blend, 1, 1), OWN(RASTER_CSM_BLEND, raster_kernel_csm_blend, 0, 0), OWN(RASTER_CSM_BLEND, raster_kernel_csm_blend, 1, 0),
    IBL(0, 1, 3), IBL(1, 1, 3), IBL(0, 0, 3), IBL(1, 0, 3),
    OWN_A(RASTER_CSM_BLEND, raster_kernel_csm_blend, 0, 1), OWN_A(RASTER_CSM_BLEND, raster_kernel_csm_blend, 1, 1), OWN_A(RASTER_CSM_BLEND, raster_kernel_csm_blend, 0, 0), OWN_A(RASTER_CSM_BLEND, raster_kernel_csm_blend, 1, 0),
    IBL_A(0, 1, 3), IBL_A(1, 1, 3), IBL_A(0, 0, 3), IBL_A(1, 0, 3),
    // 4x multisampled scopes, behind every older raster row: per program set and key
    MSAA(2, 0), MSAA(4, 0), MSAA(3, 0), MSAA(1, 0), MSAA(2, 1), MSAA(4, 1), MSAA(3, 1), MSAA(1, 1),
    // a SKYBOX segment (no key, no bins: one kernel)
    {raster_kernel_id(RASTER_SKY, 0, 0, 0, 1, 0, 4), "sky_kernel", sky_kernel},
    // a recorded transfer command (progs: PassParams::xfer)
    {raster_kernel_id(RASTER_TRANSFER, XFER_COPY, 0, 0, 1, 0, 4), "transfer_copy_kernel", transfer_copy_kernel},
    {raster_kernel_id(RASTER_TRANSFER, XFER_BLIT_NEAREST, 0, 0, 1, 0, 4), "transfer_blit_kernel<0>", transfer_blit_kernel<0>},
    {raster_kernel_id(RASTER_TRANSFER, XFER_BLIT_LINEAR, 0, 0, 1, 0, 4), "transfer_blit_kernel<1>", transfer_blit_kernel<1>},
    {raster_kernel_id(RASTER_TRANSFER, XFER_FILL, 0, 0, 1, 0, 4), "transfer_fill_kernel", transfer_fill_kernel},
    // seamless cube filtering, behind every older row: the SKYBOX segment of a seamless environment, MODEL_PBR_IBL scopes whose set has a seamless
    // cube (per key, triangle-parallel path and shadow term, as the rows of raster_kernel_ibl), their AREA forms
    {raster_kernel_id(RASTER_SKY, 0, 0, 0, 1, 0, 4, 0, 1), "sky_kernel_seamless", sky_kernel_seamless},
    IBL_S(0, 1, 0), IBL_S(1, 1, 0), IBL_S(0, 0, 0), IBL_S(1, 0, 0), IBL_S(0, 1, 1), IBL_S(1, 1, 1), IBL_S(0, 0, 1), IBL_S(1, 0, 1),
    IBL_S(0, 1, 2), IBL_S(1, 1, 2), IBL_S(0, 0, 2), IBL_S(1, 0, 2), IBL_S(0, 1, 3), IBL_S(1, 1, 3), IBL_S(0, 0, 3), IBL_S(1, 0, 3),
    IBL_SA(0, 1, 0), IBL_SA(1, 1, 0), IBL_SA(0, 0, 0), IBL_SA(1, 0, 0), IBL_SA(0, 1, 1), IBL_SA(1, 1, 1), IBL_SA(0, 0, 1), IBL_SA(1, 0, 1),
    IBL_SA(0, 1, 2), IBL_SA(1, 1, 2), IBL_SA(0, 0, 2), IBL_SA(1, 0, 2), IBL_SA(0, 1, 3), IBL_SA(1, 1, 3), IBL_SA(0, 0, 3), IBL_SA(1, 0, 3),
};
#undef IBL_S
#undef IBL_SA
#undef MSAA
#undef IBL
#undef IBL_A
#undef OWN_A
#undef PLAIN_A
#undef ORDERED
#undef OWN
#undef WIDE
#undef PLAIN
static const RasterEntry* raster_entry(const RasterVariant& v) {
    for (const RasterEntry& e : k_raster_entries) if (e.id == v.kernel_id()) return &e;
    return nullptr;
}

hipError_t launch_raster(const PassParams& P, const PassParams* dev_params, uint32_t* big_count, uint32_t programs, hipStream_t stream, LaunchTiming t, bool allow_wide) {
    if (P.tile_row_end == P.tile_row_begin || P.tiles_x == 0) return hipSuccess;
    const RasterVariant v = raster_variant(P, programs, allow_wide);
    const RasterHead H = v.family == RASTER_ORDERED ? ordered_head(P, big_count) : raster_head(P, big_count);
    const RasterEntry* e = raster_entry(v);
    if (!e) return hipErrorInvalidDeviceFunction;       // (a variant without a kernel: the selector and the table disagree)
    raster_trace(e->name);
    MIRHI_LAUNCH(e->kernel, dim3(v.grid[0], v.grid[1], v.grid[2]), dim3(v.block), stream, t, dev_params, H);
    return launch_result();
}

// ---- batched launches --------------------------------------------------------------------------------------------
hipError_t launch_vertex_batch(const PassParams* const* P, const PassParams* const* dev_params, uint32_t n, hipStream_t stream) {
    GeometryBatch B{};
    uint32_t most = 0;
    for (uint32_t i = 0; i < n; i++) { B.params[i] = dev_params[i]; most = P[i]->vs_total_slots > most ? P[i]->vs_total_slots : most; }
    if (most == 0) return hipSuccess;
    hipLaunchKernelGGL(vertex_kernel_batch, dim3(most / GEOM_THREADS, n), dim3(GEOM_THREADS), 0, stream, B);
    return launch_result();
}

hipError_t launch_geometry_batch(const PassParams* const* P, const PassParams* const* dev_params, uint32_t n, hipStream_t stream) {
    GeometryBatch B{};
    uint32_t most = 0, total = 0;
    for (uint32_t i = 0; i < n; i++) {
        B.params[i] = dev_params[i];
        B.head[i] = GeometryHead{P[i]->draws, P[i]->num_draws, (uint32_t)GEOM_THREADS, nullptr, 0u, 0u, 0u};
        B.blocks[i] = P[i]->total_slots / GEOM_THREADS;
        most = B.blocks[i] > most ? B.blocks[i] : most; total += B.blocks[i];
    }
    if (most == 0) return hipSuccess;
    if (total > 5u * 1024u) hipLaunchKernelGGL(geometry_kernel_batch<7>, dim3(most, n), dim3(GEOM_THREADS), 0, stream, B);
    else hipLaunchKernelGGL(geometry_kernel_batch<5>, dim3(most, n), dim3(GEOM_THREADS), 0, stream, B);
    return launch_result();
}

// only the variants a frame loop meets are instantiated in batched form (RasterVariant::batched_form); all of them take the plain key
struct RasterBatchEntry { uint32_t id; const char* name; void (*kernel)(const RasterBatch); };
#define BATCH(P, T, TEAMS) {raster_kernel_id(RASTER_PLAIN, P, 0, T, TEAMS, 0, 4 * TEAMS), "raster_kernel_batch<" #P ", 0, " #T ", " #TEAMS ">", raster_kernel_batch<P, 0, T, TEAMS>}
static const RasterBatchEntry k_raster_batch_entries[] = {
    BATCH(2, 1, 2), BATCH(4, 1, 2), BATCH(2, 1, 1), BATCH(3, 1, 1), BATCH(4, 1, 1), BATCH(1, 1, 1), BATCH(2, 0, 1), BATCH(4, 0, 1), BATCH(3, 0, 1), BATCH(1, 0, 1),
};
#undef BATCH
// the batched instantiation of a variant, or nullptr where none exists
static const RasterBatchEntry* raster_batch_entry(const RasterVariant& v) {
    if (!v.batched_form) return nullptr;
    for (const RasterBatchEntry& e : k_raster_batch_entries) if (e.id == v.kernel_id()) return &e;
    return nullptr;
}

// the scopes are of one variant (mirhi_queue_submit checks): the first one's
hipError_t launch_raster_batch(const PassParams* const* Ps, const PassParams* const* dev_params, uint32_t* const* big_count, uint32_t n, uint32_t programs, hipStream_t stream, hipEvent_t stop) {
    LaunchTiming t{}; t.stop = stop;
    const PassParams& P = *Ps[0];
    if (P.tile_row_end == P.tile_row_begin || P.tiles_x == 0) return hipSuccess;
    const RasterVariant v = raster_variant(P, programs, true);
    const RasterBatchEntry* e = raster_batch_entry(v);
    if (!e) return hipErrorInvalidDeviceFunction;
    raster_trace(e->name);
    RasterBatch B{};
    for (uint32_t i = 0; i < n; i++) { B.params[i] = dev_params[i]; B.head[i] = raster_head(*Ps[i], big_count[i]); }
    MIRHI_LAUNCH(e->kernel, dim3(v.grid[0], v.grid[1], n), dim3(v.block), stream, t, B);
    return launch_result();
}

// ---- multiview depth scopes: the views of one scope in one launch per stage, timed or native like a single scope's launches -----
// P[j]: view slot j's host parameters, dev_params[j] / big_count[j]: its device copy and big-list counter of this submit's parity
hipError_t launch_multiview_vertex(const PassParams* const* P, const PassParams* const* dev_params, uint32_t n, hipStream_t stream, LaunchTiming t) {
    GeometryBatch B{};
    uint32_t most = 0;
    for (uint32_t i = 0; i < n; i++) { B.params[i] = dev_params[i]; most = P[i]->vs_total_slots > most ? P[i]->vs_total_slots : most; }
    if (most == 0) return hipSuccess;
    MIRHI_LAUNCH(vertex_kernel_shadow_batch, dim3(most / GEOM_THREADS, n), dim3(GEOM_THREADS), stream, t, B);
    return launch_result();
}

hipError_t launch_multiview_geometry(const PassParams* const* P, const PassParams* const* dev_params, uint32_t n, hipStream_t stream, LaunchTiming t) {
    GeometryBatch B{};
    const uint32_t tpw = (t.tris_per_wave == 16u || t.tris_per_wave == 32u) ? t.tris_per_wave : (uint32_t)GEOM_THREADS;
    uint32_t most = 0, total = 0;
    for (uint32_t i = 0; i < n; i++) {
        B.params[i] = dev_params[i];
        B.head[i] = GeometryHead{P[i]->draws, P[i]->num_draws, tpw, nullptr, 0u, 0u, 0u};
        B.blocks[i] = P[i]->total_slots / tpw;
        most = B.blocks[i] > most ? B.blocks[i] : most; total += B.blocks[i];
    }
    if (most == 0) return hipSuccess;
    if (total > 5u * 1024u) MIRHI_LAUNCH(geometry_kernel_batch<7>, dim3(most, n), dim3(GEOM_THREADS), stream, t, B);
    else MIRHI_LAUNCH(geometry_kernel_batch<5>, dim3(most, n), dim3(GEOM_THREADS), stream, t, B);
    return launch_result();
}

// the four instantiations of raster_kernel_depth_batch, each named once, in the order of raster_kernel_depth's rows above
#define VIEWS(K, T) {raster_kernel_id(RASTER_DEPTH_VIEWS, 0, K, T, 1, 0, 4), "raster_kernel_depth_batch<" #K ", " #T ">", raster_kernel_depth_batch<K, T>}
static const RasterBatchEntry k_raster_view_entries[] = { VIEWS(0, 1), VIEWS(1, 1), VIEWS(0, 0), VIEWS(1, 0) };
#undef VIEWS
static const RasterBatchEntry* raster_view_entry(const RasterVariant& v) {
    for (const RasterBatchEntry& e : k_raster_view_entries) if (e.id == v.kernel_id()) return &e;
    return nullptr;
}
const char* multiview_raster_name(const RasterVariant& v) { const RasterBatchEntry* e = raster_view_entry(v); return e ? e->name : nullptr; }

hipError_t launch_multiview_raster(const PassParams* const* Ps, const PassParams* const* dev_params, uint32_t* const* big_count, uint32_t n, hipStream_t stream, LaunchTiming t) {
    const PassParams& P = *Ps[0];
    if (P.tile_row_end == P.tile_row_begin || P.tiles_x == 0) return hipSuccess;
    const RasterVariant v = multiview_variant(P, n);
    const RasterBatchEntry* e = raster_view_entry(v);
    if (!e) return hipErrorInvalidDeviceFunction;
    raster_trace(e->name);
    RasterBatch B{};
    for (uint32_t i = 0; i < n; i++) { B.params[i] = dev_params[i]; B.head[i] = raster_head(*Ps[i], big_count[i]); }
    MIRHI_LAUNCH(e->kernel, dim3(v.grid[0], v.grid[1], v.grid[2]), dim3(v.block), stream, t, B);
    return launch_result();
}

hipError_t launch_fragment_count(const PassParams& P, const PassParams* dev_params, uint32_t* big_count, hipStream_t stream, LaunchTiming t) {
    const uint32_t rows = P.tile_row_end - P.tile_row_begin;
    if (rows == 0 || P.tiles_x == 0 || P.ordered_recs || P.depth_only || P.sky || P.xfer) return hipSuccess;
    MIRHI_LAUNCH(fragment_count_kernel, dim3(launch_cols(P), rows), dim3(RASTER_THREADS), stream, t, dev_params, raster_head(P, big_count));
    return launch_result();
}

hipError_t launch_winner_count(const uint32_t* prim, uint32_t pixels, unsigned long long* stats, hipStream_t stream) {
    if (!pixels) return hipSuccess;
    const uint32_t blocks = (pixels + RASTER_THREADS * 16u - 1u) / (RASTER_THREADS * 16u);
    hipLaunchKernelGGL(winner_count_kernel, dim3(blocks), dim3(RASTER_THREADS), 0, stream, prim, pixels, stats);
    return launch_result();
}

// Outside the C ABI (not in include/mirhi.h) and without a HIP call: the kernel, grid and block that launch_raster -- with n_batch >= 2: launch_raster_batch
// of that many scopes -- chooses for a scope of 5 x 4 tiles.  in: programs, allow_wide, then PassParams::pred, zflip, zmask, tp_max_area, raster_teams,
// raster_wide, alpha_scope, xcd_swizzle, "ordered_recs is set", n_batch (0 = single launch).  Returns 1 where no batched form exists.
// programs == PROGS_TRANSFER: in[2] is PassParams::xfer and in[3] the launch's workgroups (PassParams::tiles_x of a transfer entry).
extern "C" int mirhi_debug_raster_choice(const uint32_t in[12], char* name, uint32_t name_len, uint32_t grid_block[4]) {
    static TriRec some_recs;
    PassParams P{};
    P.tiles_x = 5u; P.tile_row_begin = 0u; P.tile_row_end = 4u; P.tile_row_step = 1u;
    P.pred = in[2]; P.zflip = in[3]; P.zmask = in[4]; P.tp_max_area = in[5]; P.raster_teams = in[6]; P.raster_wide = in[7]; P.alpha_scope = in[8]; P.xcd_swizzle = in[9];
    P.ordered_recs = in[10] ? &some_recs : nullptr;
    if (in[0] == PROGS_TRANSFER) { P.xfer = in[2]; P.tiles_x = in[3]; P.tile_row_end = 1u; }      // (a transfer entry: in[2] is what it is -- XFER_* --, in[3] its workgroups)
    const uint32_t n = in[11];
    const RasterVariant v = raster_variant(P, in[0], n >= 2u || in[1] != 0u);
    const RasterBatchEntry* b = n >= 2u ? raster_batch_entry(v) : nullptr;
    if (n >= 2u && !b) return 1;
    snprintf(name, name_len, "%s", b ? b->name : raster_entry(v)->name);
    grid_block[0] = v.grid[0]; grid_block[1] = v.grid[1]; grid_block[2] = b ? n : v.grid[2]; grid_block[3] = v.block;
    return 0;
}

// ... the same for a scope whose latched seamless states are given: ibl_seamless = PassParams::ibl_seamless (bit 0 irradiance, bit 1 prefiltered),
// sky_seamless = PassParams::sky_seamless.  With both 0 it answers what mirhi_debug_raster_choice answers.
extern "C" int mirhi_debug_raster_choice_seamless(const uint32_t in[12], uint32_t ibl_seamless, uint32_t sky_seamless, char* name, uint32_t name_len, uint32_t grid_block[4]) {
    static TriRec some_recs;
    PassParams P{};
    P.tiles_x = 5u; P.tile_row_begin = 0u; P.tile_row_end = 4u; P.tile_row_step = 1u;
    P.pred = in[2]; P.zflip = in[3]; P.zmask = in[4]; P.tp_max_area = in[5]; P.raster_teams = in[6]; P.raster_wide = in[7]; P.alpha_scope = in[8]; P.xcd_swizzle = in[9];
    P.ordered_recs = in[10] ? &some_recs : nullptr;
    P.ibl_seamless = ibl_seamless; P.sky_seamless = sky_seamless;
    const RasterVariant v = raster_variant(P, in[0], in[1] != 0u);
    const RasterEntry* e = raster_entry(v);
    if (!e) return 1;
    snprintf(name, name_len, "%s", e->name);
    grid_block[0] = v.grid[0]; grid_block[1] = v.grid[1]; grid_block[2] = v.grid[2]; grid_block[3] = v.block;
    return 0;
}
// Outside the C ABI and without a HIP call: the name of row `row` of the launch tables above -- table 0 k_raster_entries, 1 k_raster_batch_entries,
// 2 k_raster_view_entries.  Returns 1 past the end of the table (and for a table that does not exist).
extern "C" int mirhi_debug_raster_table(uint32_t table, uint32_t row, char* name, uint32_t name_len) {
    const char* n = nullptr;
    if (table == 0u && row < sizeof k_raster_entries / sizeof k_raster_entries[0]) n = k_raster_entries[row].name;
    if (table == 1u && row < sizeof k_raster_batch_entries / sizeof k_raster_batch_entries[0]) n = k_raster_batch_entries[row].name;
    if (table == 2u && row < sizeof k_raster_view_entries / sizeof k_raster_view_entries[0]) n = k_raster_view_entries[row].name;
    if (!n) return 1;
    snprintf(name, name_len, "%s", n);
    return 0;
}
// The record of raster launches (raster_trace above): on / off (turning it on or off keeps what is recorded), and read-and-clear -- returns the number of launches
// since the last read and writes their entry names, '\n'-joined in launch order, as far as out_len allows (always terminated when out_len > 0).
extern "C" void mirhi_debug_raster_trace(uint32_t enable) { g_raster_trace_on.store(enable ? 1u : 0u, std::memory_order_relaxed); }
extern "C" uint32_t mirhi_debug_raster_trace_read(char* out, uint32_t out_len) {
    std::lock_guard<std::mutex> lock(g_raster_trace_mutex);
    if (!g_raster_trace.empty()) g_raster_trace.pop_back();      // (joined, not terminated)
    if (out && out_len) snprintf(out, out_len, "%s", g_raster_trace.c_str());
    const uint32_t n = g_raster_trace_count;
    g_raster_trace.clear(); g_raster_trace_count = 0u;
    return n;
}
// The device's table of cube edge neighbours (ibl_seamless_tap, mirhi_ibl_sample.hip.h), as plain host code: tap (i, j) of `face` at a level of n x n texels ->
// out[0] the texel's offset from the level's first texel, out[1] 1 for a corner tap.  A test compares it with the float64 model's re-projection.
extern "C" void mirhi_debug_cube_edge_tap(uint32_t n, uint32_t face, int32_t i, int32_t j, uint32_t out[2]) {
    bool corner = false;
    out[0] = ibl_seamless_tap(n, face < 6u ? face : 5u, ibl_edge_row(face), (int)i, (int)j, true, corner);
    out[1] = corner ? 1u : 0u;
}

#ifdef MIRHI_STAMPS
extern "C" int mirhi_debug_read_stamps(uint64_t* dst, uint32_t count) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps), (size_t)count * 8, 0, hipMemcpyDeviceToHost);
}
extern "C" int mirhi_debug_read_geo_stamps(uint64_t* dst, uint32_t count) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps_geo), (size_t)count * 8, 0, hipMemcpyDeviceToHost);
}
extern "C" int mirhi_debug_read_geo_clock(uint64_t* dst, uint32_t count) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stamps_geo_rt), (size_t)count * 8, 0, hipMemcpyDeviceToHost);
}
extern "C" int mirhi_debug_set_stage_limit(uint32_t v) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stage_limit), &v, sizeof v, 0, hipMemcpyHostToDevice);
}
extern "C" int mirhi_debug_clear_stamps() {
    void* p = nullptr;
    hipError_t e = hipGetSymbolAddress(&p, HIP_SYMBOL(g_stamps));
    if (e != hipSuccess) return (int)e;
    return (int)hipMemset(p, 0, sizeof(uint64_t) * 32768 * 8);
}
#endif

}  // namespace mirhi
