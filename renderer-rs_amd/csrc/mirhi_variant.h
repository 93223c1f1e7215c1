// mirhi_variant.h -- which raster kernel a scope runs, with what grid and block.  Decided here and nowhere else: the launchers
// (mirhi_kernels.hip) map the value to a kernel entry, a submit (mirhi_api.hip) compares the values of its command buffers to
// see whether they may share a batched launch.  Plain C++, no HIP: the choice can be stated and tested on a machine without a GPU.
#pragma once
#include "mirhi_device.h"

namespace mirhi {

// The program set of a scope (build_plan -> mirhi_cmd::plan_programs -> launch_raster): which fragment programs its draws name.
enum : uint32_t {
    PROGS_DEPTH_ONLY = 0u,    // the VALUE 0, not a bit: a depth-only scope (SHADOW draws): raster_kernel_depth
    PROGS_TRIANGLE = 1u,      // some draw uses the TRIANGLE program (also what a scope without draws gets)
    PROGS_MODEL = 2u,         // MODEL / MODEL_FULL without mip chains or sRGB textures
    PROGS_PBR = 4u,           // MODEL_PBR, or a MODEL draw with a mip chain or an sRGB texture (the Cook-Torrance variant's programs)
    PROGS_SHADOWED = 8u,      // a MODEL_PBR draw that samples a shadow map (always together with PROGS_PBR): raster_kernel_shadow
    PROGS_CASCADED = 16u,     // ... whose shadow term is CalculateShadowCSM (always together with PROGS_SHADOWED): raster_kernel_csm
    PROGS_IBL = 32u,          // a MODEL_PBR_IBL draw (always together with PROGS_PBR; with PROGS_SHADOWED / PROGS_CASCADED when its draws are shadowed): raster_kernel_ibl
    PROGS_SKY = 64u,          // the VALUE 64, alone: a SKYBOX segment (one SKYBOX draw, no triangles or bins): sky_kernel
    PROGS_TRANSFER = 128u,    // the VALUE 128, alone: a recorded transfer command (no scope at all): the kernels of mirhi_transfer.hip.h, by PassParams::xfer
    PROGS_CSM_BLEND = 256u,   // a bit again (64 and 128 are values used alone: the first free bit above them): some cascaded draw's shadow term is
                              // CalculateShadowCSMBlended with a threshold > 0 (always together with PROGS_CASCADED): raster_kernel_csm_blend, the blended raster_kernel_ibl
};

// (RASTER_IBL behind RASTER_ORDERED, RASTER_SKY behind RASTER_IBL, RASTER_TRANSFER behind RASTER_SKY, RASTER_CSM_BLEND behind RASTER_TRANSFER, RASTER_MSAA behind
// RASTER_CSM_BLEND: the values of the families before them are recorded in tests/golden/raster_variants.json)
enum RasterFamily : uint32_t { RASTER_PLAIN, RASTER_WIDE, RASTER_DEPTH, RASTER_SHADOW, RASTER_CSM, RASTER_ORDERED, RASTER_IBL, RASTER_SKY, RASTER_TRANSFER, RASTER_CSM_BLEND, RASTER_MSAA };
// ... and behind RASTER_MSAA, the last value of the list above: the views of a multiview depth scope in one launch (raster_kernel_depth_batch).  Never
// what raster_variant answers: multiview_variant below is the one place that names it.
constexpr RasterFamily RASTER_DEPTH_VIEWS = (RasterFamily)(RASTER_MSAA + 1u);

// the kernel instantiation alone (no launch shape) as one word
constexpr uint32_t raster_kernel_id(uint32_t family, uint32_t progs, uint32_t keyed, uint32_t tp, uint32_t teams, uint32_t masked, uint32_t waves, uint32_t area = 0u, uint32_t seamless = 0u) {
    return family | progs << 4 | keyed << 8 | tp << 12 | teams << 16 | masked << 20 | waves << 24 | area << 30 | seamless << 31;
}

// One raster launch: the kernel family and its template arguments, the grid and the block.  Equal values <=> the same kernel
// instantiation with the same launch shape.
struct RasterVariant {
    RasterFamily family;
    uint32_t progs;           // PROGS of raster_kernel / raster_kernel_wide / ordered_kernel: 1 .. 4 (0: the family takes none); RASTER_IBL: its SHADOWV, 0 .. 3
    uint32_t keyed;           // KEYED: 0 the plain key (raw float bits: LESS / LESS_OR_EQUAL), 1 the generic key, 2 predicate mode
    uint32_t tp;              // TP: 1 = with the triangle-parallel path
    uint32_t teams;           // TEAMS: 1, or 2 (the two-team mesh variants)
    uint32_t masked;          // 1: the alpha-masked variant (PassParams::alpha_scope)
    uint32_t waves;           // waves per tile: 4 x teams, or 8 / 16 (raster_kernel_wide)
    uint32_t grid[3], block;
    uint32_t batched_form;    // 1: a raster_kernel_batch instantiation exists for it and the scope may take it (plain tile order, no wide plan)
    uint32_t area;            // 1: the AREA instantiation (a partial render area); the ordered, sky and transfer kernels have one form
    uint32_t seamless;        // 1: the SEAMLESS instantiation (RASTER_IBL: a cube of the scope's IBL set is seamless; RASTER_SKY: the environment is); 0 for every other family
    constexpr uint32_t kernel_id() const { return raster_kernel_id(family, progs, keyed, tp, teams, masked, waves, area, seamless); }
    bool operator==(const RasterVariant& o) const {
        return kernel_id() == o.kernel_id() && grid[0] == o.grid[0] && grid[1] == o.grid[1] && grid[2] == o.grid[2] && block == o.block && batched_form == o.batched_form;
    }
};

// allow_wide: false = the scope's plain / two-team variant even if its plan names a wide one (PassParams::raster_wide): a submit's choice
inline RasterVariant raster_variant(const PassParams& P, uint32_t programs, bool allow_wide) {
    const uint32_t rows = P.tile_row_end - P.tile_row_begin;
    const uint32_t cols = launch_cols(P);      // (the render area's tile columns: all of them unless the area is partial)
    if (programs == PROGS_SKY) {
        // a SKYBOX segment: one 256-thread workgroup per tile of the owned rows, always the 2-D grid; no key, no bins, no batched form
        // (the environment's seamless state, latched by the draw: sky_kernel_seamless)
        return RasterVariant{RASTER_SKY, 0u, 0u, 0u, 1u, 0u, 4u, {cols, rows, 1u}, (uint32_t)RASTER_THREADS, 0u, 0u, P.sky_seamless ? 1u : 0u};
    }
    if (programs == PROGS_TRANSFER) {
        // a transfer entry: its kernel by what it is (progs = XFER_*), a 1-D grid of PassParams::tiles_x workgroups (the host's count: a blit's tiles, the
        // capped work units of a copy or clear); no key, no bins, no batched form
        return RasterVariant{RASTER_TRANSFER, P.xfer, 0u, 0u, 1u, 0u, 4u, {P.tiles_x * rows, 1u, 1u}, (uint32_t)RASTER_THREADS, 0u, 0u};
    }
    const uint32_t progs = programs >= PROGS_PBR ? 4u : ((programs == 2u || programs == 3u) ? programs : 1u);
    if (P.samples == 4u) {
        // a 4x multisampled scope: a family of its own like the shadowed and IBL ones -- one team of four waves, single-list bins, plain tile
        // order, an ordered key, pixel-parallel only (mirhi_scope.h refuses everything else where it is recorded); never batched
        return RasterVariant{RASTER_MSAA, progs, (P.zflip == 0u && P.zmask == 0xFFFFFFFFu) ? 0u : 1u, 0u, 1u, 0u, 4u, {cols, rows, 1u}, (uint32_t)RASTER_THREADS, 0u, 0u};
    }
    const bool mesh = programs == PROGS_MODEL || programs >= PROGS_PBR;      // no TRIANGLE draw: what the two-team and wide variants exist for
    // the plain key (raw float bits) serves LESS / LESS_OR_EQUAL; everything else takes the generic key
    const bool plain = P.zflip == 0u && P.zmask == 0xFFFFFFFFu;
    const uint32_t tp = P.tp_max_area ? 1u : 0u;
    RasterVariant v = {RASTER_PLAIN, progs, plain ? 0u : 1u, tp, 1u, 0u, 4u, {cols, rows, 1u}, 0u, 0u, 0u};
    if (P.ordered_recs) {           // ordered segment: fragments in primitive order (blending); always the 2-D grid
        v.family = RASTER_ORDERED; v.keyed = 0u; v.tp = 0u;
        v.block = (uint32_t)ORDERED_THREADS;
        return v;
    }
    if (P.xcd_swizzle > 1u) { v.grid[0] = P.tiles_x * rows; v.grid[1] = 1u; }      // (never with a partial render area: raster_mode)
    // a partial render area: the AREA instantiation of whatever is chosen below -- one team of four waves (raster_mode plans neither two teams nor a wide variant for it)
    const bool area = P.area_partial != 0u;
    v.area = area ? 1u : 0u;
    if (programs & PROGS_IBL) {
        // a scope with a MODEL_PBR_IBL draw: a family of its own like the shadowed ones (one team of four waves, single-list bins, plain tile order, an
        // ordered key), one kernel per shadow term of its draws
        v.family = RASTER_IBL;
        v.progs = (programs & PROGS_CSM_BLEND) ? 3u : ((programs & PROGS_CASCADED) ? 2u : ((programs & PROGS_SHADOWED) ? 1u : 0u));
        v.seamless = P.ibl_seamless ? 1u : 0u;      // a cube of the set was seamless when the draws were recorded: raster_kernel_ibl_seamless
    } else if (programs == PROGS_DEPTH_ONLY || (programs & PROGS_SHADOWED)) {
        // depth-only scopes and scopes with a shadowed draw have variants of their own, whatever the selectors below would pick (the host keeps
        // them on one team of four waves, single-list bins and the plain tile order; their key is an ordered one, never a predicate)
        v.family = programs == PROGS_DEPTH_ONLY ? RASTER_DEPTH : ((programs & PROGS_CSM_BLEND) ? RASTER_CSM_BLEND : ((programs & PROGS_CASCADED) ? RASTER_CSM : RASTER_SHADOW));
        v.progs = 0u;
    } else if (P.raster_wide && allow_wide && !P.pred && tp && !P.alpha_scope && mesh && P.xcd_swizzle <= 1u && !area) {
        // the wide mesh variants: eight or sixteen waves per tile (host-side choice, PassParams::raster_wide = waves per tile)
        v.family = RASTER_WIDE;
        v.waves = P.raster_wide >= 16u ? 16u : 8u;
    } else if (P.pred) {            // (the host keeps tp_max_area = 0 for predicate scopes)
        v.keyed = 2u; v.tp = 0u;
    } else if (tp) {
        if (P.raster_teams == 2u && mesh && !area) { v.teams = 2u; v.waves = 8u; }      // only the pure mesh variants exist with two teams
        if (P.alpha_scope) { v.masked = 1u; v.progs = 4u; }                     // alpha-masked scope: always with the triangle-parallel path and a PBR draw
    }
    v.block = v.waves * 64u;
    // only the variants a frame loop meets are instantiated in batched form: LESS / LESS_OR_EQUAL keys, with and without the triangle-parallel path and
    // the two-team mesh mode.  The XCD run-length order of a 1-D grid is a measurement knob, and a plan that names a wide variant keeps it whether or
    // not one submit takes it: neither is batched.  Nor is a scope with a partial render area (mirhi_submit.h).
    v.batched_form = (v.family == RASTER_PLAIN && v.keyed == 0u && !P.alpha_scope && P.xcd_swizzle <= 1u && !P.raster_wide && !P.area_partial) ? 1u : 0u;
    return v;
}

// The raster launch of a multiview depth scope (mirhi_cmd_begin_rendering_multiview) of `views` views: what a single view's depth-only scope would
// run (P: any view's parameters -- they differ in addresses alone), as the batched depth kernel raster_kernel_depth_batch with one grid layer per view.  Never
// an AREA form (a partial render area is refused where the scope is recorded), never batched across command buffers.
inline RasterVariant multiview_variant(const PassParams& P, uint32_t views) {
    RasterVariant v = raster_variant(P, PROGS_DEPTH_ONLY, false);
    v.family = RASTER_DEPTH_VIEWS; v.grid[2] = views; v.batched_form = 0u; v.area = 0u;
    return v;
}

// The by-value kernel argument of a scope's raster (and fragment-count) kernel
inline RasterHead raster_head(const PassParams& P, uint32_t* big_count) {
    return RasterHead{P.bin_count, P.bin_pool, big_count, P.tiles_x, P.tile_row_begin | P.tile_col_begin << 16, P.bin_cap, P.big_cap, P.sub_cap, P.count_stride, P.fixed_recs, P.tile_row_step};
}
// ... of an ordered segment: nothing is binned, a tile's single list has no fixed pages
inline RasterHead ordered_head(const PassParams& P, uint32_t* big_count) {
    RasterHead H = raster_head(P, big_count);
    H.sub_cap = P.bin_cap; H.count_stride = 0u; H.fixed_recs = 0u;
    return H;
}

}  // namespace mirhi
