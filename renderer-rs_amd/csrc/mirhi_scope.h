// mirhi_scope.h -- what kind of rendering scope a recorded segment is and how it is rastered.  Decided here and nowhere else: record_draw
// (mirhi_api.hip) builds a DepthState per draw, build_plan asks classify_scope / raster_mode / bin_geometry once per scope and writes the
// answers into PassParams, raster_variant (mirhi_variant.h) turns those into a kernel.  Plain C++, no HIP: the decisions can be stated and
// tested on a machine without a GPU (mirhi_debug_scope_plan, tests/test_scope_plan_cpu.py).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>      // environ

#include "../../include/mirhi.h"
#include "mirhi_device.h"
#include "mirhi_variant.h"

namespace mirhi {

// The depth / blend state of a segment: one raster launch resolves one of them (DESIGN.md "Depth key"), a draw with another one starts a new segment.
struct DepthState {
    bool key_set = false;                  // some draw has set the state (a scope without draws: every fragment passes, nothing is written)
    uint32_t test = 0, compare = 0, write = 0, discard = 0;      // as recorded: compare ALWAYS and no write when the depth test is off
    uint32_t blend[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // enable, src colour, dst colour, colour op, src alpha, dst alpha, alpha op, write mask
    bool operator==(const DepthState& o) const {
        return key_set == o.key_set && test == o.test && compare == o.compare && write == o.write && discard == o.discard && memcmp(blend, o.blend, sizeof blend) == 0;
    }
    // NotEqual with depth write: the stored depth depends on the order of all fragments
    bool order_dependent_depth() const { return test && write && compare == MIRHI_COMPARE_NOT_EQUAL; }
};

// the compare ops under which the nearest (or farthest) fragment wins: what a depth key resolves by minimum
inline bool ordering_compare(uint32_t op) {
    return op == MIRHI_COMPARE_LESS || op == MIRHI_COMPARE_LESS_OR_EQUAL || op == MIRHI_COMPARE_GREATER || op == MIRHI_COMPARE_GREATER_OR_EQUAL;
}

// Draws whose raster variants resolve ordered depth keys only (a shadow map, cascades, MODEL_PBR_IBL): no blending, no fragment discard, no
// predicate depth state.  needs_test: no key without the depth test either (cascades: SV_Position.z is the depth the key holds).
inline bool ordered_key_only(const DepthState& s, bool needs_test) {
    if (s.blend[0] || s.discard) return false;
    if (!s.test) return !needs_test;
    return s.write && ordering_compare(s.compare);
}

// The eight PassParams fields that make a scope's depth key
struct DepthKey {
    uint32_t clear_depth_bits, pred, zflip, zmask, idflip, strict, init_zk, init_idk;
};

inline DepthKey depth_key_setup(const DepthState& s, float clear_depth) {
    DepthKey P;
    const uint32_t cbits = [&] { float f = clear_depth; f = f > 0.0f ? (f < 1.0f ? f : 1.0f) : 0.0f; uint32_t u; memcpy(&u, &f, 4); return u; }();
    P.clear_depth_bits = cbits;
    P.pred = 0;
    const uint32_t op = s.key_set ? s.compare : (uint32_t)MIRHI_COMPARE_ALWAYS;
    const bool test = s.key_set && s.test;
    const bool write = test && s.write;
    if (!test || (op == MIRHI_COMPARE_ALWAYS && !write)) {      // every fragment passes, nothing is written: later primitive wins
        P.zflip = 0; P.zmask = 0; P.idflip = 1; P.strict = 0; P.init_zk = 0; P.init_idk = NO_PRIM; return P;
    }
    const bool ordered = write && ordering_compare(op);
    if (!ordered) {
        // Predicate mode.  Without depth write (or with Equal, which can only rewrite the same value) the stored depth
        // never changes inside the scope: every fragment is tested against the depth the scope started with and the latest
        // passing primitive owns the pixel.  Always with write: everything passes, the latest primitive's depth is stored.
        static const uint32_t bits[8] = {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u};     // Never, Less, Equal, LessOrEqual, Greater, NotEqual, GreaterOrEqual, Always
        P.pred = bits[op & 7u] | (op == MIRHI_COMPARE_ALWAYS ? 8u : 0u);
        if (P.pred == 0) P.pred = 16u;                                           // (Never is dropped at record time; keep the mode bit set)
        P.zflip = 0; P.zmask = 0xFFFFFFFFu; P.idflip = 1; P.strict = 0;
        P.init_zk = cbits; P.init_idk = NO_PRIM;
        return P;
    }
    const bool greater = (op == MIRHI_COMPARE_GREATER || op == MIRHI_COMPARE_GREATER_OR_EQUAL);
    P.strict = (op == MIRHI_COMPARE_LESS || op == MIRHI_COMPARE_GREATER) ? 1u : 0u;
    P.zflip = greater ? 0xFFFFFFFFu : 0u;
    P.zmask = 0xFFFFFFFFu;
    P.idflip = P.strict ? 0u : 1u;            // strict: earlier primitive keeps ties; or-equal: later primitive wins
    const uint32_t t = cbits ^ P.zflip;
    if (!P.strict) { P.init_zk = t; P.init_idk = NO_PRIM; }
    else if (t == 0u) { P.init_zk = 0u; P.init_idk = 0u; }   // nothing can pass
    else { P.init_zk = t - 1u; P.init_idk = NO_PRIM; }
    return P;
}

// The MIRHI_* measurement knobs the plan and the submit consult (A/B runs, tests).  Read at the start of every build_plan and every submit -- not
// once per process: tests change them between plans -- and passed down by value; nothing below asks the environment again.  `set` is kept beside
// the number: several knobs mean something unset that no value says (MIRHI_RASTER_WIDE=0 forces the plain variant, unset leaves the feedback on).
struct PlanKnobs {
    struct Knob { bool set = false; int value = 0; };      // value: atoi of the variable's text
    Knob masked_ordered;    // MIRHI_MASKED_ORDERED != 0: alpha-masked scopes take the ordered resolve
    Knob tp_density;        // MIRHI_TP_DENSITY: triangles per tile from which the triangle-parallel path is on
    Knob tp_max_area;       // MIRHI_TP_MAX_AREA: its box limit in pixels (0 = off)
    Knob raster_teams;      // MIRHI_RASTER_TEAMS: 1 / 2
    Knob xcd_bins;          // MIRHI_XCD_BINS=0: no per-XCD bins with two teams
    Knob raster_wide;       // MIRHI_RASTER_WIDE: 0 / 8 / 16 waves per tile, whatever the busy-tile feedback says
    Knob bin_cap;           // MIRHI_BIN_CAP: records per list (spill tests)
    Knob fixed_pages;       // MIRHI_FIXED_PAGES: fixed pages per tile, 1 .. 8
    Knob pool_pages;        // MIRHI_POOL_PAGES: dynamic pool pages (pool-exhaustion test); the pool then never grows
    Knob always_clear;      // MIRHI_ALWAYS_CLEAR: counters and page table cleared at every plan
    Knob xcd_run;           // MIRHI_XCD_RUN: run length of the XCD tile order (1 = plain order)
    Knob verify_idle;       // MIRHI_VERIFY_IDLE: build_plan checks on the host that the workspace was left re-armed
    // one walk over the environment (a getenv per knob would walk it twelve times, on the path of every submit); the first entry of a name counts, as with getenv
    static PlanKnobs read() {
        static const struct { const char* name; Knob PlanKnobs::*field; } table[] = {
            {"MASKED_ORDERED", &PlanKnobs::masked_ordered}, {"TP_DENSITY", &PlanKnobs::tp_density}, {"TP_MAX_AREA", &PlanKnobs::tp_max_area},
            {"RASTER_TEAMS", &PlanKnobs::raster_teams}, {"XCD_BINS", &PlanKnobs::xcd_bins}, {"RASTER_WIDE", &PlanKnobs::raster_wide},
            {"BIN_CAP", &PlanKnobs::bin_cap}, {"FIXED_PAGES", &PlanKnobs::fixed_pages}, {"POOL_PAGES", &PlanKnobs::pool_pages},
            {"ALWAYS_CLEAR", &PlanKnobs::always_clear}, {"XCD_RUN", &PlanKnobs::xcd_run}, {"VERIFY_IDLE", &PlanKnobs::verify_idle}};
        PlanKnobs k;
        for (char** e = environ; e && *e; e++) {
            if (strncmp(*e, "MIRHI_", 6) != 0) continue;
            const char* name = *e + 6;
            const char* eq = strchr(name, '=');
            if (!eq) continue;
            for (const auto& t : table) {
                Knob& knob = k.*t.field;
                if (!knob.set && strlen(t.name) == (size_t)(eq - name) && strncmp(name, t.name, (size_t)(eq - name)) == 0) { knob.set = true; knob.value = atoi(eq + 1); }
            }
        }
        return k;
    }
};

// The render area of a scope (mirhi_rendering_info::render_area) on an attachment of W x H pixels: whether it is valid, the rectangle
// it stands for, and the tiles a scope launches for it.  The tile grid is the attachment's (32 x 32 tiles from pixel (0, 0)) and pixel coordinates
// stay absolute -- an area only selects the tile columns [col_begin, col_end) and rows [row_begin, row_end) that intersect it; the kernels then
// test every pixel against the rectangle (in_area).  w <= 0 or h <= 0: the full extent.
struct RenderArea {
    bool valid;                 // x >= 0, y >= 0, x + w <= W, y + h <= H (in 64 bits); nothing else below is meaningful otherwise
    uint32_t x, y, w, h;        // the rectangle in pixels (the full extent spelled out)
    bool partial;               // smaller than the attachment
    uint32_t col_begin, col_end, row_begin, row_end;      // tiles launched
    bool edge_partial;          // some launched tile lies only partly inside the rectangle: an area edge off the tile grid, or the attachment's own ragged edge
    uint32_t tiles;             // launched tiles: what raster_mode / bin_geometry take as the scope's tile count
    uint32_t index_tiles;       // tiles the bins, counters and page table are indexed by: all columns of the attachment x the launched rows
};
inline RenderArea render_area(uint32_t W, uint32_t H, const int32_t area[4]) {
    RenderArea a{};
    const uint32_t T = (uint32_t)TILE;
    const bool full = area[2] <= 0 || area[3] <= 0;
    const int64_t x = full ? 0 : area[0], y = full ? 0 : area[1], w = full ? (int64_t)W : area[2], h = full ? (int64_t)H : area[3];
    a.valid = x >= 0 && y >= 0 && x + w <= (int64_t)W && y + h <= (int64_t)H;
    if (!a.valid) return a;
    a.x = (uint32_t)x; a.y = (uint32_t)y; a.w = (uint32_t)w; a.h = (uint32_t)h;
    a.partial = a.x != 0u || a.y != 0u || a.w != W || a.h != H;
    const bool none = a.w == 0u || a.h == 0u;      // (an attachment without pixels)
    a.col_begin = none ? 0u : a.x / T; a.col_end = none ? 0u : (a.x + a.w + T - 1u) / T;
    a.row_begin = none ? 0u : a.y / T; a.row_end = none ? 0u : (a.y + a.h + T - 1u) / T;
    a.edge_partial = !none && (a.x % T != 0u || a.y % T != 0u || (a.x + a.w) % T != 0u || (a.y + a.h) % T != 0u);
    a.tiles = (a.col_end - a.col_begin) * (a.row_end - a.row_begin);
    a.index_tiles = ((W + T - 1u) / T) * (a.row_end - a.row_begin);
    return a;
}
// what begin_rendering answers an invalid area with
inline void render_area_message(char* buf, size_t len, const int32_t area[4], uint32_t W, uint32_t H) {
    snprintf(buf, len, "Invalid handle: render area (x %d, y %d, width %d, height %d) does not lie inside the %u x %u attachment", area[0], area[1], area[2], area[3], W, H);
}

// What kind of scope a segment is: everything about it that does not depend on how many triangles or tiles it has.
struct ScopeClass {
    DepthKey key;
    // ordered: resolved fragment by fragment in primitive order (ordered_kernel) -- its colour is blended, its depth state makes the stored depth
    // depend on the order of all fragments (NotEqual with depth write), or its fragment program may discard single fragments
    // (mirhi_pipeline_desc::fragment_discard_enable: visibility then needs the program's result) ...
    bool ordered;
    // ... unless it is masked_plain: fragment_discard_enable without blending under a depth state the depth key resolves by minimum (not a predicate
    // state): visibility stays order-independent -- a kept fragment competes by its key -- so the segment keeps bins and the raster kernel, and alpha
    // is tested per covered pixel in front of the key minimum (PassParams::alpha_scope, raster_small_masked).  MIRHI_MASKED_ORDERED=1 (A/B runs):
    // the ordered resolve instead.
    bool masked_plain;
    bool tri_prog;            // some draw uses the TRIANGLE program
    bool has_draws;
    uint32_t shadowed;        // 0, 1: a draw samples a single shadow map, 2: shadow cascades (never both in one scope: record_draw), 3: cascades, and some cascaded draw
                              // blends (DrawDesc::csm_blend > 0; an unblended cascaded draw of such a scope is a blended one with threshold 0)
    uint32_t ibl;             // 1: a MODEL_PBR_IBL draw
    // Depth-only scopes, scopes with a shadowed draw and scopes with a MODEL_PBR_IBL draw have raster variants of their own (raster_kernel_depth /
    // _shadow / _csm / _ibl): one team of four waves per tile, single-list bins, plain tile order -- the team and wide selectors leave them alone.
    bool own_family;
    uint32_t programs;        // the scope's program set (mirhi_variant.h: PROGS_*)
    // A SKYBOX segment (one SKYBOX draw, always a segment of its own: record_draw): no triangles, vertex jobs or bins; its raster launch is sky_kernel.
    // A family of its own: plain tile order, no wide or two-team variant, no triangle-parallel path.
    bool sky;
    // A recorded transfer command (include/mirhi.h "Transfer commands"): no scope at all -- no attachments, draws, key or bins; its one launch is a kernel of
    // mirhi_transfer.hip.h.  A class of its own, treated by the selectors as a sky segment is.
    bool transfer;
    // A 4x multisampled scope (mirhi_cmd_begin_rendering_resolve): 4, else 1.  A family of its own (raster_kernel_msaa): one team of four waves,
    // single-list bins, plain tile order, pixel-parallel only; what its kernel does not take is refused where it is recorded (msaa_scope_refusal, msaa_draw_refusal).
    uint32_t samples;
};

// ---- 4x multisampled scopes: what is refused, with the words it is refused in ("Invalid handle: " in front, mirhi_api.hip) ----
// the sample count of mirhi_image_create_multisampled; nullptr: accepted (4)
inline const char* msaa_sample_count_refusal(uint32_t samples) {
    if (samples == 4u) return nullptr;
    if (samples == 1u) return "a multisampled image has more than one sample: use mirhi_image_create";
    return "unsupported: sample count";
}
// What begin_rendering_resolve looks at, as numbers (images: 0 = NULL; formats mirhi_format; modes mirhi_resolve_mode)
struct MsaaScopeFacts {
    uint32_t color_samples, color_format, color_w, color_h;
    int32_t color_load_op, color_store_op;
    uint32_t has_depth, depth_samples, depth_format, depth_w, depth_h;
    int32_t depth_load_op, depth_store_op;
    uint32_t has_color_resolve, cr_samples, cr_format, cr_w, cr_h, cr_same_device; int32_t color_resolve_mode;
    uint32_t has_depth_resolve, dr_samples, dr_format, dr_w, dr_h, dr_same_device; int32_t depth_resolve_mode;
    uint32_t has_prim, prim_format, prim_w, prim_h;
    uint32_t area_partial, split_device, fragment_stats;
};
// nullptr: the scope is accepted.  (The colour image is multisampled: the 1x case never gets here.)
inline const char* msaa_scope_refusal(const MsaaScopeFacts& f) {
    if (f.color_format != MIRHI_FORMAT_B8G8R8A8_SRGB && f.color_format != MIRHI_FORMAT_R32G32B32A32_SFLOAT) return "a multisampled color attachment has a non-colour format";
    if (f.color_load_op != MIRHI_LOAD_OP_CLEAR || f.color_store_op != MIRHI_STORE_OP_DONT_CARE)
        return "unsupported: multisampled attachments are transient (colour: load CLEAR, store DONT_CARE)";
    if (!f.has_color_resolve || f.color_resolve_mode != MIRHI_RESOLVE_AVERAGE) return "a multisampled color attachment needs a color_resolve_image with MIRHI_RESOLVE_AVERAGE";
    if (f.cr_samples != 1u) return "the color_resolve_image is multisampled itself";
    if (!f.cr_same_device) return "the color_resolve_image belongs to another device";
    if (f.cr_format != f.color_format || f.cr_w != f.color_w || f.cr_h != f.color_h) return "the color_resolve_image must have the multisampled attachment's format and extent";
    if (f.has_depth) {
        if (f.depth_samples != 4u) return "a multisampled color attachment with a single-sampled depth attachment (depth_image: NULL, or a multisampled D32_SFLOAT)";
        if (f.depth_format != MIRHI_FORMAT_D32_SFLOAT) return "depth attachment is not D32_SFLOAT";
        if (f.depth_w != f.color_w || f.depth_h != f.color_h) return "depth attachment extent does not match the colour attachment";
        if (f.depth_load_op != MIRHI_LOAD_OP_CLEAR || f.depth_store_op != MIRHI_STORE_OP_DONT_CARE)
            return "unsupported: multisampled attachments are transient (depth: load CLEAR, store DONT_CARE)";
    }
    if (f.has_depth_resolve || f.depth_resolve_mode != MIRHI_RESOLVE_NONE) {
        if (!f.has_depth_resolve || f.depth_resolve_mode != MIRHI_RESOLVE_SAMPLE_ZERO) return "unsupported: a depth resolve is a depth_resolve_image with MIRHI_RESOLVE_SAMPLE_ZERO";
        if (f.dr_samples != 1u) return "the depth_resolve_image is multisampled itself";
        if (!f.dr_same_device) return "the depth_resolve_image belongs to another device";
        if (f.dr_format != MIRHI_FORMAT_D32_SFLOAT || f.dr_w != f.color_w || f.dr_h != f.color_h) return "the depth_resolve_image must be D32_SFLOAT with the multisampled attachment's extent";
    }
    if (f.has_prim && (f.prim_format != MIRHI_FORMAT_R32_UINT || f.prim_w != 4u * f.color_w || f.prim_h != f.color_h))
        return "prim_id_image of a multisampled scope must be R32_UINT of 4 * width x height texels (texel (4 px + s, py): sample s)";
    if (f.area_partial) return "unsupported: a partial render area in a multisampled scope";
    if (f.split_device) return "unsupported: a multisampled scope on a split device";
    if (f.fragment_stats) return "unsupported: fragment statistics of a multisampled scope";
    return nullptr;
}
// The program of a draw recorded in a multisampled scope (mirhi_program) and whether it samples a shadow map or cascades.  record_draw asks this for a SHADOW
// pipeline ahead of its depth-only check, so that the draw gets this refusal and not the 1x one.  nullptr: accepted.
inline const char* msaa_program_refusal(int32_t program, bool shadowed) {
    if (program == MIRHI_PROGRAM_SKYBOX) return "unsupported: a SKYBOX draw in a multisampled scope";
    if (program == MIRHI_PROGRAM_SHADOW) return "unsupported: a SHADOW draw in a multisampled scope";
    if (program == MIRHI_PROGRAM_MODEL_PBR_IBL) return "unsupported: a MODEL_PBR_IBL draw in a multisampled scope";
    if (shadowed) return "unsupported: a shadowed or cascaded draw in a multisampled scope";
    return nullptr;
}
// A draw recorded in a multisampled scope: its depth / blend state, its program (mirhi_program), whether it samples a shadow map or cascades, and whether
// the segment already holds draws of another state (which would cut the scope into a second segment).  nullptr: accepted.
inline const char* msaa_draw_refusal(const DepthState& s, int32_t program, bool shadowed, bool state_change) {
    if (s.blend[0]) return "unsupported: blending in a multisampled scope";
    if (s.discard) return "unsupported: fragment_discard_enable in a multisampled scope";
    if (!ordered_key_only(s, true)) return "unsupported: a predicate depth state in a multisampled scope (depth test and write with LESS, LESS_OR_EQUAL, GREATER or GREATER_OR_EQUAL)";
    if (state_change) return "unsupported: a depth state change inside a multisampled scope (it would cut the scope into a second segment)";
    return msaa_program_refusal(program, shadowed);
}

inline ScopeClass classify_scope(const DepthState& s, float clear_depth, const DrawDesc* draws, size_t n, bool depth_only, const PlanKnobs& knobs, bool sky = false, bool transfer = false,
                                 uint32_t samples = 1u) {
    ScopeClass c{};
    c.samples = samples == 4u ? 4u : 1u;
    c.key = depth_key_setup(s, clear_depth);
    if (transfer) { c.transfer = true; c.own_family = true; c.programs = PROGS_TRANSFER; return c; }
    if (sky) {      // (the depth state is the sky kernel's own business: PassParams::sky_compare / sky_write; nothing of the segment is ordered or masked)
        c.sky = true; c.has_draws = true; c.own_family = true; c.programs = PROGS_SKY;
        return c;
    }
    c.has_draws = n != 0;
    uint32_t progs = 0;
    bool sampler_state = false;
    for (size_t i = 0; i < n; i++) {
        const DrawDesc& dd = draws[i];
        sampler_state |= dd.program == MIRHI_PROGRAM_MODEL_PBR && draw_has_base_sampler_state(dd);
        c.tri_prog |= dd.program == MIRHI_PROGRAM_TRIANGLE;
        c.shadowed |= dd.shadow_map ? (dd.shadow_layers ? (dd.csm_blend > 0.0f ? 3u : 2u) : 1u) : 0u;
        c.ibl |= dd.program == MIRHI_PROGRAM_MODEL_PBR_IBL ? 1u : 0u;
        progs |= dd.program == MIRHI_PROGRAM_TRIANGLE ? PROGS_TRIANGLE : ((dd.program == MIRHI_PROGRAM_MODEL_PBR || dd.program == MIRHI_PROGRAM_MODEL_PBR_IBL || dd.tex_any_mips || dd.tex_srgb || draw_has_sampler_state(dd)) ? PROGS_PBR : PROGS_MODEL);
    }
    // A MODEL_PBR draw whose BASE COLOUR texture has sampler state (mirhi_image_set_sampler) keeps a discard scope out of the masked raster variants:
    // their alpha test (pbr_base_alpha: texture 0 of MODEL_PBR draws, nothing else) samples under the default sampler only -- those kernels sit at
    // their register ceiling, DESIGN.md 8i -- so such a scope takes the ordered resolve, which shades every fragment through the full sampler, as
    // MIRHI_MASKED_ORDERED=1 makes every discard scope do.  State on the other four textures, or on a draw of another program, changes nothing here:
    // the variants' shading of the winning fragment knows the state.
    c.masked_plain = s.key_set && s.discard && s.blend[0] == 0 && !s.order_dependent_depth() && !(knobs.masked_ordered.set && knobs.masked_ordered.value != 0) &&
                     c.key.pred == 0u && !sampler_state;
    c.ordered = s.key_set && (s.blend[0] != 0 || (s.discard != 0 && !c.masked_plain) || s.order_dependent_depth());
    c.own_family = depth_only || c.shadowed || c.ibl || c.samples == 4u;
    const uint32_t cascaded = (c.shadowed >= 2u ? PROGS_CASCADED : 0u) | (c.shadowed == 3u ? PROGS_CSM_BLEND : 0u);
    if (c.shadowed) progs = PROGS_PBR | PROGS_SHADOWED | cascaded;
    if (c.ibl) progs = PROGS_PBR | PROGS_IBL | (c.shadowed ? PROGS_SHADOWED : 0u) | cascaded;
    c.programs = depth_only ? PROGS_DEPTH_ONLY : (progs ? progs : PROGS_TRIANGLE);
    return c;
}

// How a scope is rastered (used for sizing the workspace and for the launch):
//  tp_max_area  triangle-parallel resolve of small records pays when tiles hold many triangles (meshes); sparse scopes keep
//               the leaner pixel-parallel-only kernel.  Scopes of TRIANGLE-program draws switch at 16 triangles per tile on
//               average (their variant gives up one wave of occupancy for the LDS key array); mesh-program scopes lose nothing
//               and a mesh covers a fraction of the frame (the dancer asset: 8 per tile on average, 124 per tile it touches),
//               so they switch at 4.  Box limit 64 pixels: measured against 96 / 128 on the dancer (74 / 81 / 89 us), C3
//               (38.6 / 36.8 / 37.1), C4 (112.9 / 112.4 / 112.4) and C5 (202 / 206 / 211).
//  teams        two teams per tile + per-XCD bins when a mesh scope is dense enough for the triangle-parallel variant yet
//               averages under 16 triangles per tile: then its triangles sit in a small part of the frame (the dancer: 919 in
//               the fullest tile), the chip is far from full, the raster kernel lasts as long as the fullest tile's serial
//               chain -- which two teams cut (dancer raster 62.6 -> 44.0 us; four teams: 47.4) -- and the geometry kernel as
//               long as the queue of atomics on the hottest bin counter, which per-XCD counters cut (see reserve_bin_slots).
//  MIRHI_TP_MAX_AREA (0 = off), MIRHI_TP_DENSITY, MIRHI_RASTER_TEAMS (1 / 2) override for A/B measurements.
struct RasterMode { uint32_t tp_max_area, teams; bool wide_eligible; bool xcd_bins; uint32_t wide, xcd_swizzle; };
// tris: the segment's own triangles; spread / wide: what the command buffer's feedback asks for (Workspace::spread; Workspace::wide: 0 / 8 / 16 waves per tile)
// tiles: the tiles the scope launches (RenderArea::tiles); partial_area: not all of the attachment's
inline RasterMode raster_mode(const ScopeClass& c, size_t tiles, size_t tris, bool spread, uint32_t wide, const PlanKnobs& knobs, bool partial_area = false) {
    RasterMode m{0u, 1u, false, false, 0u, 1u};
    const size_t avg = tiles ? tris / tiles : 0;
    const size_t density = knobs.tp_density.set ? (size_t)knobs.tp_density.value : (c.tri_prog ? 16 : 4);
    const bool dense = tiles && avg >= density;
    m.tp_max_area = knobs.tp_max_area.set ? (uint32_t)knobs.tp_max_area.value : (dense ? 64u : 0u);
    if (c.key.pred) m.tp_max_area = 0;      // predicate scopes resolve pixel-parallel only (the LDS key array holds ordered keys)
    else if (c.masked_plain && m.tp_max_area == 0u) m.tp_max_area = 1u;    // alpha-masked scope: its records need the triangle-parallel path (LDS key array)
    const bool mesh_only = !c.tri_prog && c.has_draws && !c.own_family;      // (their variants: one team of four waves)
    m.teams = knobs.raster_teams.set ? (uint32_t)knobs.raster_teams.value : (avg < 16 ? 2u : 1u);
    if (!(m.tp_max_area && mesh_only && !c.ordered) || m.teams != 2u) m.teams = 1u;
    if (spread && !knobs.raster_teams.set) m.teams = 1u;      // measured on an earlier submission of this command buffer (Workspace::spread)
    // per-XCD bins go with the concentrated-mesh mode (the geometry kernel's counter contention), whichever raster variant then reads them
    m.xcd_bins = m.teams == 2u && !(knobs.xcd_bins.set && knobs.xcd_bins.value == 0);
    // The wide variants (eight / sixteen waves per tile, raster_body WPT) take over from both the plain and the two-team variant once the
    // busy-tile count says the mesh sits in few tiles.  MIRHI_RASTER_WIDE = 0 / 8 / 16 forces it (tests, A/B runs); a forced
    // MIRHI_RASTER_TEAMS = 2 keeps the two teams.
    m.wide_eligible = m.tp_max_area && mesh_only && !c.ordered && !c.masked_plain && !c.key.pred &&
                      !(knobs.raster_teams.set && knobs.raster_teams.value == 2 && !knobs.raster_wide.set);
    if (m.wide_eligible) {
        const uint32_t forced = knobs.raster_wide.set ? (uint32_t)knobs.raster_wide.value : 0xFFFFFFFFu;
        m.wide = forced == 0xFFFFFFFFu ? wide : (forced == 0u ? 0u : (forced == 8u ? 8u : 16u));
        // (teams stays what the scope gets when a submit decides against the wide variant: see allow_wide, mirhi_submit.h)
    }
    m.xcd_swizzle = knobs.xcd_run.set ? (uint32_t)knobs.xcd_run.value : 1u;
    if (c.own_family) { m.xcd_swizzle = 1u; m.wide = 0u; }      // (their own variants: plain tile order, four waves per tile)
    // A partial render area: the run-length order numbers the tiles of whole rows (a measurement knob, left to full-extent scopes), and the AREA raster
    // variants exist for one team of four waves with single-list bins (an area is a part of a frame: the two-team and wide variants answer a mesh that
    // sits in a small part of a whole frame's tiles, which launching the area's tiles alone already does)
    if (partial_area) { m.xcd_swizzle = 1u; m.teams = 1u; m.xcd_bins = false; m.wide = 0u; m.wide_eligible = false; }
    if (c.sky || c.transfer) { m.tp_max_area = 0u; m.teams = 1u; m.wide_eligible = false; m.xcd_bins = false; }
    // a 4x multisampled scope (raster_kernel_msaa): pixel-parallel only -- its four keys per pixel live in LDS where the triangle-parallel path keeps its one
    if (c.samples == 4u) { m.tp_max_area = 0u; m.teams = 1u; m.wide_eligible = false; m.xcd_bins = false; m.wide = 0u; m.xcd_swizzle = 1u; }
    return m;
}

// Writes what class and mode decide into a scope's parameters: everything raster_variant reads.  ordered_recs: the workspace's record array (used by ordered scopes only)
inline void set_raster_choice(PassParams& P, const ScopeClass& c, const RasterMode& m, const DepthState& s, TriRec* ordered_recs, uint32_t first_tri, uint32_t total_tris) {
    P.clear_depth_bits = c.key.clear_depth_bits; P.pred = c.key.pred; P.zflip = c.key.zflip; P.zmask = c.key.zmask;
    P.idflip = c.key.idflip; P.strict = c.key.strict; P.init_zk = c.key.init_zk; P.init_idk = c.key.init_idk;
    if (c.ordered) {
        P.ordered_recs = ordered_recs; P.ordered_first = first_tri; P.ordered_count = total_tris - first_tri;
        P.ord_depth_test = s.test; P.ord_depth_write = s.write; P.ord_depth_op = s.compare;
        memcpy(P.blend, s.blend, sizeof P.blend);
        P.idflip = 0; P.pred = 0;               // records carry the plain primitive id; the kernel applies the depth state itself
    }
    P.tp_max_area = m.tp_max_area;
    P.alpha_scope = c.masked_plain ? 1u : 0u;
    P.raster_teams = m.teams;
    P.raster_wide = m.wide;          // waves per tile of the wide variants: 0 (four waves), 8 or 16
    P.xcd_swizzle = m.xcd_swizzle;
    P.shadowed = c.shadowed;
    P.ibl = c.ibl;
    P.sky = c.sky ? 1u : 0u;
    P.samples = c.samples == 4u ? 4u : 0u;
}

// Bins and page pool of one scope.  tris: the segment's own triangles, total_tris: with those of the scope's earlier segments (primitive ids continue)
struct BinGeometry { uint32_t bin_cap, sub_cap, fixed_per_tile, fixed_pages; size_t pages; uint32_t big_cap; };
// index_tiles (0: = tiles): the tiles the bins are indexed by, where that is more than the scope launches (RenderArea::index_tiles: a tile's fixed pages
// sit at page = tile * fixed_per_tile, and a partial render area keeps the attachment's columns in the index); densities are judged by `tiles`
inline BinGeometry bin_geometry(size_t tiles, size_t tris, uint32_t total_tris, bool xcd_bins, uint32_t pool_scale, const PlanKnobs& knobs, size_t index_tiles = 0) {
    BinGeometry g;
    if (index_tiles == 0) index_tiles = tiles;
    // A tile's bin holds up to BIN_TABLE_ROW pages (4096 records; eight lists of 512 with per-XCD bins) before it spills into
    // the big list, which EVERY tile walks -- the limit costs nothing until it is used: pages come out of one pool, sized by
    // the scope's triangle count, not by tiles x capacity (round 1: 100 MB at 1080p, 400-510 MB at 4K per command buffer).
    // MIRHI_BIN_CAP (records per list, A/B runs and the spill tests) lowers it.
    uint32_t cap = (uint32_t)BIN_TABLE_ROW * BIN_PAGE_RECS;
    if (knobs.bin_cap.set) cap = std::min<uint32_t>(cap, std::max<uint32_t>(8u * BIN_PAGE_RECS, ((uint32_t)knobs.bin_cap.value + 511u) & ~511u));
    g.bin_cap = cap; g.sub_cap = xcd_bins ? cap / 8u : cap;
    // Pool: the first page of every single-list bin has a fixed place (page = tile); the dynamic part is sized for the
    // (triangle, tile) pairs the scope is likely to produce -- 8 per triangle for small scopes (scattered 50-pixel triangles
    // make 5), towards 1.5 for big meshes (1.2 measured on the 1M-triangle grid) -- plus one partly filled page per list.  A scope
    // that needs more spills into the big list (correct, slower) and the pool is doubled for the next submit.
    size_t pairs = std::max(std::max(std::min<size_t>(8 * tris, 262144), std::min<size_t>(3 * tris, 786432)), 3 * tris / 2);
    if (pairs > 16 * tris) pairs = 16 * tris;                        // (a binned triangle spans at most 4 x 4 tiles)
    // fixed pages per tile: what the average density fills (x 1.3 for triangles that straddle tiles), at least one, at most eight --
    // a uniform mesh (the 1M-triangle grid: 123 per tile) then bins without a single allocation, a concentrated one (the
    // dancer asset) opens pages where its triangles are
    g.fixed_per_tile = xcd_bins ? 0u : (uint32_t)std::min<size_t>(8, std::max<size_t>(1, tiles ? (13 * tris / (10 * tiles) + BIN_PAGE_RECS - 1) / BIN_PAGE_RECS : 1));
    if (knobs.fixed_pages.set && !xcd_bins) g.fixed_per_tile = (uint32_t)std::min(8, std::max(1, knobs.fixed_pages.value));   // (tests, A/B runs)
    g.fixed_pages = g.fixed_per_tile * (uint32_t)index_tiles;
    // dynamic part: the estimated pairs that the fixed pages will not take (they take at most half of it when the triangles sit
    // in a part of the frame), never less than a quarter of the estimate, plus a partly filled page for one tile in four
    const size_t fixed_capacity = (size_t)g.fixed_per_tile * tiles * BIN_PAGE_RECS;      // (of the launched tiles: the others' pages take nothing)
    const size_t dyn_records = std::max(pairs > fixed_capacity / 2 ? pairs - fixed_capacity / 2 : 0, pairs / 4) * pool_scale;
    g.pages = g.fixed_pages + ((dyn_records / BIN_PAGE_RECS + tiles * (xcd_bins ? 8 : 1) / 4 + 64 + 7) & ~(size_t)7);
    if (knobs.pool_pages.set) g.pages = g.fixed_pages + 8 * (((size_t)knobs.pool_pages.value + 7) / 8);      // (pool-exhaustion test)
    g.big_cap = total_tris + total_tris / 4 + 1024;
    return g;
}

// ---- multiview depth scopes (mirhi_cmd_begin_rendering_multiview): what is refused, in what words, and the per-view plan ----
// What begin_rendering_multiview looks at, as numbers (images and buffers: 0 = NULL; formats mirhi_format; ops mirhi_load_op / mirhi_store_op)
struct MultiviewFacts {
    uint32_t has_color, has_prim, has_depth, depth_is_array, depth_samples, depth_format, layers;
    int32_t depth_load_op, depth_store_op;
    uint32_t view_mask, has_constants, view_stride;
    uint64_t view_offset, constants_bytes;      // constants_bytes: the buffer's size
    uint32_t area_partial, split_device, fragment_stats;
};
inline uint32_t multiview_count(uint32_t mask) { return (uint32_t)__builtin_popcount(mask); }
// nullptr: the scope is accepted
inline const char* multiview_scope_refusal(const MultiviewFacts& f) {
    if (f.has_color || f.has_prim) return "unsupported: a multiview scope is depth-only (color_image and prim_id_image NULL)";
    if (f.has_depth && f.depth_samples != 1u) return "unsupported: a multisampled depth image in a multiview scope";
    if (!f.has_depth || !f.depth_is_array) return "unsupported: a multiview scope renders into an image array (mirhi_image_create_array), not a 2-D image or a layer view";
    if (f.depth_format != MIRHI_FORMAT_D32_SFLOAT) return "unsupported: a multiview depth array that is not D32_SFLOAT";
    if (f.depth_load_op != MIRHI_LOAD_OP_CLEAR && f.depth_load_op != MIRHI_LOAD_OP_LOAD) return "unsupported: the depth load op of a multiview scope is CLEAR or LOAD";
    if (f.depth_store_op != MIRHI_STORE_OP_STORE) return "unsupported: a multiview scope must store its depth (STORE)";
    if (f.view_mask == 0u) return "unsupported: an empty view mask";
    if (multiview_count(f.view_mask) > (uint32_t)MAX_BATCH) return "unsupported: more than 8 views in one multiview scope";
    if (f.layers < 32u && (f.view_mask >> f.layers) != 0u) return "unsupported: a view mask bit at or above the array's layer count";
    if (!f.has_constants) return "unsupported: a multiview scope without view_constants";
    if (f.view_stride < 64u || f.view_stride % 16u != 0u) return "unsupported: view_stride must be at least 64 and a multiple of 16";
    if (f.view_offset % 16u != 0u) return "unsupported: view_offset must be a multiple of 16";
    {
        const uint32_t top = 31u - (uint32_t)__builtin_clz(f.view_mask);
        if (f.view_offset > f.constants_bytes || (uint64_t)top * f.view_stride + 64u > f.constants_bytes - f.view_offset)
            return "unsupported: the view_constants buffer is too short for the highest view's matrix";
    }
    if (f.area_partial) return "unsupported: a partial render area in a multiview scope";
    if (f.split_device) return "unsupported: a multiview scope on a split device";
    if (f.fragment_stats) return "unsupported: fragment statistics of a multiview scope";
    return nullptr;
}
// the program of a draw recorded in a multiview scope (mirhi_program); nullptr: accepted
inline const char* multiview_program_refusal(int32_t program) {
    return program == MIRHI_PROGRAM_SHADOW ? nullptr : "unsupported: only SHADOW draws may be recorded in a multiview scope";
}
// View slot j of a scope (the j-th set bit of the mask, lowest first): its view index, where its layer starts in the array (bytes from the array's base)
// and where its matrix sits in the view constants (bytes from the buffer's base).  Returns the number of slots.
struct MultiviewSlot { uint32_t view; uint64_t layer_offset, matrix_offset; };
inline uint32_t multiview_slots(uint32_t mask, uint32_t width, uint32_t height, uint64_t view_offset, uint32_t view_stride, MultiviewSlot out[MAX_BATCH]) {
    uint32_t n = 0;
    for (uint32_t v = 0; v < 32u && n < (uint32_t)MAX_BATCH; v++)
        if ((mask >> v) & 1u) out[n++] = MultiviewSlot{v, (uint64_t)v * width * height * 4u, view_offset + (uint64_t)v * view_stride};
    return n;
}

}  // namespace mirhi
