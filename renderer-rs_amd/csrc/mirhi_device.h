// mirhi_device.h -- structures shared by the host C-ABI layer and the gfx950 kernels.
//
// Data layout in HBM (see DESIGN.md "Data layout"):
//   DrawDesc[]   one per recorded draw of a rendering scope (pointers into caller buffers + state)
//   BinRec[]     the bin pool: pages of 64 tile-relative triangle records of 32 B.  A tile's bin is a list of pages -- the
//                first one at a fixed place (page = tile), further ones taken from the pool by the geometry kernel and
//                entered in the tile's row of the page table -- written by the geometry kernel, consumed by exactly one
//                raster workgroup
//   BigRec[]     screen-space triangles (48 B, absolute coordinates) too large for the bins, clipped, cut by a scissor, or
//                spilled from a full bin / an exhausted pool; every raster workgroup scans this list
//   counters     bin_count[tiles], pool_next, big_count, status words
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mirhi {

constexpr int TILE = 32;              // screen tile edge in pixels (one raster workgroup)
constexpr int TILE_LOG2 = 5;
constexpr int BLOCK = 8;              // coverage block edge (one wave-iteration covers 8x8 px)
constexpr int RASTER_THREADS = 256;   // 4 waves; wave q owns the 16x16 quadrant q, 4 px per lane
constexpr int RASTER_CHUNK = 192;     // triangle records staged per LDS pass (12 KB)
constexpr int TP_MIN_LANES = 32;      // small records a wave must hold before it resolves them triangle-parallel
constexpr int GEOM_THREADS = 64;
constexpr int MAX_BIN_SPAN = 4;       // triangles spanning more than 4x4 tiles go to the big list
constexpr float GUARD_PX = 16000.0f;  // guard band: snapped coordinates stay inside +-2^22 sub-pixels
constexpr int BIN_PAGE_RECS = 64;     // records per bin page (2 KB)
constexpr int BIN_PAGE_LOG2 = 6;
constexpr int BIN_TABLE_ROW = 64;     // page-table entries per tile: 64 pages of one list, or 8 pages for each of 8 per-XCD lists
constexpr int POOL_COUNTER_STRIDE = 32;        // words between the per-XCD pool counters (128 B)
// Words between two bin counters (64 B): one counter per cache line sector.  Packed 32 to a 128-byte line (rounds 1-3) the counters of a whole row segment of
// tiles queued their atomics on ONE line -- a scattered scope (C2: 50k reservations on 2,040 counters, every wave all over the frame) puts ~800 of them on each
// line, one after the other: tools/microbench/atomic_pad.hip, the reservation pattern of a C2 geometry wave: 5.7 us from its first atomic to its last result
// with packed counters, 1.7 us with one counter per 64 bytes (128 bytes: the same), kernel 8.2 -> 4.0 us.  Counter c lives at bin_count[c * BIN_COUNT_STRIDE].
constexpr uint32_t BIN_COUNT_STRIDE = 16;
constexpr uint32_t PAGE_EMPTY = 0xFFFFFFFFu;   // table entry not (yet) published
constexpr uint32_t PAGE_NONE = 0xFFFFFFFEu;    // the pool was exhausted when this page was asked for: its records go to the big list
constexpr uint32_t NO_PRIM = 0xFFFFFFFFu;
constexpr uint32_t MAX_PRIM_ID = 0xFFFFFFFDu;

enum : uint32_t { STATUS_BIG_OVERFLOW = 1u, STATUS_ALPHA_TEST_TEXTURED = 2u,
                  STATUS_POOL_EXHAUSTED = 4u,      // not an error: records went to the big list instead; the host grows the pool
                  STATUS_PAGE_TIMEOUT = 8u };      // a page was never published (cannot happen by construction; bounded wait)
constexpr uint32_t ORDERED_MARKER = 0xFFFFFFFFu;   // bbox-y word of an ordered slot whose triangle was clipped: pieces live in the big list
constexpr int ORDERED_THREADS = 256;

struct DrawDesc {
    const uint8_t* vb;            // binding 0 base + bind offset
    const uint8_t* ib;            // index base + bind offset (nullptr for draw)
    const float*   camera;        // b0 CameraData
    const float*   object;        // b1 ObjectData
    const uint8_t* lights;        // b2 LightUBO
    const uint8_t* material;      // b3 MaterialData
    const uint8_t* point_lights;  // t0 space1
    const uint8_t* spot_lights;   // t1 space1
    const uint8_t* tex[5];        // t0 albedo, t1 normal, t2 metallic-roughness, t3 occlusion, t4 emissive (RGBA8)
    uint32_t tex_w[5], tex_h[5];
    uint32_t tex_levels[5];       // mip levels stored behind level 0 (1 = no chain: bilinear)
    uint32_t tex_srgb;            // bit t: texture t is R8G8B8A8_SRGB (RGB decoded to linear when sampled)
    // Depth bias and depth clamp of the draw's pipeline (read by setup_triangle and the outcode step, nowhere else): bit 0
    // (DEPTH_FLAG_BIAS): add the bias to the depth plane, bit 1 (DEPTH_FLAG_CLAMP): no near / far clipping.  The word sits HERE, in the 64-byte line of
    // stride / first / tri_count (0x80-0xbf), which every geometry wave reads first whatever its scope: in a line no wave had touched its scalar load
    // was a cache miss on every wave's dependent chain, 0.08 us of the headline workload's geometry kernel (DESIGN_NOTES.md).  tex_any_mips, which
    // only the fragment programs read, moved to the pad word beside the shadow words in exchange.
    uint32_t depth_flags;
    uint32_t stride;
    uint32_t index_type;          // 0 none, 2 u16, 4 u32
    uint32_t first;               // first_vertex / first_index
    int32_t  vertex_offset;
    uint32_t tri_count;
    uint32_t prim_base;           // global primitive id of triangle 0
    uint32_t slot_base;           // first geometry-kernel lane of this draw (draws are padded to whole waves)
    uint32_t program;
    uint32_t cull_mode, front_face;
    float    hw, hh, cx, cy;      // viewport half extents and centre
    float    dscale, dmin;        // depth range
    float    gx, gy;              // guard-band plane factors
    int32_t  sx0, sy0, sx1, sy1;  // inclusive scissor (already clamped to render area and extent)
    uint32_t scissor_partial;     // scissor smaller than the target: per-pixel box test needed when it cuts a bbox
    uint32_t vs_words;            // 16-byte words per shaded vertex (3 MODEL, 5 MODEL_FULL, 0 = no vertex pre-pass)
    uint32_t tex_aniso;           // bits 4t..4t+3: max_anisotropy - 1 of texture t (0 = trilinear; set only for textures with a chain whose sampler
                                  // minifies LINEAR / MIP_LINEAR); bits 20+2t..21+2t: mirhi_mip_mode of texture t's sampler (0 = MIP_LINEAR)
    const void* vs_attr;          // shaded vertices, the other words (vs_words - 1 per vertex): see VsJob
    const void* vs_out;           // shaded vertices, clip positions (16 B per vertex), indexed like the vertex buffer: see VsJob
    const float*   shadow_map;    // MODEL_PBR with MIRHI_TEXTURE_SHADOW_MAP bound: the D32 map (t7), else nullptr (shadow = 1)
    const uint8_t* shadow_data;   // ShadowParams (96 B, shadow.hlsli:20-30) when shadow_map is set
    uint32_t shadow_w, shadow_h;  // the map's extent (with cascades: one layer's)
    uint32_t shadow_layers;       // 0: a single map (CalculateShadow); 4: mirhi_cmd_bind_shadow_cascades -- shadow_map is the base of a D32 array of
                                  // that many tightly packed layers, shadow_data its CSMParams (336 B, shadow_csm.hlsli:23-39): CalculateShadowCSM
    uint32_t tex_any_mips;        // some bound texture has a chain: the fragment program evaluates UV derivatives
    float    bias_constant, bias_clamp, bias_slope;      // mirhi_depth_bias; read under DEPTH_FLAG_BIAS only
    // Sampler state of the five textures (mirhi_image_set_sampler), read by the fragment programs alone and so kept out of the 0x80-0xbf
    // line: bits 6t..6t+5 of texture t = address_u | address_v << 2 | mag_filter << 4 | min_filter << 5 (mirhi_address_mode, mirhi_sampler_filter: LINEAR = 0 -- not the blit's mirhi_filter).  With the mip
    // mode in tex_aniso that is eight bits per texture; all zero = REPEAT / LINEAR / MIP_LINEAR, the sampler of every draw before the state existed.
    uint32_t tex_sampler;
    // blendThreshold of CalculateShadowCSMBlended (mirhi_cmd_bind_shadow_cascades_blended), latched with the cascade binding; 0: the draw's
    // shadow term is CalculateShadowCSM.  Read by the blended fragment programs alone: a line of its own behind everything else, far from 0x80-0xbf.
    float    csm_blend;
    uint32_t csm_pad[3];
};
constexpr uint32_t DEPTH_FLAG_BIAS = 1u, DEPTH_FLAG_CLAMP = 2u;
constexpr uint32_t TEX_MIP_MODE_SHIFT = 20u;     // DrawDesc::tex_aniso: where the mip modes start
// some texture of the draw has a sampler other than REPEAT / LINEAR / MIP_LINEAR: the draw belongs to the full-featured program class (classify_scope)
inline bool draw_has_sampler_state(const DrawDesc& d) { return d.tex_sampler != 0u || (d.tex_aniso >> TEX_MIP_MODE_SHIFT) != 0u; }
// ... and its texture 0 has: the one texture the masked raster variants' alpha test reads (pbr_base_alpha, under the default sampler only)
inline bool draw_has_base_sampler_state(const DrawDesc& d) { return (d.tex_sampler & 63u) != 0u || ((d.tex_aniso >> TEX_MIP_MODE_SHIFT) & 3u) != 0u; }
static_assert(sizeof(DrawDesc) % 16 == 0, "DrawDesc must stay 16-byte sized");

// Vertex-shader pre-pass (vertex/model.hlsl:39-68 run once per vertex, as a GPU's vertex stage does, instead of three
// times per shaded pixel): one job per distinct (vertex buffer range, camera, object, program class) of a scope.
// Shaded vertex = vs_words 16-byte words in TWO streams: the clip position on its own (what the geometry kernel gathers for every
// triangle of every rank: 16 B per vertex, not a 48 / 80-byte row -- C4: 8 MB instead of 24 MB per frame and rank), the rest behind it
//   clip[v]  = clip position
//   attr[v]  = { world.xyz, N.x }, { N.y, N.z, u, v }                     (vs_words - 1 = 2 words, MODEL)
//              + { T.xyz, B.x }, { B.y, B.z, 0, 0 }                       (vs_words - 1 = 4 words, MODEL_FULL / MODEL_PBR)
//              nothing                                                    (vs_words = 1, SHADOW: camera = ShadowConstants, object = its model @64)
// A job's output is [count x 16 B clip, rounded up to 256 B][count x (words - 1) x 16 B]: vs_attr_of() below.
struct VsJob {
    const uint8_t* vb;
    const float*   camera;
    const float*   object;
    void*          out;
    uint32_t stride, count, slot_base, words;
};
static_assert(sizeof(VsJob) == 48, "VsJob is 48 bytes");
// the attribute stream of a job's output block `out` for `count` vertices (host and device agree through this one function)
#if defined(__HIPCC__) || defined(__CUDACC__)
__host__ __device__
#endif
inline size_t vs_attr_offset(uint32_t count) { return ((size_t)count * 16u + 255u) & ~(size_t)255u; }

// Screen-space triangle record, 12 dwords = three 16-byte words.  Written once per overlapped tile into
// that tile's bin (and once into the big list for triangles that span more than 4x4 tiles, were clipped,
// or found a bin full); the raster kernel turns it into a tile-relative record in LDS.
//   w0 = { X0, Y0, X1, Y1 }    snapped vertices, 1/256 px, orientation normalised (interior has E > 0)
//   w1 = { X2, Y2, z0, zx }    depth of vertex 0 and depth plane d/dx
//   w2 = { zy, idk, bx, by }   d/dy, primitive id in tie-break order,
//                              bx = minx | maxx << 16 | boxed << 31, by = miny | maxy << 16 (inclusive pixel box)
struct TriRec { uint32_t w[12]; };
static_assert(sizeof(TriRec) == 48, "TriRec is 48 bytes");
typedef TriRec BigRec;    // the big list holds TriRecs

// Bin record, 8 dwords = two 16-byte words: the same triangle relative to the tile whose bin it sits in.  Only triangles whose
// pixel box spans at most 4 x 4 tiles and whose vertices lie within 65535 sub-pixels of each other are binned, so every
// coordinate is a 16-bit number; the pixel box is recomputed from the vertices (a box cut by a scissor goes to the big list).
//   w0 = { ox | oy << 16,      smallest vertex x / y minus the tile origin, 1/256 px, signed 16 bit
//          x0 | y0 << 16, x1 | y1 << 16, x2 | y2 << 16 }   vertices minus (smallest x, smallest y), unsigned 16 bit
//   w1 = { z0, zx, zy, idk }   as in TriRec
struct BinRec { uint32_t w[8]; };
static_assert(sizeof(BinRec) == 32, "BinRec is 32 bytes");

// One region of a recorded transfer command, resolved at record time (mirhi_api.hip record_transfer).  `first`: the region's first work unit of the
// launch -- the units of all regions are numbered through, a workgroup finds its region by these.
//   copy  a rectangle of `rows` rows of `row_bytes` bytes from src (pitch src_pitch) to dst (pitch dst_pitch); unit = 16, 4 or 1: the widest access
//         every row's source and destination are co-aligned for; a work unit is 256 such accesses of one row (`chunks` per row)
//   fill  row_bytes bytes at dst (4-byte texels or float4 ones; a work unit is 256 16-byte stores)
//   blit  src / dst are the bases of the two levels, src_w x src_h and dst_w their extents in texels; the destination rectangle [dx0, dx1) x [dy0, dy1)
//         is cut into 32 x 32 tiles aligned to the level's origin (tiles_x per row of tiles; a work unit is a tile).  Column i samples the source at
//         u = sx0 + (xn0 + xns (i - dx0)) / xd (xd > 0; integers: the texel index of NEAREST and LINEAR is exact, a LINEAR weight is rounded once),
//         which is include/mirhi.h's u (NEAREST) or u - 1/2 (LINEAR); rows likewise.
struct XferRegion {
    const uint8_t* src; uint8_t* dst;
    uint64_t src_pitch, dst_pitch, row_bytes;
    uint32_t rows, unit, chunks, first;
    uint32_t src_w, src_h, dst_w, tiles_x;
    int32_t  dx0, dy0, dx1, dy1;
    int32_t  sx0, xn0, xns, xd;
    int32_t  sy0, yn0, yns, yd;
};
static_assert(sizeof(XferRegion) == 120, "XferRegion is 120 bytes");
enum : uint32_t { XFER_NONE = 0u, XFER_COPY = 1u, XFER_BLIT_NEAREST = 2u, XFER_BLIT_LINEAR = 3u, XFER_FILL = 4u };
constexpr uint32_t XFER_MAX_REGIONS = 16u;
constexpr uint32_t XFER_MAX_GROUPS = 2048u;      // workgroups of a copy or fill launch (grid-strided beyond)

struct PassParams {
    uint32_t width, height;           // colour target extent
    uint32_t tiles_x, tiles_y;
    // Tile rows rasterized on this device (tile-row split): rows tile_row_begin + k * tile_row_step, k = 0 .. tile_row_end - tile_row_begin - 1.
    // One contiguous band per rank: step 1 (begin / end are then the band itself); interleaved rows (rank r owns rows r, r + world, ...): begin = r,
    // step = world, end - begin = the number of rows owned.  Bins, counters and the raster grid are indexed by k ("owned row"), not by the row itself.
    uint32_t tile_row_begin, tile_row_end, tile_row_step;
    uint32_t num_draws, total_tris;
    uint32_t total_slots;             // geometry-kernel lanes (every draw padded to a multiple of 64)
    const DrawDesc* draws;
    const VsJob* vs_jobs; uint32_t num_vs_jobs, vs_total_slots;
    // depth key (DESIGN.md "Depth key"): zk = (bits(z) ^ zflip) & zmask ; idk = idflip ? MAX-id : id
    uint32_t zflip, zmask, idflip;
    uint32_t strict;                  // compare op is LESS / GREATER (ties with the stored depth fail)
    uint32_t pred;                    // != 0: predicate mode -- bit 0/1/2: a fragment passes when its depth is </==/> the scope's
                                      // initial depth; bit 3: the winner's depth replaces it (ALWAYS with depth write)
    uint32_t init_zk, init_idk;       // state of an uncovered pixel when depth is cleared
    uint32_t clear_depth_bits;
    float    clear_color[4];
    uint32_t clear_packed;            // clear colour in the target's B8G8R8A8_SRGB encoding (host-computed)
    uint32_t color_load;              // 1 = keep existing colour where nothing is drawn
    uint32_t color_format;            // mirhi_format
    void*    color;
    float*   depth;                   // optional D32 image (load and/or store)
    uint32_t depth_load, depth_store;
    uint32_t* prim_out;               // optional R32_UINT image
    // workspace
    BinRec*   bin_pool; uint32_t* bin_count; uint32_t bin_cap;     // bin_cap: records a tile's bin can hold (all of its lists)
    uint32_t* bin_table;              // [tiles][BIN_TABLE_ROW] pool page of the list's p-th page (PAGE_EMPTY until published)
    uint32_t* pool_next;              // [8][POOL_COUNTER_STRIDE] dynamic pages handed out in this scope by the waves of each XCD (re-armed by
                                      // the raster kernel): one counter per XCD, a cache line apart -- a single counter that every XCD adds
                                      // to ping-pongs between their L2s (C4: geometry 57 -> 132 us)
    uint32_t  pool_dyn_base, pool_dyn_pages;   // XCD x hands out pool pages [pool_dyn_base + x * pool_dyn_pages, ... + pool_dyn_pages)
    uint32_t  fixed_recs;             // slots [0, fixed_recs) of a tile's single list live in the tile's own fixed pages (page = tile *
                                      // fixed_recs / 64 + slot / 64): 64 x the pages the scope's average triangle density fills, 0 with per-XCD lists
    BigRec*   big_recs; uint32_t* big_count; uint32_t big_cap;
    uint32_t* big_count_next;         // the other parity's counter: zeroed by this scope for the next one
    uint32_t* prim_draw;              // per primitive of the scope (index prim - first_prim): its draw, written by the geometry kernel when
    uint32_t  first_prim;             // the scope has several draws -- one load in the resolve instead of a binary search per pixel
    uint32_t* flat_color;             // per primitive: B8G8R8A8_SRGB colour if its three vertex colours are equal (TRIANGLE
                                      // program, sRGB8 target), else 0; lets the resolve skip interpolation + OETF
    uint32_t tp_max_area;             // records whose pixel box inside the tile has at most this many pixels are resolved
                                      // triangle-parallel (LDS ds_min) instead of pixel-parallel
    uint32_t xcd_swizzle;             // run length G of consecutive tiles placed on one XCD (1 = plain order)
    uint32_t raster_teams;            // 2: the mesh variant with two teams of four waves per tile (host-side choice, see raster_kernel)
    // Per-XCD bins (only together with raster_teams == 2): a tile's bin is eight lists of sub_cap records, one per XCD,
    // each with its own counter (bin_count[xcd * count_stride + tile]) and its own eight entries of the tile's page-table row,
    // so that a hot tile's counter line stays in one XCD's L2 -- see reserve_bin_slots.  Off: count_stride = 0, sub_cap =
    // bin_cap, and the first page of every tile's single list has a fixed place in the pool (page = tile): the common bin
    // needs neither an allocation nor a table entry.
    uint32_t sub_cap, count_stride;
    uint32_t raster_wide;             // 1: the wide mesh variant, sixteen waves per tile (host-side choice from the busy-tile count, see raster_body)
    uint32_t resolve_flat_only;       // 1: a wave whose covered pixels all carry a packed flat colour may store and leave (flat colours exist, depth was not loaded,
                                      // the target is 8-bit, no primitive-id image, no depth store) -- the four conditions as one host-computed word: one scalar load
                                      // in the resolve instead of four dependent ones
    // Busy-tile count (feedback for that choice): every raster workgroup whose tile holds something adds 1 to active[(tile & 7) * 32] (eight
    // counters, one per XCD residue, a cache line apart); the workgroup of tile 0 reports the sum of the PREVIOUS scope's counters
    // (active_prev: the other parity, complete by then) in status[3] and re-arms them.
    uint32_t* active; uint32_t* active_prev;
    // ordered segments (blending; any depth state whose result depends on the order of all fragments): the geometry kernel
    // writes triangle t of the segment to ordered_recs[t] instead of binning it, the ordered kernel walks that array
    TriRec*  ordered_recs; uint32_t ordered_first, ordered_count;
    uint32_t ord_depth_test, ord_depth_write, ord_depth_op;
    uint32_t blend[8];                // enable, src colour, dst colour, colour op, src alpha, dst alpha, alpha op, write mask
    uint32_t alpha_scope;             // 1: a plain (bins + depth key) scope whose pipelines set fragment_discard_enable: records of draws whose texel
                                      // alpha straddles the material's cutoff are resolved triangle-parallel with the alpha test per pixel (raster_small_masked)
    uint32_t* status;                 // pinned host memory: [0] status bits (atomicOr), [1] big-list length, [2] dynamic pages of the last scope,
                                      // [3] busy tiles of the scope before it | 0x80000000
    unsigned long long* frag_stats;   // device counters of the statistics pass (never touched by geometry / raster kernels): [0] pixels that
                                      // ran a fragment program (winners of the depth resolve), [1] fragments covered before the depth test
    uint32_t depth_only;              // 1: a depth-only scope (SHADOW draws; color == nullptr): raster_kernel_depth stores the depth image and nothing else
    uint32_t shadowed;                // 1: some MODEL_PBR draw of the scope samples a shadow map (raster_kernel_shadow); 2: a cascade array (raster_kernel_csm); 3: ... and some cascaded draw blends (raster_kernel_csm_blend)
    // The IBL set of a scope with MODEL_PBR_IBL draws (mirhi_cmd_bind_ibl: set 3 of pixel/model_pbr_ibl.hlsl; one set per scope; raster_kernel_ibl alone
    // reads these words): base of the irradiance cube (level 0 is sampled), of the prefiltered cube's chain and of the square BRDF LUT -- float4
    // texels in the layouts of include/mirhi.h "IBL precompute" -- with their edge lengths and the prefiltered chain's level count.  0 / nullptr otherwise.
    uint32_t ibl;                     // 1: some draw of the scope is MODEL_PBR_IBL
    uint32_t ibl_irr_size, ibl_pre_size, ibl_pre_levels, ibl_lut_size, ibl_pad;
    const float* ibl_irradiance; const float* ibl_prefiltered; const float* ibl_lut;
    // A SKYBOX segment (vertex/skybox.hlsl + pixel/skybox.hlsl: one draw, a segment of its own; sky_kernel alone reads these words).
    // The triangle is set up on the host: oriented integer edge functions with the top-left bias, E_i(px, py) = sky_e0[i] + 256 (sky_a[i] px +
    // sky_b[i] py) >= 0 for all i <=> pixel (px, py) is covered; LocalPos at a pixel centre = sky_pos0 + sky_posx (px + 1/2) + sky_posy (py + 1/2).
    uint32_t sky;                     // 1: the segment is a SKYBOX draw (no DrawDesc, no bins)
    uint32_t sky_visible;             // 0: culled, degenerate or cut away by an empty scissor: only the load / clear / store ops happen
    uint32_t sky_size, sky_levels;    // the environment cube's edge and level count (level 0 is sampled)
    const float* sky_env;             // its base (float4 texels, the layout of include/mirhi.h "IBL precompute")
    int32_t  sky_a[3], sky_b[3];
    int32_t  sky_scissor[4];          // inclusive x0, y0, x1, y1
    long long sky_e0[3];
    float    sky_pos0[3], sky_posx[3], sky_posy[3];
    uint32_t sky_depth_bits;          // the viewport's max_depth: the fragment's depth
    uint32_t sky_compare, sky_write;  // mirhi_compare_op (ALWAYS when the depth test is off), 1: passing fragments store sky_depth_bits
    uint32_t sky_prim;                // the draw's primitive id
    // A transfer command (include/mirhi.h "Transfer commands"; an entry of the recording of its own: no attachments, draws or bins; the kernels of
    // mirhi_transfer.hip.h alone read these words).  Its regions sit in the parameter block behind the draw descriptors.
    uint32_t xfer;                    // XFER_NONE, or what the entry is: XFER_COPY, XFER_BLIT_NEAREST, XFER_BLIT_LINEAR, XFER_FILL
    uint32_t xfer_count;              // regions (1 .. 16)
    uint32_t xfer_src_format, xfer_dst_format;      // mirhi_format of a blit's source / a blit's or clear's destination
    const XferRegion* xfer_regions;
    float    xfer_color[4];           // a clear's value (depth: [0])
    uint32_t xfer_groups, xfer_pad;   // work units of all regions together (XferRegion::first of a region behind the last)
    // The render area (mirhi_rendering_info::render_area): pixels [area_x0, area_x0 + area_w) x [area_y0, area_y0 + area_h) of the
    // attachments are the scope's -- loaded, cleared, resolved and stored; no kernel writes a pixel outside.  A full-extent scope: 0, 0, width, height,
    // and its raster kernels (the AREA = false instantiations of raster_body) never read these words: behind everything else, so that every word in
    // front of them sits where it sat before there were areas.
    uint32_t area_x0, area_y0, area_w, area_h;
    // The launch of a scope with a partial area: the tile grid stays the attachment's and every pixel coordinate absolute; the launch
    // spans tile columns [tile_col_begin, tile_col_begin + tile_cols) of the rows tile_row_begin .. tile_row_end (tile_cols == 0: all tiles_x columns --
    // parameters made without a plan).  Bins, counters and the page table keep tiles_x entries per owned row: a draw's scissor lies inside the area,
    // so the columns outside stay empty and unvisited.
    uint32_t tile_col_begin, tile_cols;
    uint32_t area_partial, area_pad;  // 1: the area is smaller than the attachment
    // A 4x multisampled scope (mirhi_cmd_begin_rendering_resolve; geometry_kernel_msaa and raster_kernel_msaa alone read the word): 4, else 0.
    // The attachments are transient: `color` is the colour RESOLVE target (1x), `depth` the depth resolve target (sample 0; depth_store = 1) or nullptr,
    // `prim_out` an image of 4 * width x height texels, texel (4 px + s, py) the winner of sample s.  Behind everything else, like the area words.
    uint32_t samples, samples_pad;
    // Seamless cube filtering (mirhi_image_set_cube_seamless), latched when the draw was recorded.  ibl_seamless: bit 0 the irradiance cube's
    // state, bit 1 the prefiltered cube's (raster_kernel_ibl_seamless alone reads it; != 0 selects that kernel); sky_seamless: 1 = the SKYBOX segment's
    // environment is seamless (selects sky_kernel_seamless; no kernel reads it).  Behind everything else, like the area words.
    uint32_t ibl_seamless, sky_seamless;
};
static_assert(sizeof(PassParams) % 8 == 0, "PassParams holds pointers");

// Kernel arguments passed by value next to the PassParams pointer: what a wave needs before anything else, so that its
// first dependent loads (draw table, bin counter -> bin records) hang off the kernarg load, not off a second memory hop.
struct GeometryHead {
    const DrawDesc* draws; uint32_t num_draws;
    uint32_t tris_per_wave;          // triangles a 64-lane workgroup takes: 64, or 32 / 16 for small scopes (the other lanes help with the pairs)
    // Scopes of ONE non-indexed draw of the TRIANGLE program (the reference's own frame, BASELINE configs[0] and [1]): where its vertices are, by value, so
    // that a wave's vertex loads hang off the kernarg load alone -- beside the descriptor's scalar loads instead of behind them (0.85 us of a wave's 9).
    // vb0 == nullptr: the descriptor says where (every other scope).
    const uint8_t* vb0; uint32_t stride0, first0, tris0;
};
struct RasterHead {
    uint32_t* bin_count; const BinRec* bin_pool; uint32_t* big_count;
    uint32_t tiles_x;
    uint32_t tile_origin;             // PassParams::tile_row_begin | PassParams::tile_col_begin << 16 (both below 2^9: one word, the head stays 56 bytes --
                                      // with the parameter pointer one 64-byte kernarg load): grid row k / column j is tile row (tile_origin & 0xFFFF) +
                                      // k * tile_row_step / tile column (tile_origin >> 16) + j; the column origin is 0 unless the render area is partial
    uint32_t bin_cap, big_cap;
    uint32_t sub_cap, count_stride;   // per-XCD bins (PassParams); read by the two-team variant only
    uint32_t fixed_recs;              // PassParams::fixed_recs
    uint32_t tile_row_step;           // PassParams::tile_row_step: grid row k is tile row tile_row_begin + k * tile_row_step
};
static_assert(sizeof(RasterHead) == 56, "RasterHead and the parameter pointer are one 64-byte kernarg load");
// tile columns a scope's raster launch spans
inline uint32_t launch_cols(const PassParams& P) { return P.tile_cols ? P.tile_cols : P.tiles_x; }

// A batched launch: the independent rendering scopes of one mirhi_queue_submit (equal target shape, equal raster variant) share
// one vertex, one geometry and one raster launch; their arguments travel by value in the kernarg segment.
constexpr int MAX_BATCH = 8;
struct GeometryBatch { const PassParams* params[MAX_BATCH]; GeometryHead head[MAX_BATCH]; uint32_t blocks[MAX_BATCH]; };
struct RasterBatch { const PassParams* params[MAX_BATCH]; RasterHead head[MAX_BATCH]; };

}  // namespace mirhi
