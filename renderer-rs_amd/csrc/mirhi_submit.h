// mirhi_submit.h -- how a submit goes out: as one batched launch triple, as AQL packets or as HIP launches; what carries its fence; and, per scope,
// the memory scopes of its packets, the triangles per geometry wave, whether it may take a wide variant, whether it is timed and counted.  Decided
// here and nowhere else: submit_now (mirhi_api.hip) gathers the facts, asks, and issues what the answers say.  Plain C++, no HIP, no HSA: the
// decisions can be stated and tested on a machine without a GPU (mirhi_debug_submit_path, tests/test_submit_path_cpu.py).
#pragma once
#include <stdint.h>

#include "../../include/mirhi.h"
#include "mirhi_device.h"
#include "mirhi_native_flags.h"
#include "mirhi_variant.h"

namespace mirhi {

// ---- the facts a submit looks at ----
// The once-per-process switches (NativeEnv of mirhi_api.hip) and the one per-submit knob (PlanKnobs) the submit reads, by value
struct SubmitSwitches {
    bool no_batch, fence_record;      // MIRHI_NO_BATCH, MIRHI_FENCE_RECORD
    int system_scope;                 // MIRHI_NATIVE_SYSTEM_SCOPE: 1 system scope on every packet, 2 on every scope's first (A/B runs)
    int geom_tpw;                     // MIRHI_GEOM_TPW: triangles per geometry wave (16 / 32 / 64; 0 = the host's choice)
    bool wide_set;                    // MIRHI_RASTER_WIDE is set (PlanKnobs::raster_wide.set)
};
struct SubmitDevice {
    uint32_t profiling;               // MIRHI_PROFILE_* bits; bits 8..15: lane + 1 that timing is restricted to
    bool native_ok;                   // native dispatch is there (mirhi_device::native && native->ok)
    bool owns_stream, native_on_external;
    uint32_t lanes;                   // queue lanes of the device
};
// One command buffer of the submit ...
struct SubmitCmd {
    const void* self;                 // which one it is (a submit may name a command buffer twice)
    uint32_t lane, scopes;            // its queue lane, entries of its plan
    bool any_ordered;                 // some scope is an ordered segment (PassParams::ordered_recs)
    bool last_has_tiles;              // it has a last scope and that one a raster launch (has_tiles)
};
// ... and its first scope, looked at only while the submit may still be batched (raster_variant is not free, and a submit of one command buffer never asks)
struct SubmitHead {
    RasterVariant variant;            // (a plan that names a wide variant is not batched, whether or not a submit would take it: the variant as with allow_wide)
    uint32_t programs;
    bool color_load, depth_load;
    const void *color, *depth, *prim_out;
};
inline SubmitHead submit_head(const PassParams& P, uint32_t programs) {
    return SubmitHead{raster_variant(P, programs, true), programs, P.color_load != 0u, P.depth_load != 0u, P.color, P.depth, P.prim_out};
}

// a scope has a raster launch (its band of a split frame may be empty)
inline bool has_tiles(const PassParams& P) { return P.tile_row_end > P.tile_row_begin && P.tiles_x; }
// plan: the command buffer's scopes (mirhi_cmd::plan)
inline SubmitCmd submit_cmd(const void* self, uint32_t lane, const PassParams* plan, size_t scopes) {
    bool ordered = false;
    for (size_t i = 0; i < scopes; i++) ordered = ordered || plan[i].ordered_recs;
    return SubmitCmd{self, lane, (uint32_t)scopes, ordered, scopes != 0 && has_tiles(plan[scopes - 1])};
}

// ---- the path ----
struct SubmitPath {
    uint32_t count, last_scopes;      // command buffers; scopes of the last one
    bool batched;                     // one vertex, one geometry and one raster launch for all command buffers
    bool native;                      // AQL packets on the lane's own queue.  From submit_path: eligible -- the lane's queue may still not open
                                      // (native_lane, mirhi_api.hip), the caller then clears it; fence_carrier takes the final answer
    bool one_lane, last_has_tiles;
};

// cmd_at(i) -> SubmitCmd, head_at(i) -> SubmitHead of command buffer i (asked at most once each, head_at only of command buffers with one scope)
template <typename CmdAt, typename HeadAt>
inline SubmitPath submit_path(const SubmitDevice& d, const SubmitSwitches& sw, uint32_t count, CmdAt&& cmd_at, HeadAt&& head_at) {
    SubmitPath p{count, 0u, false, false, true, false};
    // Batched form: the command buffers of one submit, when each is one plain rendering scope of the same shape and kernel variants
    // (the frames of a frame loop), share one vertex, one geometry and one raster launch on the first one's queue lane -- the
    // ramp-up and drain of a kernel and the latency chain of the geometry kernel are paid once per batch, not once per frame.
    // Only frames that are independent of each other may share a launch: every scope clears (no LOAD of colour or depth -- what it
    // would load might be written by another scope of the batch), no two scopes share a colour, depth or primitive-id attachment, and
    // all command buffers sit on the first one's queue lane (so the batch keeps their order against earlier work of that lane).
    // A scope with a partial render area never joins a batch: the batched raster kernel takes one grid for all its scopes, and an area
    // scope's grid is its own tile range (RasterVariant::batched_form is 0 for it, so the comparison below fails whatever the other scopes are).
    // Nor does a 4x multisampled scope: its family has no batched form (RasterVariant::batched_form is 0), and its geometry kernel is not the batch's.
    // Anything else runs command buffer by command buffer, in submission order on each lane.
    p.batched = count >= 2 && count <= (uint32_t)MAX_BATCH && d.profiling == 0 && !sw.no_batch;
    SubmitHead heads[MAX_BATCH];
    const void* selves[MAX_BATCH];
    uint32_t lane0 = 0;
    bool lanes_exist = true, any_ordered = false;
    for (uint32_t i = 0; i < count; i++) {
        const SubmitCmd c = cmd_at(i);
        if (i == 0) lane0 = c.lane;
        p.one_lane = p.one_lane && c.lane == lane0;
        lanes_exist = lanes_exist && c.lane < d.lanes;
        any_ordered = any_ordered || c.any_ordered;
        if (i + 1 == count) { p.last_scopes = c.scopes; p.last_has_tiles = c.last_has_tiles; }
        if (!p.batched) continue;
        p.batched = c.scopes == 1 && c.lane == lane0;
        if (!p.batched) continue;
        const SubmitHead& h = heads[i] = head_at(i);
        selves[i] = c.self;
        p.batched = h.variant.batched_form && h.variant == heads[0].variant && h.programs == heads[0].programs && !h.color_load && !h.depth_load;
        for (uint32_t j = 0; p.batched && j < i; j++) {
            const SubmitHead& a = heads[j];
            p.batched = selves[j] != c.self && a.color != h.color && !(a.depth && a.depth == h.depth) && !(a.prim_out && a.prim_out == h.prim_out);
        }
    }
    // Native dispatch (mirhi_native.h): the submit's kernels go out as AQL packets on the lane's own queue -- when nothing of the submit
    // needs the HIP stream: no timed dispatches, no batch, no tile split (the band exchange lives on HIP streams), no ordered segment
    // (its clear is a HIP memset), every command buffer on one lane.
    // A device made on the caller's stream (mirhi_device_create_on_stream) promised that lane 0's work is issued on that stream: submits to lane 0 stay in
    // stream order (HIP launches) unless the caller opted in (mirhi_device_set_native_dispatch); lanes the library made itself are the library's.
    p.native = !p.batched && count >= 1 && d.native_ok && d.profiling == 0 && (d.owns_stream || d.native_on_external || lane0 != 0u) &&
               p.one_lane && lanes_exist && !any_ordered;
    return p;
}

// ---- the fence ----
// What signals a submit's fence
enum FenceCarrier : uint32_t {
    FENCE_NONE,             // the submit has no fence
    FENCE_STOP_EVENT,       // the stop event of the submit's last dispatch (hipExtLaunchKernelGGL)
    FENCE_NATIVE_SIGNAL,    // the completion signal of its last packet
    FENCE_EVENT_RECORD,     // an event record on the last command buffer's lane, after joining the other lanes of the submit
    FENCE_NATIVE_DRAIN,     // nothing to ride on (no tiles to raster): the host drains the queue and stores the signal, the fence is signalled at once
};
// p: with `native` as it came out in the end
inline FenceCarrier fence_carrier(const SubmitPath& p, const SubmitDevice& d, const SubmitSwitches& sw, bool has_fence) {
    if (!has_fence) return FENCE_NONE;
    if (p.native) return p.last_has_tiles ? FENCE_NATIVE_SIGNAL : FENCE_NATIVE_DRAIN;
    // The fence rides on the submit's last dispatch (its completion signal: hipExtLaunchKernelGGL stop event) when there is one and
    // everything of the submit runs on one stream -- an event RECORD is a command of its own in the stream: 4.5 us of stream time and
    // a round trip of 12-14 us against 6-9 us (tools/microbench/fence_latency.hip).
    const bool one_stream = p.count >= 1 && d.profiling == 0 && !sw.fence_record && (p.batched || p.one_lane);      // (never together with a timed dispatch)
    return one_stream && p.last_has_tiles ? FENCE_STOP_EVENT : FENCE_EVENT_RECORD;
}
// scope `scope` of command buffer `cmd` is the one whose raster launch carries the fence (of a submit that is not batched: a batch has one raster launch)
inline bool carries_fence(FenceCarrier k, const SubmitPath& p, uint32_t cmd, size_t scope) {
    return (k == FENCE_STOP_EVENT || k == FENCE_NATIVE_SIGNAL) && cmd + 1 == p.count && scope + 1 == p.last_scopes;
}

// ---- per scope ----
// A SKYBOX segment takes no bins and touches no counter: it re-arms nothing and the parity of the big-list counters stays where it is -- the raster
// kernel that follows finds the counters as the one before the sky left them; and so a transfer entry.  Neither has a
// vertex or geometry packet.
inline bool single_packet(const PassParams& P) { return P.sky || P.xfer; }
inline bool flips_parity(const PassParams& P) { return !single_packet(P); }

// NATIVE_* flags of a scope's vertex, geometry and raster packet.  The scope's first kernels see what the host wrote (parameter block, buffers
// uploaded since); its raster kernel publishes the frame -- the acquire is at system scope when something other than this library's kernels wrote
// device memory since this queue last acquired at system scope (unseen_foreign: mirhi_device::foreign_writes against NativeQueue::seen_foreign;
// ws_foreign: Workspace::foreign).
struct PacketScopes { uint32_t vertex, geometry, raster; };
inline PacketScopes packet_scopes(const PassParams& P, int system_scope, bool unseen_foreign, bool ws_foreign) {
    const bool sys = system_scope == 1;
    const bool head_sys = sys || system_scope == 2 || unseen_foreign || ws_foreign;
    PacketScopes f;
    f.vertex = (head_sys ? NATIVE_ACQUIRE_SYSTEM : 0u) | (sys ? NATIVE_RELEASE_SYSTEM : 0u);
    f.geometry = (((P.vs_total_slots == 0u && head_sys) || sys) ? NATIVE_ACQUIRE_SYSTEM : 0u) | (sys ? NATIVE_RELEASE_SYSTEM : 0u);      // (behind a vertex kernel: that one took the acquire)
    f.raster = NATIVE_RELEASE_SYSTEM | (sys ? NATIVE_ACQUIRE_SYSTEM : 0u);
    if (single_packet(P) && head_sys) f.raster |= NATIVE_ACQUIRE_SYSTEM;      // (a SKYBOX segment or a transfer has no vertex or geometry packet: its only one takes the head's acquire)
    return f;
}

// small scopes: fewer triangles per geometry wave (GeometryHead::tris_per_wave) -- the chip is mostly idle, a shorter wave is a shorter frame
inline uint32_t tris_per_wave(const PassParams& P, int geom_tpw) {
    const uint32_t geo_waves = P.total_slots / (uint32_t)GEOM_THREADS;
    return geom_tpw ? (uint32_t)geom_tpw : (geo_waves <= 256u ? 16u : (geo_waves <= 512u ? 32u : 64u));
}

// in_flight: frames in flight, this one included (command buffers submitted and not yet known to have finished).  The wide mesh variants trade
// throughput for latency -- a frame alone on the chip finishes sooner (C3 raster 32 -> 25 us), four frames in flight leave each
// other less room (C3 16.2 -> 19.8 us per frame) -- so a submit takes them only while the queue is shallow: the reference's
// MAX_FRAMES_IN_FLIGHT = 2 loop does, a loop that keeps four frames queued gets the plain / two-team variants.
inline bool allow_wide(int in_flight, bool wide_set) { return in_flight <= 2 || wide_set; }

// (timing may be restricted to one queue lane -- bits 8..15 of the mask hold lane + 1 -- so that the other lanes run
// untimed: a timed dispatch completes through its own signal and does not overlap its neighbours the way an untimed one does)
inline bool scope_timed(uint32_t profiling, uint32_t lane) {
    const uint32_t only_lane = (profiling >> 8) & 0xFFu;
    return (profiling & MIRHI_PROFILE_TIMING) != 0 && (only_lane == 0u || only_lane - 1u == lane);
}
// the statistics pass runs for the scope (ordered -- blended -- segments, depth-only scopes, SKYBOX segments and transfers are not counted)
inline bool scope_counted(uint32_t profiling, const PassParams& P) {
    return (profiling & MIRHI_PROFILE_FRAGMENTS) != 0 && has_tiles(P) && !P.ordered_recs && !P.depth_only && !P.sky && !P.xfer && !P.samples;      // (a multisampled scope: refused by build_plan)
}

// ---- feedback (status_of) ----
// Waves per tile of the wide variant a command buffer should plan next, from the busy tiles of its last scope and the width in use (Workspace::wide).
// Sixteen waves per tile are one workgroup per CU at a time: for up to ~240 busy tiles (the dancer asset: 232; raster 39 -> 30 us);
// eight waves are two per CU: up to ~512 (the 70k-triangle sphere: 419; 32.5 -> 24.8 us, sixteen: 31.7 in two rounds).  Hysteresis
// of a quarter so that a frame loop does not flip between two plans.
inline uint32_t wide_wanted(uint32_t busy_tiles, uint32_t cur) {
    if (busy_tiles == 0u) return 0u;
    if (busy_tiles <= (cur == 16u ? 300u : 240u)) return 16u;
    if (busy_tiles <= (cur == 8u ? 640u : 512u)) return 8u;
    return 0u;
}

// ---- as words (mirhi_debug_submit_path: tests/test_submit_path_cpu.py replays tests/golden/submit_paths.json through it) ----
// in[0] says what is asked; returns 0, or -1 for words it cannot take.
// 0  the path.  in: profiling, native available, owns_stream, native_on_external, lanes, no_batch, fence_record, "the lane's queue opens", "with a
//    fence", command buffers (at most MAX_BATCH + 1); per command buffer 16 words: id, lane, scopes (at most 2), of a second scope: ordered, has tile
//    rows; of the first: programs, tp_max_area, tiles_x, tile rows, raster_wide, ordered, color_load, depth_load, colour, depth, prim_out (addresses
//    as numbers).  The facts are gathered from scopes made of these words as submit_now gathers them (submit_cmd, submit_head).
//    out: batched, native-eligible, native, fence carrier, the command buffer and the scope that carry it (~0: none does)
// 1  a scope.  in: system_scope, unseen foreign write, Workspace::foreign, vs_total_slots, kind (0 plain, 1 ordered, 2 depth-only, 3 sky, 4 transfer),
//    total_slots, geom_tpw, frames in flight, MIRHI_RASTER_WIDE set, profiling, lane, tile rows, tiles_x.
//    out: flags of the vertex, geometry and raster packet, triangles per wave, allow_wide, timed, counted, parity flips
// 2  the wide feedback.  in: busy tiles, width in use.  out: width wanted
inline int submit_words(const uint32_t* in, uint32_t* out) {
    static TriRec some_recs;
    if (in[0] == 2u) { out[0] = wide_wanted(in[1], in[2]); return 0; }
    if (in[0] == 1u) {
        PassParams P{};
        P.vs_total_slots = in[4]; P.total_slots = in[6]; P.tile_row_end = in[12]; P.tiles_x = in[13];
        P.ordered_recs = in[5] == 1u ? &some_recs : nullptr; P.depth_only = in[5] == 2u; P.sky = in[5] == 3u; P.xfer = in[5] == 4u;
        const PacketScopes f = packet_scopes(P, (int)in[1], in[2] != 0u, in[3] != 0u);
        const uint32_t words[8] = {f.vertex, f.geometry, f.raster, tris_per_wave(P, (int)in[7]), allow_wide((int)in[8], in[9] != 0u), scope_timed(in[10], in[11]),
                                   scope_counted(in[10], P), flips_parity(P)};
        for (int i = 0; i < 8; i++) out[i] = words[i];
        return 0;
    }
    const uint32_t n = in[10];
    if (in[0] != 0u || n > (uint32_t)MAX_BATCH + 1u) return -1;
    const SubmitDevice d{in[1], in[2] != 0u, in[3] != 0u, in[4] != 0u, in[5]};
    const SubmitSwitches sw{in[6] != 0u, in[7] != 0u, 0, 0, false};
    const uint32_t* cmds = in + 11;
    for (uint32_t i = 0; i < n; i++) if (cmds[16 * i + 2] > 2u) return -1;
    auto scope_at = [&](uint32_t i, uint32_t scope) {
        const uint32_t* w = cmds + 16 * i;
        PassParams P{};
        P.zmask = 0xFFFFFFFFu; P.tiles_x = 5u; P.tile_row_end = 4u; P.tile_row_step = 1u;
        if (scope == 0u) {
            P.tp_max_area = w[6]; P.tiles_x = w[7]; P.tile_row_end = w[8]; P.raster_wide = w[9]; P.ordered_recs = w[10] ? &some_recs : nullptr;
            P.color_load = w[11]; P.depth_load = w[12]; P.color = (void*)(uintptr_t)w[13]; P.depth = (float*)(uintptr_t)w[14]; P.prim_out = (uint32_t*)(uintptr_t)w[15];
        } else { P.ordered_recs = w[3] ? &some_recs : nullptr; P.tile_row_end = w[4] ? 4u : 0u; }
        return P;
    };
    SubmitPath p = submit_path(d, sw, n,
                               [&](uint32_t i) {
                                   const uint32_t* w = cmds + 16 * i;
                                   const PassParams plan[2] = {scope_at(i, 0u), scope_at(i, 1u)};
                                   return submit_cmd((const void*)(uintptr_t)w[0], w[1], plan, w[2]);
                               },
                               [&](uint32_t i) { return submit_head(scope_at(i, 0u), cmds[16 * i + 5]); });
    out[0] = p.batched; out[1] = p.native;
    p.native = p.native && in[8] != 0u;
    const FenceCarrier k = fence_carrier(p, d, sw, in[9] != 0u);
    out[2] = p.native; out[3] = k; out[4] = out[5] = ~0u;
    for (uint32_t i = 0; !p.batched && i < n; i++)
        for (uint32_t pi = 0; pi < cmds[16 * i + 2]; pi++)
            if (carries_fence(k, p, i, pi)) {
                if (out[4] != ~0u) return -1;
                out[4] = i; out[5] = pi;
            }
    return 0;
}

}  // namespace mirhi
