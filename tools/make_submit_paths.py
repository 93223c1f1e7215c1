#!/usr/bin/env python3
"""Records what a commit's submit_now decides about a submit: tests/golden/submit_paths.json.

    tools/make_submit_paths.py CHECKOUT [--out FILE]

CHECKOUT is a checkout of the commit that still decides these things inside submit_now and status_of of csrc/mirhi_api.hip (the fixture
names it: "parent").  The deciding lines are cut out of that file by anchor lines (ANCHORS; every anchor must match exactly once), the
NATIVE_* flags out of its csrc/mirhi_native.h.  The text is compiled with g++ in a temporary directory against that checkout's plain
headers and stub mirhi_cmd, mirhi_device, mirhi_fence, NativeQueue and native_env() definitions, and run over the grids below.  No GPU,
no HIP.

The fixture is what tests/test_submit_path_cpu.py replays through mirhi_debug_submit_path of the library under test; a row's input
words are that export's (csrc/mirhi_submit.h: submit_words).

The grids, each a full product of its axes (first axis slowest).
 "batch"    what the batched form looks at.  Command buffers 1 / 2 / 3 / MAX_BATCH / MAX_BATCH + 1; all on lane 0 or the last on lane 1; the
            last one's first scope against the others': equal, another kernel (triangle-parallel path), another grid, no batched form
            (raster_wide), another program set -- or equal with no batched form in any of them; no LOAD, a colour LOAD, a depth LOAD (in the
            last); the last shares nothing, its colour, depth or primitive-id address with the first, is the first once more -- or none of
            them has a depth, or a primitive-id attachment; the last has 0 / 1 / 2 scopes; profiling 0 / timing / fragments; MIRHI_NO_BATCH.
            Held: no native dispatch, a fence, every scope with tiles.
 "path"     what native dispatch and the fence look at.  Command buffers and lanes as above; batchable or not (the last one's grid); the last
            has 0 / 1 / 2 scopes; no ordered scope, its last or its first; its last scope with tiles; profiling 0 / timing / fragments; native dispatch
            there; owns_stream; native_on_external; the first lane 0 / 1; a device of 1 / 4 lanes; the lane's queue opens; a fence;
            MIRHI_FENCE_RECORD.  Held: MIRHI_NO_BATCH unset, no LOAD, nothing shared (the batched answer enters as one bit: "batch" has it).
 "flags"    MIRHI_NATIVE_SYSTEM_SCOPE 0 / 1 / 2; a foreign write the queue has not seen; Workspace::foreign; vs_total_slots 0 / 64; a plain,
            sky or transfer scope.
 "tpw"      total_slots at geometry waves 0, 256, 257 - 1 slot, 257, 512, 513 - 1 slot, 513; MIRHI_GEOM_TPW 0 / 16 / 32 / 64.
 "wide"     frames in flight 1 / 2 / 3; MIRHI_RASTER_WIDE set.
 "profile"  profiling 0, timing, fragments, timing on lane 0 only, timing on lane 1 only, timing + fragments; lane 0 / 1; a plain, ordered,
            depth-only, sky or transfer scope; tile rows 4 / 0; tiles_x 5 / 0.
 "feedback" busy tiles 0, 240, 241, 300, 301, 512, 513, 640, 641; width in use 0 / 8 / 16.
"""
import argparse
import hashlib
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BATCH, GEOM_THREADS = 8, 64
TIMING, FRAGMENTS = 1, 2
COUNTS = [1, 2, 3, MAX_BATCH, MAX_BATCH + 1]
VARIANTS = ["equal", "kernel", "grid", "batched_form", "programs", "none_batched"]
LOADS = ["none", "colour", "depth"]
SHARED = ["none", "colour", "depth", "prim_out", "same", "no_depth", "no_prim_out"]
SCOPES = [0, 1, 2]
BATCH_AXES = [("count", COUNTS), ("other_lane", [0, 1]), ("variant", VARIANTS), ("load", LOADS), ("shared", SHARED), ("scopes", SCOPES),
              ("profiling", [0, TIMING, FRAGMENTS]), ("no_batch", [0, 1])]
PATH_AXES = [("count", COUNTS), ("other_lane", [0, 1]), ("batchable", [1, 0]), ("scopes", SCOPES), ("ordered", ["none", "last", "first"]), ("tiles", [1, 0]),
             ("profiling", [0, TIMING, FRAGMENTS]), ("native", [0, 1]), ("owns_stream", [0, 1]), ("native_on_external", [0, 1]), ("lane0", [0, 1]),
             ("lanes", [1, 4]), ("queue_opens", [1, 0]), ("fence", [0, 1]), ("fence_record", [0, 1])]
KINDS = ["plain", "ordered", "depth_only", "sky", "transfer"]
FLAGS_AXES = [("system_scope", [0, 1, 2]), ("unseen_foreign", [0, 1]), ("ws_foreign", [0, 1]), ("vs_total_slots", [0, 64]), ("kind", ["plain", "sky", "transfer"])]
TPW_AXES = [("total_slots", [0, 256 * GEOM_THREADS, 257 * GEOM_THREADS - 1, 257 * GEOM_THREADS, 512 * GEOM_THREADS, 513 * GEOM_THREADS - 1, 513 * GEOM_THREADS]),
            ("geom_tpw", [0, 16, 32, 64])]
WIDE_AXES = [("in_flight", [1, 2, 3]), ("wide_set", [0, 1])]
PROFILE_AXES = [("profiling", [0, TIMING, FRAGMENTS, TIMING | 1 << 8, TIMING | 2 << 8, TIMING | FRAGMENTS]), ("lane", [0, 1]), ("kind", KINDS), ("tile_rows", [4, 0]), ("tiles_x", [5, 0])]
FEEDBACK_AXES = [("busy_tiles", [0, 240, 241, 300, 301, 512, 513, 640, 641]), ("wide", [0, 8, 16])]
PIECE = 64


def cmd_words(ident, lane=0, scopes=1, ordered="none", tiles=1, variant="equal", load="none", color=None, depth=None, prim_out=None):
    """The 16 words of one command buffer: a frame of a frame loop (one PBR scope of 5 x 4 tiles with targets of its own), changed as asked.  ordered: "none", or
    the "first" or the "last" scope is an ordered one; tiles: the last scope has tile rows (a first of two always has)."""
    first_ordered = int(scopes >= 1 and (ordered == "first" or (ordered == "last" and scopes == 1)))
    return [ident, lane, scopes, int(scopes == 2 and ordered == "last"), int(scopes == 2 and tiles),
            5 if variant == "programs" else 4, 64 if variant == "kernel" else 0, 6 if variant == "grid" else 5, 4 if (scopes != 1 or tiles) else 0,
            8 if variant == "batched_form" else 0, first_ordered, int(load == "colour"), int(load == "depth"),
            1000 + ident if color is None else color, 2000 + ident if depth is None else depth, 3000 + ident if prim_out is None else prim_out]


def path_words(cmds, profiling=0, native=0, owns_stream=1, native_on_external=0, lanes=4, no_batch=0, fence_record=0, queue_opens=1, fence=1):
    return [0, profiling, native, owns_stream, native_on_external, lanes, no_batch, fence_record, queue_opens, fence, len(cmds)] + [w for c in cmds for w in c]


def batch_row(count, other_lane, variant, load, shared, scopes, profiling, no_batch):
    every = {}          # what the axis value says of every command buffer, not of the last alone
    if shared == "no_depth":
        every["depth"] = 0
    if shared == "no_prim_out":
        every["prim_out"] = 0
    if variant == "none_batched":
        every["variant"] = variant = "batched_form"
    cmds = [cmd_words(i + 1, **every) for i in range(count - 1)]
    if shared == "same" and count >= 2:
        cmds.append(list(cmds[0]))          # (the first once more: whatever the other axes say)
    else:
        last = dict(every, variant=variant, **{"colour": dict(color=1001), "depth": dict(depth=2001), "prim_out": dict(prim_out=3001)}.get(shared, {}))
        cmds.append(cmd_words(count, lane=other_lane, scopes=scopes, load=load, **last))
    return path_words(cmds, profiling=profiling, no_batch=no_batch)


def path_row(count, other_lane, batchable, scopes, ordered, tiles, profiling, native, owns_stream, native_on_external, lane0, lanes, queue_opens, fence, fence_record):
    cmds = [cmd_words(i + 1, lane=lane0, tiles=tiles) for i in range(count - 1)]
    cmds.append(cmd_words(count, lane=lane0 ^ other_lane, scopes=scopes, ordered=ordered, tiles=tiles, variant="equal" if batchable else "grid"))
    return path_words(cmds, profiling=profiling, native=native, owns_stream=owns_stream, native_on_external=native_on_external, lanes=lanes,
                      fence_record=fence_record, queue_opens=queue_opens, fence=fence)


def scope_words(system_scope=0, unseen_foreign=0, ws_foreign=0, vs_total_slots=64, kind="plain", total_slots=64, geom_tpw=0, in_flight=1, wide_set=0, profiling=0, lane=0, tile_rows=4, tiles_x=5):
    return [1, system_scope, unseen_foreign, ws_foreign, vs_total_slots, KINDS.index(kind), total_slots, geom_tpw, in_flight, wide_set, profiling, lane, tile_rows, tiles_x]


def feedback_words(busy_tiles, wide):
    return [2, busy_tiles, wide]


# name -> (axes, input words of a row, first and number of the output words the grid is about)
GRIDS = {"batch": (BATCH_AXES, batch_row, 0, 6), "path": (PATH_AXES, path_row, 0, 6),
         "flags": (FLAGS_AXES, lambda **a: scope_words(**a), 0, 3), "tpw": (TPW_AXES, lambda **a: scope_words(**a), 3, 1),
         "wide": (WIDE_AXES, lambda **a: scope_words(**a), 4, 1), "profile": (PROFILE_AXES, lambda **a: scope_words(**a), 5, 3),
         "feedback": (FEEDBACK_AXES, lambda **a: feedback_words(**a), 0, 1)}


def rows_of(grid):
    axes, make, _, _ = GRIDS[grid]
    names = [n for n, _ in axes]
    for values in itertools.product(*[v for _, v in axes]):
        yield make(**dict(zip(names, values)))


# (start of the line that begins the cut, start of the line that ends it and is not part of it)
ANCHORS = {
    "path": ("    bool batched = cmd_count >= 2 && cmd_count <= (uint32_t)MAX_BATCH", "    if (use_native) keep_locked = true;"),
    "fence": ("        bool one_stream = cmd_count >= 1", "    }\n    if (batched) {\n        hipStream_t stream"),
    "batch_fence": ("        fence_attached = fence_stop != nullptr;", "    }\n    for (uint32_t i = 0; !batched && i < cmd_count; i++) {"),
    "wide": ("        int in_flight = 1;", "        c->last_stream = use_native ? nullptr : stream;"),
    "parity": ("            if (!P.sky && !P.xfer) c->ws.parity ^= 1u;", "            // ordered segment: slots of primitives"),
    "flags": ("            if (use_native) {\n                tv.native = nq;", "            // (timing may be restricted to one queue lane"),
    "timed": ("            const uint32_t only_lane = ", "            if (timed) {"),
    "tiles": ("            const bool has_tiles = P.tile_row_end", "            const uint32_t* winners = nullptr;"),
    "counted": ("            if (counted && has_tiles && ", "                if (timed && (r = timing_begin(dev, MIRHI_KERNEL_FRAGMENT_COUNT"),
    "carrier": ("            if (fence_stop && i + 1 == cmd_count", "            if (!keep_locked) lock.unlock();\n            le = launch_raster("),
    "want": ("            const uint32_t b = c->ws.busy_tiles, cur = c->ws.wide;", "            if (want != cur && c->ws.wide_eligible"),
}
NATIVE_FLAGS = ("enum : uint32_t { NATIVE_ACQUIRE_SYSTEM", "hipError_t native_enqueue(")

HARNESS = r"""
#include <atomic>
#include <cstdio>
#include <cstring>
#include <vector>
#include "mirhi.h"
#include "mirhi_device.h"
#include "mirhi_variant.h"
#include "mirhi_scope.h"
using namespace mirhi;
typedef void* hipEvent_t;
typedef void* hipStream_t;
@native_flags@
struct NativeQueue { uint64_t seen_foreign = 0; };
struct NativeDevice { bool ok = false; };
struct NativeEnv { int system_scope = 0, geom_tpw = 0; bool no_batch = false, fence_record = false; };
static NativeEnv g_env;
static const NativeEnv& native_env() { return g_env; }
struct LaunchTiming { hipEvent_t start = nullptr, stop = nullptr; NativeQueue* native = nullptr; uint64_t native_signal = 0; uint32_t native_flags = 0, tris_per_wave = 0; const DrawDesc* head_draw = nullptr; };
struct Planned { std::vector<DrawDesc> draws; };
struct mirhi_cmd {
    uint32_t lane = 0; bool pending = false;
    std::vector<PassParams> plan; std::vector<uint32_t> plan_programs; std::vector<Planned> planned;
    struct { bool foreign = false; uint32_t parity = 0, busy_tiles = 0, wide = 0; } ws;
};
struct mirhi_device {
    uint32_t profiling = 0; NativeDevice* native = nullptr; bool owns_stream = false, native_on_external = false;
    std::vector<hipStream_t> lanes; std::vector<mirhi_cmd*> cmds; std::atomic<uint64_t> foreign_writes{1};
};
struct mirhi_fence { hipEvent_t event; struct { uint64_t handle; } native_sig; };
static NativeQueue g_queue;
static bool g_queue_opens, g_queue_asked;
static NativeQueue* native_lane(mirhi_device*, uint32_t) { g_queue_asked = true; return g_queue_opens ? &g_queue : nullptr; }
static TriRec some_recs;
enum { NONE, STOP_EVENT, NATIVE_SIGNAL, EVENT_RECORD, NATIVE_DRAIN };

static int path(mirhi_device* dev, uint32_t cmd_count, mirhi_cmd* const* cmds, mirhi_fence* fence, unsigned out[6]) {
    bool keep_locked = false;
    g_queue_asked = false;
@path@
    const bool eligible = g_queue_asked;
    hipEvent_t fence_stop = nullptr;
    bool fence_attached = false;
    if (fence && !use_native) {
@fence@
    }
    if (batched) {
@batch_fence@
    }
    unsigned carrier_cmd = ~0u, carrier_scope = ~0u;
    for (uint32_t i = 0; !batched && i < cmd_count; i++) {
        mirhi_cmd* c = cmds[i];
        for (size_t pi = 0; pi < c->plan.size(); pi++) {
            const PassParams& P = c->plan[pi];
            LaunchTiming tr{};
            fence_attached = false;
@tiles@
@carrier@
            if (fence_attached && carrier_cmd != ~0u) return 5;
            if (fence_attached) { carrier_cmd = i; carrier_scope = (unsigned)pi; }
            if (fence_attached != ((tr.stop != nullptr) != (tr.native_signal != 0))) return 6;
        }
    }
    if (carrier_cmd != ~0u) fence_attached = true;
    // (what submit_now does with a fence that nothing carried: drain and store natively, else join the lanes and record the event)
    const unsigned carrier = !fence ? NONE : (use_native ? (fence_attached ? NATIVE_SIGNAL : NATIVE_DRAIN) : (fence_attached ? STOP_EVENT : EVENT_RECORD));
    out[0] = batched; out[1] = eligible; out[2] = use_native; out[3] = carrier; out[4] = carrier_cmd; out[5] = carrier_scope;
    (void)keep_locked; (void)nq;
    return 0;
}

static void scope(mirhi_device* dev, mirhi_cmd* c, NativeQueue* nq, const PlanKnobs& knobs, unsigned out[8]) {
    const bool use_native = true;
    const size_t pi = 0;
    const PassParams& P = c->plan[0];
    LaunchTiming tv{}, tg{}, tr{};
    const uint32_t parity = c->ws.parity;
@wide@
@parity@
@flags@
@timed@
@tiles@
    bool is_counted = false;
@counted@
        (void)r; is_counted = true;
    }
    const unsigned words[8] = {tv.native_flags, tg.native_flags, tr.native_flags, tg.tris_per_wave, allow_wide, timed, is_counted, c->ws.parity != parity};
    memcpy(out, words, sizeof words);
}

static unsigned feedback(mirhi_cmd* c) {
@want@
    return want;
}

// stdin: one row per line, the input words of mirhi_debug_submit_path; stdout: its output words
int main() {
    unsigned mode;
    while (scanf("%u", &mode) == 1) {
        unsigned in[11 + 16 * (MAX_BATCH + 1)] = {mode};
        const unsigned fixed = mode == 0u ? 11u : (mode == 1u ? 14u : 3u);
        for (unsigned i = 1; i < fixed; i++) if (scanf("%u", &in[i]) != 1) return 2;
        mirhi_device dev;
        NativeDevice nd;
        if (mode == 2u) {
            mirhi_cmd c; c.ws.busy_tiles = in[1]; c.ws.wide = in[2];
            printf("%u\n", feedback(&c));
            continue;
        }
        if (mode == 1u) {
            g_env = NativeEnv{(int)in[1], (int)in[7], false, false};
            dev.profiling = in[10];
            dev.foreign_writes = 5; g_queue.seen_foreign = in[2] ? 4 : 5;
            mirhi_cmd c, idle, busy[2];
            c.lane = in[11]; c.ws.foreign = in[3] != 0u;
            PassParams P{};
            P.vs_total_slots = in[4]; P.total_slots = in[6]; P.tile_row_end = in[12]; P.tiles_x = in[13];
            P.ordered_recs = in[5] == 1u ? &some_recs : nullptr; P.depth_only = in[5] == 2u; P.sky = in[5] == 3u; P.xfer = in[5] == 4u;
            c.plan.push_back(P);
            dev.cmds = {&idle, &c};
            for (unsigned i = 1; i < in[8] && i < 3; i++) { busy[i - 1].pending = true; dev.cmds.push_back(&busy[i - 1]); }
            PlanKnobs knobs;
            knobs.raster_wide.set = in[9] != 0u;
            unsigned out[8];
            scope(&dev, &c, &g_queue, knobs, out);
            if (g_queue.seen_foreign != 5 || c.ws.foreign) return 7;
            printf("%u %u %u %u %u %u %u %u\n", out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7]);
            continue;
        }
        const unsigned n = in[10];
        if (n > (unsigned)MAX_BATCH + 1u) return 3;
        for (unsigned i = 0; i < 16 * n; i++) if (scanf("%u", &in[11 + i]) != 1) return 2;
        g_env = NativeEnv{0, 0, in[6] != 0u, in[7] != 0u};
        dev.profiling = in[1]; nd.ok = true; dev.native = in[2] ? &nd : nullptr; dev.owns_stream = in[3] != 0u; dev.native_on_external = in[4] != 0u;
        dev.lanes.resize(in[5]);
        g_queue_opens = in[8] != 0u;
        mirhi_fence fence{&dev, {7}};
        mirhi_cmd storage[MAX_BATCH + 1];
        mirhi_cmd* by_id[MAX_BATCH + 2] = {};
        mirhi_cmd* cmds[MAX_BATCH + 1];
        for (unsigned i = 0; i < n; i++) {
            const unsigned* w = in + 11 + 16 * i;
            if (w[0] > (unsigned)MAX_BATCH + 1u || w[2] > 2u) return 3;
            if (by_id[w[0]]) { cmds[i] = by_id[w[0]]; continue; }      // (the same command buffer once more)
            mirhi_cmd* c = cmds[i] = by_id[w[0]] = &storage[i];
            c->lane = w[1];
            for (unsigned s = 0; s < w[2]; s++) {
                PassParams P{};
                P.zmask = 0xFFFFFFFFu; P.tiles_x = 5; P.tile_row_end = 4; P.tile_row_step = 1;
                if (s == 0) {
                    P.tp_max_area = w[6]; P.tiles_x = w[7]; P.tile_row_end = w[8]; P.raster_wide = w[9]; P.ordered_recs = w[10] ? &some_recs : nullptr;
                    P.color_load = w[11]; P.depth_load = w[12]; P.color = (void*)(size_t)w[13]; P.depth = (float*)(size_t)w[14]; P.prim_out = (uint32_t*)(size_t)w[15];
                }
                if (s + 1 == w[2] && s != 0) { P.tile_row_end = w[4] ? 4 : 0; P.ordered_recs = w[3] ? &some_recs : nullptr; }
                c->plan.push_back(P);
                c->plan_programs.push_back(s == 0 ? w[5] : 4u);
            }
        }
        unsigned out[6];
        const int rc = path(&dev, n, cmds, in[9] ? &fence : nullptr, out);
        if (rc) return rc;
        printf("%u %u %u %u %u %u\n", out[0], out[1], out[2], out[3], out[4], out[5]);
    }
    return 0;
}
"""


def cut(text, anchors, what):
    start, end = anchors
    if text.count("\n" + start) != 1 or text.count("\n" + end) != 1:
        sys.exit(f"anchor of '{what}' matches {text.count(chr(10) + start)} / {text.count(chr(10) + end)} times, not once: {anchors}")
    a = text.index("\n" + start) + 1
    b = text.index("\n" + end) + 1
    if b <= a:
        sys.exit(f"anchors of '{what}' are out of order")
    return text[a:b]


def record(checkout):
    """The output words of every row of every grid, in the order of GRIDS."""
    csrc = os.path.join(checkout, "renderer-rs_amd", "csrc")
    api = open(os.path.join(csrc, "mirhi_api.hip")).read()
    src = HARNESS.replace("@native_flags@", cut(open(os.path.join(csrc, "mirhi_native.h")).read(), NATIVE_FLAGS, "native flags"))
    for what, anchors in ANCHORS.items():
        src = src.replace("@" + what + "@", cut(api, anchors, what))
    feed = "".join(" ".join(map(str, w)) + "\n" for grid in GRIDS for w in rows_of(grid))
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "submit.cpp"), os.path.join(tmp, "submit")
        open(cpp, "w").write(src)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", csrc, "-I", os.path.join(checkout, "include"), cpp, "-o", exe])
        out = subprocess.run([exe], input=feed, capture_output=True, text=True, check=True).stdout.splitlines()
    return [[int(x) for x in line.split()] for line in out]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "submit_paths.json"))
    a = ap.parse_args()
    commit = subprocess.check_output(["git", "-C", a.checkout, "rev-parse", "HEAD"], text=True).strip()
    rows = record(a.checkout)
    # Storage, lossless and blind to what the words mean: a grid's answers (the output words it is about) are kept once each, its rows as a list of
    # pieces of PIECE consecutive answer numbers, each piece kept once.
    fixture = {"about": "tools/make_submit_paths.py: what the parent's submit_now and status_of decide: per grid, the output words of mirhi_debug_submit_path "
                        "(from word `first`) over the full product of the grid's axes, first axis slowest; row i has answers[p[i % piece]] with p = pieces[rows[i // piece]]; inputs: sha256 of the grid's input words, a row per line",
               "parent": commit, "max_batch": MAX_BATCH, "piece": PIECE, "grids": {}}
    at = 0
    for grid, (axes, _, first, count) in GRIDS.items():
        n = 1
        for _, values in axes:
            n *= len(values)
        mine, at = rows[at:at + n], at + n
        assert len(mine) == n, (grid, len(mine), n)
        answers, pieces = {}, {}
        ids = [answers.setdefault(tuple(r[first:first + count]), len(answers)) for r in mine]
        seq = [pieces.setdefault(tuple(ids[i:i + PIECE]), len(pieces)) for i in range(0, n, PIECE)]
        inputs = hashlib.sha256("".join(" ".join(map(str, w)) + "\n" for w in rows_of(grid)).encode()).hexdigest()
        fixture["grids"][grid] = {"axes": [[name, values] for name, values in axes], "first": first, "inputs": inputs, "answers": [list(x) for x in answers],
                                  "pieces": [list(x) for x in pieces], "rows": seq}
    assert at == len(rows), (at, len(rows))
    with open(a.out, "w") as f:
        json.dump(fixture, f, separators=(",", ":"))
        f.write("\n")
    print(f"{a.out}: {len(rows)} rows of {commit[:12]}, {os.path.getsize(a.out)} bytes; " +
          ", ".join(f"{g}: {len(v['answers'])} answers, {len(v['pieces'])} pieces" for g, v in fixture["grids"].items()))


if __name__ == "__main__":
    sys.exit(main())
