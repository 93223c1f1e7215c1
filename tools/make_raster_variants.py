#!/usr/bin/env python3
"""Records which raster kernel, grid and block a commit's launchers choose: tests/golden/raster_variants.json.

    tools/make_raster_variants.py CHECKOUT [--out FILE]

CHECKOUT is a checkout of the commit that still has the hand-written launch ladder (the fixture names it: "parent").  Its
launch_raster_k, launch_raster, raster_variant_key, launch_raster_batch_k, launch_raster_batch and raster_batchable are cut
out of csrc/mirhi_kernels.hip as they stand and compiled with g++ in a temporary directory, against that checkout's
mirhi_device.h.  MIRHI_LAUNCH is redefined to record instead of launching; the kernels are stubs that name themselves with
every template argument spelled out (the macro's #kernel would still hold KEYED, TP and TEAMS as words).  No GPU, no HIP.

The fixture is what tests/test_raster_variants_cpu.py replays through mirhi_debug_raster_choice of the library under test.
A row is its index in the product of AXES (first axis slowest); rows are grouped under "<kernel> grid X Y Z block B".
"""
import argparse
import collections
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = [("programs", [0, 1, 2, 3, 4, 7, 12, 28]),
        ("key_state", ["plain", "flipped", "predicate"]),      # (zflip, zmask, pred): KEY_STATES
        ("tp_max_area", [0, 64]),
        ("raster_teams", [1, 2]),
        ("raster_wide", [0, 8, 16]),
        ("alpha_scope", [0, 1]),
        ("xcd_swizzle", [1, 2]),
        ("ordered", [0, 1]),
        ("allow_wide", [0, 1])]                                  # last: rows 2k and 2k + 1 differ in allow_wide alone
KEY_STATES = {"plain": (0, 0xFFFFFFFF, 0), "flipped": (0xFFFFFFFF, 0xFFFFFFFF, 0), "predicate": (0, 0xFFFFFFFF, 5)}
NOT_BATCHABLE = "not batchable"


def rows():
    """Every row of the grid as the twelve words of mirhi_debug_raster_choice, n_batch left 0."""
    for programs, ks, tp, teams, wide, alpha, swz, ordered, allow in itertools.product(*(v for _, v in AXES)):
        zflip, zmask, pred = KEY_STATES[ks]
        yield [programs, allow, pred, zflip, zmask, tp, teams, wide, alpha, swz, ordered, 0]


HARNESS_HEAD = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "mirhi_device.h"
struct dim3 { uint32_t x, y, z; dim3(uint32_t x_ = 1, uint32_t y_ = 1, uint32_t z_ = 1) : x(x_), y(y_), z(z_) {} };
typedef int hipError_t; typedef void* hipStream_t; typedef void* hipEvent_t;
constexpr hipError_t hipSuccess = 0;
namespace mirhi {
struct LaunchTiming { hipEvent_t start = nullptr, stop = nullptr; };
static std::string g_name; static dim3 g_grid, g_block; static int g_launches;
static hipError_t launch_result() { return hipSuccess; }
static void named(const char* fmt, int a = 0, int b = 0, int c = 0, int d = 0, const char* e = "") { char s[96]; snprintf(s, sizeof s, fmt, a, b, c, d, e); g_name = s; }
template <int PROGS, int KEYED, int TP, int TEAMS = 1, bool MASKEDV = false> void raster_kernel(const PassParams*, const RasterHead) { named("raster_kernel<%d, %d, %d, %d, %s>", PROGS, KEYED, TP, TEAMS, MASKEDV ? "true" : "false"); }
template <int PROGS, int KEYED, int WPT> void raster_kernel_wide(const PassParams*, const RasterHead) { named("raster_kernel_wide<%d, %d, %d>", PROGS, KEYED, WPT); }
template <int KEYED, int TP> void raster_kernel_depth(const PassParams*, const RasterHead) { named("raster_kernel_depth<%d, %d>", KEYED, TP); }
template <int KEYED, int TP> void raster_kernel_shadow(const PassParams*, const RasterHead) { named("raster_kernel_shadow<%d, %d>", KEYED, TP); }
template <int KEYED, int TP> void raster_kernel_csm(const PassParams*, const RasterHead) { named("raster_kernel_csm<%d, %d>", KEYED, TP); }
template <int PROGS> void ordered_kernel(const PassParams*, const RasterHead) { named("ordered_kernel<%d>", PROGS); }
template <int PROGS, int KEYED, int TP, int TEAMS = 1> void raster_kernel_batch(const RasterBatch) { named("raster_kernel_batch<%d, %d, %d, %d>", PROGS, KEYED, TP, TEAMS); }
#define MIRHI_LAUNCH(kernel, grid, block, stream, t, ...) do { kernel(__VA_ARGS__); g_grid = grid; g_block = block; g_launches++; (void)stream; (void)t; } while (0)
"""

HARNESS_TAIL = r"""
}  // namespace mirhi
using namespace mirhi;
// stdin: one row per line (the twelve words of mirhi_debug_raster_choice); stdout: name | gx gy gz bx | key
int main() {
    static TriRec some_recs;
    unsigned in[12];
    while (scanf("%u %u %u %u %u %u %u %u %u %u %u %u", &in[0], &in[1], &in[2], &in[3], &in[4], &in[5], &in[6], &in[7], &in[8], &in[9], &in[10], &in[11]) == 12) {
        PassParams P;
        memset(&P, 0, sizeof P);
        P.tiles_x = 5; P.tile_row_begin = 0; P.tile_row_end = 4; P.tile_row_step = 1;
        P.pred = in[2]; P.zflip = in[3]; P.zmask = in[4]; P.tp_max_area = in[5]; P.raster_teams = in[6]; P.raster_wide = in[7]; P.alpha_scope = in[8]; P.xcd_swizzle = in[9];
        P.ordered_recs = in[10] ? &some_recs : nullptr;
        // what build_plan derives the program word from
        P.depth_only = in[0] == 0u ? 1u : 0u;
        P.shadowed = (in[0] & 8u) ? ((in[0] & 16u) ? 2u : 1u) : 0u;
        g_launches = 0; g_name = "";
        if (in[11] >= 2u) {
            if (!raster_batchable(P)) g_name = "NOT_BATCHABLE";
            else {
                const PassParams* Ps[MAX_BATCH] = {}; const PassParams* dp[MAX_BATCH] = {}; uint32_t* big[MAX_BATCH] = {};
                for (unsigned i = 0; i < in[11]; i++) Ps[i] = &P;
                launch_raster_batch(Ps, dp, big, in[11], in[0], nullptr, nullptr);
            }
        } else launch_raster(P, nullptr, nullptr, in[0], nullptr, LaunchTiming{}, in[1] != 0u);
        if (g_launches != (g_name == "NOT_BATCHABLE" ? 0 : 1)) { fprintf(stderr, "row launched %d kernels\n", g_launches); return 1; }
        printf("%s|%u %u %u %u|%llu\n", g_name.c_str(), g_grid.x, g_grid.y, g_grid.z, g_block.x, (unsigned long long)raster_variant_key(P, in[0]));
    }
    return 0;
}
"""


def cut(text, start, end):
    """The lines of `text` from the one that begins with `start` up to (not including) the one that begins with `end`."""
    a = text.index("\n" + start) + 1
    return text[a:text.index("\n" + end, a) + 1]


def record(checkout, n_batch):
    csrc = os.path.join(checkout, "renderer-rs_amd", "csrc")
    src = open(os.path.join(csrc, "mirhi_kernels.hip")).read()
    ladder = "template <int KEYED, int TP, int TEAMS = 1>\nstatic void "
    body = (cut(src, ladder + "launch_raster_k", "hipError_t launch_vertex_batch") +       # launch_raster_k, launch_raster, raster_variant_key
            cut(src, ladder + "launch_raster_batch_k", "hipError_t launch_fragment_count"))   # launch_raster_batch_k, launch_raster_batch, raster_batchable
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "ladder.cpp"), os.path.join(tmp, "ladder")
        open(cpp, "w").write(HARNESS_HEAD + body + HARNESS_TAIL.replace("NOT_BATCHABLE", NOT_BATCHABLE))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", csrc, cpp, "-o", exe])
        feed = "".join(" ".join(str(w) for w in r[:11] + [n_batch]) + "\n" for r in rows())
        out = subprocess.run([exe], input=feed, capture_output=True, text=True, check=True).stdout.splitlines()
    result = []
    for line in out:
        name, shape, key = line.split("|")
        gx, gy, gz, bx = shape.split()
        result.append((name if name == NOT_BATCHABLE else f"{name} grid {gx} {gy} {gz} block {bx}", int(key)))
    return result


def grouped(pairs):
    g = collections.OrderedDict()
    for i, k in pairs:
        g.setdefault(k, []).append(i)
    return g


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "raster_variants.json"))
    a = ap.parse_args()
    commit = subprocess.check_output(["git", "-C", a.checkout, "rev-parse", "HEAD"], text=True).strip()
    single, batched = record(a.checkout, 0), record(a.checkout, 2)
    n = len(single)
    assert n == len(batched) == 4608
    # the ladder does not look at allow_wide when it batches, and its key never does
    for i in range(0, n, 2):
        assert batched[i] == batched[i + 1], (i, batched[i], batched[i + 1])
        assert single[i][1] == single[i + 1][1] == batched[i][1]
    fixture = {
        "about": "tools/make_raster_variants.py: the kernel, grid and block the parent's launch_raster / launch_raster_batch choose for a scope of 5 x 4 tiles; "
                 "a row is its index in the product of the axes, first axis slowest",
        "parent": commit,
        "axes": AXES,
        "key_states": {k: {"zflip": v[0], "zmask": v[1], "pred": v[2]} for k, v in KEY_STATES.items()},
        "single": grouped((i, s[0]) for i, s in enumerate(single)),
        "batched": grouped((i, b[0]) for i, b in enumerate(batched)),                       # n_batch = 2
        "parent_keys": grouped((i, str(s[1])) for i, s in enumerate(single) if i % 2 == 0),   # raster_variant_key of rows 2k and 2k + 1
    }
    with open(a.out, "w") as f:
        json.dump(fixture, f, separators=(",", ":"))
        f.write("\n")
    print(f"{a.out}: {n} single + {n} batched rows of {commit[:12]}, {len(fixture['single'])} + {len(fixture['batched'])} groups, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    sys.exit(main())
