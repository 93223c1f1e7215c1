#!/usr/bin/env python3
"""Records what a commit's build_plan decides about a rendering scope: tests/golden/scope_plans.json.

    tools/make_scope_plans.py CHECKOUT [--out FILE]

CHECKOUT is a checkout of the commit that still decides these things inside csrc/mirhi_api.hip (the fixture names it: "parent").
RecordedPass, depth_key_setup, pass_is_masked_plain, pass_is_ordered, pass_is_depth_or_shadowed, RasterMode and raster_mode are cut
out of that file as they stand.  build_plan has no function for the body of its sizing loop, nor for the lines that fill the depth
key, the raster mode, P.shadowed / P.ibl, the own-family override and the program set: those are cut by anchor lines (ANCHORS;
every anchor must match exactly once).  The table of raster kernels is cut out of csrc/mirhi_kernels.hip for the kernel names.  The
text is compiled with g++ in a temporary directory against that checkout's headers -- the kernels are empty stubs -- and run over the
grid below with the MIRHI_* variables of each row set.  No GPU, no HIP.

The fixture is what tests/test_scope_plan_cpu.py replays through mirhi_debug_scope_plan of the library under test.

The grid.  A "scope" is a depth state with a draw mix.  Depth states: the 8 compare ops x depth test x depth write x blending x
fragment discard as a pipeline names them (128), and "no draw set the key".  Every mix with draws meets every depth state, except
those record_draw or pipeline creation refuse: a mix with a shadow map or a MODEL_PBR_IBL draw only states without blending and
discard whose key is an ordered one (depth test off, or test and write with LESS / LESS_OR_EQUAL / GREATER / GREATER_OR_EQUAL); a mix
with cascades, and the depth-only SHADOW scope, only the latter four.  "No draw set the key" is the state of the scope without draws
(and of no other: a recorded draw sets the key).  Every scope meets every value of triangles per tile (at 20 tiles), spread, wide and
every knob setting: the full product.  Held at one value where no decision of the plan can see them: allow_wide = 1 (only
raster_variant reads it: tests/golden/raster_variants.json), clear depth = 1.0 (only the depth key reads it: the "clear" grid crosses
its four values with every depth state, for a MODEL draw), pool_scale = 1 and the geometry knobs (only bin_geometry reads them: the
"bins" grid), blend factors and ops other than the enable word (copied, never looked at).
"""
import argparse
import itertools
import json
import os
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIANGLE, MODEL, MODEL_FULL, MODEL_PBR, SHADOW, MODEL_PBR_IBL = 0, 1, 2, 3, 4, 5
ORDERING = (1, 3, 4, 6)       # LESS, LESS_OR_EQUAL, GREATER, GREATER_OR_EQUAL
# a draw: [program, shadow kind (0, 1 = a single map, 2 = cascades), has a mip chain or an sRGB texture]; needs: what record_draw asks of the depth state
MIXES = [("triangle", 0, "", [[TRIANGLE, 0, 0]]),
         ("model", 0, "", [[MODEL, 0, 0]]),
         ("model_textured", 0, "", [[MODEL, 0, 1]]),
         ("model_full", 0, "", [[MODEL_FULL, 0, 0]]),
         ("triangle+model", 0, "", [[TRIANGLE, 0, 0], [MODEL, 0, 0]]),
         ("model+pbr", 0, "", [[MODEL, 0, 0], [MODEL_PBR, 0, 0]]),
         ("pbr", 0, "", [[MODEL_PBR, 0, 0]]),
         ("pbr_map", 0, "ordered key", [[MODEL_PBR, 1, 0]]),
         ("pbr_cascades", 0, "tested ordered key", [[MODEL_PBR, 2, 0]]),
         ("ibl", 0, "ordered key", [[MODEL_PBR_IBL, 0, 0]]),
         ("ibl_map", 0, "ordered key", [[MODEL_PBR_IBL, 1, 0]]),
         ("ibl_cascades", 0, "tested ordered key", [[MODEL_PBR_IBL, 2, 0]]),
         ("ibl+pbr", 0, "ordered key", [[MODEL_PBR_IBL, 0, 0], [MODEL_PBR, 0, 0]]),
         ("shadow_depth_only", 1, "tested ordered key", [[SHADOW, 0, 0]]),
         ("no_draws", 0, "no key", [])]
# [key_set, test, compare, write, discard, blend]
STATES = [[1, t, op, w, d, b] for op in range(8) for t in (0, 1) for w in (0, 1) for b in (0, 1) for d in (0, 1)] + [[0, 0, 0, 0, 0, 0]]
TRIS_PER_TILE, SPREAD, WIDE, TILES = [0, 3, 4, 15, 16, 200], [0, 1], [0, 8, 16], 20
KNOBS = [("none", {}), ("teams1", {"MIRHI_RASTER_TEAMS": "1"}), ("teams2", {"MIRHI_RASTER_TEAMS": "2"}), ("wide0", {"MIRHI_RASTER_WIDE": "0"}),
         ("wide8", {"MIRHI_RASTER_WIDE": "8"}), ("wide16", {"MIRHI_RASTER_WIDE": "16"}), ("teams2_wide8", {"MIRHI_RASTER_TEAMS": "2", "MIRHI_RASTER_WIDE": "8"}),
         ("tp_max_area0", {"MIRHI_TP_MAX_AREA": "0"}), ("tp_density1", {"MIRHI_TP_DENSITY": "1"}), ("masked_ordered", {"MIRHI_MASKED_ORDERED": "1"}),
         ("xcd_bins0", {"MIRHI_XCD_BINS": "0"}), ("xcd_run2", {"MIRHI_XCD_RUN": "2"})]
CLEAR = [0.0, 0.5, 1.0, 1.5]
BIN_TILES, BIN_TRIS, BIN_XCD, BIN_SCALE = [1, 20, 2040], [0, 1, 100, 10000, 1000000], [0, 1], [1, 2]
# per-XCD bins are an answer of raster_mode, not an input: two forced teams with the triangle-parallel path on give them, one forced team does not
BIN_XCD_ENV = [{"MIRHI_RASTER_TEAMS": "1"}, {"MIRHI_RASTER_TEAMS": "2", "MIRHI_TP_MAX_AREA": "64"}]
BIN_KNOBS = [("none", {}), ("bin_cap100", {"MIRHI_BIN_CAP": "100"}), ("bin_cap100000", {"MIRHI_BIN_CAP": "100000"}), ("fixed_pages3", {"MIRHI_FIXED_PAGES": "3"}),
             ("pool_pages5", {"MIRHI_POOL_PAGES": "5"})]
N_IN, N_OUT = 27, 32


def allowed(state, needs):
    key_set, test, op, write, discard, blend = state
    if needs == "no key" or not key_set:
        return needs == "no key" and not key_set
    if needs == "":
        return True
    ordered_key = test and write and op in ORDERING
    return not blend and not discard and (ordered_key or (needs == "ordered key" and not test))


def scopes():
    """[state index, mix index] of every scope of the grid, mix slowest."""
    return [[si, mi] for mi, (_, _, needs, _) in enumerate(MIXES) for si, st in enumerate(STATES) if allowed(st, needs)]


def words(state, mix, clear=1.0, tiles=TILES, tris=0, spread=0, wide=0, pool_scale=1, allow_wide=1):
    """The input words of mirhi_debug_scope_plan."""
    _, depth_only, _, draws = mix
    w = list(state) + [struct.unpack("<I", struct.pack("<f", clear))[0], depth_only, tiles, tris, spread, wide, pool_scale, allow_wide, len(draws)]
    for d in draws:
        w += d
    return w + [0] * (N_IN - len(w))


def all_rows():
    """(environment, input words) of every row: the main grid (knob, scope, triangles per tile, spread, wide: first slowest), then "clear", then "bins"."""
    model = MIXES[1]
    for _, env in KNOBS:
        for si, mi in scopes():
            for per_tile, spread, wide in itertools.product(TRIS_PER_TILE, SPREAD, WIDE):
                yield env, words(STATES[si], MIXES[mi], tris=per_tile * TILES, spread=spread, wide=wide)
    for st, clear in itertools.product(STATES, CLEAR):
        yield {}, words(st, model if st[0] else MIXES[-1], clear=clear, tris=200 * TILES)
    for (_, env), xcd, tiles, tris, scale in itertools.product(BIN_KNOBS, BIN_XCD, BIN_TILES, BIN_TRIS, BIN_SCALE):
        yield dict(BIN_XCD_ENV[xcd], **env), words(STATES[STATES.index([1, 1, 1, 1, 0, 0])], model, tiles=tiles, tris=tris, pool_scale=scale)


# (start of the line that begins the cut, start of the line that ends it and is not part of it)
ANCHORS = {
    "RecordedPass": ("struct RecordedPass {", "// Words of the counter block that never move"),
    "decisions": ("static void depth_key_setup(PassParams& P, const RecordedPass& pass);", "// Sizes the workspace of a recorded command buffer"),
    "Geo": ("    struct Geo { uint32_t tiles_x", "    std::vector<Geo> geo;"),
    "sizing": ("        const RasterMode mode = raster_mode(pass, tiles, cmd->ws.spread, cmd->ws.wide);", "        geo.push_back(g);"),
    "key": ("        depth_key_setup(P, pass);", "        memcpy(P.clear_color, pass.info.clear_color"),
    "mode": ("        {\n            // (evaluated again, not kept from the sizing loop above", "        P.vs_jobs = dev_jobs + jobs_done;"),
    "programs": ("        uint32_t progs = 0;         // the scope's program set", "        cmd->plan_tris += "),
}
KERNEL_TABLE = ("struct RasterEntry {", "hipError_t launch_raster(")

HARNESS = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "mirhi.h"
#include "mirhi_device.h"
#include "mirhi_variant.h"
using namespace mirhi;
@RecordedPass@
@decisions@
struct Workspace { uint32_t pool_scale; bool spread; uint32_t wide; TriRec* ordered; };
struct Cmd { Workspace ws; std::vector<uint32_t> plan_programs; };
@Geo@
static size_t sizing(Cmd* cmd, RecordedPass& pass, Geo& g, size_t tiles) {
@sizing@
    return pages;
}
static void fill(Cmd* cmd, RecordedPass& pass, const Geo& g, PassParams& P, size_t max_tiles, bool& any_wide_eligible) {
    Workspace& w = cmd->ws;
    std::vector<DrawDesc>& draws = pass.draws;
@key@
@mode@
@programs@
}
template <int P> void ordered_kernel(const PassParams*, const RasterHead) {}
template <int K, int T> void raster_kernel_depth(const PassParams*, const RasterHead) {}
template <int K, int T> void raster_kernel_shadow(const PassParams*, const RasterHead) {}
template <int K, int T> void raster_kernel_csm(const PassParams*, const RasterHead) {}
template <int K, int T, int S> void raster_kernel_ibl(const PassParams*, const RasterHead) {}
template <int P, int K, int W> void raster_kernel_wide(const PassParams*, const RasterHead) {}
template <int P, int K, int T, int TEAMS = 1, bool M = false> void raster_kernel(const PassParams*, const RasterHead) {}
@kernel_table@
// stdin: one row per line: "NAME=VALUE,..." (or "-"), then the input words of mirhi_debug_scope_plan; stdout: its output words, then the kernel name
int main() {
    static float some_map; static TriRec some_recs;
    char env[256]; unsigned in[27];
    std::vector<std::string> set;
    while (scanf("%255s", env) == 1) {
        for (unsigned& v : in) if (scanf("%u", &v) != 1) return 2;
        for (const std::string& name : set) unsetenv(name.c_str());
        set.clear();
        for (char* tok = strtok(env, ","); tok && strcmp(tok, "-") != 0; tok = strtok(nullptr, ",")) {
            char* eq = strchr(tok, '='); *eq = 0;
            setenv(tok, eq + 1, 1); set.push_back(tok);
        }
        RecordedPass pass;
        pass.key_set = in[0] != 0u; pass.depth_test = in[1]; pass.depth_compare = in[2]; pass.depth_write = in[3]; pass.frag_discard = in[4]; pass.blend[0] = in[5];
        memcpy(&pass.info.clear_depth, &in[6], 4);
        pass.depth_only = in[7] != 0u;
        pass.total_tris = in[9];
        for (unsigned i = 0; i < in[14]; i++) {
            DrawDesc d;
            memset(&d, 0, sizeof d);
            d.program = in[15 + 3 * i];
            if (in[16 + 3 * i]) { d.shadow_map = &some_map; d.shadow_layers = in[16 + 3 * i] == 2u ? 4u : 0u; }
            d.tex_any_mips = in[17 + 3 * i];
            pass.draws.push_back(d);
        }
        Cmd cmd; cmd.ws = Workspace{in[12], in[10] != 0u, in[11], &some_recs};
        Geo g;
        g.tiles_x = in[8]; g.tiles_y = 1; g.r0 = 0; g.r1 = 1; g.rstep = 1;       // (tiles = tiles_x * (r1 - r0))
        const size_t pages = sizing(&cmd, pass, g, in[8]);
        PassParams P;
        memset(&P, 0, sizeof P);
        bool wide_eligible = false;
        fill(&cmd, pass, g, P, in[8], wide_eligible);
        const unsigned programs = cmd.plan_programs.at(0);
        const bool ordered = pass_is_ordered(pass), masked = pass_is_masked_plain(pass), own = pass_is_depth_or_shadowed(pass);
        PassParams K{};        // the key as depth_key_setup leaves it (an ordered scope's parameters hold idflip = pred = 0)
        depth_key_setup(K, pass);
        if (ordered != (P.ordered_recs != nullptr) || masked != (P.alpha_scope != 0u) || own != (P.depth_only || P.shadowed || P.ibl)) return 3;
        P.tiles_x = 5; P.tile_row_begin = 0; P.tile_row_end = 4; P.tile_row_step = 1;
        const RasterVariant v = raster_variant(P, programs, in[13] != 0u);
        const RasterEntry* e = raster_entry(v);
        if (!e) return 4;
        printf("%u %u %u %u %u %u %u %u  %u %u %u %u %u %u %u  %u %u %u %u %u %u  %u %u %u %u %u %u %u  %u %u %u %u %s\n",
               K.clear_depth_bits, K.pred, K.zflip, K.zmask, K.idflip, K.strict, K.init_zk, K.init_idk,
               (unsigned)ordered, (unsigned)masked, (unsigned)g.tri_prog, P.shadowed, P.ibl, (unsigned)own, programs,
               P.tp_max_area, P.raster_teams, (unsigned)wide_eligible, (unsigned)g.xcd_bins, P.raster_wide, P.xcd_swizzle,
               g.bin_cap, g.sub_cap, g.fixed_per_tile, g.fixed_pages, (unsigned)pages, (unsigned)((unsigned long long)pages >> 32), g.big_cap,
               v.grid[0], v.grid[1], v.grid[2], v.block, e->name);
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
    """[output words..., kernel name] of every row of all_rows()."""
    csrc = os.path.join(checkout, "renderer-rs_amd", "csrc")
    api = open(os.path.join(csrc, "mirhi_api.hip")).read()
    src = HARNESS.replace("@kernel_table@", cut(open(os.path.join(csrc, "mirhi_kernels.hip")).read(), KERNEL_TABLE, "kernel table"))
    for what, anchors in ANCHORS.items():
        src = src.replace("@" + what + "@", cut(api, anchors, what))
    feed = "".join((",".join(f"{k}={v}" for k, v in env.items()) or "-") + " " + " ".join(map(str, w)) + "\n" for env, w in all_rows())
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "scope.cpp"), os.path.join(tmp, "scope")
        open(cpp, "w").write(src)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", csrc, "-I", os.path.join(checkout, "include"), cpp, "-o", exe])
        env = {k: v for k, v in os.environ.items() if not k.startswith("MIRHI_")}
        out = subprocess.run([exe], input=feed, capture_output=True, text=True, check=True, env=env).stdout.splitlines()
    rows = []
    for line in out:
        parts = line.split(None, N_OUT)
        rows.append([int(x) for x in parts[:N_OUT]] + [parts[N_OUT]])
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "scope_plans.json"))
    a = ap.parse_args()
    commit = subprocess.check_output(["git", "-C", a.checkout, "rev-parse", "HEAD"], text=True).strip()
    rows = record(a.checkout)
    sc = scopes()
    inner = len(TRIS_PER_TILE) * len(SPREAD) * len(WIDE)
    n_main, n_clear = len(KNOBS) * len(sc) * inner, len(STATES) * len(CLEAR)
    n_bins = len(BIN_KNOBS) * len(BIN_XCD) * len(BIN_TILES) * len(BIN_TRIS) * len(BIN_SCALE)
    assert len(rows) == n_main + n_clear + n_bins, (len(rows), n_main, n_clear, n_bins)
    # Storage, lossless and blind to what the words mean.  An answer is split by position into its scope part (key and class: the first 15 words) and
    # its plan part, a pair of raster part (mode, grid, block, kernel) and bins part (the seven words in between), each kept once.  A scope's scope part does not change over its inner axes (checked here, not
    # assumed); its plan parts over them are a pattern, kept once; a knob setting is one vector of scope parts and one of patterns, kept once.
    # Patterns and vectors are written as lists of pieces (6 and 8 consecutive entries), each piece kept once.
    SPLIT = 15
    scope_parts, raster_parts, bins_parts, plan_parts, patterns, vectors = {}, {}, {}, {}, {}, {}

    def plan_part(r):
        pair = (raster_parts.setdefault(tuple(r[15:21] + r[28:]), len(raster_parts)), bins_parts.setdefault(tuple(r[21:28]), len(bins_parts)))
        return plan_parts.setdefault(pair, len(plan_parts))

    def in_pieces(lists, n):
        pieces = {}
        return [[pieces.setdefault(tuple(v[i:i + n]), len(pieces)) for i in range(0, len(v), n)] for v in lists], [list(p) for p in pieces]
    ids = [(scope_parts.setdefault(tuple(r[:SPLIT]), len(scope_parts)), plan_part(r)) for r in rows]
    main_rows = {}
    for ki, (kname, _) in enumerate(KNOBS):
        base = ki * len(sc) * inner
        per_scope = [ids[base + i * inner:base + (i + 1) * inner] for i in range(len(sc))]
        if any(len({s for s, _ in chunk}) != 1 for chunk in per_scope):
            sys.exit("a scope's key or class changes with triangles per tile, spread or wide: this storage cannot hold that")
        main_rows[kname] = [vectors.setdefault(tuple(chunk[0][0] for chunk in per_scope), len(vectors)),
                            vectors.setdefault(tuple(patterns.setdefault(tuple(p for _, p in chunk), len(patterns)) for chunk in per_scope), len(vectors))]
    for i, (_, xcd, *_) in enumerate(itertools.product(BIN_KNOBS, BIN_XCD, BIN_TILES, BIN_TRIS, BIN_SCALE)):
        assert rows[n_main + n_clear + i][18] == xcd, "the bins grid did not get the per-XCD bins it asked for"
    patterns_out, pattern_pieces = in_pieces(patterns, 6)
    vectors_out, vector_pieces = in_pieces(vectors, 8)
    fixture = {
        "about": "tools/make_scope_plans.py: what the parent's build_plan decides for a scope: the output words of mirhi_debug_scope_plan and the kernel name, "
                 "split into scope part (the first 15 words) and plan part.  main[knob] = [vector of scope parts, vector of patterns], one entry per scope "
                 "(mixes slowest, then the states the mix may meet); a pattern is a scope's plan parts over (triangles per tile, spread, wide), first slowest; "
                 "patterns and vectors are lists of pieces (pattern_pieces, vector_pieces) to be joined",
        "parent": commit,
        "states": STATES, "mixes": [[n, d, needs, draws] for n, d, needs, draws in MIXES],
        "tris_per_tile": TRIS_PER_TILE, "spread": SPREAD, "wide": WIDE, "tiles": TILES, "knobs": KNOBS,
        "scope_parts": [list(o) for o in scope_parts], "raster_parts": [list(o) for o in raster_parts], "bins_parts": [list(o) for o in bins_parts],
        "plan_parts": [list(o) for o in plan_parts], "patterns": patterns_out, "pattern_pieces": pattern_pieces,
        "vectors": vectors_out, "vector_pieces": vector_pieces, "main": main_rows,
        "clear": {"values": CLEAR, "answers": ids[n_main:n_main + n_clear]},          # (state, clear value), state slowest
        "bins": {"knobs": BIN_KNOBS, "xcd_bins": BIN_XCD, "xcd_bins_env": BIN_XCD_ENV, "tiles": BIN_TILES, "tris": BIN_TRIS, "pool_scale": BIN_SCALE,
                 "answers": ids[n_main + n_clear:]},
    }
    with open(a.out, "w") as f:
        json.dump(fixture, f, separators=(",", ":"))
        f.write("\n")
    print(f"{a.out}: {len(rows)} rows of {commit[:12]} ({len(sc)} scopes), {len(scope_parts)} scope parts, {len(plan_parts)} plan parts, {len(patterns)} patterns, "
          f"{len(vectors)} vectors, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    sys.exit(main())
