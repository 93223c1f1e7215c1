"""4x MSAA without a GPU (include/mirhi.h "4x MSAA"): the condition the GPU tests' yardstick rests on, for every case; the float64 model against
closed forms and against the unchanged oracle; the names through every binding; the selector; the refusal texts that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import msaa_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("mirhi_image_create_multisampled", "mirhi_image_samples", "mirhi_resolve_info_default", "mirhi_cmd_begin_rendering_resolve")


@pytest.fixture(scope="module")
def all_cases(scenes):
    return mc.cases(scenes)


# ---- the condition, and the oracle alone ---------------------------------------------------------------------------------------------------
def test_every_vertex_of_every_case_meets_the_condition(scenes, all_cases):
    assert len(all_cases) >= 14
    for name, scene in all_cases.items():
        for sc in (scene, mc.oracle_scene(scenes, name, scene)):
            checked, failed = mc.condition_holds(scenes, sc)
            assert checked >= sum(d.count for d in sc.draws) and failed == 0, (name, checked, failed)


def test_the_condition_can_fail(scenes):
    """the check is no tautology: off the 1/256 grid, a vertex just below window x = 128 moves into the next binade under a moved viewport, where binary32 keeps
    one bit less -- some of them then snap elsewhere"""
    failed = 0
    for j in range(3000):
        scene = mc._scene(scenes, "off-grid", 256, 256, mc.draw(scenes, [(127.9 + j * 2.0 ** -17, 10.0, 0.5), (30.0, 20.0, 0.5), (10.0, 30.0, 0.5)]))
        failed += mc.condition_holds(scenes, scene)[1]
    assert failed > 0


def test_oracle_alone_satisfies_the_equivalence(scenes, oracle, all_cases):
    """the four moved-viewport oracle frames ARE the four samples: winners equal the float64 model's per-sample winners at every texel, depths agree (bit for bit
    where the depth plane is dyadic, to binary32 rounding elsewhere) -- shown without the code under test"""
    for name, scene in all_cases.items():
        if name == "near-clip":       # (the model knows no clipping: the case's yardstick is the oracle itself)
            continue
        sc = mc.oracle_scene(scenes, name, scene)
        prim, depth, _ = mc.oracle_samples(scenes, oracle, sc)
        model = scenes.msaa_model(sc)
        assert np.array_equal(model["prim"], prim), name
        err = float(np.abs(model["depth"] - depth).max())
        assert err < 1.2e-5, (name, err)
        if name in ("slivers", "sample-edges", "tile-corner", "big-list", "biased-clamped"):      # flat or dyadic planes
            assert err == 0.0, (name, err)


def test_slivers_show_nothing_at_1x(scenes, oracle, all_cases):
    prim, _, one = mc.oracle_samples(scenes, oracle, all_cases["slivers"])
    assert (one["prim"] == mc.NONE).all()
    covered = (prim != mc.NONE)
    assert covered.sum(axis=2).max() == 1 and all(covered[:, :, s].sum() > 50 for s in range(4))      # exactly one sample of a pixel, every sample somewhere


# ---- the model against closed forms ---------------------------------------------------------------------------------------------------------
def test_vertical_edge_at_half_a_pixel_takes_two_samples_of_four(scenes):
    col = [[0.25, 0.5, 0.75]] * 3
    scene = mc._scene(scenes, "edge", 64, 64, mc.draw(scenes, [(10.5, -50.0, 0.5), (10.5, 200.0, 0.5), (300.0, 80.0, 0.5)], col), clear_color=(0.0, 0.0, 0.0, 1.0))
    m = scenes.msaa_model(scene)
    assert list(m["prim"][20, 10] != scenes.NO_PRIM) == [False, True, False, True]       # x = 0.875 and 0.625 lie right of the edge
    assert np.array_equal(m["color"][20, 10], np.array([0.125, 0.25, 0.375, 1.0]))       # ((0 + c) + (0 + c)) / 4
    assert (m["prim"][20, 9] == scenes.NO_PRIM).all() and (m["prim"][20, 11] == 0).all()
    # a pixel inside a triangle gives the triangle's colour bit for bit: (c + c) + (c + c) times 1/4 is c, in binary32 too
    c = np.array([0.3, 0.7, 0.1, 1.0], dtype=np.float32)
    assert np.array_equal(scenes.msaa_resolve(c, c, c, c, np.float32).view(np.uint32), c.view(np.uint32))
    assert np.array_equal(m["color"][20, 11], np.array([0.25, 0.5, 0.75, 1.0]))


def test_resolve_order_is_the_stated_one(scenes):
    """((c0 + c1) + (c2 + c3)) * 0.25 with every operation rounded to binary32: on these inputs a left-to-right sum gives other bits"""
    c = [np.float32(v) for v in (1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24)]
    want = np.float32(np.float32(np.float32(c[0] + c[1]) + np.float32(c[2] + c[3])) * np.float32(0.25))
    other = np.float32(np.float32(np.float32(np.float32(c[0] + c[1]) + c[2]) + c[3]) * np.float32(0.25))
    assert scenes.msaa_resolve(*c, dtype=np.float32) == want and want != other


def test_sample_positions_are_vulkans(scenes):
    assert scenes.MSAA_SAMPLES == ((0.375, 0.125), (0.875, 0.375), (0.125, 0.625), (0.625, 0.875))
    assert tuple((int(x * 256), int(y * 256)) for x, y in scenes.MSAA_SAMPLES) == mc.SAMPLES_256
    # (the kernel's closed form of the table, msaa_sample_x / msaa_sample_y: the GPU visibility tests are what pins the kernel to it)
    assert [(96 + 128 * (s & 1) - 64 * (s >> 1), 32 + 64 * s) for s in range(4)] == list(mc.SAMPLES_256)


def test_sample_scene_moves_viewports_and_keeps_scissors(scenes, all_cases):
    sc = all_cases["scissor"]
    for s, (sx, sy) in enumerate(scenes.MSAA_SAMPLES):
        moved = scenes.msaa_sample_scene(sc, s)
        assert moved.draws[0].viewport == (0.5 - sx, 0.5 - sy, 256.0, 256.0, 0.0, 1.0) and moved.draws[0].scissor == sc.draws[0].scissor


# ---- names through every binding ------------------------------------------------------------------------------------------------------------
def test_header_abi_and_names(mirhi):
    header = open(os.path.join(ROOT, "include", "mirhi.h")).read()
    assert "#define MIRHI_ABI_VERSION 5u" in header and mirhi.ABI_VERSION == 5
    assert "MIRHI_RESOLVE_NONE = 0, MIRHI_RESOLVE_SAMPLE_ZERO = 1, MIRHI_RESOLVE_AVERAGE = 2" in header
    lib = mirhi.lib()
    for fn in NEW_FUNCTIONS:
        assert re.search(r"\b%s\(" % fn, header), fn
        assert hasattr(lib, fn), fn
    assert lib.mirhi_image_samples(None) == 0
    r = mirhi.ResolveInfo(1, 2, 3, 1)
    lib.mirhi_resolve_info_default(C.byref(r))
    assert (r.color_resolve_image, r.color_resolve_mode, r.depth_resolve_image, r.depth_resolve_mode) == (None, 0, None, 0)
    assert C.sizeof(mirhi.ResolveInfo) == 32
    for phrase in ("(0.375, 0.125)", "((c0 + c1) + (c2 + c3)) * 0.25f", "multisampled attachments are transient", "4 * width x height", "pixel centre"):
        assert phrase in header, phrase


def test_python_names(mirhi):
    assert (mirhi.ResolveMode.NONE, mirhi.ResolveMode.SAMPLE_ZERO, mirhi.ResolveMode.AVERAGE) == (0, 1, 2)
    b = mirhi.GraphicsPipelineBuilder()
    assert b.desc.rasterization_samples == 1 and b.rasterization_samples(4) is b and b.desc.rasterization_samples == 4
    assert callable(mirhi.Image.multisampled) and hasattr(mirhi.CommandBuffer, "begin_rendering_resolve") and hasattr(mirhi.CommandBuffer, "begin_rendering_attachments")

    class Img:       # (no device: the attachment classes only carry handles)
        def __init__(self, h):
            self.handle = h
    ms, one, msd, oned = Img(11), Img(12), Img(13), Img(14)
    ca = mirhi.ColorAttachment(ms, clear_color=(0.5, 0.25, 0.125, 1.0)).with_resolve(one)
    da = mirhi.DepthAttachment(msd, clear_depth=0.5).with_resolve(oned)
    info, res = mirhi.attachment_infos(ca, da)
    assert (info.color_image, info.depth_image, res.color_resolve_image, res.depth_resolve_image) == (11, 13, 12, 14)
    assert (res.color_resolve_mode, res.depth_resolve_mode) == (mirhi.ResolveMode.AVERAGE, mirhi.ResolveMode.SAMPLE_ZERO)
    assert info.color_store_op == mirhi.StoreOp.DONT_CARE and info.color_load_op == mirhi.LoadOp.CLEAR and info.clear_depth == 0.5
    info, res = mirhi.attachment_infos(mirhi.ColorAttachment(one))
    assert (res.color_resolve_image, res.color_resolve_mode, res.depth_resolve_mode) == (None, 0, 0) and info.color_store_op == mirhi.StoreOp.STORE


def test_cpp_names(tmp_path):
    hpp = open(os.path.join(ROOT, "renderer-rs_amd", "host", "mirhi.hpp")).read()
    for name in ("static Image multisampled(", "rasterization_samples(uint32_t samples)", "ColorAttachment& with_resolve(", "DepthAttachment& with_resolve(",
                 "mirhi_cmd_begin_rendering_resolve(h_, &cfg.build(), &cfg.resolve())"):
        assert name in hpp, name
    src = tmp_path / "msaa_names.cpp"
    src.write_text('#include "mirhi.hpp"\n#include <cstdio>\n'
                   'int main() { mirhi::RenderingConfig cfg(64, 64); const mirhi_resolve_info& r = cfg.resolve();\n'
                   '  mirhi::GraphicsPipelineBuilder b; b.rasterization_samples(4);\n'
                   '  std::printf("%d %d %d %d\\n", r.color_resolve_image == nullptr, r.color_resolve_mode, r.depth_resolve_mode, (int)mirhi::ResolveMode::Average); return 0; }\n')
    pkg = os.path.join(ROOT, "renderer-rs_amd")
    exe = tmp_path / "msaa_names"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", "-I", os.path.join(pkg, "host"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", pkg, "-lmirhi", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.check_output([str(exe)]).decode().split() == ["1", "0", "0", "2"]


def test_rust_coverage():
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "mirhi-sys", "src", "lib.rs")).read()
    for fn in NEW_FUNCTIONS:
        assert re.search(r"pub fn %s\(" % fn, sys_rs), fn
    assert "pub struct mirhi_resolve_info" in sys_rs and "pub const MIRHI_RESOLVE_AVERAGE: mirhi_resolve_mode = 2;" in sys_rs
    wrap = lambda f: open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", f)).read()
    assert "pub fn rasterization_samples(mut self, samples: u32) -> Self" in wrap("pipeline.rs")
    assert "pub fn new_multisampled(" in wrap("image.rs") and "pub fn samples(&self) -> u32" in wrap("image.rs")
    cmd = wrap("command.rs")
    assert "pub fn with_resolve(mut self, target: &'a Image) -> Self" in cmd and "pub fn with_depth_resolve(mut self, target: &'a Image) -> Self" in cmd
    assert "mirhi_sys::mirhi_cmd_begin_rendering_resolve(self.raw, &ri, &res)" in cmd
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("mirhi_cmd_begin_rendering_resolve", "mirhi_image_create_multisampled", "with_resolve", "rasterization_samples"):
        assert name in integ, name


# ---- the selector ---------------------------------------------------------------------------------------------------------------------------
def _msaa(mirhi, words):
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_msaa
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32]
    words = [int(w) & 0xFFFFFFFF for w in words]
    inp, msg = (C.c_uint32 * 48)(*(words + [0] * (48 - len(words)))), C.create_string_buffer(256)
    rc = fn(inp, msg, len(msg))
    return rc, msg.value.decode()


def test_selector_picks_the_msaa_family(mirhi):
    text = open(os.path.join(ROOT, "renderer-rs_amd", "csrc", "mirhi_variant.h")).read()
    assert re.search(r"RASTER_CSM_BLEND, RASTER_MSAA \};", text)          # behind RASTER_CSM_BLEND: the recorded values stay
    for programs, progs in ((1, 1), (2, 2), (3, 3), (4, 4)):
        for zflip, keyed in ((0, 0), (0xFFFFFFFF, 1)):
            rc, msg = _msaa(mirhi, [3, programs, zflip, 0xFFFFFFFF, 4])
            assert rc == 0 and msg == f"msaa family 10 progs {progs} keyed {keyed} tp 0 grid 5 4 block 256 batched 0", msg
            rc, msg = _msaa(mirhi, [3, programs, zflip, 0xFFFFFFFF, 0])
            assert rc == 0 and msg.startswith("other family 0 "), msg


# ---- refusals that need no device -----------------------------------------------------------------------------------------------------------
def test_sample_count_refusals(mirhi):
    assert _msaa(mirhi, [0, 4]) == (0, "")
    rc, msg = _msaa(mirhi, [0, 1])
    assert rc == 1 and "use mirhi_image_create" in msg
    for n in (0, 2, 8, 16, 3):
        rc, msg = _msaa(mirhi, [0, n])
        assert rc == 1 and "unsupported: sample count" in msg, n


# the words of MsaaScopeFacts, in order (mirhi_scope.h)
FACTS = ["color_samples", "color_format", "color_w", "color_h", "color_load_op", "color_store_op", "has_depth", "depth_samples", "depth_format", "depth_w", "depth_h",
         "depth_load_op", "depth_store_op", "has_color_resolve", "cr_samples", "cr_format", "cr_w", "cr_h", "cr_same_device", "color_resolve_mode",
         "has_depth_resolve", "dr_samples", "dr_format", "dr_w", "dr_h", "dr_same_device", "depth_resolve_mode", "has_prim", "prim_format", "prim_w", "prim_h",
         "area_partial", "split_device", "fragment_stats"]
GOOD = dict(color_samples=4, color_format=2, color_w=96, color_h=80, color_load_op=1, color_store_op=1, has_depth=1, depth_samples=4, depth_format=3, depth_w=96, depth_h=80,
            depth_load_op=1, depth_store_op=1, has_color_resolve=1, cr_samples=1, cr_format=2, cr_w=96, cr_h=80, cr_same_device=1, color_resolve_mode=2,
            has_depth_resolve=1, dr_samples=1, dr_format=3, dr_w=96, dr_h=80, dr_same_device=1, depth_resolve_mode=1, has_prim=1, prim_format=5, prim_w=384, prim_h=80,
            area_partial=0, split_device=0, fragment_stats=0)


def _scope(mirhi, **change):
    f = dict(GOOD, **change)
    return _msaa(mirhi, [1] + [f[k] for k in FACTS])


def test_scope_refusals(mirhi):
    text = open(os.path.join(ROOT, "renderer-rs_amd", "csrc", "mirhi_scope.h")).read()
    decl = text[text.index("struct MsaaScopeFacts {"):text.index("};", text.index("struct MsaaScopeFacts {"))]
    assert re.findall(r"\b([a-z_]+)[,;]", decl) == FACTS       # the test's word order is the struct's
    assert _scope(mirhi) == (0, "")
    assert _scope(mirhi, has_depth=0, has_depth_resolve=0, depth_resolve_mode=0, has_prim=0) == (0, "")
    for change, phrase in ((dict(color_load_op=0), "unsupported: multisampled attachments are transient"),
                           (dict(color_store_op=0), "unsupported: multisampled attachments are transient"),
                           (dict(depth_load_op=0), "unsupported: multisampled attachments are transient"),
                           (dict(depth_store_op=0), "unsupported: multisampled attachments are transient"),
                           (dict(has_color_resolve=0), "needs a color_resolve_image"), (dict(color_resolve_mode=1), "MIRHI_RESOLVE_AVERAGE"),
                           (dict(cr_samples=4), "multisampled itself"), (dict(cr_format=1), "format and extent"), (dict(cr_w=95), "format and extent"),
                           (dict(cr_same_device=0), "another device"), (dict(depth_samples=1), "single-sampled depth attachment"),
                           (dict(depth_format=2), "not D32_SFLOAT"), (dict(depth_resolve_mode=2), "MIRHI_RESOLVE_SAMPLE_ZERO"),
                           (dict(dr_format=2), "must be D32_SFLOAT"), (dict(dr_h=81), "must be D32_SFLOAT"), (dict(prim_w=96), "4 * width x height"),
                           (dict(area_partial=1), "unsupported: a partial render area"), (dict(split_device=1), "unsupported: a multisampled scope on a split device"),
                           (dict(fragment_stats=1), "unsupported: fragment statistics")):
        rc, msg = _scope(mirhi, **change)
        assert rc == 1 and phrase in msg, (change, msg)


def test_draw_refusals(mirhi, scenes):
    S = scenes
    ok = lambda **kw: _msaa(mirhi, [2, kw.get("blend", 0), kw.get("discard", 0), kw.get("test", 1), kw.get("write", 1), kw.get("compare", S.CMP_LESS), kw.get("program", 0),
                                    kw.get("shadowed", 0), kw.get("change", 0)])
    for op in (S.CMP_LESS, S.CMP_LESS_OR_EQUAL, S.CMP_GREATER, S.CMP_GREATER_OR_EQUAL):
        for program in (S.PROGRAM_TRIANGLE, S.PROGRAM_MODEL, S.PROGRAM_MODEL_FULL, S.PROGRAM_MODEL_PBR):
            assert ok(compare=op, program=program) == (0, "")
    for kw, phrase in ((dict(blend=1), "unsupported: blending"), (dict(discard=1), "unsupported: fragment_discard_enable"),
                       (dict(test=0), "unsupported: a predicate depth state"), (dict(write=0), "unsupported: a predicate depth state"),
                       (dict(compare=S.CMP_EQUAL), "unsupported: a predicate depth state"), (dict(compare=S.CMP_ALWAYS), "unsupported: a predicate depth state"),
                       (dict(compare=S.CMP_NOT_EQUAL), "unsupported: a predicate depth state"), (dict(compare=S.CMP_NEVER), "unsupported: a predicate depth state"),
                       (dict(change=1), "unsupported: a depth state change"), (dict(program=S.PROGRAM_SKYBOX), "unsupported: a SKYBOX draw"),
                       (dict(program=S.PROGRAM_SHADOW), "unsupported: a SHADOW draw"), (dict(program=S.PROGRAM_MODEL_PBR_IBL), "unsupported: a MODEL_PBR_IBL draw"),
                       (dict(program=S.PROGRAM_MODEL_PBR, shadowed=1), "unsupported: a shadowed or cascaded draw")):
        rc, msg = ok(**kw)
        assert rc == 1 and phrase in msg, (kw, msg)
