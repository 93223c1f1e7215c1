"""Multiview depth scopes without a GPU (include/mirhi.h "Multiview depth scopes"): the new names while the ABI stays 5, through every binding;
every refusal text and the per-view plan replayed through mirhi_debug_multiview; the new raster family behind the recorded ones; the test inputs themselves."""
import ctypes as C
import json
import os
import re

import numpy as np

import multiview_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("mirhi_multiview_info_default", "mirhi_cmd_begin_rendering_multiview")
D32, CLEAR, LOAD, STORE, DONT_CARE_STORE = 3, 1, 0, 0, 1


# ---- names ------------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_names_and_the_abi_stays_5(mirhi):
    header = open(os.path.join(ROOT, "include", "mirhi.h")).read()
    assert "#define MIRHI_ABI_VERSION 5u" in header and mirhi.ABI_VERSION == 5 and mirhi.lib().mirhi_abi_version() == 5
    lib = mirhi.lib()
    for fn in NEW_FUNCTIONS:
        assert re.search(r"\b%s\(" % fn, header), fn
        assert hasattr(lib, fn), fn
    decl = header[header.index("typedef struct {\n    uint32_t      view_mask;"):header.index("} mirhi_multiview_info;")]
    assert re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", decl)) == [name for name, _ in mirhi.MultiviewInfo._fields_]
    for phrase in ("view_offset + v * view_stride", "ViewIndex", "read when the scope EXECUTES", "Layers whose bit is clear are not touched", "flip_clip_y",
                   "frames_submitted counts the scope once", "mirhi_cmd_begin_rendering itself keeps refusing an array"):
        assert phrase in header, phrase
    assert mirhi.Format.D32_SFLOAT == D32
    assert (mirhi.LoadOp.LOAD, mirhi.LoadOp.CLEAR, mirhi.StoreOp.STORE, mirhi.StoreOp.DONT_CARE) == (LOAD, CLEAR, STORE, DONT_CARE_STORE)


def test_struct_size_matches_ctypes(mirhi, tmp_path):
    import subprocess
    src = tmp_path / "size.c"
    src.write_text('#include "mirhi.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(mirhi_multiview_info),\n'
                   '  offsetof(mirhi_multiview_info, view_mask), offsetof(mirhi_multiview_info, view_constants), offsetof(mirhi_multiview_info, view_offset),\n'
                   '  offsetof(mirhi_multiview_info, view_stride)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    M = mirhi.MultiviewInfo
    want = [C.sizeof(M), M.view_mask.offset, M.view_constants.offset, M.view_offset.offset, M.view_stride.offset]
    assert [int(x) for x in subprocess.check_output([str(exe)]).decode().split()] == want == [32, 0, 8, 16, 24]
    m = M(7, 9, 11, 13)
    mirhi.lib().mirhi_multiview_info_default(C.byref(m))
    assert (m.view_mask, m.view_constants, m.view_offset, m.view_stride) == (0, None, 0, 64)


def test_python_names(mirhi, scenes):
    assert hasattr(mirhi.CommandBuffer, "begin_rendering_multiview") and callable(mirhi.multiview_info)

    class Buf:       # (no device: the info only carries the handle)
        handle = 77
    m = mirhi.multiview_info(0b1011, Buf(), 32, 80)
    assert (m.view_mask, m.view_constants, m.view_offset, m.view_stride) == (0b1011, 77, 32, 80)
    assert callable(scenes.record_cascades_multiview) and scenes.MULTIVIEW_STRIDE == 80
    spec = scenes.cascaded_ground_case(64, 48, map_size=64).cascades
    vc = scenes.cascade_view_constants(spec)
    assert len(vc) == 320
    # the layout is CSMParams' (matrix k at 80 k); the matrix is the one the casters render with: the lookup's with clip y negated
    for k in range(4):
        got = np.frombuffer(vc[80 * k:80 * k + 64], dtype=np.float32).reshape(4, 4)
        lookup = np.frombuffer(spec.params[80 * k:80 * k + 64], dtype=np.float32).reshape(4, 4)
        assert np.array_equal(got, scenes.flip_clip_y(lookup)) and not np.array_equal(got, lookup)
        assert bytes(vc[80 * k:80 * k + 64]) == bytes(spec.casters[k][0].camera[:64])


def test_cpp_and_rust_names():
    hpp = open(os.path.join(ROOT, "renderer-rs_amd", "host", "mirhi.hpp")).read()
    for name in ("RenderingConfig& with_view_mask(uint32_t mask, const Buffer& view_constants", "mirhi_cmd_begin_rendering_multiview(h_, &cfg.build(), &cfg.views())",
                 "void begin_rendering_multiview(const mirhi_rendering_info& info, const mirhi_multiview_info& views)", "mirhi_multiview_info_default(&multiview_)"):
        assert name in hpp, name
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "mirhi-sys", "src", "lib.rs")).read()
    for fn in NEW_FUNCTIONS:
        assert re.search(r"pub fn %s\(" % fn, sys_rs), fn
    decl = sys_rs[sys_rs.index("pub struct mirhi_multiview_info {"):]
    decl = decl[:decl.index("}")]
    assert re.findall(r"pub (\w+): ([^,\n]+),", decl) == [("view_mask", "u32"), ("view_constants", "*mut mirhi_buffer"), ("view_offset", "u64"), ("view_stride", "u32")]
    cmd = open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", "command.rs")).read()
    assert "pub fn begin_rendering_multiview(&self, depth_array: &Image, depth_load_op: LoadOp, clear_depth: f32, view_mask: u32, view_constants: &Buffer," in cmd
    assert "mirhi_sys::mirhi_cmd_begin_rendering_multiview(self.raw, &ri, &mv)" in cmd
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "mirhi_cmd_begin_rendering_multiview" in open(os.path.join(ROOT, doc)).read(), doc


# ---- mirhi_debug_multiview ------------------------------------------------------------------------------------------------------------------------
def _debug(mirhi, words):
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_multiview
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32]
    words = [int(w) & 0xFFFFFFFF for w in words]
    inp, out, msg = (C.c_uint32 * 32)(*(words + [0] * (32 - len(words)))), (C.c_uint32 * 48)(), C.create_string_buffer(256)
    rc = fn(inp, out, msg, len(msg))
    return rc, msg.value.decode(), list(out)


# the words of MultiviewFacts, in order (mirhi_scope.h); the 64-bit ones as (low, high)
FACTS = ["has_color", "has_prim", "has_depth", "depth_is_array", "depth_samples", "depth_format", "layers", "depth_load_op", "depth_store_op", "view_mask",
         "has_constants", "view_stride", "view_offset", "constants_bytes", "area_partial", "split_device", "fragment_stats"]
GOOD = dict(has_color=0, has_prim=0, has_depth=1, depth_is_array=1, depth_samples=1, depth_format=D32, layers=4, depth_load_op=CLEAR, depth_store_op=STORE,
            view_mask=0b1111, has_constants=1, view_stride=80, view_offset=0, constants_bytes=336, area_partial=0, split_device=0, fragment_stats=0)


def _scope(mirhi, **change):
    f = dict(GOOD, **change)
    words = [0]
    for k in FACTS:
        words += [f[k] & 0xFFFFFFFF, f[k] >> 32] if k in ("view_offset", "constants_bytes") else [f[k]]
    rc, msg, _ = _debug(mirhi, words)
    return rc, msg


def test_every_refusal_text(mirhi, scenes):
    text = open(os.path.join(ROOT, "renderer-rs_amd", "csrc", "mirhi_scope.h")).read()
    decl = text[text.index("struct MultiviewFacts {"):text.index("};", text.index("struct MultiviewFacts {"))]
    decl = re.sub(r"//[^\n]*", "", decl)
    assert re.findall(r"\b([a-z_]+)[,;]", decl) == FACTS       # the test's word order is the struct's
    assert _scope(mirhi) == (0, "")
    assert _scope(mirhi, depth_load_op=LOAD) == (0, "")
    assert _scope(mirhi, view_mask=0b1000, view_offset=16, constants_bytes=16 + 3 * 80 + 64) == (0, "")
    assert _scope(mirhi, layers=40, view_mask=0x80000001, view_stride=64, constants_bytes=32 * 64) == (0, "")
    for change, phrase in ((dict(has_color=1), "a multiview scope is depth-only (color_image and prim_id_image NULL)"),
                           (dict(has_prim=1), "a multiview scope is depth-only (color_image and prim_id_image NULL)"),
                           (dict(has_depth=0), "a multiview scope renders into an image array (mirhi_image_create_array), not a 2-D image or a layer view"),
                           (dict(depth_is_array=0), "a multiview scope renders into an image array (mirhi_image_create_array), not a 2-D image or a layer view"),
                           (dict(depth_samples=4), "a multisampled depth image in a multiview scope"),
                           (dict(depth_format=2), "a multiview depth array that is not D32_SFLOAT"),
                           (dict(depth_load_op=2), "the depth load op of a multiview scope is CLEAR or LOAD"),
                           (dict(depth_store_op=DONT_CARE_STORE), "a multiview scope must store its depth (STORE)"),
                           (dict(view_mask=0), "an empty view mask"),
                           (dict(view_mask=0x1FF, layers=16, constants_bytes=4096), "more than 8 views in one multiview scope"),
                           (dict(view_mask=0b10000), "a view mask bit at or above the array's layer count"),
                           (dict(layers=3), "a view mask bit at or above the array's layer count"),
                           (dict(has_constants=0), "a multiview scope without view_constants"),
                           (dict(view_stride=48), "view_stride must be at least 64 and a multiple of 16"),
                           (dict(view_stride=72), "view_stride must be at least 64 and a multiple of 16"),
                           (dict(view_offset=8), "view_offset must be a multiple of 16"),
                           (dict(constants_bytes=303), "the view_constants buffer is too short for the highest view's matrix"),
                           (dict(view_offset=48), "the view_constants buffer is too short for the highest view's matrix"),
                           (dict(view_offset=1 << 36), "the view_constants buffer is too short for the highest view's matrix"),
                           (dict(area_partial=1), "a partial render area in a multiview scope"),
                           (dict(split_device=1), "a multiview scope on a split device"),
                           (dict(fragment_stats=1), "fragment statistics of a multiview scope")):
        rc, msg = _scope(mirhi, **change)
        assert rc == 1 and msg == "unsupported: " + phrase, (change, msg)
    assert _scope(mirhi, constants_bytes=304) == (0, "")          # 3 * 80 + 64: the highest view's matrix ends where the buffer ends
    assert _debug(mirhi, [1, scenes.PROGRAM_SHADOW])[:2] == (0, "")
    for program in (scenes.PROGRAM_TRIANGLE, scenes.PROGRAM_MODEL, scenes.PROGRAM_MODEL_FULL, scenes.PROGRAM_MODEL_PBR, scenes.PROGRAM_MODEL_PBR_IBL, scenes.PROGRAM_SKYBOX):
        assert _debug(mirhi, [1, program])[:2] == (1, "unsupported: only SHADOW draws may be recorded in a multiview scope")
    assert _debug(mirhi, [9])[0] == -1


def test_per_view_plan(mirhi):
    """Layer bases and matrix addresses: slot j is the j-th set bit v of the mask, its layer at v * width * height * 4, its matrix at view_offset + v * view_stride."""
    for mask, w, h, offset, stride in ((0b1111, 96, 96, 32, 80), (0b1010, 1024, 1024, 0, 80), (0b100001, 2048, 2048, 16, 64), (0xFF, 7, 5, (1 << 33) + 16, 4096),
                                       (0x80000000, 4096, 4096, 0, 64)):
        rc, msg, out = _debug(mirhi, [2, mask, w, h, offset & 0xFFFFFFFF, offset >> 32, stride])
        views = [v for v in range(32) if (mask >> v) & 1]
        assert rc == 0 and msg == "" and out[0] == len(views)
        for j, v in enumerate(views):
            view, lo, hi, mlo, mhi = out[1 + 5 * j:6 + 5 * j]
            assert view == v and (lo | hi << 32) == v * w * h * 4 and (mlo | mhi << 32) == offset + v * stride, (mask, j)
    # the tests' own constants buffer puts the matrices where the plan reads them
    mats = [np.full((4, 4), k + 1, dtype=np.float32) for k in range(4)]
    buf = mc.view_constants(mats, 4)
    rc, _, out = _debug(mirhi, [2, 0b1111, mc.SIZE, mc.SIZE, mc.OFFSET, 0, mc.STRIDE])
    for j in range(4):
        at = out[1 + 5 * j + 3]
        assert np.array_equal(np.frombuffer(buf[at:at + 64].tobytes(), dtype=np.float32), mats[j].ravel())


# ---- the variant ----------------------------------------------------------------------------------------------------------------------------------
def test_new_family_sits_behind_the_recorded_rows(mirhi):
    text = open(os.path.join(ROOT, "renderer-rs_amd", "csrc", "mirhi_variant.h")).read()
    assert re.search(r"RASTER_CSM_BLEND, RASTER_MSAA \};", text) and "RASTER_DEPTH_VIEWS = (RasterFamily)(RASTER_MSAA + 1u)" in text
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "raster_variants.json")))
    recorded = json.dumps(rows)
    assert "raster_kernel_depth_batch" not in recorded and "vertex_kernel_shadow_batch" not in recorded
    for (zflip, tp), name in {(0, 64): "raster_kernel_depth_batch<0, 1>", (0xFFFFFFFF, 64): "raster_kernel_depth_batch<1, 1>",
                              (0, 0): "raster_kernel_depth_batch<0, 0>", (0xFFFFFFFF, 0): "raster_kernel_depth_batch<1, 0>"}.items():
        for views in (1, 4, 8):
            rc, msg, out = _debug(mirhi, [3, zflip, 0xFFFFFFFF, tp, views])
            family, keyed, tpv, gx, gy, gz, block, batched, last_older = out[:9]
            assert rc == 0 and msg == name, (zflip, tp, msg)
            assert family == last_older + 1 == 11 and (keyed, tpv) == (1 if zflip else 0, 1 if tp else 0)
            assert (gx, gy, gz, block, batched) == (5, 4, views, 256, 0)      # one grid layer per view; never batched across command buffers
    kernels = open(os.path.join(ROOT, "renderer-rs_amd", "csrc", "mirhi_kernels.hip")).read()
    assert kernels.index('#include "mirhi_multiview.hip.h"') > kernels.index('#include "mirhi_transfer.hip.h"')      # behind every older kernel of the code object


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------------------
def test_inputs_hold_what_the_gpu_tests_need(scenes):
    assert mc.SIZE == 96 and mc.TILES == 9 and mc.LAYERS == 4 and mc.OFFSET % 16 == 0 and mc.STRIDE % 16 == 0 and mc.STRIDE >= 64
    density = mc.tp_density()
    assert density == 4
    counts = {r: sum(int(i.size) // 3 for _, i, _ in mc.route_casters(r)[0]) for r in mc.ROUTES}
    assert counts["records65"] == 65 and counts["records193"] == 193
    assert counts["tp_below"] == density * mc.TILES - 1 and counts["tp_at"] == density * mc.TILES
    assert counts["big_list"] < density * mc.TILES and counts["near_clip"] < density * mc.TILES      # (these two also run the kernels without the triangle-parallel path)
    # the 65 / 193 records sit in the middle tile under the identity view
    for r in ("records65", "records193"):
        v, _, _ = mc.route_casters(r)[0][0]
        px = (v[:, 0:2] * 0.5 + 0.5) * mc.SIZE
        assert px.min() >= 32.0 and px.max() < 64.0
    big = mc.route_casters("big_list")[0][0][0]
    assert np.ptp((big[:, 0] * 0.5 + 0.5) * mc.SIZE) > 256.0        # more than 65535 sub-pixels apart
    assert (mc.route_casters("near_clip")[0][0][0][:, 2] < 0).sum() == 1
    x, y, w, h = mc.route_casters("scissor")[1]
    assert x % 32 and y % 32 and (x + w) % 32 and (y + h) % 32
    mats = mc.view_matrices(np.eye(4, dtype=np.float32), 6)
    assert len({m.tobytes() for m in mats}) == 6 and all(m[0, 0] >= 1.0 for m in mats)
    buf = mc.view_constants(mats, 6)
    assert buf.size == mc.OFFSET + 5 * mc.STRIDE + 64 and (buf[:mc.OFFSET] == 0xFF).all() and (buf[mc.OFFSET + 64:mc.OFFSET + mc.STRIDE] == 0xFF).all()
    s = mc.sentinels()
    assert s.shape == (4, 96, 96) and len({float(s[k, 1, 1]) for k in range(4)}) == 4
