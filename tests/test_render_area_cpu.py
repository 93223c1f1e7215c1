"""Render areas without a GPU: what render_area (mirhi_scope.h) decides -- validity, the tile range a scope launches, whether an
edge tile is partial, the tile counts handed to raster_mode / bin_geometry -- through mirhi_debug_render_area, which makes no HIP call; the
soundness of the yardstick the GPU tests compare with (tests/render_area_cases.py), shown on the oracle alone; and the mirrors: the Python keyword,
the C++ builder and the Rust wrapper all reach mirhi_rendering_info::render_area."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import render_area_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = "x y w h partial col_begin col_end row_begin row_end edge_partial tiles index_tiles".split()


@pytest.fixture(scope="module")
def plan(mirhi):
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_render_area
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32]

    def plan(width, height, area):
        """(0, dict of the output words) or (-1, the refusal's message)."""
        inp, out, msg = (C.c_int32 * 6)(width, height, *area), (C.c_uint32 * 12)(), C.create_string_buffer(256)
        r = fn(inp, out, msg, len(msg))
        return (r, dict(zip(OUT, out))) if r == 0 else (r, msg.value.decode())
    return plan


def expected(width, height, area):
    """The definition, restated: the tiles of the attachment's own 32 x 32 grid that hold a pixel of the area."""
    x, y, w, h = area if area[2] > 0 and area[3] > 0 else (0, 0, width, height)
    m = rc.mask((x, y, w, h), width, height)
    ty, tx = np.nonzero(m)
    cols, rows = np.unique(tx // 32), np.unique(ty // 32)
    whole = all(m[r * 32:(r + 1) * 32, c * 32:(c + 1) * 32].sum() == 32 * 32 for r in rows for c in cols)
    return dict(x=x, y=y, w=w, h=h, partial=int((x, y, w, h) != (0, 0, width, height)), col_begin=int(cols[0]), col_end=int(cols[-1]) + 1,
                row_begin=int(rows[0]), row_end=int(rows[-1]) + 1, edge_partial=int(not whole), tiles=len(cols) * len(rows),
                index_tiles=((width + 31) // 32) * len(rows))


@pytest.mark.parametrize("extent", [(320, 200), (256, 160), (160, 128), (500, 250), (97, 96)])
def test_tile_ranges_and_partial_flags(plan, extent):
    width, height = extent
    for name, area in rc.areas(width, height).items():
        r, got = plan(width, height, area)
        assert r == 0, (name, got)
        assert got == expected(width, height, area), (name, area)
    # the named properties of the list
    a = plan(width, height, rc.areas(width, height)["a_aligned"])[1]
    assert a["partial"] == 1 and a["edge_partial"] == 0
    b = plan(width, height, rc.areas(width, height)["b_unaligned"])[1]
    assert b["edge_partial"] == 1 and b["col_end"] - b["col_begin"] >= 2 and b["row_end"] - b["row_begin"] >= 2
    for one_tile in ("c_in_one_tile", "e_one_pixel"):
        assert plan(width, height, rc.areas(width, height)[one_tile])[1]["tiles"] == 1
    assert plan(width, height, rc.areas(width, height)["d_corner_2x2"])[1]["tiles"] == 4
    f = plan(width, height, rc.areas(width, height)["f_column"])[1]
    assert f["col_end"] - f["col_begin"] == 1 and f["row_end"] - f["row_begin"] == (height + 31) // 32
    g = plan(width, height, rc.areas(width, height)["g_bottom_right"])[1]
    assert g["col_end"] == (width + 31) // 32 and g["row_end"] == (height + 31) // 32


@pytest.mark.parametrize("extent", [(320, 200), (256, 160), (500, 250), (1, 1), (33, 31), (8192, 8192)])
def test_full_extent_is_todays_grid(plan, extent):
    """The explicit full extent, width <= 0 and height <= 0 all give the attachment's whole grid, not partial: the plan of a scope without an area."""
    width, height = extent
    tx, ty = (width + 31) // 32, (height + 31) // 32
    for area in ((0, 0, width, height), (0, 0, 0, 0), (5, 7, 0, 3), (5, 7, 3, -1)):
        r, got = plan(width, height, area)
        assert r == 0
        assert got == dict(x=0, y=0, w=width, h=height, partial=0, col_begin=0, col_end=tx, row_begin=0, row_end=ty,
                           edge_partial=int(width % 32 != 0 or height % 32 != 0), tiles=tx * ty, index_tiles=tx * ty), area


@pytest.mark.parametrize("area,why", [((-1, 0, 10, 10), "negative x"), ((0, -3, 10, 10), "negative y"), ((300, 0, 21, 10), "x + w > W"),
                                      ((0, 190, 10, 11), "y + h > H"), ((2147483647, 0, 2147483647, 10), "x + w overflows 32 bits"),
                                      ((0, 1, 10, 2147483647), "y + h overflows 32 bits"), ((320, 0, 1, 1), "origin on the far edge")])
def test_invalid_areas_are_refused_with_their_numbers(plan, area, why):
    r, msg = plan(320, 200, area)
    assert r == -1, why
    assert msg.startswith("Invalid handle: render area"), msg
    for v in (*area, 320, 200):
        assert re.search(rf"(?<![\d-]){v}(?!\d)", msg), (v, msg)


def test_the_edge_itself_is_valid(plan):
    for area in ((319, 199, 1, 1), (0, 0, 320, 1), (300, 0, 20, 200)):
        assert plan(320, 200, area)[0] == 0


@pytest.mark.parametrize("case", ["random_small", "cull_scissor", "sphere_small"])
def test_cutting_the_scissors_changes_no_pixel_inside_the_area(oracle, scenes, case):
    """The yardstick is sound: oracle(scene with scissor n area) equals oracle(scene) inside the area, bit for bit, and holds nothing outside."""
    scene = scenes.SMALL_CASES[case]()
    area = (19, 13, scene.width - 19 - 23, scene.height - 13 - 17) if scene.width >= 96 else (5, 3, scene.width - 9, scene.height - 8)
    full = oracle.render(scene, want_bgra8=True)
    cut = oracle.render(rc.cut_to_area(scene, area), want_bgra8=True)
    m = rc.mask(area, scene.width, scene.height)
    assert (full["prim"][m] != rc.NO_PRIM).any()
    for key in ("prim", "rgba", "bgra8", "depth"):
        assert rc.same_bits(np.ascontiguousarray(full[key][m]), np.ascontiguousarray(cut[key][m])), key
    assert (cut["prim"][~m] == rc.NO_PRIM).all()


def test_intersect():
    assert rc.intersect(None, (19, 13, 50, 40), 320, 200) == (19, 13, 50, 40)
    assert rc.intersect((16, 8, 90, 60), (19, 13, 50, 80), 320, 200) == (19, 13, 50, 55)
    assert rc.intersect((0, 0, 10, 10), (19, 13, 50, 40), 320, 200)[2:] == (0, 0)


# ---- the mirrors ----
def test_python_keyword_fills_the_four_ints(mirhi):
    assert list(mirhi.rendering_info().render_area) == [0, 0, 0, 0]
    assert list(mirhi.rendering_info(render_area=(19, 13, 278, 170)).render_area) == [19, 13, 278, 170]
    import inspect
    assert inspect.signature(mirhi.CommandBuffer.begin_rendering).parameters["render_area"].default is None
    assert mirhi.scenes.Scene("s", 64, 64).render_area is None
    assert rc.in_area(mirhi.scenes.Scene("s", 64, 64), (1, 2, 3, 4)).render_area == (1, 2, 3, 4)


def test_cpp_builder_fills_the_four_ints(mirhi, tmp_path):
    src = tmp_path / "area.cpp"
    src.write_text('#include <cstdio>\n#include "mirhi.hpp"\n'
                   'static void show(const mirhi_rendering_info& i) { std::printf("%d %d %d %d\\n", i.render_area[0], i.render_area[1], i.render_area[2], i.render_area[3]); }\n'
                   'int main() {\n'
                   '    show(mirhi::RenderingConfig(320, 200).build());\n'
                   '    show(mirhi::RenderingConfig(320, 200).with_render_area(mirhi_rect2d{19, 13, 278u, 170u}).build());\n'
                   '    show(mirhi::RenderingConfig(320, 200).with_offset(7, 9).build());\n'
                   '    show(mirhi::RenderingConfig(320, 200).with_render_area(mirhi_rect2d{0, 0, 64u, 32u}).with_offset(64, 96).build());\n'
                   '    return 0;\n}\n')
    pkg = os.path.dirname(mirhi.LIB_PATH)
    exe = tmp_path / "area"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", "-I", os.path.join(pkg, "host"), str(src), "-o", str(exe),
                           "-L", pkg, "-lmirhi", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"])
    lines = [[int(v) for v in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()]
    assert lines == [[0, 0, 0, 0], [19, 13, 278, 170], [7, 9, 320, 200], [64, 96, 64, 32]]


def test_rust_wrapper_field_reaches_the_sys_struct():
    cmd = open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", "command.rs")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "mirhi-sys", "src", "lib.rs")).read()
    assert re.search(r"pub render_area: \[i32; 4\]", sys_rs)
    assert re.search(r"ri\.render_area = \[info\.render_area\.x, info\.render_area\.y, info\.render_area\.width as i32, info\.render_area\.height as i32\];", cmd)
    assert re.search(r"pub fn with_render_area\(mut self, area: Rect2D\) -> Self", cmd) and re.search(r"pub fn with_offset\(mut self, x: i32, y: i32\) -> Self", cmd)


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "mirhi.h")).read()
    i = text.index("render_area[4]")
    comment = text[i:text.index("prim_id_image;", i)]
    for phrase in ("full extent", "no pixel outside is written", "split device"):
        assert phrase in comment, phrase
