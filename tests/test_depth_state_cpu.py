"""Depth bias and depth clamp, the parts that need no GPU: the float64 model of the bias (scenes.depth_bias_offset, the yardstick
of tests/test_gpu_depth_state.py) pinned against closed forms, and the ABI of mirhi_pipeline_create_with_depth_bias through every layer."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XY = [(8.0, 8.0), (72.0, 8.0), (8.0, 72.0)]           # dz/dx = (z1 - z0) / 64, dz/dy = (z2 - z0) / 64


def test_screen_parallel_triangle_has_the_constant_term_alone(scenes):
    for z, r in ((0.5, 2.0 ** -24), (0.75, 2.0 ** -24), (1.0, 2.0 ** -23), (2.0 ** -10, 2.0 ** -33), (0.0, 2.0 ** -149)):
        assert scenes.depth_bias_unit([z, z, z]) == r, z
        for c in (1.0, 1000.0, -1000.0, 2.0 ** 20):
            for s in (0.0, 7.0):                                  # (no slope: the slope factor multiplies 0)
                assert scenes.depth_bias_offset([z, z, z], XY, (c, 0.0, s)) == r * c, (z, c, s)
    # r follows the LARGEST |z| of the three vertices, whichever vertex has it, and changes exactly at the binade
    assert scenes.depth_bias_unit([0.25, 0.5, 0.25]) == 2.0 ** -24 == scenes.depth_bias_unit([0.5, 0.25, 0.25]) == scenes.depth_bias_unit([0.25, 0.25, 0.5])
    assert scenes.depth_bias_unit([0.25, float(np.nextafter(np.float32(0.5), np.float32(0))), 0.25]) == 2.0 ** -25
    assert scenes.depth_bias_unit([-0.75, 0.5, 0.25]) == 2.0 ** -24
    assert scenes.depth_bias_unit([1e-40, 0.0, 0.0]) == 2.0 ** -149          # a denormal maximum takes e = -126


def test_slope_term_on_a_plane_with_dyadic_slopes(scenes):
    z = [0.25, 0.5, 0.25]                                         # zx = 2^-8, zy = 0
    for s in (1.0, 4.0, -4.0):
        assert scenes.depth_bias_offset(z, XY, (0.0, 0.0, s)) == s * 2.0 ** -8
    assert scenes.depth_bias_offset(z, XY, (3.0, 0.0, 4.0)) == 4.0 * 2.0 ** -8 + 3.0 * 2.0 ** -24
    # |.|: a plane falling in x or in y has the same m; the vertex order does not matter
    assert scenes.depth_bias_offset([0.5, 0.25, 0.5], XY, (0.0, 0.0, 1.0)) == 2.0 ** -8
    assert scenes.depth_bias_offset([0.25, 0.25, 0.5], XY, (0.0, 0.0, 1.0)) == 2.0 ** -8
    assert scenes.depth_bias_offset([z[0], z[2], z[1]], [XY[0], XY[2], XY[1]], (0.0, 0.0, 1.0)) == 2.0 ** -8
    # m is the larger of the two slopes
    assert scenes.depth_bias_offset([0.25, 0.5, 0.375], XY, (0.0, 0.0, 1.0)) == 2.0 ** -8
    assert scenes.depth_bias_offset([0.25, 0.375, 0.5], XY, (0.0, 0.0, 1.0)) == 2.0 ** -8


def test_clamp_follows_the_sign_rule(scenes):
    z = [0.25, 0.5, 0.25]
    q = 2.0 ** -8
    assert scenes.depth_bias_offset(z, XY, (0.0, q, 4.0)) == q              # clamp > 0: min
    assert scenes.depth_bias_offset(z, XY, (0.0, q, -4.0)) == -4.0 * q      # ... and only an upper bound
    assert scenes.depth_bias_offset(z, XY, (0.0, -q, -4.0)) == -q           # clamp < 0: max
    assert scenes.depth_bias_offset(z, XY, (0.0, -q, 4.0)) == 4.0 * q       # ... and only a lower bound
    assert scenes.depth_bias_offset(z, XY, (0.0, 0.0, 4.0)) == 4.0 * q      # clamp 0: none
    assert scenes.depth_bias_offset(z, XY, (0.0, 0.0, -4.0)) == -4.0 * q


def test_m_is_the_max_form_not_the_sqrt_form(scenes):
    z = [0.25, 0.5, 0.5]                                          # zx = zy = 2^-8
    o = scenes.depth_bias_offset(z, XY, (0.0, 0.0, 1.0))
    assert o == 2.0 ** -8
    assert abs(o - math.sqrt(2.0) * 2.0 ** -8) > 0.4 * 2.0 ** -8  # the sqrt form would be larger by sqrt(2)


def test_abi_of_the_new_export(mirhi):
    header = open(os.path.join(ROOT, "include", "mirhi.h")).read()
    assert "#define MIRHI_ABI_VERSION 5u" in header and mirhi.ABI_VERSION == 5
    assert re.search(r"typedef struct \{ float constant_factor, clamp, slope_factor; \} mirhi_depth_bias;", header)
    decl = re.search(r"^mirhi_result mirhi_pipeline_create_with_depth_bias\(mirhi_device\* \w+, const mirhi_pipeline_desc\* \w+, const mirhi_depth_bias\* \w+, "
                     r"mirhi_pipeline\*\* \w+\);(.*)$", header, flags=re.M)
    assert decl and re.search(r":\d{3}", decl.group(1)), "the export cites the rhi method it replaces"
    assert C.sizeof(mirhi.DepthBias) == 12 and [f[0] for f in mirhi.DepthBias._fields_] == ["constant_factor", "clamp", "slope_factor"]
    # mirhi_pipeline_desc keeps the layout it had before depth bias existed (its size is part of ABI 5: callers pass it by pointer)
    assert C.sizeof(mirhi.PipelineDesc) == 140
    assert mirhi.PipelineDesc.fragment_discard_enable.offset == 136 and mirhi.PipelineDesc.depth_clamp_enable.offset == 48 and mirhi.PipelineDesc.depth_bias_enable.offset == 56
    res, args = mirhi._SIGNATURES["mirhi_pipeline_create_with_depth_bias"]
    assert res is C.c_int32 and len(args) == 4 and args[2] is C.POINTER(mirhi.DepthBias)
    assert hasattr(C.CDLL(mirhi.LIB_PATH), "mirhi_pipeline_create_with_depth_bias")
    hpp = open(os.path.join(ROOT, "renderer-rs_amd", "host", "mirhi.hpp")).read()
    assert "mirhi_pipeline_create_with_depth_bias(" in hpp and re.search(r"depth_bias\(float constant_factor, float clamp, float slope_factor\)", hpp)
    assert "depth_clamp_enable(bool" in hpp
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "mirhi-sys", "src", "lib.rs")).read()
    assert "pub fn mirhi_pipeline_create_with_depth_bias(dev: *mut mirhi_device, desc: *const mirhi_pipeline_desc, bias: *const mirhi_depth_bias, out: *mut *mut mirhi_pipeline) -> mirhi_result;" in sys_rs
    assert re.search(r"pub struct mirhi_depth_bias \{\n    pub constant_factor: f32,\n    pub clamp: f32,\n    pub slope_factor: f32,\n\}", sys_rs)
    pipe_rs = open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", "pipeline.rs")).read()
    assert "pub fn depth_bias(mut self, constant_factor: f32, clamp: f32, slope_factor: f32)" in pipe_rs and "pub fn depth_clamp_enable(mut self, on: bool)" in pipe_rs
    assert "mirhi_sys::mirhi_pipeline_create_with_depth_bias" in pipe_rs


def test_builder_and_specs_carry_the_two_states(mirhi, scenes):
    b = mirhi.GraphicsPipelineBuilder()
    assert b.desc.depth_clamp_enable == 0 and b.desc.depth_bias_enable == 0 and b.bias is None         # pipeline.rs:662-667 defaults
    b.depth_bias(1.5, -0.25, 2.0).depth_clamp_enable(True)
    assert b.desc.depth_bias_enable == 1 and b.desc.depth_clamp_enable == 1
    assert (b.bias.constant_factor, b.bias.clamp, b.bias.slope_factor) == (1.5, -0.25, 2.0)
    d = scenes.DrawSpec(vertices=np.zeros((3, 6), dtype=np.float32), stride=24, count=3)
    assert d.depth_bias is None and d.depth_clamp is False
    for spec in (scenes.ShadowSpec(casters=[d]), scenes.CascadeSpec(casters=[[d]])):
        assert spec.depth_bias is None and spec.depth_clamp is False
    # a caster without its own takes its spec's
    spec = scenes.ShadowSpec(casters=[d], depth_bias=(0.0, 0.0, 2.0), depth_clamp=True)
    assert mirhi._depth_state(None, d, spec) == ((0.0, 0.0, 2.0), True)
    own = scenes.DrawSpec(vertices=d.vertices, stride=24, count=3, depth_bias=(1.0, 0.0, 0.0))
    assert mirhi._depth_state(None, own, spec) == ((1.0, 0.0, 0.0), True)
    assert mirhi._depth_state(None, d) == (None, False)


def test_binding_refuses_a_library_without_the_symbol(tmp_path):
    """A libmirhi.so that lacks mirhi_pipeline_create_with_depth_bias (a stale build: every other export present, ABI 5) is refused by the binding's own
    loader, lib(), in a fresh interpreter -- an AttributeError that names the symbol, not a crash at the first biased pipeline."""
    import subprocess
    import sys
    import textwrap
    header = open(os.path.join(ROOT, "include", "mirhi.h")).read()
    names = sorted(set(n for n in re.findall(r"\b(mirhi_[a-z0-9_]+)\s*\(", header) if not n.endswith("_t")))
    assert "mirhi_pipeline_create_with_depth_bias" in names
    stub = tmp_path / "stub.c"
    stub.write_text("".join(f"unsigned {n}(void) {{ return 5u; }}\n" for n in names if n != "mirhi_pipeline_create_with_depth_bias"))
    pkg = tmp_path / "renderer-rs_amd"
    pkg.mkdir()
    for f in os.listdir(os.path.join(ROOT, "renderer-rs_amd")):
        if f.endswith(".py"):
            (pkg / f).write_bytes(open(os.path.join(ROOT, "renderer-rs_amd", f), "rb").read())
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(stub), "-o", str(pkg / "libmirhi_stub.so")])
    prog = textwrap.dedent(f"""
        import importlib.util, sys
        spec = importlib.util.spec_from_file_location("renderer_rs_amd", {str(pkg / "__init__.py")!r}, submodule_search_locations=[{str(pkg)!r}])
        m = importlib.util.module_from_spec(spec); sys.modules["renderer_rs_amd"] = m; spec.loader.exec_module(m)
        try:
            m.lib()
        except AttributeError as e:
            print("REFUSED", e); sys.exit(0)
        print("LOADED"); sys.exit(1)
        """)
    env = dict(os.environ, MIRHI_LIB_NAME="libmirhi_stub.so")
    r = subprocess.run([sys.executable, "-c", prog], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "REFUSED" in r.stdout and "mirhi_pipeline_create_with_depth_bias" in r.stdout, (r.stdout, r.stderr[-2000:])
