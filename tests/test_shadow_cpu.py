"""Shadow mapping without a GPU: the new names agree across include/mirhi.h, the ctypes binding and the Rust sys crate; ShadowParams and
ShadowConstants pack the HLSL layouts; the numpy PCF model that test_gpu_shadow.py checks the GPU against works a hand example."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_values():
    text = open(os.path.join(ROOT, "include", "mirhi.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b(MIRHI_(?:PROGRAM|SLOT|TEXTURE)_\w+)\s*=\s*(-?\d+)", text)}


def test_shadow_names_agree_across_header_binding_and_rust(mirhi):
    h = _header_values()
    assert h["MIRHI_PROGRAM_SHADOW"] == mirhi.Program.SHADOW == 4
    assert h["MIRHI_SLOT_SHADOW_DATA"] == mirhi.Slot.SHADOW_DATA == 6 and h["MIRHI_SLOT_COUNT"] == 7
    assert h["MIRHI_TEXTURE_SHADOW_MAP"] == mirhi.TextureSlot.SHADOW_MAP == 5 and h["MIRHI_TEXTURE_COUNT"] == 6
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "mirhi-sys", "src", "lib.rs")).read()
    for name in ("MIRHI_PROGRAM_SHADOW", "MIRHI_SLOT_SHADOW_DATA", "MIRHI_TEXTURE_SHADOW_MAP", "MIRHI_SLOT_COUNT", "MIRHI_TEXTURE_COUNT"):
        m = re.search(rf"pub const {name}: \w+ = (-?\d+);", sys_rs)
        assert m and int(m.group(1)) == h[name], name
    wrapper = open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", "command.rs")).read()
    assert "ShadowData = 6" in wrapper and "ShadowMap = 5" in wrapper
    assert "Shadow = 4" in open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", "pipeline.rs")).read()
    assert "Shadow = 4" in open(os.path.join(ROOT, "renderer-rs_amd", "host", "mirhi.hpp")).read()


def test_shadow_ubo_packs_the_std140_layout(scenes):
    ls = scenes.light_space_matrix((0.3, -1.0, 0.2))
    raw = scenes.shadow_ubo(ls, bias=0.004, normal_bias=0.03, size=(1024, 512), strength=0.7)
    assert len(raw) == 96
    f = np.frombuffer(raw, dtype=np.float32)
    assert np.array_equal(f[:16], ls.reshape(-1))                      # LightSpaceMatrix @0
    assert f[16] == np.float32(0.004) and f[17] == np.float32(0.03)    # ShadowBias @64, NormalBias @68
    assert f[18] == 1024.0 and f[19] == 512.0                          # ShadowMapSize @72
    assert f[20] == np.float32(0.7) and not f[21:].any()               # ShadowStrength @80, padding
    model = scenes.trs((2.0, 2.0, 2.0), (0.0, 0.0, 0.0, 1.0), (1.0, 2.0, 3.0))
    c = np.frombuffer(scenes.shadow_constants_ubo(ls, model), dtype=np.float32)
    assert c.size == 32 and np.array_equal(c[:16], ls.reshape(-1)) and np.array_equal(c[16:], model.reshape(-1))


def test_orthographic_light_matrix_maps_its_frustum():
    import __graft_entry__ as ge
    scenes = ge.load_package().scenes
    ls = scenes.light_space_matrix((0.0, -1.0, 0.0), center=(0.0, 0.0, 0.0), half_extent=2.0, near=0.1, far=20.0, distance=10.0)
    M = ls.T.astype(np.float64)
    for p, want in (((2.0, 0.0, 0.0), (1.0, None)), ((-2.0, 0.0, 0.0), (-1.0, None))):
        c = M @ np.array([*p, 1.0])
        assert abs(c[0] - want[0]) < 1e-6 and abs(c[3] - 1.0) < 1e-7
    near = M @ np.array([0.0, 9.9, 0.0, 1.0])
    far = M @ np.array([0.0, -10.0, 0.0, 1.0])
    assert abs(near[2]) < 1e-6 and abs(far[2] - 1.0) < 1e-6                # depth 0 at near, 1 at far
    f = scenes.flip_clip_y(ls)
    assert np.array_equal(f[:, 1], -ls[:, 1]) and np.array_equal(f[:, 0], ls[:, 0])


def test_pcf_model_hand_worked_4x4(scenes):
    """A 4 x 4 map, texel size 1/4; a sample at the centre of texel (1, 1) sees texels [0..2] x [0..2]; one at texel (0, 3) sees the clamped
    neighbourhood (columns 0, 0, 1 and rows 2, 3, 3)."""
    m = np.array([[1.0, 0.2, 1.0, 1.0],
                  [1.0, 1.0, 0.2, 1.0],
                  [0.2, 1.0, 1.0, 1.0],
                  [0.2, 0.2, 1.0, 0.2]], dtype=np.float32)
    u = np.array([1.5 / 4, 0.5 / 4, 3.5 / 4])
    v = np.array([1.5 / 4, 3.5 / 4, 0.5 / 4])
    dref = np.full(3, 0.5)
    # column 1, row 1: rows 0-2 x columns 0-2 hold three 0.2 texels -> 6 lit taps
    # column 0, row 3: columns (0, 0, 1) x rows (2, 3, 3): only m[2, 1] is lit -> 1
    # column 3, row 0: columns (2, 3, 3) x rows (0, 0, 1): 3 + 3 + 2 -> 8
    s = scenes.pcf_factor(m, u, v, dref)
    assert np.allclose(s, [6 / 9, 1 / 9, 8 / 9])
    assert np.allclose(scenes.pcf_factor(m, u, v, dref, strength=0.6), 1.0 + (np.array([6, 1, 8]) / 9 - 1.0) * 0.6)
    assert np.allclose(scenes.pcf_factor(m, u, v, np.full(3, 1.5)), [6 / 9, 1 / 9, 8 / 9])     # D_ref clamped to 1: the 1.0 texels stay lit
    assert np.allclose(scenes.pcf_factor(m, u, v, np.full(3, -1.0)), 1.0)                     # clamped to 0: every tap lit
