"""Cascaded shadow maps without a GPU: the new entry points agree across include/mirhi.h, the ctypes binding, mirhi.hpp and the Rust crates;
CSMParams packs the HLSL layout; the numpy model of CalculateShadowCSM works a hand example; csm_cascades encloses its frustum slices; and the
inputs of test_gpu_csm.py satisfy, on oracle output alone, the conditions that test asserts (csm_cases.py)."""
import os
import re

import numpy as np

import csm_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("mirhi_image_create_array", "mirhi_image_create_layer_view", "mirhi_image_layers", "mirhi_cmd_bind_shadow_cascades")


def test_csm_names_agree_across_header_binding_hpp_and_rust(mirhi):
    header = open(os.path.join(ROOT, "include", "mirhi.h")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "mirhi-sys", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "renderer-rs_amd", "host", "mirhi.hpp")).read()
    wrapper = "".join(open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", f)).read() for f in ("image.rs", "command.rs"))
    for name in NEW_FUNCTIONS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in mirhi._SIGNATURES and hasattr(mirhi.lib(), name), name
        assert f"pub fn {name}(" in sys_rs, name
        assert f"{name}(" in hpp and f"mirhi_sys::{name}(" in wrapper, name
    assert len(mirhi._SIGNATURES["mirhi_image_create_array"][1]) == 6 and len(mirhi._SIGNATURES["mirhi_cmd_bind_shadow_cascades"][1]) == 5
    for attr in ("array", "layer_view", "layers"):
        assert hasattr(mirhi.Image, attr), attr
    assert hasattr(mirhi.CommandBuffer, "bind_shadow_cascades")
    # new functions only: the ABI version, the slot counts and the struct layouts stay
    assert "#define MIRHI_ABI_VERSION 5u" in header and "MIRHI_SLOT_COUNT = 7" in header and "MIRHI_TEXTURE_COUNT = 6" in header
    assert mirhi.lib().mirhi_image_layers(None) == 0


def test_csm_ubo_packs_the_hlsl_layout(scenes):
    mats = [scenes.light_space_matrix((0.3, -1.0, 0.2), half_extent=2.0 + k) for k in range(4)]
    raw = scenes.csm_ubo(mats, [0.91, 0.95, 0.98, 0.995], bias=0.004, normal_bias=0.03, map_size=1024.0)
    assert len(raw) == 336
    f = np.frombuffer(raw, dtype=np.float32)
    for k in range(4):
        assert np.array_equal(f[20 * k:20 * k + 16], mats[k].reshape(-1))                  # Cascades[k].ViewProjection @80k
        assert f[20 * k + 16] == np.float32([0.91, 0.95, 0.98, 0.995][k])                  # Cascades[k].SplitDepth @80k + 64
        assert not f[20 * k + 17:20 * k + 20].any()                                        # float3 Padding
    assert f[80] == np.float32(0.004) and f[81] == np.float32(0.03) and f[82] == 1024.0 and f[83] == 0.0     # @320, @324, @328, padding @332
    three = np.frombuffer(scenes.csm_ubo(mats, [0.91, 0.95, 0.98]), dtype=np.float32)
    assert three[16] == np.float32(0.91) and three[56] == np.float32(0.98) and three[82] == 2048.0


def _down(scenes, half, centre=(0.0, 0.0, 0.0)):
    return scenes.light_space_matrix((0.0, -1.0, 0.0), center=centre, half_extent=half, near=0.0, far=20.0, distance=10.0)


def test_csm_model_hand_worked_4x4(scenes):
    """Four 4 x 4 layers, four lights straight down at the origin (up = -z: u = (x / half + 1) / 2, v = (z / half + 1) / 2, depth = (10 - y) / 20),
    half extents 2, 4, 8, 16; a flat receiver at y = 0 (depth 0.5, dref 0.4995), splits 0.2 / 0.4 / 0.6."""
    layers = np.ones((4, 4, 4), dtype=np.float32)
    layers[0, 1, 1] = 0.2                 # one occluded texel in the middle of layer 0
    layers[1, :, 0] = 0.2                 # layer 1: column 0 occluded
    layers[2] = 0.2                       # layer 2: everything occluded
    layers[3, 3, :] = 0.2                 # layer 3: the last row occluded
    mats = [_down(scenes, h) for h in (2.0, 4.0, 8.0, 16.0)]
    splits = np.array([0.2, 0.4, 0.6], dtype=np.float32)
    up, L = (0.0, 1.0, 0.0), (0.0, 1.0, 0.0)

    def f(pos, clip_depth, normal=up, nb=0.0, sp=splits):
        return float(scenes.csm_factor(layers, mats, sp, np.array(pos, dtype=np.float64), normal, L, np.float32(clip_depth), 0.005, nb, 4.0))
    # cascade 0 (clip depth 0.1): texel size 1 world unit; (x, z) = (-0.5, -0.5) is the centre of texel (1, 1): taps cover [0..2]^2 -> 8 of 9 lit
    assert np.isclose(f((-0.5, 0.0, -0.5), 0.1), 8 / 9)
    # cascade 1 (0.3): texel 2 units; x = -3 is the centre of column 0 (clamp-to-edge inside the layer: columns 0, 0, 1) -> 3 of 9 lit
    assert np.isclose(f((-3.0, 0.0, 1.0), 0.3), 3 / 9)
    # cascade 2 (0.5): all occluded -> 0; cascade 3 (0.7): z = 12 is row 3 (rows 2, 3, 3): 3 of 9 lit
    assert f((1.0, 0.0, 1.0), 0.5) == 0.0
    assert np.isclose(f((0.0, 0.0, 12.0), 0.7), 3 / 9)
    # exactly AT a split: `>` is strict, the fragment stays in the nearer cascade
    assert np.isclose(f((-0.5, 0.0, -0.5), np.float32(0.2)), 8 / 9) and np.isclose(f((-3.0, 0.0, 1.0), np.float32(0.4)), 3 / 9)
    assert np.isclose(f((-0.5, 0.0, -0.5), np.nextafter(np.float32(0.2), np.float32(1.0))), 6 / 9)      # just past it: cascade 1, column 1 of layer 1 with columns 0..2 tapped
    # unsorted splits: the LAST split passed decides (0.5 > 0.45 -> cascade 3), not the first cascade that "contains" the depth
    assert np.isclose(f((0.0, 0.0, 12.0), 0.5, sp=np.array([0.6, 0.7, 0.45], dtype=np.float32)), 3 / 9)
    # the bounds test is on the OFFSET position: x = 1.9 is inside cascade 0, 1.9 + 0.2 is not -> 1.0 (layer 0's texel would not matter)
    n = (1.0, 0.0, 0.0)
    assert f((1.9, 0.0, 0.5), 0.1, normal=n, nb=0.2) == 1.0
    # ... and the offset moves the lookup: from texel (2, 1) to texel (1, 1) of layer 0, N.L = 0 -> bias 0.005
    assert np.isclose(f((0.5, 0.0, -0.5), 0.1, normal=(-1.0, 0.0, 0.0), nb=1.0), 8 / 9)
    assert scenes.csm_select(splits, np.float32([0.1, 0.2, 0.21, 0.4, 0.5, 0.6, 0.61])).tolist() == [0, 0, 1, 1, 2, 2, 3]


def test_csm_model_equals_pcf_with_equal_cascades(scenes):
    """All four matrices and layers equal, ShadowStrength 1: csm_factor is pcf_factor at the normal-offset position."""
    rng = np.random.default_rng(7)
    layer = np.where(rng.random((16, 16)) < 0.5, 0.3, 1.0).astype(np.float32)
    ls = scenes.light_space_matrix((0.3, -1.0, 0.2), half_extent=3.0)
    pos = rng.uniform(-3.5, 3.5, size=(500, 3)) * np.array([1.0, 0.1, 1.0])
    n = np.array([0.0, 1.0, 0.0])
    L = -np.array([0.3, -1.0, 0.2]) / np.linalg.norm([0.3, -1.0, 0.2])
    clip_depth = rng.random(500).astype(np.float32)
    s = scenes.csm_factor(np.stack([layer] * 4), [ls] * 4, [0.25, 0.5, 0.75], pos, n, L, clip_depth, 0.005, 0.05, 16.0)
    off = pos + n * 0.05
    clip = np.concatenate([off, np.ones((500, 1))], axis=1) @ ls.astype(np.float64)
    u, v, z = clip[:, 0] * 0.5 + 0.5, 1.0 - (clip[:, 1] * 0.5 + 0.5), clip[:, 2]
    inside = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1) & (z >= 0) & (z <= 1)
    bias = max(0.005 * (1.0 - float(n @ L)), 0.0005)
    want = np.where(inside, scenes.pcf_factor(layer, u, v, z - bias, texel=(1 / 16.0, 1 / 16.0)), 1.0)
    assert inside.sum() > 200 and (~inside).sum() > 20
    assert np.array_equal(s, want)


def test_csm_cascades_enclose_their_slices(scenes):
    view, proj, _ = scenes.default_camera(480, 360, eye=scenes.CASCADED_GROUND_EYE, target=scenes.CASCADED_GROUND_TARGET)
    near, far = scenes.CASCADED_GROUND_RANGE
    for lam in (0.0, 0.6, 1.0):
        cas = scenes.csm_cascades(view, proj, scenes.CASCADED_GROUND_LIGHT, near, far, lam=lam)
        d = cas.distances
        assert d[0] == near and abs(d[-1] - far) < 1e-9 and np.all(np.diff(d) > 0)
        assert np.all(np.diff(cas.split_depths.astype(np.float64)) > 0), "split depths must increase strictly"
        p = proj.astype(np.float64)
        want = np.array([(p[2, 2] * -x + p[3, 2]) / x for x in d[1:]])
        assert np.allclose(cas.split_depths, want, rtol=0, atol=1e-7)
        # ... which is what the camera gives a point at that view distance
        vp = scenes.mat_mul(proj, view).astype(np.float64)
        inv_view = np.linalg.inv(view.astype(np.float64).T)
        for k in range(3):
            c = (inv_view @ np.array([0.3, -0.2, -d[k + 1], 1.0])) @ vp
            assert abs(c[2] / c[3] - float(cas.split_depths[k])) < 1e-6
        for k in range(4):
            c = np.concatenate([cas.corners[k], np.ones((8, 1))], axis=1) @ cas.matrices[k].astype(np.float64)
            assert np.allclose(c[:, 3], 1.0)
            assert np.all(np.abs(c[:, 0]) <= 1 + 1e-6) and np.all(np.abs(c[:, 1]) <= 1 + 1e-6), (lam, k)
            assert np.all(c[:, 2] >= -1e-6) and np.all(c[:, 2] <= 1 + 1e-6), (lam, k)
        i = np.arange(1, 5) / 4
        if lam == 0.0:
            assert np.allclose(d[1:], near + (far - near) * i)
        if lam == 1.0:
            assert np.allclose(d[1:], near * (far / near) ** i)


def test_pattern_input_satisfies_its_conditions(scenes, oracle):
    """The conditions test_gpu_csm.py asserts before it compares a single pixel, on the same oracle data."""
    expect, splits, facts = csm_cases.pattern_expectation(scenes, oracle, csm_cases.pattern_layers())
    csm_cases.assert_pattern_conditions(facts)
    assert np.all(np.diff(splits) > 0) and expect.shape == (2 * csm_cases.PATTERN_LAYER, 2 * csm_cases.PATTERN_LAYER, 3)


def test_cascaded_ground_case_satisfies_its_conditions(scenes, oracle):
    """Class sizes of the end-to-end scene: at least 300 pixels inside and outside the footprints in every cascade, at most a quarter of
    the ground pixels in neither class."""
    scene = scenes.cascaded_ground_case()
    assert scene.cascades is not None and len(scene.cascades.casters) == 4 and len(scene.cascades.params) == 336
    assert all(len(layer) == 5 for layer in scene.cascades.casters)          # four boxes and the sphere, into every layer
    csm_cases.assert_ground_conditions(csm_cases.ground_classes(scenes, oracle, scene))


def test_existing_scenes_carry_no_cascades(scenes):
    for name, make in scenes.SMALL_CASES.items():
        assert make().cascades is None, name
    assert scenes.shadowed_ground_case().cascades is None
