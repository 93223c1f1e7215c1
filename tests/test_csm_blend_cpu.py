"""Cascade blending and stabilised cascades without a GPU: the float64 model of CalculateShadowCSMBlended (shadow_csm.hlsli:212-277) against closed
forms, the conditions of the inputs the GPU tests use (tests/csm_blend_cases.py), texel-snapped cascades over seeded camera poses, the bindings'
agreement on the new call, the raster variant a scope with a blended cascaded draw gets, and GetCascadeDebugColor on a depth image."""
import ctypes as C
import inspect
import itertools
import json
import math
import os
import re

import numpy as np
import pytest

import csm_blend_cases as cases
import csm_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGS_CSM, PROGS_CSM_BLEND, PROGS_IBL = 4 | 8 | 16, 4 | 8 | 16 | 256, 32


# ---- the model against closed forms ---------------------------------------------------------------------------------------------------------
def _flat_inputs(scenes, depth):
    """Samples at the origin under csm_cases' four lights that look straight down: every cascade holds them, the tap is the layer's centre."""
    depth = np.asarray(depth)
    world = np.zeros(depth.shape + (3,))
    return csm_cases.pattern_matrices(scenes), world, np.array([0.0, 1.0, 0.0]), (0.0, 1.0, 0.0)


def _constant_layers(values):
    return np.stack([np.full((8, 8), v, dtype=np.float32) for v in values])


def test_threshold_zero_is_csm_factor(scenes):
    layers = csm_cases.pattern_layers()
    mats = csm_cases.pattern_matrices(scenes)
    world, n = cases.pattern_world()
    depth = np.broadcast_to(np.linspace(0.45, 0.55, world.shape[1], dtype=np.float32), world.shape[:2])
    splits = np.array([0.475, 0.5, 0.525], dtype=np.float32)
    args = (layers, mats, splits, world, n, (0.0, 1.0, 0.0), depth, csm_cases.PATTERN_BIAS, 0.0, float(csm_cases.PATTERN_LAYER))
    plain = scenes.csm_factor(*args)
    assert np.array_equal(scenes.csm_factor_blended(*args, 0.0), plain)
    assert set(np.unique(scenes.csm_select(splits, depth)).tolist()) == {0, 1, 2, 3} and (plain < 1.0).any() and (plain == 1.0).any()
    assert not np.array_equal(scenes.csm_factor_blended(*args, 0.5), plain)


@pytest.mark.parametrize("frac", [0.25, 0.5, 0.75])
def test_blend_is_exact_on_two_constant_layers(scenes, frac):
    """Cascade 1 between splits 0.25 and 0.5, threshold 0.5: the region is 0.125 deep.  Layer 1 holds 1.0 (shadow = 1), layer 2 holds 0.0
    (nextShadow = 0): lerp(0, 1, blendFactor) is blendFactor itself, and every number here is a float32."""
    splits = np.array([0.25, 0.5, 0.75], dtype=np.float32)
    depth = np.array([0.5 - frac * 0.125], dtype=np.float32)
    mats, world, n, L = _flat_inputs(scenes, depth)
    got = scenes.csm_factor_blended(_constant_layers([0.5, 1.0, 0.0, 0.5]), mats, splits, world, n, L, depth, 0.005, 0.0, 8.0, 0.5)
    assert got.shape == (1,) and got[0] == frac
    # the other way round: 1 - blendFactor
    got = scenes.csm_factor_blended(_constant_layers([0.5, 0.0, 1.0, 0.5]), mats, splits, world, n, L, depth, 0.005, 0.0, 8.0, 0.5)
    assert got[0] == 1.0 - frac


def test_cascade_three_never_blends_and_cascade_zero_measures_from_zero(scenes):
    splits = np.array([0.5, 0.75, 0.875], dtype=np.float32)
    layers = _constant_layers([1.0, 0.0, 1.0, 0.0])
    depth = np.array([0.9, 0.95, 0.999, 1.0], dtype=np.float32)
    mats, world, n, L = _flat_inputs(scenes, depth)
    for thr in (0.1, 1.0):
        assert np.array_equal(scenes.csm_factor_blended(layers, mats, splits, world, n, L, depth, 0.005, 0.0, 8.0, thr), np.zeros(4))
        assert not scenes.csm_blend_terms(splits, depth, thr)[1].any()
    # cascade 0: prevSplit = 0, so the range is the split depth itself (0.5) and threshold 0.5 gives a region of 0.25
    depth = np.array([0.2, 0.25, 0.375, 0.4375], dtype=np.float32)
    mats, world, n, L = _flat_inputs(scenes, depth)
    idx, blending, dist, region = scenes.csm_blend_terms(splits, depth, 0.5)
    assert np.array_equal(idx, [0, 0, 0, 0]) and np.array_equal(region, np.full(4, 0.25, dtype=np.float32))
    assert np.array_equal(blending, [False, False, True, True])          # 0.25 is the edge itself: distanceToEdge < blendRegion fails
    got = scenes.csm_factor_blended(layers, mats, splits, world, n, L, depth, 0.005, 0.0, 8.0, 0.5)
    assert np.array_equal(got, [1.0, 1.0, 0.5, 0.25])


@pytest.mark.parametrize("k", [0, 1, 2])
def test_blend_is_continuous_at_both_ends_of_the_region(scenes, k):
    """In float64 depth arithmetic (the model's function of a real depth): entering the region at distanceToEdge = blendRegion the factor is 1 --
    the primary sample alone, as in front of the region --, leaving it at the split the factor is 0 -- the next cascade's sample, which is what
    the next cascade's pixels behind the split get.  |jump| < 1e-12."""
    splits = np.array([0.25, 0.5, 0.75], dtype=np.float32)
    layers = _constant_layers([0.0, 1.0, 0.0, 1.0])
    thr, eps = 0.5, 1e-14
    split, prev = float(splits[k]), float(splits[k - 1]) if k else 0.0
    region = (split - prev) * thr
    depth = np.array([split - region - eps, split - region + eps, split - eps, split + eps], dtype=np.float64)
    mats, world, n, L = _flat_inputs(scenes, depth)
    got = scenes.csm_factor_blended(layers, mats, splits, world, n, L, depth, 0.005, 0.0, 8.0, thr, depth_dtype=np.float64)
    idx, blending, _, _ = scenes.csm_blend_terms(splits, depth, thr, np.float64)
    assert np.array_equal(idx, [k, k, k, k + 1]) and np.array_equal(blending, [False, True, True, False])
    assert abs(got[1] - got[0]) < 1e-12 and abs(got[3] - got[2]) < 1e-12
    assert abs(got[0] - got[3]) == 1.0                                       # (the two ends are the two layers: there is something to be continuous about)


# ---- the pattern inputs ---------------------------------------------------------------------------------------------------------------------
def test_pattern_inputs_meet_their_conditions(scenes, oracle):
    expect, plain, splits, facts, depth = cases.pattern_expectation(scenes, oracle)
    print("blended pattern facts:", facts)
    cases.assert_blend_conditions(facts)
    assert expect.shape == (256, 256, 3) and not np.array_equal(expect, plain)


def test_ground_classes_of_the_stabilised_blended_frame(scenes, oracle):
    c = cases.ground_classes(scenes, oracle)
    print("stabilised ground classes:", [(int((c["inside"] & (c["idx"] == k)).sum()), int((c["outside"] & (c["idx"] == k)).sum())) for k in range(4)],
          "blending pixels:", int(c["blending"].sum()))
    cases.assert_ground_conditions(c)


# ---- stabilised cascades ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def posed(scenes):
    out = []
    for offset, yaw in cases.seeded_poses():
        view, proj, _, _ = cases.ground_view(scenes, offset=offset, yaw=yaw)
        out.append(cases.stable_cascades(scenes, view, proj))
    return out


def test_every_slice_lies_inside_its_cascade(posed):
    for cas in posed:
        for k in range(4):
            p4 = np.concatenate([cas.corners[k], np.ones((8, 1))], axis=1)
            clip = p4 @ cas.matrices[k].astype(np.float64)
            assert cas.matrices[k].dtype == np.float32 and np.all(clip[:, 3] == 1.0)
            assert np.all(np.abs(clip[:, :2]) < 1.0) and np.all(clip[:, 2] > 0.0) and np.all(clip[:, 2] < 1.0), (k, clip)


def test_radius_does_not_depend_on_the_pose(posed):
    for k in range(4):
        radii = {cas.half_extents[k] for cas in posed}
        assert len(radii) == 1, (k, radii)
        r = radii.pop()
        rq = r * (1.0 - 2.0 / cases.STABLE_MAP)                       # the quantised radius in front of the one-texel pad
        assert abs(rq * 16.0 - round(rq * 16.0)) < 1e-9 and r > rq
    assert all(np.array_equal(cas.split_depths, posed[0].split_depths) for cas in posed)
    assert posed[0].half_extents[0] < posed[0].half_extents[1] < posed[0].half_extents[2] < posed[0].half_extents[3]


def test_a_world_point_moves_by_whole_texels(posed):
    """u * map_size and v * map_size of a fixed world point, in float64 from the float32 matrices, differ between any two poses by a whole number
    to within 0.01: only the translation column depends on the pose; below 16 in magnitude it is rounded to float32 within 2^-20, which is
    2^-20 * map_size / 2 = 0.001 texel at 2048 -- the bound is ten times that."""
    points = np.array([[0.0, 0.0, 0.0, 1.0], [3.7, 0.0, -11.3, 1.0], [-1.6, 0.8, 1.5, 1.0], [17.25, 2.5, -40.0, 1.0]])
    worst = 0.0
    for k in range(4):
        t = np.array([cas.matrices[k][3, :3] for cas in posed], dtype=np.float64)
        assert np.abs(t[:, :2]).max() < 16.0, (k, np.abs(t).max())
        rot = np.array([cas.matrices[k][:3] for cas in posed])
        assert all(np.array_equal(r, rot[0]) for r in rot), "the rotation and scale entries do not depend on the pose"
        uv = np.array([(points @ cas.matrices[k].astype(np.float64))[:, :2] * 0.5 * cases.STABLE_MAP for cas in posed])      # (poses, points, 2)
        diff = uv[:, None] - uv[None, :]
        off = np.abs(diff - np.round(diff))
        worst = max(worst, float(off.max()))
        assert len({tuple(np.round(d).astype(np.int64).reshape(-1)) for d in diff[0]}) > 32, "the poses do differ"
    print("worst distance from a whole number of texels:", worst)
    assert worst <= 0.01


def test_matrices_change_in_texel_steps_only(scenes):
    """200 camera steps of 0.05 texel of cascade 0 along the light's x axis (10 texels of cascade 0 in all): cascade k's matrix takes at most
    ceil(10 texel_0 / texel_k) + 1 distinct values; the unstabilised matrices take 200."""
    axis = cases.light_x_axis(scenes)
    view, proj, _, _ = cases.ground_view(scenes)
    base = cases.stable_cascades(scenes, view, proj)
    texel = [2.0 * r / cases.STABLE_MAP for r in base.half_extents]
    seen, plain = [set() for _ in range(4)], [set() for _ in range(4)]
    for step in range(200):
        off = axis * (0.05 * texel[0] * step)
        view, proj, _, _ = cases.ground_view(scenes, offset=tuple(off))
        for k, m in enumerate(cases.stable_cascades(scenes, view, proj).matrices):
            seen[k].add(m.tobytes())
        for k, m in enumerate(cases.stable_cascades(scenes, view, proj, stabilize=False).matrices):
            plain[k].add(m.tobytes())
    counts = [len(s) for s in seen]
    print("distinct stabilised matrices over 200 steps:", counts)
    for k in range(4):
        assert 1 <= counts[k] <= math.ceil(10.0 * texel[0] / texel[k]) + 1, (k, counts)
        assert len(plain[k]) == 200, (k, len(plain[k]))
    assert counts[0] >= 10


def test_unstabilised_cascades_are_the_parents_bit_for_bit(scenes):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "csm_cascades_parent.json")))["cases"]
    assert len(golden) == 4
    for g in golden:
        view, proj, _ = scenes.default_camera(g["width"], g["height"], eye=tuple(g["eye"]), target=tuple(g["target"]))
        for kw in ({}, {"stabilize": False}, {"stabilize": False, "map_size": 512}):
            cas = scenes.csm_cascades(view, proj, tuple(g["light"]), g["near"], g["far"], lam=g["lam"], caster_margin=g["caster_margin"], **kw)
            for k in range(4):
                assert cas.matrices[k].dtype == np.float32
                assert cas.matrices[k].reshape(-1).view(np.uint32).tolist() == g["matrices"][k], (g["eye"], k)
            assert np.asarray(cas.split_depths, dtype=np.float32).view(np.uint32).tolist() == g["split_depths"]
            assert [float(h).hex() for h in cas.half_extents] == g["half_extents"]
    with pytest.raises(AssertionError, match="map_size"):
        scenes.csm_cascades(view, proj, (0.0, -1.0, 0.0), 1.0, 10.0, stabilize=True)


def test_ground_case_passes_the_new_arguments_on(scenes):
    plain, same = scenes.cascaded_ground_case(160, 120, map_size=256), scenes.cascaded_ground_case(160, 120, map_size=256, stabilize=False, blend_threshold=0.0)
    assert plain.cascades.params == same.cascades.params and plain.cascades.blend_threshold == 0.0
    st = cases.ground_scene(scenes)
    assert st.cascades.blend_threshold == 0.1 and st.cascades.params != plain.cascades.params
    assert st.cascades.params[64:68] == plain.cascades.params[64:68], "the split depths are unchanged"
    view, proj, _ = scenes.default_camera(160, 120, eye=scenes.CASCADED_GROUND_EYE, target=scenes.CASCADED_GROUND_TARGET)
    cas = cases.stable_cascades(scenes, view, proj, 256)
    assert st.cascades.params == scenes.csm_ubo(cas.matrices, cas.split_depths, 0.005, 0.01, 256.0)
    assert scenes.CascadeSpec([[], [], [], []]).blend_threshold == 0.0 and scenes.DrawSpec(vertices=np.zeros(1), stride=48, count=0).csm_blend is None


# ---- bindings -----------------------------------------------------------------------------------------------------------------------------------
def test_every_binding_carries_the_new_call(mirhi):
    name = "mirhi_cmd_bind_shadow_cascades_blended"
    header = open(os.path.join(ROOT, "include", "mirhi.h")).read()
    assert re.search(r"mirhi_result " + name + r"\(mirhi_cmd\* cmd, mirhi_image\* array, mirhi_buffer\* params,\s*uint64_t offset, uint64_t range, float blend_threshold\);", header)
    assert "#define MIRHI_ABI_VERSION 5u" in header
    res, args = mirhi._SIGNATURES[name]
    assert res is C.c_int32 and args == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_float]
    assert mirhi._SIGNATURES["mirhi_cmd_bind_shadow_cascades"][1] == args[:5]
    assert hasattr(C.CDLL(mirhi.LIB_PATH), name)
    sig = inspect.signature(mirhi.CommandBuffer.bind_shadow_cascades)
    assert sig.parameters["blend_threshold"].default == 0.0 and list(sig.parameters)[-1] == "blend_threshold"
    assert hasattr(mirhi.CommandBuffer, "bind_shadow_cascades_blended")
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "mirhi-sys", "src", "lib.rs")).read()
    assert ("pub fn " + name + "(cmd: *mut mirhi_cmd, array: *mut mirhi_image, params: *mut mirhi_buffer, offset: u64, range: u64, "
            "blend_threshold: f32) -> mirhi_result;") in sys_rs
    safe = open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", "command.rs")).read()
    assert "mirhi_sys::" + name + "(" in safe and "blend_threshold: f32" in safe
    hpp = open(os.path.join(ROOT, "renderer-rs_amd", "host", "mirhi.hpp")).read()
    assert name + "(" in hpp and "float blend_threshold" in hpp


# ---- the selector ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def choose(mirhi):
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_raster_choice
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]

    def choose(programs, zflip=0, tp=0, teams=1, wide=0, swz=1, allow=1, n_batch=0, pred=0):
        name, shape = C.create_string_buffer(96), (C.c_uint32 * 4)()
        rc = fn((C.c_uint32 * 12)(programs, allow, pred, zflip, 0xFFFFFFFF, tp, teams, wide, 0, swz, 0, n_batch), name, len(name), shape)
        return rc, name.value.decode(), tuple(shape)
    return choose


def test_the_new_bit_names_the_blended_kernels(choose):
    names = set()
    for ibl in (0, PROGS_IBL):
        for zflip, tp, teams, wide, allow in itertools.product((0, 0xFFFFFFFF), (0, 64), (1, 2), (0, 8, 16), (0, 1)):
            rc, name, shape = choose(PROGS_CSM_BLEND | ibl, zflip, tp, teams, wide, 1, allow)
            k, t = 1 if zflip else 0, 1 if tp else 0              # the plain key, the flipped (generic) key; no predicate form: a cascaded draw has none
            assert rc == 0 and name == (f"raster_kernel_ibl<{k}, {t}, 3>" if ibl else f"raster_kernel_csm_blend<{k}, {t}>"), name
            assert shape == (5, 4, 1, 256) == choose(PROGS_CSM | ibl, zflip, tp, teams, wide, 1, allow)[2]      # the shape of the CSM family
            assert choose(PROGS_CSM_BLEND | ibl, zflip, tp, teams, wide, 1, allow, n_batch=2)[0] == 1               # never batched
            names.add(name)
    assert len(names) == 8
    # without the bit: the kernels of before
    assert choose(PROGS_CSM)[1] == "raster_kernel_csm<0, 0>" and choose(PROGS_CSM | PROGS_IBL)[1] == "raster_kernel_ibl<0, 0, 2>"
    assert choose(12)[1].startswith("raster_kernel_shadow<") and choose(0)[1].startswith("raster_kernel_depth<")
    assert choose(64)[1] == "sky_kernel" and choose(4)[1].startswith("raster_kernel<4")


def _scope_plan(mirhi, draws, clear_depth=1.0):
    """mirhi_debug_scope_plan (tests/test_scope_plan_cpu.py) for LESS / test / write and draws of (program, shadow kind): (shadowed, programs, kernel)."""
    import struct
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_scope_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32]
    words = [1, 1, 1, 1, 0, 0, struct.unpack("<I", struct.pack("<f", clear_depth))[0], 0, 20, 12, 0, 0, 1, 1, len(draws)]
    for program, kind in draws:
        words += [program, kind, 0]
    inp, out, name = (C.c_uint32 * 27)(*(words + [0] * (27 - len(words)))), (C.c_uint32 * 32)(), C.create_string_buffer(96)
    assert fn(inp, out, name, len(name)) == 0
    return out[11], out[14], name.value.decode()


def test_scope_class_takes_the_value_three(mirhi, scenes):
    PBR, IBL = scenes.PROGRAM_MODEL_PBR, scenes.PROGRAM_MODEL_PBR_IBL
    assert _scope_plan(mirhi, [(PBR, 2)])[:2] == (2, PROGS_CSM) and _scope_plan(mirhi, [(PBR, 2)])[2].startswith("raster_kernel_csm<")
    for draws in ([(PBR, 3)], [(PBR, 2), (PBR, 3)], [(PBR, 3), (PBR, 2), (PBR, 0)]):          # blended and unblended cascaded draws share a scope
        shadowed, programs, kernel = _scope_plan(mirhi, draws)
        assert (shadowed, programs) == (3, PROGS_CSM_BLEND) and kernel.startswith("raster_kernel_csm_blend<"), (draws, shadowed, programs, kernel)
    shadowed, programs, kernel = _scope_plan(mirhi, [(IBL, 3), (PBR, 2)])
    assert (shadowed, programs) == (3, PROGS_CSM_BLEND | PROGS_IBL) and kernel.startswith("raster_kernel_ibl<") and kernel.endswith(", 3>")


# ---- GetCascadeDebugColor -----------------------------------------------------------------------------------------------------------------------
def test_debug_colours_follow_select_cascade(scenes):
    rng = np.random.default_rng(11)
    splits = np.array([0.3, 0.6, 0.9], dtype=np.float32)
    depth = rng.uniform(0.0, 1.0, (40, 30)).astype(np.float32)
    depth[0, :3] = splits                                              # a depth ON a split has not passed it
    col = scenes.csm_debug_colors(splits, depth)
    assert col.shape == (40, 30, 3) and col.dtype == np.float32
    idx = scenes.csm_select(splits, depth)
    table = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 0.0)]
    for k in range(4):
        assert (idx == k).any() and np.all(col[idx == k] == np.array(table[k], dtype=np.float32))
    assert np.array_equal(col[0, :3], np.array([table[0], table[1], table[2]], dtype=np.float32))
