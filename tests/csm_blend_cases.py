"""Inputs shared by test_csm_blend_cpu.py and test_gpu_csm_blend.py: the pattern scene of tests/csm_cases.py under CalculateShadowCSMBlended
(shadow_csm.hlsli:212-277), the poses of a camera that moves over cascaded_ground_case, and the footprint classes of its stabilised, blended
frame -- with the conditions that depend on the oracle or the float64 model alone, which the CPU test asserts so that a GPU visit never
discovers a badly chosen input."""
import dataclasses
import functools
import math

import numpy as np

import csm_cases

PATTERN_THRESHOLD = 0.5       # blendThreshold of the pattern tests: half of each cascade's split range blends


def pattern_world():
    """World positions (float64) and the normal of the pattern receiver's pixel centres (csm_cases.pattern_expectation's)."""
    size, e, a = 2 * csm_cases.PATTERN_LAYER, csm_cases.PATTERN_E, csm_cases.PATTERN_TILT
    px, py = np.meshgrid(np.arange(size) + 0.5, np.arange(size) + 0.5, indexing="xy")
    x = e * (px / size * 2 - 1)
    z = -e * (py / size * 2 - 1)
    return np.stack([x, a * x, z], axis=-1), np.array([-a, 1.0, 0.0]) / np.sqrt(1.0 + a * a)


@functools.lru_cache(maxsize=None)
def _pattern_frames(scenes, oracle):
    lit = oracle.render(csm_cases.pattern_scene(scenes), want_bgra8=False)
    unlit = oracle.render(csm_cases.pattern_scene(scenes, intensity=0.0), want_bgra8=False)["rgba"]
    assert (lit["prim"] != 0xFFFFFFFF).all(), "the receiver must fill the frame"
    return lit, unlit


@functools.lru_cache(maxsize=None)
def pattern_expectation(scenes, oracle, threshold=PATTERN_THRESHOLD):
    """(expected RGB frame, unblended expected RGB frame, splits, facts, oracle depth) of the pattern under `threshold`, computed once per run.
    facts: csm_cases' own (of the primary samples) plus what the blended conditions are asserted on."""
    layers = csm_cases.pattern_layers()
    _, splits, facts = csm_cases.pattern_expectation(scenes, oracle, layers)
    lit, unlit = _pattern_frames(scenes, oracle)
    depth = lit["depth"]
    world, n = pattern_world()
    mats = csm_cases.pattern_matrices(scenes)
    L, bias = (0.0, 1.0, 0.0), csm_cases.PATTERN_BIAS
    size = float(csm_cases.PATTERN_LAYER)
    s = scenes.csm_factor_blended(layers, mats, splits, world, n, L, depth, bias, 0.0, size, threshold)
    s0 = scenes.csm_factor(layers, mats, splits, world, n, L, depth, bias, 0.0, size)
    idx, blending, dist, region = scenes.csm_blend_terms(splits, depth, threshold)
    per = scenes.csm_cascade_samples(layers, mats, world, n, L, bias, 0.0, size)
    # taps into layer k + 1 of the pixels that select k: distance from a texel boundary, and of dref from the layer's two values
    p4 = np.concatenate([world, np.ones(world.shape[:-1] + (1,))], axis=-1)
    ab = max(bias * (1.0 - float(n[1])), 0.0005)
    next_tap_gap, next_dref_gap = 1.0, np.inf
    for k in range(3):
        clip = p4 @ mats[k + 1].astype(np.float64)
        u, v, zk = clip[..., 0] * 0.5 + 0.5, 1.0 - (clip[..., 1] * 0.5 + 0.5), clip[..., 2]
        sel = idx == k
        for off in (-1, 0, 1):
            for t in ((u + off / size) * size, (v + off / size) * size):
                next_tap_gap = min(next_tap_gap, float(np.abs(t[sel] - np.round(t[sel])).min()))
        dref = zk[sel] - ab
        next_dref_gap = min(next_dref_gap, float(np.abs(dref - csm_cases.PATTERN_LOW).min()), float(np.abs(dref - 1.0).min()))
        assert ((u[sel] > 0) & (u[sel] < 1) & (v[sel] > 0) & (v[sel] < 1)).all(), "the next cascade holds every pixel of this one"
    # distance of the blend decision from its two edges, in float32 units of the depth
    d64, r64 = dist.astype(np.float64), region.astype(np.float64)
    edge_gap = float(np.abs(d64 - r64)[idx < 3].min())
    facts = dict(facts, next_tap_gap=next_tap_gap, next_dref_gap=next_dref_gap, edge_gap=edge_gap,
                 region_share=[float((blending & (idx == k)).mean()) for k in range(3)],
                 region_differs=[bool((per[k + 1] != per[k])[blending & (idx == k)].any()) for k in range(3)],
                 blended_differs=int((s != s0).sum()))
    rgb = lambda f: unlit[..., :3] + f[..., None] * (lit["rgba"][..., :3] - unlit[..., :3])
    return rgb(s), rgb(s0), splits, facts, depth


def assert_blend_conditions(facts):
    csm_cases.assert_pattern_conditions(facts)
    assert facts["next_tap_gap"] >= 1.0 / 16, facts
    assert facts["next_dref_gap"] > 1e-3, facts
    assert facts["edge_gap"] > 1e-6, facts            # (no pixel sits on the edge of a blend region: 8 float32 steps of a depth near 0.5 and more)
    assert min(facts["region_share"]) >= 0.05, facts
    assert all(facts["region_differs"]), facts
    assert facts["blended_differs"] > 1000, facts


def pattern_spec(scenes, splits, threshold=PATTERN_THRESHOLD):
    return dataclasses.replace(csm_cases.pattern_spec(scenes, splits), blend_threshold=float(threshold))


# ---- a camera that moves over cascaded_ground_case -------------------------------------------------------------------------------------
STABLE_MAP = 2048


def ground_view(scenes, width=160, height=120, offset=(0.0, 0.0, 0.0), yaw=0.0):
    """(view, proj, eye, target) of cascaded_ground_case's camera translated by `offset` and turned by `yaw` about the world's y axis."""
    eye = np.array(scenes.CASCADED_GROUND_EYE, dtype=np.float64)
    fwd = np.array(scenes.CASCADED_GROUND_TARGET, dtype=np.float64) - eye
    c, s = math.cos(yaw), math.sin(yaw)
    fwd = np.array([c * fwd[0] + s * fwd[2], fwd[1], -s * fwd[0] + c * fwd[2]])
    eye = eye + np.asarray(offset, dtype=np.float64)
    target = eye + fwd
    view, proj, _ = scenes.default_camera(width, height, eye=tuple(eye), target=tuple(target))
    return view, proj, tuple(float(v) for v in eye), tuple(float(v) for v in target)


def seeded_poses(n=64, seed=20250):
    """n poses: translation in +-20 units on every axis but y (+-2: the camera stays above the ground), yaw in +-pi."""
    rng = np.random.default_rng(seed)
    return [((float(rng.uniform(-20, 20)), float(rng.uniform(-2, 2)), float(rng.uniform(-20, 20))), float(rng.uniform(-math.pi, math.pi))) for _ in range(n)]


def stable_cascades(scenes, view, proj, map_size=STABLE_MAP, stabilize=True):
    return scenes.csm_cascades(view, proj, scenes.CASCADED_GROUND_LIGHT, *scenes.CASCADED_GROUND_RANGE, lam=scenes.CASCADED_GROUND_LAM,
                               stabilize=stabilize, map_size=map_size if stabilize else None)


def light_x_axis(scenes):
    """The light's x axis in world space: the first basis vector of the stabilised cascades."""
    d = scenes._normalize(scenes.CASCADED_GROUND_LIGHT)
    return scenes.look_at_rh((0.0, 0.0, 0.0), d, (0.0, 1.0, 0.0)).astype(np.float64)[:3, 0]


# ---- footprint classes of the stabilised, blended ground frame ----------------------------------------------------------------------------
GROUND_ARGS = dict(width=160, height=120, map_size=256, stabilize=True, blend_threshold=0.1)
# The frame of the tests that check footprint CLASSES.  At 160 x 120 the boxes' footprints hold 298, 152, 114 and 194 ground pixels per cascade with no
# margin at all (92 .. 118 with the three texels), short of the 300 per cascade and class the classes are asked to hold; 320 x 240 is the
# smallest of 160 x 120, 240 x 180 (204 .. 267) and 320 x 240 (369 .. 537) that holds them.  The bit-equality tests keep 160 x 120.
CLASS_SIZE = dict(width=320, height=240)


def ground_scene(scenes, **over):
    a = dict(GROUND_ARGS, **over)
    return scenes.cascaded_ground_case(a.pop("width"), a.pop("height"), **a)


@functools.lru_cache(maxsize=None)
def ground_classes(scenes, oracle, margin_texels=3.0):
    """csm_cases.ground_classes for ground_scene: the same construction (analytic footprints of the boxes on the ground plane, the sphere's hull)
    with the stabilised cascades, and with each pixel's margin in texels of the COARSER of the cascades it samples -- the next cascade's where
    CalculateShadowCSMBlended takes the second sample."""
    scene = ground_scene(scenes, **CLASS_SIZE)
    ref = oracle.render(dataclasses.replace(scene, cascades=None), want_bgra8=False)
    ground = ref["prim"] < 2
    h, w = ground.shape
    view, proj, _ = scenes.default_camera(w, h, eye=scenes.CASCADED_GROUND_EYE, target=scenes.CASCADED_GROUND_TARGET)
    cas = stable_cascades(scenes, view, proj, GROUND_ARGS["map_size"])
    inv = np.linalg.inv(scenes.mat_mul(proj, view).T.astype(np.float64))
    px, py = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5, indexing="xy")
    nx, ny = px / w * 2 - 1, py / h * 2 - 1

    def unproject(zc):
        p = np.stack([nx, ny, np.full_like(nx, zc), np.ones_like(nx)], axis=-1) @ inv.T
        return p[..., :3] / p[..., 3:4]
    a, b = unproject(0.0), unproject(1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = a[..., 1] / (a[..., 1] - b[..., 1])
    hit = a + (b - a) * t[..., None]
    x, z = hit[..., 0], hit[..., 2]
    d = np.array(scenes.CASCADED_GROUND_LIGHT, dtype=np.float64)
    idx, blending, _, _ = scenes.csm_blend_terms(cas.split_depths, ref["depth"], GROUND_ARGS["blend_threshold"])
    coarse = np.where(blending, np.minimum(idx + 1, 3), idx)
    texel = np.array([2.0 * hk / GROUND_ARGS["map_size"] for hk in cas.half_extents]) * np.linalg.norm(d) / abs(d[1])
    margin = margin_texels * texel[coarse]
    near_split = np.abs(ref["depth"].astype(np.float64)[..., None] - cas.split_depths[:3].astype(np.float64)).min(axis=-1) <= 1e-5
    inside = np.zeros(ground.shape, dtype=bool)
    outside = np.ones(ground.shape, dtype=bool)
    for (cx, cy, cz), (hx, hy, hz) in scenes.cascaded_ground_boxes(scenes.CASCADED_GROUND_LAM):
        pts = []
        for sx in (-1, 1):
            for sy in (-1, 1):
                for sz in (-1, 1):
                    p = np.array([cx + sx * hx, cy + sy * hy, cz + sz * hz])
                    q = p - d * (p[1] / d[1])
                    pts.append((q[0], q[2]))
        ind, outd = csm_cases._hull_distances(csm_cases._hull(pts), x, z)
        inside |= ind > margin
        outside &= (ind < 0) & (outd > margin)
    sphere = scene.draws[-1]
    sv = np.ascontiguousarray(sphere.vertices, dtype=np.float32).reshape(-1, 12)[:, :3].astype(np.float64)
    model = scenes.trs(*scenes.CASCADED_GROUND_SPHERE[:1], (0.0, 0.0, 0.0, 1.0), scenes.CASCADED_GROUND_SPHERE[1]).astype(np.float64)
    sw = np.concatenate([sv, np.ones((sv.shape[0], 1))], axis=1) @ model
    q = sw[:, :3] - d * (sw[:, 1:2] / d[1])
    ind, outd = csm_cases._hull_distances(csm_cases._hull(q[:, [0, 2]]), x, z)
    under_sphere = ~((ind < 0) & (outd > margin))
    keep = ground & ~near_split & np.isfinite(x) & ~under_sphere
    return dict(ground=ground, idx=idx, blending=blending & ground, coarse=coarse, inside=inside & keep, outside=outside & keep, ref=ref, cascades=cas)


def assert_ground_conditions(c):
    for k in range(4):
        sel = c["idx"] == k
        ni, no = int((c["inside"] & sel).sum()), int((c["outside"] & sel).sum())
        assert ni >= 300 and no >= 300, (k, ni, no)
    assert int(c["blending"].sum()) >= 100, int(c["blending"].sum())
