"""Inputs shared by test_csm_cpu.py and test_gpu_csm.py: the pattern scene of the CSM term and the footprint classes of cascaded_ground_case,
with the conditions that depend on oracle output alone -- the CPU test evaluates them so that a GPU visit never discovers a badly chosen input."""
import dataclasses

import numpy as np

PATTERN_LAYER = 128           # texels per side of a layer; the frame has twice the resolution
PATTERN_E = 2.0               # half extent of the camera's (and cascade 0's) frustum
PATTERN_TILT = -0.5           # the receiver is y = PATTERN_TILT * x: tilted about the world z axis, depth grows from column to column
PATTERN_LOW = 0.25            # the pattern's low value (below every reachable dref); the other is 1.0
PATTERN_BIAS = 0.005


def _camera_from(vp, eye=(0.0, 10.0, 0.0)):
    z = np.zeros((4, 4), dtype=np.float32)
    return z.tobytes() + z.tobytes() + vp.astype(np.float32).tobytes() + np.array([*eye, 0.0], dtype=np.float32).tobytes()


PATTERN_EXTENTS = (1.0, 1.5, 2.0, 3.0)      # cascade k's half extent in units of e


def pattern_matrices(scenes):
    """Four lights that look straight down at the origin, half extents e, 1.5e, 2e, 3e.  With a half extent r * e a pixel centre lies at an
    odd multiple of 1 / (4r) texel (plus a whole number of texels when the layer size is a multiple of 2r, of thirds otherwise -- still odd
    multiples), so the distance of a tap from a texel boundary is at least 1/4, 1/6, 1/8 and 1/12 texel.  (Half extents e, 2e, 4e, 8e would put
    cascade 3's taps at odd multiples of 1/32 texel, short of the 1/16 texel the condition asks for: r may not exceed 4.)"""
    return [scenes.light_space_matrix((0.0, -1.0, 0.0), half_extent=PATTERN_E * r, near=0.1, far=20.0) for r in PATTERN_EXTENTS]


def pattern_layers(seed=20241):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((4, PATTERN_LAYER, PATTERN_LAYER)) < 0.85, 1.0, PATTERN_LOW).astype(np.float32)


def pattern_scene(scenes, intensity=3.0, cascades=None):
    """The tilted receiver seen through cascade 0's frustum at 2 x PATTERN_LAYER pixels; cascades: a CascadeSpec, or None for the oracle."""
    size, a = 2 * PATTERN_LAYER, PATTERN_TILT
    x0, z0 = 1.5 * PATTERN_E, 1.5 * PATTERN_E
    pos = np.array([[-x0, -a * x0, z0], [x0, a * x0, z0], [x0, a * x0, -z0], [-x0, -a * x0, -z0]], dtype=np.float64)
    n = np.array([-a, 1.0, 0.0]) / np.sqrt(1.0 + a * a)
    verts = scenes._pack_vertex48(pos, np.tile(n, (4, 1)), np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.float32),
                                  np.tile(np.array([1.0, 0.0, 0.0, 1.0]), (4, 1)))
    idx = np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32)
    light = scenes.light_ubo(direction=(0.0, -1.0, 0.0), intensity=intensity, color=(1.0, 0.9, 0.8))
    d = scenes.DrawSpec(vertices=verts, stride=48, count=6, indices=idx, program=scenes.PROGRAM_MODEL_PBR, cull_mode=scenes.CULL_NONE,
                        camera=_camera_from(pattern_matrices(scenes)[0]), object=scenes.object_ubo(np.eye(4, dtype=np.float32)), light=light,
                        material=scenes.pbr_material_ubo((0.7, 0.7, 0.7, 1.0), 0.0, 0.6))
    return scenes.Scene("csm-pattern", size, size, [d], cascades=cascades)


def pattern_splits(depth):
    """Three split depths: midpoints between the oracle depths of the columns on either side of a quarter of the frame."""
    w = depth.shape[1]
    cols = [w // 4, w // 2, 3 * w // 4]
    return np.array([0.5 * (float(depth[:, c - 1].max()) + float(depth[:, c].min())) for c in cols], dtype=np.float32)


def pattern_spec(scenes, splits):
    mats = pattern_matrices(scenes)
    return scenes.CascadeSpec([[], [], [], []], (PATTERN_LAYER, PATTERN_LAYER),
                              scenes.csm_ubo(mats, splits, PATTERN_BIAS, 0.0, float(PATTERN_LAYER)), load_op=scenes.LOAD_OP_LOAD)


def pattern_expectation(scenes, oracle, layers):
    """(expected RGB frame, splits, facts) from oracle frames and the numpy model; `facts` holds what the conditions are asserted on."""
    size, e, a = 2 * PATTERN_LAYER, PATTERN_E, PATTERN_TILT
    lit = oracle.render(pattern_scene(scenes), want_bgra8=False)
    unlit = oracle.render(pattern_scene(scenes, intensity=0.0), want_bgra8=False)["rgba"]
    depth = lit["depth"]
    assert (lit["prim"] != 0xFFFFFFFF).all(), "the receiver must fill the frame"
    splits = pattern_splits(depth)
    px, py = np.meshgrid(np.arange(size) + 0.5, np.arange(size) + 0.5, indexing="xy")
    x = e * (px / size * 2 - 1)
    z = -e * (py / size * 2 - 1)             # the light's up vector is -z and clip y is not flipped: the top row is ndc y = -1
    world = np.stack([x, a * x, z], axis=-1)
    n = np.array([-a, 1.0, 0.0]) / np.sqrt(1.0 + a * a)
    mats = pattern_matrices(scenes)
    s = scenes.csm_factor(layers, mats, splits, world, n, (0.0, 1.0, 0.0), depth, PATTERN_BIAS, 0.0, float(PATTERN_LAYER))
    idx = scenes.csm_select(splits, depth)
    # the figures the conditions are about
    split_gap = float(np.abs(depth.astype(np.float64)[..., None] - splits.astype(np.float64)).min())
    frac, dref_gap = 1.0, np.inf
    p4 = np.concatenate([world, np.ones(world.shape[:-1] + (1,))], axis=-1)
    ab = max(PATTERN_BIAS * (1.0 - float(n[1])), 0.0005)
    for k in range(4):
        clip = p4 @ mats[k].astype(np.float64)
        u, v, zk = clip[..., 0] * 0.5 + 0.5, 1.0 - (clip[..., 1] * 0.5 + 0.5), clip[..., 2]
        sel = idx == k
        for off in (-1, 0, 1):
            for t in ((u + off / PATTERN_LAYER) * PATTERN_LAYER, (v + off / PATTERN_LAYER) * PATTERN_LAYER):
                f = np.abs(t[sel] - np.round(t[sel]))
                frac = min(frac, float(f.min()))
        dref = zk[sel] - ab
        dref_gap = min(dref_gap, float(np.abs(dref - PATTERN_LOW).min()), float(np.abs(dref - 1.0).min()))
    facts = dict(split_gap=split_gap, tap_gap=frac, dref_gap=dref_gap, share=[float((idx == k).mean()) for k in range(4)],
                 below=[bool((s[idx == k] < 1.0).any()) for k in range(4)], full=[bool((s[idx == k] == 1.0).any()) for k in range(4)])
    expect = unlit[..., :3] + s[..., None] * (lit["rgba"][..., :3] - unlit[..., :3])
    return expect, splits, facts


def assert_pattern_conditions(facts):
    assert facts["split_gap"] > 1e-5, facts
    assert facts["tap_gap"] >= 1.0 / 16, facts
    assert facts["dref_gap"] > 1e-3, facts
    assert min(facts["share"]) >= 0.15, facts
    assert all(facts["below"]) and all(facts["full"]), facts


# ---- cascaded_ground_case: footprint classes ------------------------------------------------------------------------------------------
def _hull(pts):
    pts = sorted(set((round(float(p[0]), 9), round(float(p[1]), 9)) for p in pts))

    def cross(o, p, q):
        return (p[0] - o[0]) * (q[1] - o[1]) - (p[1] - o[1]) * (q[0] - o[0])
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return np.array(lower[:-1] + upper[:-1])               # counter-clockwise in (x, z)


def _hull_distances(hull, x, z):
    """(signed distance to the nearest edge line, positive inside; distance to the hull's boundary)."""
    inside_d, out_d = np.full(x.shape, np.inf), np.full(x.shape, np.inf)
    for k in range(len(hull)):
        p0, p1 = hull[k], hull[(k + 1) % len(hull)]
        e = p1 - p0
        n = np.array([-e[1], e[0]]) / np.linalg.norm(e)
        inside_d = np.minimum(inside_d, (x - p0[0]) * n[0] + (z - p0[1]) * n[1])
        tt = np.clip(((x - p0[0]) * e[0] + (z - p0[1]) * e[1]) / (e @ e), 0.0, 1.0)
        out_d = np.minimum(out_d, np.hypot(x - (p0[0] + tt * e[0]), z - (p0[1] + tt * e[1])))
    return inside_d, out_d


def ground_classes(scenes, oracle, scene, margin_texels=3.0):
    """Per ground pixel of cascaded_ground_case: the cascade it selects (from the oracle's depth), `inside` (more than margin_texels texels
    of that cascade inside a box's analytic footprint), `outside` (more than that outside every caster's footprint, the sphere's included),
    `ground`.  Pixels within 1e-5 of a split depth, and pixels under the sphere's (not exactly convex) footprint, belong to neither."""
    ref = oracle.render(dataclasses.replace(scene, cascades=None), want_bgra8=False)
    ground = ref["prim"] < 2
    h, w = ground.shape
    view, proj, _ = scenes.default_camera(w, h, eye=scenes.CASCADED_GROUND_EYE, target=scenes.CASCADED_GROUND_TARGET)
    cas = scenes.csm_cascades(view, proj, scenes.CASCADED_GROUND_LIGHT, *scenes.CASCADED_GROUND_RANGE, lam=scenes.CASCADED_GROUND_LAM)
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
    idx = scenes.csm_select(cas.split_depths, ref["depth"])
    size = scene.cascades.size[0]
    texel = np.array([2.0 * hk / size for hk in cas.half_extents]) * np.linalg.norm(d) / abs(d[1])
    margin = margin_texels * texel[idx]
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
        ind, outd = _hull_distances(_hull(pts), x, z)
        inside |= ind > margin
        outside &= (ind < 0) & (outd > margin)
    sphere = scene.draws[-1]
    sv = np.ascontiguousarray(sphere.vertices, dtype=np.float32).reshape(-1, 12)[:, :3].astype(np.float64)
    model = scenes.trs(*scenes.CASCADED_GROUND_SPHERE[:1], (0.0, 0.0, 0.0, 1.0), scenes.CASCADED_GROUND_SPHERE[1]).astype(np.float64)
    sw = np.concatenate([sv, np.ones((sv.shape[0], 1))], axis=1) @ model
    q = sw[:, :3] - d * (sw[:, 1:2] / d[1])
    ind, outd = _hull_distances(_hull(q[:, [0, 2]]), x, z)
    under_sphere = ~((ind < 0) & (outd > margin))
    inside &= ~under_sphere
    outside &= ~under_sphere
    keep = ground & ~near_split & np.isfinite(x)
    return dict(ground=ground, idx=idx, inside=inside & keep, outside=outside & keep, ref=ref, cascades=cas)


def assert_ground_conditions(c):
    g = int(c["ground"].sum())
    for k in range(4):
        sel = c["idx"] == k
        ni, no = int((c["inside"] & sel).sum()), int((c["outside"] & sel).sum())
        assert ni >= 300 and no >= 300, (k, ni, no)
    neither = int((c["ground"] & ~c["inside"] & ~c["outside"]).sum())
    assert neither <= 0.25 * g, (neither, g)
