"""Shared by tests/test_seamless_cpu.py and tests/test_gpu_seamless.py: the inputs of the seamless cube filtering checks (include/mirhi.h "The sampler",
DESIGN.md 8o), the conditions those inputs have to meet, and the planted errors the comparison has to notice.

The yardstick is renderer_rs_amd.ibl with seamless=True in float64; the metric and the bound are ibl_cases.err / ibl_cases.bound (max(8 E32, 1e-4), E32 from
the float32 run of the same model), lit frames use ibl_shading_cases.RGB_TOL.  No pixel is left out of any comparison: the seamless value is continuous, so
a float32 face flip costs nothing."""
import dataclasses
import functools
import math

import numpy as np

import ibl_cases
import ibl_shading_cases

W, H = 96, 64
SKY_SIZES = (1, 2, 4, 16)
# (yaw, pitch of scenes.sky_rotation, vertical field of view in degrees): a wide-angle camera that looks at the cube corner (1, 1, 1) -- at 120 degrees the
# three neighbouring corners come into the frame as well --, and one that looks along the middle of the edge between +X and +Y.  The fields of view are the
# ones at which a 96 x 64 frame of a 16^2 cube holds at least 8 corner-tap pixels (test_seamless_cpu.py asserts the counts): a corner tap needs a direction
# within half a texel of two edges at once, about one square degree per face at 16 texels.
POSES = {"corner": (-3.0 * math.pi / 4.0, math.asin(1.0 / math.sqrt(3.0)), 120.0), "edge": (-math.pi / 2.0, math.pi / 4.0, 65.0)}
VIEWPORT = (0.0, 0.0, float(W), float(H))
CLEAR = (0.01, 0.02, 0.03, 1.0)
ROUGHNESSES = (0.1, 0.5, 1.0)
IRR_SIZE, PRE_SIZE, PRE_LEVELS, LUT_SIZE = 8, 16, 5, 16
ENV_SIZE, ENV_LEVELS = 16, 5
PREFILTER_CASE = (16, 5, 64)         # size, levels, samples
IRRADIANCE_OUT = 8


def pkg():
    import __graft_entry__ as ge
    return ge.load_package()


def random_cube(n: int, seed: int, levels: int = 1):
    """`levels` levels of an n^2 cube, independent uniform values in [0, 1) (float32, alpha 1): no two neighbouring texels agree, so every wrong texel shows."""
    rng = np.random.default_rng(seed)
    out = []
    for l in range(levels):
        a = rng.random((6, n >> l, n >> l, 4)).astype(np.float32)
        a[..., 3] = 1.0
        out.append(a)
    return out


@functools.lru_cache(maxsize=None)
def sky_matrix(pose: str):
    s = pkg().scenes
    yaw, pitch, fov = POSES[pose]
    view = s.sky_rotation(yaw, pitch)
    proj = s.perspective_rh(math.radians(fov), W / H, 0.1, 100.0)
    m = s.inverse_view_projection(view, proj)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def sky_directions(pose: str):
    d = pkg().ibl.skybox_directions(sky_matrix(pose), VIEWPORT, W, H)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def sky_case(pose: str, n: int):
    """(levels, M64, M32) of one sky frame: a random n^2 cube under the pose, seamless."""
    m = pkg().ibl
    levels = random_cube(n, 100 + n)
    m64 = m.skybox(levels, sky_matrix(pose), VIEWPORT, W, H, np.float64, seamless=True)
    m32 = m.skybox(levels, sky_matrix(pose), VIEWPORT, W, H, np.float32, seamless=True)
    m64.setflags(write=False); m32.setflags(write=False)
    return levels, m64, m32


def tap_classes(n: int, d):
    """(has an edge tap, has a corner tap) per direction, by the model's own tap classification."""
    m = pkg().ibl
    face, s, t = m.select_face(np.asarray(d, dtype=np.float64))
    _, corner, edge, _, _ = m.seamless_taps(n, face, s, t)
    return np.any(edge, axis=0), np.any(corner, axis=0)


# ---- planted errors: the seamless lookup of one level with one thing wrong ---------------------------------------------------------------------
PLANTS = ("clamped", "wrong_face", "mirrored", "corner_is_one_tap", "corner_mean_of_four")


def planted_level(level, d, plant: str):
    """The float64 seamless lookup of `level` [6, n, n, C] along d, with the named error planted in it."""
    m = pkg().ibl
    level = np.asarray(level, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    if plant == "clamped":                      # clamping instead of crossing
        return m.sample_cube([level], d, 0.0, np.float64, seamless=False)
    n = level.shape[1]
    flat = level.reshape(-1, level.shape[-1])
    face, s, t = m.select_face(d)
    x, y = s * n - 0.5, t * n - 0.5
    i0, j0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    fx, fy = (x - np.floor(x))[..., None], (y - np.floor(y))[..., None]
    vals, corners = [], []
    for dj in (0, 1):
        for di in (0, 1):
            i, j = i0 + di, j0 + dj
            ox, oy = (i < 0) | (i > n - 1), (j < 0) | (j > n - 1)
            ic, jc = np.clip(i, 0, n - 1), np.clip(j, 0, n - 1)
            edge = ox ^ oy
            ti, tj = np.where(edge, i, ic), np.where(edge, j, jc)
            if plant == "mirrored":             # the position along the shared edge runs the wrong way
                ti, tj = np.where(edge & oy, n - 1 - ti, ti), np.where(edge & ox, n - 1 - tj, tj)
            f2, i2, j2 = m.edge_neighbour(n, face, ti, tj)
            if plant == "wrong_face":           # the texel of another face than the neighbour
                f2 = np.where(edge, (f2 + 1) % 6, f2)
            vals.append(flat[np.where(edge, (f2 * n + j2) * n + i2, (face * n + jc) * n + ic)])
            corners.append(ox & oy)
    for c in range(4):
        o = [vals[k] for k in range(4) if k != c]
        if plant == "corner_is_one_tap":        # one of the three instead of their mean
            v = o[0]
        elif plant == "corner_mean_of_four":    # a mean over four taps, the fourth the clamped in-face texel (a duplicate of one of the three)
            v = (o[0] + o[1] + o[2] + vals[c]) / 4.0
        else:
            v = (o[0] + o[1] + o[2]) / 3.0
        vals[c] = np.where(corners[c][..., None], v, vals[c])
    top = vals[0] * (1.0 - fx) + vals[1] * fx
    bot = vals[2] * (1.0 - fx) + vals[3] * fx
    return top * (1.0 - fy) + bot * fy


def one_level_seamless(levels, d, lod: float):
    """The sixth planted error: seamless applied to the lower of the two levels of a trilinear lookup only (float64)."""
    m = pkg().ibl
    l0 = int(math.floor(lod))
    f = lod - l0
    a = m.sample_cube([levels[l0]], d, 0.0, np.float64, seamless=True)
    b = m.sample_cube([levels[min(l0 + 1, len(levels) - 1)]], d, 0.0, np.float64, seamless=False)
    return a * (1.0 - f) + b * f


# ---- MODEL_PBR_IBL: scenes.ibl_facets_case (the scene ibl_shading_cases models: N constant per quad and known) at one roughness ---------------------
# The quads' (made-up) normals: scenes.IBL_FACETS keeps every normal well inside a face, where an 8^2 irradiance cube has no tap to cross with.  Here six lie
# within half an irradiance texel of a face edge, three of a cube corner, three inside a face (unnormalised; the two largest components' ratio says which).
FACET_NORMALS = ((1.0, 0.95, 0.1), (-1.0, 0.3, 0.97), (0.2, 1.0, -0.93), (0.96, -1.0, 0.3), (0.3, 0.97, 1.0), (-0.98, 0.1, -1.0),
                 (1.0, 0.95, 0.93), (-0.94, -1.0, 0.96), (0.97, -0.93, -1.0), (0.9, 0.3, 0.25), (-0.3, 0.2, -0.85), (0.25, 0.3, 0.9))


def ibl_set(seed: int = 7):
    """Random cubes for the set (irradiance 8^2, prefiltered 16^2 x 5) and the LUT of scenes.ibl_test_images."""
    s = pkg().scenes
    spec = s.ibl_test_images(PRE_SIZE, PRE_LEVELS, IRR_SIZE, LUT_SIZE)
    return s.IblSpec(irradiance=random_cube(IRR_SIZE, seed)[0], prefiltered=random_cube(PRE_SIZE, seed + 1, PRE_LEVELS), lut=spec.lut)


@functools.lru_cache(maxsize=None)
def facets_scene(roughness: float):
    """ibl_facets_case (unlit: colour = ambient + emissive) at W x H with every quad's roughness replaced and the random set of ibl_set()."""
    s = pkg().scenes
    base = s.ibl_facets_case(W, H)
    draws, facets = [], []
    for d, f, nrm in zip(base.draws, base.facets, FACET_NORMALS):
        mat = np.frombuffer(d.material, dtype=np.float32).copy()
        mat[5] = roughness                       # pbr_material_ubo: base colour (4), metallic, roughness, ao, normal scale
        verts = np.array(d.vertices, dtype=np.float32).reshape(4, 12)      # position, normal, uv, tangent
        n = np.asarray(nrm, dtype=np.float64)
        verts[:, 3:6] = (n / np.linalg.norm(n)).astype(np.float32)
        draws.append(dataclasses.replace(d, material=mat.tobytes(), vertices=verts))
        facets.append(dict(f, roughness=float(np.float32(roughness)), normal=verts[0, 3:6].copy()))
    scene = dataclasses.replace(base, draws=draws, ibl=ibl_set())
    scene.facets = facets
    scene.view, scene.proj, scene.eye = base.view, base.proj, base.eye
    return scene


def expected_ambient(scene, images, py, px, facet, dtype, irradiance_seamless: bool, prefiltered_seamless: bool):
    """ambient + emissive of the listed pixels (ibl_shading_cases.surface gives N, V and the material), each cube under its own state."""
    s = ibl_shading_cases.surface(scene, py, px, facet, dtype)
    irr, pre, lut = images
    a = pkg().ibl.ambient(irr, pre, lut, s["N"], s["V"], s["albedo"], s["metallic"], s["roughness"], s["ao"], dtype,
                          irradiance_seamless=irradiance_seamless, prefiltered_seamless=prefiltered_seamless)
    return a.astype(np.float64) + s["emissive"].astype(np.float64), s


def prefiltered_lods(scene, facet):
    """lod = clamp(max(roughness, 0.04) * 7, 0, levels - 1) of the listed facets' pixels."""
    r = np.array([f["roughness"] for f in scene.facets], dtype=np.float64)[facet]
    return np.clip(np.maximum(r, 0.04) * 7.0, 0.0, PRE_LEVELS - 1.0)


# ---- precompute: a seamless 16^2 environment with its chain ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def environment():
    m = pkg().ibl
    level0 = random_cube(ENV_SIZE, 31)[0]
    return [np.asarray(l, dtype=np.float32) for l in m.cube_mips(level0, ENV_LEVELS, dtype=np.float32)]


@functools.lru_cache(maxsize=None)
def irradiance_models(seamless: bool):
    m = pkg().ibl
    return tuple(m.irradiance(environment(), IRRADIANCE_OUT, dtype=t, seamless=seamless) for t in (np.float64, np.float32))


@functools.lru_cache(maxsize=None)
def prefilter_models(seamless: bool):
    m = pkg().ibl
    size, levels, samples = PREFILTER_CASE
    return tuple(m.prefilter(environment(), size, levels, samples, dtype=t, seamless=seamless) for t in (np.float64, np.float32))


err, bound, packed = ibl_cases.err, ibl_cases.bound, ibl_cases.packed
