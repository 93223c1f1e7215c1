"""Shared by tests/test_lighting_cpu.py and tests/test_gpu_lighting.py: the two small lit scenes (`sphere`, `ground`) every direct-lighting path of
MODEL / MODEL_FULL / MODEL_PBR is measured on, the float64 / float32 model frames of renderer_rs_amd.lighting for a prim-id image, the pixels left
out (the Blinn-Phong terminator), and the comparison of DESIGN.md 8d: err = max |X - M64| / max(|M64|, 1e-3 max |M64|) over RGB against
bound = max(8 E32, 1e-4), alpha within 1e-5.  E32 comes from the float32 model alone, never from the oracle or the GPU."""
import dataclasses
import functools
import math

import numpy as np

from ibl_shading_cases import bound_for, rel_err

NO_PRIM = 0xFFFFFFFF
W, H = 160, 120
ROUGHNESS = (0.0, 0.3, 1.0)
TERMINATOR = 1e-4                 # |N.L| below which a Blinn-Phong pixel is left out (specular appears at N.L > 0: lights.hlsli:108)
LEFT_OUT_CAP = 5e-3
ALPHA_TOL = 1e-5


def _S():
    from renderer_rs_amd import scenes
    return scenes


def _texture(rng, w, h, lo=0, hi=256, **kw):
    t = rng.integers(lo, hi, (h, w, 4), dtype=np.uint8)
    return _S().Texture(t, **kw)


def _normal_map(rng, w, h, **kw):
    t = np.zeros((h, w, 4), dtype=np.uint8)
    t[..., :2] = rng.integers(70, 186, (h, w, 2), dtype=np.uint8)
    t[..., 2] = rng.integers(200, 246, (h, w), dtype=np.uint8)
    t[..., 3] = 255
    return _S().Texture(t, **kw)


SPHERE_LIGHTS = dict(
    directional=dict(direction=(-0.3, -0.7, -0.6), intensity=1.1, color=(1.0, 0.96, 0.9)),
    points=(((1.25, 0.75, 1.55), 1.3, (0.5, 0.8, 1.0), 6.0),           # its radius ends inside the mesh
            ((-2.0, 1.0, 2.5), 9.0, (1.0, 0.6, 0.4), 5.0)),            # reaches all of it
    # (position, inner cos, direction -- NOT normalised --, outer cos, colour, intensity): both cone edges cross the mesh
    spots=(((0.5, 2.0, 3.0), 0.985, (-0.25 * 1.7, -1.0 * 1.7, -1.55 * 1.7), 0.955, (0.9, 1.0, 0.7), 14.0),
           ((-1.6, -0.6, 3.0), 0.996, (0.9 * 0.4, 0.3 * 0.4, -1.6 * 0.4), 0.988, (0.7, 0.6, 1.0), 12.0)),
)
GROUND_LIGHTS = dict(
    directional=dict(direction=(0.3, -1.0, -0.4), intensity=0.5, color=(1.0, 0.95, 0.85)),
    points=(((0.8, 1.2, -1.0), 3.0, (0.6, 0.8, 1.0), 7.0),),
    spots=(((-0.8, 2.5, 1.0), 0.94, (0.3 * 2.0, -1.0 * 2.0, -0.9 * 2.0), 0.86, (1.0, 0.9, 0.7), 16.0),),
)


def _light_blocks(L, extra_points=()):
    S = _S()
    points = tuple(L["points"]) + tuple(extra_points)
    return dict(light=S.light_ubo(num_point=len(points), num_spot=len(L["spots"]), **L["directional"]),
                point_lights=b"".join(S.point_light(*p) for p in points), spot_lights=b"".join(S.spot_light(*s) for s in L["spots"]))


@functools.lru_cache(maxsize=None)
def sphere(program, roughness=0.3, srgb=False, extra_points=()):
    """displaced_sphere(12, 9) under a non-uniformly scaled, rotated model matrix and an off-axis camera; uv spans about [-1.25, 1.75] x [-0.5, 1.5];
    tangent w = -1 on every second vertex.  MODEL_PBR: all five textures, none a power of two but the normal map, sRGB albedo and emissive,
    normalScale 0.7, alpha 0.9 and no cutoff.  MODEL_FULL: albedo and normal map, linear without chains (program set 2) or with an sRGB albedo
    (program set 4).  MODEL: the bare mesh."""
    S = _S()
    rng = np.random.default_rng(0x11C47)
    mesh = S.displaced_sphere(12, 9, W, H, seed=23).draws[0]
    verts = np.array(mesh.vertices, dtype=np.float32)
    verts[:, 6] = verts[:, 6] * 3.0 - 1.25
    verts[:, 7] = verts[:, 7] * 2.0 - 0.5
    verts[1::2, 11] = -1.0
    eye = (1.2, 0.9, 4.0)
    view, proj, cam = S.default_camera(W, H, eye=eye, target=(0.1, 0.0, 0.0))
    model = S.trs((1.3, 0.8, 1.1), S.quat_axis_angle((0.3, 1.0, 0.2), 0.7), (0.1, -0.05, 0.0))
    albedo = _texture(rng, 7, 5, 40, 256, srgb=True)
    albedo.rgba8[..., 3] = rng.integers(200, 256, (5, 7), dtype=np.uint8)
    normal = _normal_map(rng, 16, 16)
    mr, occ, emi = _texture(rng, 5, 9, 20, 256), _texture(rng, 4, 4, 100, 256), _texture(rng, 3, 8, srgb=True)
    common = dict(vertices=verts, stride=48, count=mesh.count, indices=mesh.indices, program=program, cull_mode=S.CULL_BACK, front_face=mesh.front_face,
                  camera=cam, object=S.object_ubo(model), **_light_blocks(SPHERE_LIGHTS, extra_points))
    if program == S.PROGRAM_MODEL:
        d = S.DrawSpec(**common)
    elif program == S.PROGRAM_MODEL_FULL:
        d = S.DrawSpec(material=S.material_ubo((0.9, 0.8, 0.7, 0.8), 0.0, roughness, 0.85),
                       albedo_map=dataclasses.replace(albedo, srgb=srgb), normal_map=normal, **common)
    else:
        d = S.DrawSpec(material=S.pbr_material_ubo((1.0, 0.9, 0.8, 0.9), 0.8, roughness, 0.9, normal_scale=0.7, emissive=(0.3, 0.2, 0.4), alpha_cutoff=0.0,
                                                   has_base_color=True, has_normal=True, has_metallic_roughness=True, has_occlusion=True, has_emissive=True),
                       albedo_map=albedo, normal_map=normal, metallic_roughness_map=mr, occlusion_map=occ, emissive_map=emi, **common)
    name = f"sphere {('TRIANGLE', 'MODEL', 'FULL', 'PBR')[program]}{' sRGB' if srgb else ''} r={roughness:g}{' +2 dark' if extra_points else ''}"
    return S.Scene(name, W, H, [d], clear_color=(0.05, 0.06, 0.08, 1.0))


@functools.lru_cache(maxsize=None)
def ground(program):
    """A quad from z = -12 to z = +6 under the camera: it crosses the near plane and w = 0.  uv (0..6, 0..13), tangent w = -1, mip-chained sRGB
    albedo, normal (not a power of two) and metallic-roughness textures, one point light whose radius ends on the quad and one spot light."""
    S = _S()
    rng = np.random.default_rng(0x6120D)
    quad = S._pack_vertex48(np.array([[-4, 0, 6], [4, 0, 6], [4, 0, -12], [-4, 0, -12]], dtype=np.float32),
                            np.tile(np.array([0, 1, 0], dtype=np.float32), (4, 1)),
                            np.array([[0, 0], [6, 0], [6, 13], [0, 13]], dtype=np.float32), np.tile(np.array([1, 0, 0, -1], dtype=np.float32), (4, 1)))
    idx = np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32)
    view, proj, cam = S.default_camera(W, H, eye=(0.3, 1.5, 3.0), target=(0.0, 0.2, -2.0))
    model = S.trs((1.0, 1.0, 1.0), S.quat_axis_angle((0.0, 1.0, 0.0), 0.2), (0.0, 0.0, 0.0))
    albedo, normal, mr = _texture(rng, 32, 32, 30, 256, mips=True, srgb=True), _normal_map(rng, 24, 20, mips=True), _texture(rng, 16, 16, 30, 256, mips=True)
    albedo.rgba8[..., 3] = 255
    common = dict(vertices=quad, stride=48, count=6, indices=idx, program=program, cull_mode=S.CULL_NONE, camera=cam, object=S.object_ubo(model),
                  albedo_map=albedo, normal_map=normal, **_light_blocks(GROUND_LIGHTS))
    if program == S.PROGRAM_MODEL_FULL:
        d = S.DrawSpec(material=S.material_ubo((0.9, 0.9, 0.8, 1.0), 0.0, 0.4, 0.9), **common)
    else:
        d = S.DrawSpec(material=S.pbr_material_ubo((0.9, 0.9, 0.8, 1.0), 0.7, 0.9, 0.8, normal_scale=1.3, emissive=(0.02, 0.03, 0.01),
                                                   has_base_color=True, has_normal=True, has_metallic_roughness=True),
                       metallic_roughness_map=mr, **common)
    return S.Scene(f"ground {('TRIANGLE', 'MODEL', 'FULL', 'PBR')[program]}", W, H, [d], clear_color=(0.2, 0.3, 0.5, 1.0))


def all_cases():
    """Every case / program / roughness of the plain route, in a fixed order."""
    S = _S()
    out = [sphere(S.PROGRAM_MODEL_PBR, r) for r in ROUGHNESS]
    out += [sphere(S.PROGRAM_MODEL_FULL, r, srgb) for srgb in (False, True) for r in ROUGHNESS]
    out += [sphere(S.PROGRAM_MODEL), ground(S.PROGRAM_MODEL_PBR), ground(S.PROGRAM_MODEL_FULL)]
    return out


CASE_COUNT = 12


def case(i):
    return all_cases()[i]


# ---- the model's frames ----------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Model:
    py: np.ndarray
    px: np.ndarray
    m64: np.ndarray          # [n, 4]
    m32: np.ndarray
    keep: np.ndarray         # [n] bool: not within TERMINATOR of a Blinn-Phong terminator
    aux: dict

    @property
    def left_out(self):
        return 1.0 - float(self.keep.mean()) if self.keep.size else 0.0

    @property
    def e32(self):
        return rel_err(self.m32[self.keep, :3], self.m64[self.keep, :3])

    @property
    def bound(self):
        return bound_for(self.e32)


_models = {}


def model(scene, prim, ibl_zero_env=False, cache=True):
    """The float64 and float32 model frames of the lit pixels of a prim-id image, computed once per (scene, image) and left unchanged."""
    from renderer_rs_amd import lighting
    S = _S()
    key = (scene.name, hash(np.ascontiguousarray(prim).tobytes()), ibl_zero_env)
    if cache and key in _models:
        return _models[key]
    py, px, m64, aux = lighting.shade_frame(scene, prim, np.float64, ibl_zero_env=ibl_zero_env, want_aux=True)
    _, _, m32, _ = lighting.shade_frame(scene, prim, np.float32, ibl_zero_env=ibl_zero_env)
    keep = np.ones(py.size, dtype=bool)
    for di, a in aux["draws"].items():
        if scene.draws[di].program in (S.PROGRAM_MODEL, S.PROGRAM_MODEL_FULL):
            keep[a["sel"]] = ~np.any(a["lit"] & (np.abs(a["ndl"]) < TERMINATOR), axis=-1)
    m = Model(py, px, m64, m32.astype(np.float64), keep, aux)
    if cache:
        _models[key] = m
    return m


def measure(frame, m, mask=None):
    """(err over RGB, max |d alpha|, pixels compared) of an [H, W, 4] frame against M64 on the kept pixels (and inside `mask` [H, W])."""
    k = m.keep if mask is None else m.keep & mask[m.py, m.px]
    x = np.asarray(frame)[m.py[k], m.px[k]].astype(np.float64)
    if not k.any():
        return 0.0, 0.0, 0
    return rel_err(x[:, :3], m.m64[k, :3]), float(np.max(np.abs(x[:, 3] - m.m64[k, 3]))), int(k.sum())


def check(label, scene, prim, frame, who, ibl_zero_env=False, mask=None, min_pixels=1000):
    """Asserts the frame within the bound of the scene's model; prints and returns (E32, bound, err)."""
    m = model(scene, prim, ibl_zero_env)
    err, da, n = measure(frame, m, mask)
    print(f"LIGHT {label or scene.name}: pixels {n} left out {m.py.size - int(m.keep.sum())} E32 {m.e32:.3e} bound {m.bound:.3e} {who} {err:.3e} alpha {da:.1e}")
    assert m.left_out <= LEFT_OUT_CAP, f"{scene.name}: {m.left_out:.3%} of the covered pixels are left out"
    assert n >= min_pixels, f"{scene.name}: only {n} pixels compared"
    assert np.all(np.isfinite(m.m64))
    assert err <= m.bound, f"{label or scene.name}: {who} {err:.3e} > bound {m.bound:.3e} (E32 {m.e32:.3e})"
    assert da < ALPHA_TOL, f"{label or scene.name}: {who} alpha off by {da:.3e}"
    return m.e32, m.bound, err


def srgb8_oetf(linear):
    """The float64 sRGB OETF to bytes (round to nearest) of linear values, as a B8G8R8A8_SRGB store applies it to RGB."""
    c = np.clip(np.asarray(linear, dtype=np.float64), 0.0, 1.0)
    return np.rint(np.where(c <= 0.0031308, c * 12.92, 1.055 * np.power(c, 1.0 / 2.4) - 0.055) * 255.0)


def interior_mask(prim):
    """Pixels whose eight neighbours carry a primitive of the same quad (primitives 2 q and 2 q + 1) as they do."""
    q = np.where(prim == NO_PRIM, -1, prim.astype(np.int64) // 2)
    p = np.pad(q, 1, constant_values=-2)
    ok = q >= 0
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            ok &= p[dy:dy + q.shape[0], dx:dx + q.shape[1]] == q
    return ok
