"""Synthetic scenes for the BASELINE.json configs and small parity cases.

Host-side data only: vertex/index streams in the reference's layouts
(`TriangleVertex` 24 B / `Vertex` 48 B, crates/rhi/src/vertex.rs:20-61,88-170; u32 indices,
crates/resources/src/model.rs:41) and uniform blocks in the HLSL layouts
(shaders/hlsl/vertex/model.hlsl:5-19, shaders/hlsl/lights.hlsli:17-55,
shaders/hlsl/pixel/model_full.hlsl:34-41).  Nothing here touches a GPU or the oracle.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

PROGRAM_TRIANGLE, PROGRAM_MODEL, PROGRAM_MODEL_FULL, PROGRAM_MODEL_PBR, PROGRAM_SHADOW, PROGRAM_MODEL_PBR_IBL, PROGRAM_SKYBOX = 0, 1, 2, 3, 4, 5, 6
LOAD_OP_LOAD, LOAD_OP_CLEAR = 0, 1
CULL_NONE, CULL_FRONT, CULL_BACK, CULL_FRONT_AND_BACK = 0, 1, 2, 3
FRONT_CCW, FRONT_CW = 0, 1
CMP_NEVER, CMP_LESS, CMP_EQUAL, CMP_LESS_OR_EQUAL, CMP_GREATER, CMP_NOT_EQUAL, CMP_GREATER_OR_EQUAL, CMP_ALWAYS = range(8)
# crates/rhi/src/pipeline.rs:411-448 BlendFactor, :452-476 BlendOp (reference enum order)
(BF_ZERO, BF_ONE, BF_SRC_COLOR, BF_ONE_MINUS_SRC_COLOR, BF_DST_COLOR, BF_ONE_MINUS_DST_COLOR, BF_SRC_ALPHA, BF_ONE_MINUS_SRC_ALPHA,
 BF_DST_ALPHA, BF_ONE_MINUS_DST_ALPHA, BF_CONSTANT_COLOR, BF_ONE_MINUS_CONSTANT_COLOR, BF_CONSTANT_ALPHA, BF_ONE_MINUS_CONSTANT_ALPHA,
 BF_SRC_ALPHA_SATURATE) = range(15)
BO_ADD, BO_SUBTRACT, BO_REVERSE_SUBTRACT, BO_MIN, BO_MAX = range(5)
# ColorBlendAttachment::alpha_blend() (pipeline.rs:518-529): (src colour, dst colour, colour op, src alpha, dst alpha, alpha op, write mask)
ALPHA_BLEND = (BF_SRC_ALPHA, BF_ONE_MINUS_SRC_ALPHA, BO_ADD, BF_ONE, BF_ZERO, BO_ADD, 0xF)

f32 = np.float32


# ------------------------------------------------------------------------------------------------
# PCG32 (O'Neill, XSH-RR 64/32) -- the seeded generator SURVEY 8d names for the synthetic inputs
# ------------------------------------------------------------------------------------------------
class PCG32:
    MULT = 6364136223846793005
    MASK = (1 << 64) - 1

    def __init__(self, seed: int, seq: int = 0xDA3E39CB94B95BDB):
        self.inc = ((seq << 1) | 1) & self.MASK
        self.state = 0
        self.next_u32()
        self.state = (self.state + seed) & self.MASK
        self.next_u32()

    def next_u32(self) -> int:
        old = self.state
        self.state = (old * self.MULT + self.inc) & self.MASK
        xorshifted = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        return ((xorshifted >> rot) | (xorshifted << ((-rot) & 31))) & 0xFFFFFFFF

    def uniform(self, n: int) -> np.ndarray:
        """n float64 values uniform in [0,1) with 32 random bits each."""
        out = np.empty(n, dtype=np.float64)
        for i in range(n):
            out[i] = self.next_u32() * (1.0 / 4294967296.0)
        return out


# ------------------------------------------------------------------------------------------------
# glam-style float32 matrix helpers (column-major, m[col, row] flattened col-major to 16 floats)
# restating crates/scene/src/camera.rs:110-142 and crates/resources/src/ubo.rs:109-117,243-259
# ------------------------------------------------------------------------------------------------
def _v(x):
    return np.asarray(x, dtype=f32)


def _normalize(v):
    v = _v(v)
    return (v / f32(math.sqrt(float(np.dot(v, v))))).astype(f32)


def perspective_rh(fovy, aspect, near, far) -> np.ndarray:
    s, c = f32(math.sin(0.5 * fovy)), f32(math.cos(0.5 * fovy))
    h = f32(c / s)
    w = f32(h / f32(aspect))
    r = f32(f32(far) / f32(f32(near) - f32(far)))
    m = np.zeros((4, 4), dtype=f32)  # m[col][row]
    m[0, 0] = w
    m[1, 1] = h
    m[2, 2] = r
    m[2, 3] = -1.0
    m[3, 2] = f32(r * f32(near))
    return m


def look_at_rh(eye, center, up) -> np.ndarray:
    eye, center, up = _v(eye), _v(center), _v(up)
    f = _normalize(center - eye)
    s = _normalize(np.cross(f, up).astype(f32))
    u = np.cross(s, f).astype(f32)
    m = np.zeros((4, 4), dtype=f32)
    m[0] = [s[0], u[0], -f[0], 0]
    m[1] = [s[1], u[1], -f[1], 0]
    m[2] = [s[2], u[2], -f[2], 0]
    m[3] = [-np.dot(eye, s), -np.dot(eye, u), np.dot(eye, f), 1]
    return m


def mat_mul(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """glam a * b for column-major [col,row] arrays."""
    return (b.astype(f32) @ a.astype(f32)).astype(f32)


def projection_vulkan(fovy, aspect, near, far) -> np.ndarray:
    p = perspective_rh(fovy, aspect, near, far)
    p[1, 1] = f32(-p[1, 1])  # camera.rs:135 Vulkan Y flip
    return p


def trs(scale, quat, translation) -> np.ndarray:
    x, y, z, w = [f32(q) for q in quat]
    x2, y2, z2 = x + x, y + y, z + z
    xx, xy, xz, yy, yz, zz = x * x2, x * y2, x * z2, y * y2, y * z2, z * z2
    wx, wy, wz = w * x2, w * y2, w * z2
    s = _v(scale)
    m = np.zeros((4, 4), dtype=f32)
    m[0] = [(1 - (yy + zz)) * s[0], (xy + wz) * s[0], (xz - wy) * s[0], 0]
    m[1] = [(xy - wz) * s[1], (1 - (xx + zz)) * s[1], (yz + wx) * s[1], 0]
    m[2] = [(xz + wy) * s[2], (yz - wx) * s[2], (1 - (xx + yy)) * s[2], 0]
    m[3] = [translation[0], translation[1], translation[2], 1]
    return m


def quat_axis_angle(axis, angle) -> np.ndarray:
    a = _normalize(axis)
    s = math.sin(0.5 * angle)
    return np.array([a[0] * s, a[1] * s, a[2] * s, math.cos(0.5 * angle)], dtype=f32)


def normal_matrix(model: np.ndarray) -> np.ndarray:
    m64 = model.astype(np.float64).T  # row-major maths matrix
    det = np.linalg.det(m64)
    if abs(det) < 1e-6:
        return np.eye(4, dtype=f32)
    inv_t = np.linalg.inv(m64).T  # maths matrix (row-major) of inverse-transpose
    return inv_t.T.astype(f32)  # back to [col,row]


def orthographic_rh(left, right, bottom, top, near, far) -> np.ndarray:
    """glam Mat4::orthographic_rh (depth 0 at near, 1 at far), [col,row] like perspective_rh."""
    rw, rh = f32(1.0 / (f32(right) - f32(left))), f32(1.0 / (f32(top) - f32(bottom)))
    r = f32(1.0 / (f32(near) - f32(far)))
    m = np.zeros((4, 4), dtype=f32)
    m[0, 0], m[1, 1], m[2, 2] = rw + rw, rh + rh, r
    m[3] = [-(f32(left) + f32(right)) * rw, -(f32(top) + f32(bottom)) * rh, r * f32(near), 1.0]
    return m


def light_space_matrix(direction, center=(0.0, 0.0, 0.0), half_extent: float = 6.0, near: float = 0.1, far: float = 25.0,
                       distance: float = 10.0) -> np.ndarray:
    """Orthographic light matrix of a directional light (projection * view, the convention of CameraData.viewProjection):
    looks along `direction` at `center` from `distance` away, a square frustum of +-half_extent."""
    d = _normalize(direction)
    up = (0.0, 1.0, 0.0) if abs(float(d[1])) < 0.99 else (0.0, 0.0, -1.0)
    eye = _v(center) - d * f32(distance)
    view = look_at_rh(eye, center, up)
    return mat_mul(orthographic_rh(-half_extent, half_extent, -half_extent, half_extent, near, far), view)


def flip_clip_y(m: np.ndarray) -> np.ndarray:
    """m with clip y negated (the Vulkan y flip projection_vulkan applies to a camera, camera.rs:135).  The shadow pass renders with
    flip_clip_y(L) into a plain viewport, so that map row j holds v = (j + 0.5) / H of the lookup's v = 1 - (y * 0.5 + 0.5) with
    ShadowParams.LightSpaceMatrix = L (shadow.hlsli:65-66)."""
    out = m.astype(f32).copy()
    out[:, 1] = -out[:, 1]
    return out


def shadow_constants_ubo(light_space: np.ndarray, model: np.ndarray) -> bytes:
    """ShadowConstants 128 B of the SHADOW program (vertex/shadow.hlsl:7-11): lightSpaceMatrix@0 model@64."""
    return light_space.astype(f32).tobytes() + model.astype(f32).tobytes()


def shadow_ubo(light_space: np.ndarray, bias: float = 0.005, normal_bias: float = 0.02, size=(2048, 2048), strength: float = 1.0) -> bytes:
    """ShadowParams 96 B (shaders/hlsl/shadow.hlsli:20-30): LightSpaceMatrix@0 ShadowBias@64 NormalBias@68 ShadowMapSize@72
    ShadowStrength@80, padding to 96."""
    out = (light_space.astype(f32).tobytes() + np.array([bias, normal_bias, size[0], size[1], strength, 0, 0, 0], dtype=f32).tobytes())
    assert len(out) == 96
    return out


def camera_ubo(view: np.ndarray, proj: np.ndarray, eye) -> bytes:
    """CameraData 208 B: view@0 projection@64 viewProjection@128 cameraPosition@192 (ubo.rs:64-117)."""
    vp = mat_mul(proj, view)
    return (view.astype(f32).tobytes() + proj.astype(f32).tobytes() + vp.tobytes()
            + _v(eye).tobytes() + f32(0).tobytes())


def object_ubo(model: np.ndarray) -> bytes:
    """ObjectData 128 B: model@0 normalMatrix@64 (ubo.rs:174-259)."""
    return model.astype(f32).tobytes() + normal_matrix(model).tobytes()


def light_ubo(direction=(0.0, -1.0, 0.0), intensity=0.0, color=(1.0, 1.0, 1.0), num_point=0, num_spot=0) -> bytes:
    """LightUBO 48 B in the HLSL layout (lights.hlsli:17-23,49-55): dir, intensity, colour, pad, counts."""
    return (_v(direction).tobytes() + f32(intensity).tobytes() + _v(color).tobytes() + f32(0).tobytes()
            + np.array([num_point, num_spot], dtype=np.uint32).tobytes() + np.zeros(2, dtype=f32).tobytes())


def material_ubo(base_color=(1.0, 1.0, 1.0, 1.0), metallic=0.0, roughness=0.5, ao=1.0) -> bytes:
    """MaterialData 32 B (model_full.hlsl:34-41; defaults crates/resources/src/material.rs:20-30)."""
    return _v(base_color).tobytes() + np.array([metallic, roughness, ao, 0.0], dtype=f32).tobytes()


def pbr_material_ubo(base_color=(1.0, 1.0, 1.0, 1.0), metallic=0.0, roughness=0.5, ao=1.0, normal_scale=1.0,
                     emissive=(0.0, 0.0, 0.0), alpha_cutoff=0.0, has_base_color=False, has_normal=False,
                     has_metallic_roughness=False, has_occlusion=False, has_emissive=False) -> bytes:
    """MaterialData 80 B of the Cook-Torrance program (pixel/model_pbr.hlsl:36-59)."""
    out = (_v(base_color).tobytes() + np.array([metallic, roughness, ao, normal_scale], dtype=f32).tobytes()
           + _v(emissive).tobytes() + f32(alpha_cutoff).tobytes()
           + np.array([has_base_color, has_normal, has_metallic_roughness, has_occlusion, has_emissive, 0, 0, 0],
                      dtype=np.int32).tobytes())
    assert len(out) == 80
    return out


def point_light(position, radius, color, intensity) -> bytes:
    """PointLight 32 B (lights.hlsli:27-33 == crates/scene/src/light.rs:31-42)."""
    return _v(position).tobytes() + f32(radius).tobytes() + _v(color).tobytes() + f32(intensity).tobytes()


def spot_light(position, inner_cos, direction, outer_cos, color, intensity) -> bytes:
    """SpotLight 48 B in the HLSL layout (lights.hlsli:37-45)."""
    return (_v(position).tobytes() + f32(inner_cos).tobytes() + _v(direction).tobytes() + f32(outer_cos).tobytes()
            + _v(color).tobytes() + f32(intensity).tobytes())


# ------------------------------------------------------------------------------------------------
# scene description shared by the oracle binding (tests/) and the product binding
# ------------------------------------------------------------------------------------------------
@dataclass
class Texture:
    rgba8: np.ndarray  # (h, w, 4) uint8
    mips: bool = False  # sampled trilinearly through a full mip chain (mirhi_image_generate_mips / mip_chain below)
    srgb: bool = False  # R8G8B8A8_SRGB: the RGB bytes are decoded to linear when sampled
    max_anisotropy: int = 1  # > 1 (at most 16, needs mips): anisotropic filtering (mirhi_image_set_max_anisotropy)
    # the rest of the sampler state (mirhi_image_set_sampler; the values of mirhi_address_mode, mirhi_sampler_filter, mirhi_mip_mode): all zero =
    # REPEAT / LINEAR / MIP_LINEAR, the only sampler the oracle has
    address_u: int = 0
    address_v: int = 0
    mag_filter: int = 0
    min_filter: int = 0
    mip_mode: int = 0

    @property
    def width(self):
        return int(self.rgba8.shape[1])

    @property
    def height(self):
        return int(self.rgba8.shape[0])


def mip_chain(rgba8: np.ndarray) -> List[np.ndarray]:
    """Full mip chain of an (h, w, 4) uint8 image, level 0 first: 2x2 box filter on the stored bytes, round half up, edge clamp
    for odd sizes -- the specification `mirhi_image_generate_mips` and the oracle's callers follow (include/mirhi.h)."""
    levels = [np.ascontiguousarray(rgba8, dtype=np.uint8)]
    while levels[-1].shape[0] > 1 or levels[-1].shape[1] > 1:
        src = levels[-1].astype(np.uint32)
        h, w = src.shape[:2]
        dh, dw = max(1, h >> 1), max(1, w >> 1)
        y0 = np.minimum(2 * np.arange(dh), h - 1); y1 = np.minimum(2 * np.arange(dh) + 1, h - 1)
        x0 = np.minimum(2 * np.arange(dw), w - 1); x1 = np.minimum(2 * np.arange(dw) + 1, w - 1)
        acc = src[y0][:, x0] + src[y0][:, x1] + src[y1][:, x0] + src[y1][:, x1]
        levels.append(((acc + 2) >> 2).astype(np.uint8))
    return levels


@dataclass
class DrawSpec:
    vertices: np.ndarray                  # uint8 bytes or structured float32 (n, stride/4)
    stride: int
    count: int                            # vertex_count or index_count
    indices: Optional[np.ndarray] = None  # uint16 / uint32
    first: int = 0
    vertex_offset: int = 0
    program: int = PROGRAM_TRIANGLE
    cull_mode: int = CULL_BACK            # pipeline.rs:661 default
    front_face: int = FRONT_CCW           # pipeline.rs:662 default
    depth_test: bool = True               # pipeline.rs:677-679 defaults
    depth_write: bool = True
    depth_compare: int = CMP_LESS
    viewport: Optional[tuple] = None      # (x, y, w, h, min_depth, max_depth); None = full extent, 0..1
    scissor: Optional[tuple] = None       # (x, y, w, h); None = full extent
    camera: Optional[bytes] = None
    object: Optional[bytes] = None
    light: Optional[bytes] = None
    material: Optional[bytes] = None
    point_lights: bytes = b""
    spot_lights: bytes = b""
    albedo_map: Optional[Texture] = None
    normal_map: Optional[Texture] = None
    metallic_roughness_map: Optional[Texture] = None   # MODEL_PBR only (model_pbr.hlsl:62-95 t2..t4)
    occlusion_map: Optional[Texture] = None
    emissive_map: Optional[Texture] = None
    alpha_test: bool = False              # pipeline fragment_discard_enable: alpha-masked MODEL_PBR material (per-fragment discard)
    instances: int = 1                    # instance_count of the draw call: the same primitives again, instance after instance
    blend: Optional[tuple] = None         # None = opaque; else (src colour, dst colour, colour op, src alpha, dst alpha, alpha op, write mask)
    depth_bias: Optional[tuple] = None    # pipeline depth bias (constant_factor, clamp, slope_factor), pipeline.rs:781-788; None = off
    depth_clamp: bool = False             # pipeline depth_clamp_enable (pipeline.rs:769)
    csm_blend: Optional[float] = None     # a cascaded draw's own blend threshold (bind_shadow_cascades(..., blend_threshold=)); None = CascadeSpec.blend_threshold

    @property
    def textures(self):
        return (self.albedo_map, self.normal_map, self.metallic_roughness_map, self.occlusion_map, self.emissive_map)

    @property
    def index_type(self) -> int:
        if self.indices is None:
            return 0
        return 2 if self.indices.dtype == np.uint16 else 4

    @property
    def num_triangles(self) -> int:
        return (self.count // 3) * self.instances

    def vertex_bytes(self) -> np.ndarray:
        return np.ascontiguousarray(self.vertices).view(np.uint8).reshape(-1)


@dataclass
class ShadowSpec:
    """A depth-only shadow scope ahead of a scene's main scope: the casters are PROGRAM_SHADOW draws (camera =
    shadow_constants_ubo(flip_clip_y(L), model), viewport None = the map's extent), `params` the ShadowParams (LightSpaceMatrix L)
    every MODEL_PBR draw of the scene samples the map with."""
    casters: List[DrawSpec]
    size: tuple = (2048, 2048)
    params: bytes = b""
    clear_depth: float = 1.0
    load_op: int = LOAD_OP_CLEAR
    depth_bias: Optional[tuple] = None    # the map's pipelines: depth bias (constant_factor, clamp, slope_factor) of casters that set none themselves
    depth_clamp: bool = False             # ... and depth_clamp_enable ("pancaking": casters in front of the light's near plane stay in the map at depth 0)
    render_area: Optional[tuple] = None   # (x, y, w, h): the scope clears and draws this rectangle of the map only (a shadow atlas); None = all of it


@dataclass
class CascadeSpec:
    """Four depth-only shadow scopes ahead of a scene's main scope, one per layer of a D32 array (shadow_csm.hlsli:19 CASCADE_COUNT):
    casters[k] are the PROGRAM_SHADOW draws of layer k (camera = shadow_constants_ubo(flip_clip_y(M_k), model)), `params` the CSMParams
    (csm_ubo) every MODEL_PBR draw of the scene samples the array with."""
    casters: List[List[DrawSpec]]
    size: tuple = (1024, 1024)            # one layer's extent
    params: bytes = b""
    clear_depth: float = 1.0
    load_op: int = LOAD_OP_CLEAR
    depth_bias: Optional[tuple] = None    # the map's pipelines: depth bias (constant_factor, clamp, slope_factor) of casters that set none themselves
    depth_clamp: bool = False             # ... and depth_clamp_enable ("pancaking": casters in front of the light's near plane stay in the map at depth 0)
    blend_threshold: float = 0.0          # blendThreshold of CalculateShadowCSMBlended (bind_shadow_cascades(..., blend_threshold=)); 0: CalculateShadowCSM


@dataclass
class IblSpec:
    """The IBL set of a scene's MODEL_PBR_IBL draws (mirhi_cmd_bind_ibl): either three existing images (`images`: irradiance cube, prefiltered
    cube, BRDF LUT -- the caller's) or the arrays to upload: `irradiance` one level [6, n, n, 4], `prefiltered` a list of levels [6, m >> l, m >> l, 4],
    `lut` [k, k, 4] (float32; the layouts of renderer-rs_amd/ibl.py)."""
    irradiance: Optional[np.ndarray] = None
    prefiltered: Optional[list] = None
    lut: Optional[np.ndarray] = None
    images: Optional[tuple] = None

    def create_images(self, device, image_cls, lut_format: int = 2):
        """Three new images holding the arrays (the caller destroys them): (irradiance cube, prefiltered cube, LUT).  lut_format: the caller's
        R32G32B32A32_SFLOAT (mirhi_format; this module knows no Format class)."""
        from . import ibl as _ibl
        irr = image_cls.create_cube(device, int(self.irradiance.shape[1]), 1)
        irr.upload(_ibl.pack_cube([self.irradiance]))
        pre = image_cls.create_cube(device, int(self.prefiltered[0].shape[1]), len(self.prefiltered))
        pre.upload(_ibl.pack_cube(self.prefiltered))
        lut = image_cls(device, int(self.lut.shape[1]), int(self.lut.shape[0]), lut_format)
        lut.upload(np.ascontiguousarray(self.lut, dtype=np.float32))
        return irr, pre, lut


@dataclass
class SkySpec:
    """The sky of a scene (PROGRAM_SKYBOX, mirhi_cmd_bind_skybox): the environment cube -- `levels`, a list of [6, n >> l, n >> l, 4] float32
    arrays to upload, or `image`, an existing cube (the caller's) -- and inverseViewProjection ([col, row] float32, the push constants).
    Drawn after the scene's draws with LESS_OR_EQUAL and no depth write, as the reference intends; first=True: ahead of them."""
    inv_view_proj: np.ndarray
    levels: Optional[list] = None
    image: Optional[object] = None
    depth_test: bool = True
    depth_write: bool = False
    depth_compare: int = CMP_LESS_OR_EQUAL
    cull_mode: int = CULL_NONE
    front_face: int = FRONT_CCW
    viewport: Optional[tuple] = None      # (x, y, w, h, min_depth, max_depth); None = full extent, 0..1
    scissor: Optional[tuple] = None
    first: bool = False

    def create_image(self, device, image_cls):
        from . import ibl as _ibl
        img = image_cls.create_cube(device, int(self.levels[0].shape[1]), len(self.levels))
        img.upload(_ibl.pack_cube([np.asarray(l, dtype=np.float32) for l in self.levels]))
        return img


@dataclass
class Scene:
    name: str
    width: int
    height: int
    draws: List[DrawSpec] = field(default_factory=list)
    clear_color: tuple = (0.0, 0.0, 0.0, 1.0)  # rendering.rs:102-115 default
    clear_depth: float = 1.0                   # rendering.rs:356-370 default
    shadow: Optional[ShadowSpec] = None        # None: no shadow scope (the oracle's PBR frame: shadow = 1)
    cascades: Optional["CascadeSpec"] = None   # shadow cascades (shadow_csm.hlsli): four depth-only scopes ahead of the main scope; not with `shadow`
    ibl: Optional["IblSpec"] = None            # the IBL set of the scene's MODEL_PBR_IBL draws (mirhi_cmd_bind_ibl)
    sky: Optional["SkySpec"] = None            # the environment drawn behind the scene (PROGRAM_SKYBOX, mirhi_cmd_bind_skybox)
    render_area: Optional[tuple] = None        # (x, y, w, h): the main scope draws into this rectangle of its attachments only; None = full extent

    @property
    def num_triangles(self) -> int:
        return sum(d.num_triangles for d in self.draws)

    def algorithmic_bytes(self, bpp_out: int = 4) -> int:
        """Nv*stride + Ni*4 + W*H*bpp_out (+ texture bytes), summed over draws."""
        total = self.width * self.height * bpp_out
        seen = set()
        for d in self.draws:
            key = id(d.vertices)
            if key not in seen:
                seen.add(key)
                total += d.vertex_bytes().size
            if d.indices is not None and id(d.indices) not in seen:
                seen.add(id(d.indices))
                total += d.indices.size * d.indices.dtype.itemsize
            for t in d.textures:
                if t is not None and id(t) not in seen and t.rgba8.size > 4:
                    seen.add(id(t))
                    total += t.rgba8.size
        return total


# ------------------------------------------------------------------------------------------------
# C1: hello triangle (crates/renderer/src/renderer.rs:228-246,479-518)
# ------------------------------------------------------------------------------------------------
def hello_triangle(width: int = 256, height: int = 256) -> Scene:
    verts = np.array([
        [0.0, -0.5, 0.0, 1.0, 0.0, 0.0],   # top - red
        [-0.5, 0.5, 0.0, 0.0, 1.0, 0.0],   # bottom-left - green
        [0.5, 0.5, 0.0, 0.0, 0.0, 1.0],    # bottom-right - blue
    ], dtype=f32)
    d = DrawSpec(vertices=verts, stride=24, count=3, program=PROGRAM_TRIANGLE, cull_mode=CULL_NONE,
                 depth_test=False, depth_write=False)
    return Scene("C1-hello-triangle", width, height, [d], clear_color=(0.1, 0.1, 0.15, 1.0))


# ------------------------------------------------------------------------------------------------
# C2: N random flat-shaded triangles
# ------------------------------------------------------------------------------------------------
def random_triangles(n: int = 10000, width: int = 1920, height: int = 1080, seed: int = 0x5EED0002,
                     rmin: float = 4.0, rmax: float = 48.0) -> Scene:
    rng = PCG32(seed)
    u = rng.uniform(n * 10).reshape(n, 10)
    cx = u[:, 0] * 2.0 - 1.0
    cy = u[:, 1] * 2.0 - 1.0
    z = 0.05 + 0.9 * u[:, 2]
    r = rmin + (rmax - rmin) * u[:, 3]
    ang = u[:, 4:7] * (2.0 * math.pi)
    col = u[:, 7:10]
    verts = np.empty((n, 3, 6), dtype=f32)
    for k in range(3):
        verts[:, k, 0] = cx + r * np.cos(ang[:, k]) * (2.0 / width)
        verts[:, k, 1] = cy + r * np.sin(ang[:, k]) * (2.0 / height)
        verts[:, k, 2] = z
        verts[:, k, 3:6] = col
    d = DrawSpec(vertices=verts.reshape(n * 3, 6), stride=24, count=3 * n, program=PROGRAM_TRIANGLE,
                 cull_mode=CULL_NONE, depth_test=True, depth_write=True, depth_compare=CMP_LESS)
    return Scene(f"C2-random-{n}", width, height, [d], clear_color=(0.1, 0.1, 0.15, 1.0))


# ------------------------------------------------------------------------------------------------
# seeded value noise on a lattice (periodic in u), used by the C3/C4 stand-ins
# ------------------------------------------------------------------------------------------------
def _value_noise(u: np.ndarray, v: np.ndarray, seed: int, cells_u: int, cells_v: int, periodic_u: bool) -> np.ndarray:
    rng = PCG32(seed)
    lat = rng.uniform((cells_u + 1) * (cells_v + 1)).reshape(cells_v + 1, cells_u + 1)
    if periodic_u:
        lat[:, cells_u] = lat[:, 0]
    fu, fv = u * cells_u, v * cells_v
    iu = np.clip(np.floor(fu).astype(np.int64), 0, cells_u - 1)
    iv = np.clip(np.floor(fv).astype(np.int64), 0, cells_v - 1)
    au, av = fu - iu, fv - iv
    au = au * au * (3 - 2 * au)
    av = av * av * (3 - 2 * av)
    a = lat[iv, iu] * (1 - au) + lat[iv, iu + 1] * au
    b = lat[iv + 1, iu] * (1 - au) + lat[iv + 1, iu + 1] * au
    return a * (1 - av) + b * av


def _grid_indices(nu: int, nv: int) -> np.ndarray:
    """Two CCW (as seen from +normal with u to the right, v up) triangles per quad; (nu+1) verts per row."""
    j, i = np.meshgrid(np.arange(nv, dtype=np.uint32), np.arange(nu, dtype=np.uint32), indexing="ij")
    v00 = j * (nu + 1) + i
    v10 = v00 + 1
    v01 = v00 + (nu + 1)
    v11 = v01 + 1
    tris = np.stack([v00, v10, v11, v00, v11, v01], axis=-1)
    return tris.reshape(-1).astype(np.uint32)


def _smooth_normals(pos: np.ndarray, idx: np.ndarray) -> np.ndarray:
    p = pos.astype(np.float64)
    t = idx.reshape(-1, 3)
    fn = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    n = np.zeros_like(p)
    for k in range(3):
        np.add.at(n, t[:, k], fn)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    ln[ln == 0] = 1.0
    return n / ln


def _pack_vertex48(pos, nrm, uv, tan) -> np.ndarray:
    n = pos.shape[0]
    v = np.zeros((n, 12), dtype=f32)
    v[:, 0:3] = pos
    v[:, 3:6] = nrm
    v[:, 6:8] = uv
    v[:, 8:12] = tan
    return v


def default_camera(width: int, height: int, eye=(0.0, 0.0, 5.0), target=(0.0, 0.0, 0.0), fov_deg: float = 45.0):
    """Reference default camera (camera.rs:43-56): fov 45 deg, near 0.1, far 1000; aspect from the target."""
    view = look_at_rh(eye, target, (0.0, 1.0, 0.0))
    proj = projection_vulkan(math.radians(fov_deg), width / height, 0.1, 1000.0)
    return view, proj, camera_ubo(view, proj, eye)


WHITE_1X1 = Texture(np.full((1, 1, 4), 255, dtype=np.uint8))


# ------------------------------------------------------------------------------------------------
# C3: "bunny" stand-in -- displaced UV sphere, Phong + 1 point light
# ------------------------------------------------------------------------------------------------
def displaced_sphere(nu: int = 188, nv: int = 187, width: int = 1920, height: int = 1080,
                     seed: int = 0x5EED0003, program: int = PROGRAM_MODEL_FULL) -> Scene:
    uu, vv = np.meshgrid(np.linspace(0.0, 1.0, nu + 1), np.linspace(0.0, 1.0, nv + 1), indexing="xy")
    uu, vv = uu.reshape(-1), vv.reshape(-1)
    theta = uu * 2.0 * math.pi
    phi = (0.02 + 0.96 * vv) * math.pi  # keep a small hole at the poles: no degenerate fans
    rad = 1.0 + 0.12 * (_value_noise(uu, vv, seed, 12, 8, True) - 0.5) * 2.0
    pos = np.stack([rad * np.sin(phi) * np.cos(theta), rad * np.cos(phi), rad * np.sin(phi) * np.sin(theta)], axis=1)
    idx = _grid_indices(nu, nv)
    # orientation: make triangles CCW seen from outside
    t = idx.reshape(-1, 3)
    fn = np.cross(pos[t[0, 1]] - pos[t[0, 0]], pos[t[0, 2]] - pos[t[0, 0]])
    if np.dot(fn, pos[t[0, 0]]) < 0:
        idx = t[:, [0, 2, 1]].reshape(-1).astype(np.uint32)
    nrm = _smooth_normals(pos, idx)
    tan = np.stack([-np.sin(theta), np.zeros_like(theta), np.cos(theta), np.ones_like(theta)], axis=1)
    verts = _pack_vertex48(pos, nrm, np.stack([uu, vv], axis=1), tan)
    # camera: reference default eye (0,0,5) looking at the origin; sphere radius ~1 spans ~60 % of height
    view, proj, cam = default_camera(width, height, eye=(0.0, 0.0, 4.0))
    model = trs((1.0, 1.0, 1.0), quat_axis_angle((0.0, 1.0, 0.0), 0.6), (0.0, 0.0, 0.0))
    d = DrawSpec(vertices=verts, stride=48, count=idx.size, indices=idx, program=program,
                 cull_mode=CULL_BACK, front_face=FRONT_CCW,
                 camera=cam, object=object_ubo(model),
                 light=light_ubo(direction=(0.0, -1.0, 0.0), intensity=0.0, num_point=1),
                 material=material_ubo((0.7, 0.7, 0.7, 1.0), 0.0, 0.5, 1.0),
                 point_lights=point_light((2.0, 2.0, 2.0), 10.0, (1.0, 1.0, 1.0), 5.0),
                 albedo_map=WHITE_1X1, normal_map=WHITE_1X1)
    return Scene(f"C3-sphere-{idx.size // 3}", width, height, [d], clear_color=(0.1, 0.1, 0.15, 1.0))


# ------------------------------------------------------------------------------------------------
# C4: 1M-triangle height-field grid, fallback Blinn-Phong
# ------------------------------------------------------------------------------------------------
def heightfield_grid(nu: int = 1000, nv: int = 500, width: int = 3840, height: int = 2160,
                     seed: int = 0x5EED0004) -> Scene:
    uu, vv = np.meshgrid(np.linspace(0.0, 1.0, nu + 1), np.linspace(0.0, 1.0, nv + 1), indexing="xy")
    uu, vv = uu.reshape(-1), vv.reshape(-1)
    h = 0.15 * (_value_noise(uu, vv, seed, 40, 20, False) - 0.5)
    aspect = width / height
    pos = np.stack([(uu - 0.5) * 2.0 * aspect * 1.9, (vv - 0.5) * 2.0 * 1.9, h], axis=1)
    idx = _grid_indices(nu, nv)
    nrm = _smooth_normals(pos, idx)
    tan = np.tile(np.array([1.0, 0.0, 0.0, 1.0]), (pos.shape[0], 1))
    verts = _pack_vertex48(pos, nrm, np.stack([uu, vv], axis=1), tan)
    view, proj, cam = default_camera(width, height, eye=(0.0, 0.0, 5.0))
    model = trs((1.0, 1.0, 1.0), quat_axis_angle((1.0, 0.0, 0.0), -math.radians(30.0)), (0.0, 0.0, 0.0))
    d = DrawSpec(vertices=verts, stride=48, count=idx.size, indices=idx, program=PROGRAM_MODEL,
                 cull_mode=CULL_BACK, front_face=FRONT_CCW, camera=cam, object=object_ubo(model))
    return Scene(f"C4-grid-{idx.size // 3}", width, height, [d], clear_color=(0.1, 0.1, 0.15, 1.0))


# ------------------------------------------------------------------------------------------------
# C5: "Sponza" stand-in -- boxes in a hall, 4 point lights, 4 procedural textures
# ------------------------------------------------------------------------------------------------
def _procedural_texture(kind: int, size: int, seed: int) -> Texture:
    rng = PCG32(seed + kind)
    base = (rng.uniform(3) * 0.5 + 0.4)
    y, x = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    if kind % 2 == 0:   # checker
        m = (((x // (size // 16)) + (y // (size // 16))) & 1).astype(np.float64)
        val = 0.55 + 0.45 * m
    else:               # brick
        row = y // (size // 16)
        xo = (x + (row & 1) * (size // 16)) % (size // 8)
        mortar = ((y % (size // 16)) < 3) | (xo < 3)
        val = np.where(mortar, 0.35, 1.0)
    img = np.zeros((size, size, 4), dtype=np.uint8)
    for c in range(3):
        img[:, :, c] = np.clip(val * base[c] * 255.0 + 0.5, 0, 255).astype(np.uint8)
    img[:, :, 3] = 255
    return Texture(img)


def _box_mesh(center, half, sides=(8, 7), caps=(4, 4)):
    """Axis-aligned box, 4 side faces sides[0]*sides[1] quads + 2 caps caps[0]*caps[1] quads = 512 tris."""
    cx, cy, cz = center
    hx, hy, hz = half
    faces = [  # origin corner, u axis, v axis (u x v = outward normal), subdivision
        ((cx - hx, cy - hy, cz + hz), (2 * hx, 0, 0), (0, 2 * hy, 0), sides),   # +Z
        ((cx + hx, cy - hy, cz - hz), (-2 * hx, 0, 0), (0, 2 * hy, 0), sides),  # -Z
        ((cx + hx, cy - hy, cz + hz), (0, 0, -2 * hz), (0, 2 * hy, 0), sides),  # +X
        ((cx - hx, cy - hy, cz - hz), (0, 0, 2 * hz), (0, 2 * hy, 0), sides),   # -X
        ((cx - hx, cy + hy, cz + hz), (2 * hx, 0, 0), (0, 0, -2 * hz), caps),   # +Y
        ((cx - hx, cy - hy, cz - hz), (2 * hx, 0, 0), (0, 0, 2 * hz), caps),    # -Y
    ]
    vs, ids, base = [], [], 0
    for o, du, dv, (nu, nv) in faces:
        o, du, dv = np.array(o), np.array(du), np.array(dv)
        uu, vv = np.meshgrid(np.linspace(0, 1, nu + 1), np.linspace(0, 1, nv + 1), indexing="xy")
        uu, vv = uu.reshape(-1), vv.reshape(-1)
        pos = o[None, :] + uu[:, None] * du[None, :] + vv[:, None] * dv[None, :]
        n = np.cross(du, dv)
        n = n / np.linalg.norm(n)
        t = du / np.linalg.norm(du)
        nrm = np.tile(n, (pos.shape[0], 1))
        tan = np.tile(np.array([t[0], t[1], t[2], 1.0]), (pos.shape[0], 1))
        scale = max(np.linalg.norm(du), np.linalg.norm(dv))
        uv = np.stack([uu * np.linalg.norm(du) / scale * 2.0, vv * np.linalg.norm(dv) / scale * 2.0], axis=1)
        vs.append(_pack_vertex48(pos, nrm, uv, tan))
        ids.append(_grid_indices(nu, nv) + base)
        base += pos.shape[0]
    return np.concatenate(vs, axis=0), np.concatenate(ids).astype(np.uint32)


def box_hall(n_boxes: int = 512, width: int = 3840, height: int = 2160, seed: int = 0x5EED0005,
             tex_size: int = 1024) -> Scene:
    rng = PCG32(seed)
    u = rng.uniform(n_boxes * 6).reshape(n_boxes, 6)
    textures = [_procedural_texture(k, tex_size, seed) for k in range(4)]
    eye = (0.0, 2.5, 14.0)
    view, proj, cam = default_camera(width, height, eye=eye, target=(0.0, 2.0, 0.0), fov_deg=60.0)
    lights = b"".join([
        point_light((-8.0, 6.0, 4.0), 30.0, (1.0, 0.9, 0.8), 40.0),
        point_light((8.0, 6.0, 4.0), 30.0, (0.8, 0.9, 1.0), 40.0),
        point_light((0.0, 8.0, -4.0), 30.0, (1.0, 1.0, 1.0), 40.0),
        point_light((0.0, 2.0, 10.0), 30.0, (1.0, 1.0, 0.9), 30.0),
    ])
    model = np.eye(4, dtype=f32)
    obj = object_ubo(model)
    groups = [([], [], 0) for _ in range(4)]
    groups = [{"v": [], "i": [], "base": 0} for _ in range(4)]
    for b in range(n_boxes):
        c = ((u[b, 0] - 0.5) * 30.0, u[b, 1] * 10.0, (u[b, 2] - 0.5) * 15.0 - 2.0)
        hsz = (0.25 + 0.6 * u[b, 3], 0.25 + 0.9 * u[b, 4], 0.25 + 0.6 * u[b, 5])
        v, i = _box_mesh(c, hsz)
        g = groups[b % 4]
        g["v"].append(v)
        g["i"].append(i + g["base"])
        g["base"] += v.shape[0]
    draws = []
    for k, g in enumerate(groups):
        if not g["v"]:
            continue
        verts = np.concatenate(g["v"], axis=0)
        idx = np.concatenate(g["i"]).astype(np.uint32)
        draws.append(DrawSpec(vertices=verts, stride=48, count=idx.size, indices=idx, program=PROGRAM_MODEL_FULL,
                              cull_mode=CULL_BACK, front_face=FRONT_CCW, camera=cam, object=obj,
                              light=light_ubo(direction=(0.3, -1.0, 0.2), intensity=0.15, num_point=4),
                              material=material_ubo((1.0, 1.0, 1.0, 1.0), 0.0, 0.35 + 0.15 * k, 1.0),
                              point_lights=lights, albedo_map=textures[k], normal_map=WHITE_1X1))
    return Scene(f"C5-boxhall-{sum(d.num_triangles for d in draws)}", width, height, draws,
                 clear_color=(0.02, 0.02, 0.03, 1.0))


# ------------------------------------------------------------------------------------------------
# small parity cases (edge cases the domain has: clipping, culling, shared edges, depth ties, scissor)
# ------------------------------------------------------------------------------------------------
def _tri_verts(pts, cols=None) -> np.ndarray:
    pts = np.asarray(pts, dtype=f32).reshape(-1, 3)
    if cols is None:
        cols = np.tile(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=f32), (pts.shape[0] // 3 + 1, 1))[:pts.shape[0]]
    return np.concatenate([pts, np.asarray(cols, dtype=f32).reshape(-1, 3)], axis=1)


def shared_edge_fan(width: int = 160, height: int = 120, n: int = 24, seed: int = 7) -> Scene:
    """A fan of thin triangles sharing edges and a centre: every pixel must be covered exactly once
    (top-left rule), including along shared edges; no depth test so double hits would be visible."""
    rng = PCG32(seed)
    ang = np.sort(rng.uniform(n)) * 2 * math.pi
    pts, cols = [], []
    col = rng.uniform(3 * n).reshape(n, 3)
    for k in range(n):
        a0, a1 = ang[k], ang[(k + 1) % n]
        pts += [(0.013, -0.021, 0.5), (0.9 * math.cos(a0), 0.9 * math.sin(a0), 0.5), (0.9 * math.cos(a1), 0.9 * math.sin(a1), 0.5)]
        cols += [col[k]] * 3
    d = DrawSpec(vertices=_tri_verts(pts, cols), stride=24, count=3 * n, cull_mode=CULL_NONE, depth_test=False,
                 depth_write=False)
    return Scene("shared-edge-fan", width, height, [d])


def near_clip_case(width: int = 200, height: int = 150) -> Scene:
    """A ground quad through the camera: crosses the near plane and w=0 (exercises real clipping)."""
    q = 20.0
    pos = np.array([[-q, 0, q], [q, 0, q], [q, 0, -q], [-q, 0, -q]], dtype=f32)
    nrm = np.tile(np.array([0, 1, 0], dtype=f32), (4, 1))
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=f32)
    tan = np.tile(np.array([1, 0, 0, 1], dtype=f32), (4, 1))
    verts = _pack_vertex48(pos, nrm, uv, tan)
    idx = np.array([0, 1, 2, 0, 2, 3], dtype=np.uint16)
    view, proj, cam = default_camera(width, height, eye=(0.0, 1.0, 3.0), target=(0.0, 0.5, 0.0))
    d = DrawSpec(vertices=verts, stride=48, count=6, indices=idx, program=PROGRAM_MODEL, cull_mode=CULL_NONE,
                 camera=cam, object=object_ubo(np.eye(4, dtype=f32)))
    return Scene("near-clip-quad", width, height, [d], clear_color=(0.1, 0.1, 0.15, 1.0))


def depth_tie_case(width: int = 96, height: int = 64) -> Scene:
    """Coplanar overlapping triangles at identical depth: LESS keeps the earlier primitive."""
    pts = [(-0.8, -0.8, 0.5), (0.8, -0.8, 0.5), (0.0, 0.8, 0.5),
           (-0.8, 0.8, 0.5), (0.0, -0.8, 0.5), (0.8, 0.8, 0.5),
           (-0.5, -0.5, 0.25), (0.5, -0.5, 0.75), (0.0, 0.5, 0.5)]
    cols = [(1, 0, 0)] * 3 + [(0, 1, 0)] * 3 + [(0, 0, 1)] * 3
    d = DrawSpec(vertices=_tri_verts(pts, cols), stride=24, count=9, cull_mode=CULL_NONE)
    return Scene("depth-tie", width, height, [d])


def cull_scissor_case(width: int = 128, height: int = 96) -> Scene:
    """Back-face culling with default CCW front face + a scissor/viewport smaller than the target."""
    pts = [(-0.9, -0.9, 0.3), (-0.1, -0.9, 0.3), (-0.5, 0.9, 0.3),      # one winding
           (0.1, -0.9, 0.4), (0.5, 0.9, 0.4), (0.9, -0.9, 0.4)]         # the opposite winding
    d = DrawSpec(vertices=_tri_verts(pts), stride=24, count=6, cull_mode=CULL_BACK, front_face=FRONT_CCW,
                 viewport=(8.0, 4.0, 100.0, 80.0, 0.0, 1.0), scissor=(16, 8, 90, 60))
    return Scene("cull-scissor", width, height, [d], clear_color=(0.2, 0.3, 0.4, 1.0))


def multi_draw_case(width: int = 160, height: int = 128) -> Scene:
    """Two draws with different programs in one rendering scope + first_vertex / vertex_offset use."""
    s1 = random_triangles(40, width, height, seed=11, rmin=6, rmax=30).draws[0]
    s1.first = 6
    s1.count = 3 * 36
    sph = displaced_sphere(12, 9, width, height, seed=5, program=PROGRAM_MODEL).draws[0]
    pad = np.zeros((5, 12), dtype=f32)
    sph.vertices = np.concatenate([pad, sph.vertices], axis=0)
    sph.vertex_offset = 5
    sph.first = 3
    sph.count -= 6
    return Scene("multi-draw", width, height, [s1, sph], clear_color=(0.05, 0.05, 0.05, 1.0))


def huge_triangle_case(width: int = 192, height: int = 108) -> Scene:
    """Triangles far larger than the guard band and off-screen ones (guard-band clipping, trivial reject)."""
    pts = [(-300.0, -200.0, 0.5), (300.0, -250.0, 0.6), (10.0, 500.0, 0.4),
           (2.0, 2.0, 0.5), (3.0, 2.0, 0.5), (2.0, 3.0, 0.5),
           (-0.2, -0.2, 0.1), (0.3, -0.1, 0.1), (0.0, 0.4, 0.1)]
    d = DrawSpec(vertices=_tri_verts(pts), stride=24, count=9, cull_mode=CULL_NONE)
    return Scene("huge-triangle", width, height, [d])


def textured_quad_case(width: int = 160, height: int = 120) -> Scene:
    """model_full with a real albedo texture, a tangent-space normal map, a spot light and a point light."""
    pos = np.array([[-1.5, -1, 0], [1.5, -1, 0], [1.5, 1, 0], [-1.5, 1, 0]], dtype=f32)
    nrm = np.tile(np.array([0, 0, 1], dtype=f32), (4, 1))
    uv = np.array([[0, 0], [3, 0], [3, 2], [0, 2]], dtype=f32)
    tan = np.tile(np.array([1, 0, 0, 1], dtype=f32), (4, 1))
    verts = _pack_vertex48(pos, nrm, uv, tan)
    idx = np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32)
    albedo = _procedural_texture(1, 64, 99)
    rng = PCG32(123)
    nm = np.zeros((16, 16, 4), dtype=np.uint8)
    r = rng.uniform(16 * 16 * 2).reshape(16, 16, 2)
    nm[:, :, 0] = (128 + (r[:, :, 0] - 0.5) * 80).astype(np.uint8)
    nm[:, :, 1] = (128 + (r[:, :, 1] - 0.5) * 80).astype(np.uint8)
    nm[:, :, 2] = 230
    nm[:, :, 3] = 255
    view, proj, cam = default_camera(width, height, eye=(0.5, 0.3, 3.0))
    model = trs((1.0, 1.2, 1.0), quat_axis_angle((0.0, 1.0, 0.0), 0.5), (0.1, 0.0, 0.0))
    d = DrawSpec(vertices=verts, stride=48, count=6, indices=idx, program=PROGRAM_MODEL_FULL, cull_mode=CULL_NONE,
                 camera=cam, object=object_ubo(model),
                 light=light_ubo(direction=(0.2, -0.5, -1.0), intensity=0.4, color=(1.0, 0.95, 0.9), num_point=1, num_spot=1),
                 material=material_ubo((0.9, 0.8, 0.7, 0.5), 0.0, 0.3, 0.8),
                 point_lights=point_light((1.0, 1.0, 2.0), 8.0, (0.6, 0.7, 1.0), 4.0),
                 spot_lights=spot_light((-1.0, 0.5, 2.5), 0.95, (0.3, -0.1, -1.0), 0.8, (1.0, 0.8, 0.6), 6.0),
                 albedo_map=albedo, normal_map=Texture(nm))
    return Scene("textured-quad", width, height, [d], clear_color=(0.0, 0.0, 0.0, 1.0))


def alpha_mask_case(width: int = 200, height: int = 140) -> Scene:
    """Alpha-masked Cook-Torrance materials (`if (baseColor.a < alphaCutoff) discard;`, pixel/model_pbr.hlsl:176-179; glTF alphaMode
    MASK): an opaque back wall, in front of it a tilted cut-out quad whose texture alpha runs through every value (a fragment is
    kept or dropped one by one, and a dropped one leaves colour, depth and id to whatever lies behind), a second cut-out that is
    also alpha-blended, and a masked quad BEHIND the wall (its kept fragments fail the depth test).  The masked pipelines set
    fragment_discard_enable, so their segments are resolved in primitive order."""
    rng = PCG32(0xA1FA)
    view, proj, cam = default_camera(width, height, eye=(0.3, 0.2, 3.4))
    light = light_ubo(direction=(0.2, -0.6, -0.8), intensity=1.4, color=(1.0, 0.97, 0.92), num_point=1)
    points = point_light((1.0, 1.5, 2.0), 9.0, (0.6, 0.8, 1.0), 5.0)
    n = 32
    yy, xx = np.mgrid[0:n, 0:n]
    leaf = np.zeros((n, n, 4), dtype=np.uint8)
    leaf[..., 0] = 40 + 3 * xx; leaf[..., 1] = 120 + 4 * yy; leaf[..., 2] = 30; leaf[..., 3] = ((xx * 37 + yy * 91 + (xx * yy) % 7 * 29) % 256).astype(np.uint8)
    disc = np.zeros((n, n, 4), dtype=np.uint8)
    rr = np.hypot(xx - 15.5, yy - 15.5)
    disc[..., 0] = 220; disc[..., 1] = 150 + (r8 := (rng.uniform(n * n).reshape(n, n) * 60).astype(np.uint8)); disc[..., 2] = 60
    disc[..., 3] = np.clip(255 - rr * 18, 0, 255).astype(np.uint8)
    wall_tex = _procedural_texture(3, 32, 5)
    quad = lambda w, h, uvs: _pack_vertex48(np.array([[-w, -h, 0], [w, -h, 0], [w, h, 0], [-w, h, 0]], dtype=f32),
                                            np.tile(np.array([0, 0, 1], dtype=f32), (4, 1)),
                                            np.array([[0, 0], [uvs, 0], [uvs, uvs], [0, uvs]], dtype=f32), np.tile(np.array([1, 0, 0, 1], dtype=f32), (4, 1)))
    idx = np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32)
    common = dict(stride=48, count=6, indices=idx, program=PROGRAM_MODEL_PBR, cull_mode=CULL_NONE, camera=cam, light=light, point_lights=points)
    draws = [
        DrawSpec(vertices=quad(2.2, 1.6, 2.0), object=object_ubo(trs((1, 1, 1), quat_axis_angle((0, 1, 0), 0.15), (0.0, 0.0, -0.8))),
                 material=pbr_material_ubo((0.9, 0.9, 0.9, 1.0), 0.1, 0.6, 1.0, has_base_color=True), albedo_map=wall_tex, **common),
        DrawSpec(vertices=quad(1.1, 0.9, 2.5), object=object_ubo(trs((1, 1, 1), quat_axis_angle((0.2, 1, 0.1), 0.7), (-0.5, 0.1, 0.3))),
                 material=pbr_material_ubo((1.0, 1.0, 1.0, 0.9), 0.0, 0.5, 1.0, alpha_cutoff=0.45, has_base_color=True), albedo_map=Texture(leaf),
                 alpha_test=True, **common),
        DrawSpec(vertices=quad(0.8, 0.8, 1.0), object=object_ubo(trs((1, 1, 1), quat_axis_angle((1, 0, 0), -0.4), (0.9, -0.2, 0.6))),
                 material=pbr_material_ubo((1.0, 1.0, 1.0, 1.0), 0.3, 0.4, 1.0, alpha_cutoff=0.25, has_base_color=True), albedo_map=Texture(disc),
                 alpha_test=True, blend=ALPHA_BLEND, **common),
        DrawSpec(vertices=quad(1.5, 1.0, 3.0), object=object_ubo(trs((1, 1, 1), quat_axis_angle((0, 1, 0), 0.0), (0.2, 0.0, -2.0))),
                 material=pbr_material_ubo((0.2, 0.3, 1.0, 1.0), 0.0, 0.5, 1.0, alpha_cutoff=0.5, has_base_color=True), albedo_map=Texture(leaf),
                 alpha_test=True, **common),
    ]
    return Scene("alpha-mask", width, height, draws, clear_color=(0.05, 0.06, 0.1, 1.0))


def pbr_spheres_case(width: int = 224, height: int = 144) -> Scene:
    """Cook-Torrance program (pixel/model_pbr.hlsl): five draws covering every material switch -- factors only,
    all five textures, metallic, a constant-alpha draw the cutoff removes, and a textured draw whose cutoff is
    below every possible texel alpha."""
    rng = PCG32(0xB0B)
    view, proj, cam = default_camera(width, height, eye=(0.0, 0.4, 4.2))
    light = light_ubo(direction=(0.3, -0.8, -0.5), intensity=1.6, color=(1.0, 0.96, 0.9), num_point=2, num_spot=1)
    points = point_light((1.5, 1.2, 2.0), 9.0, (0.5, 0.7, 1.0), 6.0) + point_light((-2.0, 0.3, 1.5), 7.0, (1.0, 0.5, 0.3), 4.0)
    spots = spot_light((0.0, 2.5, 2.5), 0.93, (0.0, -0.7, -0.7), 0.75, (0.9, 1.0, 0.8), 9.0)
    base = _procedural_texture(2, 32, 7)
    nm = np.zeros((16, 16, 4), dtype=np.uint8)
    r = rng.uniform(16 * 16 * 2).reshape(16, 16, 2)
    nm[:, :, 0] = (128 + (r[:, :, 0] - 0.5) * 90).astype(np.uint8)
    nm[:, :, 1] = (128 + (r[:, :, 1] - 0.5) * 90).astype(np.uint8)
    nm[:, :, 2] = 225
    nm[:, :, 3] = 255
    mr = (rng.uniform(8 * 8 * 4).reshape(8, 8, 4) * 255).astype(np.uint8)
    occ = (128 + rng.uniform(8 * 8 * 4).reshape(8, 8, 4) * 127).astype(np.uint8)
    emi = (rng.uniform(4 * 4 * 4).reshape(4, 4, 4) * 255).astype(np.uint8)
    sphere = displaced_sphere(20, 14, width, height, seed=11).draws[0]
    mats = [
        dict(material=pbr_material_ubo((0.8, 0.3, 0.2, 1.0), 0.0, 0.45, 0.9, emissive=(0.02, 0.0, 0.05))),
        dict(material=pbr_material_ubo((1.0, 0.9, 0.8, 0.7), 0.9, 0.8, 1.0, normal_scale=0.7, emissive=(0.5, 0.4, 0.1),
                                       has_base_color=True, has_normal=True, has_metallic_roughness=True,
                                       has_occlusion=True, has_emissive=True),
             albedo_map=base, normal_map=Texture(nm), metallic_roughness_map=Texture(mr), occlusion_map=Texture(occ),
             emissive_map=Texture(emi)),
        dict(material=pbr_material_ubo((0.95, 0.8, 0.4, 1.0), 1.0, 0.02, 1.0)),                       # roughness clamp 0.04
        dict(material=pbr_material_ubo((0.1, 0.9, 0.1, 0.3), 0.0, 0.5, 1.0, alpha_cutoff=0.5)),      # dropped by the cutoff
        dict(material=pbr_material_ubo((0.3, 0.4, 0.9, 0.6), 0.2, 0.6, 0.7, alpha_cutoff=-0.25, has_base_color=True),
             albedo_map=base),
    ]
    draws = []
    for k, extra in enumerate(mats):
        x = -2.4 + 1.2 * k
        model = trs((0.55, 0.55, 0.55), quat_axis_angle((0.3, 1.0, 0.1), 0.4 * k), (x, 0.25 * (k % 2), -0.3 * k))
        draws.append(DrawSpec(vertices=sphere.vertices, stride=48, count=sphere.count, indices=sphere.indices,
                              program=PROGRAM_MODEL_PBR, cull_mode=CULL_BACK, front_face=sphere.front_face, camera=cam,
                              object=object_ubo(model), light=light, point_lights=points, spot_lights=spots, **extra))
    return Scene("pbr-spheres", width, height, draws, clear_color=(0.02, 0.02, 0.03, 1.0))


def mip_ground_case(width: int = 240, height: int = 150, max_anisotropy: int = 1) -> Scene:
    """Texture fidelity: a ground plane receding to the horizon under a fine checker -- strong, anisotropic
    minification -- through a mip chain with trilinear filtering and an sRGB-encoded albedo, plus an upright quad that is
    magnified (lambda clamps to 0).  A non-power-of-two normal map exercises the odd-size rule of the chain.
    max_anisotropy > 1: the same frame through the anisotropic filter (albedo at max_anisotropy, normal map at a quarter of it)."""
    rng = PCG32(0x717)
    n = 64
    yy, xx = np.mgrid[0:n, 0:n]
    checker = (((xx // 2) + (yy // 2)) & 1).astype(np.uint8)
    alb = np.zeros((n, n, 4), dtype=np.uint8)
    alb[..., 0] = 40 + 190 * checker; alb[..., 1] = 60 + 150 * (1 - checker); alb[..., 2] = 90 + (xx * 2).astype(np.uint8); alb[..., 3] = 255
    nm = np.zeros((24, 40, 4), dtype=np.uint8)
    r = rng.uniform(24 * 40 * 2).reshape(24, 40, 2)
    nm[..., 0] = (128 + (r[..., 0] - 0.5) * 70).astype(np.uint8); nm[..., 1] = (128 + (r[..., 1] - 0.5) * 70).astype(np.uint8)
    nm[..., 2] = 235; nm[..., 3] = 255
    albedo = Texture(alb, mips=True, srgb=True, max_anisotropy=max_anisotropy)
    normal = Texture(nm, mips=True, max_anisotropy=max(1, max_anisotropy // 4))
    view, proj, cam = default_camera(width, height, eye=(0.0, 1.2, 4.0), target=(0.0, 0.3, 0.0))
    light = light_ubo(direction=(0.2, -1.0, -0.3), intensity=0.9, color=(1.0, 0.97, 0.9), num_point=1)
    points = point_light((1.0, 2.0, 1.5), 12.0, (0.8, 0.9, 1.0), 5.0)
    ground = _pack_vertex48(np.array([[-30, 0, 6], [30, 0, 6], [30, 0, -120], [-30, 0, -120]], dtype=f32),
                            np.tile(np.array([0, 1, 0], dtype=f32), (4, 1)),
                            np.array([[0, 0], [40, 0], [40, 84], [0, 84]], dtype=f32), np.tile(np.array([1, 0, 0, 1], dtype=f32), (4, 1)))
    wall = _pack_vertex48(np.array([[-0.6, 0.0, 1.5], [0.6, 0.0, 1.5], [0.6, 1.2, 1.5], [-0.6, 1.2, 1.5]], dtype=f32),
                          np.tile(np.array([0, 0, 1], dtype=f32), (4, 1)),
                          np.array([[0.1, 0.1], [0.3, 0.1], [0.3, 0.3], [0.1, 0.3]], dtype=f32), np.tile(np.array([1, 0, 0, 1], dtype=f32), (4, 1)))
    idx = np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32)
    common = dict(stride=48, count=6, indices=idx, program=PROGRAM_MODEL_FULL, cull_mode=CULL_NONE, camera=cam,
                  object=object_ubo(np.eye(4, dtype=f32)), light=light, point_lights=points,
                  material=material_ubo((1.0, 1.0, 1.0, 1.0), 0.0, 0.6, 0.9), albedo_map=albedo, normal_map=normal)
    return Scene("mip-ground" if max_anisotropy <= 1 else f"aniso{max_anisotropy}-ground", width, height, [DrawSpec(vertices=ground, **common), DrawSpec(vertices=wall, **common)],
                 clear_color=(0.3, 0.5, 0.8, 1.0))


def gltf_model(path: str, width: int = 1920, height: int = 1080, program: int = PROGRAM_MODEL_FULL,
               eye=(0.0, 0.0, 3.2), yaw: float = 0.4, textures: bool = False) -> Scene:
    """A glTF asset through the reference's loader semantics (gltf.load) -> `Vertex` streams, lit like config 3:
    1 point light, base colour 0.7, roughness 0.5, white 1x1 albedo / "no normal map" textures.

    textures=True binds the asset's own images where its files exist (gltf.load(images=True)): base colour as
    R8G8B8A8_SRGB, normal / metallic-roughness / occlusion as UNORM, all with a mip chain and trilinear sampling
    (model_pbr.hlsl:62-95 slot order); the material's factors replace the config-3 constants."""
    from . import gltf
    model = gltf.load(path, images=textures)
    view, proj, cam = default_camera(width, height, eye=eye)
    obj = object_ubo(trs((1.0, 1.0, 1.0), quat_axis_angle((0.0, 1.0, 0.0), yaw), (0.0, 0.0, 0.0)))
    cache = {}

    def tex(index, srgb=False):
        if not textures or index is None or index >= len(model.images) or model.images[index] is None:
            return None
        if (index, srgb) not in cache:
            cache[(index, srgb)] = Texture(model.images[index].rgba, mips=True, srgb=srgb)
        return cache[(index, srgb)]

    draws = []
    for mesh in model.meshes:
        mat = model.materials[mesh.material_index] if textures and mesh.material_index is not None and mesh.material_index < len(model.materials) else None
        maps = dict(albedo_map=WHITE_1X1, normal_map=WHITE_1X1)
        material = (pbr_material_ubo((0.7, 0.7, 0.7, 1.0), 0.0, 0.5, 1.0) if program == PROGRAM_MODEL_PBR
                    else material_ubo((0.7, 0.7, 0.7, 1.0), 0.0, 0.5, 1.0))
        if program == PROGRAM_MODEL_PBR:
            maps.update(metallic_roughness_map=WHITE_1X1, occlusion_map=WHITE_1X1, emissive_map=WHITE_1X1)
        if mat is not None:
            maps["albedo_map"] = tex(mat.base_color_image, srgb=True) or WHITE_1X1
            maps["normal_map"] = tex(mat.normal_image) or WHITE_1X1
            if program == PROGRAM_MODEL_PBR:
                slots = {"metallic_roughness_map": tex(mat.metallic_roughness_image), "occlusion_map": tex(mat.occlusion_image),
                         "emissive_map": tex(mat.emissive_image, srgb=True)}
                maps.update({k: v or WHITE_1X1 for k, v in slots.items()})
                material = pbr_material_ubo(mat.base_color, mat.metallic, mat.roughness, mat.ao, normal_scale=mat.normal_scale,
                                            emissive=mat.emissive[:3], has_base_color=maps["albedo_map"] is not WHITE_1X1,
                                            has_normal=maps["normal_map"] is not WHITE_1X1,
                                            has_metallic_roughness=slots["metallic_roughness_map"] is not None,
                                            has_occlusion=slots["occlusion_map"] is not None, has_emissive=slots["emissive_map"] is not None)
            else:
                material = material_ubo(mat.base_color, mat.metallic, mat.roughness, mat.ao)
        draws.append(DrawSpec(vertices=mesh.interleave(), stride=48, count=int(mesh.indices.size), indices=mesh.indices,
                              program=program, cull_mode=CULL_NONE, front_face=FRONT_CCW, camera=cam, object=obj,
                              light=light_ubo(direction=(0.0, -1.0, 0.0), intensity=0.0, num_point=1),
                              material=material,
                              point_lights=point_light((2.0, 2.0, 2.0), 10.0, (1.0, 1.0, 1.0), 5.0), **maps))
    tag = "-textured" if textures else ""
    return Scene(f"gltf-{os.path.basename(os.path.dirname(os.path.abspath(path)))}-{model.total_triangles}{tag}", width, height, draws,
                 clear_color=(0.1, 0.1, 0.15, 1.0))


SMALL_CASES = {
    "hello": lambda: hello_triangle(64, 64),
    "fan": shared_edge_fan,
    "near_clip": near_clip_case,
    "depth_tie": depth_tie_case,
    "cull_scissor": cull_scissor_case,
    "multi_draw": multi_draw_case,
    "huge": huge_triangle_case,
    "textured": textured_quad_case,
    "pbr": pbr_spheres_case,
    "mips": mip_ground_case,
    "aniso": lambda: mip_ground_case(max_anisotropy=16),
    "alpha_mask": alpha_mask_case,
    "random_small": lambda: random_triangles(300, 320, 200, seed=42, rmin=2, rmax=40),
    "sphere_small": lambda: displaced_sphere(24, 17, 256, 160, seed=3),
}


# ------------------------------------------------------------------------------------------------
# image-based ambient lighting (pixel/model_pbr_ibl.hlsl, MIRHI_PROGRAM_MODEL_PBR_IBL)
# ------------------------------------------------------------------------------------------------
# (normal, roughness, metallic, ao, emissive) per facet: the normals' major axes are +X -X +Y -Y +Z -Z twice over, no two largest |components|
# closer than 0.2; every roughness of {0, 0.3, 4/7, 0.8, 1} and metallic of {0, 0.5, 1} occurs
IBL_FACETS = (
    ((0.9, 0.3, 0.25), 0.0, 0.0, 1.0, (0.0, 0.0, 0.0)), ((-0.8, 0.2, 0.5), 0.3, 0.5, 0.7, (0.0, 0.0, 0.0)),
    ((0.3, 0.85, 0.4), 4.0 / 7.0, 1.0, 1.0, (0.0, 0.0, 0.0)), ((0.2, -0.9, 0.35), 0.8, 0.0, 0.4, (0.0, 0.0, 0.0)),
    ((0.25, 0.3, 0.9), 1.0, 0.5, 1.0, (0.0, 0.0, 0.0)), ((-0.3, 0.2, -0.85), 0.3, 1.0, 0.6, (0.0, 0.0, 0.0)),
    ((0.8, -0.45, -0.3), 0.8, 0.5, 1.0, (0.3, 0.1, 0.05)), ((-0.9, -0.35, 0.2), 1.0, 0.0, 0.8, (0.0, 0.0, 0.0)),
    ((-0.35, 0.8, -0.4), 0.0, 1.0, 1.0, (0.0, 0.0, 0.0)), ((-0.4, -0.85, -0.2), 4.0 / 7.0, 0.0, 0.5, (0.0, 0.0, 0.0)),
    ((-0.2, -0.45, 0.85), 0.3, 0.0, 1.0, (0.0, 0.0, 0.0)), ((0.45, 0.15, -0.9), 4.0 / 7.0, 0.5, 0.9, (0.0, 0.0, 0.0)),
)
IBL_FACETS_EYE = (0.35, 0.25, 6.0)


def ibl_test_images(pre_size: int = 16, pre_levels: int = 5, irr_size: int = 8, lut_size: int = 16, zero: bool = False):
    """Uploadable contents for an IBL set (float32): ibl.analytic_environment scaled differently per cube and per level -- a wrong level or face
    shows -- and a smooth LUT that is not symmetric in its axes.  zero: all three images zero."""
    from . import ibl as _ibl
    irr = (0.5 * _ibl.analytic_environment(irr_size)).astype(f32)
    pre = [((1.0 + 0.25 * l) * _ibl.analytic_environment(pre_size >> l)).astype(f32) for l in range(pre_levels)]
    c = (np.arange(lut_size) + 0.5) / lut_size
    ndv, rough = np.meshgrid(c, c, indexing="xy")           # column = NdotV, row = roughness
    lut = np.stack([0.9 * (1.0 - rough) + 0.1 * ndv, 0.3 * ndv * rough + 0.05, np.zeros_like(ndv), np.ones_like(ndv)], axis=-1).astype(f32)
    if zero:
        irr, pre, lut = np.zeros_like(irr), [np.zeros_like(l) for l in pre], np.zeros_like(lut)
    return IblSpec(irradiance=irr, prefiltered=pre, lut=lut)


def ibl_facets_case(width: int = 128, height: int = 96, lit: bool = False, ao=None, program: int = PROGRAM_MODEL_PBR_IBL,
                    pre_size: int = 16, pre_levels: int = 5) -> Scene:
    """Twelve flat quads in a 4 x 3 grid, each in its own plane z = const facing the camera, every vertex of a quad carrying the quad's
    (made-up) normal of IBL_FACETS, so N is constant per primitive and known; materials without textures.  lit=False: no light reaches
    anything (Lo is exact zero); lit=True: a directional, a point and a spot light.  ao: overrides every facet's occlusion factor.
    scene.facets lists, per quad (= draw d, primitives 2 d and 2 d + 1): normal, plane z, base colour, roughness, metallic, ao, emissive."""
    view, proj, cam = default_camera(width, height, eye=IBL_FACETS_EYE)
    if lit:
        light = light_ubo(direction=(0.3, -0.5, -0.8), intensity=1.5, color=(1.0, 0.95, 0.9), num_point=1, num_spot=1)
        points = point_light((1.0, 1.0, 2.5), 9.0, (0.9, 0.6, 0.4), 6.0)
        spots = spot_light((-1.5, 0.5, 4.0), math.cos(0.3), (0.3, -0.1, -1.0), math.cos(0.6), (0.4, 0.7, 1.0), 12.0)
    else:
        light, points, spots = light_ubo(intensity=0.0), b"", b""
    obj = object_ubo(np.eye(4, dtype=f32))
    idx = np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32)
    draws, facets = [], []
    for k, (nrm, rough, metal, fao, emis) in enumerate(IBL_FACETS):
        gx, gy = k % 4, k // 4
        x0, y0, z = -2.0 + gx * 1.0 + 0.06, -1.5 + gy * 1.0 + 0.06, -0.6 + 0.1 * k
        pos = np.array([[x0, y0, z], [x0 + 0.88, y0, z], [x0 + 0.88, y0 + 0.88, z], [x0, y0 + 0.88, z]])
        n = np.asarray(nrm, dtype=np.float64)
        n = n / np.linalg.norm(n)
        verts = _pack_vertex48(pos, np.tile(n, (4, 1)), np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.float64), np.tile(np.array([1.0, 0.0, 0.0, 1.0]), (4, 1)))
        base = (0.35 + 0.05 * k, 0.9 - 0.06 * k, 0.5 + 0.03 * ((k * 5) % 12), 1.0)
        fao = fao if ao is None else ao
        draws.append(DrawSpec(vertices=verts, stride=48, count=6, indices=idx, program=program, cull_mode=CULL_NONE, camera=cam, object=obj, light=light,
                              material=pbr_material_ubo(base, metal, rough, fao, emissive=emis), point_lights=points, spot_lights=spots))
        facets.append(dict(normal=verts[0, 3:6].copy(), z=float(f32(z)), base=np.asarray(base, dtype=f32), roughness=float(f32(rough)), metallic=float(f32(metal)),
                           ao=float(f32(fao)), emissive=np.asarray(emis, dtype=f32)))
    scene = Scene("ibl-facets", width, height, draws, clear_color=(0.01, 0.02, 0.03, 1.0), ibl=ibl_test_images(pre_size, pre_levels))
    scene.facets, scene.view, scene.proj, scene.eye = facets, view, proj, _v(IBL_FACETS_EYE)
    return scene


# ------------------------------------------------------------------------------------------------
# the sky (vertex/skybox.hlsl + pixel/skybox.hlsl, MIRHI_PROGRAM_SKYBOX)
# ------------------------------------------------------------------------------------------------
SKYBOX_CAMERAS = ((0.6, 0.3), (math.pi / 4.0, 0.6155))      # (yaw, pitch); the second looks at a cube corner: both see three faces


def sky_rotation(yaw: float, pitch: float) -> np.ndarray:
    """Rotation-only view matrix ([col, row] float32) of a camera turned by `yaw` about +Y, then pitched up by `pitch`."""
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    fwd = np.array([-sy * cp, sp, -cy * cp])
    right = np.array([cy, 0.0, -sy])
    up = np.cross(right, fwd)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = right, up, -fwd      # maths rows
    return m.T.astype(f32)                              # -> [col, row]


def inverse_view_projection(view: np.ndarray, proj: np.ndarray) -> np.ndarray:
    """inverse(proj * view) as [col, row] float32 (inverted in float64)."""
    vp = mat_mul(proj, view).astype(np.float64).T      # maths matrix
    return np.linalg.inv(vp).T.astype(f32)


def skybox_case(width: int = 128, height: int = 96, camera: int = 0, size: int = 16, levels: int = 5, fov_deg: float = 60.0) -> Scene:
    """The sky alone: ibl.analytic_environment of size^2 (further levels: cube_mips scaled by 1 + l / 4, which a lod-0 lookup must never
    show) behind nothing, camera SKYBOX_CAMERAS[camera] with a vertical field of view of 60 degrees.  scene.sky.inv_view_proj is the matrix."""
    from . import ibl as _ibl
    yaw, pitch = SKYBOX_CAMERAS[camera]
    view = sky_rotation(yaw, pitch)
    proj = perspective_rh(math.radians(fov_deg), width / height, 0.1, 100.0)      # (no y flip: vertex/skybox.hlsl:40 flips y itself)
    l0 = _ibl.analytic_environment(size).astype(f32)
    chain = [l0] + [((1.0 + 0.25 * (l + 1)) * m).astype(f32) for l, m in enumerate(_ibl.cube_mips(l0, levels)[1:])]
    scene = Scene(f"skybox-{camera}-{size}x{levels}", width, height, [], clear_color=(0.01, 0.02, 0.03, 1.0),
                  sky=SkySpec(inv_view_proj=inverse_view_projection(view, proj), levels=chain))
    scene.view, scene.proj = view, proj
    return scene


# ------------------------------------------------------------------------------------------------
# shadow mapping (vertex/shadow.hlsl + pixel/shadow.hlsl, shadow.hlsli CalculateShadow in model_pbr.hlsl)
# ------------------------------------------------------------------------------------------------
SHADOWED_GROUND_LIGHT = (0.45, -1.0, 0.3)
SHADOWED_GROUND_BOX = ((0.3, 1.1, 0.2), (0.7, 1.1, 0.7))        # centre, half extent
SHADOWED_GROUND_EXTENT = 8.0                                      # the light frustum's half extent: covers the whole ground


def depth_bias_unit(z_window) -> float:
    """r of DESIGN.md 8h: 2^(e - 23), e the unbiased binary32 exponent of the largest |z| of a triangle's three window depths (zero or denormal: -126)."""
    zm = float(np.float32(np.max(np.abs(np.asarray(z_window, dtype=np.float64)))))
    e = math.frexp(zm)[1] - 1 if zm >= 2.0 ** -126 else -126       # (frexp: zm = f 2^k with 1/2 <= f < 1)
    return 2.0 ** (e - 23)


def depth_bias_offset(z_window, xy_window, factors) -> float:
    """The float64 model of the depth bias (Vulkan "Depth Bias" with the max form of m and the floating-point rule for r): the offset o
    added to every fragment depth of the triangle with window depths z_window[3] at window positions xy_window[3] (pixels), for
    factors = (constant_factor, clamp, slope_factor).  o = m * slope + r * constant, m = max(|dz/dx|, |dz/dy|) of the depth plane, r = depth_bias_unit;
    clamp > 0: min(o, clamp), clamp < 0: max(o, clamp), 0: none."""
    z = np.asarray(z_window, dtype=np.float64)
    p = np.asarray(xy_window, dtype=np.float64)
    constant, clamp, slope = (float(f) for f in factors)
    x1, y1 = p[1] - p[0]
    x2, y2 = p[2] - p[0]
    area = x1 * y2 - x2 * y1
    zx = ((z[1] - z[0]) * y2 - (z[2] - z[0]) * y1) / area
    zy = ((z[2] - z[0]) * x1 - (z[1] - z[0]) * x2) / area
    o = max(abs(zx), abs(zy)) * slope + depth_bias_unit(z) * constant
    if clamp > 0.0:
        o = min(o, clamp)
    elif clamp < 0.0:
        o = max(o, clamp)
    return o


def _ground_quad(half: float, n: int) -> tuple:
    """The y = 0 plane over [-half, half]^2, n x n quads, normal +y."""
    uu, vv = np.meshgrid(np.linspace(0.0, 1.0, n + 1), np.linspace(0.0, 1.0, n + 1), indexing="xy")
    uu, vv = uu.reshape(-1), vv.reshape(-1)
    pos = np.stack([-half + 2 * half * uu, np.zeros_like(uu), half - 2 * half * vv], axis=1)
    nrm = np.tile(np.array([0.0, 1.0, 0.0]), (pos.shape[0], 1))
    tan = np.tile(np.array([1.0, 0.0, 0.0, 1.0]), (pos.shape[0], 1))
    return _pack_vertex48(pos, nrm, np.stack([uu, vv], axis=1), tan), _grid_indices(n, n).astype(np.uint32)


def shadowed_ground_case(width: int = 320, height: int = 240, map_size: int = 512, strength: float = 1.0,
                         light_dir=SHADOWED_GROUND_LIGHT, intensity: float = 2.0) -> Scene:
    """MODEL_PBR ground plane, a box that casts a shadow on it and a sphere, under one directional light; the box is the shadow
    scope's only caster."""
    view, proj, cam = default_camera(width, height, eye=(0.0, 4.5, 6.5))
    light = light_ubo(direction=light_dir, intensity=intensity, color=(1.0, 0.97, 0.9))
    ls = light_space_matrix(light_dir, half_extent=SHADOWED_GROUND_EXTENT)
    gv, gi = _ground_quad(5.0, 8)
    bv, bi = _box_mesh(*SHADOWED_GROUND_BOX)
    sphere = displaced_sphere(24, 17, width, height, seed=3).draws[0]
    eye4 = np.eye(4, dtype=f32)
    draws = [
        DrawSpec(vertices=gv, stride=48, count=gi.size, indices=gi, program=PROGRAM_MODEL_PBR, cull_mode=CULL_NONE, camera=cam,
                 object=object_ubo(eye4), light=light, material=pbr_material_ubo((0.8, 0.8, 0.75, 1.0), 0.0, 0.7)),
        DrawSpec(vertices=bv, stride=48, count=bi.size, indices=bi, program=PROGRAM_MODEL_PBR, cull_mode=CULL_BACK, front_face=FRONT_CCW,
                 camera=cam, object=object_ubo(eye4), light=light, material=pbr_material_ubo((0.6, 0.3, 0.2, 1.0), 0.0, 0.5)),
        DrawSpec(vertices=sphere.vertices, stride=48, count=sphere.count, indices=sphere.indices, program=PROGRAM_MODEL_PBR,
                 cull_mode=CULL_BACK, front_face=sphere.front_face, camera=cam,
                 object=object_ubo(trs((0.6, 0.6, 0.6), (0.0, 0.0, 0.0, 1.0), (-2.0, 0.8, 1.0))), light=light,
                 material=pbr_material_ubo((0.2, 0.4, 0.8, 1.0), 0.3, 0.4)),
    ]
    caster = DrawSpec(vertices=bv, stride=48, count=bi.size, indices=bi, program=PROGRAM_SHADOW, cull_mode=CULL_NONE,
                      camera=shadow_constants_ubo(flip_clip_y(ls), eye4))
    shadow = ShadowSpec([caster], (map_size, map_size), shadow_ubo(ls, 0.005, 0.02, (map_size, map_size), strength))
    return Scene("shadowed-ground", width, height, draws, clear_color=(0.02, 0.02, 0.03, 1.0), shadow=shadow)


def pcf_factor(depth_map: np.ndarray, u: np.ndarray, v: np.ndarray, dref: np.ndarray, texel=None, strength: float = 1.0) -> np.ndarray:
    """Numpy model of CalculateShadow's 3x3 comparison taps with this build's sampler (include/mirhi.h MIRHI_TEXTURE_SHADOW_MAP):
    LESS_OR_EQUAL against clamp(dref, 0, 1), nearest texel, clamp-to-edge; tap offsets `texel` = 1 / ShadowMapSize (default the
    map's extent).  Returns lerp(1, lit taps / 9, strength) per sample."""
    h, w = depth_map.shape
    tu, tv = (1.0 / w, 1.0 / h) if texel is None else texel
    d = np.clip(dref, 0.0, 1.0)
    lit = np.zeros(np.shape(u), dtype=np.float64)
    for x in (-1, 0, 1):
        for y in (-1, 0, 1):
            i = np.clip(np.floor((u + x * tu) * w), 0, w - 1).astype(np.int64)
            j = np.clip(np.floor((v + y * tv) * h), 0, h - 1).astype(np.int64)
            lit += (d <= depth_map[j, i]).astype(np.float64)
    s = lit / 9.0
    return 1.0 + (s - 1.0) * strength


# ------------------------------------------------------------------------------------------------
# cascaded shadow maps (shadow_csm.hlsli CalculateShadowCSM in pixel/model_pbr_ibl_csm.hlsl:280-298)
# ------------------------------------------------------------------------------------------------
CASCADE_COUNT = 4                                                   # shadow_csm.hlsli:19


def csm_ubo(matrices, split_depths, bias: float = 0.005, normal_bias: float = 0.02, map_size: float = 2048.0) -> bytes:
    """CSMParams 336 B (shaders/hlsl/shadow_csm.hlsli:23-39): Cascades[k].ViewProjection @80k, Cascades[k].SplitDepth @80k + 64 (padded to
    80), ShadowBias @320, NormalBias @324, ShadowMapSize @328, padding @332.  split_depths: three (the shader reads no more) or four."""
    assert len(matrices) == CASCADE_COUNT and len(split_depths) in (CASCADE_COUNT - 1, CASCADE_COUNT)
    splits = list(split_depths) + [1.0] * (CASCADE_COUNT - len(split_depths))
    out = b""
    for m, sd in zip(matrices, splits):
        out += np.asarray(m, dtype=f32).tobytes() + np.array([sd, 0, 0, 0], dtype=f32).tobytes()
    out += np.array([bias, normal_bias, map_size, 0], dtype=f32).tobytes()
    assert len(out) == 336
    return out


def csm_split_distances(near: float, far: float, count: int = CASCADE_COUNT, lam: float = 0.5) -> np.ndarray:
    """The practical split scheme of "Parallel-Split Shadow Maps on Programmable GPUs" (Zhang et al., the paper shadow_csm.hlsli:12 cites):
    far distance of slice i = lam * near * (far / near)^(i / count) + (1 - lam) * (near + (far - near) * i / count), i = 1 .. count
    (lam = 1 logarithmic, lam = 0 uniform)."""
    i = np.arange(1, count + 1, dtype=np.float64) / count
    return lam * near * (far / near) ** i + (1.0 - lam) * (near + (far - near) * i)


@dataclass
class Cascades:
    matrices: List[np.ndarray]            # per cascade: orthographic light matrix (projection * view), [col,row] float32
    split_depths: np.ndarray              # per cascade: the camera's clip-space depth of the slice's far distance (float32)
    distances: np.ndarray                 # count + 1 view distances: slice k is [distances[k], distances[k + 1]]
    corners: List[np.ndarray]             # per cascade: the eight world-space corners of its slice of the camera frustum (float64)
    half_extents: List[float]             # per cascade: half the side of its square light frustum (world units)


CSM_RADIUS_QUANTUM = 1.0 / 16.0                                     # world units a stabilised cascade's radius is rounded up to


def csm_cascades(view: np.ndarray, proj: np.ndarray, light_dir, near: float, far: float, count: int = CASCADE_COUNT, lam: float = 0.5,
                 caster_margin: float = 8.0, stabilize: bool = False, map_size=None) -> Cascades:
    """Splits the camera frustum between the view distances near and far into `count` slices (csm_split_distances) and gives each an
    orthographic light matrix that encloses it: the light looks along light_dir at the slice's centre, its square frustum is the slice's
    bounding box in light space (padded by 0.1 %), pulled back towards the light by caster_margin so that casters between the light and
    the slice are kept.  The split depth is what the camera's projection gives the split distance, i.e. SV_Position.z of a fragment there
    (viewport depth range 0..1).  The reference has no host code for cascades (no file under crates/ mentions one): this is this build's
    own, as small as the containment test needs -- no texel snapping, no stabilisation.
    stabilize=True (map_size, a layer's edge in texels, is then required): the cascades of a camera that moves.  Cascade k's matrix is a function
    of the light direction, a quantised radius and a snapped centre, and of nothing else:
      radius   the bounding sphere of the slice's eight corners about their mean, taken in VIEW space (where the corners do not depend on the
               pose: the same float for every camera position and orientation), rounded up to a multiple of CSM_RADIUS_QUANTUM and padded by one
               texel: R = Rq / (1 - 2 / map_size), so that R = Rq + texel with texel = 2 R / map_size -- the snapped frustum still holds the sphere
      basis    look_at_rh from the origin along light_dir with the fixed up vector: no pose in it
      frustum  square, side 2 R about the snapped centre; the eye R + caster_margin in front of it, zn = 0.1, zf = 2 R + caster_margin
      snapping the centre's three light-space coordinates to whole multiples of texel, with floor
    The matrix is put together in float64 from those numbers and rounded to float32 once: only its translation column knows the pose, in whole
    texels, so a fixed world point's texel coordinates move by whole texels from pose to pose and no shadow edge crawls.  half_extents[k] = R."""
    if stabilize:
        assert map_size is not None and int(map_size) > 2, "stabilize=True needs map_size"
    dist = np.concatenate([[float(near)], csm_split_distances(near, far, count, lam)])
    p64, inv_view = proj.astype(np.float64), np.linalg.inv(view.astype(np.float64).T)      # maths (row-major) inverse view
    tx, ty = 1.0 / abs(p64[0, 0]), 1.0 / abs(p64[1, 1])                                  # tan of the half angles
    d = _normalize(light_dir).astype(np.float64)
    up = np.array((0.0, 1.0, 0.0) if abs(d[1]) < 0.99 else (0.0, 0.0, -1.0))
    mats, corners_all, halves = [], [], []
    for k in range(count):
        cs = []
        for dd in (dist[k], dist[k + 1]):
            for sx in (-1.0, 1.0):
                for sy in (-1.0, 1.0):
                    cs.append((inv_view @ np.array([sx * dd * tx, sy * dd * ty, -dd, 1.0]))[:3])
        cs = np.array(cs)
        if stabilize:
            vs = np.array([[sx * dd * tx, sy * dd * ty, -dd] for dd in (dist[k], dist[k + 1]) for sx in (-1.0, 1.0) for sy in (-1.0, 1.0)])
            vc = vs.mean(axis=0)
            rq = math.ceil(float(np.linalg.norm(vs - vc, axis=1).max()) / CSM_RADIUS_QUANTUM) * CSM_RADIUS_QUANTUM
            r = rq / (1.0 - 2.0 / float(map_size))
            texel = 2.0 * r / float(map_size)
            rot = look_at_rh((0.0, 0.0, 0.0), d, up).astype(np.float64)[:3, :3]                   # the light basis: p @ rot = (p.s, p.u, -p.f)
            lc = (inv_view @ np.array([vc[0], vc[1], vc[2], 1.0]))[:3] @ rot
            cx, cy, dc = (math.floor(float(c) / texel) * texel for c in (lc[0], lc[1], -lc[2]))
            zn, zf = 0.1, 2.0 * r + float(caster_margin)
            e = dc - (r + float(caster_margin))                                                  # the eye's depth along the light
            m = np.zeros((4, 4), dtype=np.float64)
            m[:3, 0], m[:3, 1], m[:3, 2] = rot[:, 0] / r, rot[:, 1] / r, -rot[:, 2] / (zf - zn)
            m[3] = [-cx / r, -cy / r, -(e + zn) / (zf - zn), 1.0]
            mats.append(m.astype(f32))
            corners_all.append(cs)
            halves.append(float(r))
            continue
        centre = cs.mean(axis=0)
        radius = float(np.linalg.norm(cs - centre, axis=1).max())
        eye = centre - d * (radius + caster_margin)
        lview = look_at_rh(eye, centre, up)
        lc = np.concatenate([cs, np.ones((8, 1))], axis=1) @ lview.astype(np.float64)         # light-view space (p @ m for [col,row])
        cx, cy = 0.5 * (lc[:, 0].min() + lc[:, 0].max()), 0.5 * (lc[:, 1].min() + lc[:, 1].max())
        half = 1.001 * 0.5 * max(lc[:, 0].max() - lc[:, 0].min(), lc[:, 1].max() - lc[:, 1].min())
        zn, zf = 0.1, float(-lc[:, 2].min()) * 1.001 + 0.01
        mats.append(mat_mul(orthographic_rh(cx - half, cx + half, cy - half, cy + half, zn, zf), lview))
        corners_all.append(cs)
        halves.append(float(half))
    sd = np.array([(p64[2, 2] * -dd + p64[3, 2]) / dd for dd in dist[1:]]).astype(f32)
    return Cascades(mats, sd, dist, corners_all, halves)


def csm_select(split_depths, clip_depth) -> np.ndarray:
    """SelectCascade (shadow_csm.hlsli:55-71): the last i in 0..2 with clip_depth > SplitDepth[i], plus one (float32 comparison)."""
    cd = np.asarray(clip_depth, dtype=f32)
    idx = np.zeros(cd.shape, dtype=np.int64)
    for i in range(CASCADE_COUNT - 1):
        idx = np.where(cd > f32(split_depths[i]), i + 1, idx)
    return idx


def csm_factor(layers, matrices, split_depths, world_pos, normal, light_dir, clip_depth, bias: float, normal_bias: float,
               map_size: float) -> np.ndarray:
    """Numpy model of CalculateShadowCSM (shadow_csm.hlsli:163-194) with this build's sampler (pcf_factor): SelectCascade on clip_depth,
    then SampleCascadePCF in the selected layer -- the normal offset first, ONE matrix product, the bounds test on the offset position
    (outside: 1.0), adaptive bias max(bias * (1 - N.L), 0.0005), nine taps at uv + (x, y) / map_size, / 9.  Geometry in float64; the
    texel decisions and the comparison as the sampler is specified.  layers: (4, H, W); world_pos (..., 3); normal (..., 3) or (3,);
    light_dir: towards the light; clip_depth (...)."""
    idx = csm_select(split_depths, clip_depth)
    per = csm_cascade_samples(layers, matrices, world_pos, normal, light_dir, bias, normal_bias, map_size)
    out = np.ones(idx.shape, dtype=np.float64)
    for k in range(CASCADE_COUNT):
        out = np.where(idx == k, per[k], out)
    return out


def csm_cascade_samples(layers, matrices, world_pos, normal, light_dir, bias: float, normal_bias: float, map_size: float) -> np.ndarray:
    """SampleCascadePCF (shadow_csm.hlsli:90-146) of every sample in every cascade, (4, ...): the per-cascade sampler that csm_factor and
    csm_factor_blended share (csm_factor says what it computes)."""
    wp = np.asarray(world_pos, dtype=np.float64)
    n = np.broadcast_to(np.asarray(normal, dtype=np.float64), wp.shape)
    l = np.asarray(light_dir, dtype=np.float64)
    off = wp + n * float(normal_bias)
    p4 = np.concatenate([off, np.ones(off.shape[:-1] + (1,))], axis=-1)
    ndotl = (n * l).sum(axis=-1)
    ab = np.maximum(float(bias) * (1.0 - ndotl), 0.0005)
    out = []
    for k in range(CASCADE_COUNT):
        clip = p4 @ np.asarray(matrices[k], dtype=np.float64)
        pc = clip[..., :3] / clip[..., 3:4]
        u, v, z = pc[..., 0] * 0.5 + 0.5, 1.0 - (pc[..., 1] * 0.5 + 0.5), pc[..., 2]
        inside = (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (v <= 1.0) & (z >= 0.0) & (z <= 1.0)
        s = pcf_factor(np.asarray(layers[k]), u, v, z - ab, texel=(1.0 / map_size, 1.0 / map_size))
        out.append(np.where(inside, s, 1.0))
    return np.array(out, dtype=np.float64)


def csm_blend_terms(split_depths, clip_depth, blend_threshold: float, dtype=f32):
    """The per-sample decisions of CalculateShadowCSMBlended (shadow_csm.hlsli:242-255) in float32, as the device takes them and as csm_select
    compares: (idx, blending, distanceToEdge, blendRegion).  blending: cascadeIndex < 3 and 0 < distanceToEdge < blendRegion; prevSplit of
    cascade 0 is 0.  dtype=np.float64: the same in float64 -- the function of a real depth, for statements about its continuity."""
    cd = np.asarray(clip_depth, dtype=dtype)
    sd = np.array([split_depths[i] for i in range(CASCADE_COUNT - 1)], dtype=dtype)
    idx = np.zeros(cd.shape, dtype=np.int64)
    for i in range(CASCADE_COUNT - 1):                             # csm_select, in dtype
        idx = np.where(cd > sd[i], i + 1, idx)
    k = np.minimum(idx, CASCADE_COUNT - 2)
    split = sd[k]
    prev = np.where(k == 0, dtype(0.0), sd[np.maximum(k - 1, 0)]).astype(dtype)
    region = ((split - prev).astype(dtype) * dtype(blend_threshold)).astype(dtype)
    dist = (split - cd).astype(dtype)
    blending = (idx < CASCADE_COUNT - 1) & (dist < region) & (dist > dtype(0.0))
    return idx, blending, dist, region


def csm_factor_blended(layers, matrices, split_depths, world_pos, normal, light_dir, clip_depth, bias: float, normal_bias: float,
                       map_size: float, blend_threshold: float, depth_dtype=f32) -> np.ndarray:
    """Numpy model of CalculateShadowCSMBlended (shadow_csm.hlsli:212-277) over csm_factor's per-cascade sampler: the selected cascade's
    SampleCascadePCF and, where csm_blend_terms says the sample blends, lerp(nextShadow, shadow, distanceToEdge / blendRegion) =
    nextShadow + f (shadow - nextShadow) with the next cascade's, in float64."""
    idx, blending, dist, region = csm_blend_terms(split_depths, clip_depth, blend_threshold, depth_dtype)
    per = csm_cascade_samples(layers, matrices, world_pos, normal, light_dir, bias, normal_bias, map_size)
    shadow = np.ones(idx.shape, dtype=np.float64)
    nxt = np.ones(idx.shape, dtype=np.float64)
    for k in range(CASCADE_COUNT):
        shadow = np.where(idx == k, per[k], shadow)
        if k + 1 < CASCADE_COUNT:
            nxt = np.where(idx == k, per[k + 1], nxt)
    f = np.where(blending, dist.astype(np.float64) / np.where(blending, region, 1.0).astype(np.float64), 1.0)
    return np.where(blending, nxt + f * (shadow - nxt), shadow)


CSM_DEBUG_COLORS = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 0.0]], dtype=f32)      # shadow_csm.hlsli:293-298


def csm_debug_colors(split_depths, depth) -> np.ndarray:
    """GetCascadeDebugColor (shadow_csm.hlsli:289-301) on a read-back depth image: red, green, blue, yellow for cascades 0 .. 3 of SelectCascade,
    (..., 3) float32.  Host only -- the reference calls the function nowhere, and a read-back D32 attachment holds SV_Position.z: a way to look at
    the split layout of a frame."""
    return CSM_DEBUG_COLORS[csm_select(split_depths, depth)]


CASCADED_GROUND_LIGHT = (0.6, -1.0, 0.2)
CASCADED_GROUND_EYE, CASCADED_GROUND_TARGET = (0.0, 3.0, 6.0), (0.0, 0.0, -14.0)
CASCADED_GROUND_RANGE = (2.0, 60.0)                                # view distances the cascades cover
CASCADED_GROUND_LAM = 0.6                                          # split scheme blend (csm_split_distances)
CASCADED_GROUND_SPHERE = ((0.6, 0.6, 0.6), (-1.6, 0.8, 1.5))       # scale, translation of the displaced sphere


def cascaded_ground_boxes(lam: float = CASCADED_GROUND_LAM):
    """(centre, half extent) of one caster box per cascade of cascaded_ground_case: on the ground, at the middle view distance of the
    cascade's slice, left of the view axis (the light throws the shadows to the right, into view), growing with the distance."""
    dist = np.concatenate([[CASCADED_GROUND_RANGE[0]], csm_split_distances(*CASCADED_GROUND_RANGE, lam=lam)])
    eye, tgt = np.array(CASCADED_GROUND_EYE), np.array(CASCADED_GROUND_TARGET)
    fwd = (tgt - eye) / np.linalg.norm(tgt - eye)
    boxes = []
    for k in range(CASCADE_COUNT):
        mid = 0.5 * (dist[k] + dist[k + 1])
        t = eye[2] + (mid + eye[1] * fwd[1]) / fwd[2]              # z of the ground point (x ~ 0, y = 0) whose view distance (p - eye) . fwd is mid
        size = 0.6 + 0.03 * mid + 0.0035 * mid * mid
        boxes.append(((float(-(0.4 + 0.06 * mid) - 0.5 * size), float(size), float(t)), (float(size * 0.8), float(size), float(size * 0.8))))
    return boxes


def cascaded_ground_case(width: int = 480, height: int = 360, map_size: int = 2048, light_dir=CASCADED_GROUND_LIGHT,
                         intensity: float = 2.0, lam: float = CASCADED_GROUND_LAM, stabilize: bool = False, blend_threshold: float = 0.0,
                         eye=CASCADED_GROUND_EYE, target=CASCADED_GROUND_TARGET) -> Scene:
    """A long MODEL_PBR ground strip receding from a perspective camera, a caster box in each cascade's depth range and the displaced
    sphere, under one directional light; every box and the sphere are casters of all four cascade scopes.  stabilize: texel-snapped cascades
    (csm_cascades); blend_threshold: CascadeSpec.blend_threshold; eye / target: the camera's pose (a camera that moves over the fixed scene)."""
    view, proj, cam = default_camera(width, height, eye=eye, target=target)
    light = light_ubo(direction=light_dir, intensity=intensity, color=(1.0, 0.97, 0.9))
    cas = csm_cascades(view, proj, light_dir, *CASCADED_GROUND_RANGE, lam=lam, stabilize=stabilize, map_size=map_size if stabilize else None)
    pos = np.array([[-40.0, 0.0, 8.0], [40.0, 0.0, 8.0], [40.0, 0.0, -90.0], [-40.0, 0.0, -90.0]])
    gv = _pack_vertex48(pos, np.tile(np.array([0.0, 1.0, 0.0]), (4, 1)), np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=f32),
                        np.tile(np.array([1.0, 0.0, 0.0, 1.0]), (4, 1)))
    gi = np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32)
    eye4 = np.eye(4, dtype=f32)
    sphere = displaced_sphere(24, 17, width, height, seed=3).draws[0]
    sphere_model = trs(CASCADED_GROUND_SPHERE[0], (0.0, 0.0, 0.0, 1.0), CASCADED_GROUND_SPHERE[1])
    draws = [DrawSpec(vertices=gv, stride=48, count=gi.size, indices=gi, program=PROGRAM_MODEL_PBR, cull_mode=CULL_NONE, camera=cam,
                      object=object_ubo(eye4), light=light, material=pbr_material_ubo((0.8, 0.8, 0.75, 1.0), 0.0, 0.7))]
    meshes = []
    for centre, half in cascaded_ground_boxes(lam):
        bv, bi = _box_mesh(centre, half)
        meshes.append((bv, bi, eye4, CULL_NONE))
        draws.append(DrawSpec(vertices=bv, stride=48, count=bi.size, indices=bi, program=PROGRAM_MODEL_PBR, cull_mode=CULL_BACK,
                              front_face=FRONT_CCW, camera=cam, object=object_ubo(eye4), light=light,
                              material=pbr_material_ubo((0.6, 0.3, 0.2, 1.0), 0.0, 0.5)))
    meshes.append((sphere.vertices, sphere.indices, sphere_model, CULL_NONE))
    draws.append(DrawSpec(vertices=sphere.vertices, stride=48, count=sphere.count, indices=sphere.indices, program=PROGRAM_MODEL_PBR,
                          cull_mode=CULL_BACK, front_face=sphere.front_face, camera=cam, object=object_ubo(sphere_model), light=light,
                          material=pbr_material_ubo((0.2, 0.4, 0.8, 1.0), 0.3, 0.4)))
    casters = [[DrawSpec(vertices=v, stride=48, count=int(i.size), indices=i, program=PROGRAM_SHADOW, cull_mode=cull,
                         camera=shadow_constants_ubo(flip_clip_y(m), model)) for v, i, model, cull in meshes] for m in cas.matrices]
    spec = CascadeSpec(casters, (map_size, map_size), csm_ubo(cas.matrices, cas.split_depths, 0.005, 0.01, float(map_size)),
                       blend_threshold=float(blend_threshold))
    return Scene("cascaded-ground", width, height, draws, clear_color=(0.02, 0.02, 0.03, 1.0), cascades=spec)


# ------------------------------------------------------------------------------------------------
# Multiview depth scopes (include/mirhi.h "Multiview depth scopes"): all cascades of a CascadeSpec in ONE rendering scope
# ------------------------------------------------------------------------------------------------
MULTIVIEW_STRIDE = 80                                               # the stride of CSMParams' cascades (shadow_csm.hlsli:23-28)


def cascade_view_constants(spec: CascadeSpec, stride: int = MULTIVIEW_STRIDE) -> bytes:
    """The view constants of a multiview shadow scope over spec's cascades: view k's 64-byte light matrix at k * stride, in the layout of
    CSMParams' cascades.  The matrix is the one cascade k's casters render with (the first 64 bytes of their ShadowConstants): flip_clip_y(M_k),
    NOT the M_k that csm_ubo stores for the lookup -- these scenes render the map with clip y negated, so the shadow pass and the lookup
    cannot share one buffer; what they share is the layout."""
    out = bytearray(stride * len(spec.casters))
    for k, layer in enumerate(spec.casters):
        mats = {bytes(c.camera[:64]) for c in layer}
        assert len(mats) == 1, "the casters of one cascade render with one light matrix"
        out[k * stride:k * stride + 64] = mats.pop()
    return bytes(out)


def record_cascades_multiview(cmd, spec: CascadeSpec, array, states, view_constants, view_mask: Optional[int] = None, stride: int = MULTIVIEW_STRIDE):
    """Records all cascades of `spec` as ONE multiview scope into `cmd` (a recording CommandBuffer): the casters once -- `states`: per caster of ONE
    cascade a dict of pipe / vb / ib / camera buffers and the DrawSpec (`draw`), what SceneResources keeps per layer; every cascade has the same casters
    under another light matrix, and the caster's own CAMERA block still supplies `model` @64 -- into the layers of `array` that view_mask names (all of
    them by default), with view k's matrix at k * stride of the buffer view_constants (cascade_view_constants)."""
    w, h = spec.size
    mask = (1 << len(spec.casters)) - 1 if view_mask is None else int(view_mask)
    cmd.begin_rendering_multiview(array, mask, view_constants, 0, stride, clear_depth=spec.clear_depth, depth_load_op=spec.load_op)
    for st in states:
        d = st["draw"]
        cmd.set_viewport(*(d.viewport or (0.0, 0.0, float(w), float(h), 0.0, 1.0)))
        cmd.set_scissor(*(d.scissor or (0, 0, w, h)))
        cmd.bind_pipeline(st["pipe"])
        cmd.bind_vertex_buffers(0, [st["vb"]], [0])
        cmd.bind_uniform(0, st["camera"])                          # Slot.CAMERA
        if st["ib"] is not None:
            cmd.bind_index_buffer(st["ib"], 0, 0 if d.index_type == 2 else 1)      # IndexType.UINT16 / UINT32
            cmd.draw_indexed(d.count, 1, d.first, d.vertex_offset, 0)
        else:
            cmd.draw(d.count, 1, d.first, 0)
    cmd.end_rendering()


# ------------------------------------------------------------------------------------------------
# 4x MSAA (include/mirhi.h "4x MSAA"): the float64 model of a multisampled scope
# ------------------------------------------------------------------------------------------------
# Vulkan's standard 4x sample positions inside a pixel, as (x, y) fractions; in 1/256 px (96, 32), (224, 96), (32, 160), (160, 224)
MSAA_SAMPLES = ((0.375, 0.125), (0.875, 0.375), (0.125, 0.625), (0.625, 0.875))
NO_PRIM = 0xFFFFFFFF


def msaa_resolve(c0, c1, c2, c3, dtype=np.float64):
    """AVERAGE: ((c0 + c1) + (c2 + c3)) / 4 per channel, every operation rounded to `dtype` (np.float32: the bits the kernel stores)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=dtype) for c in (c0, c1, c2, c3))
    return (((c0 + c1).astype(dtype) + (c2 + c3).astype(dtype)).astype(dtype) * dtype(0.25)).astype(dtype)


def msaa_sample_scene(scene: "Scene", s: int) -> "Scene":
    """The 1x scene whose frame is sample `s` of the multisampled frame of `scene`: every viewport moved by (1/2 - sx, 1/2 - sy), the scissors
    unchanged -- a pixel centre of the moved frame then sits where sample s of that pixel sat.  Bit for bit in winner and depth under the condition
    tests/msaa_cases.py states (the moved viewport must move every SNAPPED vertex by exactly that offset)."""
    import dataclasses
    sx, sy = MSAA_SAMPLES[s]
    draws = []
    for d in scene.draws:
        x, y, w, h, n, f = d.viewport or (0.0, 0.0, float(scene.width), float(scene.height), 0.0, 1.0)
        draws.append(dataclasses.replace(d, viewport=(x + (0.5 - sx), y + (0.5 - sy), w, h, n, f)))
    return dataclasses.replace(scene, draws=draws)


def _msaa_triangles(scene: "Scene"):
    """The TRIANGLE-program triangles of `scene` in primitive order: (snapped X, Y in 1/256 px oriented so that the interior has E > 0, window x / y / z
    of the three vertices as float64 in the ORIGINAL order, their colours, the draw) -- or None where the draw culls it.  The model takes vertices with
    w = 1 inside the guard band and depth range; it knows no clipping."""
    out = []
    for d in scene.draws:
        if d.program != PROGRAM_TRIANGLE:
            raise NotImplementedError("the float64 MSAA model shades the TRIANGLE program only")
        v = np.ascontiguousarray(d.vertices).view(np.uint8).reshape(-1, d.stride)[:, :24].copy().view(f32).reshape(-1, 6)
        idx = (np.asarray(d.indices, dtype=np.int64)[d.first:d.first + d.count] + d.vertex_offset) if d.indices is not None else np.arange(d.first, d.first + d.count)
        vx, vy, vw, vh, zn, zf = d.viewport or (0.0, 0.0, float(scene.width), float(scene.height), 0.0, 1.0)
        for _ in range(max(0, int(d.instances))):
            for t in range(d.count // 3):
                p = v[idx[3 * t:3 * t + 3]].astype(np.float64)
                # (the kernels' binary32 viewport transform, then the snap: round-half-even to 8 sub-pixel bits)
                xs = (p[:, 0].astype(f32) * f32(0.5 * vw) + f32(vx + 0.5 * vw)).astype(f32)
                ys = (p[:, 1].astype(f32) * f32(0.5 * vh) + f32(vy + 0.5 * vh)).astype(f32)
                zs = (p[:, 2].astype(f32) * f32(zf - zn) + f32(zn)).astype(f32).astype(np.float64)
                X = np.rint(xs.astype(np.float64) * 256.0).astype(np.int64)
                Y = np.rint(ys.astype(np.float64) * 256.0).astype(np.int64)
                S = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
                front = S < 0 if d.front_face == FRONT_CCW else S > 0
                culled = S == 0 or d.cull_mode == CULL_FRONT_AND_BACK or (d.cull_mode == CULL_BACK and not front) or (d.cull_mode == CULL_FRONT and front)
                if culled:
                    out.append(None)
                    continue
                order = [0, 2, 1] if S < 0 else [0, 1, 2]
                out.append(dict(X=X[order], Y=Y[order], z=zs[order], win=np.stack([xs, ys], axis=1).astype(np.float64), col=p[:, 3:6], draw=d))
    return out


def msaa_model(scene: "Scene", positions=MSAA_SAMPLES) -> dict:
    """The float64 model of one 4x multisampled scope of TRIANGLE-program draws (one depth state: test and write with an ordering compare op).
    Returns prim [H, W, 4] uint32 (the winner of each sample, NO_PRIM where none), depth [H, W, 4] float64 (the winner's depth plane at the sample,
    the clear depth where none), sample_color [H, W, 4 samples, 4] (the winner's colour at the PIXEL CENTRE, extrapolated where it does not cover
    the centre; the clear colour where none) and color [H, W, 4] = msaa_resolve of the four.  positions: the sample positions (a single (0.5, 0.5)
    repeated gives the 1x frame four times)."""
    H, W = scene.height, scene.width
    tris = _msaa_triangles(scene)
    prim = np.full((H, W, 4), NO_PRIM, dtype=np.uint32)
    depth = np.full((H, W, 4), float(np.float32(min(max(scene.clear_depth, 0.0), 1.0))), dtype=np.float64)
    scol = np.empty((H, W, 4, 4), dtype=np.float64)
    scol[:] = np.asarray(scene.clear_color, dtype=np.float32).astype(np.float64)
    ops = {d.depth_compare for d in scene.draws}
    assert len(ops) <= 1 and all(d.depth_test and d.depth_write for d in scene.draws), "one ordering depth state per multisampled scope"
    op = ops.pop() if ops else CMP_LESS
    for pid, t in enumerate(tris):
        if t is None:
            continue
        d, X, Y, z = t["draw"], t["X"], t["Y"], t["z"]
        sx0, sy0, sw, sh = d.scissor or (0, 0, W, H)
        x0, x1 = max(int(X.min()) >> 8, sx0, 0), min((int(X.max()) >> 8) + 1, sx0 + sw, W)
        y0, y1 = max(int(Y.min()) >> 8, sy0, 0), min((int(Y.max()) >> 8) + 1, sy0 + sh, H)
        if x0 >= x1 or y0 >= y1:
            continue
        px, py = np.meshgrid(np.arange(x0, x1), np.arange(y0, y1))
        # depth plane through the snapped vertices (float64; the kernels' binary32 plane agrees to rounding, exactly on dyadic inputs)
        fx1, fy1, fx2, fy2 = (X[1] - X[0]) / 256.0, (Y[1] - Y[0]) / 256.0, (X[2] - X[0]) / 256.0, (Y[2] - Y[0]) / 256.0
        area = fx1 * fy2 - fx2 * fy1
        zx = ((z[1] - z[0]) * fy2 - (z[2] - z[0]) * fy1) / area
        zy = ((z[2] - z[0]) * fx1 - (z[1] - z[0]) * fx2) / area
        # the colour at the pixel centre from the unsnapped window positions (pixel/triangle.hlsl through shade_triangle_program), extrapolating
        ax = t["win"][:, 0][:, None, None] - (px + 0.5)[None]
        ay = t["win"][:, 1][:, None, None] - (py + 0.5)[None]
        l = np.stack([ax[1] * ay[2] - ax[2] * ay[1], ax[2] * ay[0] - ax[0] * ay[2], ax[0] * ay[1] - ax[1] * ay[0]])
        with np.errstate(divide="ignore", invalid="ignore"):
            b = l / l.sum(axis=0)
        rgb = np.einsum("kyx,kc->yxc", b, t["col"])
        rgba = np.concatenate([rgb, np.ones(rgb.shape[:2] + (1,))], axis=2)
        for s, (fx, fy) in enumerate(positions):
            SX, SY = px * 256 + int(round(fx * 256)), py * 256 + int(round(fy * 256))
            inside = np.ones(px.shape, dtype=bool)
            for i in range(3):
                a, c = i, (i + 1) % 3
                dx, dy = int(X[c] - X[a]), int(Y[c] - Y[a])
                E = -dy * (SX - int(X[a])) + dx * (SY - int(Y[a]))
                topleft = dy < 0 or (dy == 0 and dx > 0)
                inside &= (E >= 0) if topleft else (E > 0)
            zz = np.clip(z[0] + (SX / 256.0 - X[0] / 256.0) * zx + (SY / 256.0 - Y[0] / 256.0) * zy, 0.0, 1.0)
            old = depth[y0:y1, x0:x1, s]
            if op in (CMP_LESS, CMP_GREATER):       # strict: a tie keeps the earlier primitive (and the clear depth); or-equal: the later one wins
                win = (zz < old) if op == CMP_LESS else (zz > old)
            else:
                win = (zz <= old) if op == CMP_LESS_OR_EQUAL else (zz >= old)
            win &= inside
            depth[y0:y1, x0:x1, s] = np.where(win, zz, old)
            prim[y0:y1, x0:x1, s] = np.where(win, np.uint32(pid), prim[y0:y1, x0:x1, s])
            scol[y0:y1, x0:x1, s] = np.where(win[..., None], rgba, scol[y0:y1, x0:x1, s])
    return dict(prim=prim, depth=depth, sample_color=scol, color=msaa_resolve(scol[:, :, 0], scol[:, :, 1], scol[:, :, 2], scol[:, :, 3]))


def msaa_triangle_colour(scene: "Scene", pid: int) -> np.ndarray:
    """[H, W, 4] float64: the colour the TRIANGLE program gives primitive `pid` of the scene at every pixel centre, extrapolated outside the triangle
    (what a multisampled scope shades for a winner that does not cover the centre)."""
    t = _msaa_triangles(scene)[pid]
    px, py = np.meshgrid(np.arange(scene.width), np.arange(scene.height))
    ax = t["win"][:, 0][:, None, None] - (px + 0.5)[None]
    ay = t["win"][:, 1][:, None, None] - (py + 0.5)[None]
    l = np.stack([ax[1] * ay[2] - ax[2] * ay[1], ax[2] * ay[0] - ax[0] * ay[2], ax[0] * ay[1] - ax[1] * ay[0]])
    rgb = np.einsum("kyx,kc->yxc", l / l.sum(axis=0), t["col"])
    return np.concatenate([rgb, np.ones(rgb.shape[:2] + (1,))], axis=2)
