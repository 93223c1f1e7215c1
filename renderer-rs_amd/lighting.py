"""numpy model of the lit fragment programs MODEL, MODEL_FULL and MODEL_PBR (direct lighting; shadow = 1), the yardstick the raster kernels and
the CPU oracle are measured against.  Written from the HLSL alone, cited line by line: shaders/hlsl/vertex/model.hlsl,
lights.hlsli:63-231, pbr.hlsli (DistributionGGX, GeometrySmith, FresnelSchlick, CalculatePBRDirect, ClampRoughness, CalculateHemisphereAmbient),
pixel/model.hlsl, pixel/model_full.hlsl:63-150 and pixel/model_pbr.hlsl:124-320 -- not from oracle/mirhi_oracle.c and not from the kernels.

Every function takes `dtype`: np.float64 is the model M64, np.float32 the same arithmetic in single precision with left-to-right sums, whose
distance to M64 is E32.  What the HLSL leaves to the implementation is this build's stated reading (DESIGN.md 5 and "Texture
fidelity"): perspective-correct barycentrics of the pixel centre from the original clip-space triangle in the 2-D homogeneous, pixel-relative form
(valid for w <= 0 vertices); REPEAT bilinear taps at u w - 1/2; trilinear filtering with lambda = 1/2 log2 max(|d(uv size)/dx|^2, |d(uv size)/dy|^2)
from the value one pixel right / one pixel down minus the value at the pixel, clamped to [0, levels - 1], over scenes.mip_chain; the sRGB EOTF per
texel.  Anisotropic taps and non-default sampler state are not modelled (K9 and tests/sampler_cases.py hold them).

Stated domain: finite light and material parameters.  Nothing here touches a GPU or the oracle.
"""
from __future__ import annotations

import numpy as np

from . import scenes as _scenes

PI = 3.14159265358979323846        # pbr.hlsli:17
EPSILON = 0.0001                   # pbr.hlsli:18
SPOT_RADIUS = 50.0                 # lights.hlsli:217, model_pbr.hlsl:287
NO_PRIM = 0xFFFFFFFF
LIT_PROGRAMS = (_scenes.PROGRAM_MODEL, _scenes.PROGRAM_MODEL_FULL, _scenes.PROGRAM_MODEL_PBR, _scenes.PROGRAM_MODEL_PBR_IBL)


# ---- small vector helpers: left-to-right sums ----------------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _length(v):
    return np.sqrt(_dot(v, v))


def _normalize(v):
    return v / _length(v)[..., None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _saturate(x):
    return np.minimum(np.maximum(x, x.dtype.type(0.0)), x.dtype.type(1.0))


def _max0(x):
    return np.maximum(x, x.dtype.type(0.0))


def _f(buf, index, count, dtype):
    """`count` float32 values of a uniform block, from float index `index`, promoted to dtype."""
    return np.frombuffer(bytes(buf), dtype=np.float32, count=count, offset=4 * index).astype(dtype)


def _mat4(buf, index, dtype):
    """A float4x4 of a uniform block as a maths matrix (rows): the blocks hold it column by column."""
    return _f(buf, index, 16, dtype).reshape(4, 4).T


# ---- lights.hlsli --------------------------------------------------------------------------------------------------------------------------------
def attenuation(distance, radius, dtype=np.float64):
    """CalculateAttenuation, lights.hlsli:63-73."""
    T = np.dtype(dtype).type
    distance = np.asarray(distance, dtype=dtype)
    att = T(1.0) / (distance * distance + T(1.0))                                  # :66
    falloff = _saturate(T(1.0) - distance / T(radius))                             # :69
    falloff = falloff * falloff                                                    # :70
    return att * falloff                                                           # :72


def spot_attenuation(light_dir, spot_dir, inner_cos, outer_cos, dtype=np.float64):
    """CalculateSpotAttenuation, lights.hlsli:77-81."""
    T = np.dtype(dtype).type
    cos_angle = _dot(-light_dir, spot_dir)                                         # :79
    return _saturate((cos_angle - T(outer_cos)) / (T(inner_cos) - T(outer_cos)))   # :80


def spot_direction(direction, dtype=np.float64):
    """normalize(light.Direction), lights.hlsli:223 and model_pbr.hlsl:293: the buffer's direction is not trusted to be normalised."""
    return _normalize(np.asarray(direction, dtype=dtype))


def roughness_to_shininess(roughness, dtype=np.float64):
    """RoughnessToShininess, lights.hlsli:152-159: lerp(2048, 2, clamp(roughness, 0, 1))."""
    T = np.dtype(dtype).type
    r = min(max(T(roughness), T(0.0)), T(1.0))                                     # :157
    return T(2048.0) + (T(2.0) - T(2048.0)) * r                                    # :158


def blinn_phong(light_dir, view_dir, normal, light_color, albedo, shininess, dtype=np.float64):
    """CalculateBlinnPhong, lights.hlsli:95-117.  light_color: [n, 3] or [3]."""
    T = np.dtype(dtype).type
    ndl = _max0(_dot(normal, light_dir))                                           # :104
    diffuse = ndl[..., None] * light_color * albedo                                # :105
    half_dir = _normalize(light_dir + view_dir)                                    # :112
    ndh = _max0(_dot(normal, half_dir))                                            # :113
    specular = np.power(ndh, T(shininess))[..., None] * light_color                # :114
    return np.where((ndl <= T(0.0))[..., None], diffuse, diffuse + specular)       # :108-109, :116


# ---- pbr.hlsli -----------------------------------------------------------------------------------------------------------------------------------
def distribution_ggx(ndh, roughness, dtype=np.float64):
    """DistributionGGX, pbr.hlsli:55-69, of NdotH = max(dot(N, H), 0) (:61)."""
    T = np.dtype(dtype).type
    a = roughness * roughness                                                      # :58
    a2 = a * a                                                                     # :59
    denom = (ndh * ndh) * (a2 - T(1.0)) + T(1.0)                                   # :62, :65
    denom = T(PI) * denom * denom                                                  # :66
    return a2 / np.maximum(denom, T(EPSILON))                                      # :68


def geometry_schlick_ggx(ndx, roughness, dtype=np.float64):
    """GeometrySchlickGGX, pbr.hlsli:83-93: k = (roughness + 1)^2 / 8, the remapping for direct light."""
    T = np.dtype(dtype).type
    r = roughness + T(1.0)                                                         # :88
    k = (r * r) / T(8.0)                                                           # :89
    denom = ndx * (T(1.0) - k) + k                                                 # :91
    return ndx / np.maximum(denom, T(EPSILON))                                     # :92


def geometry_smith(ndv, ndl, roughness, dtype=np.float64):
    """GeometrySmith, pbr.hlsli:106-115, of the two clamped cosines (:108-109)."""
    return geometry_schlick_ggx(ndv, roughness, dtype) * geometry_schlick_ggx(ndl, roughness, dtype)


def fresnel_schlick(cos_theta, F0, dtype=np.float64):
    """FresnelSchlick, pbr.hlsli:131-136."""
    T = np.dtype(dtype).type
    ct = _saturate(cos_theta)                                                      # :134
    return F0 + (T(1.0) - F0) * np.power(T(1.0) - ct, T(5.0))[..., None]           # :135


def clamp_roughness(roughness, dtype=np.float64):
    """ClampRoughness, pbr.hlsli:476-479."""
    return np.maximum(roughness, np.dtype(dtype).type(0.04))


def pbr_direct(N, V, L, radiance, albedo, metallic, roughness, dtype=np.float64):
    """CalculatePBRDirect, pbr.hlsli:292-333."""
    T = np.dtype(dtype).type
    H = _normalize(V + L)                                                          # :299
    F0 = T(0.04) + (albedo - T(0.04)) * metallic[..., None]                        # :304-305
    ndv, ndl = _max0(_dot(N, V)), _max0(_dot(N, L))
    NDF = distribution_ggx(_max0(_dot(N, H)), roughness, dtype)                    # :308
    G = geometry_smith(ndv, ndl, roughness, dtype)                                 # :309
    F = fresnel_schlick(_max0(_dot(H, V)), F0, dtype)                              # :310
    kD = (T(1.0) - F) * (T(1.0) - metallic)[..., None]                             # :316, :319
    numerator = (NDF * G)[..., None] * F                                           # :322
    denominator = T(4.0) * ndv * ndl + T(EPSILON)                                  # :323
    specular = numerator / denominator[..., None]                                  # :324
    return (kD * albedo / T(PI) + specular) * radiance * ndl[..., None]            # :332


def hemisphere_ambient(N, albedo, metallic, ao, dtype=np.float64):
    """CalculateHemisphereAmbient (pbr.hlsli:483-492) as model_pbr.hlsl:308 applies it: lerp(ground, sky, N.y / 2 + 1 / 2) * albedo * ao * (1 - metallic)."""
    T = np.dtype(dtype).type
    N, albedo = np.asarray(N, dtype=dtype), np.asarray(albedo, dtype=dtype)
    up = N[:, 1:2] * T(0.5) + T(0.5)                                               # :488
    ground, sky = np.array([0.08, 0.06, 0.04], dtype=dtype), np.array([0.15, 0.18, 0.25], dtype=dtype)   # :485-486
    return (ground + (sky - ground) * up) * albedo * np.asarray(ao, dtype=dtype)[..., None] * (T(1.0) - np.asarray(metallic, dtype=dtype))[:, None]


def direct_ao_scale(ao, dtype=np.float64):
    """lerp(1.0, material.ao, 0.5), model_pbr.hlsl:311: the partial influence of ao on direct light."""
    T = np.dtype(dtype).type
    return T(1.0) + (ao - T(1.0)) * T(0.5)


# ---- vertex/model.hlsl ---------------------------------------------------------------------------------------------------------------------------
def gram_schmidt(Tn, N):
    """T = normalize(T - dot(T, N) * N), vertex/model.hlsl:55."""
    return _normalize(Tn - _dot(Tn, N)[..., None] * N)


def vertex_varyings(draw, vidx, dtype=np.float64):
    """VSOutput of vertex/model.hlsl:39-68 for the vertex buffer elements `vidx` (any shape): clip [.., 4], world, normal, tangent, bitangent
    [.., 3] and uv [.., 2], from the draw's float32 uniform blocks and vertex bytes promoted to dtype (`Vertex` 48 B: position @0, normal @12,
    uv @24, tangent @32)."""
    vidx = np.asarray(vidx, dtype=np.int64)
    vb = draw.vertex_bytes()
    n = vb.size // draw.stride
    rows = np.ascontiguousarray(vb[:n * draw.stride].reshape(n, draw.stride)[vidx.reshape(-1), :48]).view(np.float32).astype(dtype)
    rows = rows.reshape(vidx.shape + (12,))
    pos, nrm, uv, tan, tw = rows[..., 0:3], rows[..., 3:6], rows[..., 6:8], rows[..., 8:11], rows[..., 11]
    model, normal_matrix = _mat4(draw.object, 0, dtype), _mat4(draw.object, 16, dtype)
    view_proj = _mat4(draw.camera, 32, dtype)
    mul4 = lambda M, v: ((M[:, 0] * v[..., 0:1] + M[:, 1] * v[..., 1:2]) + M[:, 2] * v[..., 2:3]) + M[:, 3] * v[..., 3:4]
    mul3 = lambda M, v: (M[:3, 0] * v[..., 0:1] + M[:3, 1] * v[..., 1:2]) + M[:3, 2] * v[..., 2:3]
    world = mul4(model, np.concatenate([pos, np.ones(pos.shape[:-1] + (1,), dtype=dtype)], axis=-1))      # :44
    clip = mul4(view_proj, world)                                                  # :48
    N = _normalize(mul3(normal_matrix, nrm))                                       # :51
    Tn = _normalize(mul3(model, tan))                                              # :52
    Tn = gram_schmidt(Tn, N)                                                       # :55
    B = _cross(N, Tn) * tw[..., None]                                              # :58
    return dict(clip=clip, world=world[..., :3], normal=N, tangent=Tn, bitangent=B, uv=uv)


def barycentrics(clip, pxc, pyc, viewport, dtype=np.float64):
    """Perspective-correct barycentrics [n, 3] of the points (pxc, pyc) (window coordinates) in the clip-space triangles clip [n, 3, 4]: with
    a_i = ((x_i W/2 + w_i cx) - px w_i, (y_i H/2 + w_i cy) - py w_i), lambda_0 = a_1 x a_2, ..., b_i = lambda_i / sum lambda.  Nothing is divided
    by w, so vertices with w <= 0 are as good as any."""
    T = np.dtype(dtype).type
    hw, hh = T(0.5) * T(viewport[2]), T(0.5) * T(viewport[3])
    cx, cy = T(viewport[0]) + hw, T(viewport[1]) + hh
    x, y, w = clip[..., 0], clip[..., 1], clip[..., 3]
    ax = (x * hw + w * cx) - pxc[:, None] * w
    ay = (y * hh + w * cy) - pyc[:, None] * w
    l0 = ax[:, 1] * ay[:, 2] - ax[:, 2] * ay[:, 1]
    l1 = ax[:, 2] * ay[:, 0] - ax[:, 0] * ay[:, 2]
    l2 = ax[:, 0] * ay[:, 1] - ax[:, 1] * ay[:, 0]
    return np.stack([l0, l1, l2], axis=-1) / ((l0 + l1) + l2)[:, None]


def _interp(b, a):
    """sum b_i a_i of the per-vertex values a [n, 3, k]."""
    return (b[:, 0:1] * a[:, 0] + b[:, 1:2] * a[:, 1]) + b[:, 2:3] * a[:, 2]


# ---- textures ------------------------------------------------------------------------------------------------------------------------------------
def srgb_decode(byte, dtype=np.float64):
    """The sRGB EOTF of a stored byte (IEC 61966-2-1), evaluated in float64 and rounded to dtype once."""
    c = np.asarray(byte, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, np.power((c + 0.055) / 1.055, 2.4)).astype(dtype)


def _texels(level, srgb, x, y, dtype):
    """RGBA of the texels (x, y) of one level under REPEAT addressing: UNORM byte / 255, RGB through the EOTF on an sRGB texture."""
    h, w = level.shape[:2]
    t = level[np.mod(y, h), np.mod(x, w)]
    out = t.astype(dtype) / np.dtype(dtype).type(255.0)
    if srgb:
        out[..., :3] = srgb_decode(t[..., :3], dtype)
    return out


def sample_bilinear(level, srgb, u, v, dtype=np.float64):
    """One bilinear tap of an [h, w, 4] uint8 level at (u, v): the four texels around (u w - 1/2, v h - 1/2), REPEAT."""
    T = np.dtype(dtype).type
    h, w = level.shape[:2]
    fx, fy = u * T(w) - T(0.5), v * T(h) - T(0.5)
    x0f, y0f = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0f)[:, None], (fy - y0f)[:, None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    c00, c10 = _texels(level, srgb, x0, y0, dtype), _texels(level, srgb, x0 + 1, y0, dtype)
    c01, c11 = _texels(level, srgb, x0, y0 + 1, dtype), _texels(level, srgb, x0 + 1, y0 + 1, dtype)
    top, bot = c00 + (c10 - c00) * ax, c01 + (c11 - c01) * ax
    return top + (bot - top) * ay


def texture_lambda(texture, grad, dtype=np.float64):
    """lambda of a texture before clamping: 1/2 log2 max(|d(u w, v h)/dx|^2, |d(u w, v h)/dy|^2); grad = (dudx, dvdx, dudy, dvdy), each the
    value one pixel right / down minus the value at the pixel."""
    T = np.dtype(dtype).type
    w, h = T(texture.width), T(texture.height)
    ax, bx, ay, by = grad[0] * w, grad[1] * h, grad[2] * w, grad[3] * h
    rx, ry = ax * ax + bx * bx, ay * ay + by * by
    with np.errstate(divide="ignore"):
        return T(0.5) * np.log2(np.maximum(rx, ry))


def sample_trilinear(texture, u, v, grad, dtype=np.float64):
    """A texture with a chain (scenes.mip_chain): lambda clamped to [0, levels - 1], the two levels around it, linear blend."""
    T = np.dtype(dtype).type
    chain = _scenes.mip_chain(texture.rgba8)
    lam = np.minimum(np.maximum(texture_lambda(texture, grad, dtype), T(0.0)), T(len(chain) - 1))
    l0f = np.floor(lam)
    f, l0 = (lam - l0f)[:, None], l0f.astype(np.int64)
    out = np.zeros(u.shape + (4,), dtype=dtype)
    for l in range(len(chain)):
        m = l0 == l
        if not m.any():
            continue
        c0 = sample_bilinear(chain[l], texture.srgb, u[m], v[m], dtype)
        if l + 1 < len(chain):
            c1 = sample_bilinear(chain[l + 1], texture.srgb, u[m], v[m], dtype)
            c0 = c0 + (c1 - c0) * f[m]
        out[m] = c0
    return out


def sample_texture(texture, u, v, grad, dtype=np.float64):
    """Texture2D.Sample: white where nothing is bound (the default 1x1 white texture, model_full.hlsl:92), bilinear without a chain, trilinear with."""
    if texture is None:
        return np.ones(u.shape + (4,), dtype=dtype)
    if not texture.mips:
        return sample_bilinear(np.asarray(texture.rgba8), texture.srgb, u, v, dtype)
    return sample_trilinear(texture, u, v, grad, dtype)


def world_normal(N, Tn, B, normal_sample, normal_scale=None, dtype=np.float64):
    """GetWorldNormal past its early returns (model_full.hlsl:73-82; model_pbr.hlsl:143-156 with normal_scale): the tangent-space sample [n, 3] in
    [0, 1] taken to world space through normalize(T), normalize(B), N (already normalised)."""
    T = np.dtype(dtype).type
    ns = normal_sample * T(2.0) - T(1.0)                                           # full :74, pbr :144
    if normal_scale is not None:
        ns = _normalize(np.concatenate([ns[:, :2] * T(normal_scale), ns[:, 2:3]], axis=-1))      # pbr :147-148
    Tn, B = _normalize(Tn), _normalize(B)                                          # full :77-78, pbr :151-152
    return _normalize((ns[:, 0:1] * Tn + ns[:, 1:2] * B) + ns[:, 2:3] * N)         # mul(normalSample, float3x3(T, B, N))


# ---- the light loops -----------------------------------------------------------------------------------------------------------------------------
def _lights(draw, world, dtype):
    """(L [n, 3], radiance [n, 3], attenuation [n] or None, kind) of the directional light, the point lights and the spot lights in shader order:
    lights.hlsli:174-175, :191-196, :212-227 == model_pbr.hlsl:236-237, :259-268, :279-297."""
    T = np.dtype(dtype).type
    n = world.shape[0]
    lu = bytes(draw.light)
    direction, intensity, color = _f(lu, 0, 3, dtype), _f(lu, 3, 1, dtype)[0], _f(lu, 4, 3, dtype)
    counts = np.frombuffer(lu, dtype=np.uint32, count=2, offset=32)
    out = [(np.broadcast_to(_normalize(-direction), (n, 3)), np.broadcast_to(color * intensity, (n, 3)), None, "directional")]
    pl, sl = bytes(draw.point_lights or b""), bytes(draw.spot_lights or b"")
    for i in range(min(int(counts[0]), len(pl) // 32)):
        p = _f(pl, 8 * i, 8, dtype)                                                # Position, Radius, Color, Intensity
        vec = p[0:3] - world
        dist = _length(vec)
        att = attenuation(dist, p[3], dtype)
        out.append((vec / dist[:, None], (p[4:7] * p[7]) * att[:, None], att, "point"))
    for j in range(min(int(counts[1]), len(sl) // 48)):
        s = _f(sl, 12 * j, 12, dtype)                                              # Position, InnerCone, Direction, OuterCone, Color, Intensity
        vec = s[0:3] - world
        dist = _length(vec)
        L = vec / dist[:, None]
        datt = attenuation(dist, T(SPOT_RADIUS), dtype)
        satt = spot_attenuation(L, spot_direction(s[4:7], dtype), s[3], s[7], dtype)
        out.append((L, ((s[8:11] * s[11]) * datt[:, None]) * satt[:, None], datt * satt, "spot"))
    return out


def _note_lights(aux, lights, N):
    if aux is not None:
        aux["attenuation"] = [(kind, att) for _, _, att, kind in lights if att is not None]
        aux["ndl"] = np.stack([_dot(N, L) for L, _, _, _ in lights], axis=-1)
        aux["lit"] = np.stack([np.any(rad != 0, axis=-1) for _, rad, _, _ in lights], axis=-1)


# ---- the fragment programs -----------------------------------------------------------------------------------------------------------------------
def shade_model(draw, pix, dtype=np.float64, aux=None):
    """pixel/model.hlsl:29-82: the fallback constants, one directional Blinn-Phong light, ambient 0.03."""
    T = np.dtype(dtype).type
    n = pix["world"].shape[0]
    albedo = np.full(3, 0.7, dtype=dtype)                                          # :36
    one = np.ones(3, dtype=dtype)
    L = np.broadcast_to(_normalize(one), (n, 3))                                   # :41
    N = _normalize(pix["normal"])                                                  # :50
    V = _normalize(_f(draw.camera, 48, 3, dtype) - pix["world"])                   # :53
    ambient = T(0.03) * albedo * T(1.0)                                            # :60
    lighting = blinn_phong(L, V, N, one * T(1.0), albedo, roughness_to_shininess(0.5, dtype), dtype)        # :63-73
    if aux is not None:
        aux["ndl"], aux["lit"], aux["attenuation"] = _dot(N, L)[:, None], np.ones((n, 1), dtype=bool), []
    return np.concatenate([ambient + lighting, np.ones((n, 1), dtype=dtype)], axis=-1)        # :79-81


def shade_model_full(draw, pix, dtype=np.float64, aux=None):
    """pixel/model_full.hlsl:85-150 with GetWorldNormal :63-83 and the three light helpers of lights.hlsli:166-231."""
    T = np.dtype(dtype).type
    u, v = pix["uv"][:, 0], pix["uv"][:, 1]
    m = _f(draw.material, 0, 8, dtype)                                             # baseColor, metallic, roughness, ambientOcclusion :34-41
    base, roughness, ao = m[0:4], m[5], m[6]
    albedo_sample = sample_texture(draw.albedo_map, u, v, pix["grad"], dtype)      # :88
    albedo = albedo_sample[:, :3] * base[:3]                                       # :89
    check = sample_texture(draw.normal_map, u, v, pix["grad"], dtype)[:, :3]       # :93
    has_map = _length(check - T(1.0)) > T(0.01)                                    # :94
    N = _normalize(pix["normal"])                                                  # :65
    if has_map.any():
        N = np.where(has_map[:, None], world_normal(N, pix["tangent"], pix["bitangent"], check, None, dtype), N)
    V = _normalize(_f(draw.camera, 48, 3, dtype) - pix["world"])                   # :100
    ambient = T(0.03) * albedo * ao                                                # :103
    shininess = roughness_to_shininess(roughness, dtype)                           # lights.hlsli:176, :197, :228
    lights = _lights(draw, pix["world"], dtype)
    lighting = np.zeros_like(albedo)                                               # :106
    for L, color, _, _ in lights:                                                  # :109-144
        lighting = lighting + blinn_phong(L, V, N, color, albedo, shininess, dtype)
    _note_lights(aux, lights, N)
    return np.concatenate([ambient + lighting, (albedo_sample[:, 3] * base[3])[:, None]], axis=-1)          # :147-149


def shade_model_pbr(draw, pix, dtype=np.float64, aux=None, ibl_zero_env=False):
    """pixel/model_pbr.hlsl:159-320 with GetWorldNormal :128-157; shadow = 1 (no map bound, or a map cleared to 1.0).  ibl_zero_env: what
    MODEL_PBR_IBL leaves of it under an all-zero environment -- no hemisphere ambient, and direct light not scaled by ao."""
    T = np.dtype(dtype).type
    u, v, grad = pix["uv"][:, 0], pix["uv"][:, 1], pix["grad"]
    M = bytes(draw.material)
    m = _f(M, 0, 12, dtype)                                                        # :42-48
    has = np.frombuffer(M, dtype=np.int32, count=5, offset=48)                     # :51-55
    n = u.shape[0]
    base = np.broadcast_to(m[0:4], (n, 4))
    if has[0] != 0:
        base = sample_texture(draw.albedo_map, u, v, grad, dtype) * m[0:4]         # :169
    albedo = base[:, :3]                                                           # :182
    metallic, roughness = np.full(n, m[4], dtype=dtype), np.full(n, m[5], dtype=dtype)        # :185-186
    if has[2] != 0:
        mr = sample_texture(draw.metallic_roughness_map, u, v, grad, dtype)        # :189
        roughness, metallic = roughness * mr[:, 1], metallic * mr[:, 2]            # :190-191
    ao = np.full(n, m[6], dtype=dtype)                                             # :195
    if has[3] != 0:
        ao = ao * sample_texture(draw.occlusion_map, u, v, grad, dtype)[:, 0]      # :198
    emissive = np.broadcast_to(m[8:11], (n, 3))                                    # :202
    if has[4] != 0:
        emissive = emissive * sample_texture(draw.emissive_map, u, v, grad, dtype)[:, :3]     # :205
    N = _normalize(pix["normal"])                                                  # :130
    if has[1] != 0:                                                                # :133
        ns = sample_texture(draw.normal_map, u, v, grad, dtype)[:, :3]             # :137
        valid = ~(_length(ns - T(1.0)) < T(0.01))                                  # :140
        if valid.any():
            N = np.where(valid[:, None], world_normal(N, pix["tangent"], pix["bitangent"], ns, m[7], dtype), N)
    V = _normalize(_f(draw.camera, 48, 3, dtype) - pix["world"])                   # :216
    roughness = clamp_roughness(roughness, dtype)                                  # :219
    lights = _lights(draw, pix["world"], dtype)
    lighting = np.zeros((n, 3), dtype=dtype)                                       # :230
    for L, radiance, _, _ in lights:                                               # :251, :271, :300
        lighting = lighting + pbr_direct(N, V, L, radiance, albedo, metallic, roughness, dtype)
    _note_lights(aux, lights, N)
    if ibl_zero_env:
        color = lighting + emissive
    else:
        ambient = hemisphere_ambient(N, albedo, metallic, ao, dtype)               # :308
        lighting = lighting * direct_ao_scale(ao, dtype)[:, None]                  # :311
        color = (ambient + lighting) + emissive                                    # :317
    return np.concatenate([color, base[:, 3:4]], axis=-1)                          # :319


# ---- a frame -------------------------------------------------------------------------------------------------------------------------------------
def fetch_triangles(draw):
    """[count / 3, 3] vertex buffer elements of a draw's triangle list: `first`, the index type and `vertex_offset` honoured."""
    k = np.arange(3 * (draw.count // 3), dtype=np.int64) + int(draw.first)
    if draw.indices is not None:
        k = np.asarray(draw.indices).reshape(-1)[k].astype(np.int64) + int(draw.vertex_offset)
    return k.reshape(-1, 3)


def pixel_inputs(scene, draw, tri, px, py, dtype=np.float64):
    """The interpolated PSInput of the pixels (px, py) covered by triangles `tri` (indices into the draw's list) of one draw, and the footprint of uv."""
    T = np.dtype(dtype).type
    vv = vertex_varyings(draw, fetch_triangles(draw)[tri], dtype)
    viewport = draw.viewport or (0.0, 0.0, float(scene.width), float(scene.height), 0.0, 1.0)
    pxc, pyc = px.astype(dtype) + T(0.5), py.astype(dtype) + T(0.5)
    b = barycentrics(vv["clip"], pxc, pyc, viewport, dtype)
    pix = {k: _interp(b, vv[k]) for k in ("world", "normal", "tangent", "bitangent", "uv")}
    right = _interp(barycentrics(vv["clip"], pxc + T(1.0), pyc, viewport, dtype), vv["uv"]) - pix["uv"]
    down = _interp(barycentrics(vv["clip"], pxc, pyc + T(1.0), viewport, dtype), vv["uv"]) - pix["uv"]
    pix["grad"] = (right[:, 0], right[:, 1], down[:, 0], down[:, 1])
    pix["b"] = b
    return pix


def shade_frame(scene, prim, dtype=np.float64, ibl_zero_env=False, want_aux=False):
    """The expected RGBA of every pixel of a prim-id image whose primitive belongs to a MODEL, MODEL_FULL, MODEL_PBR (or, with ibl_zero_env,
    MODEL_PBR_IBL) draw: (py, px, rgba [n, 4], aux).  Primitive ids count the triangles of the scene's draws in order, an instanced draw once per
    instance.  aux (want_aux) holds per pixel `ndl` and `lit` [n, lights], `draw`, and per draw the attenuations and lambdas."""
    prim = np.asarray(prim)
    py, px = np.nonzero(prim != NO_PRIM)
    pid = prim[py, px].astype(np.int64)
    rgba = np.zeros((py.size, 4), dtype=dtype)
    done = np.zeros(py.size, dtype=bool)
    aux = dict(draws={}) if want_aux else None
    base = 0
    for di, draw in enumerate(scene.draws):
        ntri = draw.count // 3
        total = ntri * max(0, int(getattr(draw, "instances", 1)))
        sel = np.nonzero((pid >= base) & (pid < base + total))[0]
        local = (pid[sel] - base) % max(ntri, 1)
        base += total
        if sel.size == 0 or draw.program not in LIT_PROGRAMS or (draw.program == _scenes.PROGRAM_MODEL_PBR_IBL and not ibl_zero_env):
            continue
        pix = pixel_inputs(scene, draw, local, px[sel], py[sel], dtype)
        a = {} if want_aux else None
        if draw.program == _scenes.PROGRAM_MODEL:
            rgba[sel] = shade_model(draw, pix, dtype, a)
        elif draw.program == _scenes.PROGRAM_MODEL_FULL:
            rgba[sel] = shade_model_full(draw, pix, dtype, a)
        else:
            rgba[sel] = shade_model_pbr(draw, pix, dtype, a, ibl_zero_env=ibl_zero_env or draw.program == _scenes.PROGRAM_MODEL_PBR_IBL)
        done[sel] = True
        if want_aux:
            a["sel"], a["grad"] = sel, pix["grad"]
            aux["draws"][di] = a
    if want_aux:
        place = np.cumsum(done) - 1                  # `sel` as positions in the arrays returned
        for a in aux["draws"].values():
            a["sel"] = place[a["sel"]]
    return py[done], px[done], rgba[done], aux
