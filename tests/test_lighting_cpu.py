"""The float64 model of the lit fragment programs (renderer-rs_amd/lighting.py) without a GPU: the model against closed forms, the
CPU oracle against the model on every case of tests/lighting_cases.py under the measure of DESIGN.md 8d, the conditions the cases promise (from the
float64 model alone), and planted errors: a model with one subtle mistake must put the oracle's frame outside the bound."""
import dataclasses
import math

import numpy as np
import pytest

import lighting_cases as lc


@pytest.fixture(scope="module")
def lighting(mirhi):
    return mirhi.lighting


_oracle_frames = {}


def _oracle_frame(oracle, scene):
    if scene.name not in _oracle_frames:
        _oracle_frames[scene.name] = oracle.render(scene, want_bgra8=False)
    return _oracle_frames[scene.name]


# ---- the model against closed forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_attenuation_and_cone_closed_forms(lighting, dtype):
    att = lighting.attenuation(np.array([0.0, 1.0, 2.0, 5.0, 7.5, 1e9]), 5.0, dtype)
    assert att.dtype == dtype
    assert att[0] == 1.0 and att[3] == 0.0 and att[4] == 0.0 and att[5] == 0.0             # d = 0: 1; d >= radius: exactly 0
    assert att[1] == pytest.approx(0.5 * 0.8 ** 2, rel=1e-6) and att[2] == pytest.approx(0.2 * 0.6 ** 2, rel=1e-6)
    # the cone: 1 at the inner cosine and inside it, 0 at the outer cosine and outside, linear in the cosine between
    spot = np.array([[0.0, 0.0, -1.0]], dtype=dtype)
    inner, outer = 0.9, 0.6
    for cos_angle, want in ((1.0, 1.0), (inner, 1.0), (outer, 0.0), (0.3, 0.0), (-1.0, 0.0), (0.75, 0.5)):
        L = -np.array([[math.sqrt(1.0 - cos_angle ** 2), 0.0, -cos_angle]], dtype=dtype)   # lightDir: from the surface to the light
        got = lighting.spot_attenuation(L, spot, inner, outer, dtype)[0]
        assert got == pytest.approx(want, abs=1e-6), cos_angle
    assert np.allclose(lighting.spot_direction(np.array([0.0, 3.0, -4.0])), [0.0, 0.6, -0.8], atol=1e-15)
    assert lighting.roughness_to_shininess(0.0) == 2048.0 and lighting.roughness_to_shininess(1.0) == 2.0 and lighting.roughness_to_shininess(0.5) == 1025.0
    assert lighting.roughness_to_shininess(-3.0) == 2048.0 and lighting.roughness_to_shininess(7.0) == 2.0


def test_k3_fallback_pixel(lighting, scenes):
    """N = L = V = normalize(1, 1, 1): pixel/model.hlsl gives 0.03 * 0.7 + 0.7 + 1 = 1.721 (K3)."""
    n = np.array([[1.0, 1.0, 1.0]]) / math.sqrt(3.0)
    eye = n[0] * 10.0
    cam = scenes.camera_ubo(np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), tuple(eye))
    draw = scenes.DrawSpec(vertices=np.zeros((3, 12), dtype=np.float32), stride=48, count=3, camera=cam)
    out = lighting.shade_model(draw, dict(world=np.zeros((1, 3)), normal=n * 3.0))
    assert np.allclose(out[0], [1.721, 1.721, 1.721, 1.0], rtol=0, atol=1e-6)
    # facing away: no diffuse, and no specular either (lights.hlsli:108-109)
    out = lighting.shade_model(draw, dict(world=np.zeros((1, 3)), normal=-n))
    assert np.allclose(out[0, :3], 0.021, rtol=0, atol=1e-15)


def test_brdf_terms_closed_forms(lighting):
    one, half = np.array([1.0]), np.array([0.5])
    assert lighting.distribution_ggx(one, half)[0] == pytest.approx(1.0 / (math.pi * 0.0625), rel=1e-14)
    for x in (0.0, 0.3, 1.0):
        assert lighting.distribution_ggx(np.array([x]), one)[0] == pytest.approx(1.0 / math.pi, rel=1e-14)
    assert lighting.distribution_ggx(one, np.array([0.01]))[0] == pytest.approx(1e-8 / 1e-4, rel=1e-12)          # EPSILON clamp, pbr.hlsli:68
    for r in (0.04, 0.3, 1.0):
        assert lighting.geometry_schlick_ggx(one, np.array([r]))[0] == pytest.approx(1.0, rel=1e-14)               # G(1, r) = 1
    assert lighting.geometry_schlick_ggx(half, one)[0] == pytest.approx(0.5 / 0.75, rel=1e-14)
    assert lighting.geometry_schlick_ggx(np.array([0.0]), np.array([0.7]))[0] == 0.0
    # k -> EPSILON clamp of the denominator: NdotV = 0 and k = 0 cannot happen (k >= 1/8), so the clamp only guards; state it
    assert lighting.geometry_smith(one, half, one)[0] == pytest.approx(0.5 / 0.75, rel=1e-14)
    assert np.array_equal(lighting.clamp_roughness(np.array([0.0, 0.039, 0.04, 0.5, 1.0])), [0.04, 0.04, 0.04, 0.5, 1.0])
    F0 = np.array([[0.04, 0.5, 0.9]])
    assert np.array_equal(lighting.fresnel_schlick(np.array([1.0]), F0), F0) and np.allclose(lighting.fresnel_schlick(np.array([0.0]), F0), 1.0, atol=1e-15)
    assert np.array_equal(lighting.fresnel_schlick(np.array([1.5]), F0), F0)                                      # saturate
    assert lighting.direct_ao_scale(np.array([0.6]))[0] == pytest.approx(0.8, rel=1e-15)
    # CalculatePBRDirect at N = V = L, dielectric, roughness 1: kD = 0.96, D = 1/pi, G = 1, F = 0.04 -> (0.96 albedo / pi + 0.04 / (pi (4 + 1e-4))) radiance
    n = np.array([[0.0, 0.0, 1.0]])
    albedo, rad = np.array([[0.8, 0.5, 0.3]]), np.array([[2.0, 1.0, 0.5]])
    got = lighting.pbr_direct(n, n, n, rad, albedo, np.array([0.0]), np.array([1.0]))
    want = (0.96 * albedo / math.pi + (1.0 / math.pi) * 0.04 / (4.0 + 1e-4)) * rad
    assert np.allclose(got, want, rtol=1e-13, atol=0)
    # a metal has no diffuse term: at metallic 1 the result is the specular term alone, F0 = albedo
    got = lighting.pbr_direct(n, n, n, rad, albedo, np.array([1.0]), np.array([1.0]))
    assert np.allclose(got, (1.0 / math.pi) * albedo / (4.0 + 1e-4) * rad, rtol=1e-13, atol=0)
    assert np.allclose(lighting.hemisphere_ambient(np.array([[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]]), np.ones((2, 3)), np.array([0.0, 0.5]), np.array([1.0, 0.5])),
                       [[0.15, 0.18, 0.25], [0.02, 0.015, 0.01]], atol=1e-15)


def test_tbn_of_an_identity_frame(lighting, scenes):
    """Identity model matrix, N = +z, T = +x: B = +y for w = +1 and -y for w = -1; a sample (1, 1/2, 1/2) maps to +x, and (1/2, 1, 1/2) to +-y."""
    verts = np.zeros((2, 12), dtype=np.float32)
    verts[:, 3:6] = [0, 0, 2]; verts[:, 8:11] = [3, 0, 1]; verts[:, 11] = [1, -1]        # tangent not orthogonal to the normal: Gram-Schmidt
    draw = scenes.DrawSpec(vertices=verts, stride=48, count=0, object=scenes.object_ubo(np.eye(4, dtype=np.float32)),
                           camera=scenes.camera_ubo(np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), (0, 0, 1)))
    vv = lighting.vertex_varyings(draw, np.array([0, 1]))
    assert np.allclose(vv["normal"], [[0, 0, 1]] * 2, atol=1e-15) and np.allclose(vv["tangent"], [[1, 0, 0]] * 2, atol=1e-15)
    assert np.allclose(vv["bitangent"], [[0, 1, 0], [0, -1, 0]], atol=1e-15)
    s = np.array([[1.0, 0.5, 0.5], [0.5, 1.0, 0.5]])
    for k, want in ((0, [[1, 0, 0], [0, 1, 0]]), (1, [[1, 0, 0], [0, -1, 0]])):
        got = lighting.world_normal(vv["normal"][[k, k]], vv["tangent"][[k, k]], vv["bitangent"][[k, k]], s)
        assert np.allclose(got, want, atol=1e-15)
    # normalScale scales x and y before the sample is normalised: (0.5, 0, 1) at scale 2 -> (1, 0, 1) / sqrt 2
    got = lighting.world_normal(vv["normal"][:1], vv["tangent"][:1], vv["bitangent"][:1], np.array([[0.75, 0.5, 1.0]]), 2.0)
    assert np.allclose(got, [[math.sqrt(0.5), 0, math.sqrt(0.5)]], atol=1e-15)
    # a non-uniform scale: the normal goes through normalMatrix (inverse transpose), the tangent through model
    model = scenes.trs((2.0, 1.0, 1.0), (0, 0, 0, 1), (0, 0, 0))
    verts[:, 3:6] = [1, 1, 0]; verts[:, 8:11] = [1, -1, 0]
    vv = lighting.vertex_varyings(dataclasses.replace(draw, vertices=verts, object=scenes.object_ubo(model)), np.array([0]))
    assert np.allclose(vv["normal"][0], np.array([0.5, 1.0, 0.0]) / math.sqrt(1.25), atol=1e-7)
    assert np.allclose(vv["tangent"][0], np.array([2.0, -1.0, 0.0]) / math.sqrt(5.0), atol=1e-7) and abs(np.dot(vv["normal"][0], vv["tangent"][0])) < 1e-12


def test_bilinear_texel_centres_and_the_repeat_seam(lighting, scenes):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    yy, xx = np.mgrid[0:5, 0:7]
    u, v = ((xx + 0.5) / 7.0).reshape(-1), ((yy + 0.5) / 5.0).reshape(-1)
    got = lighting.sample_bilinear(img, False, u, v)
    assert np.allclose(got, img.reshape(-1, 4) / 255.0, atol=1e-14)                    # a texel centre is the texel
    for shift in (-2.0, 1.0, 3.0):                                                      # REPEAT: whole periods change nothing
        assert np.allclose(lighting.sample_bilinear(img, False, u + shift, v - shift), got, atol=1e-13)
    seam = lighting.sample_bilinear(img, False, np.array([0.0, 1.0, -1.0]), np.array([0.5 / 5.0] * 3))
    want = (img[0, 6].astype(np.float64) + img[0, 0]) / 510.0                           # u = 0: half the last column, half the first
    assert np.allclose(seam, want, atol=1e-14)
    # sRGB: the texel is decoded, then filtered; alpha stays linear
    got = lighting.sample_bilinear(img, True, np.array([0.0]), np.array([0.1]))
    eotf = lambda b: np.where(b / 255.0 <= 0.04045, b / 255.0 / 12.92, ((b / 255.0 + 0.055) / 1.055) ** 2.4)
    assert np.allclose(got[0, :3], (eotf(img[0, 6, :3].astype(np.float64)) + eotf(img[0, 0, :3].astype(np.float64))) / 2.0, atol=1e-14)
    assert got[0, 3] == pytest.approx((int(img[0, 6, 3]) + int(img[0, 0, 3])) / 510.0, abs=1e-14)
    assert lighting.srgb_decode(np.array([0, 10, 11, 255])) == pytest.approx([0.0, 10 / 255 / 12.92, ((11 / 255 + 0.055) / 1.055) ** 2.4, 1.0], rel=1e-14)


@pytest.mark.parametrize("texels_per_pixel", [0.25, 1.0, 2.0, 4.0])
def test_lambda_of_the_k8_quad(lighting, scenes, texels_per_pixel):
    """K8's quad fills the viewport with uv = s (0..1): n texels per pixel, lambda = log2(n); trilinear then reads the level that makes a 1-texel
    checker its mean from level 1 on."""
    from test_oracle_kats import _textured_quad_scene
    n = W = H = 64
    yy, xx = np.mgrid[0:n, 0:n]
    tex = np.zeros((n, n, 4), dtype=np.uint8)
    tex[..., 0:3] = (255 * ((xx + yy) & 1))[..., None]; tex[..., 3] = 255
    texture = scenes.Texture(tex, mips=True)
    sc = _textured_quad_scene(scenes, texture, W, H, uv_scale=texels_per_pixel * W / n)
    py, px = [a.reshape(-1) for a in np.mgrid[8:56, 8:56]]
    pix = lighting.pixel_inputs(sc, sc.draws[0], np.zeros(py.size, dtype=np.int64), px, py)
    lam = lighting.texture_lambda(texture, pix["grad"])
    assert np.allclose(lam, math.log2(texels_per_pixel), atol=1e-9)
    out = lighting.sample_trilinear(texture, pix["uv"][:, 0], pix["uv"][:, 1], pix["grad"])[:, 0]
    if texels_per_pixel >= 2.0:
        assert np.allclose(out, 128.0 / 255.0, atol=1e-12)
    else:
        assert out.min() < 0.3 and out.max() > 0.7


def test_barycentrics_are_perspective_correct_and_honour_the_draw(lighting, scenes):
    """A triangle with unequal w: the barycentrics of a projected interior point are the point's own weights, not the screen-space ones; the
    viewport, `first`, `vertex_offset` and 16-bit indices select and place the same triangle."""
    clip = np.array([[[-1.0, -1.0, 0.5, 1.0], [3.0, -1.0, 0.5, 3.0], [0.0, 4.0, 0.5, 5.0]]])
    b = np.array([0.2, 0.3, 0.5])
    p = b @ clip[0]
    vp = (10.0, 20.0, 64.0, 32.0, 0.0, 1.0)
    px, py = vp[0] + (p[0] / p[3] * 0.5 + 0.5) * vp[2], vp[1] + (p[1] / p[3] * 0.5 + 0.5) * vp[3]
    got = lighting.barycentrics(clip, np.array([px]), np.array([py]), vp)
    assert np.allclose(got[0], b, atol=1e-13)
    verts = np.zeros((9, 12), dtype=np.float32)
    verts[:, 0] = np.arange(9)
    d = scenes.DrawSpec(vertices=verts, stride=48, count=6, indices=np.array([9, 9, 9, 0, 1, 2, 3, 1, 0], dtype=np.uint16), first=3, vertex_offset=4)
    assert lighting.fetch_triangles(d).tolist() == [[4, 5, 6], [7, 5, 4]]
    assert lighting.fetch_triangles(dataclasses.replace(d, indices=None, first=2)).tolist() == [[2, 3, 4], [5, 6, 7]]


# ---- the oracle against the model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(lc.CASE_COUNT))
def test_oracle_against_the_model(oracle, mirhi, i):
    """Every case / program / roughness: the oracle's float frame within max(8 E32, 1e-4) of M64 on every covered pixel but the left-out ones."""
    assert len(lc.all_cases()) == lc.CASE_COUNT
    sc = lc.case(i)
    ref = _oracle_frame(oracle, sc)
    e32, bound, err = lc.check(None, sc, ref["prim"], ref["rgba"], "oracle")
    assert e32 < 5e-3                                 # (the float32 model itself stays a usable yardstick)
    m = lc.model(sc, ref["prim"])
    if sc.draws[0].program == mirhi.scenes.PROGRAM_MODEL_PBR:
        assert m.keep.all()                           # Cook-Torrance has no discontinuity: nothing is left out
    bg = ref["prim"] == lc.NO_PRIM
    assert m.py.size == int((~bg).sum())


# ---- what the cases promise, from the float64 model alone ---------------------------------------------------------------------------------------
def _blocks(m, a, flag):
    """Per 8x8 block of the frame: (covered pixels, flagged pixels) of one draw's pixels."""
    cov, fl = np.zeros((lc.H, lc.W), dtype=bool), np.zeros((lc.H, lc.W), dtype=bool)
    cov[m.py[a["sel"]], m.px[a["sel"]]] = True
    fl[m.py[a["sel"]], m.px[a["sel"]]] = flag
    by = lambda x: x.reshape(lc.H // 8, 8, lc.W // 8, 8).sum(axis=(1, 3))
    return by(cov), by(fl)


def test_case_conditions(oracle, mirhi, lighting):
    S = mirhi.scenes
    for sc, short_lights in ((lc.sphere(S.PROGRAM_MODEL_PBR, 0.3), (0, 2, 3)), (lc.sphere(S.PROGRAM_MODEL_FULL, 0.3), (0, 2, 3)),
                             (lc.ground(S.PROGRAM_MODEL_PBR), (0, 1)), (lc.ground(S.PROGRAM_MODEL_FULL), (0, 1))):
        m = lc.model(sc, _oracle_frame(oracle, sc)["prim"])
        a = m.aux["draws"][0]
        assert 3000 <= m.py.size <= 14000
        for k in short_lights:                        # the short point light and each spot: zero on 10 % .. 90 % of the covered pixels
            kind, att = a["attenuation"][k]
            zero = att == 0.0
            assert 0.1 <= zero.mean() <= 0.9, (sc.name, kind, k, zero.mean())
            cov, z = _blocks(m, a, zero)
            full = cov == 64
            assert (full & (z == 64)).any(), (sc.name, k, "no 8x8 block wholly outside: the wave-uniform early-out is not taken")
            assert (full & (z > 0) & (z < 64)).any(), (sc.name, k, "no mixed 8x8 block")
        if sc.name.startswith("sphere"):
            assert not (a["attenuation"][1][1] == 0.0).any()     # the long point light reaches all of the mesh
        for tex in (sc.draws[0].normal_map,):
            for level in (S.mip_chain(tex.rgba8) if tex.mips else [tex.rgba8]):
                n = level[..., :3].astype(np.float64) / 255.0
                assert np.all(np.abs(np.linalg.norm(n - 1.0, axis=-1) - 0.01) > 1e-3)
        if sc.name.startswith("ground"):
            lam = lighting.texture_lambda(sc.draws[0].albedo_map, a["grad"])
            assert lam.max() - max(lam.min(), 0.0) >= 2.0 and lam.min() < 0.0, (lam.min(), lam.max())
            vv = lighting.vertex_varyings(sc.draws[0], np.arange(4))
            assert (vv["clip"][:, 3] < 0).any() and (vv["clip"][:, 3] > 0).any()          # the quad crosses w = 0
    sp = lc.sphere(S.PROGRAM_MODEL_PBR, 0.3).draws[0]
    v = np.asarray(sp.vertices)
    assert v[:, 6].min() < -1.2 and v[:, 6].max() > 1.7 and v[:, 7].min() < -0.45 and v[:, 7].max() > 1.45
    assert set(v[:, 11].tolist()) == {1.0, -1.0}
    for s in lc.SPHERE_LIGHTS["spots"] + lc.GROUND_LIGHTS["spots"]:
        assert abs(np.linalg.norm(s[2]) - 1.0) > 0.2                                    # spot directions are given unnormalised


# ---- planted errors --------------------------------------------------------------------------------------------------------------------------------
def _plant(monkeypatch, lighting, scenes, what):
    L = lighting
    orig = {k: getattr(L, k) for k in ("vertex_varyings", "world_normal", "attenuation", "geometry_schlick_ggx", "barycentrics", "sample_bilinear",
                                       "shade_model_pbr")}
    if what == "model matrix for the normal":
        def f(draw, vidx, dtype=np.float64):
            o = bytes(draw.object)
            return orig["vertex_varyings"](dataclasses.replace(draw, object=o[:64] + o[:64]), vidx, dtype)
        monkeypatch.setattr(L, "vertex_varyings", f)
    elif what == "handedness dropped":
        def f(draw, vidx, dtype=np.float64):
            vv = orig["vertex_varyings"](draw, vidx, dtype)
            vv["bitangent"] = L._cross(vv["normal"], vv["tangent"])
            return vv
        monkeypatch.setattr(L, "vertex_varyings", f)
    elif what == "no Gram-Schmidt":
        monkeypatch.setattr(L, "gram_schmidt", lambda T, N: T)
    elif what == "roughness and metallic channels swapped":
        def f(draw, pix, dtype=np.float64, aux=None, ibl_zero_env=False):
            t = draw.metallic_roughness_map
            sw = dataclasses.replace(t, rgba8=np.ascontiguousarray(t.rgba8[..., [0, 2, 1, 3]]))
            return orig["shade_model_pbr"](dataclasses.replace(draw, metallic_roughness_map=sw), pix, dtype, aux, ibl_zero_env)
        monkeypatch.setattr(L, "shade_model_pbr", f)
    elif what == "spot radius 40":
        monkeypatch.setattr(L, "SPOT_RADIUS", 40.0)
    elif what == "spot direction not normalised":
        monkeypatch.setattr(L, "spot_direction", lambda d, dtype=np.float64: np.asarray(d, dtype=dtype))
    elif what == "normalScale dropped":
        monkeypatch.setattr(L, "world_normal", lambda N, T, B, s, scale=None, dtype=np.float64: orig["world_normal"](N, T, B, s, None if scale is None else 1.0, dtype))
    elif what == "no ao lerp on direct light":
        monkeypatch.setattr(L, "direct_ao_scale", lambda ao, dtype=np.float64: np.ones_like(ao))
    elif what == "falloff not squared":
        def f(distance, radius, dtype=np.float64):
            T = np.dtype(dtype).type
            d = np.asarray(distance, dtype=dtype)
            return (T(1.0) / (d * d + T(1.0))) * np.clip(T(1.0) - d / T(radius), T(0.0), T(1.0))
        monkeypatch.setattr(L, "attenuation", f)
    elif what == "wrong k":
        def f(ndx, roughness, dtype=np.float64):
            T = np.dtype(dtype).type
            k = (roughness * roughness) / T(2.0)                      # the IBL remapping, pbr.hlsli:87
            return ndx / np.maximum(ndx * (T(1.0) - k) + k, T(L.EPSILON))
        monkeypatch.setattr(L, "geometry_schlick_ggx", f)
    elif what == "Fresnel on N.V":
        direct, fresnel = L.pbr_direct, L.fresnel_schlick

        def f(N, V, Lv, radiance, albedo, metallic, roughness, dtype=np.float64):
            L.fresnel_schlick = lambda ct, F0, dtype=np.float64: fresnel(L._max0(L._dot(N, V)), F0, dtype)
            try:
                return direct(N, V, Lv, radiance, albedo, metallic, roughness, dtype)
            finally:
                L.fresnel_schlick = fresnel
        monkeypatch.setattr(L, "pbr_direct", f)
    elif what == "affine interpolation":
        def f(clip, pxc, pyc, viewport, dtype=np.float64):
            b = orig["barycentrics"](clip, pxc, pyc, viewport, dtype) * clip[..., 3]       # screen-space weights: lambda_i w_i
            return b / ((b[:, 0] + b[:, 1]) + b[:, 2])[:, None]
        monkeypatch.setattr(L, "barycentrics", f)
    elif what == "no sRGB decode":
        monkeypatch.setattr(L, "srgb_decode", lambda b, dtype=np.float64: (np.asarray(b, dtype=np.float64) / 255.0).astype(dtype))
    elif what == "no half-texel offset":
        def f(level, srgb, u, v, dtype=np.float64):
            T = np.dtype(dtype).type
            return orig["sample_bilinear"](level, srgb, u + T(0.5) / T(level.shape[1]), v + T(0.5) / T(level.shape[0]), dtype)
        monkeypatch.setattr(L, "sample_bilinear", f)
    elif what == "shininess 1024":
        monkeypatch.setattr(L, "roughness_to_shininess", lambda r, dtype=np.float64: np.dtype(dtype).type(1024.0 + (2.0 - 1024.0) * min(max(float(r), 0.0), 1.0)))
    else:
        raise KeyError(what)


PLANTED = ("model matrix for the normal", "handedness dropped", "no Gram-Schmidt", "roughness and metallic channels swapped", "spot radius 40",
           "spot direction not normalised", "normalScale dropped", "no ao lerp on direct light", "falloff not squared", "Fresnel on N.V", "wrong k",
           "affine interpolation", "no sRGB decode", "no half-texel offset", "shininess 1024")


@pytest.mark.parametrize("what", PLANTED)
def test_a_planted_error_puts_the_oracle_outside_the_bound(oracle, mirhi, lighting, monkeypatch, what):
    """One helper of the model replaced by a subtly wrong one: against that model (and the bound from ITS float32 twin) the oracle's frame must
    fail on at least one case -- the comparison would notice a kernel with the same mistake."""
    S = mirhi.scenes
    cases = [lc.sphere(S.PROGRAM_MODEL_PBR, 0.3), lc.sphere(S.PROGRAM_MODEL_FULL, 0.3, True), lc.ground(S.PROGRAM_MODEL_PBR), lc.ground(S.PROGRAM_MODEL_FULL)]
    frames = [_oracle_frame(oracle, sc) for sc in cases]
    for sc, ref in zip(cases, frames):                 # the unplanted model passes
        m = lc.model(sc, ref["prim"])
        assert lc.measure(ref["rgba"], m)[0] <= m.bound
    _plant(monkeypatch, lighting, S, what)
    worst = 0.0
    for sc, ref in zip(cases, frames):
        m = lc.model(sc, ref["prim"], cache=False)
        err = lc.measure(ref["rgba"], m)[0]
        worst = max(worst, err / m.bound)
        if err > m.bound:
            break
    print(f"LIGHT planted '{what}': err / bound {worst:.1f} on {sc.name}")
    assert worst > 1.0, f"'{what}' goes unnoticed: err / bound = {worst:.3f}"


# ---- the raster variants tests/test_gpu_lighting.py runs the fragment code through --------------------------------------------------------------
def test_routes_of_the_gpu_cases(mirhi):
    """mirhi_debug_raster_choice (no HIP call) for the program sets and knobs of the GPU file: 2 = MODEL_FULL with linear textures and no chain,
    4 = the full-featured set (Cook-Torrance, sRGB, chains), 3 = a TRIANGLE draw beside MODEL / MODEL_FULL; 8 / 32 add the shadow map / the IBL set."""
    import ctypes as C
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_raster_choice
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]

    def choose(programs, zflip=0, tp=0, teams=1, wide=0):
        name, shape = C.create_string_buffer(96), (C.c_uint32 * 4)()
        assert fn((C.c_uint32 * 12)(programs, 1, 0, zflip, 0xFFFFFFFF, tp, teams, wide, 0, 1, 0, 0), name, len(name), shape) == 0
        return name.value.decode()
    for progs in (2, 4):
        assert choose(progs) == f"raster_kernel<{progs}, 0, 0, 1, false>"                               # the plain route
        assert choose(progs, tp=64, wide=8) == f"raster_kernel_wide<{progs}, 0, 8>" and choose(progs, tp=64, wide=16) == f"raster_kernel_wide<{progs}, 0, 16>"
        assert choose(progs, tp=64, teams=2) == f"raster_kernel<{progs}, 0, 1, 2, false>"               # two teams
        assert choose(progs, zflip=0xFFFFFFFF) == f"raster_kernel<{progs}, 1, 0, 1, false>"             # the generic key (GREATER)
    assert choose(3) == "raster_kernel<3, 0, 0, 1, false>" and choose(7) == "raster_kernel<4, 0, 0, 1, false>"      # mixed sets: 3, and "all"
    assert choose(12).startswith("raster_kernel_shadow<") and choose(36).startswith("raster_kernel_ibl<")
