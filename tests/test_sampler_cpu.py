"""Sampler state of textures (include/mirhi.h mirhi_image_set_sampler), the part that needs no GPU: the equivalences the GPU tests rest on,
checked with the float64 one-level sampler of tests/sampler_cases.py over dense uv sweeps; the new names in the header, the ctypes table, the
C++ mirror and the Rust crates; the default desc; the glTF loaders' samplers; and scenes.Texture's defaults leaving the oracle's frame alone."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import sampler_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENUMS = {"mirhi_address_mode": ["MIRHI_ADDRESS_REPEAT", "MIRHI_ADDRESS_MIRRORED_REPEAT", "MIRHI_ADDRESS_CLAMP_TO_EDGE"],
         "mirhi_sampler_filter": ["MIRHI_SAMPLER_FILTER_LINEAR", "MIRHI_SAMPLER_FILTER_NEAREST"],
         "mirhi_mip_mode": ["MIRHI_MIP_LINEAR", "MIRHI_MIP_NEAREST", "MIRHI_MIP_BASE"]}
FIELDS = ["address_u", "address_v", "mag_filter", "min_filter", "mip_mode"]
TEXTURES = [sc.noise_texture(8, 8, 1), sc.noise_texture(6, 5, 2), sc.noise_texture(4, 10, 3)]


def _sweep(lo, hi, n=1531):
    """uv pairs along two incommensurable lines through [lo, hi]^2, plus the half-texel-exact points of a coarse grid"""
    t = np.linspace(lo, hi, n)
    return np.concatenate([t, t[::-1], np.round(t * 16) / 16]), np.concatenate([t * 0.731 + 0.113, t, np.round(t[::-1] * 16) / 16])


def test_address_modes_follow_the_stated_formulas():
    i = np.arange(-40, 41)
    for n in (1, 2, 5, 8):
        assert np.array_equal(sc.address(i, n, sc.REPEAT), i % n)
        assert np.array_equal(sc.address(i, n, sc.CLAMP_TO_EDGE), np.clip(i, 0, n - 1))
        period = np.concatenate([np.arange(n), np.arange(n)[::-1]])                   # 0 .. n-1, n-1 .. 0
        assert np.array_equal(sc.address(i, n, sc.MIRRORED_REPEAT), period[i % (2 * n)])
    assert list(sc.address([-2, -1, 0, 3, 4, 5, 7, 8], 4, sc.MIRRORED_REPEAT)) == [1, 0, 0, 3, 3, 2, 0, 0]


@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("tex", TEXTURES, ids=["8x8", "6x5", "4x10"])
def test_mirrored_repeat_is_repeat_on_the_mirror_tile(tex, nearest):
    """equivalence 1, over several periods and negative coordinates"""
    u, v = _sweep(-2.3, 3.1)
    got = sc.sample(tex, u, v, sc.MIRRORED_REPEAT, sc.MIRRORED_REPEAT, nearest)
    tile = sc.extended(tex, sc.MIRRORED_REPEAT, sc.MIRRORED_REPEAT)
    h, w = tex.shape[:2]
    assert tile.shape[:2] == (2 * h, 2 * w) and np.array_equal(tile[h:, w:], tex[::-1, ::-1]) and np.array_equal(tile[:h, w:], tex[:, ::-1])
    assert np.array_equal(got, sc.sample(tile, u / 2, v / 2, nearest=nearest))
    assert not np.array_equal(got, sc.sample(tex, u, v, nearest=nearest))               # (and REPEAT is something else)


@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("modes", [(sc.CLAMP_TO_EDGE, sc.CLAMP_TO_EDGE), (sc.CLAMP_TO_EDGE, sc.MIRRORED_REPEAT), (sc.REPEAT, sc.CLAMP_TO_EDGE)])
def test_clamp_to_edge_is_repeat_on_the_edge_replicated_texture(modes, nearest):
    """equivalence 2 and its mixed case (clamp in u, mirror in v): uv inside (-1/2 + 1/w, 3/2 - 1/w) on the clamped axes"""
    for tex in (TEXTURES[0], TEXTURES[2]):
        h, w = tex.shape[:2]
        lo, hi = -0.5 + 1.0 / min(w, h), 1.5 - 1.0 / min(w, h)
        u, v = _sweep(lo, hi)
        v = np.clip(v, lo, hi)
        got = sc.sample(tex, u, v, modes[0], modes[1], nearest)
        assert np.array_equal(got, sc.sample(sc.extended(tex, *modes), u / 2, v / 2, nearest=nearest)), (w, h)
        inside = (u > 0.5 / w) & (u < 1 - 0.5 / w) & (v > 0.5 / h) & (v < 1 - 0.5 / h)
        assert np.array_equal(got[inside], sc.sample(tex, u, v, nearest=nearest)[inside])        # inside the texture every mode agrees
    edge = sc.extend_axis(TEXTURES[0], 1, sc.CLAMP_TO_EDGE)
    assert np.array_equal(edge[:, 8:12], np.repeat(TEXTURES[0][:, 7:8], 4, axis=1)) and np.array_equal(edge[:, 12:], np.repeat(TEXTURES[0][:, 0:1], 4, axis=1))


def test_nearest_is_linear_on_a_rebuilt_texture():
    """equivalence 3: magnified x4 at texel fractions 1/8, 3/8, 5/8, 7/8 == LINEAR on the 4 x 4 replicated texture; at texel fraction 3/4 (a x2
    minification's pixel centres, offset by a quarter texel) == LINEAR with uv shifted by -1/4 texel -- and there NEAREST is not LINEAR."""
    tex = sc.noise_texture(16, 16, 4)
    px = (np.arange(64) + 0.5) / 64.0
    u, v = np.meshgrid(px, px)
    assert set(np.unique((u * 16) % 1.0)) == {0.125, 0.375, 0.625, 0.875}
    assert np.array_equal(sc.sample(tex, u, v, nearest=True), sc.sample(sc.replicated(tex, 4), u, v))
    tex = sc.noise_texture(32, 32, 5)
    u, v = np.meshgrid((2 * np.arange(64) + 0.75) / 32.0, (2 * np.arange(64) + 0.75) / 32.0)       # texels 2 px + 3/4 over four periods
    near = sc.sample(tex, u, v, nearest=True)
    assert np.array_equal(near, sc.sample(tex, u - 0.25 / 32, v - 0.25 / 32))
    assert np.abs(near - sc.sample(tex, u, v)).max() > 0.1
    for mode in (sc.MIRRORED_REPEAT, sc.CLAMP_TO_EDGE):                 # NEAREST goes through the address modes like LINEAR
        assert np.array_equal(sc.sample(tex, u - 1.0, v, mode, mode, True), sc.sample(tex, u - 1.0 - 0.25 / 32, v - 0.25 / 32, mode, mode))


def test_banded_texture_commutes_with_the_box_filter(mirhi):
    """What the chained CLAMP_TO_EDGE case needs: levels 0 .. log2(n/4) of the edge-replicated texture are the edge-replicated levels."""
    tex = sc.banded_texture(32, 6)
    chain, big = mirhi.scenes.mip_chain(tex), mirhi.scenes.mip_chain(sc.extended(tex, sc.CLAMP_TO_EDGE, sc.CLAMP_TO_EDGE))
    for level in range(4):                                              # texels up to 8 = n / 4 wide
        assert np.array_equal(big[level], sc.extended(chain[level], sc.CLAMP_TO_EDGE, sc.CLAMP_TO_EDGE)), level
    mirror = sc.noise_texture(8, 8, 7)
    chain, big = mirhi.scenes.mip_chain(mirror), mirhi.scenes.mip_chain(sc.extended(mirror, sc.MIRRORED_REPEAT, sc.MIRRORED_REPEAT))
    for level in range(3):                                              # below the 1 x 1 top level
        assert np.array_equal(big[level], sc.extended(chain[level], sc.MIRRORED_REPEAT, sc.MIRRORED_REPEAT)), level


def test_new_names_agree_across_header_ctypes_cpp_and_rust(mirhi):
    header = open(os.path.join(ROOT, "include", "mirhi.h")).read()
    rust_sys = open(os.path.join(ROOT, "bindings", "rust", "mirhi-sys", "src", "lib.rs")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "renderer-rhi-hip", "src", "image.rs")).read()
    hpp = open(os.path.join(ROOT, "renderer-rs_amd", "host", "mirhi.hpp")).read()
    for enum, names in ENUMS.items():
        m = re.search(r"typedef enum \{([^}]*)\} " + enum + ";", header)
        assert m, enum
        assert [(k.strip(), int(v)) for k, v in (item.split("=") for item in m.group(1).split(","))] == [(n, i) for i, n in enumerate(names)]
        for i, n in enumerate(names):
            assert f"pub const {n}: {enum} = {i};" in rust_sys and n in hpp, n
    assert re.search(r"typedef struct \{ int32_t " + ", ".join(FIELDS) + r"; \} mirhi_sampler_desc;", header)
    assert [f for f, _ in mirhi.SamplerDesc._fields_] == FIELDS and C.sizeof(mirhi.SamplerDesc) == 20
    body = re.search(r"pub struct mirhi_sampler_desc \{\n(.*?)\n\}", rust_sys, re.S).group(1)
    assert re.findall(r"pub (\w+): i32", body) == FIELDS
    for fn in ("mirhi_sampler_desc_default", "mirhi_image_set_sampler", "mirhi_image_sampler"):
        assert fn in mirhi._SIGNATURES and f"pub fn {fn}(" in rust_sys and hasattr(mirhi.lib(), fn), fn
        assert f"mirhi_sys::{fn}" in rust, fn
    # the C++ mirror calls the two image functions; its default desc is inline (host/gltf.hpp holds SamplerDesc members and has to link without
    # libmirhi, tools/fuzz_gltf.cpp), and host/test_host.cpp compares it with what mirhi_sampler_desc_default fills in
    assert "check(mirhi_image_set_sampler(h_, &s))" in hpp and "check(mirhi_image_sampler(h_, &s))" in hpp
    assert "SamplerDesc() : mirhi_sampler_desc{0, 0, 0, 0, 0} {}" in hpp and not re.search(r"[^`']mirhi_sampler_desc_default\(", hpp)
    host_test = open(os.path.join(ROOT, "renderer-rs_amd", "host", "test_host.cpp")).read()
    assert "mirhi_sampler_desc_default(&sd)" in host_test and "SamplerDesc() == sd" in host_test
    assert (mirhi.AddressMode.REPEAT, mirhi.AddressMode.MIRRORED_REPEAT, mirhi.AddressMode.CLAMP_TO_EDGE) == (0, 1, 2)
    assert (mirhi.SamplerFilter.LINEAR, mirhi.SamplerFilter.NEAREST) == (0, 1) and (mirhi.MipMode.LINEAR, mirhi.MipMode.NEAREST, mirhi.MipMode.BASE) == (0, 1, 2)
    assert (sc.REPEAT, sc.MIRRORED_REPEAT, sc.CLAMP_TO_EDGE, sc.LINEAR, sc.NEAREST, sc.MIP_LINEAR, sc.MIP_NEAREST, sc.MIP_BASE) == (0, 1, 2, 0, 1, 0, 1, 2)
    assert "pub fn set_sampler(" in rust and "set_sampler(const SamplerDesc&" in hpp


def test_default_desc_is_all_zero_and_null_handles_are_errors(mirhi):
    desc = mirhi.SamplerDesc(7, 7, 7, 7, 7)
    mirhi.lib().mirhi_sampler_desc_default(C.byref(desc))
    assert desc.as_tuple() == (0, 0, 0, 0, 0) and bytes(desc) == bytes(20)
    mirhi.lib().mirhi_sampler_desc_default(None)                       # (nothing to fill in: no crash)
    assert mirhi.lib().mirhi_image_set_sampler(None, C.byref(desc)) == mirhi.ERR_INVALID_HANDLE
    assert mirhi.lib().mirhi_image_sampler(None, C.byref(desc)) == mirhi.ERR_INVALID_HANDLE
    assert b"null" in mirhi.lib().mirhi_last_error_message()


def _gltf_doc(samplers, textures):
    import base64
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    uri = "data:application/octet-stream;base64," + base64.b64encode(pos.tobytes()).decode()
    doc = {"asset": {"version": "2.0"}, "buffers": [{"byteLength": 36, "uri": uri}], "bufferViews": [{"buffer": 0, "byteLength": 36}],
           "accessors": [{"bufferView": 0, "componentType": 5126, "count": 3, "type": "VEC3"}],
           "meshes": [{"primitives": [{"attributes": {"POSITION": 0}, "material": 0}]}],
           "textures": textures,
           "materials": [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicRoughnessTexture": {"index": 1}},
                          "normalTexture": {"index": 2}, "occlusionTexture": {"index": 3}, "emissiveTexture": {"index": 4}}]}
    if samplers is not None:
        doc["samplers"] = samplers
    return doc


def test_gltf_loader_returns_the_sampler_of_each_slot(mirhi, tmp_path):
    from renderer_rs_amd import gltf
    samplers = [{"wrapS": 33071, "wrapT": 33648, "magFilter": 9728, "minFilter": 9729},        # clamp / mirror, NEAREST, LINEAR on level 0
                {"minFilter": 9984},                                                           # NEAREST_MIPMAP_NEAREST; the rest absent
                {"wrapS": 10497, "wrapT": 33071, "magFilter": 9729, "minFilter": 9985},        # LINEAR_MIPMAP_NEAREST
                {"minFilter": 9986},                                                           # NEAREST_MIPMAP_LINEAR
                {"minFilter": 9728}]                                                           # NEAREST on level 0
    textures = [{"sampler": 0}, {"sampler": 1}, {"sampler": 2}, {"sampler": 3}, {"sampler": 4}]
    p = tmp_path / "samplers.gltf"
    p.write_text(json.dumps(_gltf_doc(samplers, textures)))
    m = gltf.load(str(p), images=True).materials[0]
    S = gltf.Sampler
    assert m.base_color_sampler == S(sc.CLAMP_TO_EDGE, sc.MIRRORED_REPEAT, sc.NEAREST, sc.LINEAR, sc.MIP_BASE)
    assert m.metallic_roughness_sampler == S(sc.REPEAT, sc.REPEAT, sc.LINEAR, sc.NEAREST, sc.MIP_NEAREST)
    assert m.normal_sampler == S(sc.REPEAT, sc.CLAMP_TO_EDGE, sc.LINEAR, sc.LINEAR, sc.MIP_NEAREST)
    assert m.occlusion_sampler == S(sc.REPEAT, sc.REPEAT, sc.LINEAR, sc.NEAREST, sc.MIP_LINEAR)
    assert m.emissive_sampler == S(sc.REPEAT, sc.REPEAT, sc.LINEAR, sc.NEAREST, sc.MIP_BASE)
    # a Sampler's fields are scenes.Texture's (and mirhi_sampler_desc's)
    import dataclasses
    names = [f.name for f in dataclasses.fields(S)]
    assert names == FIELDS and set(names) <= {f.name for f in dataclasses.fields(mirhi.scenes.Texture)}
    # the reference's loader (images discarded) says nothing about samplers
    assert gltf.load(str(p)).materials[0].base_color_sampler == S()
    # absent: no samplers array, textures without a sampler, an empty sampler object, LINEAR_MIPMAP_LINEAR -- today's sampler
    for samplers2, textures2 in ((None, [{}] * 5), ([{}], [{"sampler": 0}] * 5), ([{"magFilter": 9729, "minFilter": 9987, "wrapS": 10497, "wrapT": 10497}], [{"sampler": 0}] * 5)):
        p.write_text(json.dumps(_gltf_doc(samplers2, textures2)))
        m = gltf.load(str(p), images=True).materials[0]
        assert [m.base_color_sampler, m.metallic_roughness_sampler, m.normal_sampler, m.occlusion_sampler, m.emissive_sampler] == [S()] * 5
    # a code glTF does not define, and a sampler index outside the array
    for bad in ({"wrapS": 33069}, {"wrapT": 0}, {"magFilter": 9987}, {"minFilter": 9988}, {"minFilter": "LINEAR"}):
        p.write_text(json.dumps(_gltf_doc([bad], [{"sampler": 0}] * 5)))
        with pytest.raises(gltf.ResourceError):
            gltf.load(str(p), images=True)
    p.write_text(json.dumps(_gltf_doc([{}], [{"sampler": 3}] * 5)))
    with pytest.raises(gltf.ResourceError):
        gltf.load(str(p), images=True)
    dancer = gltf.load(os.path.join(ROOT, "tests", "golden", "dancer", "scene.gltf"), images=True).materials[0]
    assert dancer.normal_sampler == S() and dancer.base_color_sampler == S()      # 9729 / 9987 / 10497: the default, as rendered so far


def test_texture_defaults_leave_the_oracle_binding_alone(mirhi, oracle):
    """scenes.Texture's new fields default to today's sampler and are not the oracle's business: the `textured` small case, its textures rebuilt
    with every new field named, still renders to the golden vector committed before the fields existed (tests/golden/small_cases.json, the
    digests of tests/test_goldens.py) -- and a texture that names another sampler renders to it too, because the oracle has one sampler."""
    import hashlib
    scenes = mirhi.scenes
    t = scenes.Texture(np.zeros((2, 2, 4), dtype=np.uint8))
    assert (t.address_u, t.address_v, t.mag_filter, t.min_filter, t.mip_mode) == (0, 0, 0, 0, 0) and (t.mips, t.srgb, t.max_anisotropy) == (False, False, 1)
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "small_cases.json")))["textured"]

    def matches_golden(r):
        covered = r["prim"] != 0xFFFFFFFF
        depth_bits = np.where(covered, r["depth"].view(np.uint32), 0).astype(np.uint32)
        return ((int(covered.sum()), hashlib.sha256(r["prim"].tobytes()).hexdigest(), hashlib.sha256(depth_bits.tobytes()).hexdigest())
                == (g["covered"], g["prim_sha256"], g["depth_sha256"])
                and [int(x) for x in r["bgra8"].reshape(-1, 4).astype(np.uint64).sum(axis=0)] == g["bgra8_sum"])
    for state in ((0, 0, 0, 0, 0), (2, 1, 1, 1, 2)):
        scene = scenes.SMALL_CASES["textured"]()
        for d in scene.draws:
            for name in ("albedo_map", "normal_map"):
                old = getattr(d, name)
                setattr(d, name, scenes.Texture(old.rgba8, old.mips, old.srgb, old.max_anisotropy, *state))
        assert matches_golden(oracle.render(scene, want_bgra8=True)), state


def test_a_draw_with_sampler_state_takes_the_full_featured_class_and_the_ordered_resolve_of_a_discard_scope(mirhi):
    """mirhi_debug_scope_plan (no HIP call): a MODEL_FULL draw whose texture has sampler state is of the full-featured program class, like one with
    a mip chain; a MODEL_PBR draw whose base colour texture has state keeps a discard scope out of the masked raster variants (their alpha test
    knows the default sampler only), so that scope takes the ordered resolve.  Without the state both scopes are planned as before (tests/golden/scope_plans.json pins that)."""
    import struct
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_scope_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32]

    def plan(discard, program, third):
        words = [1, 1, 1, 1, discard, 0, struct.unpack("<I", struct.pack("<f", 1.0))[0], 0, 20, 40, 0, 0, 1, 1, 1, program, 0, third]
        inp, out, name = (C.c_uint32 * 27)(*(words + [0] * (27 - len(words)))), (C.c_uint32 * 32)(), C.create_string_buffer(96)
        assert fn(inp, out, name, len(name)) == 0
        return dict(ordered=out[8], masked_plain=out[9], programs=out[14], kernel=name.value.decode())
    plain, mips, state = plan(0, 2, 0), plan(0, 2, 1), plan(0, 2, 2)
    assert plain["programs"] != mips["programs"] and state["programs"] == mips["programs"] and state["kernel"] == mips["kernel"]
    assert (state["ordered"], state["masked_plain"]) == (0, 0)
    assert plan(0, 2, 4)["programs"] == mips["programs"]                  # state on texture 1 alone: the same class
    masked, masked_state = plan(1, 3, 0), plan(1, 3, 2)
    assert (masked["ordered"], masked["masked_plain"]) == (0, 1) and (masked_state["ordered"], masked_state["masked_plain"]) == (1, 0)
    assert masked_state["programs"] == masked["programs"] and "ordered" in masked_state["kernel"] and "ordered" not in masked["kernel"]
    # only the texture the alpha test reads decides: state on the normal map, or on a MODEL_FULL draw's albedo, leaves the discard scope masked
    assert plan(1, 3, 4) == masked
    full_masked = plan(1, 2, 2)
    assert (full_masked["ordered"], full_masked["masked_plain"]) == (0, 1)
