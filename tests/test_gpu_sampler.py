"""GPU tests of a texture's sampler state (include/mirhi.h mirhi_image_set_sampler): address modes, mag / min filters, mip modes.

The yardstick is the unchanged oracle under its REPEAT / LINEAR sampler, fed a transformed scene (tests/sampler_cases.py states the equivalences,
tests/test_sampler_cpu.py proves them in float64): prim ids equal, |dRGB| < 1e-4 on the float target, <= 1 LSB on sRGB8 -- `_check` of
tests/test_gpu_parity.py.  64 x 64 targets, 6 x 5 to 32 x 32 textures, the MODEL_FULL program wherever the route does not ask for another.
"""
import copy

import numpy as np
import pytest

import sampler_cases as sc
from test_gpu_parity import _check

pytestmark = pytest.mark.gpu

W = H = 64
WIDE = ((-2.3, -2.3), (3.1, 3.1))                 # several periods and negative coordinates
INSIDE_8 = ((-0.3125, -0.25), (1.3125, 1.25))     # inside (-1/2 + 1/8, 3/2 - 1/8)


def _formats(mirhi):
    return (mirhi.Format.R32G32B32A32_SFLOAT, mirhi.Format.B8G8R8A8_SRGB)


def _render(mirhi, device, scene, fmt=None, want_depth=False):
    res = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT if fmt is None else fmt, want_prim=True, want_depth=want_depth)
    res.render()
    out = {k: v.copy() for k, v in res.read().items()}
    res.destroy()
    return out


def _check_pair(mirhi, oracle, device, scene, ref_scene, name):
    """the product's frame of `scene` against the oracle's frame of `ref_scene`, on both colour formats"""
    ref = oracle.render(ref_scene, want_bgra8=True)
    assert (ref["prim"] != 0xFFFFFFFF).any(), name
    for fmt in _formats(mirhi):
        _check(_render(mirhi, device, scene, fmt), ref, f"{name}-{fmt}")
    return ref


# ---- 1. MIRRORED_REPEAT ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,mips,uv", [((8, 8), False, WIDE), ((6, 5), False, WIDE), ((8, 8), True, WIDE),
                                           ((16, 16), True, ((-2.3, -4.6), (3.1, 6.2)))],
                         ids=["8x8", "6x5-npot", "8x8-chain-magnified", "16x16-chain-minified"])
def test_mirrored_repeat_equals_repeat_on_the_mirror_tile(mirhi, oracle, device, scenes, shape, mips, uv):
    """Equivalence 1.  The 6 x 5 texture takes the division path of wrap_coord; the 16 x 16 one is minified (1.35 and 2.7 texels per pixel,
    lambda = 1.43, under its top level 4), so two levels of its generated chain are read, each mirrored with its own extent."""
    tex = sc.noise_texture(shape[0], shape[1], 11)
    scene, ref_scene = sc.pair(scenes, tex, W, H, uv[0], uv[1], sc.MIRRORED_REPEAT, sc.MIRRORED_REPEAT, mips=mips)
    _check_pair(mirhi, oracle, device, scene, ref_scene, f"mirror-{shape}")


# ---- 2. CLAMP_TO_EDGE ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modes", [(sc.CLAMP_TO_EDGE, sc.CLAMP_TO_EDGE), (sc.CLAMP_TO_EDGE, sc.MIRRORED_REPEAT), (sc.REPEAT, sc.CLAMP_TO_EDGE)],
                         ids=["clamp", "clamp-u-mirror-v", "repeat-u-clamp-v"])
def test_clamp_to_edge_equals_repeat_on_the_edge_replicated_texture(mirhi, oracle, device, scenes, modes):
    """Equivalence 2 on a generic 8 x 8 texture without a chain, and the mixed cases: the mode applies per axis."""
    tex = sc.noise_texture(8, 8, 12)
    scene, ref_scene = sc.pair(scenes, tex, W, H, INSIDE_8[0], INSIDE_8[1], modes[0], modes[1])
    _check_pair(mirhi, oracle, device, scene, ref_scene, f"clamp-{modes}")


def test_clamp_to_edge_with_a_mip_chain(mirhi, oracle, device, scenes):
    """A 32 x 32 texture whose outer quarter bands are constant, so that box-filtering and edge replication commute up to level 3: the quad
    covers 24 x 24 pixels with uv in (-0.45, 1.45), 2.53 texels per pixel, lambda = 1.34 < log2(32 / 4) - 1 = 2 -- levels 1 and 2 are read,
    each clamped to its own edge."""
    tex = sc.banded_texture(32, 13)
    scene, ref_scene = sc.pair(scenes, tex, W, H, (-0.45, -0.45), (1.45, 1.45), sc.CLAMP_TO_EDGE, sc.CLAMP_TO_EDGE, mips=True, rect=(-0.375, -0.375, 0.375, 0.375))
    ref = _check_pair(mirhi, oracle, device, scene, ref_scene, "clamp-chain")
    assert int((ref["prim"] != 0xFFFFFFFF).sum()) == 24 * 24


# ---- 3. NEAREST ------------------------------------------------------------------------------------------------------------------------
def test_nearest_magnified(mirhi, oracle, device, scenes):
    """A 16 x 16 texture over 64 x 64 pixels: pixel centres at texel fractions 1/8, 3/8, 5/8, 7/8.  NEAREST is the oracle's LINEAR on the
    texture with every texel replicated 4 x 4, at the same uv (its pixel centres are that texture's texel centres: weights 1 and 0)."""
    tex = sc.noise_texture(16, 16, 14)
    scene = sc.quad_scene(scenes, sc.texture(scenes, tex, mag_filter=sc.NEAREST, min_filter=sc.NEAREST), W, H, (0.0, 0.0), (1.0, 1.0))
    ref_scene = sc.quad_scene(scenes, sc.texture(scenes, sc.replicated(tex, 4)), W, H, (0.0, 0.0), (1.0, 1.0))
    _check_pair(mirhi, oracle, device, scene, ref_scene, "nearest-mag")


@pytest.mark.parametrize("mag", [sc.LINEAR, sc.NEAREST], ids=["mag-linear", "mag-nearest"])
def test_nearest_minified(mirhi, oracle, device, scenes, mag):
    """A 32 x 32 texture without a chain at 2 texels per pixel (lambda = 1: the min filter), offset so that pixel centres fall at texel fraction
    3/4: NEAREST is the oracle's LINEAR with uv shifted by -1/4 texel.  With mag LINEAR the two filters differ, so the draw has to evaluate the
    uv derivatives to know lambda.  LINEAR at the same uv is visibly something else (so the case cannot pass vacuously)."""
    tex = sc.noise_texture(32, 32, 15)
    o = 0.25 / 32
    uv0, uv1 = (-o, -o), (4.0 - o, 4.0 - o)                          # texel coordinate of pixel p: 2 p + 1 - 1/4
    scene = sc.quad_scene(scenes, sc.texture(scenes, tex, mag_filter=mag, min_filter=sc.NEAREST), W, H, uv0, uv1)
    ref_scene = sc.quad_scene(scenes, sc.texture(scenes, tex), W, H, (uv0[0] - o, uv0[1] - o), (uv1[0] - o, uv1[1] - o))
    _check_pair(mirhi, oracle, device, scene, ref_scene, "nearest-min")
    near = _render(mirhi, device, scene)["color"]
    linear = _render(mirhi, device, sc.quad_scene(scenes, sc.texture(scenes, tex), W, H, uv0, uv1))["color"]
    assert np.abs(near[..., :3] - linear[..., :3]).max() > 0.05


def test_mag_nearest_min_linear_in_one_frame(mirhi, oracle, device, scenes):
    """One quad whose first triangle magnifies a 16 x 16 texture 4 times (lambda = -2: mag NEAREST, the oracle's LINEAR on the 4 x 4 replicated
    texture) and whose second minifies it 2 times (lambda = 1: min LINEAR, the oracle's LINEAR on the texture itself), both under one sampler.
    The oracle takes the two triangles as two draws with a texture each; so does the product, with the one texture."""
    tex = sc.noise_texture(16, 16, 16)
    state = sc.texture(scenes, tex, mag_filter=sc.NEAREST, min_filter=sc.LINEAR)
    halves = dict(split=((0.0, 0.0), (8.0, 8.0)))
    scene = scenes.Scene("mag-min", W, H, [sc.quad_draw(scenes, state, (0.0, 0.0), (1.0, 1.0), first=0, count=3, **halves),
                                           sc.quad_draw(scenes, state, (0.0, 0.0), (1.0, 1.0), first=3, count=3, **halves)])
    ref_scene = scenes.Scene("mag-min-ref", W, H, [sc.quad_draw(scenes, sc.texture(scenes, sc.replicated(tex, 4)), (0.0, 0.0), (1.0, 1.0), first=0, count=3, **halves),
                                                   sc.quad_draw(scenes, sc.texture(scenes, tex), (0.0, 0.0), (1.0, 1.0), first=3, count=3, **halves)])
    ref = _check_pair(mirhi, oracle, device, scene, ref_scene, "mag-nearest-min-linear")
    assert set(np.unique(ref["prim"])) == {0, 1}
    # and it is neither all-NEAREST nor all-LINEAR
    for other in (dict(mag_filter=sc.NEAREST, min_filter=sc.NEAREST), dict()):
        t = sc.texture(scenes, tex, **other)
        alt = scenes.Scene("alt", W, H, [sc.quad_draw(scenes, t, (0.0, 0.0), (1.0, 1.0), first=0, count=3, **halves),
                                         sc.quad_draw(scenes, t, (0.0, 0.0), (1.0, 1.0), first=3, count=3, **halves)])
        assert np.abs(_render(mirhi, device, alt)["color"] - _render(mirhi, device, scene)["color"]).max() > 0.05


# ---- 4. mip modes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam,mode,level", [(1.25, sc.MIP_NEAREST, 1), (1.75, sc.MIP_NEAREST, 2), (1.25, sc.MIP_BASE, 0), (1.75, sc.MIP_BASE, 0)])
def test_mip_nearest_and_mip_base(mirhi, oracle, device, scenes, lam, mode, level):
    """A uniform lambda over the quad (2^lambda texels of a 32 x 32 texture per pixel).  MIP_NEAREST reads the single level ceil(lambda + 1/2) - 1,
    which is the oracle on that level of scenes.mip_chain as a texture without a chain; MIP_BASE reads level 0 whatever the chain."""
    tex = sc.noise_texture(32, 32, 17)
    s = float(2.0 ** lam) * W / 32.0
    scene = sc.quad_scene(scenes, sc.texture(scenes, tex, mips=True, mip_mode=mode), W, H, (0.0, 0.0), (s, s))
    ref_scene = sc.quad_scene(scenes, sc.texture(scenes, scenes.mip_chain(tex)[level]), W, H, (0.0, 0.0), (s, s))
    _check_pair(mirhi, oracle, device, scene, ref_scene, f"mip-mode{mode}-lambda{lam}")
    trilinear = _render(mirhi, device, sc.quad_scene(scenes, sc.texture(scenes, tex, mips=True), W, H, (0.0, 0.0), (s, s)))["color"]
    assert np.abs(trilinear - _render(mirhi, device, scene)["color"]).max() > 0.01


# ---- 5. anisotropy ---------------------------------------------------------------------------------------------------------------------
def test_anisotropic_taps_go_through_the_address_mode(mirhi, oracle, device, scenes):
    """max_anisotropy 8 on a mirrored 16 x 16 texture with a chain: 5.4 texels per pixel along x, 1.35 along y -- N = 4 taps at lambda = 0.43.
    Equivalence 1 holds with the same anisotropy on the tile."""
    tex = sc.noise_texture(16, 16, 18)
    scene, ref_scene = sc.pair(scenes, tex, W, H, (-9.2, -2.3), (12.4, 3.1), sc.MIRRORED_REPEAT, sc.MIRRORED_REPEAT, mips=True, max_anisotropy=8)
    _check_pair(mirhi, oracle, device, scene, ref_scene, "mirror-aniso8")
    iso, _ = sc.pair(scenes, tex, W, H, (-9.2, -2.3), (12.4, 3.1), sc.MIRRORED_REPEAT, sc.MIRRORED_REPEAT, mips=True)
    assert np.abs(_render(mirhi, device, iso)["color"] - _render(mirhi, device, scene)["color"]).max() > 0.01       # (the filter is on)


@pytest.mark.parametrize("state", [dict(min_filter=sc.NEAREST), dict(mip_mode=sc.MIP_NEAREST), dict(mip_mode=sc.MIP_BASE)], ids=["min-nearest", "mip-nearest", "mip-base"])
def test_anisotropy_needs_linear_minification_and_mip_linear(mirhi, device, scenes, state):
    """Otherwise the texture is sampled as if max_anisotropy were 1: the same frame bit for bit."""
    tex = sc.noise_texture(16, 16, 19)
    frames = [_render(mirhi, device, sc.quad_scene(scenes, sc.texture(scenes, tex, mips=True, max_anisotropy=a, **state), W, H, (-9.2, -2.3), (12.4, 3.1)))["color"]
              for a in (1, 8)]
    assert np.array_equal(frames[0], frames[1])


# ---- 6. defaults -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["textured", "mips", "aniso"])
def test_the_default_sampler_is_the_sampler_of_before(mirhi, device, scenes, case):
    """set_sampler(default) on every texture of a small case, then a new recording: the frame of before, bit for bit.  The getter round-trips."""
    scene = scenes.SMALL_CASES[case]()
    for fmt in _formats(mirhi):
        res = mirhi.SceneResources(device, scene, fmt, want_prim=True, want_depth=True)
        res.render()
        before = {k: v.copy() for k, v in res.read().items()}
        images = {id(img): img for st in res.draw_state for img in st["textures"] if img is not None}
        assert images
        for img in images.values():
            assert img.sampler.as_tuple() == (0, 0, 0, 0, 0)
            img.set_sampler(address_u=mirhi.AddressMode.CLAMP_TO_EDGE, min_filter=mirhi.SamplerFilter.NEAREST, mip_mode=mirhi.MipMode.BASE)
            assert img.sampler.as_tuple() == (2, 0, 0, 1, 2)
            img.set_sampler(mirhi.SamplerDesc())
            assert img.sampler.as_tuple() == (0, 0, 0, 0, 0)
        res.cmd.reset()
        res.record()
        res.render()
        after = res.read()
        for k in before:
            assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), (case, k)
        res.destroy()


def test_sampler_state_takes_effect_for_draws_recorded_afterwards(mirhi, device, scenes):
    """Like max_anisotropy: a recorded command buffer keeps the state it was recorded with."""
    tex = sc.noise_texture(8, 8, 20)
    res = mirhi.SceneResources(device, sc.quad_scene(scenes, sc.texture(scenes, tex), W, H, *WIDE), mirhi.Format.R32G32B32A32_SFLOAT, want_prim=True)
    res.render()
    repeat = res.read()["color"].copy()
    img = res.draw_state[0]["textures"][0]
    img.set_sampler(address_u=sc.MIRRORED_REPEAT, address_v=sc.MIRRORED_REPEAT)
    res.render()                                                     # the old recording
    assert np.array_equal(res.read()["color"], repeat)
    res.cmd.reset()
    res.record()
    res.render()
    mirrored = res.read()["color"].copy()
    res.destroy()
    scene, _ = sc.pair(scenes, tex, W, H, WIDE[0], WIDE[1], sc.MIRRORED_REPEAT, sc.MIRRORED_REPEAT)
    assert np.array_equal(mirrored, _render(mirhi, device, scene)["color"]) and not np.array_equal(mirrored, repeat)


# ---- 7. routes -------------------------------------------------------------------------------------------------------------------------
def _alpha_texture(seed):
    tex = sc.noise_texture(8, 8, seed)
    tex[..., 3] = np.where(tex[..., 3] > 90, 255, tex[..., 3])        # alpha on both sides of the cutoff 0.5, mostly kept
    return tex


@pytest.mark.parametrize("route", ["masked", "masked-normal", "ordered"])
def test_clamp_through_the_masked_scope_and_an_ordered_segment(mirhi, oracle, device, scenes, route):
    """MODEL_PBR draws with a clamped texture over an opaque default-sampler background.
    masked: a discard scope (fragment_discard_enable) whose front draw clamps its BASE COLOUR texture -- kept and discarded fragments are decided
      by the clamped texel's alpha; such a scope takes the ordered resolve (the masked raster variants test alpha under the default sampler only,
      DESIGN.md 8i).
    masked-normal: the same scope with the base colour under the default sampler and the NORMAL MAP clamped -- the scope stays on the masked
      raster variants, whose shading of the winning fragment knows the state.
    ordered: an alpha-blended segment."""
    tex, back = _alpha_texture(21), sc.noise_texture(8, 8, 22)
    normal = sc.noise_texture(8, 8, 28)
    normal[..., 0:2] = 88 + normal[..., 0:2] // 4
    normal[..., 2] = 230
    extra = dict(blend=scenes.ALPHA_BLEND) if route == "ordered" else dict(alpha_test=True, alpha_cutoff=0.5)
    depth = dict(depth_test=True, depth_write=True)
    on_normal = route == "masked-normal"
    clamp = dict(address_u=sc.CLAMP_TO_EDGE, address_v=sc.CLAMP_TO_EDGE)

    def build(front_tex, front_normal, uv0, uv1):
        return scenes.Scene(f"clamp-{route}", W, H, [
            sc.quad_draw(scenes, sc.texture(scenes, back), (0.0, 0.0), (2.0, 2.0), pbr=True, **depth),
            sc.quad_draw(scenes, front_tex, uv0, uv1, pbr=True, normal_map=front_normal, rect=(-0.75, -0.75, 0.875, 0.875), **depth, **extra)],
            clear_color=(0.1, 0.2, 0.3, 1.0))
    scene = build(sc.texture(scenes, tex, **({} if on_normal else clamp)), sc.texture(scenes, normal, **clamp) if on_normal else None, *INSIDE_8)
    # (inside [0, 1] every mode agrees and outside it REPEAT on [[T, T], [T, T]] with halved uv is REPEAT on T: the default-sampler texture rebuilt alike)
    ref_scene = build(sc.texture(scenes, sc.extended(tex, *((sc.REPEAT, sc.REPEAT) if on_normal else (sc.CLAMP_TO_EDGE, sc.CLAMP_TO_EDGE)))),
                      sc.texture(scenes, sc.extended(normal, sc.CLAMP_TO_EDGE, sc.CLAMP_TO_EDGE)) if on_normal else None,
                      sc.halved(INSIDE_8[0]), sc.halved(INSIDE_8[1]))
    for s in (scene, ref_scene):
        s.draws[0].vertices[:, 2], s.draws[1].vertices[:, 2] = 0.5, 0.25      # (clip z = depth: the second quad in front of the first)
    ref = oracle.render(ref_scene, want_bgra8=True)
    if route != "ordered":
        assert 200 < int((ref["prim"] >= 2).sum()) < int((ref["prim"] != 0xFFFFFFFF).sum())      # some fragments kept, some discarded
    for fmt in _formats(mirhi):
        _check(_render(mirhi, device, scene, fmt, want_depth=True), ref, f"clamp-{route}-{fmt}", depth=route != "ordered")
    if on_normal:       # the clamp shows: the frame differs from the one with the normal map under the default sampler
        plain = build(sc.texture(scenes, tex), sc.texture(scenes, normal), *INSIDE_8)
        plain.draws[0].vertices[:, 2], plain.draws[1].vertices[:, 2] = 0.5, 0.25
        assert np.abs(_render(mirhi, device, plain, want_depth=True)["color"] - _render(mirhi, device, scene, want_depth=True)["color"]).max() > 0.01


def test_pbr_draw_with_different_samplers_on_albedo_and_normal_map(mirhi, oracle, device, scenes):
    """The state is per texture slot: a mirrored NEAREST base colour and a clamped LINEAR normal map in one MODEL_PBR draw."""
    albedo = sc.noise_texture(8, 8, 23)
    normal = sc.noise_texture(8, 8, 24)
    normal[..., 0:2] = 88 + normal[..., 0:2] // 4
    normal[..., 2] = 230
    uv0, uv1 = INSIDE_8
    scene = scenes.Scene("pbr-two-samplers", W, H, [sc.quad_draw(
        scenes, sc.texture(scenes, albedo, address_u=sc.MIRRORED_REPEAT, address_v=sc.MIRRORED_REPEAT), uv0, uv1, pbr=True,
        normal_map=sc.texture(scenes, normal, address_u=sc.CLAMP_TO_EDGE, address_v=sc.CLAMP_TO_EDGE))])
    ref_scene = scenes.Scene("pbr-two-samplers-ref", W, H, [sc.quad_draw(
        scenes, sc.texture(scenes, sc.extended(albedo, sc.MIRRORED_REPEAT, sc.MIRRORED_REPEAT)), sc.halved(uv0), sc.halved(uv1), pbr=True,
        normal_map=sc.texture(scenes, sc.extended(normal, sc.CLAMP_TO_EDGE, sc.CLAMP_TO_EDGE)))])
    _check_pair(mirhi, oracle, device, scene, ref_scene, "pbr-two-samplers")
    swapped = copy.deepcopy(scene)
    swapped.draws[0].albedo_map.address_u = swapped.draws[0].albedo_map.address_v = sc.CLAMP_TO_EDGE
    assert np.abs(_render(mirhi, device, swapped)["color"] - _render(mirhi, device, scene)["color"]).max() > 0.01


def test_mixed_scope_one_default_and_one_mirrored_draw(mirhi, oracle, device, scenes):
    """Two draws of one scope, the left half under the default sampler and the right half mirrored: the scope runs the full-featured program
    class, and the default draw's slot executes the default sequence there."""
    tex = sc.noise_texture(8, 8, 25)
    left, right = (-1.0, -1.0, 0.0, 1.0), (0.0, -1.0, 1.0, 1.0)
    scene = scenes.Scene("mixed", W, H, [sc.quad_draw(scenes, sc.texture(scenes, tex), WIDE[0], WIDE[1], rect=left),
                                         sc.quad_draw(scenes, sc.texture(scenes, tex, address_u=sc.MIRRORED_REPEAT, address_v=sc.MIRRORED_REPEAT), WIDE[0], WIDE[1], rect=right)])
    ref_scene = scenes.Scene("mixed-ref", W, H, [sc.quad_draw(scenes, sc.texture(scenes, tex), WIDE[0], WIDE[1], rect=left),
                                                 sc.quad_draw(scenes, sc.texture(scenes, sc.extended(tex, sc.MIRRORED_REPEAT, sc.MIRRORED_REPEAT)),
                                                              sc.halved(WIDE[0]), sc.halved(WIDE[1]), rect=right)])
    ref = _check_pair(mirhi, oracle, device, scene, ref_scene, "mixed-scope")
    assert int((ref["prim"] < 2).sum()) == int((ref["prim"] >= 2).sum()) == W * H // 2


def test_rerecorded_frame_loop_changes_the_sampler_between_frames(mirhi, oracle, scenes):
    """Two frames in flight on two queue lanes, six frames; every frame sets another sampler on its slot's texture and re-records its command
    buffer.  Each frame is the oracle's frame of the equivalent scene."""
    dev = mirhi.Device(0)
    dev.set_queue_lanes(2)
    tex = sc.noise_texture(8, 8, 26)
    modes = [(sc.REPEAT, sc.REPEAT), (sc.MIRRORED_REPEAT, sc.MIRRORED_REPEAT), (sc.CLAMP_TO_EDGE, sc.MIRRORED_REPEAT)]
    refs = [oracle.render(sc.quad_scene(scenes, sc.texture(scenes, sc.extended(tex, *m)), W, H, sc.halved(INSIDE_8[0]), sc.halved(INSIDE_8[1])), want_bgra8=False) for m in modes]
    slots = []
    for k in range(2):
        res = mirhi.SceneResources(dev, sc.quad_scene(scenes, sc.texture(scenes, tex), W, H, *INSIDE_8), mirhi.Format.R32G32B32A32_SFLOAT, want_prim=True)
        res.cmd.set_queue_lane(k)
        slots.append((res, mirhi.Fence(dev, signaled=True)))
    expected = {}

    def verify(f):
        res, fence = slots[f % 2]
        fence.wait()
        _check({"color": res.color.read(), "prim": res.prim.read()}, expected.pop(f), f"frame {f}")

    for f in range(6):
        res, fence = slots[f % 2]
        if f >= 2:
            verify(f - 2)
        fence.reset()
        m = modes[f % 3]                                        # (slot 0: modes 0, 2, 1; slot 1: modes 1, 0, 2)
        res.draw_state[0]["textures"][0].set_sampler(address_u=m[0], address_v=m[1])
        res.cmd.reset()
        res.record()
        res.render(fence)
        expected[f] = refs[modes.index(m)]
    verify(4)
    verify(5)
    for res, fence in slots:
        res.destroy()
        fence.destroy()
    dev.destroy()


def test_tile_split_at_world_two(mirhi, scenes):
    """Each rank's tile rows of a mirrored frame, rendered one after the other into one target, tile the unsplit frame exactly."""
    from renderer_rs_amd import multigpu
    tex = sc.noise_texture(8, 8, 27)
    scene, _ = sc.pair(scenes, tex, W, 96, WIDE[0], WIDE[1], sc.MIRRORED_REPEAT, sc.CLAMP_TO_EDGE)
    dev = mirhi.Device(0)
    whole = mirhi.SceneResources(dev, scene, mirhi.Format.B8G8R8A8_SRGB)
    whole.render()
    ref = whole.read()["color"].copy()
    whole.destroy()
    target = mirhi.Image(dev, scene.width, scene.height, mirhi.Format.B8G8R8A8_SRGB)
    expect = np.full((scene.height, scene.width, 4), 0xA5, dtype=np.uint8)
    target.upload(expect)
    for rank in range(2):
        dev.set_tile_split(rank, 2, layout="bands")
        res = mirhi.SceneResources(dev, scene, mirhi.Format.B8G8R8A8_SRGB, color_image=target)
        res.render()
        dev.wait_idle()
        for r0, r1 in multigpu.owned_pixel_rows(scene.height, rank, 2, "bands"):
            expect[r0:r1] = ref[r0:r1]
        assert np.array_equal(target.read(), expect), f"rank {rank}"
        res.color = None
        res.destroy()
    assert np.array_equal(target.read(), ref) and len(np.unique(ref.reshape(-1, 4), axis=0)) > 50
    target.destroy()
    dev.set_tile_split(0, 1)
    dev.destroy()


def test_refusals(mirhi, device):
    """An enum out of range, a NULL desc, and every image that cannot sit in a material texture slot: refused with a message, state unchanged."""
    import ctypes as C
    img = mirhi.Image(device, 8, 8, mirhi.Format.R8G8B8A8_UNORM)
    img.set_sampler(address_u=mirhi.AddressMode.CLAMP_TO_EDGE)
    for field, bad in (("address_u", 3), ("address_v", -1), ("mag_filter", 2), ("min_filter", 7), ("mip_mode", 3), ("mip_mode", -2)):
        with pytest.raises(mirhi.RhiError) as e:
            img.set_sampler(**{field: bad})
        assert field in e.value.message and e.value.variant == "VulkanError", e.value.message
    assert mirhi.lib().mirhi_image_set_sampler(img.handle, None) == mirhi.ERR_INVALID_HANDLE
    assert b"null" in mirhi.lib().mirhi_last_error_message()
    assert mirhi.lib().mirhi_image_sampler(img.handle, None) == mirhi.ERR_INVALID_HANDLE
    assert img.sampler.as_tuple() == (2, 0, 0, 0, 0)
    srgb = mirhi.Image(device, 4, 4, mirhi.Format.R8G8B8A8_SRGB)
    srgb.set_sampler(mip_mode=mirhi.MipMode.NEAREST)                  # both R8G8B8A8 formats are material textures
    others = [mirhi.Image(device, 8, 8, mirhi.Format.D32_SFLOAT), mirhi.Image(device, 8, 8, mirhi.Format.R32G32B32A32_SFLOAT),
              mirhi.Image(device, 8, 8, mirhi.Format.B8G8R8A8_SRGB), mirhi.Image.create_cube(device, 8, 1)]
    array = mirhi.Image.array(device, 8, 8, 2, mirhi.Format.D32_SFLOAT)
    view = array.layer_view(1)
    for other, word in zip(others + [array, view], ["R8G8B8A8", "R8G8B8A8", "R8G8B8A8", "cube", "array", "array"]):
        with pytest.raises(mirhi.RhiError) as e:
            other.set_sampler(address_u=mirhi.AddressMode.CLAMP_TO_EDGE)
        assert e.value.variant == "InvalidHandle" and word in e.value.message, e.value.message
        desc = mirhi.SamplerDesc()
        assert mirhi.lib().mirhi_image_sampler(other.handle, C.byref(desc)) == 0 and desc.as_tuple() == (0, 0, 0, 0, 0)
    view.destroy()
    for i in others + [array, srgb, img]:
        i.destroy()
