"""Seamless cube filtering on the GPU (include/mirhi.h "The sampler", mirhi_image_set_cube_seamless): the sky as the sampler probe, the
default and the off state, an sRGB8 target, the precompute passes that read a seamless environment, MODEL_PBR_IBL with one or both cubes seamless and
under shadow cascades, both dispatch paths, a re-recorded frame loop, a tile split, mixed states in one scope, and the refusals.

Every comparison is against renderer_rs_amd.ibl with seamless=True in float64, metric and bound of tests/seamless_cases.py, on EVERY pixel: there is
no tie mask -- the seamless value is continuous, so a float32 face flip costs nothing."""
import dataclasses

import numpy as np
import pytest

import ibl_shading_cases
import seamless_cases as sc
import sky_cases

pytestmark = pytest.mark.gpu
W, H = sc.W, sc.H


class SkyRig:
    """One W x H colour target and a reusable command buffer that records begin_rendering, one SKYBOX draw of `env`, end."""

    def __init__(self, mirhi, device, levels, fmt=None, seamless=None):
        m = self.m = mirhi
        self.dev = device
        self.fmt = m.Format.R32G32B32A32_SFLOAT if fmt is None else fmt
        self.color = m.Image(device, W, H, self.fmt)
        n = int(levels[0].shape[1])
        self.env = m.Image.create_cube(device, n, len(levels)) if seamless is None else m.Image.create_cube(device, n, len(levels), seamless=seamless)
        self.env.upload(m.ibl.pack_cube([np.asarray(l, dtype=np.float32) for l in levels]))
        self.cmd = m.CommandBuffer(device)
        self.pipe = (m.GraphicsPipelineBuilder().vertex_shader(m.Program.SKYBOX).fragment_shader(m.Program.SKYBOX).vertex_binding(0).vertex_attributes(())
                     .color_attachment_format(self.fmt).cull_mode(0).depth_test_enable(False).depth_write_enable(False).build(device))

    def record(self, matrix, cmd=None):
        m, cmd = self.m, cmd or self.cmd
        cmd.begin_reusable()
        cmd.begin_rendering(self.color, clear_color=sc.CLEAR)
        cmd.set_viewport(0.0, 0.0, float(W), float(H), 0.0, 1.0)
        cmd.set_scissor(0, 0, W, H)
        cmd.bind_pipeline(self.pipe)
        cmd.bind_skybox(self.env)
        cmd.push_constants(0, 0, np.ascontiguousarray(matrix, dtype=np.float32).tobytes())
        cmd.draw(3, 1, 0, 0)
        cmd.end_rendering()
        cmd.end()

    def run(self, cmd=None):
        self.dev.submit([cmd or self.cmd], None)
        self.dev.wait_idle()
        return self.color.read()

    def frame(self, matrix):
        self.record(matrix)
        return self.run()

    def destroy(self):
        self.dev.wait_idle()
        self.cmd.destroy()
        for o in (self.pipe, self.env, self.color):
            o.destroy()


def _check(name, gpu, m64, m32):
    e32 = sc.err(m32, m64)
    limit = sc.bound(e32)
    got = sc.err(gpu, m64)
    print(f"SEAMLESS {name}: E32 {e32:.3e} bound {limit:.3e} GPU {got:.3e}")
    assert got <= limit, f"{name}: GPU {got:.3e} > bound {limit:.3e} (E32 {e32:.3e})"
    return got


# ---- the sky as the sampler probe ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.SKY_SIZES)
@pytest.mark.parametrize("pose", sorted(sc.POSES))
def test_sky_against_the_seamless_model(mirhi, device, pose, n):
    levels, m64, m32 = sc.sky_case(pose, n)
    rig = SkyRig(mirhi, device, levels, seamless=True)
    try:
        assert rig.env.cube_seamless is True
        out = rig.frame(sc.sky_matrix(pose))
    finally:
        rig.destroy()
    _check(f"sky {pose} {n}^2", out, m64, m32)          # every pixel


def test_default_and_off_state_and_latching(mirhi, device):
    """Default state, and set then cleared: the clamped sampler's frame, bit for bit the same both ways.  The state is latched when the draw is recorded:
    a recording made under one state keeps it whatever the image's state becomes, a new recording takes the new one."""
    pose, n = "corner", 4
    levels, m64, m32 = sc.sky_case(pose, n)
    matrix = sc.sky_matrix(pose)
    clamped64 = mirhi.ibl.skybox(levels, matrix, sc.VIEWPORT, W, H, np.float64)
    untouched, rig = SkyRig(mirhi, device, levels), SkyRig(mirhi, device, levels)
    try:
        assert untouched.env.cube_seamless is False
        plain = untouched.frame(matrix)
        rig.env.set_cube_seamless(True); rig.env.set_cube_seamless(False)
        assert rig.env.cube_seamless is False
        assert np.array_equal(rig.frame(matrix), plain)
        # the clamped frame is the existing model's wherever no face tie is near (the existing tests' condition), and NOT the seamless model's
        keep = ~mirhi.ibl.tie_mask(sc.sky_directions(pose))
        assert sc.err(plain[keep], clamped64[keep]) <= 1e-4
        assert sc.err(plain, m64) > 0.05
        rig.env.set_cube_seamless(True)
        assert np.array_equal(rig.run(), plain)                         # the old recording: still latched off
        rig.record(matrix)
        seamless = rig.run()
        _check("latched on", seamless, m64, m32)
        rig.env.set_cube_seamless(False)
        assert np.array_equal(rig.run(), seamless)                      # ... still latched on
        assert np.array_equal(rig.run(), seamless)
        rig.record(matrix)
        assert np.array_equal(rig.run(), plain)
    finally:
        untouched.destroy(); rig.destroy()


def test_sky_on_an_srgb8_target(mirhi, oracle, device):
    """B8G8R8A8_SRGB: each stored byte lies between the oracle's encodings of the float64 model -+ 1e-4, the bound of the float frame (cube values in
    [0, 1]: the relative metric's 1e-4 is at most 1e-4 absolute) -- one code value where the model sits within 1e-4 of a rounding step, none elsewhere."""
    pose, n = "corner", 4
    levels, m64, _ = sc.sky_case(pose, n)
    rig = SkyRig(mirhi, device, levels, fmt=mirhi.Format.B8G8R8A8_SRGB, seamless=True)
    try:
        out = rig.frame(sc.sky_matrix(pose)).astype(np.int64)
    finally:
        rig.destroy()
    lo, hi, mid = (sky_cases.encode_bgra8(oracle, np.clip(m64 + d, 0.0, 1.0)).astype(np.int64) for d in (-1e-4, 1e-4, 0.0))
    off = int((out != mid).any(axis=-1).sum())
    print(f"SEAMLESS sky8: {off} of {W * H} pixels differ from the encoded float64 model")
    assert np.all((out >= lo) & (out <= hi))
    assert off <= W * H // 20


# ---- precompute ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env_cubes(mirhi, device):
    """The 16^2 x 5 environment twice: seamless, and with the state at its default."""
    levels = sc.environment()
    cubes = []
    for seamless in (True, False):
        c = mirhi.Image.create_cube(device, sc.ENV_SIZE, sc.ENV_LEVELS, seamless=seamless)
        c.upload(sc.packed(levels))
        cubes.append(c)
    yield cubes
    device.wait_idle()
    for c in cubes:
        c.destroy()


@pytest.mark.parametrize("seamless", [True, False])
def test_irradiance_reads_the_environments_state(mirhi, device, env_cubes, seamless):
    env = env_cubes[0 if seamless else 1]
    out = mirhi.Image.create_cube(device, sc.IRRADIANCE_OUT, 1, seamless=not seamless)      # (the destination's own state is nobody's business here)
    try:
        out.ibl_irradiance(env)
        got = out.read()
    finally:
        out.destroy()
    m64, m32 = sc.irradiance_models(seamless)
    _check(f"irradiance, env seamless={seamless}", got, sc.packed([m64]), sc.packed([m32]))
    other = sc.irradiance_models(not seamless)[0]
    assert sc.err(sc.packed([other]), sc.packed([m64])) > 10 * sc.bound(sc.err(sc.packed([m32]), sc.packed([m64])))      # the two models can be told apart


@pytest.mark.parametrize("seamless", [True, False])
def test_prefilter_reads_the_environments_state(mirhi, device, env_cubes, seamless):
    size, levels, samples = sc.PREFILTER_CASE
    env = env_cubes[0 if seamless else 1]
    out = mirhi.Image.create_cube(device, size, levels)
    try:
        out.ibl_prefilter(env, samples)
        got = out.cube_levels()
        # from the next call on: the same environment under the other state gives the other result
        env.set_cube_seamless(not seamless)
        out.ibl_prefilter(env, samples)
        flipped = out.cube_levels()
    finally:
        env.set_cube_seamless(seamless)
        out.destroy()
    m64, m32 = sc.prefilter_models(seamless)
    o64, o32 = sc.prefilter_models(not seamless)
    for l in range(levels):           # every texel of every level, level 0 (the single lookup for roughness < 0.01) included
        _check(f"prefilter level {l}, env seamless={seamless}", got[l], m64[l], m32[l])
        _check(f"prefilter level {l}, env seamless={not seamless} (flipped)", flipped[l], o64[l], o32[l])
    assert sc.err(o64[levels - 1], m64[levels - 1]) > 1e-2


# ---- MODEL_PBR_IBL ------------------------------------------------------------------------------------------------------------------------------
def _ibl_frame(mirhi, device, scene, flags, fmt=None, **kw):
    """The frame of `scene` with images made from scene.ibl, the irradiance / prefiltered cubes' states = flags."""
    irr, pre, lut = scene.ibl.create_images(device, mirhi.Image)
    irr.set_cube_seamless(flags[0]); pre.set_cube_seamless(flags[1])
    res = mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT if fmt is None else fmt, want_prim=True, ibl_images=(irr, pre, lut), **kw)
    try:
        res.render()
        out = res.read()
    finally:
        res.destroy()
        for im in (irr, pre, lut):
            im.destroy()
    return out


def _check_facets(name, scene, out, flags):
    py, px, facet = ibl_shading_cases.facet_pixels(scene, out["prim"])
    assert set(facet.tolist()) == set(range(12))
    images = ibl_shading_cases.scene_images(scene)
    m64, s = sc.expected_ambient(scene, images, py, px, facet, np.float64, *flags)
    m32, _ = sc.expected_ambient(scene, images, py, px, facet, np.float32, *flags)
    got = _check(name, out["color"][py, px, :3], m64, m32)            # every covered pixel
    assert np.array_equal(out["color"][py, px, 3], s["alpha"].astype(np.float32))
    bg = out["prim"] == ibl_shading_cases.NO_PRIM
    assert np.array_equal(out["color"][bg], np.broadcast_to(np.array(scene.clear_color, dtype=np.float32), out["color"][bg].shape))
    return got


@pytest.mark.parametrize("roughness", sc.ROUGHNESSES)
def test_model_pbr_ibl_with_both_cubes_seamless(mirhi, device, roughness):
    scene = sc.facets_scene(roughness)
    _check_facets(f"facets, roughness {roughness}", scene, _ibl_frame(mirhi, device, scene, (True, True)), (True, True))


@pytest.mark.parametrize("flags", [(True, False), (False, True)])
def test_model_pbr_ibl_with_one_cube_seamless(mirhi, device, flags):
    scene = sc.facets_scene(0.5)
    _check_facets(f"facets, roughness 0.5, seamless {flags}", scene, _ibl_frame(mirhi, device, scene, flags), flags)


def test_model_pbr_ibl_under_shadow_cascades(mirhi, scenes, device):
    """The facets with the cascades of cascaded_ground_case bound: a cascaded MODEL_PBR_IBL scope (the SHADOWV = 2 instantiations).  No light reaches the
    facets, so Lo is exact zero whatever the shadow term says and the frame is the model's ambient."""
    scene = dataclasses.replace(sc.facets_scene(0.5), cascades=scenes.cascaded_ground_case(160, 120, map_size=128).cascades)
    base = sc.facets_scene(0.5)
    scene.facets, scene.view, scene.proj, scene.eye = base.facets, base.view, base.proj, base.eye
    _check_facets("facets under cascades", scene, _ibl_frame(mirhi, device, scene, (True, True)), (True, True))


# ---- the other checks ---------------------------------------------------------------------------------------------------------------------------
def _sky_scene(scenes, pose, n, roughness=0.5):
    """The facets with the random n^2 sky behind them."""
    levels, _, _ = sc.sky_case(pose, n)
    base = sc.facets_scene(roughness)
    scene = dataclasses.replace(base, sky=scenes.SkySpec(inv_view_proj=np.array(sc.sky_matrix(pose)), levels=levels))
    scene.facets, scene.view, scene.proj, scene.eye = base.facets, base.view, base.proj, base.eye
    return scene


def _scene_frame(mirhi, device, scene, ibl_flags, sky_seamless, dev=None):
    dev = dev or device
    irr, pre, lut = scene.ibl.create_images(dev, mirhi.Image)
    irr.set_cube_seamless(ibl_flags[0]); pre.set_cube_seamless(ibl_flags[1])
    env = scene.sky.create_image(dev, mirhi.Image)
    env.set_cube_seamless(sky_seamless)
    res = mirhi.SceneResources(dev, scene, mirhi.Format.R32G32B32A32_SFLOAT, want_prim=True, want_depth=True, ibl_images=(irr, pre, lut), sky_image=env)
    return res, (irr, pre, lut, env)


def _check_sky_behind(name, scene, out, pose, n, ibl_flags, sky_seamless, mirhi):
    levels, m64, m32 = sc.sky_case(pose, n)
    if not sky_seamless:
        m64, m32 = (mirhi.ibl.skybox(levels, sc.sky_matrix(pose), sc.VIEWPORT, W, H, t) for t in (np.float64, np.float32))
    sky = out["prim"] == scene.num_triangles
    assert sky.sum() > 1000 and (~sky).sum() > 1000
    if sky_seamless:
        _check(name + ": sky pixels", out["color"][sky], m64[sky], m32[sky])
    covered = dict(prim=np.where(sky, np.uint32(ibl_shading_cases.NO_PRIM), out["prim"]).astype(np.uint32), color=out["color"])
    py, px, facet = ibl_shading_cases.facet_pixels(scene, covered["prim"])
    images = ibl_shading_cases.scene_images(scene)
    a64, _ = sc.expected_ambient(scene, images, py, px, facet, np.float64, *ibl_flags)
    a32, _ = sc.expected_ambient(scene, images, py, px, facet, np.float32, *ibl_flags)
    if all(ibl_flags):
        _check(name + ": lit pixels", out["color"][py, px, :3], a64, a32)
    return sky, (py, px), (a64, m64)


def test_seamless_sky_behind_a_non_seamless_lit_set(mirhi, scenes, device):
    """One scope, two states: the IBL set's cubes at their default, the environment behind them seamless.  The lit pixels are, bit for bit, those of the same
    scope with a non-seamless sky; the sky pixels are the seamless model's."""
    pose, n = "edge", 4
    scene = _sky_scene(scenes, pose, n)
    frames = {}
    for sky_seamless in (True, False):
        res, imgs = _scene_frame(mirhi, device, scene, (False, False), sky_seamless)
        try:
            res.render()
            frames[sky_seamless] = res.read()
        finally:
            res.destroy()
            for im in imgs:
                im.destroy()
    sky, (py, px), _ = _check_sky_behind("seamless sky, default set", scene, frames[True], pose, n, (False, False), True, mirhi)
    assert np.array_equal(frames[True]["prim"], frames[False]["prim"])
    assert np.array_equal(frames[True]["color"][py, px], frames[False]["color"][py, px])
    assert not np.array_equal(frames[True]["color"][sky], frames[False]["color"][sky])


def test_both_dispatch_paths(mirhi, scenes):
    """A device on the caller's (null) stream keeps lane 0 on HIP launches until set_native_dispatch(True): the seamless kernels through both, same bits."""
    pose, n = "corner", 4
    scene = _sky_scene(scenes, pose, n)
    dev = mirhi.Device(0, stream=0)
    outs, used = [], []
    try:
        res, imgs = _scene_frame(mirhi, None, scene, (True, True), True, dev=dev)
        fence = mirhi.Fence(dev)
        for native in (False, True):
            dev.set_native_dispatch(native)
            before = dev.stats().native_dispatches
            res.render(fence)
            fence.wait(); fence.reset()
            used.append((dev.dispatch_path(), dev.stats().native_dispatches - before))
            outs.append(res.read())
        res.destroy(); fence.destroy()
        for im in imgs:
            im.destroy()
    finally:
        dev.destroy()
    for k in ("color", "prim", "depth"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert used[0][1] == 0 and (used[0][0].startswith("hip:") or "lane 0 stays on the caller's HIP stream" in used[0][0]), used
    assert used[1][0].startswith("native:") and used[1][1] == 4, used          # vertex, geometry, raster of the lit segment, the sky kernel
    _check_sky_behind("both paths", scene, outs[0], pose, n, (True, True), True, mirhi)


def test_frame_loop_toggles_the_state_every_frame(mirhi, scenes, device, monkeypatch):
    """Two frames in flight, each command buffer re-recorded every frame under MIRHI_VERIFY_IDLE=1, the three cubes' states flipped before every recording:
    each frame equals the single frame of the state it was recorded under."""
    monkeypatch.setenv("MIRHI_VERIFY_IDLE", "1")
    pose, n = "corner", 4
    scene = _sky_scene(scenes, pose, n)
    single = {}
    res0, imgs = _scene_frame(mirhi, device, scene, (False, False), False)
    irr, pre, lut, env = imgs
    frames, fences = [res0], []
    try:
        for on in (False, True):
            for im in (irr, pre, env):
                im.set_cube_seamless(on)
            res0.record(); res0.render()
            single[on] = res0.read()
        assert not np.array_equal(single[True]["color"], single[False]["color"])
        _check_sky_behind("frame loop, on", scene, single[True], pose, n, (True, True), True, mirhi)
        frames.append(mirhi.SceneResources(device, scene, mirhi.Format.R32G32B32A32_SFLOAT, want_prim=True, want_depth=True, ibl_images=(irr, pre, lut), sky_image=env))
        fences = [mirhi.Fence(device) for _ in frames]
        on = False
        for step in range(4):
            recorded = []
            for res, fence in zip(frames, fences):
                on = not on
                for im in (irr, pre, env):
                    im.set_cube_seamless(on)
                res.record()
                res.render(fence)
                recorded.append(on)
            for res, fence, state in zip(frames, fences, recorded):
                fence.wait(); fence.reset()
                out = res.read()
                for k in ("color", "prim", "depth"):
                    assert np.array_equal(out[k], single[state][k]), (step, state, k)
    finally:
        device.wait_idle()
        for res in frames:
            res.destroy()
        for fence in fences:
            fence.destroy()
        for im in imgs:
            im.destroy()


def test_tile_split_assembles_the_unsplit_frame(mirhi, scenes, device):
    pose, n = "edge", 16
    scene = _sky_scene(scenes, pose, n, roughness=1.0)

    def frame():
        res, imgs = _scene_frame(mirhi, device, scene, (True, True), True)
        try:
            res.render()
            return res.read()
        finally:
            res.destroy()
            for im in imgs:
                im.destroy()
    whole = frame()
    assembled = {k: np.zeros_like(v) for k, v in whole.items()}
    try:
        for rank in range(2):
            device.set_tile_split(rank, 2)
            part = frame()
            first, step, rows = device.split_rows(scene.height)
            for k in range(rows):
                r0 = (first + k * step) * 32
                for key in assembled:
                    assembled[key][r0:r0 + 32] = part[key][r0:r0 + 32]
    finally:
        device.set_tile_split(0, 1)
    for key in assembled:
        assert np.array_equal(assembled[key], whole[key]), key
    _check_sky_behind("tile split", scene, whole, pose, n, (True, True), True, mirhi)


def test_refusals(mirhi, scenes, device):
    I, R = mirhi.Image, mirhi.RhiError
    F32 = mirhi.Format.R32G32B32A32_SFLOAT
    flat, arr = I(device, 16, 16, F32), I.array(device, 16, 16, 2, mirhi.Format.D32_SFLOAT)
    ms = I.multisampled(device, 16, 16, F32, 4)
    cube = I.create_cube(device, 4, 1)
    try:
        for img, text in ((flat, "not a cube image"), (arr, "not a cube image"), (ms, "multisampled")):
            with pytest.raises(R) as e:
                img.set_cube_seamless(True)
            assert e.value.variant == "InvalidHandle" and text in str(e.value), str(e.value)
            assert img.cube_seamless is False
        with pytest.raises(R) as e:
            mirhi.check(mirhi.lib().mirhi_image_set_cube_seamless(cube.handle, 2))
        assert e.value.variant == "InvalidHandle" and " 2 " in str(e.value), str(e.value)
        assert cube.cube_seamless is False
        cube.set_cube_seamless(1)
        assert cube.cube_seamless is True and mirhi.lib().mirhi_image_cube_seamless(cube.handle) == 1
        cube.set_cube_seamless(0)
        assert cube.cube_seamless is False
    finally:
        for im in (flat, arr, ms, cube):
            im.destroy()
    # the latched states are part of a scope's IBL set: the same three images under another state are a different set
    scene = sc.facets_scene(0.5)
    irr, pre, lut = scene.ibl.create_images(device, I)
    res = mirhi.SceneResources(device, dataclasses.replace(scene, ibl=None), F32, ibl_images=(irr, pre, lut))
    st = res.draw_state[0]
    try:
        res.cmd.begin_reusable()
        res.cmd.begin_rendering(res.color)
        res.cmd.set_viewport(0, 0, scene.width, scene.height); res.cmd.set_scissor(0, 0, scene.width, scene.height)
        res.cmd.bind_pipeline(st["pipe"]); res.cmd.bind_vertex_buffers(0, [st["vb"]], [0])
        for slot, key in ((mirhi.Slot.CAMERA, "camera"), (mirhi.Slot.OBJECT, "object"), (mirhi.Slot.LIGHTS, "light"), (mirhi.Slot.MATERIAL, "material")):
            res.cmd.bind_uniform(slot, st[key])
        res.cmd.bind_index_buffer(st["ib"], 0, mirhi.IndexType.UINT32)
        res.cmd.bind_ibl(irr, pre, lut)
        res.cmd.draw_indexed(6)
        pre.set_cube_seamless(True)
        with pytest.raises(R) as e:
            res.cmd.draw_indexed(6)
        assert e.value.variant == "InvalidHandle" and "two different IBL sets" in str(e.value), str(e.value)
        pre.set_cube_seamless(False)
        res.cmd.draw_indexed(6)
        res.cmd.end_rendering(); res.cmd.end()
        res.record()
    finally:
        res.destroy()
        for im in (irr, pre, lut):
            im.destroy()
