"""ordered_kernel against the model of fragment order and blending (tests/ordered_cases.py) and against the oracle.

Per case the scene is rendered twice on one SceneResources (the second submit runs over the slot arrays the first one re-armed) and every live
triangle alone and opaque, on the same device.  On an R32G32B32A32_SFLOAT target the frame must EQUAL the model's frame built from the GPU's own
layers -- colour bits, depth bits, primitive ids -- and agree with the oracle's: ids and depth bit for bit, colour within the project's 1e-4.  The
launch record (mirhi_debug_raster_trace) must show ordered_kernel for every segment a case means to be ordered; the last test holds that against the
whole module.  tests/test_ordered_cpu.py holds the model, the cases' conditions and the planted errors, without a GPU."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import ordered_cases as oc
import render_area_cases as rc

pytestmark = pytest.mark.gpu

NO_PRIM = oc.NO_PRIM
FLOAT = {c.name: c for c in oc.float_cases()}
SRGB8 = {c.name: c for c in oc.srgb8_cases()}
SPLIT = {c.name: c for c in oc.split_cases()}
SENT = rc.sentinels(oc.W, oc.H, seed=5)
PRIOR = oc.Frame(SENT["float"], SENT["depth"], SENT["prim"])
ORDERED_SEEN = {}       # test id -> (ordered launches seen, ordered launches the case means)


class Trace:
    """with Trace(mirhi) as t: ...; t.names: the entry names of the raster launches in between (as tests/test_gpu_variant_ledger.py reads them)."""

    def __init__(self, mirhi):
        lib = C.CDLL(mirhi.LIB_PATH)
        self.enable, self.read = lib.mirhi_debug_raster_trace, lib.mirhi_debug_raster_trace_read
        self.enable.argtypes, self.enable.restype = [C.c_uint32], None
        self.read.argtypes, self.read.restype = [C.c_char_p, C.c_uint32], C.c_uint32
        self.names = []

    def _drain(self):
        buf = C.create_string_buffer(1 << 16)
        n = self.read(buf, len(buf))
        return buf.value.decode().split("\n") if n else []

    def __enter__(self):
        self._drain()
        self.enable(1)
        return self

    def __exit__(self, *exc):
        self.enable(0)
        self.names = self._drain()
        return False

    @property
    def ordered(self):
        return sum(1 for n in self.names if n.startswith("ordered_kernel<"))


def render(mirhi, dev, scene, fmt=None, want_depth=True, prior=None, submits=1):
    """`submits` frames of the scene on one SceneResources: (the frames, the launch record of all submits, last_status).  prior: the attachments'
    contents before the first submit."""
    F = mirhi.Format
    fmt = F.R32G32B32A32_SFLOAT if fmt is None else fmt
    imgs, kw = [], {}
    if prior is not None:
        color, prim, depth = mirhi.Image(dev, scene.width, scene.height, fmt), mirhi.Image(dev, scene.width, scene.height, F.R32_UINT), mirhi.Image(dev, scene.width, scene.height, F.D32_SFLOAT)
        imgs += [prim, depth]           # (the resources destroy the colour image)
        kw = dict(color_image=color, prim_image=prim, depth_image=depth)
    res = mirhi.SceneResources(dev, scene, fmt, want_prim=True, want_depth=want_depth, **kw)
    frames, status = [], 0
    try:
        with Trace(mirhi) as tr:
            for _ in range(submits):
                if prior is not None:
                    dev.wait_idle()
                    color.upload(np.ascontiguousarray(prior.color)); prim.upload(np.ascontiguousarray(prior.prim)); depth.upload(np.ascontiguousarray(prior.depth))
                res.render()
                frames.append(res.read())
                status |= dev.stats().last_status
    finally:
        res.destroy()
        for im in imgs:
            im.destroy()
    return frames, tr, status


@pytest.fixture(scope="module")
def layers(mirhi, device, scenes):
    """The GPU's single-layer renders, each made once: sources(case) -> key -> (cover, depth, colour)."""
    cache = {}

    def one(scene, key):
        k = (scene.width, scene.height, key)
        if k not in cache:
            (got,), _, status = render(mirhi, device, scene)
            assert status == 0
            cache[k] = got
        return cache[k]
    return lambda c: oc.sources_of(c, scenes, one)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_frames(a, b):
    return all(np.array_equal(bits(a[k]) if a[k].dtype != np.uint8 else a[k], bits(b[k]) if b[k].dtype != np.uint8 else b[k]) for k in a)


def assert_equals_model(got, frame, what):
    bad = np.any(bits(got["color"]) != bits(frame.color), axis=-1) | (got["prim"] != frame.prim)
    if "depth" in got:
        bad |= bits(got["depth"]) != bits(frame.depth)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ from the model, the first at {tuple(np.argwhere(bad)[0][::-1])}"


def oracle_frame(c, oracle, scenes, want_bgra8=False):
    scene = oc.scene_of(c, scenes, area=False)
    if c.render_area is None:
        return oracle.render(scene, want_bgra8=want_bgra8)
    ref = oracle.render(rc.cut_to_area(scene, c.render_area), want_bgra8=False)
    return {"rgba": rc.compose(ref["rgba"], PRIOR.color, c.render_area), "prim": rc.compose(ref["prim"], PRIOR.prim, c.render_area),
            "depth": rc.compose(ref["depth"], PRIOR.depth, c.render_area)}


def assert_agrees_with_oracle(got, ref, what):
    assert np.array_equal(got["prim"], ref["prim"]), f"{what}: winning primitive differs from the oracle's"
    if "depth" in got:
        assert np.array_equal(bits(got["depth"]), bits(ref["depth"])), f"{what}: depth differs from the oracle's"
    err = np.abs(got["color"].astype(np.float64) - ref["rgba"].astype(np.float64)).max()
    print(f"{what}: max |colour - oracle| {err:.3g}")
    assert err < 1e-4


def record_ordered(name, tr, c, submits):
    ORDERED_SEEN[name] = (tr.ordered, c.ordered_segments() * submits)
    assert tr.ordered == c.ordered_segments() * submits, f"{name}: {tr.ordered} ordered launches, meant {c.ordered_segments() * submits}; the launch record holds {sorted(set(tr.names))}"


def untouched(c, src, draws):
    """The pixels no fragment of `draws` can reach: outside the cover of all their layers."""
    hit = np.zeros((c.height, c.width), dtype=bool)
    for di in draws:
        for L in oc.layers_of(c, di, src):
            hit |= L.cover
    return ~hit


@pytest.mark.parametrize("name", list(FLOAT))
def test_float_case(name, mirhi, oracle, device, scenes, layers):
    c = FLOAT[name]
    prior = PRIOR if c.render_area is not None else None
    (a, b), tr, status = render(mirhi, device, oc.scene_of(c, scenes), want_depth=c.want_depth, prior=prior, submits=2)
    assert status == 0
    record_ordered(name, tr, c, 2)
    assert same_frames(a, b), "the second submit over the re-armed slot arrays gives another frame"
    src = layers(c)
    assert_equals_model(a, oc.model_frame(c, src, prior=prior), name)
    assert_agrees_with_oracle(a, oracle_frame(c, oracle, scenes), name)
    if "base_draws" in c.expect:
        # the frame the earlier segments leave alone; what the ordered segment's triangles do not cover is byte for byte that
        (base,), _, _ = render(mirhi, device, oc.scene_of(c, scenes, draws=c.expect["base_draws"]))
        keep = untouched(c, src, [di for di in range(len(c.draws)) if di not in c.expect["base_draws"]])
        assert keep[:32, 32:64].any() and not keep[:32, 32:64].all()         # tile A holds touched and untouched pixels
        for k in ("color", "prim", "depth"):
            assert np.array_equal(bits(a[k])[keep], bits(base[k])[keep]), k
    if name == "untouched_first_segment_clear":
        keep = untouched(c, src, range(len(c.draws)))
        clear = oc.initial_frame(c)
        assert np.array_equal(bits(a["color"])[keep], bits(clear.color)[keep]) and (a["prim"][keep] == NO_PRIM).all() and np.array_equal(bits(a["depth"])[keep], bits(clear.depth)[keep])
    if c.render_area is not None:
        out = ~rc.mask(c.render_area, c.width, c.height)
        assert np.array_equal(bits(a["color"])[out], bits(PRIOR.color)[out]) and np.array_equal(a["prim"][out], PRIOR.prim[out]) and np.array_equal(bits(a["depth"])[out], bits(PRIOR.depth)[out])


ONE_CODE = {}


@pytest.mark.parametrize("name", list(SRGB8))
def test_srgb8_single_segment(name, mirhi, oracle, device, scenes, layers):
    """B8G8R8A8_SRGB, one ordered segment: the model's float frame through the sRGB OETF in float64, rounded to nearest, within ONE code of the
    stored byte (the store's encode uses the hardware's 1-ulp log2 / exp2); what no fragment touched is byte for byte the frame of
    the same segment with every triangle degenerate."""
    c = SRGB8[name]
    assert c.ordered_segments() == 1 and len(c.segments()) == 1
    fmt = mirhi.Format.B8G8R8A8_SRGB
    (a, b), tr, status = render(mirhi, device, oc.scene_of(c, scenes), fmt=fmt, submits=2)
    assert status == 0
    record_ordered(name, tr, c, 2)
    assert same_frames(a, b)
    src = layers(c)
    frame = oc.model_frame(c, src)
    assert np.array_equal(a["prim"], frame.prim) and np.array_equal(bits(a["depth"]), bits(frame.depth))
    diff = np.abs(a["color"].astype(np.int32) - oc.srgb8_of(frame.color).astype(np.int32))
    ONE_CODE[name] = (int((diff.max(axis=-1) == 1).sum()), int((frame.prim != NO_PRIM).sum()))
    print(f"{name}: {ONE_CODE[name][0]} of {ONE_CODE[name][1]} touched pixels are one code from the float64 encoding, max {diff.max()}")
    assert diff.max() <= 1
    empty = dataclasses.replace(c, draws=[dataclasses.replace(d, slots=[oc.ZERO] * len(d.slots)) for d in c.draws])
    (base,), _, _ = render(mirhi, device, oc.scene_of(empty, scenes), fmt=fmt)
    keep = frame.prim == NO_PRIM
    assert keep.any() and (base["prim"] == NO_PRIM).all()
    assert np.array_equal(a["color"][keep], base["color"][keep]) and np.array_equal(bits(a["depth"])[keep], bits(base["depth"])[keep])


def test_srgb8_untouched_behind_opaque(mirhi, oracle, device, scenes, layers):
    """Case e on the 8-bit target: the ordered segment decodes, blends and re-encodes only what its triangles cover; every other byte of colour, id and
    depth is the opaque segment's.  (Two segments: the covered pixels are within the 2 codes tests/test_gpu_api.py states for a re-quantised segment.)"""
    c = FLOAT["untouched_behind_opaque"]
    fmt = mirhi.Format.B8G8R8A8_SRGB
    (a, b), tr, status = render(mirhi, device, oc.scene_of(c, scenes), fmt=fmt, submits=2)
    assert status == 0 and same_frames(a, b)
    record_ordered("srgb8_untouched_behind_opaque", tr, c, 2)
    (base,), _, _ = render(mirhi, device, oc.scene_of(c, scenes, draws=c.expect["base_draws"]), fmt=fmt)
    keep = untouched(c, layers(c), [1])
    assert keep[:32, 32:64].any() and not keep[:32, 32:64].all()
    assert np.array_equal(a["color"][keep], base["color"][keep]) and np.array_equal(a["prim"][keep], base["prim"][keep]) and np.array_equal(bits(a["depth"])[keep], bits(base["depth"])[keep])
    ref = oracle.render(oc.scene_of(c, scenes), want_bgra8=True)
    assert np.array_equal(a["prim"], ref["prim"]) and np.array_equal(bits(a["depth"]), bits(ref["depth"]))
    assert np.abs(a["color"].astype(np.int32) - ref["bgra8"].astype(np.int32)).max() <= 2


@pytest.mark.parametrize("layout", ["bands", "interleaved"])
@pytest.mark.parametrize("name", list(SPLIT))
def test_row_split(name, layout, mirhi, oracle, device, scenes, layers):
    """One GPU as rank r of a world of 2, rank after rank (as tests/test_gpu_binning.py test_row_split): the ranks' rows assemble into the unsplit
    frame bit for bit, and that frame is the model's."""
    from renderer_rs_amd import multigpu
    c = SPLIT[name]
    scene = oc.scene_of(c, scenes)
    (whole,), tr, status = render(mirhi, device, scene)
    assert status == 0
    record_ordered(f"{name}-{layout}", tr, c, 1)
    assert_equals_model(whole, oc.model_frame(c, layers(c)), name)
    assert_agrees_with_oracle(whole, oracle_frame(c, oracle, scenes), name)
    lives = untouched(c, layers(c), range(len(c.draws))) == False
    assert lives[:32].any() and lives[32:].any()        # the live triangles lie in both tile rows
    out = {k: np.zeros_like(v) for k, v in whole.items()}
    owners = np.zeros(c.height, dtype=np.int32)
    for rank in range(2):
        dev = mirhi.Device(0)
        try:
            dev.set_tile_split(rank, 2, layout=layout)
            (got,), rtr, rstatus = render(mirhi, dev, scene)
        finally:
            dev.destroy()
        assert rstatus == 0 and rtr.ordered == 1
        mine = np.zeros(c.height, dtype=bool)
        for r0, r1 in multigpu.owned_pixel_rows(c.height, rank, 2, layout):
            mine[r0:r1] = True
        for k in out:
            out[k][mine] = got[k][mine]
        owners += mine
    assert (owners == 1).all()
    for k in out:
        assert np.array_equal(bits(out[k]), bits(whole[k])), k


def test_every_case_took_the_ordered_path():
    """The closing check: every case of this module that ran showed as many ordered_kernel launches as it has ordered segments -- none passed by taking
    another path -- and the module's cases are all here."""
    assert ORDERED_SEEN and all(seen == meant and meant > 0 for seen, meant in ORDERED_SEEN.values()), {k: v for k, v in ORDERED_SEEN.items() if v[0] != v[1] or v[1] == 0}
    if len(ORDERED_SEEN) >= len(FLOAT) + len(SRGB8):        # (a run of the whole module, not of a selection)
        assert set(FLOAT) | set(SRGB8) | {"srgb8_untouched_behind_opaque"} | {f"{n}-{l}" for n in SPLIT for l in ("bands", "interleaved")} == set(ORDERED_SEEN)
    print("one-code pixels on the sRGB8 target:", ONE_CODE)
