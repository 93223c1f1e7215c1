"""Every raster kernel instantiation on the GPU against its yardstick: per row of tests/variant_cases.py the knobs are set, the launch
record (mirhi_debug_raster_trace) is switched on, the row's scene is rendered, the row's name must be among the launched kernels' and the frame
must meet the row's yardstick -- the family's anchor the comparison an existing test makes with a high-precision reference, every other row the
anchor's frame bit for bit (variant_cases states the rule).  A row whose kernel was not launched fails with both names; none is skipped.  The
last test holds the union of what this file launched against the three tables."""
import ctypes as C
import dataclasses
import importlib
import inspect

import numpy as np
import pytest

import msaa_cases
import multiview_cases
import render_area_cases as rc
import sky_cases
import variant_cases as vc
from test_gpu_parity import _check

pytestmark = pytest.mark.gpu
NO_PRIM = vc.NO_PRIM
LAUNCHED = set()          # every name a test of this file saw in the launch record


class Trace:
    """with Trace(mirhi) as t: ...; t.names: the entry names of the raster launches in between, in launch order."""

    def __init__(self, mirhi):
        lib = C.CDLL(mirhi.LIB_PATH)
        self.enable, self.read = lib.mirhi_debug_raster_trace, lib.mirhi_debug_raster_trace_read
        self.enable.argtypes, self.enable.restype = [C.c_uint32], None
        self.read.argtypes, self.read.restype = [C.c_char_p, C.c_uint32], C.c_uint32
        self.names = []

    def _drain(self):
        buf = C.create_string_buffer(1 << 16)
        n = self.read(buf, len(buf))
        names = buf.value.decode().split("\n") if n else []
        assert len(names) == n, (n, names)
        return names

    def __enter__(self):
        self._drain()
        self.enable(1)
        return self

    def __exit__(self, *exc):
        self.enable(0)
        self.names = self._drain()
        LAUNCHED.update(self.names)
        return False


@dataclasses.dataclass
class Ctx:
    mirhi: object
    scenes: object
    oracle: object
    device: object
    monkeypatch: object
    failures: list = dataclasses.field(default_factory=list)

    def knobs(self, row):
        for k, v in row.knobs.items():
            self.monkeypatch.setenv(k, v)

    def fail(self, row, what):
        self.failures.append(f"{row.name}: {what}")

    def launched(self, row, names, what=""):
        if row.name not in names:
            self.fail(row, f"not launched{what}; the launch record holds {sorted(set(names))}")
            return False
        return True

    def same(self, row, what, got, want, area=None, sentinel=None, keys=("color", "prim", "depth")):
        for d in vc.frame_differences(got, want, area, sentinel, keys):
            self.fail(row, f"{what}: {d}")

    def done(self):
        assert not self.failures, f"{len(self.failures)} failures:\n" + "\n".join(self.failures)


@pytest.fixture
def ctx(mirhi, scenes, oracle, device, monkeypatch):
    return Ctx(mirhi, scenes, oracle, device, monkeypatch)


SENT = rc.sentinels(vc.W, vc.H)
SENT_FRAME = {"color": SENT["float"], "prim": SENT["prim"], "depth": SENT["depth"]}
MAP_SENT = {"depth": rc.sentinels(vc.MAP, vc.MAP, seed=2)["depth"]}


class Target:
    """One row's scene recorded over prefilled attachments (the sentinel); samples = 4: the scope's own transient attachments, nothing prefilled."""

    def __init__(self, ctx, row, scene):
        m, dev = ctx.mirhi, ctx.device
        self.imgs, self.samples = [], row.samples
        kw = {}
        if getattr(scene, "ibl", None) is not None:
            irr, pre, lut = scene.ibl.create_images(dev, m.Image)
            irr.set_cube_seamless(row.seamless[0]); pre.set_cube_seamless(row.seamless[1])
            kw["ibl_images"] = (irr, pre, lut)
            self.imgs += [irr, pre, lut]
        F = m.Format
        if row.kind == "depth":
            self.map = m.Image(dev, vc.MAP, vc.MAP, F.D32_SFLOAT)
            self.map.upload(np.ascontiguousarray(MAP_SENT["depth"]))
            self.imgs.append(self.map)
            self.res = m.SceneResources(dev, scene, shadow_map=self.map)
        elif row.samples == 4:
            self.res = m.SceneResources(dev, scene, F.R32G32B32A32_SFLOAT, want_prim=True, want_depth=True, samples=4, **kw)
        else:
            color, prim, depth = m.Image(dev, vc.W, vc.H, F.R32G32B32A32_SFLOAT), m.Image(dev, vc.W, vc.H, F.R32_UINT), m.Image(dev, vc.W, vc.H, F.D32_SFLOAT)
            color.upload(np.ascontiguousarray(SENT["float"])); prim.upload(np.ascontiguousarray(SENT["prim"])); depth.upload(np.ascontiguousarray(SENT["depth"]))
            self.imgs += [prim, depth]          # (the resources destroy the colour image)
            self.res = m.SceneResources(dev, scene, F.R32G32B32A32_SFLOAT, color_image=color, prim_image=prim, depth_image=depth, **kw)
        self.kind = row.kind

    def read(self):
        if self.kind == "depth":
            self.res.device.wait_idle()
            return {"depth": self.map.read().reshape(vc.MAP, vc.MAP).copy()}
        return self.res.read()

    def destroy(self):
        self.res.destroy()
        for im in self.imgs:
            im.destroy()


def render(ctx, row, scene):
    """(frame, launched names) of one submit of the row's scene under the row's knobs."""
    ctx.knobs(row)
    t = Target(ctx, row, scene)
    try:
        with Trace(ctx.mirhi) as tr:
            t.res.render()
            out = t.read()
    finally:
        t.destroy()
    return out, tr.names


def scene_of(row, variant, key=None, area=None):
    if row.kind == "depth":
        return vc.depth_scene(row if area is None else dataclasses.replace(row, area=area), variant, key)
    return vc.scene_for(row, variant, key, area)


def oracle_frame(ctx, row, variant, key):
    """The oracle's prim / depth / colour of the row's geometry under a depth state, uncovered depth = the clear value."""
    if row.kind == "depth":
        ref = ctx.oracle.render(vc.depth_oracle_scene(variant, key), want_bgra8=False)
    else:
        ref = ctx.oracle.render(vc.oracle_scene(row, variant, key), want_bgra8=False)
    covered = ref["prim"] != NO_PRIM
    ref["stored"] = np.where(covered, ref["depth"], np.float32(vc.CLEAR_DEPTH[key])).astype(np.float32)
    return ref


# ---- the anchors' own checks ---------------------------------------------------------------------------------------------------------------------
def existing_comparison(ctx, anchor):
    """Runs the comparison ANCHOR_CHECKS names -- a test function of another GPU file, called with this test's fixtures -- under the anchor's knobs with
    the launch record on: its assertions are the anchor's yardstick, and the anchor must be among what it launched."""
    where, args = vc.ANCHOR_CHECKS[anchor.name]
    module, fn = where.split(":")
    f = getattr(importlib.import_module(module), fn)
    fixtures = dict(mirhi=ctx.mirhi, scenes=ctx.scenes, oracle=ctx.oracle, device=ctx.device)
    names = [p for p in inspect.signature(f).parameters]
    call = [fixtures[n] for n in names if n in fixtures] + list(args)
    assert len(call) == len(names), (where, names)
    ctx.knobs(anchor)
    with Trace(ctx.mirhi) as tr:
        f(*call)
    ctx.launched(anchor, tr.names, f" by {where}")


def facets_under_a_shadow_term(ctx, anchor):
    """seamless_cases.facets_scene with this ledger's shadow map / blended cascades bound: no light reaches the facets, so Lo is exact zero whatever the
    shadow term says and the frame is the seamless model's ambient (test_gpu_seamless.test_model_pbr_ibl_under_shadow_cascades, for the other two terms)."""
    import seamless_cases as sc
    from test_gpu_seamless import _check_facets, _ibl_frame
    base = sc.facets_scene(0.5)
    scene = dataclasses.replace(base, **vc.shadow_term(anchor.shadow))
    scene.facets, scene.view, scene.proj, scene.eye = base.facets, base.view, base.proj, base.eye
    ctx.knobs(anchor)
    with Trace(ctx.mirhi) as tr:
        out = _ibl_frame(ctx.mirhi, ctx.device, scene, (True, True))
    _check_facets(f"facets under shadow term {anchor.shadow}", scene, out, (True, True))
    ctx.launched(anchor, tr.names)


def check_against_oracle(ctx, row, frame, ref, what):
    """test_gpu_parity._check (ids bit for bit, colour within its bound, depth bits where covered), and the clear value in every uncovered depth."""
    if "prim" in frame:
        _check(frame, ref, f"{row.name} {what}", depth="depth" in frame)
    if "depth" in frame:
        assert np.array_equal(frame["depth"].view(np.uint32), ref["stored"].view(np.uint32)), f"{row.name} {what}: stored depth differs from the oracle's"


# ---- families of colour scopes -----------------------------------------------------------------------------------------------------------------
def anchor_frames(ctx, anchor):
    """The anchor's frames of the overdraw scene, the twin scene and layer B alone (full extent, LESS), each with the anchor in its launch record."""
    frames = {}
    for variant in ("overdraw", "twin", "B"):
        frames[variant], names = render(ctx, anchor, scene_of(anchor, variant, area=False))
        assert anchor.name in names, f"{anchor.name}: not launched for its own {variant} frame; the launch record holds {names}"
    return frames


def greater_expectation(ctx, row, frames):
    ref = oracle_frame(ctx, row, "overdraw", "greater")
    want = {"prim": ref["prim"], "depth": ref["stored"]}
    if row.kind != "depth":
        want["color"] = vc.compose_by_primitive(ref["prim"], frames["twin"], frames["B"], vc.CLEAR)
    return want, ref


def check_row(ctx, row, frames, want_greater=None):
    """One non-anchor row of a family whose anchor gave `frames`."""
    area = (vc.MAP_AREA if row.kind == "depth" else vc.AREA) if row.area else None
    sentinel = (MAP_SENT if row.kind == "depth" else SENT_FRAME) if row.area else None
    keys = ("depth",) if row.kind == "depth" else ("color", "prim", "depth")
    if row.key == "less":
        got, names = render(ctx, row, scene_of(row, "overdraw"))
        if ctx.launched(row, names):
            ctx.same(row, "overdraw scene against the anchor", got, frames["overdraw"], area, sentinel, keys)
        return
    got, names = render(ctx, row, scene_of(row, "twin"))
    if ctx.launched(row, names, " for the twin scene"):
        ctx.same(row, "twin scene under GREATER against the K = 0 anchor", got, vc.twin_expectation(frames["twin"]), area, sentinel, keys)
    got, names = render(ctx, row, scene_of(row, "overdraw"))
    if ctx.launched(row, names, " for the overdraw scene"):
        ctx.same(row, "overdraw scene under GREATER against the oracle's winners and depth and the anchor's colours", got, want_greater, area, sentinel, keys)


def check_batch_row(ctx, row, frames):
    """Two command buffers -- the overdraw and the twin scene -- in one submit: one batched launch, each frame the anchor's single-launch frame."""
    ctx.knobs(row)
    targets = [Target(ctx, row, scene_of(row, v)) for v in ("overdraw", "twin")]
    fence = ctx.mirhi.Fence(ctx.device)
    try:
        with Trace(ctx.mirhi) as tr:
            ctx.device.submit([t.res.cmd for t in targets], fence)
            fence.wait()
            outs = [t.read() for t in targets]
    finally:
        fence.destroy()
        for t in targets:
            t.destroy()
    if ctx.launched(row, tr.names):
        for out, v in zip(outs, ("overdraw", "twin")):
            ctx.same(row, f"{v} scene in a batched submit against the anchor's single launch", out, frames[v])


COLOUR_FAMILIES = [f for f in vc.FAMILIES if f.startswith(("plain", "masked", "shadow", "csm", "ibl", "sibl", "depth"))]


@pytest.mark.parametrize("family", COLOUR_FAMILIES)
def test_family_against_its_anchor(ctx, family):
    rows = [r for r in vc.ROWS if r.family == family]
    anchor = vc.LEDGER[rows[0].anchor] if family != "depth" else vc.LEDGER[vc.own_name("raster_kernel_depth", 0, 0)]
    check = vc.ANCHOR_CHECKS[anchor.name]
    if not isinstance(check, str):
        existing_comparison(ctx, anchor)
    elif "_check_facets" in check:
        facets_under_a_shadow_term(ctx, anchor)
    frames = anchor_frames(ctx, anchor)
    if isinstance(check, str) and "_check_facets" not in check:          # the oracle is the yardstick of the ledger's own scenes
        for variant in ("overdraw", "twin", "B"):
            check_against_oracle(ctx, anchor, frames[variant], oracle_frame(ctx, anchor, variant, "less"), variant)
    # the family's own terms show in its frames: the shadow term shades hundreds of pixels, the seamless lookups differ from the clamped ones
    for what, other, least in (("shadow term", dataclasses.replace(anchor, shadow=0), 300), ("seamless cubes", dataclasses.replace(anchor, seamless=(False, False, False)), 100)):
        if other != anchor and anchor.kind != "depth":
            without, _ = render(ctx, other, scene_of(other, "overdraw"))
            assert np.array_equal(without["prim"], frames["overdraw"]["prim"])
            changed = int((without["color"].view(np.uint32) != frames["overdraw"]["color"].view(np.uint32)).any(axis=2).sum())
            print(f"LEDGER {family}: the {what} changes {changed} pixels of the anchor's overdraw frame")
            assert changed >= least, f"{family}: the {what} changes only {changed} pixels"
    want_greater, ref_greater = greater_expectation(ctx, anchor, frames)
    assert (ref_greater["prim"] != oracle_frame(ctx, anchor, "overdraw", "less")["prim"]).sum() > 300, "GREATER changes too few winners of the overdraw scene"
    for row in rows:
        if row.name == anchor.name:
            continue
        if row.route == "batch":
            check_batch_row(ctx, row, frames)
        elif row.route == "multiview":
            check_views_row(ctx, row)
        else:
            check_row(ctx, row, frames, want_greater)
    if family.startswith(("plain", "masked")):        # the generic key's overdraw frame against the oracle's colour as well (its bound: test_gpu_parity._check)
        k1 = next(r for r in rows if r.key == "greater" and not r.area and r.route == "single")
        got, _ = render(ctx, k1, scene_of(k1, "overdraw"))
        check_against_oracle(ctx, k1, got, ref_greater, "overdraw under GREATER")
    print(f"LEDGER {family}: anchor {anchor.name}; {len(rows) - 1 - len({f.split(':')[0] for f in ctx.failures})} of {len(rows) - 1} other rows meet their yardstick bit for bit")
    ctx.done()


def check_views_row(ctx, row):
    """A multiview scope of four views against the four single-view scopes (multiview_cases), under the row's key and knobs."""
    m, S, dev = ctx.mirhi, ctx.scenes, ctx.device
    casters, base = vc.view_casters()
    bufs = multiview_cases.CasterBuffers(m, dev, casters)
    pipe = multiview_cases.shadow_pipeline(m, S, dev, compare=S.CMP_GREATER if row.key == "greater" else S.CMP_LESS)
    mats = multiview_cases.view_matrices(base)
    start = multiview_cases.sentinels(4, vc.MAP)
    ctx.knobs(row)
    try:
        args = (m, S, dev, bufs, mats, 0b1111, start, pipe)
        with Trace(m) as tr:
            multi = multiview_cases.run_multiview(*args, clear=vc.CLEAR_DEPTH[row.key])
        with Trace(m) as single_tr:
            single = multiview_cases.run_single(*args, clear=vc.CLEAR_DEPTH[row.key])
    finally:
        pipe.destroy()
        bufs.destroy()
    if ctx.launched(row, tr.names):
        if row.anchor not in single_tr.names:
            ctx.fail(row, f"the single-view scopes did not launch {row.anchor}; their launch record holds {sorted(set(single_tr.names))}")
        try:
            multiview_cases.assert_equivalent(multi, single, start, 0b1111, row.name)
        except AssertionError as e:
            ctx.fail(row, str(e))


# ---- predicate mode, the ordered resolve, 4x MSAA ------------------------------------------------------------------------------------------------
def test_predicate_rows(ctx):
    for p, kind in vc.KINDS.items():
        full, area = vc.LEDGER[vc.plain_name(p, 2, 0, 1, False)], vc.LEDGER[vc.plain_name(p, 2, 0, 1, False, True)]
        frame, names = render(ctx, full, scene_of(full, "overdraw"))
        if ctx.launched(full, names):
            ref = ctx.oracle.render(vc.oracle_scene(full, "overdraw"), want_bgra8=False)
            assert (ref["prim"] != NO_PRIM).sum() > 300
            _check(frame, ref, full.name)
            assert np.all(frame["depth"] == np.float32(vc.CLEAR_DEPTH["predicate"])), f"{full.name}: a scope without depth write changed the depth"
        got, names = render(ctx, area, scene_of(area, "overdraw"))
        if ctx.launched(area, names):
            ctx.same(area, "against its full-extent row", got, frame, vc.AREA, SENT_FRAME)
    ctx.done()


def test_ordered_rows(ctx):
    for p in vc.KINDS:
        row = vc.LEDGER[f"ordered_kernel<{p}>"]
        frame, names = render(ctx, row, scene_of(row, "overdraw"))
        if ctx.launched(row, names):
            check_against_oracle(ctx, row, frame, oracle_frame(ctx, row, "overdraw", "blend"), "overdraw, alpha-blended")
    ctx.done()


def _msaa_want(ctx, scene, clear_depth):
    prim, depth, _ = msaa_cases.oracle_samples(ctx.scenes, ctx.oracle, scene)
    return prim, np.where(prim[:, :, 0] != NO_PRIM, depth[:, :, 0], np.float32(clear_depth)).astype(np.float32)


@pytest.mark.parametrize("p", list(vc.KINDS))
def test_msaa_rows(ctx, p):
    """K = 0: the winners of every sample and the sample-0 depth are the moved-viewport oracle frames' (msaa_cases), and a pixel whose four samples share the 1x
    winner holds the 1x frame's colour bit for bit (the 1x frame: the plain family's anchor, itself held against the oracle in its own test).  K = 1: the twin
    scene reproduces the K = 0 frame; the overdraw scene has the oracle's GREATER winners and depth, and the 1x colour of the winner where the samples agree."""
    k0, k1 = vc.LEDGER[f"raster_kernel_msaa<{p}, 0>"], vc.LEDGER[f"raster_kernel_msaa<{p}, 1>"]
    one_row = vc.LEDGER[vc.plain_name(p, 0, 0, 1, False)]
    one = {v: render(ctx, one_row, scene_of(one_row, v))[0] for v in ("overdraw", "twin", "B")}
    frames = {}
    for variant in ("overdraw", "twin"):
        scene = scene_of(k0, variant)
        assert msaa_cases.condition_holds(ctx.scenes, scene)[1] == 0
        frames[variant], names = render(ctx, k0, scene)
        assert k0.name in names, f"{k0.name}: not launched; the launch record holds {names}"
        prim, depth = _msaa_want(ctx, vc.oracle_scene(k0, variant), 1.0)
        got = frames[variant]
        assert np.array_equal(got["prim"], prim), f"{k0.name} {variant}: {int((got['prim'] != prim).sum())} sample winners differ from the oracle's"
        assert np.array_equal(got["depth"].view(np.uint32), depth.view(np.uint32)), f"{k0.name} {variant}: sample-0 depth differs from the oracle's"
        same = (prim == one[variant]["prim"][:, :, None]).all(axis=2)
        assert same.sum() > 1000 and (~same).sum() > 100
        assert np.array_equal(got["color"].view(np.uint32)[same], one[variant]["color"].view(np.uint32)[same]), f"{k0.name} {variant}: fully covered pixels differ from the 1x frame"
    got, names = render(ctx, k1, scene_of(k1, "twin"))
    if ctx.launched(k1, names, " for the twin scene"):
        ctx.same(k1, "twin scene under GREATER against K = 0", got, vc.twin_expectation(frames["twin"]))
    got, names = render(ctx, k1, scene_of(k1, "overdraw"))
    if ctx.launched(k1, names, " for the overdraw scene"):
        prim, depth = _msaa_want(ctx, vc.oracle_scene(k1, "overdraw", "greater"), 0.0)
        ctx.same(k1, "overdraw scene under GREATER against the oracle's samples", got, {"prim": prim, "depth": depth}, keys=("prim", "depth"))
        agree = (prim == prim[:, :, :1]).all(axis=2)
        want = vc.compose_by_primitive(np.where(agree, prim[:, :, 0], np.uint32(NO_PRIM)), one["twin"], one["B"], vc.CLEAR)
        if not np.array_equal(got["color"].view(np.uint32)[agree], want.view(np.uint32)[agree]):
            ctx.fail(k1, "overdraw scene under GREATER: a pixel whose four samples share a winner does not hold the 1x colour of that primitive")
    ctx.done()


# ---- the sky and the transfer kernels: their own models, as their own files hold them ------------------------------------------------------------
def test_sky_rows(ctx):
    import ibl_shading_cases as ibl_cases
    from test_gpu_seamless import test_sky_against_the_seamless_model
    m = ctx.mirhi
    row = vc.LEDGER["sky_kernel"]
    case = (0, 16, 5)
    scene, m64, dirs = sky_cases.model(m, *case)
    m32 = sky_cases.model(m, *case, dtype=np.float32)[1]
    with Trace(m) as tr:
        res = m.SceneResources(ctx.device, scene, m.Format.R32G32B32A32_SFLOAT, want_prim=True, want_depth=True)
        res.render()
        out = res.read()
        res.destroy()
    if ctx.launched(row, tr.names):
        ties = m.ibl.tie_mask(dirs)
        e32, gpu = ibl_cases.rel_err(m32[~ties], m64[~ties]), ibl_cases.rel_err(out["color"][~ties], m64[~ties])
        print(f"LEDGER sky_kernel: E32 {e32:.3e} bound {ibl_cases.bound_for(e32):.3e} GPU {gpu:.3e}")
        assert ties.sum() <= 1e-3 * ties.size and gpu <= ibl_cases.bound_for(e32)
        assert (out["prim"] == 0).all() and (out["depth"] == np.float32(1.0)).all()
    row = vc.LEDGER["sky_kernel_seamless"]
    with Trace(m) as tr:
        test_sky_against_the_seamless_model(m, ctx.device, "corner", 4)
    ctx.launched(row, tr.names)
    ctx.done()


def test_transfer_rows(ctx):
    import test_gpu_transfer as tt
    import transfer_cases as tc
    calls = {"transfer_copy_kernel": (tt.test_copy_buffer_sizes_and_offsets, ()),
             "transfer_blit_kernel<0>": (tt.test_nearest_rescale_takes_the_models_texels, (37, 29)),
             "transfer_blit_kernel<1>": (tt.test_linear_into_a_float_destination, ("37x29", tt.WHOLE_SRC, tt.WHOLE_DST)),
             "transfer_fill_kernel": (tt.test_clear_color_image, (tc.RGBA32F,))}
    for name, (fn, args) in calls.items():
        rig = tt.Rig(ctx.mirhi, ctx.device)
        try:
            with Trace(ctx.mirhi) as tr:
                fn(rig, *args)
        finally:
            rig.destroy()
        ctx.launched(vc.LEDGER[name], tr.names, f" by {fn.__name__}")
    ctx.done()


# ---- both dispatch paths -------------------------------------------------------------------------------------------------------------------------
DISPATCH_ROWS = [vc.plain_name(1, 0, 1, 1, False), vc.plain_name(4, 1, 1, 1, True), vc.own_name("raster_kernel_depth", 1, 1), vc.own_name("raster_kernel_shadow", 0, 1, True),
                 vc.own_name("raster_kernel_csm", 1, 0), vc.own_name("raster_kernel_csm_blend", 0, 1), vc.ibl_name(1, 1, 2), vc.ibl_name(0, 1, 3, True, True),
                 "raster_kernel_wide<4, 0, 16>", "raster_kernel_msaa<3, 1>", "ordered_kernel<2>", vc.plain_name(3, 2, 0, 1, False)]


@pytest.mark.parametrize("name", DISPATCH_ROWS)
def test_rows_on_both_dispatch_paths(ctx, name):
    """The launch record sits in front of both paths: the row as native packets (the device's own path) and as HIP launches (timed dispatches go out as
    such), the same kernel in both records and the same bits in both frames."""
    row = vc.LEDGER[name]
    scene = scene_of(row, "overdraw")
    plain, names = render(ctx, row, scene)
    ctx.device.set_profiling(ctx.mirhi.Profile.TIMING)
    try:
        hip, hip_names = render(ctx, row, scene)
    finally:
        ctx.device.set_profiling(0)
        ctx.device.reset_kernel_times()
    print(f"LEDGER {name}: {ctx.device.dispatch_path()} and HIP launches")
    assert name in names and name in hip_names, (names, hip_names)
    ctx.same(row, "HIP launches against the device's own dispatch path", hip, plain)
    ctx.done()


# ---- the ledger is the tables ----------------------------------------------------------------------------------------------------------------------
def table_names(mirhi):
    fn = C.CDLL(mirhi.LIB_PATH).mirhi_debug_raster_table
    fn.restype, fn.argtypes = C.c_int, [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32]
    out = []
    for table in range(3):
        row, buf = 0, C.create_string_buffer(128)
        while fn(table, row, buf, len(buf)) == 0:
            out.append(buf.value.decode())
            row += 1
    return out


def test_every_table_row_was_launched(mirhi):
    """The union of the launch records of the tests above is the three tables.  Run alone, or with tests deselected, it fails: the set is then smaller."""
    names = table_names(mirhi)
    assert len(names) == len(set(names)) == 186
    reachable = {n for n in names if not vc.LEDGER[n].unreachable}
    missing = sorted(reachable - LAUNCHED)
    assert not missing, f"{len(missing)} of {len(names)} raster kernel rows were launched by no test of this file: {missing}"
    assert LAUNCHED >= reachable and {n for n in LAUNCHED if n not in names} == set(), sorted(LAUNCHED - set(names))
