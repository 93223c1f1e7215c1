"""The two bin sets of a command buffer's workspace ("Bin sets"): the scopes' own bins and the view slots' of its multiview scopes -- with the
view slices GROWING and MOVING on a live command buffer, with BOTH sets used by one recording, and with the statistics pass behind a multiview scope.  Every
case runs under MIRHI_VERIFY_IDLE=1 (each re-recording checks that the frame before left both sets re-armed), on the HIP launch path and, where the device
offers it, on the native one; what is rendered is compared bit for bit with the same scopes in command buffers of their own (multiview_cases states the
equivalence), and the workspace's size after every plan with what the commit before the bin sets gave (tests/golden/binset_workspace_bytes_parent.json)."""
import json
import os

import numpy as np
import pytest

import multiview_cases as mc
from test_gpu_shadow import _casters

pytestmark = pytest.mark.gpu

SIZE = 64
VIEWS = 6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binset_workspace_bytes_parent.json")

# (a) the frames of the growing loop: (view mask, map size, caster set).  Slot count, tiles and counter words grow at frame 1, the vertex output and the slot count
# at frame 3; frames 2 and 4 find slices wider than they need.
GROWING = [(0b000100, 32, "one"), (0b101101, 64, "one"), (0b100010, 32, "one"), (0b111111, 64, "two"), (0b011110, 64, "one")]


def caster_sets(scenes):
    """The casters of test_gpu_shadow; twice of them (the second copy moved aside); and with a triangle far larger than a map under them (the big list)."""
    ls, casters = _casters(scenes)
    moved = []
    for v, i, m in casters:
        m2 = np.array(m, dtype=np.float32).copy()
        m2[3, 0] += np.float32(0.7); m2[3, 2] -= np.float32(0.5)
        moved.append((v, i, m2))
    ground = np.zeros((3, 12), dtype=np.float32)
    ground[:, 0:3] = [[-200.0, -1.2, -200.0], [200.0, -1.2, -200.0], [0.0, -1.2, 300.0]]
    return ls, {"one": casters, "two": casters + moved, "ground": casters + [(ground, np.arange(3, dtype=np.uint32), np.eye(4, dtype=np.float32))]}


@pytest.fixture(scope="module")
def singles(mirhi, scenes, device):
    return single_view_layers(mirhi, scenes, device)


def single_view_layers(mirhi, scenes, device):
    """The right-hand side of the equivalence, once: every view of every (caster set, size) the cases use as single-view scopes, all layers."""
    ls, sets = caster_sets(scenes)
    mats = mc.view_matrices(ls, VIEWS)
    pipe = mc.shadow_pipeline(mirhi, scenes, device)
    out = {}
    for name, size in (("one", 32), ("one", 64), ("two", 64), ("ground", 64)):
        bufs = mc.CasterBuffers(mirhi, device, sets[name])
        out[name, size] = mc.run_single(mirhi, scenes, device, bufs, mats, (1 << VIEWS) - 1, mc.sentinels(VIEWS, size), pipe)
        out[name, size].setflags(write=False)
        bufs.destroy()
    pipe.destroy()
    assert not np.array_equal(out["one", 64], out["two", 64]) and not np.array_equal(out["one", 64], out["ground", 64])
    return out


def expected(singles, name, size, mask):
    want = mc.sentinels(VIEWS, size)
    for v in range(VIEWS):
        if (mask >> v) & 1:
            want[v] = singles[name, size][v]
    return want


class Bench:
    """A device of its own on one dispatch path, with the caster sets, the view constants and a SHADOW pipeline on it."""

    def __init__(self, mirhi, scenes, native):
        self.mirhi, self.scenes = mirhi, scenes
        self.dev = mirhi.Device(0, stream=0)
        self.dev.set_native_dispatch(native)
        self.native = native
        self.ls, sets = caster_sets(scenes)
        self.mats = mc.view_matrices(self.ls, VIEWS)
        self.pipe = mc.shadow_pipeline(mirhi, scenes, self.dev)
        self.bufs = {k: mc.CasterBuffers(mirhi, self.dev, v) for k, v in sets.items()}
        self.consts = mirhi.Buffer.new_with_data(self.dev, mirhi.BufferUsage.Uniform, mc.view_constants(self.mats, VIEWS))
        self.objs = []
        self.dispatches = self.dev.stats().native_dispatches

    def multiview(self, cmd, array, mask, name, size):
        cmd.begin_rendering_multiview(array, mask, self.consts, mc.OFFSET, mc.STRIDE)
        mc.record_draws(self.mirhi, self.scenes, cmd, self.dev, self.pipe, self.bufs[name], mc.DECOY, size, None, self.objs)
        cmd.end_rendering()

    def depth_scope(self, cmd, image, view, name, size):
        cmd.begin_rendering(None, depth=image, depth_store_op=self.mirhi.StoreOp.STORE)
        mc.record_draws(self.mirhi, self.scenes, cmd, self.dev, self.pipe, self.bufs[name], self.mats[view], size, None, self.objs)
        cmd.end_rendering()

    def planned(self, bytes_seen):
        """Right behind an end(): the workspace the plan just built stands on, and the status of everything submitted so far."""
        s = self.dev.stats()
        assert s.last_status == 0, f"device status {s.last_status:#x}: a pool or the big list ran out, the sizes below are not the requested ones"
        bytes_seen.append(int(s.workspace_bytes))

    def check_path(self):
        s = self.dev.stats()
        assert s.last_status == 0, f"device status {s.last_status:#x}"
        assert (s.native_dispatches - self.dispatches > 0) == self.native, (self.native, s.native_dispatches - self.dispatches, self.dev.dispatch_path())

    def close(self):
        for o in self.objs + [self.consts, self.pipe]:
            o.destroy()
        for b in self.bufs.values():
            b.destroy()
        self.dev.destroy()


def dispatch_paths(mirhi):
    """False (HIP launches) and, where this device offers native dispatch, True."""
    dev = mirhi.Device(0, stream=0)
    try:
        dev.set_native_dispatch(True)
        return [False, True] if dev.dispatch_path().startswith("native") and os.environ.get("MIRHI_NATIVE_DISPATCH") != "0" else [False]
    finally:
        dev.destroy()


def golden(case, got, paths):
    print(f"workspace bytes, {case}: {got}")
    want = json.load(open(GOLDEN))
    for native in paths:
        assert got[native] == want[case], f"{case} ({'native' if native else 'hip'}): the workspace is not the size the parent commit ({want['parent']}) gives, step by step"


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------------
def run_growing(mirhi, scenes, singles, native):
    """One command buffer re-recorded frame by frame with GROWING; returns the workspace's bytes behind every end()."""
    b = Bench(mirhi, scenes, native)
    sizes = []
    try:
        arrays = {size: mirhi.Image.array(b.dev, size, size, VIEWS, mirhi.Format.D32_SFLOAT) for size in (32, 64)}
        cmd = mirhi.CommandBuffer(b.dev)
        for f, (mask, size, name) in enumerate(GROWING):
            start = mc.sentinels(VIEWS, size)
            arrays[size].upload(start)
            cmd.reset()
            cmd.begin()
            b.multiview(cmd, arrays[size], mask, name, size)
            cmd.end()
            b.planned(sizes)
            b.dev.submit([cmd])
            b.dev.wait_idle()
            mc.assert_equivalent(arrays[size].read(), expected(singles, name, size, mask), start, mask, f"frame {f}")
        b.check_path()
        cmd.destroy()
        for a in arrays.values():
            a.destroy()
    finally:
        b.close()
    return sizes


def test_view_slices_grow_and_move_on_a_live_command_buffer(mirhi, scenes, singles, monkeypatch):
    monkeypatch.setenv("MIRHI_VERIFY_IDLE", "1")
    paths = dispatch_paths(mirhi)
    golden("growing", {native: run_growing(mirhi, scenes, singles, native) for native in paths}, paths)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------------
MASKS = [(0b1011, 0b0110), (0b0101, 0b1111)]      # the two multiview scopes' masks: as first recorded, as re-recorded


def colour_scene(scenes):
    return scenes.random_triangles(40, SIZE, SIZE, seed=9, rmin=4, rmax=24)


def run_both_sets(mirhi, scenes, singles, native):
    """Two command buffers (two frames in flight), each: a depth scope, a multiview scope, a colour scope, a second multiview scope.  Three submits of the
    recording, then a re-recording with other masks and a submit.  Returns the workspace's bytes behind every end()."""
    b = Bench(mirhi, scenes, native)
    M = mirhi
    sizes = []
    try:
        scene = colour_scene(scenes)
        alone = M.SceneResources(b.dev, scene, M.Format.R32G32B32A32_SFLOAT)      # the colour scope in a command buffer of its own
        alone.render()
        colour_ref = alone.read()["color"].copy()
        alone.destroy()
        depth_ref = singles["ground", SIZE][1]
        slots = []
        for k in range(2):
            res = M.SceneResources(b.dev, scene, M.Format.R32G32B32A32_SFLOAT)
            slots.append(dict(res=res, cmd=M.CommandBuffer(b.dev), fence=M.Fence(b.dev, signaled=True), depth=M.Image(b.dev, SIZE, SIZE, M.Format.D32_SFLOAT),
                              arrays=[M.Image.array(b.dev, SIZE, SIZE, VIEWS, M.Format.D32_SFLOAT) for _ in range(2)], masks=None))
        start = mc.sentinels(VIEWS, SIZE)

        def record(s, masks):
            s["cmd"].reset()
            s["cmd"].begin_reusable()
            b.depth_scope(s["cmd"], s["depth"], 1, "ground", SIZE)
            b.multiview(s["cmd"], s["arrays"][0], masks[0], "ground", SIZE)
            s["res"].record_scopes(s["cmd"])
            b.multiview(s["cmd"], s["arrays"][1], masks[1], "one", SIZE)
            s["cmd"].end()
            s["masks"] = masks
            b.planned(sizes)

        def clobber(s):
            s["depth"].upload(start[0])
            s["res"].color.upload(np.full((SIZE, SIZE, 4), 0.25, dtype=np.float32))
            for a in s["arrays"]:
                a.upload(start)

        def check(s, what):
            assert np.array_equal(s["depth"].read().view(np.uint32), depth_ref.view(np.uint32)), f"{what}: the depth scope differs from the scope alone"
            assert np.array_equal(s["res"].color.read(), colour_ref), f"{what}: the colour scope differs from the scope alone"
            for a, mask, name in zip(s["arrays"], s["masks"], ("ground", "one")):
                mc.assert_equivalent(a.read(), expected(singles, name, SIZE, mask), start, mask, f"{what}, mask {mask:#b}")

        frame = 0
        for round_ in range(4):
            for k, s in enumerate(slots):
                s["fence"].wait()
                if s["masks"] is not None:
                    check(s, f"frame {frame - 2}")
                s["fence"].reset()
                clobber(s)
                if round_ in (0, 3):
                    record(s, MASKS[0 if round_ == 0 else 1])
                b.dev.submit([s["cmd"]], s["fence"])
                frame += 1
        for k, s in enumerate(slots):
            s["fence"].wait()
            check(s, f"the last frame of slot {k}")
        b.check_path()
        for s in slots:
            s["res"].destroy()
            for o in [s["cmd"], s["fence"], s["depth"]] + s["arrays"]:
                o.destroy()
    finally:
        b.close()
    return sizes


def test_both_sets_in_one_command_buffer(mirhi, scenes, singles, monkeypatch):
    monkeypatch.setenv("MIRHI_VERIFY_IDLE", "1")
    paths = dispatch_paths(mirhi)
    golden("both_sets", {native: run_both_sets(mirhi, scenes, singles, native) for native in paths}, paths)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------------
def run_statistics(mirhi, scenes, singles, native):
    """A colour scope behind a multiview scope in one command buffer, counted (MIRHI_PROFILE_FRAGMENTS, set after the recording: a multiview scope is refused
    while it is on) over three submits -- both big-list parities of the statistics pass's parameter copies.  Returns (counts of the scope alone, counts here)."""
    b = Bench(mirhi, scenes, native)
    M = mirhi
    try:
        scene = colour_scene(scenes)
        res = M.SceneResources(b.dev, scene, M.Format.R32G32B32A32_SFLOAT)
        res.render()
        ref = res.read()["color"].copy()
        b.dev.reset_kernel_times()
        b.dev.set_profiling(M.Profile.FRAGMENTS)
        for _ in range(3):
            res.render()
        b.dev.set_profiling(0)
        alone = b.dev.fragment_stats()
        array = M.Image.array(b.dev, SIZE, SIZE, VIEWS, M.Format.D32_SFLOAT)
        start = mc.sentinels(VIEWS, SIZE)
        array.upload(start)
        cmd = M.CommandBuffer(b.dev)
        cmd.begin_reusable()
        b.multiview(cmd, array, 0b0111, "ground", SIZE)
        res.record_scopes(cmd)
        cmd.end()
        b.dev.submit([cmd])                       # (not counted: statistics are off)
        b.dev.wait_idle()
        b.dev.reset_kernel_times()
        b.dev.set_profiling(M.Profile.FRAGMENTS)
        for _ in range(3):
            res.color.upload(np.full((SIZE, SIZE, 4), 0.25, dtype=np.float32))
            b.dev.submit([cmd])
            b.dev.wait_idle()
            assert np.array_equal(res.color.read(), ref), "the statistics pass changed the frame"
        b.dev.set_profiling(0)
        behind = b.dev.fragment_stats()
        mc.assert_equivalent(array.read(), expected(singles, "ground", SIZE, 0b0111), start, 0b0111, "the multiview scope ahead of the counted one")
        b.check_path()
        cmd.destroy()
        res.destroy()
        array.destroy()
    finally:
        b.close()
    return alone, behind


def test_fragment_statistics_behind_a_multiview_scope(mirhi, scenes, singles, monkeypatch):
    monkeypatch.setenv("MIRHI_VERIFY_IDLE", "1")
    for native in dispatch_paths(mirhi):
        alone, behind = run_statistics(mirhi, scenes, singles, native)
        print(f"fragment statistics ({'native' if native else 'hip'}): alone {alone}, behind a multiview scope {behind}")
        assert alone[2] == 3 and alone[1] >= alone[0] > 0
        assert behind == alone, "the counts of the scope behind a multiview scope are not those of the scope alone"
