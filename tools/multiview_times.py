#!/usr/bin/env python3
"""Per-dispatch device times of the cascade pass of cascaded_ground_case in its two forms, of ONE build, interleaved in one GPU process (the method of
tools/csm_times.py): four single-view depth-only scopes into the layer views of the D32 array against one multiview scope
(mirhi_cmd_begin_rendering_multiview), at 1024^2 and 2048^2 layers.  Per form: the median over the timed repeats of the summed vertex,
geometry and raster dispatch times of a frame's cascade pass, of the wall time from its first dispatch's begin to its last one's end
(mirhi_device_timeline), and the host time of recording it again (begin, the scopes, end -- the plan cache's case: an unchanged frame).
Timed dispatches go out as HIP launches with a completion signal each, so the wall times include the gaps between dependent launches of that path.
Prints one JSON object with the build id."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

m = ge.load_package()
S = m.scenes
REPS = int(os.environ.get("MULTIVIEW_TIMES_REPS", "32"))
RECORDS = 200
FORMS = (("four_scopes", False, 12), ("multiview", True, 3))       # name, SceneResources(multiview=), dispatches per cascade pass


def summarise(frames):
    """frames: per repeat the (kernel, lane, begin_us, end_us) dispatches of one cascade pass"""
    out = {}
    for k, name in ((m.Kernel.VERTEX, "vertex_us"), (m.Kernel.GEOMETRY, "geometry_us"), (m.Kernel.RASTER, "raster_us")):
        out[name] = round(statistics.median(sum(e - b for kk, _, b, e in f if kk == k) for f in frames), 2)
    out["wall_us"] = round(statistics.median(max(e for _, _, _, e in f) - min(b for _, _, b, _ in f) for f in frames), 2)
    out["dispatches"] = len(frames[0])
    return out


def record_seconds(res):
    cmd = res.shadow_cmd
    t0 = time.perf_counter()
    for _ in range(RECORDS):
        cmd.begin_reusable()
        res._record_shadow(cmd)
        cmd.end()
    return (time.perf_counter() - t0) / RECORDS


def main():
    dev = m.Device(0)
    out = {"build_id": m.lib().mirhi_build_id().decode(), "reps": REPS, "dispatch_path": dev.dispatch_path()}
    for size in (1024, 2048):
        scene = S.cascaded_ground_case(1920, 1080, map_size=size)
        res = {name: m.SceneResources(dev, scene, m.Format.B8G8R8A8_SRGB, shadow_cmd=True, multiview=mv) for name, mv, _ in FORMS}
        layers = {}
        for name, _, _ in FORMS:
            for _ in range(4):
                dev.submit([res[name].shadow_cmd])
            dev.wait_idle()
            layers[name] = res[name].cascade_array.read().copy()
        same = bool((layers["four_scopes"].view("uint32") == layers["multiview"].view("uint32")).all())
        dev.reset_kernel_times()
        dev.set_profiling(m.Profile.TIMING)
        for _ in range(REPS):
            for name, _, _ in FORMS:      # interleaved: both forms see the same clocks and neighbours
                dev.submit([res[name].shadow_cmd])
                dev.wait_idle()
        tl = dev.timeline()
        dev.set_profiling(0)
        dev.reset_kernel_times()
        per_rep = sum(n for _, _, n in FORMS)
        assert len(tl) == REPS * per_rep, (len(tl), REPS, per_rep)
        entry = {"layers_equal": same}
        at = 0
        for name, _, n in FORMS:
            frames = [tl[r * per_rep + at:r * per_rep + at + n] for r in range(REPS)]
            entry[name] = summarise(frames)
            at += n
        # untimed: the wall time of the pass as a frame loop pays it (native dispatch where the device has it), host clock around submit + wait
        for name, _, _ in FORMS:
            ts = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                dev.submit([res[name].shadow_cmd])
                dev.wait_idle()
                ts.append((time.perf_counter() - t0) * 1e6)
            entry[name]["submit_to_idle_host_us"] = round(statistics.median(ts), 2)
            entry[name]["record_host_us"] = round(record_seconds(res[name]) * 1e6, 2)
        for r in res.values():
            r.destroy()
        out[f"layers_{size}"] = entry
    dev.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
