"""bench.py's host logic that needs no GPU: the timeline summary (overlap / gap / period arithmetic), the traffic figure's build-hash
gate, the launcher command for `--gpus N`, and the refusal to report a line whose n_gpus would not be what was asked for."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

NAMES = ("geometry", "raster", "vertex", "fragment_count")


def test_timeline_summary_serial_lane():
    # two frames on one lane, strictly serial: geometry 10 us, gap 2, raster 12 us, gap 1
    tl = [(0, 0, 0.0, 10.0), (1, 0, 12.0, 24.0), (0, 0, 25.0, 35.0), (1, 0, 37.0, 49.0), (0, 0, 50.0, 60.0), (1, 0, 62.0, 74.0)]
    s = bench.summarize_timeline(tl, NAMES)
    assert s["dispatches"] == 6 and s["geometry_us"] == 10.0 and s["raster_us"] == 12.0
    assert s["raster_overlap_us"] == 0.0 and s["geometry_to_raster_gap_us"] == 2.0 and s["frame_period_us"] == 25.0


def test_timeline_summary_overlapping_lanes():
    # two lanes, raster kernels of consecutive frames overlap by 3 us; each raster pairs with the geometry of ITS lane
    tl = [(0, 0, 0.0, 5.0), (0, 1, 1.0, 6.0), (1, 0, 6.0, 16.0), (1, 1, 13.0, 23.0), (0, 0, 17.0, 22.0), (1, 0, 24.0, 34.0)]
    s = bench.summarize_timeline(tl, NAMES)
    assert s["raster_us"] == 10.0
    assert s["raster_overlap_us"] == pytest.approx((3.0 + 0.0) / 2, abs=1e-3)
    assert s["geometry_to_raster_gap_us"] == pytest.approx((1.0 + 7.0 + 2.0) / 3, abs=1e-3)
    assert bench.summarize_timeline([], NAMES) is None


def test_traffic_is_quoted_only_for_the_same_kernel_build(tmp_path, monkeypatch):
    prof = tmp_path / "profiles"
    prof.mkdir()
    (prof / "r09_c2_hbm_traffic.json").write_text(json.dumps({"kernel_source_sha16": "aaaa", "frame_hbm_bytes": 123}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    hit, note = bench.measured_traffic("c2", "aaaa")
    assert hit["frame_hbm_bytes"] == 123 and note == "r09_c2_hbm_traffic.json"
    miss, note = bench.measured_traffic("c2", "bbbb")
    assert miss is None and "not quoted" in note
    none, note = bench.measured_traffic("c5", "aaaa")
    assert none is None and "no counters" in note


def test_gpus_flag_starts_the_ranks_itself(monkeypatch):
    seen = {}
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: seen.update(cmd=cmd, env=env) or 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    args = bench.parse_args()
    assert bench.spawn_ranks(args) == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-4:] == ["--gpus", "4", "--steps", "3"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "1"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "refusing to report" in (r.stderr + r.stdout)


def test_plain_run_is_the_default_and_full_is_asked_for(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", "out"])
    args = bench.parse_args()
    assert not args.full and args.steps == 7 and args.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse_args().full
    monkeypatch.setattr(sys, "argv", ["bench.py", "--timeline-out", "t.json"])   # the timeline comes from the passes --full runs
    with pytest.raises(SystemExit):
        bench.parse_args()


class _Frame:
    def __init__(self, px):
        self.px = px

    def read(self):
        return self.px


def test_dump_writes_the_frame_as_float32(tmp_path):
    import numpy as np
    px = np.random.default_rng(1).integers(0, 256, size=(9, 13, 4), dtype=np.uint8)
    bench.dump_frame(_Frame(px), str(tmp_path / "d"))
    got = np.load(tmp_path / "d" / "color.npy")
    assert got.dtype == np.float32 and got.shape == (9, 13, 4) and np.array_equal(got, px.astype(np.float32))


def test_dump_of_a_large_frame_is_a_fixed_sample(tmp_path, monkeypatch):
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 16 * 100)            # 100 RGBA float32 pixels
    px = np.arange(40 * 30 * 4, dtype=np.float32).reshape(40, 30, 4)
    bench.dump_frame(_Frame(px), str(tmp_path / "a"))
    bench.dump_frame(_Frame(px), str(tmp_path / "b"))
    a, b = np.load(tmp_path / "a" / "color_sample.npy"), np.load(tmp_path / "b" / "color_sample.npy")
    assert not (tmp_path / "a" / "color.npy").exists()
    assert a.dtype == np.float32 and a.shape == (100, 4) and np.array_equal(a, b)
    pix = a[:, 0] / 4                                                    # pixel index of each row (the values count up)
    assert np.all(np.diff(pix) > 0) and np.array_equal(a, px.reshape(-1, 4)[pix.astype(np.int64)])
