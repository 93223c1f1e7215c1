#!/usr/bin/env python3
"""Times of the Radiance .hdr path for a 4096 x 2048 and a 2048 x 1024 source, one GPU process; the median of nine runs of each:
  the host decode (images.decode_hdr) of a new-style RLE file and of a flat one;
  Image.upload of the RGBE bytes against Image.upload of the float form (pageable host memory, as a caller has it);
  expand_rgbe against a torch copy that moves the same total byte count (5/4 of the float image: the copy reads and writes 10 bytes per texel);
  ibl_equirect_to_cube_rgbe into a 512^2 cube against ibl_equirect_to_cube from the float image, interleaved.
Every device call has finished on the GPU when it returns, so a time is the host's clock around the call: the kernel (or copy) plus one launch and
one stream wait.  The kernels here run for tens of microseconds, which that overhead rivals: the call times say what a caller waits for, and the kernels'
own durations -- what the achieved bandwidth is computed from -- come from a kernel trace of this tool (rocprofv3 --kernel-trace --stats -- python
tools/hdr_times.py), in a run of its own.  Prints one JSON object; times in milliseconds.

The source is analytic_equirect at 512 x 256 through the tests' RGBE encoder, tiled to the extent: the decoder's and the kernels' work does not
depend on what the texels hold beyond the runs of the RLE file (smooth rows: few runs, mostly literals)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

m = ge.load_package()
from renderer_rs_amd import images  # noqa: E402
import hdr_cases  # noqa: E402

REPS = 9


def timed(fn):
    fn()                                            # warm-up: code object load, first touch of the outputs
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4)}


def timed_interleaved(a, b):
    a(); b()
    ta, tb = [], []
    for _ in range(REPS):
        t0 = time.perf_counter(); a(); t1 = time.perf_counter(); b(); t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3); tb.append((t2 - t1) * 1e3)
    return ({"median_ms": round(statistics.median(ta), 4), "min_ms": round(min(ta), 4)},
            {"median_ms": round(statistics.median(tb), 4), "min_ms": round(min(tb), 4)})


def main():
    import torch
    images.build()
    dev = m.Device(0)
    F32, RGBA8 = m.Format.R32G32B32A32_SFLOAT, m.Format.R8G8B8A8_UNORM
    out = {"build_id": m.lib().mirhi_build_id().decode(), "device": dev.name(), "reps": REPS}
    tile = hdr_cases.rgbe_from_float(np.maximum(m.ibl.analytic_equirect(512, 256), 0.0))
    for w, h in ((4096, 2048), (2048, 1024)):
        rgbe = np.ascontiguousarray(np.tile(tile, (h // 256, w // 512, 1)))
        texels = w * h
        rle, flat = images.encode_hdr(rgbe, rle=True), images.encode_hdr(rgbe, rle=False)
        hdr = images.decode_hdr(rle)
        assert np.array_equal(hdr.rgbe, rgbe) and np.array_equal(images.decode_hdr(flat).rgbe, rgbe)
        floats = hdr.to_float()
        r = {"rgbe_bytes": texels * 4, "float_bytes": texels * 16, "rle_file_bytes": len(rle), "flat_file_bytes": len(flat)}
        r["host_decode_rle"] = timed(lambda: images.decode_hdr(rle))
        r["host_decode_flat"] = timed(lambda: images.decode_hdr(flat))
        r["host_to_float"] = timed(hdr.to_float)
        src8, src32, dst32 = m.Image(dev, w, h, RGBA8), m.Image(dev, w, h, F32), m.Image(dev, w, h, F32)
        r["upload_rgbe"], r["upload_float"] = timed_interleaved(lambda: src8.upload(rgbe), lambda: src32.upload(floats))
        a = torch.empty(texels * 10, dtype=torch.uint8, device="cuda")
        b = torch.empty_like(a)

        def copy():
            b.copy_(a)
            torch.cuda.synchronize()
        r["expand_rgbe"], r["torch_copy_same_bytes"] = timed_interleaved(lambda: dst32.expand_rgbe(src8), copy)
        r["expand_traffic_bytes"] = texels * 20
        assert np.array_equal(dst32.read().view(np.uint32), floats.view(np.uint32))
        del a, b
        cube8, cube32 = m.Image.create_cube(dev, 512, 1), m.Image.create_cube(dev, 512, 1)
        r["equirect_to_cube_rgbe_512"], r["equirect_to_cube_float_512"] = timed_interleaved(lambda: cube8.ibl_equirect_to_cube_rgbe(src8),
                                                                                          lambda: cube32.ibl_equirect_to_cube(src32))
        assert np.array_equal(cube8.read().view(np.uint32), cube32.read().view(np.uint32))
        for o in (src8, src32, dst32, cube8, cube32):
            o.destroy()
        out[f"{w}x{h}"] = r
    dev.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
