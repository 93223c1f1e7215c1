#!/usr/bin/env python3
"""Per-dispatch device times (mirhi_device_timeline, the method of tools/shadow_times.py) of the recorded transfer commands: copy_buffer of 64 MiB,
copy_image of a 1920 x 1080 float frame, its 1:1 blit to B8G8R8A8_SRGB, its 2:1 LINEAR downscale to B8G8R8A8_SRGB, clear_color_image of a 1080p sRGB8 image.  Each as
the median of the timed dispatches and as (bytes read + bytes written) / time.  The yardsticks, in the same process: a torch device-to-device copy_
of the same byte count for the copies, Tensor.fill_ for the clear (event pairs around each call).  Prints one JSON object with the build id."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import shadow_times as st  # noqa: E402

m = st.m
W, H = 1920, 1080
F32, SRGB8 = m.Format.R32G32B32A32_SFLOAT, m.Format.B8G8R8A8_SRGB


def ours(dev, record, nbytes):
    cmd = m.CommandBuffer(dev)
    cmd.begin_reusable(); record(cmd); cmd.end()
    tl = st.timed(dev, lambda: dev.submit([cmd]))
    us = statistics.median(e - b for (_, _, b, e) in tl)
    dev.wait_idle(); cmd.destroy()
    return {"us": round(us, 2), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}


def torch_time(fn, nbytes):
    import torch
    for _ in range(4):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(st.REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    us = statistics.median(times)
    return {"us": round(us, 2), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)}


def main():
    import torch
    dev = m.Device(0)
    out = {"build_id": m.lib().mirhi_build_id().decode(), "reps": st.REPS}
    n = 64 << 20
    a, b = m.Buffer(dev, m.BufferUsage.Storage, n), m.Buffer(dev, m.BufferUsage.Storage, n)
    frame, copy, srgb, half = m.Image(dev, W, H, F32), m.Image(dev, W, H, F32), m.Image(dev, W, H, SRGB8), m.Image(dev, W // 2, H // 2, SRGB8)
    frame.upload(np.random.default_rng(0).random((H, W, 4)).astype(np.float32))
    whole, small = ((0, 0), (W, H)), ((0, 0), (W // 2, H // 2))
    out["copy_buffer_64MiB"] = ours(dev, lambda c: c.copy_buffer(a, b, [(0, 0, n)]), 2 * n)
    out["copy_image_1080p_float"] = ours(dev, lambda c: c.copy_image(frame, copy, [(0, (0, 0), 0, (0, 0), (W, H))]), 2 * W * H * 16)
    out["blit_1to1_float_to_srgb8"] = ours(dev, lambda c: c.blit_image(frame, srgb, [(0, whole, 0, whole)], m.Filter.NEAREST), W * H * 20)
    out["blit_2to1_linear_float_to_srgb8"] = ours(dev, lambda c: c.blit_image(frame, half, [(0, whole, 0, small)], m.Filter.LINEAR), W * H * 16 + W * H)
    out["clear_color_1080p_srgb8"] = ours(dev, lambda c: c.clear_color_image(srgb, (0.1, 0.2, 0.3, 1.0)), W * H * 4)
    for o in (a, b, frame, copy, srgb, half):
        o.destroy()
    dev.destroy()
    x, y = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    out["torch_copy_64MiB"] = torch_time(lambda: y.copy_(x), 2 * n)
    fx, fy = torch.empty(W * H * 16, dtype=torch.uint8, device="cuda"), torch.empty(W * H * 16, dtype=torch.uint8, device="cuda")
    out["torch_copy_1080p_float"] = torch_time(lambda: fy.copy_(fx), 2 * W * H * 16)
    z = torch.empty(W * H, dtype=torch.int32, device="cuda")
    out["torch_fill_1080p_4B"] = torch_time(lambda: z.fill_(0x01020304), W * H * 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
