#!/usr/bin/env python3
"""Time of each IBL precompute pass (mirhi_ibl_*) at the reference-like sizes, one GPU process:
  environment 512^2 from a 2048 x 1024 equirectangular image, its mip chain, irradiance 32^2, prefilter 128^2 x 5 levels x 1024
  samples, BRDF LUT 512^2.
A pass is an immediate call that has finished on the GPU when it returns, so the time is the host's clock around the call: the
kernel plus one launch and one stream wait (tens of microseconds, against passes of a millisecond and more).  Prints one JSON
object: the median over the timed repeats in milliseconds, the lookups (cube or equirect fetches of one filtered texel; a
trilinear one counts once) and samples of each pass, and the rate they imply."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

m = ge.load_package()
REPS = 9


def timed(fn):
    fn()                                            # warm-up: code object load, first touch of the outputs
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def main():
    dev = m.Device(0)
    F = m.Format.R32G32B32A32_SFLOAT
    src = m.Image(dev, 2048, 1024, F)
    src.upload(m.ibl.analytic_equirect(2048, 1024).astype(np.float32))
    env = m.Image.create_cube(dev, 512, 10)
    irr = m.Image.create_cube(dev, 32, 1)
    pre = m.Image.create_cube(dev, 128, 5)
    lut = m.Image(dev, 512, 512, F)
    # prefilter: level 0 is one lookup per texel; a rougher level keeps the samples with NdotL > 0 only (the kernel drops the rest)
    kept = 0
    for level in range(1, 5):
        a = (level / 4.0) ** 2
        xs, ys = m.ibl.hammersley(1024)
        cos2 = (1.0 - ys) / (1.0 + (a * a - 1.0) * ys)
        kept += int(np.count_nonzero(2.0 * cos2 - 1.0 > 0.0)) * 6 * (128 >> level) ** 2
    passes = [
        ("equirect_to_cube_512_from_2048x1024", lambda: env.ibl_equirect_to_cube(src), 6 * 512 * 512),
        ("cube_generate_mips_512", env.ibl_cube_generate_mips, 6 * sum((512 >> l) ** 2 for l in range(1, 10)) * 4),
        ("irradiance_32", lambda: irr.ibl_irradiance(env), 6 * 32 * 32 * 252 * 63),
        ("prefilter_128x5x1024", lambda: pre.ibl_prefilter(env, 1024), 6 * 128 * 128 + kept),
        ("brdf_lut_512", lut.ibl_brdf_lut, 512 * 512 * 1024),
    ]
    out = {"build_id": m.lib().mirhi_build_id().decode(), "device": dev.name(), "reps": REPS}
    for name, fn, work in passes:
        med, best = timed(fn)
        out[name] = {"median_ms": round(med, 4), "min_ms": round(best, 4), "lookups_or_samples": work, "per_second": round(work / (med * 1e-3), 1)}
    for o in (src, env, irr, pre, lut):
        o.destroy()
    dev.destroy()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
