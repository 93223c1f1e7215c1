"""Shared by test_ibl_cpu.py and test_gpu_ibl.py: the inputs, the error metric and the bound of the IBL precompute checks.

The yardstick is the numpy model of renderer_rs_amd.ibl run in float64 (M64).  The same model run in float32 (M32: the same
operations in the same order, correctly rounded libm, serial sums) gives E32 = err(M32), the error a float32 evaluation of these
formulas has on these inputs -- float32 face flips at the cube's seams included.  A GPU result must stay within
max(8 * E32, 1e-4): 1e-4 is the project's colour tolerance, the factor 8 allows for the kernels' 1-ulp
hardware reciprocal / square root / logarithm and their reordered partial sums."""
import functools

import numpy as np

ENV_SIZE = 64
ENV_LEVELS = 7                                   # the full chain of a 64^2 cube
IRRADIANCE_SIZES = (8, 32)
PREFILTER_CASES = ((32, 6, 64), (16, 5, 1024))   # (size, levels, sample_count)
LUT_SIZES = (32, 64)
EQUIRECT_EXTENT = (256, 128)                     # width, height
EQUIRECT_CUBE_SIZES = (32, 64)
# every cube size whose texel centres enter a pass as N (irradiance outputs, prefilter levels, the chain test's 8 and 16)
N_SIZES = sorted({1, 2, 4, 8, 16, 32, 64} | set(IRRADIANCE_SIZES))

COLOUR_TOLERANCE = 1e-4
FACTOR = 8.0


def ibl():
    import __graft_entry__ as ge
    return ge.load_package().ibl


def err(x, m64) -> float:
    """max |X - M64| / max(|M64|, 1e-3 max|M64|) over every texel and channel of one output."""
    m64 = np.asarray(m64, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(m64.shape)
    return float(np.max(np.abs(x - m64) / np.maximum(np.abs(m64), 1e-3 * np.max(np.abs(m64)))))


def bound(e32: float) -> float:
    return max(FACTOR * e32, COLOUR_TOLERANCE)


def packed(levels) -> np.ndarray:
    """A list of levels as the [texels, 4] chain of mirhi_image_create_cube."""
    return np.concatenate([np.asarray(l).reshape(-1, 4) for l in levels], axis=0)


def both(fn, *args):
    """(M64, M32) of one model call; array arguments are converted to the precision the model runs in by the model itself."""
    return fn(*args, dtype=np.float64), fn(*args, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def environment():
    """analytic_environment(64) with its full chain, as float32 -- what is uploaded, and what both models read."""
    m = ibl()
    level0 = m.analytic_environment(ENV_SIZE).astype(np.float32)
    return [l for l in m.cube_mips(level0, ENV_LEVELS, dtype=np.float32)]


@functools.lru_cache(maxsize=None)
def equirect():
    w, h = EQUIRECT_EXTENT
    return ibl().analytic_equirect(w, h).astype(np.float32)


@functools.lru_cache(maxsize=None)
def irradiance_models(size: int):
    return both(ibl().irradiance, environment(), size)


@functools.lru_cache(maxsize=None)
def prefilter_models(size: int, levels: int, samples: int):
    return both(ibl().prefilter, environment(), size, levels, samples)


@functools.lru_cache(maxsize=None)
def lut_models(size: int):
    return both(ibl().brdf_lut, size)


@functools.lru_cache(maxsize=None)
def equirect_models(size: int):
    return both(ibl().equirect_to_cube, equirect(), size)
