"""Render areas (include/mirhi.h, mirhi_rendering_info::render_area): the areas the tests use and the two equivalences they rest on.

The oracle has no render area: it always clears, and it has a scissor per draw.  A draw in an area scope must give every pixel of the area the
bits it gives in a full-extent scope whose scissor is `scissor n area` -- same viewport, same absolute pixel coordinates, same arithmetic -- so

  E1 (CLEAR)  inside the area the expected frame is the full-extent CLEAR scope of the same scene with every scissor cut to the area (that frame
              is itself checked against the unchanged oracle); outside it is what the attachments held before, untouched.
  E2 (LOAD)   the expected frame is the full-extent LOAD scope with every scissor cut to the area, over the same prior contents: everywhere.

Comparisons are bit for bit on colour, primitive ids and stored depth: there is no tolerance to choose.  Nothing here needs a GPU or the library;
tests/test_render_area_cpu.py shows on the oracle alone that cutting the scissors does not change a pixel inside the area."""
import dataclasses

import numpy as np

TILE = 32
NO_PRIM = 0xFFFFFFFF


def areas(width, height):
    """The areas of the GPU tests for an attachment of width x height (at least 96 x 96), by the letters of the test plan."""
    assert width >= 96 and height >= 96
    gx, gy = ((width - 1) // TILE) * TILE, ((height - 1) // TILE) * TILE       # origin of the last tile column / row
    return {
        "a_aligned": (TILE, TILE, ((width - TILE) // TILE - 1) * TILE or TILE, ((height - TILE) // TILE - 1) * TILE or TILE),
        # off the tile grid on all four sides, at least 2 x 2 tiles, and past the first tile column and row: the launch's tile origin is (1, 1)
        "b_unaligned": (TILE + 19, TILE + 13, width - (TILE + 19) - 23, height - (TILE + 13) - 17),
        "c_in_one_tile": (TILE + 9, TILE + 11, 7, 5),
        "d_corner_2x2": (2 * TILE - 1, 2 * TILE - 1, 2, 2),                    # one pixel of each of four tiles
        "e_one_pixel": (width // 2, height // 2, 1, 1),
        "f_column": (width // 3, 0, 1, height),
        "g_bottom_right": (gx - 20, gy - 9, width - (gx - 20), height - (gy - 9)),      # ends in the last tile column and row (partial when the extent is no multiple of 32)
        "h_full": (0, 0, width, height),
    }


def intersect(scissor, area, width, height):
    """scissor n area as (x, y, w, h); (x, y, 0, 0) when they do not meet.  scissor None: the full extent."""
    sx, sy, sw, sh = scissor or (0, 0, width, height)
    ax, ay, aw, ah = area
    x0, y0 = max(sx, ax), max(sy, ay)
    x1, y1 = min(sx + sw, ax + aw), min(sy + sh, ay + ah)
    if x1 <= x0 or y1 <= y0:
        return (ax, ay, 0, 0)
    return (x0, y0, x1 - x0, y1 - y0)


def cut_to_area(scene, area, name=None):
    """The yardstick's scene: `scene` with every draw's (and the sky's) scissor replaced by scissor n area, and no render area."""
    draws = [dataclasses.replace(d, scissor=intersect(d.scissor, area, scene.width, scene.height)) for d in scene.draws]
    out = dataclasses.replace(scene, draws=draws, name=name or scene.name)
    if getattr(scene, "sky", None) is not None:
        out.sky = dataclasses.replace(scene.sky, scissor=intersect(scene.sky.scissor, area, scene.width, scene.height))
    if hasattr(out, "render_area"):
        out.render_area = None
    return out


def in_area(scene, area):
    """Scene with the render area set (scissors as they are)."""
    return dataclasses.replace(scene, render_area=tuple(int(v) for v in area))


def mask(area, width, height):
    m = np.zeros((height, width), dtype=bool)
    x, y, w, h = area
    m[y:y + h, x:x + w] = True
    return m


def sentinels(width, height, seed=1):
    """Per-pixel contents to prefill attachments with: no two neighbours alike, depth in [0, 1], ids no draw produces."""
    rng = np.random.default_rng(seed)
    return {
        "float": rng.uniform(0.0, 1.0, (height, width, 4)).astype(np.float32),
        "srgb8": rng.integers(0, 256, (height, width, 4), dtype=np.uint8),
        "depth": rng.uniform(0.0, 1.0, (height, width)).astype(np.float32),
        "prim": (0x40000000 + np.arange(width * height, dtype=np.uint32)).reshape(height, width),
    }


def compose(inside, outside, area):
    """`inside` within the area, `outside` elsewhere."""
    m = mask(area, inside.shape[1], inside.shape[0])
    out = outside.copy()
    out[m] = inside[m]
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
