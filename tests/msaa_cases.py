"""4x MSAA (include/mirhi.h "4x MSAA"): the cases the tests use and the equivalence they rest on.

THE EQUIVALENCE.  Sample s of a multisampled frame is the 1x frame of the same scene with every viewport moved by (1/2 - sx, 1/2 - sy) and the scissors
unchanged (scenes.msaa_sample_scene): a pixel centre of the moved frame sits where sample s of that pixel sat.  It holds bit for bit in the winner id and
the depth bits of every pixel under ONE CONDITION: under the moved viewport every vertex must snap to its unmoved (X, Y) plus (128 - 256 sx, 128 - 256 sy)
-- then every edge function, every block mask and the depth plane's three terms are the unmoved ones, and the 1x centre test IS the sample test.
condition_holds() states that in numpy (binary32 viewport transform, round-half-even snap) and checks it for every vertex of every case, the vertices a
near-plane clip makes included; no vertex and no pixel is left out.

The inputs are chosen so that it holds: TRIANGLE-program vertices (w = 1, a power of two) whose window coordinates lie on the 1/256-pixel grid of a 256 x 256
viewport (clip = (window - 128) / 128 is then exact in binary32, as tests/test_gpu_depth_state.py builds its scenes), depths on a dyadic grid.  With such
inputs every quantity of coverage and depth is exact, so the float64 model (scenes.msaa_model) and the unchanged oracle agree bit for bit too -- which
tests/test_msaa_cpu.py shows on the CPU, for the oracle alone.

The targets are 64 x 64 (2 x 2 tiles) and 96 x 80 (3 x 3 tiles, the last row of tiles partial)."""
import numpy as np

VP = 256.0
VIEWPORT = (0.0, 0.0, VP, VP, 0.0, 1.0)
NONE = 0xFFFFFFFF
SUB = 1.0 / 256.0
# sample positions in 1/256 px (the table of include/mirhi.h)
SAMPLES_256 = ((96, 32), (224, 96), (32, 160), (160, 224))
CLEAR = (0.125, 0.25, 0.5, 1.0)


def clip_of(pts):
    """(window x, window y, depth) -> clip-space position of a w = 1 vertex under VIEWPORT"""
    return [((x - VP / 2) / (VP / 2), (y - VP / 2) / (VP / 2), z) for x, y, z in pts]


def draw(scenes, pts, cols=None, **kw):
    """A TRIANGLE-program draw of the triangles whose vertices are `pts` (window x, window y, depth), cull none, under VIEWPORT"""
    kw.setdefault("cull_mode", scenes.CULL_NONE)
    return scenes.DrawSpec(vertices=scenes._tri_verts(clip_of(pts), cols), stride=24, count=len(pts), viewport=VIEWPORT, **kw)


def quad(x0, y0, x1, y1, z):
    return [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y0, z), (x1, y1, z), (x0, y1, z)]


def random_triangles(n, w, h, seed, centre=None, spread=None, flat_depth_every=3):
    """n seeded triangles on the 1/16-pixel grid, depths on the 1/64 grid (every third one flat, so that depth ties between primitives occur), vertex colours
    on the 1/8 grid.  Geometry alone decides what is kept: extent at most 28 px and twice the area at least 16 px^2 -- the bound under which the binary32
    barycentrics of an extrapolated centre (shade_triangle_program: products below 2^10 px^2, each rounded to 2^-14) stay within 1e-5 of the float64 ones."""
    rng = np.random.default_rng(seed)
    pts, cols = [], []
    while len(pts) < 3 * n:
        c = np.array(centre if centre is not None else (rng.uniform(0, w), rng.uniform(0, h)))
        r = spread if spread is not None else 14.0
        p = np.round((c + rng.uniform(-r, r, (3, 2))) * 16.0) / 16.0
        a2 = abs((p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[2, 0] - p[0, 0]) * (p[1, 1] - p[0, 1]))
        if a2 < 16.0 or (p.max(axis=0) - p.min(axis=0)).max() > 28.0:
            continue
        k = len(pts) // 3
        z = np.round(rng.uniform(0.05, 0.95, 3) * 64.0) / 64.0
        if k % flat_depth_every == 0:
            z[:] = (8 + 8 * (k // flat_depth_every % 6)) / 64.0
        pts += [(float(p[i, 0]), float(p[i, 1]), float(z[i])) for i in range(3)]
        cols += [list(np.round(rng.uniform(0, 1, 3) * 8.0) / 8.0) for _ in range(3)]
    return pts, cols


def _scene(scenes, name, w, h, draws, **kw):
    kw.setdefault("clear_color", CLEAR)
    return scenes.Scene("msaa-" + name, w, h, draws if isinstance(draws, list) else [draws], **kw)


def _random(scenes, op, clear_depth):
    pts, cols = random_triangles(200, 96, 80, 0x5A4D0001)
    return _scene(scenes, f"random-op{op}", 96, 80, draw(scenes, pts, cols, depth_compare=op), clear_depth=clear_depth)


def _slivers(scenes):
    """Four rows of slivers 8/256 px thin, row k around the y of sample k: each covers exactly sample k of pixels 3 .. 59 of its row and no centre -- the 1x frame
    shows nothing.  Then four columns likewise around the samples' x.  Flat colours (an extrapolated centre of a sliver is far outside it)."""
    pts, cols = [], []
    for k, (sx, sy) in enumerate(SAMPLES_256):
        y = 5 + 7 * k + sy * SUB
        pts += quad(3.0, y - 4 * SUB, 60.0, y + 4 * SUB, 0.25 + 0.125 * k)
        x = 6 + 9 * k + sx * SUB
        pts += quad(x - 4 * SUB, 33.0, x + 4 * SUB, 62.0, 0.25 + 0.125 * k)
    for k in range(len(pts) // 6):
        cols += [[0.25 + 0.125 * (k % 4), 1.0 - 0.125 * k, 0.5]] * 6
    return _scene(scenes, "slivers", 64, 64, draw(scenes, pts, cols))


def _sample_edges(scenes):
    """Edges that pass exactly through sample positions: an axis-aligned quad whose left / top edges lie on sample 0's x / y and whose right / bottom edges lie on
    them again 10 px further (top-left rule: the first are in, the second out), the same on sample 3, and two triangles whose slanted edge runs through
    sample 0 and sample 1 of a pixel diagonal (slope 1/2: (96, 32) -> (224, 96))."""
    pts = []
    for k, (sx, sy) in ((0, SAMPLES_256[0]), (3, SAMPLES_256[3])):
        x0, y0 = 4 + 20 * (k % 2) + sx * SUB, 4 + sy * SUB
        pts += quad(x0, y0, x0 + 10.0, y0 + 10.0, 0.5)
    ax, ay = 8 + 96 * SUB, 30 + 32 * SUB                       # sample 0 of pixel (8, 30); + (k/2, k/4) px: samples 0 / 1 of the pixels on the line
    bx, by = ax + 32.0, ay + 16.0
    pts += [(ax, ay, 0.5), (bx, by, 0.5), (ax, by, 0.5)]       # below the line
    pts += [(ax, ay, 0.25), (bx, ay, 0.25), (bx, by, 0.25)]    # above it: the shared edge belongs to exactly one of the two
    return _scene(scenes, "sample-edges", 64, 64, draw(scenes, pts))


def _tile_corner(scenes):
    """A vertex on the corner of four tiles, edges on 8 x 8 block borders and on tile borders"""
    pts = [(32, 32, 0.5), (52, 32, 0.5), (32, 52, 0.5), (32, 32, 0.25), (12, 32, 0.25), (32, 12, 0.25),
           (32, 32, 0.75), (32, 10, 0.75), (54, 32, 0.75), (32, 32, 0.375), (32, 54, 0.375), (10, 32, 0.375)]
    pts += quad(8, 40, 24, 56, 0.5) + quad(40, 8, 48, 24, 0.625) + quad(56, 56, 64, 64, 0.5)
    return _scene(scenes, "tile-corner", 64, 64, draw(scenes, pts))


def _full_tile(scenes, n):
    """n small triangles inside tile (1, 1) of a 96 x 80 target: around the 64-lane group, around a staging pass of 192 records, beyond the tile's fixed page"""
    pts, cols = random_triangles(n, 96, 80, 0x5A4D0100 + n, centre=(48.0, 48.0), spread=9.0)
    return _scene(scenes, f"full-tile-{n}", 96, 80, draw(scenes, pts, cols))


def _big_list(scenes):
    """A triangle whose vertices lie more than 255 px apart is not binned (a bin record is 16-bit relative): the big list, which every tile walks; with
    two binned triangles in front of and behind it"""
    pts = [(-120.0, -40.0, 0.5), (190.0, 20.0, 0.5), (-60.0, 170.0, 0.5), (10, 10, 0.25), (40, 12, 0.25), (12, 44, 0.25), (50, 40, 0.75), (90, 44, 0.75), (60, 76, 0.75)]
    return _scene(scenes, "big-list", 96, 80, draw(scenes, pts))


def _near_clip(scenes):
    """A triangle that crosses the near plane: depths -0.25 and 0.75 put the cut at t = 1/4 of each crossing edge, dyadic like the vertices"""
    pts = [(8.0, 8.0, -0.25), (72.0, 8.0, 0.75), (8.0, 72.0, 0.75), (20, 50, 0.5), (80, 40, 0.5), (50, 78, 0.5)]
    return _scene(scenes, "near-clip", 96, 80, draw(scenes, pts))


def _scissor(scenes):
    pts, cols = random_triangles(60, 96, 80, 0x5A4D0002)
    return _scene(scenes, "scissor", 96, 80, draw(scenes, pts, cols, scissor=(10, 7, 50, 40)))


# the biased and clamped draw: depth plane -0.5 + (x - 8) / 64 (exact in binary32 at every sample: multiples of 2^-14 below 4), constant bias 2^20 units
RAMP = [(8.0, 8.0, -0.5), (136.0, 8.0, 1.5), (8.0, 72.0, -0.5)]
BIAS = (float(2 ** 20), 0.0, 0.0)


def _biased(scenes, flat=False):
    """flat=True: the same triangle at depth 1/2 without the two states -- the scene the oracle (which has neither state) gives the COVERAGE of; the depths
    of the real one are the closed form biased_depth()"""
    pts = [(x, y, 0.5) for x, y, _ in RAMP] if flat else RAMP
    kw = {} if flat else dict(depth_bias=BIAS, depth_clamp=True)
    return _scene(scenes, "biased-clamped", 96, 80, draw(scenes, pts, **kw))


def biased_depth(w=96, h=80):
    """[h, w, 4] binary32: clamp(-0.5 + (x_s - 8) / 64 + 2^20 r, 0, 1) at every sample, r = 2^(e - 23) with e the exponent of the largest |z| of the vertices
    (1.5: e = 0).  Every operation is exact on these inputs."""
    out = np.empty((h, w, 4), dtype=np.float64)
    for s, (sx, _) in enumerate(SAMPLES_256):
        x = np.arange(w, dtype=np.float64)[None, :] + sx * SUB
        out[:, :, s] = np.clip(-0.5 + (x - 8.0) / 64.0 + 2.0 ** 20 * 2.0 ** -23, 0.0, 1.0)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)
    return out.astype(np.float32)


def cases(scenes):
    """name -> scene, in the order the tests walk them.  Visibility (winner per sample, sample-0 depth) of every one is checked against the four moved-viewport
    oracle frames; 'biased-clamped' against the oracle's coverage of its flat twin and the closed form."""
    S = scenes
    out = {
        "random-less": _random(S, S.CMP_LESS, 1.0), "random-lequal": _random(S, S.CMP_LESS_OR_EQUAL, 1.0),
        "random-greater": _random(S, S.CMP_GREATER, 0.0), "random-gequal": _random(S, S.CMP_GREATER_OR_EQUAL, 0.0),
        "slivers": _slivers(S), "sample-edges": _sample_edges(S), "tile-corner": _tile_corner(S),
        "full-tile-65": _full_tile(S, 65), "full-tile-193": _full_tile(S, 193), "full-tile-300": _full_tile(S, 300),
        "big-list": _big_list(S), "near-clip": _near_clip(S), "scissor": _scissor(S), "biased-clamped": _biased(S),
    }
    return out


def oracle_scene(scenes, name, scene):
    """the scene whose moved-viewport oracle frames give the case's winners"""
    return _biased(scenes, flat=True) if name == "biased-clamped" else scene


# ---- the condition --------------------------------------------------------------------------------------------------------------------------------
def _near_clipped(v):
    """v: [3, 3] binary32 clip-space (x, y, z) of a w = 1 triangle -> the vertices the near plane (z >= 0) leaves, by the geometry stage's rule
    (t = da / (da - db), p + t (q - p), every operation in binary32)"""
    f = np.float32
    out = []
    for i in range(3):
        a, b = v[i], v[(i + 1) % 3]
        ina, inb = a[2] >= 0, b[2] >= 0
        if ina:
            out.append(a)
        if ina != inb:
            p, q = (a, b) if ina else (b, a)
            t = f(p[2]) / f(f(p[2]) - f(q[2]))
            out.append(np.array([f(p[k] + f(t * f(q[k] - p[k]))) for k in range(3)], dtype=f))
    return out


def condition_holds(scenes, scene):
    """(vertices checked, vertices that fail): every vertex of every draw of `scene`, after the near-plane clip, snaps under each of the four moved viewports to
    its unmoved snapped position plus (128 - 256 sx, 128 - 256 sy)"""
    f = np.float32
    checked = failed = 0
    for d in scene.draws:
        v = np.ascontiguousarray(d.vertices).view(np.uint8).reshape(-1, d.stride)[:, :12].copy().view(f).reshape(-1, 3)
        idx = np.arange(d.first, d.first + d.count) if d.indices is None else np.asarray(d.indices)[d.first:d.first + d.count] + d.vertex_offset
        x, y, w, h, _, _ = d.viewport or (0.0, 0.0, float(scene.width), float(scene.height), 0.0, 1.0)
        for t in range(d.count // 3):
            tri = v[idx[3 * t:3 * t + 3]]
            verts = tri if (d.depth_clamp or (tri[:, 2] >= 0).all()) else _near_clipped(tri)
            for p in verts:
                def snap(vx, vy):
                    hw, hh = f(0.5) * f(w), f(0.5) * f(h)
                    xs = f(f(f(p[0]) * hw) + f(f(vx) + hw))
                    ys = f(f(f(p[1]) * hh) + f(f(vy) + hh))
                    return int(np.rint(np.float64(xs) * 256.0)), int(np.rint(np.float64(ys) * 256.0))
                X0, Y0 = snap(x, y)
                checked += 1
                for sx, sy in SAMPLES_256:
                    Xs, Ys = snap(x + (0.5 - sx * SUB), y + (0.5 - sy * SUB))
                    if (Xs, Ys) != (X0 + 128 - sx, Y0 + 128 - sy):
                        failed += 1
                        break
    return checked, failed


def oracle_samples(scenes, oracle, scene):
    """prim [H, W, 4] and depth [H, W, 4] of the four moved-viewport oracle frames, and the 1x frame"""
    frames = [oracle.render(scenes.msaa_sample_scene(scene, s), want_bgra8=False) for s in range(4)]
    return (np.stack([fr["prim"] for fr in frames], axis=2), np.stack([fr["depth"] for fr in frames], axis=2), oracle.render(scene, want_bgra8=False))

