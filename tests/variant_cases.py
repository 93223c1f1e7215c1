"""The ledger of raster kernel instantiations: one entry per row of k_raster_entries, k_raster_batch_entries and k_raster_view_entries
(csrc/mirhi_kernels.hip), keyed by the row's exact name, with the scene, depth state, knobs, render area, seamless flags and yardstick under which
tests/test_gpu_variant_ledger.py launches and checks it.  tests/test_variant_ledger_cpu.py holds the ledger against the tables and checks the
scenes' conditions on the oracle alone.

THE RULE.  Per family one ANCHOR row: the instantiation an existing test compares with a high-precision reference; the ledger test runs that
comparison on it (ANCHOR_CHECKS names it).  Every other row of the family reproduces the anchor's frame of the same scene bit for bit -- colour,
primitive ids, stored depth: one set of fragment functions, contraction off.  AREA rows: inside the area; outside it the prefilled sentinel
(render_area_cases).  Generic-key rows (K = 1): the TWIN scene (no pixel covered twice) under GREATER / clear 0 equals the K = 0 anchor's frame
under LESS / clear 1, and the OVERDRAW scene under GREATER has the oracle's GREATER winners and depth, each pixel's colour being -- bit for bit --
the colour the K = 0 anchor gives that primitive at that pixel (taken from the anchor's frames of the scene's two layers, each drawn alone: a
fragment's colour depends on its primitive and pixel, not on what else is drawn).

THE SCENES.  Targets of 100 x 100 (4 x 4 tiles, the last column and row partial: render_area_cases.areas asks for at least 96 both ways),
shadow maps of 128^2, the unaligned area of render_area_cases.areas.  One geometry for every rastered scene, in window coordinates on the
1/16-pixel grid of msaa_cases.VIEWPORT under an identity camera (so the multisample equivalence of msaa_cases holds for it too):
  layer A (the twin scene)   a quad over 3 x 4 tiles, down into the partial bottom row (two triangles that each span more than 2 x 2 tiles), and
                             72 triangles of 2.25 x 2.5 pixels inside tile (2, 1), which with the quad's two holds 74 records: past one
                             64-lane group.  Nothing overlaps.
  layer B (drawn after A's   two more quads (one into the partial right column and bottom row) and 16 small triangles over layer A, in front
  draws: the overdraw scene) of it here and behind it there, none over another of its own layer."""
import dataclasses
import functools

import numpy as np

import msaa_cases
import render_area_cases as rc

W = H = 100
MAP = 128
VIEWPORT = msaa_cases.VIEWPORT
NO_PRIM = 0xFFFFFFFF
AREA = rc.areas(W, H)["b_unaligned"]
MAP_AREA = rc.areas(MAP, MAP)["b_unaligned"]
CLEAR = (0.125, 0.25, 0.5, 1.0)
BUSY_TILE = (2, 1)


def _S():
    from renderer_rs_amd import scenes
    return scenes


# ---- the geometry ------------------------------------------------------------------------------------------------------------------------
def _quad(x0, y0, x1, y1, z00, z10, z11, z01):
    return [(x0, y0, z00), (x1, y0, z10), (x1, y1, z11), (x0, y0, z00), (x1, y1, z11), (x0, y1, z01)]


def _cells(x0, y0, nx, ny, dx, dy, depth):
    pts = []
    for j in range(ny):
        for i in range(nx):
            cx, cy, z = x0 + i * dx, y0 + j * dy, depth(j * nx + i)
            pts += [(cx + 0.25, cy + 0.25, z), (cx + 2.5, cy + 0.5, z), (cx + 0.75, cy + 2.75, z)]
    return pts


@functools.lru_cache(maxsize=None)
def layer_points(layer):
    """(big triangles, small triangles) of layer "A" / "B" as lists of (window x, window y, depth), three per triangle."""
    if layer == "A":
        return (_quad(6.5, 5.25, 70.25, 98.0, 0.375, 0.625, 0.625, 0.375),
                _cells(72.5, 34.5, 8, 9, 2.75, 3.0, lambda k: (8 + (k * 5) % 48) / 64.0))
    return (_quad(30.0, 20.5, 60.5, 70.0, 0.5, 0.5, 0.5, 0.5) + _quad(64.25, 40.0, 98.5, 99.25, 0.25, 0.25, 0.75, 0.75),
            _cells(10.0, 60.0, 4, 4, 4.0, 4.0, lambda k: 0.25 if k % 2 else 0.875))


def _clip(pts):
    return np.array(msaa_cases.clip_of(pts), dtype=np.float32)


def _v48(pts):
    """Vertex (48 B) streams of window-space points: normals tilted up to about 60 degrees off the view axis (they cross cube faces), uv = window / 16."""
    S = _S()
    win = np.array(pts, dtype=np.float64)
    n = np.stack([np.sin(win[:, 0] * 0.21), np.cos(win[:, 1] * 0.17), np.full(len(pts), -0.6)], axis=1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return S._pack_vertex48(_clip(pts), n, win[:, :2] / 16.0, np.tile(np.array([1.0, 0.0, 0.0, 1.0]), (len(pts), 1)))


def _colours(n, seed):
    return np.round(np.random.default_rng(seed).uniform(0, 1, (n, 3)) * 8.0) / 8.0


@functools.lru_cache(maxsize=None)
def _textures():
    S = _S()
    rng = np.random.default_rng(0x1ED6E2)
    albedo = rng.integers(40, 256, (16, 16, 4), dtype=np.uint8)
    albedo[..., 3] = 255
    masked = albedo.copy()
    yy, xx = np.mgrid[0:16, 0:16]
    masked[..., 3] = np.where(((xx // 3) + (yy // 2)) % 2 == 0, 255, 0).astype(np.uint8)      # about half of every quad's texels lie under the cutoff
    return S.Texture(albedo), S.Texture(masked)


def _identity_camera():
    S = _S()
    eye = np.eye(4, dtype=np.float32)
    return S.camera_ubo(eye, eye, (0.0, 0.0, -2.0))


PROGRAM_SETS = {"tri": 1, "model": 2, "mixed": 3, "pbr": 4, "masked": 4}


def _draws(kind, layer, key):
    """The draws of one layer for a scene kind: tri / model / mixed / pbr / masked / ibl, under depth state `key`."""
    S = _S()
    big, small = layer_points(layer)
    state = {"less": dict(depth_compare=S.CMP_LESS), "greater": dict(depth_compare=S.CMP_GREATER),
             "predicate": dict(depth_compare=S.CMP_LESS_OR_EQUAL, depth_write=False), "blend": dict(depth_compare=S.CMP_LESS, blend=S.ALPHA_BLEND)}[key]
    common = dict(cull_mode=S.CULL_NONE, viewport=VIEWPORT, **state)
    eye4 = np.eye(4, dtype=np.float32)

    def tri(pts, seed):
        return S.DrawSpec(vertices=S._tri_verts(_clip(pts), _colours(len(pts), seed)), stride=24, count=len(pts), program=S.PROGRAM_TRIANGLE, **common)

    def mesh(pts, program):
        albedo, masked = _textures()
        lights = dict(light=S.light_ubo(direction=(0.3, 0.2, 1.0), intensity=0.8, color=(1.0, 0.95, 0.9), num_point=1),
                      point_lights=S.point_light((-0.6, -0.5, -1.0), 6.0, (0.7, 0.8, 1.0), 3.0))
        kw = dict(vertices=_v48(pts), stride=48, count=len(pts), program=program, camera=_identity_camera(), object=S.object_ubo(eye4), **lights, **common)
        if program == S.PROGRAM_MODEL:
            return S.DrawSpec(**kw)
        cut = kind == "masked"
        material = S.pbr_material_ubo((0.9, 0.8, 0.7, 0.8), 0.3, 0.45, 0.9, emissive=(0.02, 0.01, 0.03), alpha_cutoff=0.4 if cut else 0.0, has_base_color=True)
        return S.DrawSpec(material=material, albedo_map=masked if cut else albedo, alpha_test=cut, **kw)

    seed = 11 if layer == "A" else 12
    if kind == "tri":
        return [tri(big + small, seed)]
    if kind == "mixed":
        return [mesh(big, S.PROGRAM_MODEL), tri(small, seed)]
    program = {"model": S.PROGRAM_MODEL, "pbr": S.PROGRAM_MODEL_PBR, "masked": S.PROGRAM_MODEL_PBR, "ibl": S.PROGRAM_MODEL_PBR_IBL}[kind]
    return [mesh(big + small, program)]


def layer_triangles(layer):
    big, small = layer_points(layer)
    return (len(big) + len(small)) // 3


# ---- shadow scopes of the lit families ----------------------------------------------------------------------------------------------------
def _light_matrix(scale):
    """Light clip = scale * (x, y) + (scale - 1) of the world (= the camera's clip) position, depth = z: the 100 x 100 window region fills a good part of the map."""
    m = np.eye(4, dtype=np.float32)
    m[0, 0] = m[1, 1] = np.float32(scale)
    m[3, 0] = m[3, 1] = np.float32(scale - 1.0)
    return m


def caster_points():
    """Casters in front of every receiver (depth 1/8): a quad and a dozen small triangles over layer A's quad, a quad over its small triangles."""
    return (_quad(18.0, 12.0, 47.5, 38.0, 0.125, 0.125, 0.125, 0.125) + _quad(70.0, 30.0, 84.0, 50.0, 0.125, 0.125, 0.125, 0.125)
            + _cells(12.0, 44.0, 4, 3, 11.0, 9.0, lambda k: 0.125))


def _casters(matrix, pts=None, compare=None, viewport=None, flip=True):
    """One SHADOW draw of the points; flip: into a map that is looked up with `matrix` (scenes.flip_clip_y), else as a depth image of its own."""
    S = _S()
    pts = caster_points() if pts is None else pts
    return [S.DrawSpec(vertices=_v48(pts), stride=48, count=len(pts), program=S.PROGRAM_SHADOW, cull_mode=S.CULL_NONE, viewport=viewport,
                       depth_compare=S.CMP_LESS if compare is None else compare,
                       camera=S.shadow_constants_ubo(S.flip_clip_y(matrix) if flip else matrix, np.eye(4, dtype=np.float32)))]


CASCADE_SCALES = (2.5, 2.2, 1.9, 1.6)
CASCADE_SPLITS = (0.4375, 0.53125, 0.6875, 1.0)      # the receivers' depths run from 1/4 to 7/8: every cascade is selected somewhere
BLEND_THRESHOLD = 0.3


def shadow_term(term):
    """Scene keywords of shadow term 0 (none), 1 (one map), 2 (cascades), 3 (blended cascades)."""
    S = _S()
    if term == 0:
        return {}
    if term == 1:
        m = _light_matrix(CASCADE_SCALES[0])
        return dict(shadow=S.ShadowSpec(_casters(m), (MAP, MAP), S.shadow_ubo(m, 0.005, 0.02, (MAP, MAP), 0.8)))
    mats = [_light_matrix(s) for s in CASCADE_SCALES]
    return dict(cascades=S.CascadeSpec([_casters(m) for m in mats], (MAP, MAP), S.csm_ubo(mats, CASCADE_SPLITS, 0.005, 0.01, float(MAP)),
                                       blend_threshold=BLEND_THRESHOLD if term == 3 else 0.0))


# ---- the rows -------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Row:
    name: str
    family: str               # the GPU test's parameter
    kind: str                 # the scene: tri / model / mixed / pbr / masked / ibl (rastered colour scopes), depth, views, sky, transfer
    key: str = "less"         # depth state: less (LESS, clear 1), greater (GREATER, clear 0: the generic key), predicate (LESS_OR_EQUAL without write over 0.6), blend
    tp: int = 0               # MIRHI_TP_MAX_AREA: 64 / 0 (MIRHI_TP_DENSITY is set to 0 beside it: the limit alone decides)
    teams: int = 1            # MIRHI_RASTER_TEAMS
    wide: int = 0             # MIRHI_RASTER_WIDE
    area: bool = False        # the unaligned render area
    shadow: int = 0           # shadow term of the lit families
    seamless: tuple = (False, False, False)      # irradiance cube, prefiltered cube, sky environment
    samples: int = 1
    route: str = "single"     # single / batch (two command buffers in one submit) / multiview
    anchor: str = ""          # the family's anchor row ("" for a row that is its own yardstick's subject)
    yardstick: str = ""       # what the row is held against, in words
    xfer: str = ""            # transfer rows: the command
    unreachable: str = ""     # the line of raster_variant / mirhi_scope.h that excludes the row (none does: every row can be launched)

    @property
    def knobs(self):
        return {"MIRHI_TP_MAX_AREA": str(self.tp), "MIRHI_TP_DENSITY": "0", "MIRHI_RASTER_TEAMS": str(self.teams), "MIRHI_RASTER_WIDE": str(self.wide)}


def _b(v):
    return "true" if v else "false"


def plain_name(p, k, t, teams, masked, area=False):
    return f"raster_kernel<{p}, {k}, {t}, {teams}, {_b(masked)}{', true' if area else ''}>"


def own_name(kernel, k, t, area=False):
    return f"{kernel}<{k}, {t}{', true' if area else ''}>"


def ibl_name(k, t, s, area=False, seamless=False):
    return f"raster_kernel_ibl{'_seamless' if seamless else ''}<{k}, {t}, {s}{', true' if area else ''}>"


EQUAL = "the anchor's frame of the same scene, bit for bit"
TWIN = "twin scene under GREATER = the K = 0 anchor's frame; overdraw scene: the oracle's GREATER winners and depth, the anchor's colour per primitive and pixel"
KINDS = {1: "tri", 2: "model", 3: "mixed", 4: "pbr"}


def _build():
    rows = []

    def add(name, family, kind, anchor, k=0, yardstick=None, **kw):
        if k == 1:
            kw["key"] = "greater"
        if yardstick is None:
            yardstick = "its own anchor check" if name == anchor else (TWIN if k == 1 else EQUAL)
        if kw.get("area"):
            yardstick += "; inside the area, the sentinel outside"
        rows.append(Row(name=name, family=family, kind=kind, anchor=anchor, yardstick=yardstick, **kw))

    # the plain family per program set, with its wide, two-team, AREA and batched forms; anchor: the pixel-parallel plain-key row against the oracle
    for p, kind in KINDS.items():
        fam, anchor = f"plain{p}", plain_name(p, 0, 0, 1, False)
        for k in (0, 1):
            for t in (0, 1):
                add(plain_name(p, k, t, 1, False), fam, kind, anchor, k, tp=64 * t)
                add(plain_name(p, k, t, 1, False, True), fam, kind, anchor, k, tp=64 * t, area=True)
            if p in (2, 4):
                add(plain_name(p, k, 1, 2, False), fam, kind, anchor, k, tp=64, teams=2)
                for w in (8, 16):
                    add(f"raster_kernel_wide<{p}, {k}, {w}>", fam, kind, anchor, k, tp=64, wide=w)
        for t, teams in ((1, 2), (1, 1), (0, 1)):
            if teams == 1 or p in (2, 4):
                add(f"raster_kernel_batch<{p}, 0, {t}, {teams}>", fam, kind, anchor, tp=64 * t, teams=teams, route="batch",
                    yardstick="two command buffers (overdraw and twin scene) in one submit: each frame = the anchor's single-launch frame, bit for bit")
        # predicate mode and the ordered resolve: each row against the oracle, the AREA row against its full-extent row
        pred = plain_name(p, 2, 0, 1, False)
        add(pred, "predicate", kind, pred, key="predicate", yardstick="the oracle's primitive ids and colour (test_gpu_parity._check)")
        add(plain_name(p, 2, 0, 1, False, True), "predicate", kind, pred, key="predicate", area=True, yardstick=EQUAL)
        add(f"ordered_kernel<{p}>", "ordered", kind, f"ordered_kernel<{p}>", key="blend", yardstick="the oracle's primitive ids, depth and colour (test_gpu_parity._check)")
        for k in (0, 1):
            add(f"raster_kernel_msaa<{p}, {k}>", "msaa", kind, f"raster_kernel_msaa<{p}, 0>", k, samples=4)
    anchor = plain_name(4, 0, 1, 1, True)
    for k in (0, 1):
        add(plain_name(4, k, 1, 1, True), "masked", "masked", anchor, k, tp=64)
        add(plain_name(4, k, 1, 2, True), "masked", "masked", anchor, k, tp=64, teams=2)
        add(plain_name(4, k, 1, 1, True, True), "masked", "masked", anchor, k, tp=64, area=True)
    # depth-only scopes: the shadow map itself is the frame; their multiview forms against the single-view scopes (multiview_cases)
    anchor = own_name("raster_kernel_depth", 0, 0)
    for k in (0, 1):
        for t in (0, 1):
            add(own_name("raster_kernel_depth", k, t), "depth", "depth", anchor, k, tp=64 * t)
            add(own_name("raster_kernel_depth", k, t, True), "depth", "depth", anchor, k, tp=64 * t, area=True)
            add(own_name("raster_kernel_depth_batch", k, t), "depth", "views", own_name("raster_kernel_depth", k, t), k, tp=64 * t, route="multiview",
                yardstick="every layer = its single-view scope, bit for bit (multiview_cases.assert_equivalent)")
    # the lit families: MODEL_PBR per shadow term, MODEL_PBR_IBL per shadow term, seamless or not
    for term, kernel in ((1, "raster_kernel_shadow"), (2, "raster_kernel_csm"), (3, "raster_kernel_csm_blend")):
        for k in (0, 1):
            for t in (0, 1):
                for area in (False, True):
                    add(own_name(kernel, k, t, area), kernel[len("raster_kernel_"):], "pbr", own_name(kernel, 0, 0), k, tp=64 * t, area=area, shadow=term)
    for seamless in (False, True):
        for term in range(4):
            for k in (0, 1):
                for t in (0, 1):
                    for area in (False, True):
                        add(ibl_name(k, t, term, area, seamless), f"{'s' if seamless else ''}ibl{term}", "ibl", ibl_name(0, 0, term, False, seamless), k,
                            tp=64 * t, area=area, shadow=term, seamless=(seamless, seamless, False))
    for name, seamless in (("sky_kernel", False), ("sky_kernel_seamless", True)):
        add(name, "sky", "sky", name, seamless=(False, False, seamless), yardstick="the float64 sky model (sky_cases.model / seamless_cases.sky_case), max(8 E32, 1e-4)")
    for name, xfer in (("transfer_copy_kernel", "copy_buffer"), ("transfer_blit_kernel<0>", "blit NEAREST"), ("transfer_blit_kernel<1>", "blit LINEAR"),
                       ("transfer_fill_kernel", "clear_color_image")):
        add(name, "transfer", "transfer", name, xfer=xfer, yardstick="transfer_cases' models, as tests/test_gpu_transfer.py holds them")
    return rows


ROWS = _build()
LEDGER = {r.name: r for r in ROWS}
assert len(LEDGER) == len(ROWS), "a row name occurs twice in the ledger"
FAMILIES = sorted({r.family for r in ROWS})

# Per anchor: the existing comparison the ledger test runs while the trace is on ("module:function" and its arguments after the fixtures mirhi, scenes,
# oracle, device as the function names them), under the anchor's knobs; "ledger:..." is a comparison on the ledger's own scene with the named existing helper.
ANCHOR_CHECKS = {
    **{plain_name(p, 0, 0, 1, False): "ledger:test_gpu_parity._check against the oracle (prim, depth, colour)" for p in KINDS},
    plain_name(4, 0, 1, 1, True): "ledger:test_gpu_parity._check against the oracle (prim, depth, colour)",
    **{f"raster_kernel_msaa<{p}, 0>": "ledger:msaa_cases.oracle_samples (winners per sample, sample-0 depth); fully covered pixels = the 1x frame" for p in KINDS},
    own_name("raster_kernel_depth", 0, 0): "ledger:the oracle's MODEL depth (test_gpu_shadow.test_depth_only_pass_matches_the_oracle_model_depth's statement)",
    own_name("raster_kernel_shadow", 0, 0): ("test_gpu_shadow:test_pcf_factor_matches_the_numpy_model", (1.0,)),
    own_name("raster_kernel_csm", 0, 0): ("test_gpu_csm:test_csm_factor_matches_the_numpy_model", ()),
    own_name("raster_kernel_csm_blend", 0, 0): ("test_gpu_csm_blend:test_blended_factor_matches_the_model", (False,)),
    ibl_name(0, 0, 0): ("test_gpu_ibl_shading:test_ambient_against_the_float64_model", (16, 5)),
    ibl_name(0, 0, 1): ("test_gpu_ibl_shading:test_zero_environment_equals_model_pbr_single_map", ()),
    ibl_name(0, 0, 2): ("test_gpu_ibl_shading:test_zero_environment_equals_model_pbr_cascades", ()),
    ibl_name(0, 0, 3): ("test_gpu_csm_blend:test_model_pbr_ibl_with_blended_cascades", ()),
    ibl_name(0, 0, 0, False, True): ("test_gpu_seamless:test_model_pbr_ibl_with_both_cubes_seamless", (0.5,)),
    ibl_name(0, 0, 1, False, True): "ledger:test_gpu_seamless._check_facets on seamless_cases.facets_scene under this module's shadow map",
    ibl_name(0, 0, 2, False, True): ("test_gpu_seamless:test_model_pbr_ibl_under_shadow_cascades", ()),
    ibl_name(0, 0, 3, False, True): "ledger:test_gpu_seamless._check_facets on seamless_cases.facets_scene under this module's blended cascades",
}


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
CLEAR_DEPTH = {"less": 1.0, "greater": 0.0, "predicate": 0.6, "blend": 1.0}


def scene_for(row, variant, key=None, area=None):
    """The scene of a rastered colour row.  variant: overdraw (layers A then B), twin (A alone), B (B alone: a yardstick's helper)."""
    S = _S()
    key = row.key if key is None else key
    draws = []
    for layer in {"overdraw": "AB", "twin": "A", "B": "B"}[variant]:
        draws += _draws(row.kind, layer, key)
    extra = shadow_term(row.shadow)
    if row.kind == "ibl":
        import seamless_cases
        extra["ibl"] = seamless_cases.ibl_set()
    scene = S.Scene(f"ledger {row.kind} {variant} {key} shadow{row.shadow}", W, H, draws, clear_color=CLEAR, clear_depth=CLEAR_DEPTH[key], **extra)
    if row.area if area is None else area:
        scene = rc.in_area(scene, AREA)
    return scene


def oracle_scene(row, variant, key=None):
    """What the oracle renders for it: no shadow scopes or IBL set, MODEL_PBR for the program it lacks (as ibl_shading_cases.with_program)."""
    import ibl_shading_cases
    S = _S()
    sc = scene_for(dataclasses.replace(row, shadow=0, kind="pbr" if row.kind == "ibl" else row.kind), variant, key, area=False)
    return ibl_shading_cases.with_program(sc, S.PROGRAM_MODEL_PBR) if row.kind == "ibl" else sc


def depth_points(variant):
    pts = []
    for layer in {"overdraw": "AB", "twin": "A", "B": "B"}[variant]:
        big, small = layer_points(layer)
        pts += big + small
    return pts


def depth_scene(row, variant, key=None):
    """A depth-only scope over the geometry into a MAP x MAP image (the frame), ahead of an empty colour scope."""
    S = _S()
    key = row.key if key is None else key
    compare = S.CMP_GREATER if key == "greater" else S.CMP_LESS
    casters = _casters(np.eye(4, dtype=np.float32), depth_points(variant), compare, VIEWPORT, flip=False)
    spec = S.ShadowSpec(casters, (MAP, MAP), S.shadow_ubo(np.eye(4, dtype=np.float32), size=(MAP, MAP)), clear_depth=CLEAR_DEPTH[key],
                        render_area=MAP_AREA if row.area else None)
    return S.Scene(f"ledger depth {variant} {key}", 64, 64, [], shadow=spec)


def depth_oracle_scene(variant, key):
    """The same geometry as MODEL draws of a MAP x MAP colour scope: the oracle's depth image is the depth-only scope's."""
    S = _S()
    pts = depth_points(variant)
    d = S.DrawSpec(vertices=_v48(pts), stride=48, count=len(pts), program=S.PROGRAM_MODEL, cull_mode=S.CULL_NONE, viewport=VIEWPORT,
                   depth_compare=S.CMP_GREATER if key == "greater" else S.CMP_LESS, camera=_identity_camera(), object=S.object_ubo(np.eye(4, dtype=np.float32)))
    return S.Scene(f"ledger depth oracle {variant} {key}", MAP, MAP, [d], clear_depth=CLEAR_DEPTH[key])


def view_casters(variant="overdraw"):
    """multiview_cases' caster tuples (vertices, indices, model) of the geometry, and the base matrix that shows it at MAP x MAP as VIEWPORT does."""
    pts = depth_points(variant)
    base = np.eye(4, dtype=np.float32)
    base[0, 0] = base[1, 1] = 2.0
    base[3, 0] = base[3, 1] = 1.0
    return [(_v48(pts), np.arange(len(pts), dtype=np.uint32), np.eye(4, dtype=np.float32))], base


# ---- the comparison --------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype == np.uint8 else a.view(np.uint32)


def frame_differences(got, want, area=None, sentinel=None, keys=("color", "prim", "depth")):
    """Every way `got` is not `want`, bit for bit, as a list of sentences (empty: the same frame).  With an area: `want` counts inside it, and outside it
    `sentinel` (the attachments' contents before the scope: color, prim, depth) must stand untouched."""
    out = []
    for k in keys:
        if k not in want:
            continue
        if k not in got:
            out.append(f"{k}: missing")
            continue
        w = want[k]
        if area is not None:
            w = rc.compose(want[k], sentinel[k], area)
        g = got[k]
        if g.shape != w.shape or g.dtype != w.dtype:
            out.append(f"{k}: shape / type {g.shape} {g.dtype} against {w.shape} {w.dtype}")
            continue
        diff = _bits(g) != _bits(w)
        if diff.any():
            first = tuple(int(v) for v in np.argwhere(diff)[0])
            where = ""
            if area is not None:
                inside = rc.mask(area, g.shape[1], g.shape[0])
                pix = diff.reshape(diff.shape[0], diff.shape[1], -1).any(axis=2)
                where = f" ({int((pix & inside).sum())} pixels inside the area, {int((pix & ~inside).sum())} sentinel pixels outside it)"
            out.append(f"{k}: {int(diff.sum())} words differ{where}, first at {first}: got {g[first[:g.ndim]]!r} want {w[first[:w.ndim]]!r}")
    return out


def twin_expectation(anchor_frame, clear_depth=0.0):
    """What the twin scene under GREATER / clear 0 must give, from the K = 0 anchor's frame of it under LESS / clear 1: the same colour and ids, the same depth
    where a primitive won, the other clear value elsewhere."""
    want = dict(anchor_frame)
    if "depth" in want:
        covered = (want["prim"] != NO_PRIM) if "prim" in want and want["prim"].ndim == 2 else (want["depth"] != np.float32(1.0))
        want["depth"] = np.where(covered, want["depth"], np.float32(clear_depth)).astype(np.float32)
    return want


def compose_by_primitive(prim, frame_a, frame_b, clear, n_a=None):
    """The colour image of a primitive-id image of the overdraw scene from the anchor's frames of its two layers drawn alone: a pixel won by a primitive of
    layer A holds frame_a's colour there, one won by layer B (ids from n_a on) frame_b's, an empty one the clear colour."""
    n_a = layer_triangles("A") if n_a is None else n_a
    out = np.empty_like(frame_a["color"])
    out[:] = np.array(clear, dtype=np.float32)
    a, b = (prim != NO_PRIM) & (prim < n_a), (prim != NO_PRIM) & (prim >= n_a)
    assert np.array_equal(frame_a["prim"][a], prim[a]) and np.array_equal(frame_b["prim"][b] + np.uint32(n_a), prim[b]), "a layer drawn alone shows another primitive there"
    out[a], out[b] = frame_a["color"][a], frame_b["color"][b]
    return out
