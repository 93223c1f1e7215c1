"""Multiview depth scopes (include/mirhi.h "Multiview depth scopes"): the statement the tests check, and their inputs.

THE EQUIVALENCE.  A multiview scope with view mask M over a D32 array is, bit for bit in every layer, the single-view scopes of the same build: for each
set bit v of M, a depth-only scope into layer_view(v) that records the same binds and draws, with the first 64 bytes of the ShadowConstants at
Slot.CAMERA (lightSpaceMatrix) replaced by the 64 bytes at view_offset + v * view_stride of the view constants; `model` @64 stays the draw's own.
Layers whose bit is clear are not touched.  run_single renders the right-hand side, run_multiview the left-hand side; both start from the same
sentinel-filled array and return all layers.

Inputs: 96 x 96 layers (3 x 3 tiles of 32 pixels), four layers (six for one test), the casters of test_gpu_shadow._casters under four scaled and
shifted copies of their light matrix (every layer's image differs), and small clip-space caster sets that take the raster kernel's other routes."""
import re
import os

import numpy as np

SIZE = 96
LAYERS = 4
STRIDE = 80               # view_stride of the tests: CSMParams' cascade stride
OFFSET = 32               # view_offset of the tests (a multiple of 16, not 0: the address arithmetic is part of what is checked)
TILES = (SIZE // 32) ** 2

# clip-space scale and shift (in NDC units) of view v's matrix against the base matrix: every scale >= 1, so that no view covers fewer texels than the base
VIEW_XFORM = [(1.0, 0.0, 0.0), (1.3, 0.2, -0.1), (1.15, -0.25, 0.15), (1.45, 0.1, 0.3), (1.2, -0.1, -0.2), (1.05, 0.3, 0.05)]


def view_matrix(base: np.ndarray, v: int) -> np.ndarray:
    """base ([col, row] float32, as every matrix of the interface) with clip x, y scaled by s and shifted by (tx, ty) * w."""
    s, tx, ty = VIEW_XFORM[v]
    m = base.astype(np.float32).copy()
    m[:, 0] = np.float32(s) * base[:, 0] + np.float32(tx) * base[:, 3]
    m[:, 1] = np.float32(s) * base[:, 1] + np.float32(ty) * base[:, 3]
    return m


def view_matrices(base: np.ndarray, count: int = LAYERS):
    return [view_matrix(base, v) for v in range(count)]


def sentinels(count: int = LAYERS, size: int = SIZE) -> np.ndarray:
    """As test_gpu_csm.test_shadow_scope_into_a_layer_view fills its array: a value per layer, a sparse pattern on top."""
    out = np.stack([np.full((size, size), 0.9 - 0.1 * k, dtype=np.float32) for k in range(count)])
    out[:, ::7, ::5] += np.float32(0.01)
    return out


def view_constants(mats, count: int, stride: int = STRIDE, offset: int = OFFSET) -> np.ndarray:
    """The view constants buffer: view v's matrix at offset + v * stride; every other byte 0xFF (a matrix read from the wrong place is NaNs)."""
    buf = np.full(offset + stride * (count - 1) + 64, 0xFF, dtype=np.uint8)
    for v, m in enumerate(mats[:count]):
        buf[offset + v * stride:offset + v * stride + 64] = np.frombuffer(np.asarray(m, dtype=np.float32).tobytes(), dtype=np.uint8)
    return buf


def tp_density() -> int:
    """Triangles per tile from which raster_mode switches a mesh-program (here: SHADOW) scope to the triangle-parallel path, read from mirhi_scope.h."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "renderer-rs_amd", "csrc", "mirhi_scope.h")).read()
    return int(re.search(r"c\.tri_prog \? 16 : (\d+)", src).group(1))


# ---- caster sets in clip space (model = identity, base light matrix = identity: vertex x, y are NDC, z the depth) ------------------------------
def _v48(pos: np.ndarray) -> np.ndarray:
    v = np.zeros((pos.shape[0], 12), dtype=np.float32)
    v[:, 0:3] = pos
    return v


def small_triangles(n: int, seed: int, lo: float = -0.28, hi: float = 0.28, edge: float = 0.05):
    """n triangles of about 2 x 2 pixels with random depths, all inside NDC [lo, hi]^2: at 96 x 96 under the identity that is pixels 35 .. 61, the
    middle tile alone."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(lo + edge, hi - edge, size=(n, 2))
    z = rng.uniform(0.1, 0.9, size=(n, 1))
    d = rng.uniform(0.5, 1.0, size=(n, 3, 2)) * edge * np.array([[-1.0, -1.0], [1.0, -0.6], [0.1, 1.0]])
    pos = np.concatenate([c[:, None, :] + d, np.repeat(z[:, None, :], 3, axis=1) + rng.uniform(-0.05, 0.05, size=(n, 3, 1))], axis=2)
    return _v48(pos.reshape(-1, 3)), np.arange(3 * n, dtype=np.uint32), np.eye(4, dtype=np.float32)


def route_casters(route: str):
    """One caster set per route of the raster kernel (DESIGN.md "Kernels"): (casters, scissor or None)."""
    eye = np.eye(4, dtype=np.float32)
    if route == "records65":        # one page of 64 records and one record of the next
        return [small_triangles(65, 1)], None
    if route == "records193":       # one LDS chunk of 192 records and one record of the next
        return [small_triangles(193, 2)], None
    if route == "big_list":         # vertices more than 65535 sub-pixels apart: no bin record can hold it
        pos = np.array([[-5.0, -4.0, 0.3], [5.0, -4.5, 0.6], [0.3, 5.0, 0.45]])
        return [(_v48(pos), np.arange(3, dtype=np.uint32), eye), small_triangles(5, 3)], None
    if route == "near_clip":        # one vertex in front of the near plane (z < 0): clipped, the pieces go to the big list
        pos = np.array([[-0.7, -0.6, 0.4], [0.8, -0.5, 0.5], [0.1, 0.9, -0.6]])
        return [(_v48(pos), np.arange(3, dtype=np.uint32), eye), small_triangles(5, 4)], None
    if route == "scissor":          # a scissor whose edges run through tiles
        return [small_triangles(40, 5, -0.9, 0.9, 0.2)], (10, 20, 50, 41)
    if route == "tp_below":         # one triangle fewer than the triangle-parallel threshold of this size: the pixel-parallel-only kernel
        return [small_triangles(tp_density() * TILES - 1, 6, -0.9, 0.9, 0.08)], None
    if route == "tp_at":            # the threshold itself: the kernel with the triangle-parallel path
        return [small_triangles(tp_density() * TILES, 7, -0.9, 0.9, 0.08)], None
    raise KeyError(route)


ROUTES = ["records65", "records193", "big_list", "near_clip", "scissor", "tp_below", "tp_at"]


# ---- the two sides of the equivalence -----------------------------------------------------------------------------------------------------------
def shadow_pipeline(mirhi, scenes, dev, compare=None, cull=None, bias=None):
    b = (mirhi.GraphicsPipelineBuilder().vertex_shader(mirhi.Program.SHADOW).fragment_shader(mirhi.Program.SHADOW)
         .vertex_binding(48).vertex_attributes(mirhi.SHADOW_VERTEX_OFFSETS)
         .color_attachment_format(mirhi.Format.UNDEFINED).depth_attachment_format(mirhi.Format.D32_SFLOAT)
         .cull_mode(scenes.CULL_NONE if cull is None else cull).depth_compare_op(scenes.CMP_LESS if compare is None else compare))
    if bias is not None:
        b.depth_bias(*bias)
    return b.build(dev)


class CasterBuffers:
    """Vertex and index buffers of a caster set, uploaded once and shared by both sides."""

    def __init__(self, mirhi, dev, casters):
        self.items = [(mirhi.Buffer.new_with_data(dev, mirhi.BufferUsage.Vertex, np.ascontiguousarray(v, dtype=np.float32)),
                       mirhi.Buffer.new_with_data(dev, mirhi.BufferUsage.Index, np.asarray(i).astype(np.uint32)), int(np.asarray(i).size), m) for v, i, m in casters]

    def destroy(self):
        for vb, ib, _, _ in self.items:
            vb.destroy(); ib.destroy()


def record_draws(mirhi, scenes, cmd, dev, pipe, bufs, matrix, size, scissor, objs, instances=1):
    """The binds and draws of one scope: each caster's ShadowConstants hold `matrix` @0 and the caster's model @64."""
    cmd.set_viewport(0.0, 0.0, float(size), float(size))
    cmd.set_scissor(*(scissor or (0, 0, size, size)))
    cmd.bind_pipeline(pipe)
    for vb, ib, count, m in bufs.items:
        ub = mirhi.Buffer.new_with_data(dev, mirhi.BufferUsage.Uniform, np.frombuffer(scenes.shadow_constants_ubo(matrix, m), dtype=np.uint8))
        objs.append(ub)
        cmd.bind_vertex_buffers(0, [vb], [0])
        cmd.bind_index_buffer(ib, 0, mirhi.IndexType.UINT32)
        cmd.bind_uniform(mirhi.Slot.CAMERA, ub)
        cmd.draw_indexed(count, instances, 0, 0, 0)


# what a multiview scope's draws carry @0 of their own CAMERA block: NOT a light matrix of any view (the scope must not read it)
DECOY = np.diag([7.0, -3.0, 0.25, 1.0]).astype(np.float32)


def run_single(mirhi, scenes, dev, bufs, mats, mask, start, pipe, load=False, clear=1.0, scissor=None, instances=1):
    """Right-hand side: one depth-only scope per set bit of mask into layer_view(v), all in one command buffer.  Returns the array's layers."""
    count, size = start.shape[0], start.shape[1]
    array = mirhi.Image.array(dev, size, size, count, mirhi.Format.D32_SFLOAT)
    array.upload(start)
    views, objs = [], []
    cmd = mirhi.CommandBuffer(dev)
    cmd.begin()
    for v in range(count):
        if not (mask >> v) & 1:
            continue
        view = array.layer_view(v)
        views.append(view)
        cmd.begin_rendering(None, depth=view, clear_depth=clear, depth_store_op=mirhi.StoreOp.STORE,
                            depth_load_op=mirhi.LoadOp.LOAD if load else mirhi.LoadOp.CLEAR)
        record_draws(mirhi, scenes, cmd, dev, pipe, bufs, mats[v], size, scissor, objs, instances)
        cmd.end_rendering()
    cmd.end()
    dev.submit([cmd])
    dev.wait_idle()
    out = array.read().copy()
    cmd.destroy()
    for o in views + objs:
        o.destroy()
    array.destroy()
    return out


def run_multiview(mirhi, scenes, dev, bufs, mats, mask, start, pipe, load=False, clear=1.0, scissor=None, instances=1):
    """Left-hand side: ONE multiview scope.  Returns the array's layers."""
    count, size = start.shape[0], start.shape[1]
    array = mirhi.Image.array(dev, size, size, count, mirhi.Format.D32_SFLOAT)
    array.upload(start)
    consts = mirhi.Buffer.new_with_data(dev, mirhi.BufferUsage.Uniform, view_constants(mats, count))
    objs = [consts]
    cmd = mirhi.CommandBuffer(dev)
    cmd.begin()
    cmd.begin_rendering_multiview(array, mask, consts, OFFSET, STRIDE, clear_depth=clear, depth_load_op=mirhi.LoadOp.LOAD if load else mirhi.LoadOp.CLEAR)
    record_draws(mirhi, scenes, cmd, dev, pipe, bufs, DECOY, size, scissor, objs, instances)
    cmd.end_rendering()
    cmd.end()
    dev.submit([cmd])
    dev.wait_idle()
    out = array.read().copy()
    cmd.destroy()
    for o in objs:
        o.destroy()
    array.destroy()
    return out


def assert_equivalent(multi, single, start, mask, name=""):
    for v in range(start.shape[0]):
        if (mask >> v) & 1:
            assert np.array_equal(multi[v].view(np.uint32), single[v].view(np.uint32)), f"{name}: layer {v} differs from its single-view scope"
            assert not np.array_equal(multi[v].view(np.uint32), start[v].view(np.uint32)), f"{name}: layer {v} was not rendered"
        else:
            assert np.array_equal(multi[v].view(np.uint32), start[v].view(np.uint32)), f"{name}: layer {v} lost its sentinel"
            assert np.array_equal(single[v].view(np.uint32), start[v].view(np.uint32))
