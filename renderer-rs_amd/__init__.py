"""renderer_rs_amd -- Python host binding of libmirhi.so, the MI355X-native compute rasterizer.

The product is the C-ABI shared library (include/mirhi.h); this module is a thin ctypes mirror of
the reference's `crates/rhi` object names (Device, Buffer, BufferUsage, GraphicsPipelineBuilder,
CommandBuffer, Fence, ...) used by tests/ and bench.py.  There is no CPU fallback: if the library
cannot be loaded the import fails, and creating a Device without a gfx950 GPU raises RhiError.

The directory name contains a hyphen, so load it with `load_package()` from
`__graft_entry__.py` (registers the module as `renderer_rs_amd`).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import build as _build
from . import scenes  # noqa: F401  (re-export)
from . import ibl  # noqa: F401  (re-export: the numpy model of the IBL precompute passes)
from . import lighting  # noqa: F401  (re-export: the numpy model of the lit fragment programs)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, os.environ.get("MIRHI_LIB_NAME", "libmirhi.so"))   # MIRHI_LIB_NAME: diagnostic builds only
INCLUDE = os.path.join(os.path.dirname(HERE), "include", "mirhi.h")

# ---- enums (include/mirhi.h) ------------------------------------------------------------------------
OK, ERR_DEVICE, ERR_LOADING, ERR_ALLOCATOR, ERR_NO_SUITABLE_GPU, ERR_SHADER, ERR_SURFACE, ERR_SWAPCHAIN, \
    ERR_INVALID_HANDLE, ERR_PIPELINE, ERR_LOCK_POISONED, TIMEOUT, NOT_READY = range(13)


class BufferUsage:  # crates/rhi/src/buffer.rs:47-60
    Vertex, Index, Uniform, Storage, Staging, Indirect = range(6)


class Format:
    UNDEFINED, B8G8R8A8_SRGB, R32G32B32A32_SFLOAT, D32_SFLOAT, R8G8B8A8_UNORM, R32_UINT, R8G8B8A8_SRGB = range(7)


class Program:
    NONE, TRIANGLE, MODEL, MODEL_FULL, MODEL_PBR, SHADOW, MODEL_PBR_IBL, SKYBOX = -1, 0, 1, 2, 3, 4, 5, 6


class PrimitiveTopology:  # pipeline.rs:274-282
    PointList, LineList, LineStrip, TriangleList, TriangleStrip, TriangleFan = range(6)


class PolygonMode:
    Fill, Line, Point = range(3)


class CullMode:  # pipeline.rs:329-336
    NONE, Front, Back, FrontAndBack = range(4)


class FrontFace:
    CounterClockwise, Clockwise = range(2)


class CompareOp:  # pipeline.rs:375-386
    Never, Less, Equal, LessOrEqual, Greater, NotEqual, GreaterOrEqual, Always = range(8)


class BlendFactor:  # pipeline.rs:411-448
    (Zero, One, SrcColor, OneMinusSrcColor, DstColor, OneMinusDstColor, SrcAlpha, OneMinusSrcAlpha, DstAlpha, OneMinusDstAlpha,
     ConstantColor, OneMinusConstantColor, ConstantAlpha, OneMinusConstantAlpha, SrcAlphaSaturate) = range(15)


class BlendOp:  # pipeline.rs:452-476
    Add, Subtract, ReverseSubtract, Min, Max = range(5)


class LoadOp:
    LOAD, CLEAR, DONT_CARE = range(3)


class StoreOp:
    STORE, DONT_CARE = range(2)


class IndexType:
    UINT16, UINT32 = range(2)


class Slot:
    CAMERA, OBJECT, LIGHTS, MATERIAL, POINT_LIGHTS, SPOT_LIGHTS, SHADOW_DATA = range(7)


class TextureSlot:
    ALBEDO, NORMAL, METALLIC_ROUGHNESS, OCCLUSION, EMISSIVE, SHADOW_MAP = range(6)


class Kernel:
    GEOMETRY, RASTER, VERTEX, FRAGMENT_COUNT = range(4)
    NAMES = ("geometry", "raster", "vertex", "fragment_count")


class Profile:
    TIMING, FRAGMENTS = 1, 2


class GatherAlgo:
    DIRECT, BROADCAST = range(2)


class Filter:
    """mirhi_filter (VkFilter) of CommandBuffer.blit_image"""
    NEAREST, LINEAR = range(2)


class AddressMode:
    """mirhi_address_mode of a texture's sampler (SamplerDesc.address_u / address_v)"""
    REPEAT, MIRRORED_REPEAT, CLAMP_TO_EDGE = range(3)


class SamplerFilter:
    """mirhi_sampler_filter of a texture's sampler (SamplerDesc.mag_filter / min_filter): zero is LINEAR, unlike the blit's Filter"""
    LINEAR, NEAREST = range(2)


class MipMode:
    """mirhi_mip_mode of a texture's sampler: BASE samples level 0 whatever the chain"""
    LINEAR, NEAREST, BASE = range(3)


class SplitLayout:
    """mirhi_split_layout: which tile rows a rank of a tile split rasterizes"""
    BANDS, INTERLEAVED = range(2)
    NAMES = {"bands": 0, "interleaved": 1}


ABI_VERSION = 5                 # MIRHI_ABI_VERSION of include/mirhi.h this file mirrors
COMM_ID_BYTES = 128


MAX_FRAMES_IN_FLIGHT = 2  # crates/renderer/src/lib.rs:43


# ---- structs ------------------------------------------------------------------------------------------
class PipelineDesc(C.Structure):
    _fields_ = [
        ("vertex_program", C.c_int32), ("fragment_program", C.c_int32), ("vertex_stride", C.c_uint32),
        ("attribute_count", C.c_uint32), ("attribute_offsets", C.c_uint32 * 4),
        ("topology", C.c_int32), ("polygon_mode", C.c_int32), ("cull_mode", C.c_int32), ("front_face", C.c_int32),
        ("depth_clamp_enable", C.c_uint32), ("rasterizer_discard_enable", C.c_uint32), ("depth_bias_enable", C.c_uint32),
        ("rasterization_samples", C.c_uint32), ("depth_test_enable", C.c_uint32), ("depth_write_enable", C.c_uint32),
        ("depth_compare_op", C.c_int32), ("blend_enable", C.c_uint32), ("blend_attachment_count", C.c_uint32),
        ("color_attachment_count", C.c_uint32), ("color_attachment_formats", C.c_int32 * 4),
        ("depth_attachment_format", C.c_int32),
        ("src_color_blend_factor", C.c_int32), ("dst_color_blend_factor", C.c_int32), ("color_blend_op", C.c_int32),
        ("src_alpha_blend_factor", C.c_int32), ("dst_alpha_blend_factor", C.c_int32), ("alpha_blend_op", C.c_int32),
        ("color_write_mask", C.c_uint32),
        ("fragment_discard_enable", C.c_uint32),
    ]


class DepthBias(C.Structure):
    """mirhi_depth_bias: the factors of GraphicsPipelineBuilder::depth_bias (pipeline.rs:781-788)"""
    _fields_ = [("constant_factor", C.c_float), ("clamp", C.c_float), ("slope_factor", C.c_float)]


class SamplerDesc(C.Structure):
    """mirhi_sampler_desc: the sampler state of a texture (Image.set_sampler); all zero = REPEAT / LINEAR / MIP_LINEAR, the default"""
    _fields_ = [("address_u", C.c_int32), ("address_v", C.c_int32), ("mag_filter", C.c_int32), ("min_filter", C.c_int32), ("mip_mode", C.c_int32)]

    def as_tuple(self):
        return (self.address_u, self.address_v, self.mag_filter, self.min_filter, self.mip_mode)


class RenderingInfo(C.Structure):
    _fields_ = [
        ("color_image", C.c_void_p), ("color_load_op", C.c_int32), ("color_store_op", C.c_int32),
        ("clear_color", C.c_float * 4),
        ("depth_image", C.c_void_p), ("depth_load_op", C.c_int32), ("depth_store_op", C.c_int32),
        ("clear_depth", C.c_float), ("render_area", C.c_int32 * 4), ("prim_id_image", C.c_void_p),
    ]


class ResolveMode:   # mirhi_resolve_mode (VkResolveModeFlagBits)
    NONE, SAMPLE_ZERO, AVERAGE = range(3)


class ResolveInfo(C.Structure):      # mirhi_resolve_info
    _fields_ = [("color_resolve_image", C.c_void_p), ("color_resolve_mode", C.c_int32),
                ("depth_resolve_image", C.c_void_p), ("depth_resolve_mode", C.c_int32)]


class MultiviewInfo(C.Structure):      # mirhi_multiview_info
    _fields_ = [("view_mask", C.c_uint32), ("view_constants", C.c_void_p), ("view_offset", C.c_uint64), ("view_stride", C.c_uint32)]


class Viewport(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("width", C.c_float), ("height", C.c_float),
                ("min_depth", C.c_float), ("max_depth", C.c_float)]


class Rect2D(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_uint32), ("height", C.c_uint32)]


# regions of the recorded transfer commands (include/mirhi.h "Transfer commands"); the CommandBuffer methods also take plain tuples in field order
class BufferCopy(C.Structure):           # VkBufferCopy
    _fields_ = [("src_offset", C.c_uint64), ("dst_offset", C.c_uint64), ("size", C.c_uint64)]


class BufferImageCopy(C.Structure):      # VkBufferImageCopy (2-D, one layer); row length / image height 0 = tightly packed
    _fields_ = [("buffer_offset", C.c_uint64), ("buffer_row_length", C.c_uint32), ("buffer_image_height", C.c_uint32),
                ("mip_level", C.c_uint32), ("image_offset", C.c_int32 * 2), ("image_extent", C.c_uint32 * 2)]


class ImageCopy(C.Structure):            # VkImageCopy
    _fields_ = [("src_mip_level", C.c_uint32), ("src_offset", C.c_int32 * 2), ("dst_mip_level", C.c_uint32), ("dst_offset", C.c_int32 * 2),
                ("extent", C.c_uint32 * 2)]


class ImageBlit(C.Structure):            # VkImageBlit: offsets[corner][x, y]
    _fields_ = [("src_mip_level", C.c_uint32), ("src_offsets", (C.c_int32 * 2) * 2), ("dst_mip_level", C.c_uint32), ("dst_offsets", (C.c_int32 * 2) * 2)]


def _regions(cls, regions):
    """A ctypes array of `cls` from structures of that class or tuples in its field order (nested tuples for the array fields)."""
    def one(r):
        if isinstance(r, cls):
            return r
        out = cls()
        for (name, ctype), value in zip(cls._fields_, r):
            if issubclass(ctype, C.Array):
                flat = np.asarray(value).reshape(-1).tolist()
                words = (C.c_int32 * len(flat))(*[int(v) for v in flat])      # (ctypes integers wrap: the bits of a uint32 field too)
                C.memmove(C.addressof(out) + getattr(cls, name).offset, words, 4 * len(flat))
            else:
                setattr(out, name, int(value))
        return out
    items = [one(r) for r in regions]
    return (cls * max(1, len(items)))(*items), len(items)


class DispatchTime(C.Structure):
    _fields_ = [("kernel", C.c_uint32), ("lane", C.c_uint32), ("begin_us", C.c_double), ("end_us", C.c_double)]


class DeviceStats(C.Structure):
    _fields_ = [("frames_submitted", C.c_uint64), ("triangles_submitted", C.c_uint64), ("workspace_bytes", C.c_uint64),
                ("last_big_list", C.c_uint32), ("last_status", C.c_uint32), ("last_bin_pages", C.c_uint32), ("native_dispatches", C.c_uint32),
                ("dispatch_path", C.c_uint32), ("device_lost", C.c_uint32), ("reserved", C.c_uint32)]


class RhiError(RuntimeError):
    """crates/rhi/src/error.rs:6-50; `.code` is the mirhi_result, `.variant` the RhiError variant name."""

    def __init__(self, code: int, message: str, variant: str):
        super().__init__(f"[{variant}] {message}")
        self.code, self.message, self.variant = code, message, variant


# ---- library loading ------------------------------------------------------------------------------------
_lib = None

_SIGNATURES = {
    "mirhi_last_error_message": (C.c_char_p, []),
    "mirhi_result_name": (C.c_char_p, [C.c_int32]),
    "mirhi_abi_version": (C.c_uint32, []),
    "mirhi_device_count": (C.c_int32, [C.POINTER(C.c_int32)]),
    "mirhi_device_create": (C.c_int32, [C.c_int32, C.POINTER(C.c_void_p)]),
    "mirhi_device_create_on_stream": (C.c_int32, [C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mirhi_device_wait_idle": (C.c_int32, [C.c_void_p]),
    "mirhi_device_destroy": (C.c_int32, [C.c_void_p]),
    "mirhi_device_name": (C.c_int32, [C.c_void_p, C.c_char_p, C.c_uint32]),
    "mirhi_device_set_tile_split": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "mirhi_device_set_queue_lanes": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "mirhi_device_set_submit_thread": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "mirhi_device_band_rows": (C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mirhi_device_set_tile_split_layout": (C.c_int32, [C.c_void_p, C.c_int32]),
    "mirhi_device_split_rows": (C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mirhi_buffer_create": (C.c_int32, [C.c_void_p, C.c_int32, C.c_uint64, C.POINTER(C.c_void_p)]),
    "mirhi_buffer_create_with_data": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "mirhi_buffer_write": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "mirhi_buffer_upload": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mirhi_buffer_upload_via_staging": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mirhi_buffer_wrap_device_memory": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "mirhi_buffer_read": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    "mirhi_buffer_size": (C.c_uint64, [C.c_void_p]),
    "mirhi_buffer_usage_of": (C.c_int32, [C.c_void_p]),
    "mirhi_buffer_device_ptr": (C.c_void_p, [C.c_void_p]),
    "mirhi_buffer_destroy": (C.c_int32, [C.c_void_p]),
    "mirhi_image_create": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]),
    "mirhi_image_wrap_device_memory": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mirhi_image_create_array": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]),
    "mirhi_image_create_layer_view": (C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mirhi_image_layers": (C.c_uint32, [C.c_void_p]),
    "mirhi_image_create_multisampled": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mirhi_image_samples": (C.c_uint32, [C.c_void_p]),
    "mirhi_image_create_cube": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]),
    "mirhi_ibl_equirect_to_cube": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mirhi_image_expand_rgbe": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mirhi_ibl_equirect_to_cube_rgbe": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mirhi_ibl_cube_generate_mips": (C.c_int32, [C.c_void_p]),
    "mirhi_ibl_irradiance": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mirhi_ibl_prefilter": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "mirhi_ibl_brdf_lut": (C.c_int32, [C.c_void_p]),
    "mirhi_image_upload": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mirhi_image_read": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "mirhi_image_generate_mips": (C.c_int32, [C.c_void_p]),
    "mirhi_image_set_max_anisotropy": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "mirhi_image_max_anisotropy": (C.c_uint32, [C.c_void_p]),
    "mirhi_sampler_desc_default": (None, [C.c_void_p]),
    "mirhi_image_set_sampler": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mirhi_image_sampler": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mirhi_image_set_cube_seamless": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "mirhi_image_cube_seamless": (C.c_uint32, [C.c_void_p]),
    "mirhi_image_mip_levels": (C.c_uint32, [C.c_void_p]),
    "mirhi_image_width": (C.c_uint32, [C.c_void_p]),
    "mirhi_image_height": (C.c_uint32, [C.c_void_p]),
    "mirhi_image_format": (C.c_int32, [C.c_void_p]),
    "mirhi_image_size_bytes": (C.c_uint64, [C.c_void_p]),
    "mirhi_image_device_ptr": (C.c_void_p, [C.c_void_p]),
    "mirhi_image_destroy": (C.c_int32, [C.c_void_p]),
    "mirhi_pipeline_desc_default": (None, [C.POINTER(PipelineDesc)]),
    "mirhi_pipeline_create": (C.c_int32, [C.c_void_p, C.POINTER(PipelineDesc), C.POINTER(C.c_void_p)]),
    "mirhi_pipeline_create_with_depth_bias": (C.c_int32, [C.c_void_p, C.POINTER(PipelineDesc), C.POINTER(DepthBias), C.POINTER(C.c_void_p)]),
    "mirhi_pipeline_destroy": (C.c_int32, [C.c_void_p]),
    "mirhi_rendering_info_default": (None, [C.POINTER(RenderingInfo)]),
    "mirhi_cmd_create": (C.c_int32, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "mirhi_cmd_destroy": (C.c_int32, [C.c_void_p]),
    "mirhi_cmd_set_queue_lane": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "mirhi_cmd_draw_indirect": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]),
    "mirhi_cmd_draw_indexed_indirect": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]),
    "mirhi_cmd_push_constants": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]),
    "mirhi_cmd_begin": (C.c_int32, [C.c_void_p]),
    "mirhi_cmd_begin_reusable": (C.c_int32, [C.c_void_p]),
    "mirhi_cmd_end": (C.c_int32, [C.c_void_p]),
    "mirhi_cmd_reset": (C.c_int32, [C.c_void_p]),
    "mirhi_cmd_begin_rendering": (C.c_int32, [C.c_void_p, C.POINTER(RenderingInfo)]),
    "mirhi_resolve_info_default": (None, [C.POINTER(ResolveInfo)]),
    "mirhi_cmd_begin_rendering_resolve": (C.c_int32, [C.c_void_p, C.POINTER(RenderingInfo), C.POINTER(ResolveInfo)]),
    "mirhi_multiview_info_default": (None, [C.POINTER(MultiviewInfo)]),
    "mirhi_cmd_begin_rendering_multiview": (C.c_int32, [C.c_void_p, C.POINTER(RenderingInfo), C.POINTER(MultiviewInfo)]),
    "mirhi_cmd_end_rendering": (C.c_int32, [C.c_void_p]),
    "mirhi_cmd_bind_pipeline": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mirhi_cmd_bind_vertex_buffers": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "mirhi_cmd_bind_index_buffer": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32]),
    "mirhi_cmd_bind_uniform": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_uint64]),
    "mirhi_cmd_bind_texture": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p]),
    "mirhi_cmd_bind_shadow_cascades": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "mirhi_cmd_bind_shadow_cascades_blended": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_float]),
    "mirhi_cmd_bind_ibl": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mirhi_cmd_bind_skybox": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "mirhi_cmd_copy_buffer": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(BufferCopy)]),
    "mirhi_cmd_copy_buffer_to_image": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(BufferImageCopy)]),
    "mirhi_cmd_copy_image_to_buffer": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(BufferImageCopy)]),
    "mirhi_cmd_copy_image": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ImageCopy)]),
    "mirhi_cmd_blit_image": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(ImageBlit), C.c_int32]),
    "mirhi_cmd_clear_color_image": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
    "mirhi_cmd_clear_depth_stencil_image": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_float]),
    "mirhi_cmd_set_viewport": (C.c_int32, [C.c_void_p, C.POINTER(Viewport)]),
    "mirhi_cmd_set_scissor": (C.c_int32, [C.c_void_p, C.POINTER(Rect2D)]),
    "mirhi_cmd_draw": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "mirhi_cmd_draw_indexed": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_uint32]),
    "mirhi_queue_submit": (C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.c_void_p]),
    "mirhi_fence_create": (C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mirhi_fence_wait": (C.c_int32, [C.c_void_p, C.c_uint64]),
    "mirhi_fence_reset": (C.c_int32, [C.c_void_p]),
    "mirhi_fence_status": (C.c_int32, [C.c_void_p]),
    "mirhi_fence_destroy": (C.c_int32, [C.c_void_p]),
    "mirhi_device_set_profiling": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "mirhi_device_kernel_time": (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "mirhi_device_reset_kernel_times": (C.c_int32, [C.c_void_p]),
    "mirhi_device_timeline": (C.c_int32, [C.c_void_p, C.POINTER(DispatchTime), C.c_uint32, C.POINTER(C.c_uint32)]),
    "mirhi_device_fragment_stats": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mirhi_comm_unique_id": (C.c_int32, [C.c_void_p]),
    "mirhi_comm_create": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mirhi_comm_world": (C.c_uint32, [C.c_void_p]),
    "mirhi_comm_rank": (C.c_uint32, [C.c_void_p]),
    "mirhi_comm_all_gather_bands": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "mirhi_comm_destroy": (C.c_int32, [C.c_void_p]),
    "mirhi_device_get_stats": (C.c_int32, [C.c_void_p, C.POINTER(DeviceStats)]),
    "mirhi_device_dispatch_path": (C.c_int32, [C.c_void_p, C.c_char_p, C.c_uint32]),
    "mirhi_device_measure_roundtrip": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]),
    "mirhi_device_set_native_dispatch": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "mirhi_build_id": (C.c_char_p, []),
}


def lib():
    """Loads libmirhi.so (building it first if the sources are newer). Raises if unavailable."""
    global _lib
    if _lib is None:
        if _build.needs_build() and LIB_PATH.endswith("libmirhi.so"):
            _build.build()
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: the HIP extension must be built (python __graft_entry__.py)")
        # (a variant build named by MIRHI_LIB_NAME is loaded globally, so that libmirhost.so -- linked against libmirhi.so -- binds to IT)
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL if os.environ.get("MIRHI_LIB_NAME") else C.DEFAULT_MODE)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError = header/library mismatch: fail loudly
            fn.restype, fn.argtypes = res, args
        if L.mirhi_abi_version() != ABI_VERSION:        # struct layouts (mirhi_pipeline_desc, ...) are this binding's: a stale library must not be driven with them
            raise ImportError(f"{LIB_PATH} has ABI {L.mirhi_abi_version()}, this binding is written for ABI {ABI_VERSION}: rebuild (python __graft_entry__.py)")
        _lib = L
    return _lib


def check(rc: int):
    if rc != OK:
        L = lib()
        raise RhiError(rc, L.mirhi_last_error_message().decode("utf-8", "replace"), L.mirhi_result_name(rc).decode())


def _as_bytes(data):
    if isinstance(data, (bytes, bytearray)):
        return np.frombuffer(bytes(data), dtype=np.uint8)
    return np.ascontiguousarray(data).view(np.uint8).reshape(-1)


# ---- object wrappers (names follow crates/rhi) -----------------------------------------------------------
class Device:
    """rhi::Device (crates/rhi/src/device.rs:120-233)."""

    def __init__(self, ordinal: int = 0, stream: Optional[int] = None):
        h = C.c_void_p()
        if stream is None:
            check(lib().mirhi_device_create(ordinal, C.byref(h)))
        else:
            check(lib().mirhi_device_create_on_stream(ordinal, C.c_void_p(stream), C.byref(h)))
        self.handle = h

    @staticmethod
    def count() -> int:
        n = C.c_int32()
        check(lib().mirhi_device_count(C.byref(n)))
        return n.value

    def wait_idle(self):
        check(lib().mirhi_device_wait_idle(self.handle))

    def name(self) -> str:
        buf = C.create_string_buffer(256)
        check(lib().mirhi_device_name(self.handle, buf, 256))
        return buf.value.decode()

    def set_tile_split(self, rank: int, world: int, layout=None):
        """layout: None = keep the device's (default interleaved, MIRHI_SPLIT in the environment), SplitLayout.* or 'bands' / 'interleaved'"""
        if layout is not None:
            check(lib().mirhi_device_set_tile_split_layout(self.handle, SplitLayout.NAMES[layout] if isinstance(layout, str) else int(layout)))
        check(lib().mirhi_device_set_tile_split(self.handle, rank, world))

    def set_split_layout(self, layout):
        """SplitLayout.* or 'bands' / 'interleaved' (mirhi_device_set_tile_split_layout): before set_tile_split / Comm"""
        check(lib().mirhi_device_set_tile_split_layout(self.handle, SplitLayout.NAMES[layout] if isinstance(layout, str) else int(layout)))

    def split_rows(self, height: int):
        """(first tile row, step, number of tile rows) this device rasterizes of a frame `height` pixels high"""
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().mirhi_device_split_rows(self.handle, height, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_queue_lanes(self, lanes: int):
        check(lib().mirhi_device_set_queue_lanes(self.handle, lanes))

    def set_submit_thread(self, enable: bool = True):
        """vkQueueSubmit semantics: submit() queues the work and returns, a thread of the device makes the launches (include/mirhi.h)"""
        check(lib().mirhi_device_set_submit_thread(self.handle, int(enable)))

    def band_rows(self, height: int):
        a, b = C.c_uint32(), C.c_uint32()
        check(lib().mirhi_device_band_rows(self.handle, height, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_profiling(self, enable):
        """False / 0 = off, True = Profile.TIMING, or a mask of Profile.TIMING | Profile.FRAGMENTS."""
        check(lib().mirhi_device_set_profiling(self.handle, int(enable)))

    def kernel_time(self, kernel: int):
        ms, n = C.c_double(), C.c_uint64()
        check(lib().mirhi_device_kernel_time(self.handle, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def timeline(self):
        """Every timed dispatch since the last reset: list of (kernel, lane, begin_us, end_us) on one GPU time axis."""
        n = C.c_uint32(0)
        check(lib().mirhi_device_timeline(self.handle, None, 0, C.byref(n)))
        arr = (DispatchTime * max(1, n.value))()
        check(lib().mirhi_device_timeline(self.handle, arr, n.value, C.byref(n)))
        return [(arr[i].kernel, arr[i].lane, arr[i].begin_us, arr[i].end_us) for i in range(n.value)]

    def fragment_stats(self):
        """(shaded pixels, covered fragments, scopes) accumulated under Profile.FRAGMENTS since the last reset."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().mirhi_device_fragment_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def reset_kernel_times(self):
        check(lib().mirhi_device_reset_kernel_times(self.handle))

    def stats(self) -> DeviceStats:
        s = DeviceStats()
        check(lib().mirhi_device_get_stats(self.handle, C.byref(s)))
        return s

    def dispatch_path(self) -> str:
        """'native: ...' or 'hip: <why>' (mirhi_device_dispatch_path)."""
        buf = C.create_string_buffer(512)
        check(lib().mirhi_device_dispatch_path(self.handle, buf, 512))
        return buf.value.decode()

    def measure_roundtrip(self, lane: int = 0, reps: int = 200):
        """(empty-kernel round trip, barrier-packet round trip) in microseconds on queue lane `lane` (mirhi_device_measure_roundtrip)."""
        out = (C.c_double * 2)()
        check(lib().mirhi_device_measure_roundtrip(self.handle, lane, reps, out))
        return out[0], out[1]

    def set_native_dispatch(self, enable: bool):
        check(lib().mirhi_device_set_native_dispatch(self.handle, 1 if enable else 0))

    def submit(self, cmds: Sequence["CommandBuffer"], fence: Optional["Fence"] = None):
        """vkQueueSubmit (crates/renderer/src/renderer.rs:407-424)."""
        arr = (C.c_void_p * len(cmds))(*[c.handle for c in cmds])
        check(lib().mirhi_queue_submit(self.handle, len(cmds), arr, fence.handle if fence else None))

    def destroy(self):
        if self.handle:
            check(lib().mirhi_device_destroy(self.handle))
            self.handle = None


class Buffer:
    """rhi::Buffer (crates/rhi/src/buffer.rs:149-417)."""

    def __init__(self, device: Device, usage: int, size: int):
        h = C.c_void_p()
        check(lib().mirhi_buffer_create(device.handle, usage, size, C.byref(h)))
        self.handle, self.device = h, device

    @classmethod
    def new_with_data(cls, device: Device, usage: int, data) -> "Buffer":
        arr = _as_bytes(data)
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(lib().mirhi_buffer_create_with_data(device.handle, usage, arr.ctypes.data, arr.size, C.byref(h)))
        self.handle, self.device = h, device
        return self

    @classmethod
    def wrap(cls, device: Device, usage: int, device_ptr: int, size: int) -> "Buffer":
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(lib().mirhi_buffer_wrap_device_memory(device.handle, usage, C.c_void_p(device_ptr), size, C.byref(h)))
        self.handle, self.device = h, device
        return self

    def write_data(self, offset: int, data):
        arr = _as_bytes(data)
        check(lib().mirhi_buffer_write(self.handle, offset, arr.ctypes.data if arr.size else None, arr.size))

    def upload(self, data):
        self.write_data(0, data)

    def upload_via_staging(self, data):
        arr = _as_bytes(data)
        check(lib().mirhi_buffer_upload_via_staging(self.handle, arr.ctypes.data if arr.size else None, arr.size))

    def read(self, offset: int, size: int) -> np.ndarray:
        out = np.empty(size, dtype=np.uint8)
        check(lib().mirhi_buffer_read(self.handle, offset, out.ctypes.data, size))
        return out

    def size(self) -> int:
        return lib().mirhi_buffer_size(self.handle)

    def usage(self) -> int:
        return lib().mirhi_buffer_usage_of(self.handle)

    def destroy(self):
        if self.handle:
            check(lib().mirhi_buffer_destroy(self.handle))
            self.handle = None


class Image:
    """Colour target / DepthBuffer (crates/renderer/src/depth_buffer.rs:117-243) / sampled texture."""
    is_cube = False     # True on what create_cube returns

    def __init__(self, device: Device, width: int, height: int, fmt: int, device_ptr: Optional[int] = None):
        h = C.c_void_p()
        if device_ptr is None:
            check(lib().mirhi_image_create(device.handle, width, height, fmt, C.byref(h)))
        else:
            check(lib().mirhi_image_wrap_device_memory(device.handle, width, height, fmt, C.c_void_p(device_ptr), C.byref(h)))
        self.handle, self.device, self.width, self.height, self.format = h, device, width, height, fmt

    @classmethod
    def _adopt(cls, handle, device, width, height, fmt) -> "Image":
        img = cls.__new__(cls)
        img.handle, img.device, img.width, img.height, img.format = handle, device, width, height, fmt
        return img

    @classmethod
    def array(cls, device: Device, width: int, height: int, layers: int, fmt: int) -> "Image":
        """mirhi_image_create_array: `layers` tightly packed width x height levels in one allocation (D32_SFLOAT only)."""
        h = C.c_void_p()
        check(lib().mirhi_image_create_array(device.handle, width, height, layers, fmt, C.byref(h)))
        return cls._adopt(h, device, width, height, fmt)

    @classmethod
    def multisampled(cls, device: Device, width: int, height: int, fmt: int, samples: int = 4) -> "Image":
        """mirhi_image_create_multisampled: the transient attachment of a 4x multisampled scope (include/mirhi.h "4x MSAA").  It owns no memory and is
        nothing but an attachment: CommandBuffer.begin_rendering_resolve takes it with a resolve target."""
        h = C.c_void_p()
        check(lib().mirhi_image_create_multisampled(device.handle, width, height, fmt, samples, C.byref(h)))
        return cls._adopt(h, device, width, height, fmt)

    @property
    def samples(self) -> int:
        return int(lib().mirhi_image_samples(self.handle))

    @classmethod
    def create_cube(cls, device: Device, size: int, levels: int = 1, fmt: int = Format.R32G32B32A32_SFLOAT, seamless: bool = False) -> "Image":
        """mirhi_image_create_cube: six faces and `levels` mip levels in one allocation (R32G32B32A32_SFLOAT only); level-major, then
        face-major (+X, -X, +Y, -Y, +Z, -Z), then row-major.  seamless=True: set_cube_seamless(True) on the new cube."""
        h = C.c_void_p()
        check(lib().mirhi_image_create_cube(device.handle, size, levels, fmt, C.byref(h)))
        img = cls._adopt(h, device, size, size, fmt)
        img.is_cube = True
        if seamless:
            img.set_cube_seamless(True)
        return img

    def set_cube_seamless(self, enable=True):
        """mirhi_image_set_cube_seamless: lookups in this cube filter across face edges and corners (include/mirhi.h "The sampler"), for draws
        recorded afterwards and for the precompute passes that read it from their next call on.  True / False, or 0 / 1 as the C call takes it."""
        check(lib().mirhi_image_set_cube_seamless(self.handle, int(enable)))

    @property
    def cube_seamless(self) -> bool:
        return bool(lib().mirhi_image_cube_seamless(self.handle))

    def cube_levels(self, packed=None):
        """The levels of a cube's packed chain (default: read it back) as views [6, n >> l, n >> l, 4] of that one array."""
        packed = self.read() if packed is None else packed
        return ibl.unpack_cube(packed, self.width, self.mip_levels)

    def cube_face(self, level: int, face: int, packed=None) -> np.ndarray:
        return self.cube_levels(packed)[level][face]

    # the IBL precompute passes (include/mirhi.h "IBL precompute"): immediate, finished on return
    def ibl_equirect_to_cube(self, src2d: "Image"):
        """equirect_to_cubemap.hlsl: level 0 of this cube from the 2-D equirectangular image."""
        check(lib().mirhi_ibl_equirect_to_cube(src2d.handle, self.handle))

    def ibl_equirect_to_cube_rgbe(self, rgbe8: "Image"):
        """mirhi_ibl_equirect_to_cube_rgbe: level 0 of this cube from a 2-D R8G8B8A8_UNORM image holding Radiance RGBE bytes (Image.from_hdr)."""
        check(lib().mirhi_ibl_equirect_to_cube_rgbe(rgbe8.handle, self.handle))

    def expand_rgbe(self, rgbe8: "Image"):
        """mirhi_image_expand_rgbe: this 2-D R32G32B32A32_SFLOAT image receives the exact float texels of the RGBE image of the same extent."""
        check(lib().mirhi_image_expand_rgbe(rgbe8.handle, self.handle))

    @classmethod
    def from_hdr(cls, device: Device, hdr) -> "Image":
        """The R8G8B8A8_UNORM image of an images.HdrImage's RGBE bytes (images.decode_hdr / load_hdr), uploaded."""
        img = cls(device, hdr.width, hdr.height, Format.R8G8B8A8_UNORM)
        try:
            img.upload(np.ascontiguousarray(hdr.rgbe, dtype=np.uint8))
        except Exception:
            img.destroy()
            raise
        return img

    def ibl_cube_generate_mips(self):
        check(lib().mirhi_ibl_cube_generate_mips(self.handle))

    def ibl_irradiance(self, env: "Image"):
        """irradiance_map.hlsl: level 0 of this cube from the environment cube."""
        check(lib().mirhi_ibl_irradiance(env.handle, self.handle))

    def ibl_prefilter(self, env: "Image", sample_count: int = 1024):
        """prefilter_map.hlsl: every level of this cube from the environment cube's chain."""
        check(lib().mirhi_ibl_prefilter(env.handle, self.handle, int(sample_count)))

    def ibl_brdf_lut(self):
        """brdf_lut.hlsl: this square 2-D image receives (A, B, 0, 1)."""
        check(lib().mirhi_ibl_brdf_lut(self.handle))

    def layer_view(self, layer: int) -> "Image":
        """mirhi_image_create_layer_view: a non-owning 2-D image of one layer (destroy it before the array)."""
        h = C.c_void_p()
        check(lib().mirhi_image_create_layer_view(self.handle, layer, C.byref(h)))
        return Image._adopt(h, self.device, self.width, self.height, self.format)

    @property
    def layers(self) -> int:
        return int(lib().mirhi_image_layers(self.handle))

    def upload(self, data):
        arr = _as_bytes(data)
        check(lib().mirhi_image_upload(self.handle, arr.ctypes.data, arr.size))

    def generate_mips(self):
        """Full mip chain from level 0 (include/mirhi.h); the image is sampled trilinearly from then on."""
        check(lib().mirhi_image_generate_mips(self.handle))

    @property
    def mip_levels(self) -> int:
        return int(lib().mirhi_image_mip_levels(self.handle))

    def set_max_anisotropy(self, max_anisotropy: int):
        """Sampler state of a texture with a mip chain (include/mirhi.h): 1 = trilinear, up to 16 = anisotropic."""
        check(lib().mirhi_image_set_max_anisotropy(self.handle, int(max_anisotropy)))

    @property
    def max_anisotropy(self) -> int:
        return int(lib().mirhi_image_max_anisotropy(self.handle))

    def set_sampler(self, desc=None, **fields):
        """Sampler state of a material texture (include/mirhi.h mirhi_image_set_sampler), for draws recorded afterwards: a SamplerDesc, or its
        fields by name (address_u, address_v, mag_filter, min_filter, mip_mode; those not named are the default's)."""
        if desc is None:
            desc = SamplerDesc()
            lib().mirhi_sampler_desc_default(C.byref(desc))
            for k, v in fields.items():
                if k not in dict(SamplerDesc._fields_):
                    raise TypeError(f"SamplerDesc has no field {k!r}")
                setattr(desc, k, int(v))
        elif fields:
            raise TypeError("pass a SamplerDesc or fields by name, not both")
        check(lib().mirhi_image_set_sampler(self.handle, C.byref(desc)))

    @property
    def sampler(self) -> SamplerDesc:
        desc = SamplerDesc()
        check(lib().mirhi_image_sampler(self.handle, C.byref(desc)))
        return desc

    def read(self) -> np.ndarray:
        n = lib().mirhi_image_size_bytes(self.handle)
        raw = np.empty(n, dtype=np.uint8)
        check(lib().mirhi_image_read(self.handle, raw.ctypes.data, n))
        if self.is_cube:     # the packed chain, [texels, 4]: cube_levels() gives the level / face views
            return raw.view(np.float32).reshape(-1, 4)
        layers = self.layers
        if layers > 1:      # an array (D32_SFLOAT): the layers in order
            return raw.view(np.float32).reshape(layers, self.height, self.width)
        if self.format == Format.R32G32B32A32_SFLOAT:
            return raw.view(np.float32).reshape(self.height, self.width, 4)
        if self.format == Format.D32_SFLOAT:
            return raw.view(np.float32).reshape(self.height, self.width)
        if self.format == Format.R32_UINT:
            return raw.view(np.uint32).reshape(self.height, self.width)
        return raw.reshape(self.height, self.width, 4)

    def destroy(self):
        if self.handle:
            check(lib().mirhi_image_destroy(self.handle))
            self.handle = None


class GraphicsPipelineBuilder:
    """crates/rhi/src/pipeline.rs:590-1059 -- same setter names, same defaults, same build() errors."""

    def __init__(self):
        self.desc = PipelineDesc()
        self.bias = None        # depth_bias(): the factors, built through mirhi_pipeline_create_with_depth_bias
        lib().mirhi_pipeline_desc_default(C.byref(self.desc))

    def vertex_shader(self, program: int):
        self.desc.vertex_program = program
        return self

    def fragment_shader(self, program: int):
        self.desc.fragment_program = program
        return self

    def vertex_binding(self, stride: int):
        self.desc.vertex_stride = stride
        return self

    def vertex_attributes(self, offsets: Sequence[int]):
        self.desc.attribute_count = len(offsets)
        for i, o in enumerate(offsets[:4]):
            self.desc.attribute_offsets[i] = o
        return self

    def topology(self, t: int):
        self.desc.topology = t
        return self

    def polygon_mode(self, m: int):
        self.desc.polygon_mode = m
        return self

    def cull_mode(self, m: int):
        self.desc.cull_mode = m
        return self

    def front_face(self, f: int):
        self.desc.front_face = f
        return self

    def depth_test_enable(self, e: bool):
        self.desc.depth_test_enable = int(e)
        return self

    def depth_write_enable(self, e: bool):
        self.desc.depth_write_enable = int(e)
        return self

    def depth_compare_op(self, op: int):
        self.desc.depth_compare_op = op
        return self

    def blend_enable(self, e: bool):
        self.desc.blend_enable = int(e)
        return self

    def depth_clamp_enable(self, e: bool):
        """pipeline.rs:769: no near / far clipping, fragment depth clamped to [0, 1]."""
        self.desc.depth_clamp_enable = int(e)
        return self

    def depth_bias(self, constant_factor: float, clamp: float, slope_factor: float):
        """pipeline.rs:781-788: enables depth bias with the three factors."""
        self.desc.depth_bias_enable = 1
        self.bias = DepthBias(constant_factor, clamp, slope_factor)
        return self

    def rasterization_samples(self, samples: int):
        """pipeline.rs:796: 1, or 4 for a pipeline that draws in 4x multisampled scopes (include/mirhi.h "4x MSAA")."""
        self.desc.rasterization_samples = int(samples)
        return self

    def fragment_discard_enable(self, e: bool):
        """Pipelines of alpha-masked MODEL_PBR materials (model_pbr.hlsl:176-179 `discard`): per-fragment, ordered resolve."""
        self.desc.fragment_discard_enable = int(e)
        return self

    def color_blend_attachment(self, src_color, dst_color, color_op, src_alpha, dst_alpha, alpha_op, write_mask=0xF):
        """ColorBlendAttachment (pipeline.rs:478-531) with blending enabled."""
        d = self.desc
        d.blend_enable = 1
        d.src_color_blend_factor, d.dst_color_blend_factor, d.color_blend_op = src_color, dst_color, color_op
        d.src_alpha_blend_factor, d.dst_alpha_blend_factor, d.alpha_blend_op = src_alpha, dst_alpha, alpha_op
        d.color_write_mask = write_mask
        return self

    def alpha_blend(self):
        """ColorBlendAttachment::alpha_blend() (pipeline.rs:518-529): src * src_alpha + dst * (1 - src_alpha)."""
        return self.color_blend_attachment(BlendFactor.SrcAlpha, BlendFactor.OneMinusSrcAlpha, BlendOp.Add, BlendFactor.One, BlendFactor.Zero, BlendOp.Add)

    def color_attachment_format(self, fmt: int):
        n = self.desc.color_attachment_count
        self.desc.color_attachment_formats[n] = fmt
        self.desc.color_attachment_count = n + 1
        return self

    def depth_attachment_format(self, fmt: int):
        self.desc.depth_attachment_format = fmt
        return self

    def build(self, device: Device) -> "Pipeline":
        h = C.c_void_p()
        if self.bias is not None:
            check(lib().mirhi_pipeline_create_with_depth_bias(device.handle, C.byref(self.desc), C.byref(self.bias), C.byref(h)))
        else:
            check(lib().mirhi_pipeline_create(device.handle, C.byref(self.desc), C.byref(h)))
        return Pipeline(h)


class Pipeline:
    def __init__(self, handle):
        self.handle = handle

    def destroy(self):
        if self.handle:
            check(lib().mirhi_pipeline_destroy(self.handle))
            self.handle = None


TRIANGLE_VERTEX_STRIDE, TRIANGLE_VERTEX_OFFSETS = 24, (0, 12)        # vertex.rs:35-61
SHADOW_VERTEX_OFFSETS = (0,)                                         # vertex/shadow.hlsl:13-16: position only, any stride >= 12
VERTEX_STRIDE, VERTEX_OFFSETS = 48, (0, 12, 24, 32)                  # vertex.rs:130-170


def rendering_info(color=None, clear_color=(0.0, 0.0, 0.0, 1.0), color_load_op=LoadOp.CLEAR, depth=None, clear_depth: float = 1.0,
                   depth_load_op=LoadOp.CLEAR, depth_store_op=StoreOp.DONT_CARE, prim_id=None, render_area=None) -> RenderingInfo:
    """The mirhi_rendering_info that CommandBuffer.begin_rendering records: the library's defaults, then the arguments.
    render_area: None (the full extent) or (x, y, width, height).  Test plumbing: lets a test without a device see what the keyword fills in."""
    info = RenderingInfo()
    lib().mirhi_rendering_info_default(C.byref(info))
    info.color_image = color.handle if color is not None else None
    info.color_load_op = color_load_op
    info.clear_color = (C.c_float * 4)(*clear_color)
    if depth is not None:
        info.depth_image = depth.handle
    info.depth_load_op, info.depth_store_op, info.clear_depth = depth_load_op, depth_store_op, clear_depth
    if prim_id is not None:
        info.prim_id_image = prim_id.handle
    if render_area is not None:
        x, y, w, h = (int(v) for v in render_area)
        info.render_area = (C.c_int32 * 4)(x, y, w, h)
    return info


def resolve_info(color_resolve=None, depth_resolve=None, color_mode=None, depth_mode=None) -> ResolveInfo:
    """The mirhi_resolve_info of CommandBuffer.begin_rendering_resolve: an image names its usual mode (AVERAGE for colour, SAMPLE_ZERO for depth) unless
    a mode is given."""
    r = ResolveInfo()
    lib().mirhi_resolve_info_default(C.byref(r))
    if color_resolve is not None:
        r.color_resolve_image = color_resolve.handle
    if depth_resolve is not None:
        r.depth_resolve_image = depth_resolve.handle
    r.color_resolve_mode = color_mode if color_mode is not None else (ResolveMode.AVERAGE if color_resolve is not None else ResolveMode.NONE)
    r.depth_resolve_mode = depth_mode if depth_mode is not None else (ResolveMode.SAMPLE_ZERO if depth_resolve is not None else ResolveMode.NONE)
    return r


def multiview_info(view_mask: int, view_constants=None, view_offset: int = 0, view_stride: int = 64) -> MultiviewInfo:
    """The mirhi_multiview_info of CommandBuffer.begin_rendering_multiview: the library's defaults, then the arguments."""
    m = MultiviewInfo()
    lib().mirhi_multiview_info_default(C.byref(m))
    m.view_mask = int(view_mask)
    m.view_constants = view_constants.handle if view_constants is not None else None
    m.view_offset, m.view_stride = int(view_offset), int(view_stride)
    return m


class ColorAttachment:
    """rhi::ColorAttachment (rendering.rs:65-115): the image with its ops; with_resolve (rendering.rs:238) names the 1x image a multisampled one resolves to."""

    def __init__(self, image: "Image", load_op=LoadOp.CLEAR, store_op=StoreOp.STORE, clear_color=(0.0, 0.0, 0.0, 1.0)):
        self.image, self.load_op, self.store_op, self.clear_color = image, load_op, store_op, tuple(clear_color)
        self.resolve_image, self.resolve_mode = None, ResolveMode.NONE

    def with_resolve(self, image: "Image", mode: int = ResolveMode.AVERAGE):
        self.resolve_image, self.resolve_mode = image, mode
        self.store_op = StoreOp.DONT_CARE      # (the multisampled contents are transient: what is kept is the resolve)
        return self


class DepthAttachment:
    """rhi::DepthAttachment (rendering.rs:319-370); with_resolve (rendering.rs:477): the 1x D32_SFLOAT image sample 0's depth is written to."""

    def __init__(self, image: "Image", load_op=LoadOp.CLEAR, store_op=StoreOp.DONT_CARE, clear_depth: float = 1.0):
        self.image, self.load_op, self.store_op, self.clear_depth = image, load_op, store_op, clear_depth
        self.resolve_image, self.resolve_mode = None, ResolveMode.NONE

    def with_resolve(self, image: "Image", mode: int = ResolveMode.SAMPLE_ZERO):
        self.resolve_image, self.resolve_mode = image, mode
        return self


def attachment_infos(color: ColorAttachment, depth: Optional[DepthAttachment] = None, prim_id=None, render_area=None):
    """(RenderingInfo, ResolveInfo) of a scope given by attachments.  Test plumbing as rendering_info is."""
    info = rendering_info(color.image, color.clear_color, color.load_op, depth.image if depth else None, depth.clear_depth if depth else 1.0,
                          depth.load_op if depth else LoadOp.CLEAR, depth.store_op if depth else StoreOp.DONT_CARE, prim_id, render_area)
    info.color_store_op = color.store_op
    res = resolve_info(color.resolve_image, depth.resolve_image if depth else None, color.resolve_mode, depth.resolve_mode if depth else ResolveMode.NONE)
    return info, res


class CommandBuffer:
    """rhi::CommandBuffer (crates/rhi/src/command.rs:297-628)."""

    def __init__(self, device: Device):
        h = C.c_void_p()
        check(lib().mirhi_cmd_create(device.handle, C.byref(h)))
        self.handle, self.device = h, device

    def begin(self):
        check(lib().mirhi_cmd_begin(self.handle))

    def begin_reusable(self):
        check(lib().mirhi_cmd_begin_reusable(self.handle))

    def end(self):
        check(lib().mirhi_cmd_end(self.handle))

    def reset(self):
        check(lib().mirhi_cmd_reset(self.handle))

    def begin_rendering(self, color: Optional[Image], clear_color=(0.0, 0.0, 0.0, 1.0), color_load_op=LoadOp.CLEAR,
                        depth: Optional[Image] = None, clear_depth: float = 1.0, depth_load_op=LoadOp.CLEAR,
                        depth_store_op=StoreOp.DONT_CARE, prim_id: Optional[Image] = None, render_area=None):
        """color=None with a depth image: a depth-only scope (Program.SHADOW draws).
        render_area=(x, y, width, height) in pixels of the attachment: the scope loads, clears, draws and stores inside that rectangle only
        (include/mirhi.h, mirhi_rendering_info::render_area); None: the full extent."""
        info = rendering_info(color, clear_color, color_load_op, depth, clear_depth, depth_load_op, depth_store_op, prim_id, render_area)
        check(lib().mirhi_cmd_begin_rendering(self.handle, C.byref(info)))

    def begin_rendering_resolve(self, color: Image, color_resolve: Optional[Image], clear_color=(0.0, 0.0, 0.0, 1.0), depth: Optional[Image] = None,
                                depth_resolve: Optional[Image] = None, clear_depth: float = 1.0, prim_id: Optional[Image] = None, color_load_op=LoadOp.CLEAR,
                                color_store_op=StoreOp.DONT_CARE, depth_load_op=LoadOp.CLEAR, depth_store_op=StoreOp.DONT_CARE, color_mode=None, depth_mode=None,
                                render_area=None):
        """mirhi_cmd_begin_rendering_resolve: a 4x multisampled scope (color: Image.multisampled) whose averaged colour goes to color_resolve and, optionally,
        whose sample-0 depth goes to depth_resolve.  prim_id: R32_UINT of 4 * width x height, texel (4 px + s, py) the winner of sample s."""
        info = rendering_info(color, clear_color, color_load_op, depth, clear_depth, depth_load_op, depth_store_op, prim_id, render_area)
        info.color_store_op = color_store_op
        res = resolve_info(color_resolve, depth_resolve, color_mode, depth_mode)
        check(lib().mirhi_cmd_begin_rendering_resolve(self.handle, C.byref(info), C.byref(res)))

    def begin_rendering_multiview(self, depth_array: Optional[Image], view_mask: int, view_constants: Optional["Buffer"], view_offset: int = 0, view_stride: int = 64,
                                  clear_depth: float = 1.0, depth_load_op=LoadOp.CLEAR, depth_store_op=StoreOp.STORE, color: Optional[Image] = None,
                                  prim_id: Optional[Image] = None, render_area=None):
        """mirhi_cmd_begin_rendering_multiview: ONE depth-only scope whose Program.SHADOW draws are rendered once per set bit v of view_mask into layer v of
        depth_array (Image.array), with the light matrix of view v read at view_offset + v * view_stride of view_constants when the scope executes (the draw's own
        CAMERA block still supplies `model` @64).  color / prim_id / render_area exist to show the refusals."""
        info = rendering_info(color, depth=depth_array, clear_depth=clear_depth, depth_load_op=depth_load_op, depth_store_op=depth_store_op, prim_id=prim_id,
                              render_area=render_area)
        mv = multiview_info(view_mask, view_constants, view_offset, view_stride)
        check(lib().mirhi_cmd_begin_rendering_multiview(self.handle, C.byref(info), C.byref(mv)))

    def begin_rendering_attachments(self, color: ColorAttachment, depth: Optional[DepthAttachment] = None, prim_id: Optional[Image] = None, render_area=None):
        """The scope given by attachments, as the reference's RenderingConfig takes them; a with_resolve attachment makes it a multisampled scope."""
        info, res = attachment_infos(color, depth, prim_id, render_area)
        check(lib().mirhi_cmd_begin_rendering_resolve(self.handle, C.byref(info), C.byref(res)))

    def end_rendering(self):
        check(lib().mirhi_cmd_end_rendering(self.handle))

    def bind_pipeline(self, p: Pipeline):
        check(lib().mirhi_cmd_bind_pipeline(self.handle, p.handle))

    def bind_vertex_buffers(self, first_binding: int, buffers: Sequence[Buffer], offsets: Sequence[int]):
        arr = (C.c_void_p * len(buffers))(*[b.handle for b in buffers])
        offs = (C.c_uint64 * len(offsets))(*offsets)
        check(lib().mirhi_cmd_bind_vertex_buffers(self.handle, first_binding, len(buffers), arr, offs))

    def bind_index_buffer(self, buffer: Buffer, offset: int, index_type: int):
        check(lib().mirhi_cmd_bind_index_buffer(self.handle, buffer.handle, offset, index_type))

    def bind_uniform(self, slot: int, buffer: Buffer, offset: int = 0, range_: int = 0):
        check(lib().mirhi_cmd_bind_uniform(self.handle, slot, buffer.handle, offset, range_))

    def bind_texture(self, slot: int, image: Optional[Image]):
        check(lib().mirhi_cmd_bind_texture(self.handle, slot, image.handle if image else None))

    def bind_shadow_cascades(self, array: Optional[Image], params: Optional[Buffer] = None, offset: int = 0, range_: int = 0, blend_threshold: float = 0.0):
        """mirhi_cmd_bind_shadow_cascades: the four-layer D32 array and its CSMParams (scenes.csm_ubo); array=None unbinds.
        blend_threshold other than the default goes through mirhi_cmd_bind_shadow_cascades_blended (CalculateShadowCSMBlended's blendThreshold, in [0, 1])."""
        if isinstance(blend_threshold, (int, float)) and blend_threshold == 0.0:
            check(lib().mirhi_cmd_bind_shadow_cascades(self.handle, array.handle if array else None, params.handle if params else None, offset, range_))
        else:
            self.bind_shadow_cascades_blended(array, params, offset, range_, blend_threshold)

    def bind_shadow_cascades_blended(self, array: Optional[Image], params: Optional[Buffer] = None, offset: int = 0, range_: int = 0, blend_threshold: float = 0.0):
        """mirhi_cmd_bind_shadow_cascades_blended, whatever the threshold (0.0 records what bind_shadow_cascades records)."""
        check(lib().mirhi_cmd_bind_shadow_cascades_blended(self.handle, array.handle if array else None, params.handle if params else None, offset, range_,
                                                           float(blend_threshold)))

    def bind_ibl(self, irradiance: Optional[Image], prefiltered: Optional[Image] = None, brdf_lut: Optional[Image] = None):
        """mirhi_cmd_bind_ibl: the irradiance cube, the prefiltered cube and the BRDF LUT Program.MODEL_PBR_IBL draws sample; all None unbinds."""
        check(lib().mirhi_cmd_bind_ibl(self.handle, *(i.handle if i is not None else None for i in (irradiance, prefiltered, brdf_lut))))

    def bind_skybox(self, environment: Optional[Image]):
        """mirhi_cmd_bind_skybox: the environment cube Program.SKYBOX draws sample; None unbinds."""
        check(lib().mirhi_cmd_bind_skybox(self.handle, environment.handle if environment is not None else None))

    def set_viewport(self, x, y, width, height, min_depth=0.0, max_depth=1.0):
        vp = Viewport(x, y, width, height, min_depth, max_depth)
        check(lib().mirhi_cmd_set_viewport(self.handle, C.byref(vp)))

    def set_scissor(self, x, y, width, height):
        sc = Rect2D(x, y, width, height)
        check(lib().mirhi_cmd_set_scissor(self.handle, C.byref(sc)))

    def draw_indirect(self, buffer: Buffer, offset: int, draw_count: int, stride: int):
        check(lib().mirhi_cmd_draw_indirect(self.handle, buffer.handle, offset, draw_count, stride))

    def draw_indexed_indirect(self, buffer: Buffer, offset: int, draw_count: int, stride: int):
        check(lib().mirhi_cmd_draw_indexed_indirect(self.handle, buffer.handle, offset, draw_count, stride))

    def push_constants(self, stage_flags: int, offset: int, data: bytes):
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data) if data else None
        check(lib().mirhi_cmd_push_constants(self.handle, stage_flags, offset, buf, len(data)))

    # ---- transfer commands (include/mirhi.h "Transfer commands"): recorded outside a rendering scope; regions are the structures above or tuples ----
    def copy_buffer(self, src: Buffer, dst: Buffer, regions):
        """regions: BufferCopy or (src_offset, dst_offset, size)"""
        arr, n = _regions(BufferCopy, regions)
        check(lib().mirhi_cmd_copy_buffer(self.handle, src.handle, dst.handle, n, arr))

    def copy_buffer_to_image(self, src: Buffer, dst: Image, regions):
        """regions: BufferImageCopy or (buffer_offset, buffer_row_length, buffer_image_height, mip_level, (x, y), (width, height))"""
        arr, n = _regions(BufferImageCopy, regions)
        check(lib().mirhi_cmd_copy_buffer_to_image(self.handle, src.handle, dst.handle, n, arr))

    def copy_image_to_buffer(self, src: Image, dst: Buffer, regions):
        arr, n = _regions(BufferImageCopy, regions)
        check(lib().mirhi_cmd_copy_image_to_buffer(self.handle, src.handle, dst.handle, n, arr))

    def copy_image(self, src: Image, dst: Image, regions):
        """regions: ImageCopy or (src_mip_level, (sx, sy), dst_mip_level, (dx, dy), (width, height))"""
        arr, n = _regions(ImageCopy, regions)
        check(lib().mirhi_cmd_copy_image(self.handle, src.handle, dst.handle, n, arr))

    def blit_image(self, src: Image, dst: Image, regions, filter: int = Filter.NEAREST):
        """regions: ImageBlit or (src_mip_level, ((x0, y0), (x1, y1)), dst_mip_level, ((x0, y0), (x1, y1))); reversed corners flip"""
        arr, n = _regions(ImageBlit, regions)
        check(lib().mirhi_cmd_blit_image(self.handle, src.handle, dst.handle, n, arr, filter))

    def clear_color_image(self, image: Image, color):
        check(lib().mirhi_cmd_clear_color_image(self.handle, image.handle, (C.c_float * 4)(*[float(c) for c in color])))

    def clear_depth_stencil_image(self, image: Image, depth: float):
        check(lib().mirhi_cmd_clear_depth_stencil_image(self.handle, image.handle, float(depth)))

    def set_queue_lane(self, lane: int):
        check(lib().mirhi_cmd_set_queue_lane(self.handle, lane))

    def draw(self, vertex_count, instance_count=1, first_vertex=0, first_instance=0):
        check(lib().mirhi_cmd_draw(self.handle, vertex_count, instance_count, first_vertex, first_instance))

    def draw_indexed(self, index_count, instance_count=1, first_index=0, vertex_offset=0, first_instance=0):
        check(lib().mirhi_cmd_draw_indexed(self.handle, index_count, instance_count, first_index, vertex_offset, first_instance))

    def destroy(self):
        if self.handle:
            check(lib().mirhi_cmd_destroy(self.handle))
            self.handle = None


class Fence:
    """rhi::Fence (crates/rhi/src/sync.rs:168-298)."""

    def __init__(self, device: Device, signaled: bool = False):
        h = C.c_void_p()
        check(lib().mirhi_fence_create(device.handle, int(signaled), C.byref(h)))
        self.handle = h

    def wait(self, timeout_ns: int = 2 ** 64 - 1):
        check(lib().mirhi_fence_wait(self.handle, timeout_ns))

    def reset(self):
        check(lib().mirhi_fence_reset(self.handle))

    def is_signaled(self) -> bool:
        return lib().mirhi_fence_status(self.handle) == OK

    def destroy(self):
        if self.handle:
            check(lib().mirhi_fence_destroy(self.handle))
            self.handle = None


class Comm:
    """Exchange of the finished bands of a tile-row split over RCCL (include/mirhi.h; no reference counterpart:
    crates/rhi/src/device.rs:61-77 drives a single VkDevice)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        check(lib().mirhi_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, device: Device, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == COMM_ID_BYTES
        h = C.c_void_p()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        check(lib().mirhi_comm_create(device.handle, buf, rank, world, C.byref(h)))
        self.handle, self.device = h, device

    def world(self) -> int:
        return lib().mirhi_comm_world(self.handle)

    def rank(self) -> int:
        return lib().mirhi_comm_rank(self.handle)

    def all_gather_bands(self, frame: Image, after: Optional["CommandBuffer"] = None, algo: int = GatherAlgo.DIRECT):
        check(lib().mirhi_comm_all_gather_bands(self.handle, frame.handle, after.handle if after else None, algo))

    def destroy(self):
        if self.handle:
            check(lib().mirhi_comm_destroy(self.handle))
            self.handle = None


# ---- scene helper: records a scenes.Scene the way crates/renderer records a frame ---------------------------
def _depth_state(builder, draw, spec=None):
    """The depth_bias=(constant, clamp, slope) and depth_clamp=True pipeline arguments of a scenes.DrawSpec -- a shadow caster without its own takes
    its ShadowSpec's / CascadeSpec's -- applied to `builder`; with builder None: the pair itself (a pipeline cache key)."""
    bias = draw.depth_bias if draw.depth_bias is not None else getattr(spec, "depth_bias", None)
    clamp = bool(draw.depth_clamp or getattr(spec, "depth_clamp", False))
    if builder is None:
        return (tuple(bias) if bias is not None else None, clamp)
    if bias is not None:
        builder.depth_bias(*bias)
    if clamp:
        builder.depth_clamp_enable(True)
    return builder


class SceneResources:
    """Uploads a scenes.Scene once (vertex/index/uniform buffers, textures, pipelines) and records it into
    a reusable command buffer, mirroring Renderer::create_triangle_resources + record_commands
    (crates/renderer/src/renderer.rs:205-260,452-557)."""

    def __init__(self, device: Device, scene, color_format: int = Format.R32G32B32A32_SFLOAT, want_prim: bool = False,
                 want_depth: bool = False, color_image: Optional[Image] = None, wrap_buffers=None,
                 color_load_op: int = LoadOp.CLEAR, shadow_cmd: bool = False, shadow_map: Optional[Image] = None,
                 cascade_array: Optional[Image] = None, ibl_images: Optional[Sequence[Image]] = None, sky_image: Optional[Image] = None,
                 depth_image: Optional[Image] = None, prim_image: Optional[Image] = None, depth_load_op: int = LoadOp.CLEAR, samples: int = 1,
                 multiview: bool = False):
        """scene.shadow (scenes.ShadowSpec) adds a depth-only shadow scope ahead of the main scope: recorded into the same command
        buffer, or with shadow_cmd=True into a command buffer of its own (self.shadow_cmd; render() submits both, the shadow one first --
        put it on another queue lane with set_queue_lane).  shadow_map: an existing D32 image to render into (shared between frames).
        scene.cascades (scenes.CascadeSpec): four depth-only scopes instead, one per layer view of a D32 array (self.cascade_array, or the
        existing one passed as cascade_array=), in the same command buffer or with shadow_cmd=True in self.shadow_cmd; the MODEL_PBR draws
        sample the array through bind_shadow_cascades, with the spec's blend_threshold.
        scene.ibl (scenes.IblSpec): the IBL set bound for the scene's MODEL_PBR_IBL draws -- the spec's own images, images created here from its
        arrays and uploaded (self.ibl_images, destroyed with the resources), or the existing three passed as ibl_images= (irradiance cube,
        prefiltered cube, BRDF LUT; shared between frames, the caller's to destroy).
        scene.sky (scenes.SkySpec): a Program.SKYBOX draw behind (or with first=True ahead of) the scene's draws; its environment cube is the spec's
        image, one created here from its levels (self.sky_image, destroyed with the resources) or the existing one passed as sky_image=.
        scene.render_area ((x, y, width, height) or None): the main scope's render area (include/mirhi.h, mirhi_rendering_info::render_area).
        depth_image / prim_image / depth_load_op: test plumbing for the render-area tests -- existing attachments to render into, like color_image
        (the caller's to destroy), and the main scope's depth load op, so that a scope can start from prefilled contents.
        samples=4: the main scope is a 4x multisampled one (include/mirhi.h "4x MSAA"): transient multisampled colour and depth images are built here
        (self.ms_color, self.ms_depth), the pipelines get rasterization_samples = 4, and the scope is recorded through begin_rendering_resolve --
        self.color is the colour resolve target, self.depth (want_depth) the sample-0 depth resolve, self.prim (want_prim) the 4 * width x height
        image of per-sample winners, which read() returns as [height, width, 4]."""
        self.device, self.scene = device, scene
        self.samples = int(samples)
        self.multiview = bool(multiview)      # scene.cascades: ONE multiview scope for all cascades (scenes.record_cascades_multiview) instead of one scope per layer view
        self.color_load_op = color_load_op
        self.owns_color = color_image is None
        self.objs = []
        self.color = color_image or Image(device, scene.width, scene.height, color_format)
        self.color_format = self.color.format
        self.depth_load_op = depth_load_op
        self.owns_prim, self.owns_depth = prim_image is None, depth_image is None
        self.prim = prim_image or (Image(device, scene.width * (4 if self.samples == 4 else 1), scene.height, Format.R32_UINT) if want_prim else None)
        self.depth = depth_image or (Image(device, scene.width, scene.height, Format.D32_SFLOAT) if want_depth else None)
        self.ms_color = self.ms_depth = None
        if self.samples != 1:
            self.ms_color = Image.multisampled(device, scene.width, scene.height, self.color_format, self.samples)
            self.ms_depth = Image.multisampled(device, scene.width, scene.height, Format.D32_SFLOAT, self.samples)
            self.objs += [self.ms_color, self.ms_depth]
        self.cmd = CommandBuffer(device)
        self.draw_state = []
        cache = {}

        def buf(usage, data, key=None):
            if data is None:
                return None
            key = key if key is not None else id(data)
            if (usage, key) in cache:
                return cache[(usage, key)]
            arr = _as_bytes(data)
            if arr.size == 0:
                return None
            if wrap_buffers is not None:
                b = wrap_buffers(device, usage, arr)
            else:
                b = Buffer.new_with_data(device, usage, arr)
            cache[(usage, key)] = b
            self.objs.append(b)
            return b

        def tex(t):
            if t is None:
                return None
            if id(t) in cache:
                return cache[id(t)]
            img = Image(device, t.width, t.height, Format.R8G8B8A8_SRGB if t.srgb else Format.R8G8B8A8_UNORM)
            img.upload(np.ascontiguousarray(t.rgba8))
            if t.mips:
                img.generate_mips()
            if getattr(t, "max_anisotropy", 1) > 1:
                img.set_max_anisotropy(t.max_anisotropy)
            state = tuple(int(getattr(t, k, 0)) for k, _ in SamplerDesc._fields_)
            if any(state):
                img.set_sampler(SamplerDesc(*state))
            cache[id(t)] = img
            self.objs.append(img)
            return img

        for d in scene.draws:
            model = d.program != scenes.PROGRAM_TRIANGLE
            b = (GraphicsPipelineBuilder().vertex_shader(Program.MODEL if model else Program.TRIANGLE)
                 .fragment_shader(d.program)
                 .vertex_binding(d.stride)
                 .vertex_attributes(VERTEX_OFFSETS if model else TRIANGLE_VERTEX_OFFSETS)
                 .color_attachment_format(self.color_format)
                 .cull_mode(d.cull_mode).front_face(d.front_face)
                 .depth_test_enable(d.depth_test).depth_write_enable(d.depth_write).depth_compare_op(d.depth_compare))
            if d.depth_test or d.depth_write:
                b.depth_attachment_format(Format.D32_SFLOAT)
            if getattr(d, "blend", None) is not None:
                b.color_blend_attachment(*d.blend)
            if getattr(d, "alpha_test", False):
                b.fragment_discard_enable(True)
            _depth_state(b, d)
            if self.samples != 1:
                b.rasterization_samples(self.samples)
            pipe = b.build(device)
            self.objs.append(pipe)
            st = dict(pipe=pipe, vb=buf(BufferUsage.Vertex, d.vertices),
                      ib=buf(BufferUsage.Index, d.indices) if d.indices is not None else None,
                      camera=buf(BufferUsage.Uniform, d.camera, key=("u", d.camera)),
                      object=buf(BufferUsage.Uniform, d.object, key=("u", d.object)),
                      light=buf(BufferUsage.Uniform, d.light, key=("u", d.light)),
                      material=buf(BufferUsage.Uniform, d.material, key=("u", d.material)),
                      point=buf(BufferUsage.Storage if False else BufferUsage.Uniform, d.point_lights or None, key=("u", d.point_lights)),
                      spot=buf(BufferUsage.Uniform, d.spot_lights or None, key=("u", d.spot_lights)),
                      textures=[tex(t) for t in d.textures], draw=d)
            self.draw_state.append(st)
        self.shadow, self.shadow_cmd, self.shadow_state, self.owns_shadow_map = getattr(scene, "shadow", None), None, [], False
        if self.shadow is not None:
            sh = self.shadow
            self.shadow_map = shadow_map
            if self.shadow_map is None:
                self.shadow_map, self.owns_shadow_map = Image(device, sh.size[0], sh.size[1], Format.D32_SFLOAT), True
            self.shadow_data = buf(BufferUsage.Uniform, sh.params, key=("u", sh.params))
            for c in sh.casters:
                pb = (GraphicsPipelineBuilder().vertex_shader(Program.SHADOW).fragment_shader(Program.SHADOW)
                      .vertex_binding(c.stride).vertex_attributes(SHADOW_VERTEX_OFFSETS)
                      .color_attachment_format(Format.UNDEFINED).depth_attachment_format(Format.D32_SFLOAT)
                      .cull_mode(c.cull_mode).front_face(c.front_face).depth_compare_op(c.depth_compare))
                _depth_state(pb, c, sh)
                pipe = pb.build(device)
                self.objs.append(pipe)
                self.shadow_state.append(dict(pipe=pipe, vb=buf(BufferUsage.Vertex, c.vertices),
                                              ib=buf(BufferUsage.Index, c.indices) if c.indices is not None else None,
                                              camera=buf(BufferUsage.Uniform, c.camera, key=("u", c.camera)), draw=c))
            if shadow_cmd:
                self.shadow_cmd = CommandBuffer(device)
        self.cascades, self.cascade_array, self.cascade_views, self.cascade_state, self.owns_cascade_array = getattr(scene, "cascades", None), None, [], [], False
        if self.cascades is not None:
            assert self.shadow is None, "a scene has a single shadow map or cascades, not both"
            cs = self.cascades
            self.cascade_array = cascade_array
            if self.cascade_array is None:
                self.cascade_array, self.owns_cascade_array = Image.array(device, cs.size[0], cs.size[1], len(cs.casters), Format.D32_SFLOAT), True
            self.cascade_views = [self.cascade_array.layer_view(k) for k in range(len(cs.casters))]
            self.cascade_params = buf(BufferUsage.Uniform, cs.params, key=("u", cs.params))
            self.view_constants = None
            if self.multiview:
                vc = scenes.cascade_view_constants(cs)
                self.view_constants = buf(BufferUsage.Uniform, vc, key=("u", vc))
            for layer in cs.casters:
                states = []
                for c in layer:
                    pkey = ("shadow-pipe", c.stride, c.cull_mode, c.front_face, c.depth_compare, _depth_state(None, c, cs))
                    if pkey not in cache:
                        cache[pkey] = _depth_state(GraphicsPipelineBuilder().vertex_shader(Program.SHADOW).fragment_shader(Program.SHADOW)
                                                   .vertex_binding(c.stride).vertex_attributes(SHADOW_VERTEX_OFFSETS)
                                                   .color_attachment_format(Format.UNDEFINED).depth_attachment_format(Format.D32_SFLOAT)
                                                   .cull_mode(c.cull_mode).front_face(c.front_face).depth_compare_op(c.depth_compare), c, cs).build(device)
                        self.objs.append(cache[pkey])
                    states.append(dict(pipe=cache[pkey], vb=buf(BufferUsage.Vertex, c.vertices),
                                       ib=buf(BufferUsage.Index, c.indices) if c.indices is not None else None,
                                       camera=buf(BufferUsage.Uniform, c.camera, key=("u", c.camera)), draw=c))
                self.cascade_state.append(states)
            if shadow_cmd:
                self.shadow_cmd = CommandBuffer(device)
        self.ibl, self.ibl_images, self.owns_ibl = getattr(scene, "ibl", None), None, False
        if ibl_images is not None:
            self.ibl_images = tuple(ibl_images)
        elif self.ibl is not None and self.ibl.images is not None:
            self.ibl_images = tuple(self.ibl.images)
        elif self.ibl is not None:
            self.ibl_images, self.owns_ibl = self.ibl.create_images(device, Image, Format.R32G32B32A32_SFLOAT), True
        self.sky, self.sky_image, self.owns_sky, self.sky_pipe = getattr(scene, "sky", None), sky_image, False, None
        if self.sky is not None:
            if self.sky_image is None and self.sky.image is not None:
                self.sky_image = self.sky.image
            elif self.sky_image is None:
                self.sky_image, self.owns_sky = self.sky.create_image(device, Image), True
            k = self.sky
            b = (GraphicsPipelineBuilder().vertex_shader(Program.SKYBOX).fragment_shader(Program.SKYBOX).vertex_binding(0).vertex_attributes(())
                 .color_attachment_format(self.color_format).cull_mode(k.cull_mode).front_face(k.front_face)
                 .depth_test_enable(k.depth_test).depth_write_enable(k.depth_write).depth_compare_op(k.depth_compare))
            if k.depth_test or k.depth_write:
                b.depth_attachment_format(Format.D32_SFLOAT)
            self.sky_pipe = b.build(device)
            self.objs.append(self.sky_pipe)
        self.record()

    def _record_sky(self, cmd: "CommandBuffer"):
        s, k = self.scene, self.sky
        cmd.set_viewport(*(k.viewport or (0.0, 0.0, float(s.width), float(s.height), 0.0, 1.0)))
        cmd.set_scissor(*(k.scissor or (0, 0, s.width, s.height)))
        cmd.bind_pipeline(self.sky_pipe)
        cmd.bind_skybox(self.sky_image)
        cmd.push_constants(0, 0, np.ascontiguousarray(k.inv_view_proj, dtype=np.float32).tobytes())
        cmd.draw(3, 1, 0, 0)

    def _record_shadow(self, cmd: "CommandBuffer"):
        if self.cascades is not None and self.multiview:
            scenes.record_cascades_multiview(cmd, self.cascades, self.cascade_array, self.cascade_state[0], self.view_constants)
        elif self.cascades is not None:
            for view, states in zip(self.cascade_views, self.cascade_state):
                self._record_depth_scope(cmd, self.cascades, view, states)
        else:
            self._record_depth_scope(cmd, self.shadow, self.shadow_map, self.shadow_state)

    @staticmethod
    def _record_depth_scope(cmd: "CommandBuffer", sh, target: Image, states):
        w, h = sh.size
        cmd.begin_rendering(None, depth=target, clear_depth=sh.clear_depth, depth_load_op=sh.load_op, depth_store_op=StoreOp.STORE,
                            render_area=getattr(sh, "render_area", None))      # (sh: a ShadowSpec, or a CascadeSpec, which has no area)
        for st in states:
            d = st["draw"]
            cmd.set_viewport(*(d.viewport or (0.0, 0.0, float(w), float(h), 0.0, 1.0)))
            cmd.set_scissor(*(d.scissor or (0, 0, w, h)))
            cmd.bind_pipeline(st["pipe"])
            cmd.bind_vertex_buffers(0, [st["vb"]], [0])
            cmd.bind_uniform(Slot.CAMERA, st["camera"])
            if st["ib"] is not None:
                cmd.bind_index_buffer(st["ib"], 0, IndexType.UINT16 if d.index_type == 2 else IndexType.UINT32)
                cmd.draw_indexed(d.count, 1, d.first, d.vertex_offset, 0)
            else:
                cmd.draw(d.count, 1, d.first, 0)
        cmd.end_rendering()

    def record(self):
        s, cmd = self.scene, self.cmd
        if self.shadow_cmd is not None:
            self.shadow_cmd.begin_reusable()
            self._record_shadow(self.shadow_cmd)
            self.shadow_cmd.end()
        cmd.begin_reusable()
        self.record_scopes(cmd)
        cmd.end()

    def record_scopes(self, cmd: "CommandBuffer"):
        """The scene's scopes (shadow scopes unless they have a command buffer of their own, then the main scope) into `cmd`, which is recording: several
        scenes can share one command buffer."""
        s = self.scene
        if (self.shadow is not None or self.cascades is not None) and self.shadow_cmd is None:
            self._record_shadow(cmd)
        if self.samples != 1:
            cmd.begin_rendering_resolve(self.ms_color, self.color, clear_color=s.clear_color, depth=self.ms_depth, depth_resolve=self.depth, clear_depth=s.clear_depth,
                                        prim_id=self.prim, color_load_op=self.color_load_op, depth_load_op=self.depth_load_op, render_area=s.render_area)
        else:
            cmd.begin_rendering(self.color, clear_color=s.clear_color, color_load_op=self.color_load_op, depth=self.depth, clear_depth=s.clear_depth,
                                depth_load_op=self.depth_load_op, depth_store_op=StoreOp.STORE if self.depth else StoreOp.DONT_CARE, prim_id=self.prim,
                                render_area=s.render_area)
        if self.sky is not None and self.sky.first:
            self._record_sky(cmd)
        for st in self.draw_state:
            d = st["draw"]
            vp = d.viewport or (0.0, 0.0, float(s.width), float(s.height), 0.0, 1.0)
            sc = d.scissor or (0, 0, s.width, s.height)
            cmd.set_viewport(*vp)
            cmd.set_scissor(*sc)
            cmd.bind_pipeline(st["pipe"])
            cmd.bind_vertex_buffers(0, [st["vb"]], [0])
            for slot, key in ((Slot.CAMERA, "camera"), (Slot.OBJECT, "object"), (Slot.LIGHTS, "light"),
                              (Slot.MATERIAL, "material"), (Slot.POINT_LIGHTS, "point"), (Slot.SPOT_LIGHTS, "spot")):
                if st[key] is not None:
                    cmd.bind_uniform(slot, st[key])
            for slot, img in enumerate(st["textures"]):
                if img is not None or slot < 2:
                    cmd.bind_texture(slot, img)
            pbr = d.program in (scenes.PROGRAM_MODEL_PBR, scenes.PROGRAM_MODEL_PBR_IBL)     # the Cook-Torrance programs take the same shadow bindings
            if d.program == scenes.PROGRAM_MODEL_PBR_IBL:
                assert self.ibl_images is not None, "a MODEL_PBR_IBL draw needs scene.ibl or ibl_images="
                cmd.bind_ibl(*self.ibl_images)
            if self.shadow is not None and pbr:
                cmd.bind_uniform(Slot.SHADOW_DATA, self.shadow_data)
                cmd.bind_texture(TextureSlot.SHADOW_MAP, self.shadow_map)
            elif self.shadow is not None:
                cmd.bind_texture(TextureSlot.SHADOW_MAP, None)
            if self.cascades is not None and pbr:
                # (a draw may carry a threshold of its own, DrawSpec.csm_blend; otherwise the spec's holds)
                blend = getattr(d, "csm_blend", None)
                cmd.bind_shadow_cascades(self.cascade_array, self.cascade_params, blend_threshold=self.cascades.blend_threshold if blend is None else blend)
            elif self.cascades is not None:
                cmd.bind_shadow_cascades(None)
            if st["ib"] is not None:
                cmd.bind_index_buffer(st["ib"], 0, IndexType.UINT16 if d.index_type == 2 else IndexType.UINT32)
                cmd.draw_indexed(d.count, getattr(d, "instances", 1), d.first, d.vertex_offset, 0)
            else:
                cmd.draw(d.count, getattr(d, "instances", 1), d.first, 0)
        if self.sky is not None and not self.sky.first:
            self._record_sky(cmd)
        cmd.end_rendering()

    def render(self, fence: Optional[Fence] = None):
        self.device.submit([self.shadow_cmd, self.cmd] if self.shadow_cmd is not None else [self.cmd], fence)

    def read(self):
        self.device.wait_idle()
        out = {"color": self.color.read()}
        if self.prim:
            out["prim"] = self.prim.read()
            if self.samples == 4:      # texel (4 px + s, py) is sample s of pixel (px, py)
                out["prim"] = out["prim"].reshape(self.scene.height, self.scene.width, 4)
        if self.depth:
            out["depth"] = self.depth.read()
        return out

    def destroy(self):
        self.device.wait_idle()
        self.cmd.destroy()
        if self.shadow_cmd is not None:
            self.shadow_cmd.destroy()
        if self.owns_shadow_map:
            self.shadow_map.destroy()
        for v in self.cascade_views:
            v.destroy()
        if self.owns_cascade_array:
            self.cascade_array.destroy()
        if self.owns_ibl:
            for img in self.ibl_images:
                img.destroy()
        if self.owns_sky:
            self.sky_image.destroy()
        for o in self.objs:
            o.destroy()
        for o, owned in ((self.prim, self.owns_prim), (self.depth, self.owns_depth), (self.color, True)):
            if o is not None and owned:
                o.destroy()
        self.objs = []


def load_environment(device: Device, path_or_bytes, env_size: int, irradiance_size: int = 32, prefiltered_size: int = 128, prefilter_samples: int = 1024,
                     lut_size: int = 512, seamless: bool = False):
    """A Radiance .hdr file (a path, or the file's bytes) to the images of an IBL set: host decode (images.load_hdr / decode_hdr), upload of the RGBE
    bytes, ibl_equirect_to_cube_rgbe, the cube's mip chain, irradiance, prefilter and the BRDF LUT.  Returns (environment, irradiance, prefiltered,
    brdf_lut): the environment cube (env_size, full chain; what bind_skybox takes) and the three images of bind_ibl.  The defaults are the reference's
    sizes (irradiance 32, prefiltered 128 with its full chain and 1024 samples, LUT 512).  seamless=True sets set_cube_seamless on the three cubes before
    the passes that read them run.  The caller destroys the four images."""
    from . import images
    hdr = images.decode_hdr(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else images.load_hdr(os.fspath(path_or_bytes))
    made = []
    try:
        src = Image.from_hdr(device, hdr)
        made.append(src)
        env = Image.create_cube(device, env_size, int(env_size).bit_length(), seamless=seamless)
        made.append(env)
        irr = Image.create_cube(device, irradiance_size, 1, seamless=seamless)
        made.append(irr)
        pre = Image.create_cube(device, prefiltered_size, int(prefiltered_size).bit_length(), seamless=seamless)
        made.append(pre)
        lut = Image(device, lut_size, lut_size, Format.R32G32B32A32_SFLOAT)
        made.append(lut)
        env.ibl_equirect_to_cube_rgbe(src)
        env.ibl_cube_generate_mips()
        irr.ibl_irradiance(env)
        pre.ibl_prefilter(env, prefilter_samples)
        lut.ibl_brdf_lut()
    except Exception:
        for img in made:
            img.destroy()
        raise
    src.destroy()
    return env, irr, pre, lut
