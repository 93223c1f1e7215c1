//! crates/rhi/src/command.rs:52-628 and rendering.rs:65-115,319-370: recording is host-only, one recorder per thread.
use crate::buffer::Buffer;
use crate::device::Device;
use crate::error::{check, RhiResult};
use crate::image::Image;
use crate::pipeline::Pipeline;
use std::sync::Arc;

#[repr(i32)] #[derive(Clone, Copy, Debug, PartialEq, Eq)] pub enum LoadOp { Load = 0, Clear = 1, DontCare = 2 }
#[repr(i32)] #[derive(Clone, Copy, Debug, PartialEq, Eq)] pub enum StoreOp { Store = 0, DontCare = 1 }
#[repr(i32)] #[derive(Clone, Copy, Debug, PartialEq, Eq)] pub enum IndexType { Uint16 = 0, Uint32 = 1 }
/// The registers of the HLSL the reference binds through descriptor sets (b0..b3, t0/t1 space1): INTEGRATION.md section 4.
#[repr(i32)] #[derive(Clone, Copy, Debug, PartialEq, Eq)] pub enum UniformSlot { Camera = 0, Object = 1, Lights = 2, Material = 3, PointLights = 4, SpotLights = 5, ShadowData = 6 }
/// model_pbr.hlsl:62-95 slot order
#[repr(i32)] #[derive(Clone, Copy, Debug, PartialEq, Eq)] pub enum TextureSlot { Albedo = 0, Normal = 1, MetallicRoughness = 2, Occlusion = 3, Emissive = 4, ShadowMap = 5 }

#[derive(Clone, Copy, Debug)] pub struct Viewport { pub x: f32, pub y: f32, pub width: f32, pub height: f32, pub min_depth: f32, pub max_depth: f32 }
#[derive(Clone, Copy, Debug)] pub struct Rect2D { pub x: i32, pub y: i32, pub width: u32, pub height: u32 }
#[derive(Clone, Copy, Debug)] pub enum ClearValue { Color([f32; 4]), Depth(f32) }
#[repr(i32)] #[derive(Clone, Copy, Debug, PartialEq, Eq)] pub enum Filter { Nearest = 0, Linear = 1 }
pub use mirhi_sys::{mirhi_buffer_copy as BufferCopy, mirhi_buffer_image_copy as BufferImageCopy, mirhi_image_blit as ImageBlit, mirhi_image_copy as ImageCopy};

/// What `RenderingConfig::build` (rendering.rs:908-995) hands to `begin_rendering`: one colour attachment, optional depth.
pub struct RenderingInfo<'a> {
    pub color: &'a Image, pub color_load_op: LoadOp, pub color_store_op: StoreOp, pub clear_color: [f32; 4],
    pub depth: Option<&'a Image>, pub depth_load_op: LoadOp, pub depth_store_op: StoreOp, pub clear_depth: f32,
    pub render_area: Rect2D,
    /// ColorAttachment::with_resolve / DepthAttachment::with_resolve (rendering.rs:238, :477): the 1x images a multisampled scope resolves to
    pub color_resolve: Option<&'a Image>, pub depth_resolve: Option<&'a Image>,
}
impl<'a> RenderingInfo<'a> {
    /// rendering.rs defaults: colour CLEAR/STORE to (0,0,0,1); depth CLEAR/DONT_CARE to 1.0 (1027-1073)
    pub fn new(color: &'a Image) -> Self {
        Self { color, color_load_op: LoadOp::Clear, color_store_op: StoreOp::Store, clear_color: [0.0, 0.0, 0.0, 1.0],
               depth: None, depth_load_op: LoadOp::Clear, depth_store_op: StoreOp::DontCare, clear_depth: 1.0,
               render_area: Rect2D { x: 0, y: 0, width: color.width(), height: color.height() }, color_resolve: None, depth_resolve: None }
    }
    /// rendering.rs:238: `color` is a multisampled image (`Image::new_multisampled`) whose four samples are averaged into `target` (AVERAGE); the
    /// multisampled contents are transient (store DONT_CARE).
    pub fn with_resolve(mut self, target: &'a Image) -> Self { self.color_resolve = Some(target); self.color_store_op = StoreOp::DontCare; self }
    /// rendering.rs:477: sample 0 of the multisampled depth attachment is written to `target` (SAMPLE_ZERO).
    pub fn with_depth_resolve(mut self, target: &'a Image) -> Self { self.depth_resolve = Some(target); self }
    /// rendering.rs:818-838: the scope loads, clears, draws and stores inside `area` only; no pixel outside is written.
    pub fn with_render_area(mut self, area: Rect2D) -> Self { self.render_area = area; self }
    pub fn with_offset(mut self, x: i32, y: i32) -> Self { self.render_area.x = x; self.render_area.y = y; self }
}

/// command.rs:52-106.  libmirhi keeps one workspace per command buffer; the pool only carries the device.
pub struct CommandPool { device: Arc<Device> }
impl CommandPool {
    pub fn new(device: Arc<Device>, _queue_family_index: u32) -> RhiResult<Self> { Ok(Self { device }) }
    pub fn device(&self) -> &Arc<Device> { &self.device }
}

pub struct CommandBuffer {
    #[allow(dead_code)]
    device: Arc<Device>,
    pub(crate) raw: *mut mirhi_sys::mirhi_cmd,
}
unsafe impl Send for CommandBuffer {}

impl CommandBuffer {
    pub fn new(device: Arc<Device>, _pool: &CommandPool) -> RhiResult<Self> {                           // command.rs:297
        let mut raw = std::ptr::null_mut();
        check(unsafe { mirhi_sys::mirhi_cmd_create(device.raw, &mut raw) })?;
        Ok(Self { device, raw })
    }
    pub fn begin(&self) -> RhiResult<()> { check(unsafe { mirhi_sys::mirhi_cmd_begin(self.raw) }) }                   // :333 one-time submit
    pub fn begin_reusable(&self) -> RhiResult<()> { check(unsafe { mirhi_sys::mirhi_cmd_begin_reusable(self.raw) }) } // :353
    pub fn end(&self) -> RhiResult<()> { check(unsafe { mirhi_sys::mirhi_cmd_end(self.raw) }) }                       // :372
    pub fn reset(&self) -> RhiResult<()> { check(unsafe { mirhi_sys::mirhi_cmd_reset(self.raw) }) }                   // :387

    // The reference's recording calls return (); libmirhi reports misuse (wrong state, missing binding) -- surfaced here.
    pub fn begin_rendering(&self, info: &RenderingInfo<'_>) -> RhiResult<()> {                                       // :408
        let mut ri = std::mem::MaybeUninit::<mirhi_sys::mirhi_rendering_info>::zeroed();
        unsafe { mirhi_sys::mirhi_rendering_info_default(ri.as_mut_ptr()) };
        let mut ri = unsafe { ri.assume_init() };
        ri.color_image = info.color.raw; ri.color_load_op = info.color_load_op as i32; ri.color_store_op = info.color_store_op as i32;
        ri.clear_color = info.clear_color;
        ri.depth_image = info.depth.map_or(std::ptr::null_mut(), |d| d.raw);
        ri.depth_load_op = info.depth_load_op as i32; ri.depth_store_op = info.depth_store_op as i32; ri.clear_depth = info.clear_depth;
        ri.render_area = [info.render_area.x, info.render_area.y, info.render_area.width as i32, info.render_area.height as i32];
        let res = mirhi_sys::mirhi_resolve_info {
            color_resolve_image: info.color_resolve.map_or(std::ptr::null_mut(), |i| i.raw),
            color_resolve_mode: if info.color_resolve.is_some() { mirhi_sys::MIRHI_RESOLVE_AVERAGE } else { mirhi_sys::MIRHI_RESOLVE_NONE },
            depth_resolve_image: info.depth_resolve.map_or(std::ptr::null_mut(), |i| i.raw),
            depth_resolve_mode: if info.depth_resolve.is_some() { mirhi_sys::MIRHI_RESOLVE_SAMPLE_ZERO } else { mirhi_sys::MIRHI_RESOLVE_NONE },
        };
        // (no resolve on a 1x scope: exactly mirhi_cmd_begin_rendering)
        check(unsafe { mirhi_sys::mirhi_cmd_begin_rendering_resolve(self.raw, &ri, &res) })
    }
    /// A depth-only scope (shadow pass, ShaderProgram::Shadow draws only): no colour attachment, `depth` stored; its extent is the render area.
    pub fn begin_rendering_depth_only(&self, depth: &Image, depth_load_op: LoadOp, clear_depth: f32) -> RhiResult<()> {
        let mut ri = std::mem::MaybeUninit::<mirhi_sys::mirhi_rendering_info>::zeroed();
        unsafe { mirhi_sys::mirhi_rendering_info_default(ri.as_mut_ptr()) };
        let mut ri = unsafe { ri.assume_init() };
        ri.color_image = std::ptr::null_mut();
        ri.depth_image = depth.raw;
        ri.depth_load_op = depth_load_op as i32; ri.depth_store_op = StoreOp::Store as i32; ri.clear_depth = clear_depth;
        check(unsafe { mirhi_sys::mirhi_cmd_begin_rendering(self.raw, &ri) })
    }
    /// A multiview depth scope (RenderingConfig::with_view_mask, rendering.rs:841-862): the Shadow draws recorded in it are rendered once per set bit `v` of
    /// `view_mask` into layer `v` of `depth_array` (`Image::new_array`), with view `v`'s 64-byte light matrix read at `view_offset + v * view_stride` of
    /// `view_constants` when the scope executes; the draw's own Camera block still supplies `model`.  One scope, one launch per stage, all cascades.
    pub fn begin_rendering_multiview(&self, depth_array: &Image, depth_load_op: LoadOp, clear_depth: f32, view_mask: u32, view_constants: &Buffer,
                                     view_offset: u64, view_stride: u32) -> RhiResult<()> {
        let mut ri = std::mem::MaybeUninit::<mirhi_sys::mirhi_rendering_info>::zeroed();
        unsafe { mirhi_sys::mirhi_rendering_info_default(ri.as_mut_ptr()) };
        let mut ri = unsafe { ri.assume_init() };
        ri.color_image = std::ptr::null_mut();
        ri.depth_image = depth_array.raw;
        ri.depth_load_op = depth_load_op as i32; ri.depth_store_op = StoreOp::Store as i32; ri.clear_depth = clear_depth;
        let mv = mirhi_sys::mirhi_multiview_info { view_mask, view_constants: view_constants.raw, view_offset, view_stride };
        check(unsafe { mirhi_sys::mirhi_cmd_begin_rendering_multiview(self.raw, &ri, &mv) })
    }
    pub fn end_rendering(&self) -> RhiResult<()> { check(unsafe { mirhi_sys::mirhi_cmd_end_rendering(self.raw) }) }  // :417
    pub fn bind_pipeline(&self, pipeline: &Pipeline) -> RhiResult<()> {                                              // :433
        check(unsafe { mirhi_sys::mirhi_cmd_bind_pipeline(self.raw, pipeline.raw) })
    }
    pub fn bind_vertex_buffers(&self, first_binding: u32, buffers: &[&Buffer], offsets: &[u64]) -> RhiResult<()> {   // :448
        let raws: Vec<*mut mirhi_sys::mirhi_buffer> = buffers.iter().map(|b| b.raw).collect();
        check(unsafe { mirhi_sys::mirhi_cmd_bind_vertex_buffers(self.raw, first_binding, raws.len() as u32, raws.as_ptr(), offsets.as_ptr()) })
    }
    pub fn bind_index_buffer(&self, buffer: &Buffer, offset: u64, index_type: IndexType) -> RhiResult<()> {          // :471
        check(unsafe { mirhi_sys::mirhi_cmd_bind_index_buffer(self.raw, buffer.raw, offset, index_type as i32) })
    }
    /// Stands in for `bind_descriptor_sets` (:493): one call per register; `range` 0 = to the end of the buffer.
    pub fn bind_uniform(&self, slot: UniformSlot, buffer: &Buffer, offset: u64, range: u64) -> RhiResult<()> {
        check(unsafe { mirhi_sys::mirhi_cmd_bind_uniform(self.raw, slot as i32, buffer.raw, offset, range) })
    }
    pub fn bind_texture(&self, slot: TextureSlot, image: Option<&Image>) -> RhiResult<()> {
        check(unsafe { mirhi_sys::mirhi_cmd_bind_texture(self.raw, slot as i32, image.map_or(std::ptr::null_mut(), |i| i.raw)) })
    }
    /// Set 2, bindings 3 / 4 of pixel/model_pbr_ibl_csm.hlsl:115-127: the four-layer D32 array and its `CSMParams` (336 B); `None` unbinds.
    pub fn bind_shadow_cascades(&self, cascades: Option<(&Image, &Buffer)>, offset: u64, range: u64) -> RhiResult<()> {
        let (array, params) = cascades.map_or((std::ptr::null_mut(), std::ptr::null_mut()), |(a, b)| (a.raw, b.raw));
        check(unsafe { mirhi_sys::mirhi_cmd_bind_shadow_cascades(self.raw, array, params, offset, range) })
    }
    /// The same binding with cascade blending (`CalculateShadowCSMBlended`, shadow_csm.hlsli:212-277): `blend_threshold` in [0, 1] is latched per draw
    /// with the binding; 0.0 records exactly what `bind_shadow_cascades` records.
    pub fn bind_shadow_cascades_blended(&self, cascades: Option<(&Image, &Buffer)>, offset: u64, range: u64, blend_threshold: f32) -> RhiResult<()> {
        let (array, params) = cascades.map_or((std::ptr::null_mut(), std::ptr::null_mut()), |(a, b)| (a.raw, b.raw));
        check(unsafe { mirhi_sys::mirhi_cmd_bind_shadow_cascades_blended(self.raw, array, params, offset, range, blend_threshold) })
    }
    /// Set 3 of pixel/model_pbr_ibl.hlsl:133-155: irradiance cube, prefiltered cube and BRDF LUT of `ShaderProgram::ModelPbrIbl` draws; `None` unbinds.
    pub fn bind_ibl(&self, set: Option<(&Image, &Image, &Image)>) -> RhiResult<()> {
        let n = std::ptr::null_mut();
        let (irradiance, prefiltered, brdf_lut) = set.map_or((n, n, n), |(a, b, c)| (a.raw, b.raw, c.raw));
        check(unsafe { mirhi_sys::mirhi_cmd_bind_ibl(self.raw, irradiance, prefiltered, brdf_lut) })
    }
    /// Set 0 of pixel/skybox.hlsl: the environment cube of `ShaderProgram::Skybox` draws (`draw(3, 1, 0, 0)`; the first 64 bytes of
    /// the push constants are inverseViewProjection); `None` unbinds.
    pub fn bind_skybox(&self, environment: Option<&Image>) -> RhiResult<()> {
        check(unsafe { mirhi_sys::mirhi_cmd_bind_skybox(self.raw, environment.map_or(std::ptr::null_mut(), |i| i.raw)) })
    }
    pub fn set_viewport(&self, v: &Viewport) -> RhiResult<()> {                                                      // :522
        let raw = mirhi_sys::mirhi_viewport { x: v.x, y: v.y, width: v.width, height: v.height, min_depth: v.min_depth, max_depth: v.max_depth };
        check(unsafe { mirhi_sys::mirhi_cmd_set_viewport(self.raw, &raw) })
    }
    pub fn set_scissor(&self, s: &Rect2D) -> RhiResult<()> {                                                         // :549
        let raw = mirhi_sys::mirhi_rect2d { x: s.x, y: s.y, width: s.width, height: s.height };
        check(unsafe { mirhi_sys::mirhi_cmd_set_scissor(self.raw, &raw) })
    }
    pub fn draw(&self, vertex_count: u32, instance_count: u32, first_vertex: u32, first_instance: u32) -> RhiResult<()> {   // :583
        check(unsafe { mirhi_sys::mirhi_cmd_draw(self.raw, vertex_count, instance_count, first_vertex, first_instance) })
    }
    pub fn draw_indexed(&self, index_count: u32, instance_count: u32, first_index: u32, vertex_offset: i32, first_instance: u32) -> RhiResult<()> {   // :610
        check(unsafe { mirhi_sys::mirhi_cmd_draw_indexed(self.raw, index_count, instance_count, first_index, vertex_offset, first_instance) })
    }
    /// Arguments are read from `buffer` when this call records (libmirhi latches them; Vulkan reads them at execution).
    pub fn draw_indirect(&self, buffer: &Buffer, offset: u64, draw_count: u32, stride: u32) -> RhiResult<()> {              // :630
        check(unsafe { mirhi_sys::mirhi_cmd_draw_indirect(self.raw, buffer.raw, offset, draw_count, stride) })
    }
    pub fn draw_indexed_indirect(&self, buffer: &Buffer, offset: u64, draw_count: u32, stride: u32) -> RhiResult<()> {      // :646
        check(unsafe { mirhi_sys::mirhi_cmd_draw_indexed_indirect(self.raw, buffer.raw, offset, draw_count, stride) })
    }
    pub fn push_constants_bytes(&self, stages: u32, offset: u32, data: &[u8]) -> RhiResult<()> {                            // :752
        check(unsafe { mirhi_sys::mirhi_cmd_push_constants(self.raw, stages, offset, data.as_ptr() as *const std::os::raw::c_void, data.len() as u32) })
    }
    pub fn push_constants<T: Copy>(&self, stages: u32, offset: u32, data: &T) -> RhiResult<()> {                            // :732
        let bytes = unsafe { std::slice::from_raw_parts(data as *const T as *const u8, std::mem::size_of::<T>()) };
        self.push_constants_bytes(stages, offset, bytes)
    }
    // ---- the transfer group, command.rs:844-1019 (include/mirhi.h "Transfer commands"): recorded outside a rendering scope.  Regions are the sys
    // crate's `#[repr(C)]` structs (VkBufferCopy, VkBufferImageCopy, VkImageCopy, VkImageBlit cut down to 2-D, one layer); there are no image layouts.
    pub fn copy_buffer(&self, src: &Buffer, dst: &Buffer, regions: &[BufferCopy]) -> RhiResult<()> {                        // :844
        check(unsafe { mirhi_sys::mirhi_cmd_copy_buffer(self.raw, src.raw, dst.raw, regions.len() as u32, regions.as_ptr()) })
    }
    pub fn copy_buffer_to_image(&self, src: &Buffer, dst: &Image, regions: &[BufferImageCopy]) -> RhiResult<()> {           // :860
        check(unsafe { mirhi_sys::mirhi_cmd_copy_buffer_to_image(self.raw, src.raw, dst.raw, regions.len() as u32, regions.as_ptr()) })
    }
    pub fn copy_image_to_buffer(&self, src: &Image, dst: &Buffer, regions: &[BufferImageCopy]) -> RhiResult<()> {           // :886
        check(unsafe { mirhi_sys::mirhi_cmd_copy_image_to_buffer(self.raw, src.raw, dst.raw, regions.len() as u32, regions.as_ptr()) })
    }
    pub fn copy_image(&self, src: &Image, dst: &Image, regions: &[ImageCopy]) -> RhiResult<()> {                            // :913
        check(unsafe { mirhi_sys::mirhi_cmd_copy_image(self.raw, src.raw, dst.raw, regions.len() as u32, regions.as_ptr()) })
    }
    pub fn blit_image(&self, src: &Image, dst: &Image, regions: &[ImageBlit], filter: Filter) -> RhiResult<()> {            // :943
        check(unsafe { mirhi_sys::mirhi_cmd_blit_image(self.raw, src.raw, dst.raw, regions.len() as u32, regions.as_ptr(), filter as i32) })
    }
    /// The whole image, every level.
    pub fn clear_color_image(&self, image: &Image, color: &[f32; 4]) -> RhiResult<()> {                                     // :977
        check(unsafe { mirhi_sys::mirhi_cmd_clear_color_image(self.raw, image.raw, color.as_ptr()) })
    }
    /// D32_SFLOAT: the whole image, or the one layer a layer view stands for (the path has no stencil).
    pub fn clear_depth_stencil_image(&self, image: &Image, depth: f32) -> RhiResult<()> {                                   // :1003
        check(unsafe { mirhi_sys::mirhi_cmd_clear_depth_stencil_image(self.raw, image.raw, depth) })
    }
    /// Queue lane (`Device::set_queue_lanes`) this command buffer is submitted on; several command buffers handed to one
    /// `Queue::submit` that are frames of the same shape run as one batch of launches on the first one's lane.
    pub fn set_queue_lane(&self, lane: u32) -> RhiResult<()> {
        check(unsafe { mirhi_sys::mirhi_cmd_set_queue_lane(self.raw, lane) })
    }
}

impl Drop for CommandBuffer {
    fn drop(&mut self) { unsafe { mirhi_sys::mirhi_cmd_destroy(self.raw) }; }
}
