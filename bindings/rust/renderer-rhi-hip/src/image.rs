//! Attachments and textures: crates/renderer/src/depth_buffer.rs:117-127, crates/rhi/src/{image,texture}.rs (stubs in the reference).
use crate::device::Device;
use crate::error::{check, RhiResult};
use std::sync::Arc;

#[repr(i32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Format { Undefined = 0, B8G8R8A8Srgb = 1, R32G32B32A32Sfloat = 2, D32Sfloat = 3, R8G8B8A8Unorm = 4, R32Uint = 5, R8G8B8A8Srgb = 6 }

pub struct Image {
    #[allow(dead_code)]
    device: Arc<Device>,
    pub(crate) raw: *mut mirhi_sys::mirhi_image,
}
unsafe impl Send for Image {}

impl Image {
    pub fn new(device: Arc<Device>, width: u32, height: u32, format: Format) -> RhiResult<Self> {     // (zero size => error, depth_buffer.rs:117-127)
        let mut raw = std::ptr::null_mut();
        check(unsafe { mirhi_sys::mirhi_image_create(device.raw, width, height, format as i32, &mut raw) })?;
        Ok(Self { device, raw })
    }
    /// `layers` tightly packed width x height levels in one allocation (D32Sfloat only): the `Texture2DArray<float>` of shadow_csm.hlsli.
    pub fn new_array(device: Arc<Device>, width: u32, height: u32, layers: u32, format: Format) -> RhiResult<Self> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { mirhi_sys::mirhi_image_create_array(device.raw, width, height, layers, format as i32, &mut raw) })?;
        Ok(Self { device, raw })
    }
    /// A non-owning 2-D image of one layer (a `vk::ImageView` with `layer_count` 1, what `DepthAttachment` takes, rendering.rs:319-370).
    /// Drop it before the array: the array refuses to be destroyed while a view is alive.
    pub fn layer_view(&self, layer: u32) -> RhiResult<Self> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { mirhi_sys::mirhi_image_create_layer_view(self.raw, layer, &mut raw) })?;
        Ok(Self { device: self.device.clone(), raw })
    }
    /// The transient attachment of a 4x multisampled scope (`samples` = 4): it owns no memory and is nothing but an attachment --
    /// `RenderingInfo::with_resolve` names the 1x image its averaged colour is written to.
    pub fn new_multisampled(device: Arc<Device>, width: u32, height: u32, format: Format, samples: u32) -> RhiResult<Self> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { mirhi_sys::mirhi_image_create_multisampled(device.raw, width, height, format as i32, samples, &mut raw) })?;
        Ok(Self { device, raw })
    }
    /// 4 for a multisampled image, 1 for every other.
    pub fn samples(&self) -> u32 { unsafe { mirhi_sys::mirhi_image_samples(self.raw) } }
    /// Six faces (+X, -X, +Y, -Y, +Z, -Z) and `levels` mip levels in one allocation (R32G32B32A32Sfloat only): level-major, then face-major,
    /// then row-major.  What the IBL precompute passes below read and write.
    pub fn new_cube(device: Arc<Device>, size: u32, levels: u32, format: Format) -> RhiResult<Self> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { mirhi_sys::mirhi_image_create_cube(device.raw, size, levels, format as i32, &mut raw) })?;
        Ok(Self { device, raw })
    }
    /// Sample count the prefilter pass uses when the caller has no reason for another.
    pub const DEFAULT_PREFILTER_SAMPLES: u32 = 1024;
    /// equirect_to_cubemap.hlsl: level 0 of this cube from a 2-D equirectangular image.
    pub fn ibl_equirect_to_cube(&self, src2d: &Image) -> RhiResult<()> { check(unsafe { mirhi_sys::mirhi_ibl_equirect_to_cube(src2d.raw, self.raw) }) }
    /// The same pass from a 2-D R8G8B8A8_UNORM image holding Radiance RGBE bytes (R, G, B, E): each tap is decoded before the blend.
    pub fn ibl_equirect_to_cube_rgbe(&self, rgbe8: &Image) -> RhiResult<()> { check(unsafe { mirhi_sys::mirhi_ibl_equirect_to_cube_rgbe(rgbe8.raw, self.raw) }) }
    /// This 2-D R32G32B32A32_SFLOAT image receives the exact float texels of the RGBE image of the same extent.
    pub fn expand_rgbe(&self, rgbe8: &Image) -> RhiResult<()> { check(unsafe { mirhi_sys::mirhi_image_expand_rgbe(rgbe8.raw, self.raw) }) }
    /// Levels 1.. of this cube from its level 0 (2 x 2 box filter per face).
    pub fn ibl_cube_generate_mips(&self) -> RhiResult<()> { check(unsafe { mirhi_sys::mirhi_ibl_cube_generate_mips(self.raw) }) }
    /// irradiance_map.hlsl: level 0 of this cube from the environment cube.
    pub fn ibl_irradiance(&self, env: &Image) -> RhiResult<()> { check(unsafe { mirhi_sys::mirhi_ibl_irradiance(env.raw, self.raw) }) }
    /// prefilter_map.hlsl: every level of this cube from the environment cube's chain; `sample_count` in 1..=4096.
    pub fn ibl_prefilter(&self, env: &Image, sample_count: u32) -> RhiResult<()> {
        check(unsafe { mirhi_sys::mirhi_ibl_prefilter(env.raw, self.raw, sample_count) })
    }
    /// brdf_lut.hlsl: this square 2-D R32G32B32A32Sfloat image receives (A, B, 0, 1).
    pub fn ibl_brdf_lut(&self) -> RhiResult<()> { check(unsafe { mirhi_sys::mirhi_ibl_brdf_lut(self.raw) }) }
    pub fn layers(&self) -> u32 { unsafe { mirhi_sys::mirhi_image_layers(self.raw) } }
    /// RGBA8 / float texels of level 0, row-major, top row first.
    pub fn upload(&self, texels: &[u8]) -> RhiResult<()> {
        check(unsafe { mirhi_sys::mirhi_image_upload(self.raw, texels.as_ptr().cast(), texels.len() as u64) })
    }
    /// Full mip chain behind level 0 (2x2 box on the stored bytes); the image is then sampled trilinearly.
    pub fn generate_mips(&self) -> RhiResult<()> { check(unsafe { mirhi_sys::mirhi_image_generate_mips(self.raw) }) }
    /// Readback of a finished target -- the reference presents instead (swapchain.rs:255) and has no such call.
    pub fn read(&self, dst: &mut [u8]) -> RhiResult<()> {
        check(unsafe { mirhi_sys::mirhi_image_read(self.raw, dst.as_mut_ptr().cast(), dst.len() as u64) })
    }
    pub fn width(&self) -> u32 { unsafe { mirhi_sys::mirhi_image_width(self.raw) } }
    pub fn height(&self) -> u32 { unsafe { mirhi_sys::mirhi_image_height(self.raw) } }
    pub fn size_bytes(&self) -> u64 { unsafe { mirhi_sys::mirhi_image_size_bytes(self.raw) } }
    pub fn mip_levels(&self) -> u32 { unsafe { mirhi_sys::mirhi_image_mip_levels(self.raw) } }
    /// Sampler state: 1 = trilinear, up to 16 = anisotropic (the device enables `sampler_anisotropy`, device.rs:161-165).
    pub fn set_max_anisotropy(&self, max_anisotropy: u32) -> RhiResult<()> {
        check(unsafe { mirhi_sys::mirhi_image_set_max_anisotropy(self.raw, max_anisotropy) })
    }
    pub fn max_anisotropy(&self) -> u32 { unsafe { mirhi_sys::mirhi_image_max_anisotropy(self.raw) } }
    /// The rest of the sampler state (include/mirhi.h `mirhi_image_set_sampler`): address modes, mag / min filters and mip mode, for draws
    /// recorded afterwards.  `default_sampler()` is REPEAT / LINEAR / MIP_LINEAR.
    pub fn set_sampler(&self, desc: &mirhi_sys::mirhi_sampler_desc) -> RhiResult<()> {
        check(unsafe { mirhi_sys::mirhi_image_set_sampler(self.raw, desc) })
    }
    pub fn sampler(&self) -> RhiResult<mirhi_sys::mirhi_sampler_desc> {
        let mut desc = Self::default_sampler();
        check(unsafe { mirhi_sys::mirhi_image_sampler(self.raw, &mut desc) })?;
        Ok(desc)
    }
    /// A cube's seamless state (include/mirhi.h "The sampler"): lookups filter across face edges and corners, for draws recorded afterwards
    /// and from the precompute passes' next call on.  Off by default; refused on anything but a cube image.
    pub fn set_cube_seamless(&self, enable: bool) -> RhiResult<()> {
        check(unsafe { mirhi_sys::mirhi_image_set_cube_seamless(self.raw, enable as u32) })
    }
    pub fn cube_seamless(&self) -> bool { unsafe { mirhi_sys::mirhi_image_cube_seamless(self.raw) != 0 } }
    pub fn default_sampler() -> mirhi_sys::mirhi_sampler_desc {
        let mut desc = mirhi_sys::mirhi_sampler_desc {
            address_u: mirhi_sys::MIRHI_ADDRESS_REPEAT, address_v: mirhi_sys::MIRHI_ADDRESS_REPEAT, mag_filter: mirhi_sys::MIRHI_SAMPLER_FILTER_LINEAR,
            min_filter: mirhi_sys::MIRHI_SAMPLER_FILTER_LINEAR, mip_mode: mirhi_sys::MIRHI_MIP_LINEAR,
        };
        unsafe { mirhi_sys::mirhi_sampler_desc_default(&mut desc) };
        desc
    }
}

impl Drop for Image {
    fn drop(&mut self) { unsafe { mirhi_sys::mirhi_image_destroy(self.raw) }; }
}
