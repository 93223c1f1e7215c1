/*
 * mirhi.h -- C ABI of the MI355X-native compute rasterizer (libmirhi.so).
 *
 * Drop-in boundary for the draw path of itsakeyfut/renderer-rs: every entry point below
 * replaces one public method of the reference's `crates/rhi` object surface (the reference has
 * no trait / plugin seam, SURVEY.md section 0.2, so the seam is the rhi structs' methods) or one step
 * of `crates/renderer`'s draw-submit loop.  Plain pointers, sizes and #[repr(C)]-compatible
 * structs only: a Rust `mirhi-sys` crate binds this header 1:1.
 *
 * Conventions
 *   - every function returns mirhi_result; MIRHI_OK == 0; on failure
 *     mirhi_last_error_message() returns a thread-local description whose text mirrors the
 *     reference's RhiError payload (crates/rhi/src/error.rs:6-50).
 *   - never aborts, never throws across the ABI.
 *   - threading contract = the reference's: a device is shared freely (device.rs:379-380),
 *     command buffers / recording are externally synchronised (command.rs:48-51).
 *   - there is NO CPU fallback: creating a device without a HIP GPU fails with
 *     MIRHI_ERR_NO_SUITABLE_GPU.
 */
#ifndef MIRHI_H
#define MIRHI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIRHI_ABI_VERSION 5u     /* 3: mirhi_pipeline_desc.fragment_discard_enable; 4: mirhi_device_set_submit_thread; 5: mirhi_device_set_native_dispatch,
                                    mirhi_device_dispatch_path, mirhi_device_measure_roundtrip, mirhi_build_id, mirhi_device_set_tile_split_layout,
                                    mirhi_device_split_rows, mirhi_device_stats grew four words;
                                    still 5 (new enum values only): MIRHI_PROGRAM_SHADOW, MIRHI_SLOT_SHADOW_DATA, MIRHI_TEXTURE_SHADOW_MAP, depth-only
                                    pipelines (colour format UNDEFINED) and depth-only rendering scopes (color_image NULL);
                                    still 5 (new functions only): mirhi_image_create_array, mirhi_image_create_layer_view, mirhi_image_layers,
                                    mirhi_cmd_bind_shadow_cascades;
                                    still 5 (one new function): mirhi_cmd_bind_shadow_cascades_blended;
                                    still 5 (new functions only): mirhi_image_create_cube and the five mirhi_ibl_ passes;
                                    still 5 (one new enum value, one new function): MIRHI_PROGRAM_MODEL_PBR_IBL, mirhi_cmd_bind_ibl;
                                    still 5 (one new enum value, one new function): MIRHI_PROGRAM_SKYBOX, mirhi_cmd_bind_skybox;
                                    still 5 (new functions, structs and one enum only): the seven transfer commands, mirhi_buffer_copy, mirhi_buffer_image_copy,
                                    mirhi_image_copy, mirhi_image_blit, mirhi_filter;
                                    still 5 (new functions, one struct and one enum only; rasterization_samples = 4 accepted): mirhi_image_create_multisampled,
                                    mirhi_image_samples, mirhi_resolve_mode, mirhi_resolve_info, mirhi_cmd_begin_rendering_resolve;
                                    still 5 (two new functions and one struct only): mirhi_multiview_info, mirhi_multiview_info_default,
                                    mirhi_cmd_begin_rendering_multiview;
                                    still 5 (two new functions only): mirhi_image_set_cube_seamless, mirhi_image_cube_seamless;
                                    still 5 (new functions only): mirhi_image_expand_rgbe, mirhi_ibl_equirect_to_cube_rgbe */

/* ---- errors: one code per RhiError variant (crates/rhi/src/error.rs:6-50) ------------------------ */
typedef int32_t mirhi_result;
enum {
    MIRHI_OK = 0,
    MIRHI_ERR_DEVICE = 1,           /* RhiError::VulkanError  -> any HIP runtime failure */
    MIRHI_ERR_LOADING = 2,          /* RhiError::LoadingError -> HIP runtime / code object unavailable */
    MIRHI_ERR_ALLOCATOR = 3,        /* RhiError::AllocatorError -> hipMalloc failure */
    MIRHI_ERR_NO_SUITABLE_GPU = 4,  /* RhiError::NoSuitableGpu */
    MIRHI_ERR_SHADER = 5,           /* RhiError::ShaderError  -> unknown mirhi_program */
    MIRHI_ERR_SURFACE = 6,          /* RhiError::SurfaceError (unused: offscreen only) */
    MIRHI_ERR_SWAPCHAIN = 7,        /* RhiError::SwapchainError (unused: offscreen only) */
    MIRHI_ERR_INVALID_HANDLE = 8,   /* RhiError::InvalidHandle */
    MIRHI_ERR_PIPELINE = 9,         /* RhiError::PipelineError */
    MIRHI_ERR_LOCK_POISONED = 10,   /* RhiError::LockPoisoned */
    MIRHI_TIMEOUT = 11,             /* RhiError::VulkanError(vk::Result::TIMEOUT) from Fence::wait */
    MIRHI_NOT_READY = 12            /* vk::Result::NOT_READY from a fence status query */
};
const char* mirhi_last_error_message(void);
const char* mirhi_result_name(mirhi_result r);
uint32_t    mirhi_abi_version(void);

/* ---- opaque handles ------------------------------------------------------------------------------- */
typedef struct mirhi_device   mirhi_device;    /* rhi::Device        crates/rhi/src/device.rs:61-77 */
typedef struct mirhi_buffer   mirhi_buffer;    /* rhi::Buffer        crates/rhi/src/buffer.rs:124-135 */
typedef struct mirhi_image    mirhi_image;     /* swapchain image / DepthBuffer / texture (image.rs is a stub) */
typedef struct mirhi_pipeline mirhi_pipeline;  /* rhi::Pipeline      crates/rhi/src/pipeline.rs:161-168 */
typedef struct mirhi_cmd      mirhi_cmd;       /* rhi::CommandBuffer crates/rhi/src/command.rs:279-284 */
typedef struct mirhi_fence    mirhi_fence;     /* rhi::Fence         crates/rhi/src/sync.rs:134-137 */

/* ---- device: Device::new / wait_idle / Drop (device.rs:120-233,290-293,356-372) ------------------- */
mirhi_result mirhi_device_count(int32_t* out_count);                      /* physical_device.rs:202-254 */
mirhi_result mirhi_device_create(int32_t hip_ordinal, mirhi_device** out);
/* same, but all work is issued on an existing HIP stream (e.g. torch.cuda.current_stream().cuda_stream) */
mirhi_result mirhi_device_create_on_stream(int32_t hip_ordinal, void* hip_stream, mirhi_device** out);
/* Native dispatch (csrc/mirhi_native.h): a plain submit leaves the library as AQL packets on a ROCr queue of the lane's own, NOT on a HIP stream.  A device
 * made by mirhi_device_create does that on every lane.  A device made on the caller's stream keeps the promise above for queue lane 0 -- submits to lane 0
 * are HIP launches on `hip_stream`, ordered against whatever else the caller put there -- and dispatches natively only on the lanes the library created
 * (mirhi_device_set_queue_lanes), which were never ordered against that stream.  enable = 1 opts lane 0 in as well: the caller then orders its own stream
 * against the frames with fences / wait_idle (hipStreamSynchronize knows nothing about the device's queues).  enable = 0: back to the default. */
mirhi_result mirhi_device_set_native_dispatch(mirhi_device* dev, uint32_t enable);
mirhi_result mirhi_device_wait_idle(mirhi_device* dev);                   /* Device::wait_idle :290-293; also reports (once) the device-side
                                                                             status of frames submitted without a fence, as mirhi_fence_wait does */
mirhi_result mirhi_device_destroy(mirhi_device* dev);                     /* fails if children are alive */
mirhi_result mirhi_device_name(mirhi_device* dev, char* out, uint32_t out_len);
/* screen-tile-row split: this device rasterizes only the tile rows owned by `rank` of `world` (which ones: the
 * layout below); rank 0 / world 1 = whole frame.  Gathering the rows is mirhi_comm_all_gather_bands, or the caller's collective.
 * Depth-only scopes (shadow maps, MIRHI_PROGRAM_SHADOW) are not split: every rank renders the whole depth image, because each rank's
 * rows of a shadowed MODEL_PBR scope may sample any texel of it.  A recorded transfer command ("Transfer commands") is not split either: every
 * rank moves what its own memory holds. */
mirhi_result mirhi_device_set_tile_split(mirhi_device* dev, uint32_t rank, uint32_t world);
/* Which tile rows a rank gets.  BANDS: one contiguous band of ceil(tile rows / world) rows per rank (the last rank's may be short).  INTERLEAVED (the
 * default; MIRHI_SPLIT=bands|interleaved in the environment sets another default): rank r owns tile rows r, r + world, r + 2 world, ... -- every rank then
 * holds the same share of every part of the frame, so the slowest rank is the average one whatever the scene puts where ("interleave bands").
 * Every rank of a communicator must use the same layout; set it before mirhi_device_set_tile_split / mirhi_comm_create. */
typedef enum { MIRHI_SPLIT_BANDS = 0, MIRHI_SPLIT_INTERLEAVED = 1 } mirhi_split_layout;
mirhi_result mirhi_device_set_tile_split_layout(mirhi_device* dev, mirhi_split_layout layout);
/* the tile rows (32 pixel rows each, the last one of a frame possibly short) this device rasterizes of a frame `height` pixels high:
 * rows first_tile_row + k * tile_row_step, k = 0 .. tile_rows - 1 */
mirhi_result mirhi_device_split_rows(mirhi_device* dev, uint32_t height, uint32_t* first_tile_row, uint32_t* tile_row_step, uint32_t* tile_rows);
/* frames in flight (crates/renderer/src/lib.rs:43 MAX_FRAMES_IN_FLIGHT): command buffers are assigned round-robin to
 * `lanes` submit streams at creation, so independent frames (own command buffer, own target) overlap on the GPU the way
 * the reference's per-frame command buffers do between their semaphores.  Default 1 = strict submission order.  Set before
 * creating command buffers.  Work submitted on different lanes is unordered unless a fence is waited. */
mirhi_result mirhi_device_set_queue_lanes(mirhi_device* dev, uint32_t lanes);
/* Submit thread (default off).  vkQueueSubmit hands its work to the driver and returns (renderer.rs:407-424); with the thread on,
 * mirhi_queue_submit validates the submission, queues it and returns, and a thread of the device makes the kernel launches (HIP takes
 * 2.3 - 3 us of host time per launch whatever the entry point: 5 - 7 us per frame the render thread can spend recording the next
 * frame instead).  Everything else keeps its meaning: a fence waits for its submission, wait_idle and every call that reads or writes
 * a resource first wait until all queued submissions have been issued; an error the launches raise is reported by the submission's
 * fence (or by wait_idle if it has none).  Submissions are issued in the order they were made. */
mirhi_result mirhi_device_set_submit_thread(mirhi_device* dev, uint32_t enable);
/* first/last+1 pixel row of the band rendered by this device for a target of `height` rows (MIRHI_SPLIT_BANDS; with interleaved rows there is no single band:
 * InvalidHandle -- use mirhi_device_split_rows) */
mirhi_result mirhi_device_band_rows(mirhi_device* dev, uint32_t height, uint32_t* row_begin, uint32_t* row_end);

/* ---- buffers: BufferUsage + Buffer (buffer.rs:47-112,149-293,345-417) ------------------------------ */
typedef enum {
    MIRHI_BUFFER_VERTEX = 0, MIRHI_BUFFER_INDEX = 1, MIRHI_BUFFER_UNIFORM = 2,
    MIRHI_BUFFER_STORAGE = 3, MIRHI_BUFFER_STAGING = 4, MIRHI_BUFFER_INDIRECT = 5
} mirhi_buffer_usage;
mirhi_result mirhi_buffer_create(mirhi_device* dev, mirhi_buffer_usage usage, uint64_t size, mirhi_buffer** out); /* Buffer::new :149 (size 0 -> InvalidHandle) */
mirhi_result mirhi_buffer_create_with_data(mirhi_device* dev, mirhi_buffer_usage usage, const void* data, uint64_t len, mirhi_buffer** out); /* Buffer::new_with_data :227 */
mirhi_result mirhi_buffer_write(mirhi_buffer* buf, uint64_t offset, const void* data, uint64_t len);   /* Buffer::write_data :247 (bounds-checked; Storage/Indirect are "not mapped") */
mirhi_result mirhi_buffer_upload(mirhi_buffer* buf, const void* data, uint64_t len);                    /* Buffer::upload :291 */
mirhi_result mirhi_buffer_upload_via_staging(mirhi_buffer* buf, const void* data, uint64_t len);        /* Buffer::upload_via_staging :345 */
/* wrap memory that is already resident in HBM (e.g. a torch tensor); not freed on destroy */
mirhi_result mirhi_buffer_wrap_device_memory(mirhi_device* dev, mirhi_buffer_usage usage, void* device_ptr, uint64_t size, mirhi_buffer** out);
mirhi_result mirhi_buffer_read(mirhi_buffer* buf, uint64_t offset, void* dst, uint64_t len);           /* added: reference has no readback */
uint64_t     mirhi_buffer_size(const mirhi_buffer* buf);                                                /* Buffer::size :409 */
int32_t      mirhi_buffer_usage_of(const mirhi_buffer* buf);                                            /* Buffer::usage :415 */
void*        mirhi_buffer_device_ptr(const mirhi_buffer* buf);                                          /* Buffer::handle :403 */
mirhi_result mirhi_buffer_destroy(mirhi_buffer* buf);

/* ---- images: colour targets, DepthBuffer, textures -------------------------------------------------
 * formats: swapchain.rs:561-570 (B8G8R8A8_SRGB), depth_buffer.rs:48 (D32_SFLOAT); RGBA32F is the
 * parity target (linear, pre-quantisation); RGBA8_UNORM is the sampled-texture format. */
typedef enum {
    MIRHI_FORMAT_UNDEFINED = 0,
    MIRHI_FORMAT_B8G8R8A8_SRGB = 1,
    MIRHI_FORMAT_R32G32B32A32_SFLOAT = 2,
    MIRHI_FORMAT_D32_SFLOAT = 3,
    MIRHI_FORMAT_R8G8B8A8_UNORM = 4,
    MIRHI_FORMAT_R32_UINT = 5,      /* debug/parity: winning primitive id per pixel */
    MIRHI_FORMAT_R8G8B8A8_SRGB = 6  /* sampled colour textures: RGB decoded to linear on sampling */
} mirhi_format;
mirhi_result mirhi_image_create(mirhi_device* dev, uint32_t width, uint32_t height, mirhi_format format, mirhi_image** out); /* DepthBuffer::new depth_buffer.rs:117-127 (0 size -> error) */
mirhi_result mirhi_image_wrap_device_memory(mirhi_device* dev, uint32_t width, uint32_t height, mirhi_format format, void* device_ptr, mirhi_image** out);
/* Layered images: the Texture2DArray<float> of pixel/model_pbr_ibl_csm.hlsl:115-116 (four shadow cascades, shadow_csm.hlsli:19).  ONE allocation of
 * `layers` tightly packed width x height levels, layer k at byte offset k * width * height * bytes per texel.  D32_SFLOAT only (every other format:
 * InvalidHandle); layers in [1, 2048] (Vulkan's guaranteed maxImageArrayLayers).  mirhi_image_width / _height report one layer's extent,
 * mirhi_image_size_bytes the whole allocation, mirhi_image_upload / _read move the whole allocation (layers in order).  An array is no 2-D image: it is
 * refused as an attachment and at MIRHI_TEXTURE_SHADOW_MAP; its layers are rendered and sampled one by one through layer views, and the whole of it is
 * sampled through mirhi_cmd_bind_shadow_cascades. */
mirhi_result mirhi_image_create_array(mirhi_device* dev, uint32_t width, uint32_t height, uint32_t layers, mirhi_format format, mirhi_image** out);
/* A non-owning 2-D image of one layer: a VkImageView with baseArrayLayer = layer, layerCount = 1, which is what the reference's DepthAttachment takes
 * (crates/rhi/src/rendering.rs:319-370).  Accepted wherever a D32_SFLOAT image is: as the depth_image of a depth-only scope, by mirhi_image_upload /
 * _read (that layer only) and at MIRHI_TEXTURE_SHADOW_MAP (one layer as an ordinary shadow map).  layer >= layers: InvalidHandle.  Destroying a view
 * frees nothing; destroying an array with live views fails as destroying a device with live children does.  Attachment ordering across queue lanes
 * goes by the ARRAY: a scope that samples the array (or a view) waits for the scopes that wrote any of its layers on another lane, and the other way
 * round; two scopes that write different layers of one array may be serialised. */
mirhi_result mirhi_image_create_layer_view(mirhi_image* array, uint32_t layer, mirhi_image** out);
uint32_t     mirhi_image_layers(const mirhi_image* img);   /* layers of an array; 1 for every other image (views included) */
/* Multisampled images: the TRANSIENT attachments of a 4x multisampled rendering scope (mirhi_cmd_begin_rendering_resolve).  samples = 4
 * only (1: InvalidHandle "use mirhi_image_create"; anything else: InvalidHandle "unsupported: sample count"); format B8G8R8A8_SRGB, R32G32B32A32_SFLOAT or
 * D32_SFLOAT.  Such an image owns NO memory -- its samples live on the chip while a tile is rasterized and only the resolved pixel is written --:
 * mirhi_image_size_bytes is 0, mirhi_image_device_ptr NULL.  It is an attachment and nothing else: upload, read, every texture slot, the cascade, IBL
 * and skybox bindings, the transfer commands, layer views, mirhi_image_generate_mips and the sampler setters refuse it (InvalidHandle, "multisampled"). */
mirhi_result mirhi_image_create_multisampled(mirhi_device* dev, uint32_t width, uint32_t height, mirhi_format format, uint32_t samples, mirhi_image** out);
uint32_t     mirhi_image_samples(const mirhi_image* img);  /* 4, or 1 for every other image */
mirhi_result mirhi_image_upload(mirhi_image* img, const void* src, uint64_t len);
mirhi_result mirhi_image_read(mirhi_image* img, void* dst, uint64_t len);   /* added: swapchain images have no readback (swapchain.rs:255) */
/* Texture fidelity (image.rs / sampler.rs / texture.rs are stubs in the reference, the shaders assume
 * `SamplerState` filtering, model_full.hlsl:44-46): builds the full mip chain of an owned R8G8B8A8 image from its level 0
 * (2x2 box filter on the stored bytes, round half up, edge clamp for odd sizes).  A texture with a chain is sampled
 * trilinearly (LOD from the analytic screen-space UV derivatives), one without bilinearly.  Call again after an upload. */
mirhi_result mirhi_image_generate_mips(mirhi_image* img);
uint32_t     mirhi_image_mip_levels(const mirhi_image* img);
/* Sampler state of a texture (sampler.rs is a stub; Device::new enables `sampler_anisotropy`, device.rs:161-165):
 * max_anisotropy in [1, 16], 1 = plain trilinear (the default).  Takes effect on textures with a mip chain, for draws recorded
 * afterwards: N = min(ceil(Pmax / Pmin), max_anisotropy) trilinear taps along the longer axis of the pixel's footprint at
 * lambda = log2(Pmax / N), averaged (the example filter of the Vulkan specification, "Texel Anisotropic Filtering"). */
mirhi_result mirhi_image_set_max_anisotropy(mirhi_image* img, uint32_t max_anisotropy);
uint32_t     mirhi_image_max_anisotropy(const mirhi_image* img);
/* Sampler state of a texture, beside max_anisotropy (sampler.rs is a stub; per-image state is this build's form of a VkSampler).  The semantics
 * are the Vulkan specification's, "Texel Coordinate Systems" / "Texel Filtering"; the all-zero state is the sampler every texture had before this
 * state existed (REPEAT, LINEAR, trilinear with a chain), and a texture in that state is sampled exactly as before.
 *   Addressing, per axis and per mip level with that level's extent n: REPEAT i mod n; MIRRORED_REPEAT (n - 1) - mirror((i mod 2n) - n) with
 *     mirror(a) = a >= 0 ? a : -(1 + a); CLAMP_TO_EDGE clamp(i, 0, n - 1).
 *   Filters: lambda is the level of detail before clamping (mirhi_image_generate_mips above: log2 of the longer footprint axis in texels; with
 *     anisotropy the filter's own log2(Pmax / N)).  mag_filter applies where lambda <= 0 (and where the footprint is zero), min_filter where
 *     lambda > 0 -- also on a texture without a chain.  NEAREST reads the one texel at floor(u w), floor(v h); LINEAR the four around
 *     u w - 1/2, v h - 1/2; both then go through the address modes.
 *   Mip mode (textures with a chain; one without has level 0 only): MIP_LINEAR two levels around lambda clamped to [0, levels - 1], weighted;
 *     MIP_NEAREST the single level ceil(lambda + 1/2) - 1 clamped to [0, levels - 1]; MIP_BASE level 0 whatever the chain (glTF's NEAREST / LINEAR
 *     minification filters).
 *   Anisotropy applies only when min_filter is LINEAR and mip_mode MIP_LINEAR; otherwise the texture is sampled as if max_anisotropy were 1.
 *     Its N taps go through the same address modes and filters.
 * Cost: a texture with state is sampled by a slower path than one in the default state; and a scope of fragment_discard_enable pipelines in which a
 * MODEL_PBR draw's BASE COLOUR texture (the one the alpha test reads) has state is resolved in primitive order, as a blended scope is, instead of by
 * the masked depth-key variants.  State on the other textures does not change how a scope is resolved.
 * Takes effect for draws recorded afterwards, like max_anisotropy.  Refused: a NULL desc and a value outside its enum (Vulkan error, the message
 * names the field); an image that cannot sit in a material texture slot -- cube, array, layer view, D32 and float formats (InvalidHandle).  The
 * comparison sampler of MIRHI_TEXTURE_SHADOW_MAP, the cube sampler of the IBL set and the skybox, and mirhi_cmd_blit_image's filter are not
 * sampler state of an image and stay as stated where they are declared.  (The filter values are an enum of their own: zero has to be LINEAR here,
 * and mirhi_filter, the blit's VkFilter, counts NEAREST first.) */
typedef enum { MIRHI_ADDRESS_REPEAT = 0, MIRHI_ADDRESS_MIRRORED_REPEAT = 1, MIRHI_ADDRESS_CLAMP_TO_EDGE = 2 } mirhi_address_mode;
typedef enum { MIRHI_SAMPLER_FILTER_LINEAR = 0, MIRHI_SAMPLER_FILTER_NEAREST = 1 } mirhi_sampler_filter;
typedef enum { MIRHI_MIP_LINEAR = 0, MIRHI_MIP_NEAREST = 1, MIRHI_MIP_BASE = 2 } mirhi_mip_mode;
typedef struct { int32_t address_u, address_v, mag_filter, min_filter, mip_mode; } mirhi_sampler_desc;
void         mirhi_sampler_desc_default(mirhi_sampler_desc* desc);          /* all zero: REPEAT, REPEAT, LINEAR, LINEAR, MIP_LINEAR */
mirhi_result mirhi_image_set_sampler(mirhi_image* img, const mirhi_sampler_desc* desc);
mirhi_result mirhi_image_sampler(const mirhi_image* img, mirhi_sampler_desc* out);
uint32_t     mirhi_image_width(const mirhi_image* img);
uint32_t     mirhi_image_height(const mirhi_image* img);
int32_t      mirhi_image_format(const mirhi_image* img);
uint64_t     mirhi_image_size_bytes(const mirhi_image* img);
void*        mirhi_image_device_ptr(const mirhi_image* img);
mirhi_result mirhi_image_destroy(mirhi_image* img);

/* ---- IBL precompute: cube images and the reference's four compute shaders (shaders/hlsl/compute/) -------------------------------------
 * What pixel/model_pbr_ibl_csm.hlsl samples as irradianceMap, prefilteredMap and brdfLUT, made on the device.  No Rust code of the reference runs
 * these shaders, so the shaders are the specification.  Nothing here is recorded into a command buffer: each pass is an immediate operation
 * like mirhi_image_generate_mips (it waits for every queue lane, runs on the device's stream and has finished when it returns).
 *
 * Cube images.  format R32G32B32A32_SFLOAT only (the environment is HDR, the shaders write float4); size a power of two in [1, 4096]; levels in
 * [1, log2(size) + 1].  ONE allocation, level-major, then face-major, then row-major: level l holds six faces of (size >> l)^2 texels, faces
 * 0..5 = +X, -X, +Y, -Y, +Z, -Z (GetCubemapDirection, equirect_to_cubemap.hlsl:22-56), rows top first; level l starts at texel
 * 6 * sum over k < l of (size >> k)^2.  mirhi_image_width / _height report the size, mirhi_image_layers 6, mirhi_image_mip_levels `levels`,
 * mirhi_image_size_bytes the whole chain, and mirhi_image_upload / _read move the whole chain.  A cube is no 2-D image and no array: it is refused
 * (InvalidHandle, the message says "cube") as a colour, depth or prim-id attachment, at every mirhi_texture_slot, by mirhi_cmd_bind_shadow_cascades,
 * mirhi_image_create_layer_view, mirhi_image_generate_mips and mirhi_image_set_max_anisotropy, and there is no wrapped cube.  A frame samples cubes
 * through mirhi_cmd_bind_ibl (MIRHI_PROGRAM_MODEL_PBR_IBL) and mirhi_cmd_bind_skybox (MIRHI_PROGRAM_SKYBOX) and nowhere else.
 *
 * The sampler (the reference's sampler.rs is empty: this is the build's reading of `LinearSampler`).
 *   Cube lookup, TextureCube.SampleLevel(LinearSampler, dir, lod): face and (s, t) by the Vulkan specification's cube-map face selection table --
 *   major axis = the component of largest magnitude, ties prefer z, then y, then x; (sc, tc) = +X (-z, -y), -X (+z, -y), +Y (+x, +z), -Y (+x, -z),
 *   +Z (+x, -y), -Z (-x, -y); s = sc / (2 |ma|) + 1/2, t likewise -- which is the inverse of GetCubemapDirection.  Bilinear inside the selected face
 *   with clamp to edge, not seamless across faces unless the cube's seamless state is on (below): x = s n - 1/2, x0 = floor(x), fraction x - x0, the four texels at x0, x0 + 1 (and rows
 *   likewise) each clamped to [0, n - 1].  lod is clamped to [0, levels - 1]; the levels floor(lod) and floor(lod) + 1 (clamped to the last)
 *   are each filtered so and lerped by lod's fraction.
 *   Seamless cubes (mirhi_image_set_cube_seamless; the state `cube_seamless` of a cube image, 0 or 1, default 0; what Vulkan does by default).  At one
 *   level with faces of n x n texels: face, s and t as above; x = s n - 1/2, y = t n - 1/2, i0 = floor(x), j0 = floor(y); the fractions and the four
 *   taps (i0 + di, j0 + dj) as above but NOT clamped.  A tap with both indices in [0, n - 1] is that texel.  A tap with exactly one index outside (-1
 *   or n) is an edge tap: the texel of the face on the other side of that edge, in that face's border row or column, at the same position along the
 *   shared edge -- equivalently: extend the face plane to the tap's centre ((i + 1/2) / n, (j + 1/2) / n), take that point's direction
 *   (GetCubemapDirection's table with |u| or |v| > 1), run the face selection on it and take the texel (floor(s' n), floor(t' n)) clamped to
 *   [0, n - 1]; s' n stays 1 / (n + 1) away from an integer, so the two statements agree for every n up to 4096.  A tap with both indices outside is a
 *   corner tap (at most one of the four): it has no texel, its value is the mean of the other three, (a + b + c) / 3.  The four values are weighted by
 *   the fractions exactly as above; level selection and the lerp between levels are unchanged; n = 1 is legal.  Wherever all four taps lie in the face
 *   the result is the clamped sampler's.
 *   2-D lookup of the equirectangular source, Texture2D.SampleLevel(LinearSampler, uv, 0): bilinear at level 0, u repeats (longitude wraps),
 *   v clamps to the edge.
 * Numerics: float32 throughout, not bit-exact against anything: the kernels contract, use the hardware reciprocal / square root / logarithm and
 * sum in parallel (tests bound the error against a float64 model).  Only mirhi_ibl_cube_generate_mips is exact.
 * Refused with InvalidHandle: a non-cube where a cube is due (and the other way round), any format but R32G32B32A32_SFLOAT, source == destination,
 * images of two devices. */
mirhi_result mirhi_image_create_cube(mirhi_device* dev, uint32_t size, uint32_t levels, mirhi_format format, mirhi_image** out);
/* The seamless state of a cube image ("The sampler" above; VkSamplerCreateInfo without NON_SEAMLESS_CUBE_MAP, the reference's sampler.rs is empty):
 * enable 0 / 1, default 0.  Like mirhi_image_set_sampler it takes effect for draws recorded afterwards -- the state is latched when a draw is recorded
 * and is part of what a recording is compared by.  It is read by mirhi_cmd_bind_ibl's set (the irradiance cube and the prefiltered cube each carry
 * their own; the LUT is 2-D), by mirhi_cmd_bind_skybox's environment, and by mirhi_ibl_irradiance and mirhi_ibl_prefilter for `env`, the cube they
 * READ (from their next call on; prefilter's single lookup for Roughness < 0.01 included).  mirhi_ibl_cube_generate_mips (a box filter inside a face)
 * and mirhi_ibl_equirect_to_cube (a 2-D source) are unaffected.  The latched states are part of a scope's IBL set: the same three images under
 * different states within one scope are two different IBL sets.  Refused with InvalidHandle: a non-cube ("not a cube image"), a multisampled image,
 * enable > 1 (the message names the value).  mirhi_image_cube_seamless: the state; 0 for every non-cube and for NULL. */
mirhi_result mirhi_image_set_cube_seamless(mirhi_image* cube, uint32_t enable);
uint32_t     mirhi_image_cube_seamless(const mirhi_image* img);
/* equirect_to_cubemap.hlsl:78-105: level 0 of `cube`, all four channels, from the 2-D image `src2d` (DirectionToEquirectUV :59-75) */
mirhi_result mirhi_ibl_equirect_to_cube(mirhi_image* src2d, mirhi_image* cube);
/* Radiance RGBE sources.  An RGBE image on the device is an ordinary 2-D R8G8B8A8_UNORM image whose four bytes are (R, G, B, E) -- what
 * mires_hdr_decode (include/miresources.h) yields, made with mirhi_image_create and filled with mirhi_image_upload: no new format, no new upload path, a
 * quarter of the float form's bytes.  Both calls are immediate passes like the others; an `rgbe8` with a mip chain is accepted and its level 0 is read.
 * InvalidHandle: an rgbe8 that is a cube, an array, a layer view or multisampled ("the RGBE source must be a 2-D image"), of any other format
 * (R8G8B8A8_SRGB included: the bytes are no colours), a destination of another extent, images of two devices.
 * level 0 of the 2-D R8G8B8A8_UNORM image `rgbe8`, read as Radiance RGBE, into the 2-D R32G32B32A32_SFLOAT image `dst` of the same extent:
 * E = 0 -> (0,0,0,1), else (R,G,B) * 2^(E-136), alpha 1.  Exact. */
mirhi_result mirhi_image_expand_rgbe(mirhi_image* rgbe8, mirhi_image* dst);
/* mirhi_ibl_equirect_to_cube with an RGBE source: level 0 of `cube` from `rgbe8`, each of the four taps decoded as above before the
 * bilinear blend; the same uv, wrap (u repeats, v clamps) and blend as the float path. */
mirhi_result mirhi_ibl_equirect_to_cube_rgbe(mirhi_image* rgbe8, mirhi_image* cube);
/* Levels 1.. of a cube from its level 0, face by face with a 2 x 2 box filter in float, ((a + b) + (c + d)) * 0.25 (exact operations in this
 * order).  The build's own definition: the reference never builds the chain that prefilter_map.hlsl:212 samples. */
mirhi_result mirhi_ibl_cube_generate_mips(mirhi_image* cube);
/* irradiance_map.hlsl:63-143: level 0 of `out` = (rgb, 1); IrradianceMapSize = out's size; sampleDelta 0.025 (:97), whose float32 loops (:101-103)
 * make 252 phi x 63 theta steps; every lookup at level 0 of `env` */
mirhi_result mirhi_ibl_irradiance(mirhi_image* env, mirhi_image* out);
/* prefilter_map.hlsl:134-229 once per level of `out`, all levels in one launch: MipSize = size >> l, Roughness = l / (levels - 1) (0 when levels
 * is 1); Roughness < 0.01 is the single lookup at R, level 0 (:168-173); resolution = 512.0 stays hard-coded (:204); the lookups use the whole
 * chain of `env` (:212).  SourceMipLevel is read by nothing in the shader and is no parameter.  sample_count in [1, 4096] (the wrappers default
 * to 1024). */
mirhi_result mirhi_ibl_prefilter(mirhi_image* env, mirhi_image* out, uint32_t sample_count);
/* brdf_lut.hlsl:116-206: the square 2-D R32G32B32A32_SFLOAT image `out2d` receives (A, B, 0, 1) -- the consumer declares Texture2D<float4> and
 * reads .rg; 1024 samples (:133), NdotV = max(u, 0.001) (:198).  The reference stores rg16f (:18); that rounding is NOT reproduced (float
 * storage, no new format). */
mirhi_result mirhi_ibl_brdf_lut(mirhi_image* out2d);

/* ---- pipeline: GraphicsPipelineBuilder (pipeline.rs:590-1059) -------------------------------------- */
typedef enum {   /* replaces Shader::from_spirv_file (shader.rs:244-330): precompiled .hip programs */
    MIRHI_PROGRAM_NONE = -1,
    MIRHI_PROGRAM_TRIANGLE = 0,     /* vertex/triangle.hlsl + pixel/triangle.hlsl */
    MIRHI_PROGRAM_MODEL = 1,        /* vertex/model.hlsl + pixel/model.hlsl (hard-coded fallback light/material) */
    MIRHI_PROGRAM_MODEL_FULL = 2,   /* vertex/model.hlsl + pixel/model_full.hlsl + lights.hlsli */
    MIRHI_PROGRAM_MODEL_PBR = 3,    /* vertex/model.hlsl + pixel/model_pbr.hlsl + pbr.hlsli (Cook-Torrance GGX); the directional light is multiplied
                                       by CalculateShadow (shadow.hlsli:49-121, model_pbr.hlsl:238-251) when MIRHI_TEXTURE_SHADOW_MAP is bound, else shadow = 1 */
    MIRHI_PROGRAM_SHADOW = 4,       /* vertex/shadow.hlsl + pixel/shadow.hlsl: depth-only pass in light space.  Reads ShadowConstants (vertex/shadow.hlsl:7-11:
                                       lightSpaceMatrix @0, model @64, 128 B) from the b0 slot MIRHI_SLOT_CAMERA; position only, attribute_offsets[0] = 0 of
                                       attribute_count 1, any vertex_stride >= 12 that is a multiple of 4 (a packed position stream or the 48-byte Vertex).
                                       Clip = lightSpaceMatrix * (model * p), in the MODEL vertex path's operation order (vertex/model.hlsl:44-48): a SHADOW
                                       draw and a MODEL draw with viewProjection = lightSpaceMatrix give the same depth bits.
                                       Pipelines: vertex = fragment = SHADOW, color_attachment_count 1 with color_attachment_formats[0] = UNDEFINED (Vulkan's
                                       "no attachment at this location"), depth D32_SFLOAT with test and write on and LESS / LESS_OR_EQUAL / GREATER /
                                       GREATER_OR_EQUAL; no blending, no fragment discard.  SHADOW draws are recorded only in depth-only scopes
                                       (mirhi_rendering_info.color_image NULL) and only SHADOW draws there. */
    MIRHI_PROGRAM_MODEL_PBR_IBL = 5,/* vertex/model.hlsl + pixel/model_pbr_ibl.hlsl: MODEL_PBR's vertex layout, uniform slots, five material textures and 80-byte
                                       MaterialData, with the image-based ambient term of mirhi_cmd_bind_ibl (below) in place of the hemisphere ambient.  The
                                       directional light's shadow term comes from what is bound, exactly as for MODEL_PBR: nothing = 1, MIRHI_TEXTURE_SHADOW_MAP =
                                       CalculateShadow, mirhi_cmd_bind_shadow_cascades = CalculateShadowCSM (which is pixel/model_pbr_ibl_csm.hlsl). */
    MIRHI_PROGRAM_SKYBOX = 6        /* vertex/skybox.hlsl + pixel/skybox.hlsl: the environment cube behind the scene (mirhi_cmd_bind_skybox, below).  Valid only as
                                       the pair SKYBOX / SKYBOX; no vertex input: vertex_stride and attribute_count 0, no vertex buffer at the draw. */
} mirhi_program;
typedef enum { MIRHI_TOPOLOGY_POINT_LIST = 0, MIRHI_TOPOLOGY_LINE_LIST = 1, MIRHI_TOPOLOGY_LINE_STRIP = 2,
               MIRHI_TOPOLOGY_TRIANGLE_LIST = 3, MIRHI_TOPOLOGY_TRIANGLE_STRIP = 4, MIRHI_TOPOLOGY_TRIANGLE_FAN = 5 } mirhi_topology;   /* pipeline.rs:274-300 */
typedef enum { MIRHI_POLYGON_FILL = 0, MIRHI_POLYGON_LINE = 1, MIRHI_POLYGON_POINT = 2 } mirhi_polygon_mode;                          /* :306-325 */
typedef enum { MIRHI_CULL_NONE = 0, MIRHI_CULL_FRONT = 1, MIRHI_CULL_BACK = 2, MIRHI_CULL_FRONT_AND_BACK = 3 } mirhi_cull_mode;        /* :329-351 */
typedef enum { MIRHI_FRONT_FACE_COUNTER_CLOCKWISE = 0, MIRHI_FRONT_FACE_CLOCKWISE = 1 } mirhi_front_face;                              /* :355-371 */
typedef enum { MIRHI_COMPARE_NEVER = 0, MIRHI_COMPARE_LESS = 1, MIRHI_COMPARE_EQUAL = 2, MIRHI_COMPARE_LESS_OR_EQUAL = 3,
               MIRHI_COMPARE_GREATER = 4, MIRHI_COMPARE_NOT_EQUAL = 5, MIRHI_COMPARE_GREATER_OR_EQUAL = 6, MIRHI_COMPARE_ALWAYS = 7 } mirhi_compare_op; /* :375-409 */

/* ColorBlendAttachment (pipeline.rs:478-531): BlendFactor :411-448, BlendOp :452-476, in the reference's enum order.  The
 * CONSTANT_* factors need blend constants, which the reference's command buffer has no call for: refused at pipeline create. */
typedef enum { MIRHI_BLEND_ZERO = 0, MIRHI_BLEND_ONE, MIRHI_BLEND_SRC_COLOR, MIRHI_BLEND_ONE_MINUS_SRC_COLOR, MIRHI_BLEND_DST_COLOR,
               MIRHI_BLEND_ONE_MINUS_DST_COLOR, MIRHI_BLEND_SRC_ALPHA, MIRHI_BLEND_ONE_MINUS_SRC_ALPHA, MIRHI_BLEND_DST_ALPHA,
               MIRHI_BLEND_ONE_MINUS_DST_ALPHA, MIRHI_BLEND_CONSTANT_COLOR, MIRHI_BLEND_ONE_MINUS_CONSTANT_COLOR, MIRHI_BLEND_CONSTANT_ALPHA,
               MIRHI_BLEND_ONE_MINUS_CONSTANT_ALPHA, MIRHI_BLEND_SRC_ALPHA_SATURATE } mirhi_blend_factor;
typedef enum { MIRHI_BLEND_OP_ADD = 0, MIRHI_BLEND_OP_SUBTRACT, MIRHI_BLEND_OP_REVERSE_SUBTRACT, MIRHI_BLEND_OP_MIN, MIRHI_BLEND_OP_MAX } mirhi_blend_op;

typedef struct {
    int32_t  vertex_program;            /* builder.vertex_shader();   MIRHI_PROGRAM_NONE -> "Vertex shader is required" */
    int32_t  fragment_program;          /* builder.fragment_shader(); MIRHI_PROGRAM_NONE -> "Fragment shader is required" */
    uint32_t vertex_stride;             /* vertex_binding(): 24 TriangleVertex / 48 Vertex (vertex.rs:35-41,130-136) */
    uint32_t attribute_count;           /* vertex_attributes(): byte offsets by location (vertex.rs:44-61,139-170) */
    uint32_t attribute_offsets[4];
    int32_t  topology;                  /* default TRIANGLE_LIST   pipeline.rs:655 */
    int32_t  polygon_mode;              /* default FILL            :659 */
    int32_t  cull_mode;                 /* default BACK            :660 */
    int32_t  front_face;                /* default COUNTER_CLOCKWISE :661 */
    uint32_t depth_clamp_enable;        /* default 0               :662 */
    uint32_t rasterizer_discard_enable; /* default 0               :663 */
    uint32_t depth_bias_enable;         /* default 0               :664 */
    uint32_t rasterization_samples;     /* default 1               :671; 4: a pipeline for 4x multisampled scopes (mirhi_cmd_begin_rendering_resolve) */
    uint32_t depth_test_enable;         /* default 1               :676 */
    uint32_t depth_write_enable;        /* default 1               :677 */
    int32_t  depth_compare_op;          /* default LESS            :678 */
    uint32_t blend_enable;              /* default 0               :499-512 */
    uint32_t blend_attachment_count;    /* default 0 = one default attachment per colour format :1007-1018 */
    uint32_t color_attachment_count;    /* default 0 -> "At least one color attachment format is required" */
    int32_t  color_attachment_formats[4];
    int32_t  depth_attachment_format;   /* default UNDEFINED (None) :690 */
    /* the colour attachment's ColorBlendAttachment, used when blend_enable != 0 (defaults :499-512: One, Zero, Add, One, Zero, Add,
     * RGBA).  Blended draws are resolved fragment by fragment in primitive order (DESIGN.md "Ordered segments"). */
    int32_t  src_color_blend_factor, dst_color_blend_factor, color_blend_op;
    int32_t  src_alpha_blend_factor, dst_alpha_blend_factor, alpha_blend_op;
    uint32_t color_write_mask;          /* bit 0 R, 1 G, 2 B, 3 A */
    /* default 0.  The MODEL_PBR fragment program ends fragments whose base-colour alpha is below the material's alphaCutoff
     * (`discard`, pixel/model_pbr.hlsl:176-179).  With a base colour texture that is a decision per fragment, taken before the depth
     * write: pipelines for alpha-masked materials (glTF alphaMode MASK) set this.  Their draws form a rendering-scope segment of their
     * own whose raster kernel tests alpha per covered pixel in front of the depth key (blended or predicate-depth-state ones are resolved
     * fragment by fragment in primitive order instead, DESIGN.md "Ordered segments").  Without it such a draw is refused loudly at the
     * fence ("alpha cutoff"); draws whose alpha cannot cross the cutoff (no texture, or cutoff <= 0) never need it. */
    uint32_t fragment_discard_enable;
} mirhi_pipeline_desc;
void         mirhi_pipeline_desc_default(mirhi_pipeline_desc* desc);                      /* GraphicsPipelineBuilder::new :645-698 */
mirhi_result mirhi_pipeline_create(mirhi_device* dev, const mirhi_pipeline_desc* desc, mirhi_pipeline** out); /* build :918-1057 */
/* Depth bias and depth clamp.  depth_bias_enable adds o = m * slope_factor + r * constant_factor to every fragment depth of a triangle:
 * m = max(|dz/dx|, |dz/dy|) of its window-space depth plane, r = 2^(e - 23) with e the exponent of the largest |z| of its three vertices (Vulkan's rule
 * for a floating-point depth attachment); clamp > 0: o = min(o, clamp), clamp < 0: o = max(o, clamp), 0: none.  mirhi_pipeline_create takes
 * depth_bias_enable = 1 with the builder's default factors (0, 0, 0 :665-667); this call implies depth_bias_enable = 1 and takes the factors.
 * depth_clamp_enable: no clipping against the near and far planes, fragment depth clamped to [0, 1] -- draws need a viewport depth range of exactly [0, 1].
 * Refused ("unsupported:"): a NULL or non-finite bias, either state on a SKYBOX pipeline or together with rasterizer_discard_enable. */
typedef struct { float constant_factor, clamp, slope_factor; } mirhi_depth_bias;          /* GraphicsPipelineBuilder::depth_bias pipeline.rs:781-788 */
mirhi_result mirhi_pipeline_create_with_depth_bias(mirhi_device* dev, const mirhi_pipeline_desc* desc, const mirhi_depth_bias* bias, mirhi_pipeline** out); /* depth_bias :781-788 + build :918-1057 */
mirhi_result mirhi_pipeline_destroy(mirhi_pipeline* p);

/* ---- command recording: CommandBuffer (command.rs:297-628) ------------------------------------------ */
typedef enum { MIRHI_LOAD_OP_LOAD = 0, MIRHI_LOAD_OP_CLEAR = 1, MIRHI_LOAD_OP_DONT_CARE = 2 } mirhi_load_op;
typedef enum { MIRHI_STORE_OP_STORE = 0, MIRHI_STORE_OP_DONT_CARE = 1 } mirhi_store_op;
typedef enum { MIRHI_INDEX_UINT16 = 0, MIRHI_INDEX_UINT32 = 1 } mirhi_index_type;

typedef struct {     /* RenderingConfig / ColorAttachment / DepthAttachment (rendering.rs:65-115,319-370,680-726) */
    mirhi_image* color_image;        /* required -- except in a depth-only scope (MIRHI_PROGRAM_SHADOW): NULL with a depth_image, whose extent is then the
                                        render area; depth load CLEAR / LOAD, store STORE; no prim_id_image */
    int32_t      color_load_op;      /* default CLEAR  rendering.rs:106 */
    int32_t      color_store_op;     /* default STORE  :107 */
    float        clear_color[4];     /* default (0,0,0,1) :108-112 */
    mirhi_image* depth_image;        /* optional; NULL + a depth-testing pipeline keeps depth on chip only */
    int32_t      depth_load_op;      /* default CLEAR  :360 */
    int32_t      depth_store_op;     /* default DONT_CARE :361 */
    float        clear_depth;        /* default 1.0    :362-366 */
    int32_t      render_area[4];     /* x, y, width, height in pixels of the attachment; width <= 0 or height <= 0 -> full extent (rendering.rs:713-726,
                                        with_render_area / with_offset :818-838).  A rectangle inside the attachment (x, y >= 0, x + width and y + height
                                        within its extent; anything else: MIRHI_ERR_INVALID_HANDLE) -- in colour and in depth-only scopes, on images and
                                        on layer views.  Load, clear and store ops apply inside it only and no pixel outside is written, colour, depth and
                                        prim_id_image alike; fragments do not move: viewport and scissor stay in attachment coordinates, a draw gives
                                        every pixel of the area the bits it gives in a full-extent scope whose scissor is cut to the area.  Only the
                                        tiles the area touches are launched.  Refused ("unsupported:"): a partial area on a split device. */
    mirhi_image* prim_id_image;      /* optional R32_UINT: winning global primitive id (parity instrumentation) */
} mirhi_rendering_info;
void mirhi_rendering_info_default(mirhi_rendering_info* info);

typedef struct { float x, y, width, height, min_depth, max_depth; } mirhi_viewport;  /* vk::Viewport, renderer.rs:504-512 */
typedef struct { int32_t x, y; uint32_t width, height; } mirhi_rect2d;              /* vk::Rect2D,   renderer.rs:514-518 */

/* descriptor stand-in: register slots of shaders/hlsl (model.hlsl:5-19, model_full.hlsl:27-50) */
typedef enum {
    MIRHI_SLOT_CAMERA = 0,        /* b0 CameraData 208 B */
    MIRHI_SLOT_OBJECT = 1,        /* b1 ObjectData 128 B */
    MIRHI_SLOT_LIGHTS = 2,        /* b2 LightUBO 48 B */
    MIRHI_SLOT_MATERIAL = 3,      /* b3 MaterialData 32 B (model_full.hlsl:34-41); 80 B for MODEL_PBR (model_pbr.hlsl:36-59) */
    MIRHI_SLOT_POINT_LIGHTS = 4,  /* t0,space1 StructuredBuffer<PointLight> */
    MIRHI_SLOT_SPOT_LIGHTS = 5,   /* t1,space1 StructuredBuffer<SpotLight> */
    MIRHI_SLOT_SHADOW_DATA = 6,   /* ShadowData: ShadowParams 96 B (shadow.hlsli:20-30, model_pbr.hlsl:110-115): LightSpaceMatrix @0 (the convention of
                                     CameraData.viewProjection), ShadowBias @64, NormalBias @68, ShadowMapSize @72, ShadowStrength @80.  Required (>= 96 B)
                                     by a MODEL_PBR draw recorded with MIRHI_TEXTURE_SHADOW_MAP bound */
    MIRHI_SLOT_COUNT = 7
} mirhi_uniform_slot;
/* MIRHI_TEXTURE_SHADOW_MAP: t7 / s5 of model_pbr.hlsl:103-108, D32_SFLOAT images only (D32 stays refused in the five colour slots).  The reference's
 * sampler.rs is empty, so this build fixes the comparison sampler: compare op LESS_OR_EQUAL (shadow.hlsli:42), a tap is 1 when clamp(D_ref, 0, 1) <= texel;
 * nearest texel i = clamp(floor(u * W), 0, W - 1), j = clamp(floor(v * H), 0, H - 1) with W x H the image's extent (clamp-to-edge addressing); the
 * 3 x 3 tap offsets are 1 / ShadowMapSize of the UBO, as the shader has them.  MODEL / MODEL_FULL have no shadow term and ignore the slot.  A
 * shadowed draw's pipeline may not blend, discard fragments or use a predicate depth state (depth test without write, EQUAL, NOT_EQUAL, ALWAYS). */
typedef enum { MIRHI_TEXTURE_ALBEDO = 0 /* t0 */, MIRHI_TEXTURE_NORMAL = 1 /* t1 */,
               MIRHI_TEXTURE_METALLIC_ROUGHNESS = 2 /* t2 */, MIRHI_TEXTURE_OCCLUSION = 3 /* t3 */, MIRHI_TEXTURE_EMISSIVE = 4 /* t4 (model_pbr.hlsl:62-95) */,
               MIRHI_TEXTURE_SHADOW_MAP = 5 /* t7 / s5 (model_pbr.hlsl:103-108) */,
               MIRHI_TEXTURE_COUNT = 6 } mirhi_texture_slot;

mirhi_result mirhi_cmd_create(mirhi_device* dev, mirhi_cmd** out);                 /* CommandPool::new + CommandBuffer::new :89,:297 */
mirhi_result mirhi_cmd_destroy(mirhi_cmd* cmd);
/* Queue lane (mirhi_device_set_queue_lanes) this command buffer is submitted on; by default command buffers take the lanes round
 * robin in creation order.  A submit of several command buffers that are each one plain rendering scope of the same shape (the
 * frames of a frame loop) runs as ONE batch of launches on the first one's lane (vkQueueSubmit with several command buffers,
 * renderer.rs:407-424: no ordering between them is promised without a barrier). */
mirhi_result mirhi_cmd_set_queue_lane(mirhi_cmd* cmd, uint32_t lane);
mirhi_result mirhi_cmd_begin(mirhi_cmd* cmd);                                       /* begin :333 (ONE_TIME_SUBMIT) */
mirhi_result mirhi_cmd_begin_reusable(mirhi_cmd* cmd);                              /* begin_reusable :353 */
mirhi_result mirhi_cmd_end(mirhi_cmd* cmd);                                         /* end :372 */
mirhi_result mirhi_cmd_reset(mirhi_cmd* cmd);                                       /* reset :387 */
mirhi_result mirhi_cmd_begin_rendering(mirhi_cmd* cmd, const mirhi_rendering_info* info);  /* begin_rendering :408 */
/* 4x MSAA (ColorAttachment::with_resolve / DepthAttachment::with_resolve rendering.rs:238,:477, rasterization_samples pipeline.rs:796).
 * A scope whose color_image is multisampled (mirhi_image_create_multisampled).  Semantics:
 *   samples   Vulkan's standard 4x positions inside pixel (px, py): s0 (0.375, 0.125), s1 (0.875, 0.375), s2 (0.125, 0.625), s3 (0.625, 0.875).
 *   coverage  per sample: the 1x path's snapped vertices, edge functions and fill rule at the sample position.  The scissor applies to the pixel, so to all four.
 *   depth     per sample: the triangle's depth plane (with depth bias and clamp) at the sample position; compare, write and tie-break as at 1x.
 *   shading   once per pixel for each distinct primitive that wins at least one of its samples, at the pixel centre (px + 1/2, py + 1/2) whether or not the
 *             primitive covers the centre (attributes extrapolate): no centroid interpolation, no sample shading.  A sample no primitive won has the clear colour.
 *   resolve   AVERAGE: per channel, alpha included, ((c0 + c1) + (c2 + c3)) * 0.25f in binary32, in this order, nothing fused; a B8G8R8A8_SRGB target
 *             averages the linear values and encodes once.  SAMPLE_ZERO (depth): the depth of sample 0, the clear depth where no primitive reached it.
 *   prim_id_image  R32_UINT of 4 * width x height texels: texel (4 px + s, py) is the winning global primitive id of sample s, or 0xFFFFFFFF.
 * Attachments: color_load_op CLEAR and color_store_op DONT_CARE (anything else: "unsupported: multisampled attachments are transient"); color_resolve_image a 1x
 * image of the same format, extent and device with MIRHI_RESOLVE_AVERAGE; depth_image NULL (depth stays on chip) or a multisampled D32_SFLOAT with load CLEAR,
 * store DONT_CARE; depth_resolve_image optional, a 1x D32_SFLOAT image or layer view with MIRHI_RESOLVE_SAMPLE_ZERO (a later 1x scope can LOAD it) -- also
 * with depth_image NULL: the per-sample depth is then the scope's on-chip depth (cleared to clear_depth), and sample 0 of it is what is written.
 * Ordering across queue lanes goes by the resolve images: they are what the scope writes.
 * A pipeline with rasterization_samples = 4 draws in such a scope and nowhere else (a draw whose pipeline's sample count differs from its scope's is refused
 * when it is recorded).  Taken: TRIANGLE, MODEL, MODEL_FULL and MODEL_PBR without a shadow binding (mip chains, sRGB textures, anisotropy, sampler state); depth
 * test and write with LESS, LESS_OR_EQUAL, GREATER or GREATER_OR_EQUAL; depth bias and clamp; scissor and viewport; indexed, instanced and indirect draws.
 * Refused with "unsupported:" where it is recorded: blending, fragment_discard_enable, predicate depth states, a depth state change inside the scope, SKYBOX,
 * SHADOW, MODEL_PBR_IBL, shadowed or cascaded draws, a partial render area, a split device, fragment statistics.
 * resolve NULL, or all NONE / NULL, with a 1x color_image: exactly mirhi_cmd_begin_rendering. */
typedef enum { MIRHI_RESOLVE_NONE = 0, MIRHI_RESOLVE_SAMPLE_ZERO = 1, MIRHI_RESOLVE_AVERAGE = 2 } mirhi_resolve_mode;   /* VkResolveModeFlagBits */
typedef struct {
    mirhi_image* color_resolve_image;  /* NULL, or the 1x image the averaged colour is written to */
    int32_t      color_resolve_mode;   /* mirhi_resolve_mode: NONE or AVERAGE */
    mirhi_image* depth_resolve_image;  /* NULL, or the 1x D32_SFLOAT image (or layer view) sample 0's depth is written to */
    int32_t      depth_resolve_mode;   /* mirhi_resolve_mode: NONE or SAMPLE_ZERO */
} mirhi_resolve_info;
void         mirhi_resolve_info_default(mirhi_resolve_info* resolve);   /* NULL / NONE */
mirhi_result mirhi_cmd_begin_rendering_resolve(mirhi_cmd* cmd, const mirhi_rendering_info* info, const mirhi_resolve_info* resolve);
/* Multiview depth scopes (RenderingConfig::with_view_mask / with_layer_count rendering.rs:841-862): ONE depth-only scope that renders its draws
 * once per set bit of view_mask, view v into layer v of a D32_SFLOAT image array -- all cascades of a cascaded shadow map recorded once and dispatched as one
 * vertex, one geometry and one raster launch.  Semantics: the scope is, bit for bit in every layer, the single-view depth-only scopes of
 * mirhi_cmd_begin_rendering: for each set bit v the same binds and draws into the layer view of layer v, with the first 64 bytes of the ShadowConstants at
 * MIRHI_SLOT_CAMERA (lightSpaceMatrix) replaced by the 64 bytes at view_offset + v * view_stride of view_constants; `model` @64 still comes from the draw's own
 * CAMERA block, which must be bound as for any SHADOW draw.  v is Vulkan's ViewIndex.  The matrices are read when the scope EXECUTES, like every uniform.
 *   info   depth_image is the ARRAY itself (mirhi_image_create_array), not a layer view; color_image and prim_id_image NULL; depth_load_op CLEAR or LOAD;
 *          depth_store_op STORE; the full extent.  Layers whose bit is clear are not touched.
 *   state  viewport, scissor, depth bias and clamp, cull mode and front face, indexed, instanced and indirect draws apply to every view alike.
 *   order  across queue lanes by the array ("ordering is by the parent").  mirhi_device_stats: frames_submitted counts the scope once, triangles_submitted its
 *          triangles once per view.
 * Matrix storage: as ShadowConstants stores lightSpaceMatrix (16 floats, the order of every matrix of this interface).  With view_stride = 80 and view_offset = 0
 * the layout is CSMParams' (Cascades[k].ViewProjection @80k, shadow_csm.hlsli:23-28), so one buffer can feed the shadow pass and mirhi_cmd_bind_shadow_cascades --
 * PROVIDED the shadow pass renders with the very matrix the lookup uses.  A shadow pass that renders into a plain viewport with clip y negated (the lookup's
 * v = 1 - (y * 0.5 + 0.5), shadow.hlsli:65-66: what the scenes of this repository do, scenes.flip_clip_y) needs view constants of its own: the CSMParams
 * matrices with the second component of every column negated, at the same stride.
 * Refused with "unsupported:" where it is recorded: a colour attachment or prim_id_image; a depth image that is not an array, or is multisampled; load / store ops
 * other than the above; an empty mask, more than 8 bits, a bit at or above mirhi_image_layers; NULL, misaligned or too short view constants, a view_stride below 64
 * or not a multiple of 16; a partial render area; a split device; MIRHI_PROFILE_FRAGMENTS; any draw whose program is not SHADOW.  The scope ends with
 * mirhi_cmd_end_rendering.  mirhi_cmd_begin_rendering itself keeps refusing an array. */
typedef struct {
    uint32_t      view_mask;        /* bit v: view v is rendered into layer v of the depth array; 1..8 bits set, every set bit < mirhi_image_layers */
    mirhi_buffer* view_constants;   /* per-view constants, read when the scope executes (not latched at record time) */
    uint64_t      view_offset;      /* view v reads its 64-byte lightSpaceMatrix at view_offset + v * view_stride; a multiple of 16 */
    uint32_t      view_stride;      /* >= 64, a multiple of 16 */
} mirhi_multiview_info;
void         mirhi_multiview_info_default(mirhi_multiview_info* multiview);   /* mask 0, NULL, offset 0, stride 64 */
mirhi_result mirhi_cmd_begin_rendering_multiview(mirhi_cmd* cmd, const mirhi_rendering_info* info, const mirhi_multiview_info* multiview);
mirhi_result mirhi_cmd_end_rendering(mirhi_cmd* cmd);                               /* end_rendering :417 */
mirhi_result mirhi_cmd_bind_pipeline(mirhi_cmd* cmd, mirhi_pipeline* pipeline);     /* bind_pipeline :433 */
mirhi_result mirhi_cmd_bind_vertex_buffers(mirhi_cmd* cmd, uint32_t first_binding, uint32_t count, mirhi_buffer* const* buffers, const uint64_t* offsets); /* :448 */
mirhi_result mirhi_cmd_bind_index_buffer(mirhi_cmd* cmd, mirhi_buffer* buffer, uint64_t offset, mirhi_index_type type); /* :471 */
mirhi_result mirhi_cmd_bind_uniform(mirhi_cmd* cmd, mirhi_uniform_slot slot, mirhi_buffer* buffer, uint64_t offset, uint64_t range); /* bind_descriptor_sets :493 + descriptor.rs:390-409 buffer_info */
mirhi_result mirhi_cmd_bind_texture(mirhi_cmd* cmd, mirhi_texture_slot slot, mirhi_image* image);   /* descriptor.rs:411-420 image_info */
/* Shadow cascades: set 2, bindings 3 and 4 of pixel/model_pbr_ibl_csm.hlsl:115-127 (Texture2DArray<float> shadowMap t10 / s8 and cbuffer ShadowData b3
 * { CSMParams }).  `array`: a D32_SFLOAT array (not a view) of exactly CASCADE_COUNT = 4 layers (shadow_csm.hlsli:19), or NULL to unbind (the buffer is
 * then ignored).  `params`: a uniform buffer holding CSMParams (shadow_csm.hlsli:23-39, 336 B, range >= 336; range 0 = to the end of the buffer):
 * Cascades[k].ViewProjection @80k (the convention of ShadowParams.LightSpaceMatrix / CameraData.viewProjection), Cascades[k].SplitDepth @80k + 64,
 * ShadowBias @320, NormalBias @324, ShadowMapSize @328.  The binding lives with the command buffer like the textures and is latched per draw.
 * A MODEL_PBR draw recorded with cascades bound multiplies the directional light by CalculateShadowCSM (shadow_csm.hlsli:163-194,
 * model_pbr_ibl_csm.hlsl:280-298) instead of by 1: SelectCascade on SV_Position.z (the depth the draw's scope resolves for the pixel), one
 * 3 x 3 PCF in the selected layer with the comparison sampler of MIRHI_TEXTURE_SHADOW_MAP (taps are clamped to the edge WITHIN the layer), offsets of
 * 1 / ShadowMapSize on both axes.  MODEL / MODEL_FULL / TRIANGLE ignore the binding.  A MODEL_PBR draw with a single shadow map AND cascades bound is
 * refused (InvalidHandle), as are single-map and cascaded draws in one rendering scope; a cascaded draw's pipeline may not blend, discard fragments
 * or use a predicate depth state, and needs the depth test (its depth key is where SV_Position.z comes from). */
mirhi_result mirhi_cmd_bind_shadow_cascades(mirhi_cmd* cmd, mirhi_image* array, mirhi_buffer* params, uint64_t offset, uint64_t range);
/* The same binding with cascade blending: a MODEL_PBR / MODEL_PBR_IBL draw recorded under it multiplies the directional light by CalculateShadowCSMBlended
 * (shadow_csm.hlsli:212-277) -- the selected cascade's PCF and, for a pixel whose depth lies within blend_threshold x (the cascade's split range) in front of
 * its split, the next cascade's, blended by the distance to the split (no seam at a split depth).  Validation, lifetime and latching are those of
 * mirhi_cmd_bind_shadow_cascades; blend_threshold is `blendThreshold`, latched per draw with the binding.  A threshold that is not finite, below 0 or above
 * 1 is refused (InvalidHandle, "unsupported:").  0.0 is legal and records exactly what mirhi_cmd_bind_shadow_cascades records (which implies a threshold
 * of 0); array == NULL unbinds either way, and mirhi_cmd_begin* / mirhi_cmd_reset clear the threshold with the binding.  Every refusal of a cascaded draw
 * holds for a blended one; blended and unblended cascaded draws may share a rendering scope.  Cascade 3 never blends; cascade 0 measures its range from 0. */
mirhi_result mirhi_cmd_bind_shadow_cascades_blended(mirhi_cmd* cmd, mirhi_image* array, mirhi_buffer* params, uint64_t offset, uint64_t range, float blend_threshold);
/* The IBL set: descriptor set 3 of pixel/model_pbr_ibl.hlsl:133-155 (= model_pbr_ibl_csm.hlsl) -- TextureCube irradianceMap (t7), TextureCube prefilteredMap
 * (t8), Texture2D<float4> brdfLUT (t9): what mirhi_ibl_irradiance, mirhi_ibl_prefilter and mirhi_ibl_brdf_lut make (or any upload of the same shape).  All three
 * NULL unbinds the set; mirhi_cmd_begin* and mirhi_cmd_reset clear it, as they clear the cascades.  The set lives with the command buffer and is latched by
 * MIRHI_PROGRAM_MODEL_PBR_IBL draws; draws of every other program ignore it (their frames keep their bits).  There is no texture slot for these images:
 * MIRHI_TEXTURE_COUNT stays 6 and a cube stays refused at every mirhi_texture_slot.
 *
 * What a MODEL_PBR_IBL fragment computes -- the build's reading of the shader, with the sampler stated above ("IBL precompute", "The sampler"):
 *   Front half, the three light loops and the shadow term: model_pbr_ibl.hlsl:205-346, line for line those of model_pbr.hlsl (same device code).
 *   Ambient (:355-384).  ambient = (kD * irradiance * albedo + prefiltered * (F0 * brdf.x + brdf.y)) * ao with F0 = lerp(0.04, albedo, metallic) (:356),
 *     NdotV = max(dot(N, V), 0) (:359), F = FresnelSchlickRoughness(NdotV, F0, roughness) = F0 + (max(1 - roughness, F0) - F0) * (1 - saturate(NdotV))^5
 *     (:362, pbr.hlsli:147-152), kD = (1 - F) * (1 - metallic) (:365-366), R = reflect(-V, N) = 2 dot(N, V) N - V (:259), N = GetWorldNormal's result,
 *     roughness taken after ClampRoughness (:262: max(roughness, 0.04)).
 *   Final colour (:393-395).  color = ambient + Lo + emissive, alpha = baseColor.a.  There is no hemisphere ambient, and Lo is NOT multiplied by
 *     lerp(1, ao, 0.5): that factor is model_pbr.hlsl's alone (model_pbr.hlsl:311).
 *   irradianceMap.Sample(N) (:369) is the cube lookup at lod 0 (level 0 of `irradiance`; further levels are never read); .rgb is used.
 *   prefilteredMap.SampleLevel(R, roughness * MAX_REFLECTION_LOD) (:373-377) is the cube lookup at lod = roughness * 7.0: MAX_REFLECTION_LOD = 7.0 stays
 *     hard-coded (pbr.hlsli:373) whatever the cube's chain; the sampler clamps the lod to [0, levels - 1] as stated, so a 5-level cube saturates at
 *     roughness 4/7 and an 8-level one uses its whole chain.
 *   brdfLUT.Sample(float2(NdotV, roughness)) (:380) is bilinear at level 0 with clamp to edge on both axes -- the filter of one cube face applied to
 *     the n x n image: x = NdotV n - 1/2 along a row, y = roughness n - 1/2 down the rows; only .rg is read.
 *   Numerics: float32, not bit-exact -- the ambient term contracts and is bounded against the float64 model of renderer-rs_amd/ibl.py; Lo
 *   keeps MODEL_PBR's exact sequences.  Where the two largest |components| of N or R tie, float32 may select another face than exact arithmetic, and the
 *   stated sampler is not seamless there unless the cube's seamless state is on (then the lookup is continuous and the flip costs nothing).
 * Refused with InvalidHandle: `irradiance` or `prefiltered` that is no cube; a `brdf_lut` that is a cube, an array (or layer view), not square or not
 * R32G32B32A32_SFLOAT; some arguments NULL but not all; images of two devices or of another device than `cmd`.  At the draw: a MODEL_PBR_IBL draw with no
 * IBL set bound; with blending, fragment discard or a predicate depth state (the rule of the shadowed variants); a rendering scope whose MODEL_PBR_IBL
 * draws were recorded under two different sets (unsupported: the set is per scope); the single-map / cascades rules of MODEL_PBR apply unchanged.
 * `discard` below alphaCutoff (:216-220) is decided per draw as for MODEL_PBR; a draw that would need it per fragment is reported at the fence ("alpha cutoff").
 * The images are ordered across queue lanes like shadow maps a scope samples; the mirhi_ibl_ passes wait for every lane, so a pass on a bound image never
 * overlaps a frame that samples it. */
mirhi_result mirhi_cmd_bind_ibl(mirhi_cmd* cmd, mirhi_image* irradiance, mirhi_image* prefiltered, mirhi_image* brdf_lut);
/* SKYBOX: set 0, bindings 0 / 1 of pixel/skybox.hlsl (TextureCube environmentMap + sampler).  `environment`: an R32G32B32A32_SFLOAT cube of the command
 * buffer's device with any number of levels; NULL unbinds; mirhi_cmd_begin* and mirhi_cmd_reset clear it.  There is no texture slot for it either.
 *
 * What a MIRHI_PROGRAM_SKYBOX draw is -- the build's reading of the two shaders:
 *   The draw is mirhi_cmd_draw(cmd, 3, 1, 0, 0): no vertex buffer, no index buffer.  One primitive, the triangle with clip positions (-1, -1, 1, 1),
 *     (3, -1, 1, 1), (-1, 3, 1, 1) from SV_VertexID (vertex/skybox.hlsl:20-35).  It goes through the draw's viewport and scissor like any triangle (snapped
 *     to 1 / 256 pixel, top-left rule; the part outside the viewport rectangle is covered too and is the scissor's to cut), is kept or culled by
 *     cull_mode / front_face under the geometry kernel's winding rule (a negative-height viewport flips it), and takes one primitive id, which the
 *     prim-id attachment holds wherever the sky is visible.  Its depth is the viewport's max_depth (z = w = 1).
 *   Push constants (vertex/skybox.hlsl:5-9): bytes [0, 64) at the time of the draw are inverseViewProjection, in the memory convention of
 *     CameraData.viewProjection.  They are latched when the draw is recorded; a later mirhi_cmd_push_constants does not change a recorded draw.
 *   Direction (vertex/skybox.hlsl:40-42, pixel/skybox.hlsl:24).  At each vertex w = M (x, -y, 1, 1), LocalPos = w.xyz / w.w, computed on the host in
 *     double from the float32 matrix (no less exact than the shader's float32); per pixel LocalPos is the AFFINE interpolation of the three vertex values at the pixel centre (all clip w are 1: perspective-correct and
 *     linear interpolation coincide) -- not M clip / w per pixel, which differs when M's last row has x or y in it; then normalize.
 *   Colour (pixel/skybox.hlsl:25-30): the cube lookup of "IBL precompute" at lod 0, all four channels, written through the colour store and encoding of a
 *     raster resolve for both colour formats.  Lod 0 is a stated deviation like irradianceMap.Sample's above: `Sample` takes an implicit lod, the path has
 *     no derivatives.  Numerics as for MODEL_PBR_IBL: float32, not bit-exact, bounded against the float64 model.
 *   Depth state: every compare op, with or without the depth test and depth write, under CLEAR or LOAD of colour and depth.  A fragment passes when
 *     compare(max_depth, stored) holds (always, with the test off); with depth write the stored depth becomes max_depth; NEVER keeps the id and draws
 *     nothing.  The reference draws it after the models with LESS_OR_EQUAL and no write; drawn first into cleared attachments it fills the frame.
 *     In a scope without a depth_image `stored` is what the scope's earlier segments resolved (depth stays on chip / in the library's own buffer, as
 *     for every depth-testing draw), or clear_depth when nothing was drawn before the sky.
 *   A SKYBOX draw is always a segment of its rendering scope of its own.  The environment is ordered across queue lanes like the IBL set.
 * Refused with InvalidHandle: a non-cube, another format or another device's image here; at the draw: no environment bound; vertex_count != 3,
 * first_vertex != 0 or instance_count > 1; mirhi_cmd_draw_indexed or an indirect draw with a SKYBOX pipeline; a pipeline with blend_enable or
 * fragment_discard_enable; a depth-only rendering scope.  A pipeline that pairs SKYBOX with another program is refused at creation (ShaderError). */
mirhi_result mirhi_cmd_bind_skybox(mirhi_cmd* cmd, mirhi_image* environment);
mirhi_result mirhi_cmd_set_viewport(mirhi_cmd* cmd, const mirhi_viewport* viewport);  /* set_viewport :522 */
mirhi_result mirhi_cmd_set_scissor(mirhi_cmd* cmd, const mirhi_rect2d* scissor);      /* set_scissor :549 */
/* instance_count > 1 (at most 4096): the path has no instance-rate input (binding 0 is per-vertex, vertex.rs:35-41,130-136; no program
 * reads SV_InstanceID), so instance i draws the same primitives again behind instance i - 1; first_instance has nothing to offset. */
mirhi_result mirhi_cmd_draw(mirhi_cmd* cmd, uint32_t vertex_count, uint32_t instance_count, uint32_t first_vertex, uint32_t first_instance); /* draw :583 */
mirhi_result mirhi_cmd_draw_indexed(mirhi_cmd* cmd, uint32_t index_count, uint32_t instance_count, uint32_t first_index, int32_t vertex_offset, uint32_t first_instance); /* draw_indexed :610 */

/* draw_indirect :630 / draw_indexed_indirect :646 (VkDrawIndirectCommand: 4 x u32; VkDrawIndexedIndirectCommand: 4 x u32 + i32 vertexOffset at
 * word 3).  The arguments live in a device buffer; this build READS THEM WHEN THE COMMAND IS RECORDED (one synchronous device -> host copy of
 * draw_count x stride bytes) and records the equivalent direct draws -- Vulkan reads them when the command executes, so a command buffer
 * whose indirect arguments change afterwards must be recorded again.  stride: multiple of 4, >= 16 / 20 when draw_count > 1. */
mirhi_result mirhi_cmd_draw_indirect(mirhi_cmd* cmd, mirhi_buffer* buffer, uint64_t offset, uint32_t draw_count, uint32_t stride);
mirhi_result mirhi_cmd_draw_indexed_indirect(mirhi_cmd* cmd, mirhi_buffer* buffer, uint64_t offset, uint32_t draw_count, uint32_t stride);
/* push_constants / push_constants_bytes :732-769.  Validated as Vulkan does (offset and length multiples of 4, offset + length <= 128) and kept
 * with the command buffer (mirhi_cmd_begin* and mirhi_cmd_reset zero them); MIRHI_PROGRAM_SKYBOX reads bytes [0, 64) when its draw is recorded,
 * no other program reads any. */
mirhi_result mirhi_cmd_push_constants(mirhi_cmd* cmd, uint32_t stage_flags, uint32_t offset, const void* data, uint32_t len);

/* ---- Transfer commands: the transfer group of CommandBuffer (crates/rhi/src/command.rs:844-1019) ------------------------------------------
 * copy_buffer :844, copy_buffer_to_image :860, copy_image_to_buffer :886, copy_image :913, blit_image :943, clear_color_image :977,
 * clear_depth_stencil_image :1003.  The semantics are the Vulkan specification's (vkCmdCopyBuffer, vkCmdCopyBufferToImage, vkCmdCopyImageToBuffer,
 * vkCmdCopyImage, vkCmdBlitImage, vkCmdClearColorImage, vkCmdClearDepthStencilImage), stated here once.
 *
 * Where.  Recorded outside a rendering scope; inside one the call returns MIRHI_ERR_DEVICE.  They execute in recording order with the rendering scopes
 *   of their command buffer, on its queue lane: a scope recorded before a transfer has stored its attachments when the transfer runs, a scope recorded
 *   after it (LOAD) finds what the transfer wrote.  A command buffer that holds a transfer never takes the batched submit form.
 * Ordering across lanes.  A destination image is ordered like an attachment and a source image like a sampled shadow map (a layer view stands for
 *   its array): a submit on another lane that uses the image waits for it and is waited for.  Buffers keep the documented rule: work on different
 *   lanes is unordered unless a fence is waited.  mirhi_buffer_write waits for the pending submissions whose transfers read or write the buffer.
 * Images taken.  2-D images, layer views (one layer of a D32_SFLOAT array) and, through mip_level, the levels of an image with a chain (level l has
 *   max(1, width >> l) x max(1, height >> l) texels).  An array object or a cube as the handle is refused (InvalidHandle), as everywhere else.
 *   There are no image layouts, no 3-D regions, no aspect masks and no subresource ranges: a clear takes the whole image.
 * Tile split.  Not split: every rank moves what its own memory holds (mirhi_device_set_tile_split).
 *
 * Copies move raw texels, no conversion.  mirhi_cmd_copy_image needs equal texel size and both colour or both D32_SFLOAT (so B8G8R8A8_SRGB <->
 *   R8G8B8A8_UNORM copies the bytes as they are).  Buffer <-> image copies take every format; texel (x, y) of the region sits at
 *   buffer_offset + ((y * row_length) + x) * texel size, row_length = buffer_row_length, or image_extent[0] when that is 0 (tightly packed);
 *   buffer_row_length / buffer_image_height, when not 0, must be at least the extent.
 * Refused at record time (InvalidHandle; the message names the cause): a region outside its resource, offsets that overflow, a zero extent or
 *   size, region_count 0 or above 16, overlapping source and destination ranges of one resource, a buffer_offset that is not a multiple of the
 *   texel size, resources of another device than the command buffer's.
 *
 * Blit.  Source and destination are each one of B8G8R8A8_SRGB, R8G8B8A8_UNORM, R8G8B8A8_SRGB, R32G32B32A32_SFLOAT (D32_SFLOAT and R32_UINT are
 *   refused) and must be different images.  A region maps the source rectangle src_offsets[0] .. src_offsets[1] onto the destination rectangle
 *   dst_offsets[0] .. dst_offsets[1]; every corner lies inside its level ([0, width] x [0, height]); a rectangle of zero area is refused.
 *   For destination texel (i, j) of the region, min(xdst0, xdst1) <= i < max(xdst0, xdst1):
 *       u = (i + 1/2 - xdst0) * (xsrc1 - xsrc0) / (xdst1 - xdst0) + xsrc0,      v likewise from j and the y offsets.
 *   Reversed offsets on either side flip the image.  NEAREST takes texel (floor(u), floor(v)).  LINEAR takes the four texels (i0, j0), (i0 + 1, j0),
 *   (i0, j0 + 1), (i0 + 1, j0 + 1), i0 = floor(u - 1/2), j0 = floor(v - 1/2), with the weights a = frac(u - 1/2), b = frac(v - 1/2):
 *       ((1 - a) t00 + a t10) (1 - b) + ((1 - a) t01 + a t11) b.      Indices are clamped to the level's edge.
 *   floor and frac are exact (the offsets are integers: the quotient is formed in integer arithmetic), a weight is rounded to float32 once.
 *   Conversion: an sRGB source is decoded per texel before the filter, through the 256-entry table the samplers use; alpha is linear (a / 255).
 *   A store to an 8-bit destination is the raster resolve's: saturate, the sRGB OETF on RGB of an _SRGB format, round-to-nearest-even of x * 255,
 *   in the destination's byte order.  A float destination is stored unclamped.
 * Clears.  A clear is a blit store of one value to every texel: mirhi_cmd_clear_color_image takes the four blit formats and clears every level of
 *   the image; mirhi_cmd_clear_depth_stencil_image takes D32_SFLOAT only (the path has no stencil) and stores `depth` as it is -- the whole image,
 *   or the one layer a layer view stands for. */
typedef struct { uint64_t src_offset, dst_offset, size; } mirhi_buffer_copy;                     /* VkBufferCopy */
typedef struct { uint64_t buffer_offset; uint32_t buffer_row_length, buffer_image_height;        /* VkBufferImageCopy, 2-D, one layer; */
                 uint32_t mip_level; int32_t image_offset[2]; uint32_t image_extent[2]; } mirhi_buffer_image_copy;  /* 0 = tightly packed */
typedef struct { uint32_t src_mip_level; int32_t src_offset[2]; uint32_t dst_mip_level; int32_t dst_offset[2]; uint32_t extent[2]; } mirhi_image_copy;   /* VkImageCopy */
typedef struct { uint32_t src_mip_level; int32_t src_offsets[2][2]; uint32_t dst_mip_level; int32_t dst_offsets[2][2]; } mirhi_image_blit;              /* VkImageBlit: offsets[corner][x, y] */
typedef enum { MIRHI_FILTER_NEAREST = 0, MIRHI_FILTER_LINEAR = 1 } mirhi_filter;                 /* VkFilter */
mirhi_result mirhi_cmd_copy_buffer(mirhi_cmd* cmd, mirhi_buffer* src, mirhi_buffer* dst, uint32_t region_count, const mirhi_buffer_copy* regions);
mirhi_result mirhi_cmd_copy_buffer_to_image(mirhi_cmd* cmd, mirhi_buffer* src_buffer, mirhi_image* dst_image, uint32_t region_count, const mirhi_buffer_image_copy* regions);
mirhi_result mirhi_cmd_copy_image_to_buffer(mirhi_cmd* cmd, mirhi_image* src_image, mirhi_buffer* dst_buffer, uint32_t region_count, const mirhi_buffer_image_copy* regions);
mirhi_result mirhi_cmd_copy_image(mirhi_cmd* cmd, mirhi_image* src_image, mirhi_image* dst_image, uint32_t region_count, const mirhi_image_copy* regions);
mirhi_result mirhi_cmd_blit_image(mirhi_cmd* cmd, mirhi_image* src_image, mirhi_image* dst_image, uint32_t region_count, const mirhi_image_blit* regions, mirhi_filter filter);
mirhi_result mirhi_cmd_clear_color_image(mirhi_cmd* cmd, mirhi_image* image, const float color[4]);          /* the whole image, every level */
mirhi_result mirhi_cmd_clear_depth_stencil_image(mirhi_cmd* cmd, mirhi_image* image, float depth);           /* D32_SFLOAT: the whole image (a layer view: that layer) */

/* ---- submit + sync: vkQueueSubmit (renderer.rs:407-424, frame_manager.rs:439-462), Fence (sync.rs:168-298) */
mirhi_result mirhi_queue_submit(mirhi_device* dev, uint32_t cmd_count, mirhi_cmd* const* cmds, mirhi_fence* fence /* may be NULL */);
mirhi_result mirhi_fence_create(mirhi_device* dev, uint32_t signaled, mirhi_fence** out);   /* Fence::new :168 */
mirhi_result mirhi_fence_wait(mirhi_fence* fence, uint64_t timeout_ns);                     /* Fence::wait :228 (UINT64_MAX = forever) */
mirhi_result mirhi_fence_reset(mirhi_fence* fence);                                         /* Fence::reset :264 */
mirhi_result mirhi_fence_status(mirhi_fence* fence);    /* MIRHI_OK = signaled, MIRHI_NOT_READY = unsignaled; Fence::is_signaled :294 */
mirhi_result mirhi_fence_destroy(mirhi_fence* fence);

/* ---- measurement: per-dispatch device time, fragment statistics ---------------------------------- */
typedef enum { MIRHI_KERNEL_GEOMETRY = 0, MIRHI_KERNEL_RASTER = 1, MIRHI_KERNEL_VERTEX = 2, MIRHI_KERNEL_FRAGMENT_COUNT = 3,
               MIRHI_KERNEL_COUNT = 4 } mirhi_kernel_id;
/* enable: 0 = off, or a mask of
 *   MIRHI_PROFILE_TIMING     every kernel dispatch carries its own event pair (hipExtLaunchKernelGGL start / stop events): the
 *                            duration is the dispatch's begin -> end on the GPU clock, as rocprofv3 --kernel-trace reports it;
 *                            no event-record commands enter the stream and nothing is subtracted
 *   MIRHI_PROFILE_FRAGMENTS  fragment statistics (below): one extra counting kernel per scope and a few instructions in the
 *                            resolve -- never combine with a throughput measurement */
enum { MIRHI_PROFILE_TIMING = 1, MIRHI_PROFILE_FRAGMENTS = 2 };
/* MIRHI_PROFILE_TIMING | MIRHI_PROFILE_ONE_LANE(k): only the dispatches of queue lane k are timed; the other lanes run as in an
 * untimed frame loop (a timed dispatch is completed through its own signal and overlaps its neighbours less than an untimed one) */
#define MIRHI_PROFILE_ONE_LANE(k) ((((uint32_t)(k) + 1u) & 0xFFu) << 8)
mirhi_result mirhi_device_set_profiling(mirhi_device* dev, uint32_t enable);
/* accumulated since the last reset; waits for outstanding dispatches */
mirhi_result mirhi_device_kernel_time(mirhi_device* dev, mirhi_kernel_id kernel, double* total_ms, uint64_t* launches);
/* every timed dispatch since the last reset, in submission order: begin / end in microseconds on one GPU time axis that starts
 * at the begin of the first of them -- overlap between the queue lanes' kernels and the gaps between dependent launches can be
 * read off directly.  Writes min(capacity, *count) records; `out` may be NULL to query the count. */
typedef struct { uint32_t kernel /* mirhi_kernel_id */, lane; double begin_us, end_us; } mirhi_dispatch_time;
mirhi_result mirhi_device_timeline(mirhi_device* dev, mirhi_dispatch_time* out, uint32_t capacity, uint32_t* count);
/* SURVEY 8d "shaded Mpix/s ... report overdraw separately", summed over the scopes rendered with MIRHI_PROFILE_FRAGMENTS since
 * the last reset: shaded_pixels = pixels whose fragment program ran (the winners of the depth resolve: this design shades
 * visible pixels only), covered_fragments = pixel centres covered by a triangle before any depth test (what a GPU's
 * rasterizer emits); overdraw = covered_fragments / shaded_pixels.  Blended (ordered) segments are not counted. */
mirhi_result mirhi_device_fragment_stats(mirhi_device* dev, uint64_t* shaded_pixels, uint64_t* covered_fragments, uint64_t* scopes);
mirhi_result mirhi_device_reset_kernel_times(mirhi_device* dev);   /* also clears the timeline and the fragment statistics */
typedef struct {
    uint64_t frames_submitted;      /* rendering scopes executed */
    uint64_t triangles_submitted;   /* input triangles over those scopes */
    uint64_t workspace_bytes;       /* HBM held for bins / records */
    uint32_t last_big_list;         /* triangles that took the large/overflow list in the last finished scope */
    uint32_t last_status;           /* device status word of the last finished scope (0 = ok; bit 2: the bin pool ran out and is grown) */
    uint32_t last_bin_pages;        /* 2 KB bin pages the last finished scope took from the pool (beyond each tile's fixed first page) */
    uint32_t native_dispatches;     /* kernels this device dispatched as AQL packets on its own ROCr queues (csrc/mirhi_native.h) instead of through
                                       HIP launches (low 32 bits of the count); 0 on a device whose native dispatcher could not start */
    uint32_t dispatch_path;         /* how a plain submit leaves the library: 0 HIP launches (mirhi_device_dispatch_path says why), 1 AQL packets on the
                                       device's own hardware queues, 2 AQL packets on a queue a tool intercepts (MIRHI_NATIVE_DISPATCH=2 only) */
    uint32_t device_lost;           /* 1: a wait on one of the device's queues ran into its deadline; every later submit and wait fails with VulkanError */
    uint32_t reserved;
} mirhi_device_stats;
mirhi_result mirhi_device_get_stats(mirhi_device* dev, mirhi_device_stats* out);
/* "native: ..." or "hip: <why the native dispatcher is not used>", NUL-terminated into out[0 .. out_len) */
mirhi_result mirhi_device_dispatch_path(mirhi_device* dev, char* out, uint32_t out_len);
/* Measurement: round trip of ONE dispatch on queue lane `lane`, host store of the packet -> host sees its completion signal, averaged over `reps` dispatches
 * one at a time: [0] an empty one-wave kernel (doorbell -> packet processor -> wave -> end-of-kernel release -> signal -> host), [1] a barrier packet (no
 * wave).  What a fence-gated frame pays around its kernels.  Fails with LoadingError on a device without native dispatch. */
mirhi_result mirhi_device_measure_roundtrip(mirhi_device* dev, uint32_t lane, uint32_t reps, double* out_us /* [2] */);
/* the build this library is: first 16 hex digits of the sha256 over csrc/ and include/mirhi.h (renderer-rs_amd/build.py::source_hash).  The code object the
 * native dispatcher loads (libmirhi_kernels.hsaco) carries the same id and is refused if it differs. */
const char* mirhi_build_id(void);

/* ---- multi-GPU: screen-tile-row split + exchange of the finished RGBA bands over RCCL / xGMI ------------------
 * The reference drives one VkDevice (crates/rhi/src/device.rs:61-77) and has nothing to mirror here; BASELINE.json's north_star
 * defines the split.  One process per GPU: every rank creates its device, calls mirhi_device_set_tile_split(rank, world)
 * (mirhi_comm_create does it), renders -- only its band of 32-pixel tile rows is rasterized -- and calls
 * mirhi_comm_all_gather_bands on the frame: afterwards every rank holds the whole image.  librccl is loaded with dlopen the
 * first time one of these functions runs: a single-GPU host never loads or initialises RCCL. */
typedef struct mirhi_comm mirhi_comm;
#define MIRHI_COMM_ID_BYTES 128                     /* = NCCL_UNIQUE_ID_BYTES */
/* rank 0: fills `id` (ncclGetUniqueId); ship the 128 bytes to the other ranks over any host channel (the launcher's) */
mirhi_result mirhi_comm_unique_id(uint8_t* id /* [MIRHI_COMM_ID_BYTES] */);
/* collective over all `world` ranks (ncclCommInitRank); also applies mirhi_device_set_tile_split(dev, rank, world) */
mirhi_result mirhi_comm_create(mirhi_device* dev, const uint8_t* id, uint32_t rank, uint32_t world, mirhi_comm** out);
uint32_t mirhi_comm_world(const mirhi_comm* comm);  /* ranks RCCL counts in the communicator (ncclCommCount) */
uint32_t mirhi_comm_rank(const mirhi_comm* comm);
typedef enum {
    MIRHI_GATHER_DIRECT = 0,      /* one grouped batch of ncclSend / ncclRecv: every rank sends its band straight to every peer --
                                     xGMI is a full mesh of point-to-point links, so the 7 transfers of a rank run in parallel
                                     (4K BGRA8 on 8 GPUs: 4.15 MB per link) where a ring would pass 7 hops one after another */
    MIRHI_GATHER_BROADCAST = 1    /* one grouped batch of `world` in-place ncclBroadcast, one band each; RCCL picks the algorithm */
} mirhi_gather_algo;
/* In place on `frame` (a colour image every rank created with the same extent and format): the rows this rank rendered -- its band, or with interleaved
 * rows one 32-row piece per tile row it owns (mirhi_device_split_rows) -- are sent, the other ranks' rows received, all pieces in ONE RCCL group.  Shares may
 * differ in size (the last band / tile row is short when the rows do not divide).  Enqueued on the queue lane of `after` (the command buffer that rendered the
 * frame; NULL = lane 0), so it runs behind that frame's raster kernel; completion through mirhi_device_wait_idle or a later
 * submit on the same lane. */
mirhi_result mirhi_comm_all_gather_bands(mirhi_comm* comm, mirhi_image* frame, mirhi_cmd* after, mirhi_gather_algo algo);
mirhi_result mirhi_comm_destroy(mirhi_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* MIRHI_H */
