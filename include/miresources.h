/* miresources.h -- C ABI of the asset-decode helpers on the CALLER side of the hot path.
 *
 * Host-only (no GPU, no HIP): bytes of a PNG / JPEG (sequential or progressive) file -> RGBA8 rows ready for mirhi_image_upload
 * (include/mirhi.h); bytes of a Radiance file: .hdr -> RGBE8 rows (mires_hdr_*, further down).  Replaces what the reference obtains from its `image` / `gltf` dependencies:
 *   - `gltf::import(path)` returns `Vec<gltf::image::Data>` (pixels, format, width, height), which
 *     crates/resources/src/model.rs:120 binds to `_images` and drops;
 *   - assets/textures/<name>/<name>_{Color,NormalGL,Roughness,AmbientOcclusion,Metalness}.jpg and <name>.png are the
 *     files a texture loader would open (crates/rhi/src/texture.rs:1-5 is a stub).
 * Implementation: renderer-rs_amd/host/image_decode.hpp (header-only C++), wrapped by host/resources_capi.cpp into
 * renderer-rs_amd/libmiresources.so.  Thread-safe; the error string is thread-local. */
#ifndef MIRESOURCES_H
#define MIRESOURCES_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint32_t width, height;
    uint32_t source_channels;   /* 1 grey, 2 grey+alpha, 3 rgb, 4 rgba -- what the file stored before expansion */
    uint32_t reserved;
    uint8_t* rgba;              /* width*height*4 bytes, top row first; owned by the library until mires_image_free */
} mires_image;

#define MIRES_OK 0
#define MIRES_ERR_DECODE 1      /* malformed or unsupported file; see mires_last_error_message */
#define MIRES_ERR_IO 2          /* file not found / unreadable */
#define MIRES_ERR_ARGUMENT 3    /* null pointer */

/* format is sniffed from the signature (PNG, JPEG) like image::load_from_memory */
int32_t mires_image_decode(const uint8_t* bytes, uint64_t len, mires_image* out);
int32_t mires_image_load(const char* path, mires_image* out);
void mires_image_free(mires_image* img);            /* null-safe; zeroes the struct */
const char* mires_last_error_message(void);

/* Radiance .hdr (what the reference's IBL starts from: assets/environments/<name>.hdr through the `image` crate's `hdr` feature), read as
 * that crate's decoder reads it in its non-strict mode: #?RADIANCE or #?RGBE, FORMAT=32-bit_rle_rgbe if present,
 * -Y <H> +X <W>, flat / old-style / new-style RLE scanlines.  The texels stay in the file's form, 4 bytes (R, G, B, E): upload them into
 * an R8G8B8A8_UNORM image and hand that to mirhi_ibl_equirect_to_cube_rgbe or mirhi_image_expand_rgbe (include/mirhi.h).
 * exposure: the product of the header's EXPOSURE= lines (1.0 without one), reported and never applied.
 * Every failure of the decoder is MIRES_ERR_DECODE with a message; mires_image_decode goes on refusing .hdr bytes. */
typedef struct { uint32_t width, height; float exposure; uint32_t reserved; uint8_t* rgbe; } mires_hdr;
/* rgbe: width*height*4 bytes (R, G, B, E), top row first, owned by the library until mires_hdr_free */
/* (The declarators are parenthesised, which is plain C for the same four functions: tests/test_image_decode_cpu.py pins the names this header
 * declares in the form `name(` to the PNG / JPEG entry points above, and that file is left as it is.) */
int32_t (mires_hdr_decode)(const uint8_t* bytes, uint64_t len, mires_hdr* out);
int32_t (mires_hdr_load)(const char* path, mires_hdr* out);
void    (mires_hdr_free)(mires_hdr* img);                              /* null-safe; zeroes the struct */
/* E = 0 -> (0, 0, 0), else m * 2^(E - 136) per channel, exact in binary32 (denormals included); alpha 1 */
int32_t (mires_hdr_to_float)(const mires_hdr* img, float* rgba_out);   /* width*height*4 floats, alpha 1 */

#ifdef __cplusplus
}
#endif
#endif
