// texture.h -- the resident texture set of a context (mrt_upload_textures): the descriptor's checks, the layout of the pooled texel
// buffer and its descriptor table (host/texture_data.cpp), and what the textured resolve takes (surface_kernel.h).  Host-only code
// may include this without HIP.
#pragma once
#include <cstdint>
#include "../../include/mrt_hip.h"

static_assert(sizeof(mrt_texture) == 24, "mrt_texture must be 24 bytes");
static_assert(sizeof(mrt_material_textures) == 16, "mrt_material_textures must be 16 bytes: one 16-byte load");
static_assert(sizeof(mrt_texture_set) == 48, "mrt_texture_set must be 48 bytes");

namespace mrt {

// One texture on the device: 16 bytes, one load.  Texel (x, y) of an RGBA8 image is the 4 bytes at pool + offset16 * 16 +
// (y * width + x) * 4, of an RGBA32F image the 16 bytes at pool + offset16 * 16 + (y * width + x) * 16.
struct TextureDesc { uint32_t offset16, width, height, format; };
static_assert(sizeof(TextureDesc) == 16, "TextureDesc must be 16 bytes");

// What the textured resolve reads besides SurfaceParams (all device pointers; tangents may be null).
struct TextureParams {
	const void *texels;      // the pool
	const void *table;       // n_textures x TextureDesc
	const void *bindings;    // n_bindings x mrt_material_textures
	const void *tangents;    // n_tangent_tris x 48 bytes {t0 xyz, t1 xyz, t2 xyz, sign0, sign1, sign2}, or null
	uint32_t n_bindings, n_tangent_tris;
};

// host/texture_data.cpp (no device, no library)
// Bytes of one texel of a format (0: unknown).
uint32_t texel_bytes(uint32_t format);
// What mrt_upload_textures refuses about its descriptor, in the order include/mrt_hip.h lists, or null.  Reads the texture and the
// binding list, never a pixel or a tangent.
const char *texture_set_invalid(const mrt_texture_set *set);
// The pool's layout of a set that texture_set_invalid passed: table[t] for every texture (each image starts on a 16-byte boundary, in
// list order, nothing between them but that padding); returns the pool's size in 16-byte units.
uint64_t texture_pool_layout(const mrt_texture_set *set, TextureDesc *table);

} // namespace mrt
