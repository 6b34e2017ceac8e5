// texture_data.cpp -- host side of mrt_upload_textures: the refusals in the order include/mrt_hip.h lists and the layout of the pooled
// texel buffer with its descriptor table (texture.h).  No device and no HIP call, so that csrc/host/texture_data_test.cpp drives it
// alone.
#include "../texture.h"

#include <cmath>

namespace mrt {

uint32_t texel_bytes(uint32_t format)
{
	return format == MRT_TEXEL_RGBA8 ? 4u : format == MRT_TEXEL_RGBA32F ? 16u : 0u;
}

// 16-byte units of one image (dimensions and format already checked: at most 2^28)
static uint64_t image_units(const mrt_texture &t)
{
	return ((uint64_t)t.width * t.height * texel_bytes(t.format) + 15u) / 16u;
}

const char *texture_set_invalid(const mrt_texture_set *set)
{
	if (!set) return "null texture set descriptor";
	if (set->struct_size != sizeof(mrt_texture_set)) return "mrt_texture_set.struct_size does not match";
	if (set->flags & ~(uint32_t)MRT_TEXTURES_ON_DEVICE) return "unknown flag for a texture set";
	if (set->n_textures && !set->textures) return "n_textures > 0 with null textures";
	if (set->n_bindings && !set->bindings) return "n_bindings > 0 with null bindings";
	if (set->n_tangent_tris && !set->tangents12) return "n_tangent_tris > 0 with null tangents12";
	for (uint32_t t = 0; t < set->n_textures; t++) {
		const mrt_texture &T = set->textures[t];
		if (T.width == 0u || T.height == 0u || T.width > MRT_TEXTURE_MAX_DIM || T.height > MRT_TEXTURE_MAX_DIM)
			return "a texture's width or height is 0 or above MRT_TEXTURE_MAX_DIM";
		if (texel_bytes(T.format) == 0u) return "a texture's format is unknown";
		if (!T.pixels) return "a texture's pixels are null";
	}
	for (uint32_t b = 0; b < set->n_bindings; b++) {
		const mrt_material_textures &B = set->bindings[b];
		if ((B.albedo_texture != MRT_NO_TEXTURE && B.albedo_texture >= set->n_textures) ||
				(B.normal_texture != MRT_NO_TEXTURE && B.normal_texture >= set->n_textures))
			return "a binding's texture index is neither MRT_NO_TEXTURE nor below n_textures";
		if (!std::isfinite(B.normal_scale)) return "a binding's normal_scale is not finite";
	}
	uint64_t units = 0;
	for (uint32_t t = 0; t < set->n_textures; t++) {
		units += image_units(set->textures[t]); // (at most 2^28 each: no wrap below 2^36 textures)
		if (units > 0xFFFFFFFFull) return "the pooled texels exceed what a descriptor's offset addresses (2^32 16-byte units)";
	}
	return nullptr;
}

uint64_t texture_pool_layout(const mrt_texture_set *set, TextureDesc *table)
{
	uint64_t units = 0;
	for (uint32_t t = 0; t < set->n_textures; t++) {
		const mrt_texture &T = set->textures[t];
		table[t].offset16 = (uint32_t)units; table[t].width = T.width; table[t].height = T.height; table[t].format = T.format;
		units += image_units(T);
	}
	return units;
}

} // namespace mrt
