// gbuffer_data.cpp -- host side of mrt_cast_gbuffer_reflections and mrt_reflection_image: what the calls refuse of a descriptor and a
// frame size, in the order include/mrt_hip.h lists.  No context, no device and no HIP call, so that csrc/host/gbuffer_data_test.cpp
// drives it alone.
#include "../gbuffer.h"

namespace mrt {
namespace gb {

namespace {

const char *images_null(const mrt_gbuffer *g)
{
	if (!g->d_depth) return "null d_depth";
	if (!g->d_normal_roughness) return "null d_normal_roughness";
	return nullptr;
}

// from struct_size on
const char *fields_invalid(const mrt_gbuffer *g, uint32_t w, uint32_t h)
{
	if (g->struct_size != sizeof(mrt_gbuffer)) return "struct_size is not sizeof(mrt_gbuffer)";
	if (g->normal_kind > (uint32_t)MRT_NORMAL_WORLD) return "unknown normal_kind";
	for (float x : g->inv_projection)
		if (!finite(x)) return "a non-finite inv_projection";
	for (float x : g->inv_view)
		if (!finite(x)) return "a non-finite inv_view";
	if (!(finite(g->roughness_threshold) && g->roughness_threshold > 0.0f)) return "roughness_threshold must be finite and > 0";
	if (!(finite(g->max_distance) && g->max_distance > 0.0f)) return "max_distance must be finite and > 0";
	if (w != 0u && (uint64_t)h > UINT64_MAX / 32u / (uint64_t)w) return "W * H * 32 overflows";
	return nullptr;
}

} // namespace

const char *cast_invalid(const mrt_gbuffer *g, uint32_t w, uint32_t h, const void *d_out_hits)
{
	if (!g) return "null descriptor";
	if (const char *why = images_null(g)) return why;
	if (!d_out_hits) return "null d_out_hits";
	return fields_invalid(g, w, h);
}

const char *image_invalid(const mrt_gbuffer *g, uint32_t w, uint32_t h, const void *d_hits, const void *d_reflection, uint32_t flags)
{
	if (!g) return "null descriptor";
	if (!d_hits) return "null d_hits";
	if (!d_reflection) return "null d_reflection";
	if (flags & ~(uint32_t)MRT_FLAG_ASYNC) return "unknown flag for mrt_reflection_image";
	if (const char *why = images_null(g)) return why;
	return fields_invalid(g, w, h);
}

} // namespace gb
} // namespace mrt
