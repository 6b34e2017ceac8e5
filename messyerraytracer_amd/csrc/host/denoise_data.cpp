// denoise_data.cpp -- host side of the reflection effect's image passes: the refusals of mrt_denoise_spatial, mrt_denoise_temporal,
// mrt_composite_reflections, mrt_resolve_reflections and mrt_reflection_guides in the order include/mrt_hip.h lists, and the kernel's
// arguments (the clamped radius, the 3x3 of inv_view, the w_spatial table).  No context, no device and no HIP call, so that
// csrc/host/denoise_data_test.cpp drives it alone.
#include "../denoise.h"

namespace mrt {
namespace dn {

namespace {

bool finite(float x) { return x - x == 0.0f; }

} // namespace

const char *denoise_invalid(int call, const mrt_denoise_params *p, uint32_t w, uint32_t h, const void *d_reflection, const void *d_depth,
		const void *d_guide, const void *d_history, const void *d_color, const void *d_out, uint32_t flags)
{
	if (!p) return "null params";
	// the images, each in the order of the call's arguments
	if (!d_reflection) return call == DN_TEMPORAL ? "null d_current" : "null d_reflection";
	if (call != DN_TEMPORAL) {
		if (!d_depth) return "null d_depth";
		if (!d_guide) return "null d_normal_roughness";
	}
	if ((call == DN_TEMPORAL || call == DN_RESOLVE) && !d_history) return "null d_history";
	if ((call == DN_COMPOSITE || call == DN_RESOLVE) && !d_color) return "null d_color";
	if ((call == DN_SPATIAL || call == DN_TEMPORAL) && !d_out) return "null d_out";
	if (p->struct_size != sizeof(mrt_denoise_params)) return "struct_size is not sizeof(mrt_denoise_params)";
	if (flags & ~(uint32_t)MRT_FLAG_ASYNC) return "unknown flag for a denoise call";
	if (p->normal_kind > (uint32_t)MRT_NORMAL_WORLD) return "unknown normal_kind";
	const float scalars[8] = {p->depth_sigma, p->normal_sigma, p->color_sigma, p->blend_factor, p->depth_threshold, p->roughness_threshold,
			p->intensity, p->f0};
	for (float x : scalars)
		if (!finite(x)) return "a non-finite parameter";
	for (float x : p->inv_view)
		if (!finite(x)) return "a non-finite inv_view";
	if (w != 0u && (uint64_t)h > UINT64_MAX / 32u / (uint64_t)w) return "W * H * 32 overflows";
	if (call == DN_SPATIAL && d_out == d_reflection) return "d_out is d_reflection";
	if (call == DN_RESOLVE) {
		const void *outs[3] = {d_history, d_color, d_out}; // (d_out: the optional d_denoised)
		for (const void *o : outs)
			if (o && (o == d_reflection || o == d_depth || o == d_guide)) return "an output is an image read across pixels";
	}
	return nullptr;
}

const char *guides_invalid(const void *d_hits, const void *d_rows, uint64_t count, float inv_depth_range, const void *d_depth,
		const void *d_guide, uint32_t flags)
{
	if (!d_hits) return "null d_hits";
	if (!d_rows) return "null d_rows";
	if (!d_depth) return "null d_depth";
	if (!d_guide) return "null d_normal_roughness";
	if (flags & ~(uint32_t)MRT_FLAG_ASYNC) return "unknown flag for mrt_reflection_guides";
	if (!finite(inv_depth_range)) return "a non-finite inv_depth_range";
	if (count > UINT64_MAX / 64u) return "count * 64 overflows";
	return nullptr;
}

void fill_denoise_args(const mrt_denoise_params *p, uint32_t w, uint32_t h, DenoiseArgs &a)
{
	a = DenoiseArgs{};
	a.w = w; a.h = h;
	a.radius = clamp_radius(p->kernel_radius);
	a.normal_kind = p->normal_kind; a.has_history = p->has_history != 0u;
	a.depth_sigma = p->depth_sigma; a.normal_sigma = p->normal_sigma; a.color_sigma = p->color_sigma;
	a.blend = p->blend_factor; a.depth_threshold = p->depth_threshold; a.roughness_threshold = p->roughness_threshold;
	a.intensity = p->intensity; a.f0 = p->f0;
	for (int c = 0; c < 3; c++)
		for (int r = 0; r < 3; r++) a.m[3 * c + r] = p->inv_view[4 * c + r];
	spatial_table(a.radius, a.w_spatial);
}

} // namespace dn
} // namespace mrt
