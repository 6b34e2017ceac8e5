// source_cast_data.cpp -- host side of the record-driven casts (source_cast.h): what each family refuses of its arguments, in the order
// the header's table gives, and the kernels' argument.  No context, no device and no HIP call, so that
// csrc/host/source_cast_data_test.cpp drives it alone.
#include "../source_cast.h"

#include <cfloat>
#include <cstring>

namespace mrt {
namespace sc {

namespace {

const char *unknown_light_type(const mrt_light *lights, uint32_t n_lights)
{
	for (uint32_t l = 0; l < n_lights; l++)
		if (lights[l].type > MRT_LIGHT_SPOT) return "unknown light type";
	return nullptr;
}

} // namespace

void fill_shadow_lights(const mrt_light *lights, uint32_t n_lights, ShadowLight *out)
{
	for (uint32_t l = 0; l < n_lights; l++) {
		const mrt_light &L = lights[l];
		ShadowLight &d = out[l];
		d.kind = !L.cast_shadows ? SHADOW_OFF : (L.type == MRT_LIGHT_DIRECTIONAL ? SHADOW_DIRECTIONAL : SHADOW_POINT);
		const float *v = L.type == MRT_LIGHT_DIRECTIONAL ? L.direction : L.position;
		d.v[0] = v[0]; d.v[1] = v[1]; d.v[2] = v[2];
	}
}

void hemisphere_jumps(uint32_t first_draw, uint32_t n_samples, HemiJump *out)
{
	HemiJump j = pcg_jump(first_draw);
	for (uint32_t s = 0; s < n_samples; s++) {
		out[s] = j;
		for (int k = 0; k < 2; k++) { j.a = kPcgMul * j.a; j.c = kPcgMul * j.c + kPcgInc; }
	}
}

// ---- shadow ---------------------------------------------------------------------------------------------------------------------------

const char *shadow_invalid(bool array_entry, const void *d_rays, const void *d_hits, uint64_t count, const mrt_light *lights,
		uint32_t n_lights, const uint8_t *d_mask, uint32_t flags)
{
	if (array_entry && !d_rays) return "null rays";
	if (unknown_flag(array_entry, flags)) return "unknown flag for a shadow cast";
	if (n_lights > MRT_MAX_LIGHTS) return "more than MRT_MAX_LIGHTS lights";
	if (!d_hits || !d_mask || (n_lights && !lights)) return "null hits / lights / mask";
	if (n_lights && count > ~0ull / n_lights) return "count * n_lights overflows";
	return unknown_light_type(lights, n_lights);
}

void fill_shadow(const void *d_hits, uint64_t count, const mrt_light *lights, uint32_t n_lights, ShadowParams &s)
{
	std::memset(&s, 0, sizeof(s));
	s.records = d_hits; s.pixels = count;
	fill_shadow_lights(lights, n_lights, s.light);
}

// ---- selected shadow ------------------------------------------------------------------------------------------------------------------

const char *selected_shadow_invalid(bool array_entry, const void *d_rays, const void *d_hits, const mrt_light_select *desc,
		const mrt_light *lights, uint32_t n_lights, const uint8_t *d_mask, uint32_t flags)
{
	if (!d_rays) return "null rays";
	if (!d_hits) return "null hits";
	if (!desc) return "null descriptor";
	if (!d_mask) return "null mask";
	if (!desc->d_out_light) return "null d_out_light";
	if (n_lights && !lights) return "n_lights > 0 with null lights";
	if (unknown_flag(array_entry, flags)) return "unknown flag for a selected-shadow cast";
	if (n_lights > MRT_MAX_LIGHTS) return "more than MRT_MAX_LIGHTS lights";
	if (const char *why = unknown_light_type(lights, n_lights)) return why;
	if (desc->frame > MRT_PATH_MAX_FRAME) return "frame > MRT_PATH_MAX_FRAME";
	return nullptr;
}

void fill_selected_shadow(const void *d_hits, const mrt_light_select *desc, const mrt_light *lights, uint32_t n_lights, uint32_t pixel0,
		SelectShadowParams &s)
{
	std::memset(&s, 0, sizeof(s));
	s.records = d_hits; s.select = desc->d_select; s.out_light = desc->d_out_light;
	s.seed_add = seed_add(pixel0, desc->frame);
	s.jump = pcg_jump(desc->select_draw);
	s.n_lights = n_lights;
	fill_shadow_lights(lights, n_lights, s.light);
}

// ---- reflection -----------------------------------------------------------------------------------------------------------------------

const char *reflection_invalid(bool array_entry, const void *d_rays, const void *d_hits, float max_distance, const void *d_out_hits,
		uint32_t flags)
{
	if (array_entry && !d_rays) return "null rays";
	if (unknown_flag(array_entry, flags)) return "unknown flag for a reflection cast";
	if (!d_hits || !d_out_hits) return "null hits / output hits";
	if (!(max_distance > 0.0f && max_distance <= FLT_MAX)) return "max_distance must be finite and > 0";
	return nullptr;
}

void fill_reflection(const void *d_hits, const uint8_t *d_select, float max_distance, void *d_out_rays, ReflectParams &s)
{
	std::memset(&s, 0, sizeof(s));
	s.records = d_hits; s.select = d_select; s.out_rays = d_out_rays; s.max_distance = max_distance;
}

// ---- hemisphere -----------------------------------------------------------------------------------------------------------------------

const char *hemisphere_invalid(bool array_entry, const void *d_rays, const void *d_hits, uint64_t count, const mrt_hemisphere *desc,
		const void *d_out, const void *d_out_rays, int mode, uint32_t flags)
{
	if (array_entry && !d_rays) return "null rays";
	if (unknown_flag(array_entry, flags)) return "unknown flag for a hemisphere cast";
	if (!desc) return "null descriptor";
	if (desc->n_samples < 1u || desc->n_samples > MRT_MAX_HEMISPHERE_SAMPLES) return "n_samples outside 1 .. MRT_MAX_HEMISPHERE_SAMPLES";
	if (!(desc->t_max > 1e-4f && desc->t_max <= FLT_MAX)) return "t_max must be finite and > 1e-4 (t_min)";
	if (mode != MRT_MODE_NEAREST && mode != MRT_MODE_ANY_HIT) return "unknown mode";
	if (mode == MRT_MODE_ANY_HIT && d_out_rays) return "any-hit writes no rays: d_out_rays must be null";
	if (!d_hits || !d_out) return "null hits / output";
	if (count > ~0ull / desc->n_samples) return "count * n_samples overflows";
	return nullptr;
}

void fill_hemisphere(const void *d_hits, uint64_t count, uint32_t pixel0, const mrt_hemisphere *desc, void *d_out_rays, HemiParams &s)
{
	std::memset(&s, 0, sizeof(s));
	s.records = d_hits; s.select = desc->d_select; s.out_rays = d_out_rays; s.pixels = count; s.t_max = desc->t_max;
	s.seed_add = seed_add(pixel0, desc->frame);
	hemisphere_jumps(desc->first_draw, desc->n_samples, s.jump);
}

// ---- bounce ---------------------------------------------------------------------------------------------------------------------------

const char *bounce_invalid(bool array_entry, const void *d_rays, const void *d_hits, const mrt_bounce *desc, const void *d_out_hits,
		uint32_t flags)
{
	if (array_entry && !d_rays) return "null rays";
	if (unknown_flag(array_entry, flags)) return "unknown flag for a bounce cast";
	if (!desc) return "null descriptor";
	if (!(desc->t_max > 1e-4f && desc->t_max <= FLT_MAX)) return "t_max must be finite and > 1e-4 (t_min)";
	if (!desc->d_surface) { // (the comparisons are false for a NaN)
		if (!(desc->metallic >= 0.0f && desc->metallic <= 1.0f)) return "metallic must be in [0, 1]";
		if (!(desc->roughness >= 0.0f && desc->roughness <= 1.0f)) return "roughness must be in [0, 1]";
	}
	if (!d_hits || !d_out_hits) return "null hits / output";
	return nullptr;
}

void fill_bounce(const void *d_hits, uint32_t pixel0, const mrt_bounce *desc, void *d_out_rays, BounceParams &s)
{
	std::memset(&s, 0, sizeof(s));
	s.records = d_hits; s.select = desc->d_select; s.surface = desc->d_surface; s.out_rays = d_out_rays; s.out_lobe = desc->d_out_lobe;
	s.t_max = desc->t_max; s.metallic = desc->metallic; s.roughness = desc->roughness;
	s.seed_add = seed_add(pixel0, desc->frame);
	s.jump = pcg_jump(desc->first_draw);
}

} // namespace sc
} // namespace mrt
