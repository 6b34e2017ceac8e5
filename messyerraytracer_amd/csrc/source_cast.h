// source_cast.h -- host side of the record-driven casts (include/mrt_hip.h: mrt_cast_shadows, mrt_cast_selected_shadows,
// mrt_cast_reflections, mrt_cast_hemisphere, mrt_cast_bounce and their grid forms): per family what a call refuses before any device
// work (*_invalid: the reason, or null), the kernels' argument from the caller's (fill_*), and the batch the entry point sets on
// TraceParams (*_batch: count, out_fmt and the mode).  host/source_cast_data.cpp; no context, no device and no HIP call, so that
// host/source_cast_data_test.cpp drives all of it alone.  cast.hip keeps the entry points and the run.  The G-buffer family's pair is
// gbuffer.h's (shared with the image pass); its flags are checked with unknown_flag like everyone's.
//
// The order of refusals, first to last.  Every call starts with "null context" (MRT_ERR_INVALID, no text) and then the array form's
// "null rays", or the grid form's grid refusals (grid_params: "bad grid", "bad camera kind", "camera was set up for another
// resolution"); *_invalid(array_entry = true) makes the "null rays" check itself.  Every call ends with "no scene uploaded", "collect
// the pending dispatch first", and only then an empty cast returning MRT_OK with nothing touched.  Between them:
//
//   shadow           unknown flag | more than MRT_MAX_LIGHTS lights | null hits / lights / mask | count * n_lights overflows |
//                    unknown light type
//   selected shadow  null hits | null descriptor | null mask | null d_out_light | n_lights > 0 with null lights | unknown flag |
//                    more than MRT_MAX_LIGHTS lights | unknown light type | frame > MRT_PATH_MAX_FRAME   (pointers before flags)
//   reflection       unknown flag | null hits / output hits | max_distance must be finite and > 0
//   hemisphere       unknown flag | null descriptor | n_samples outside 1 .. MRT_MAX_HEMISPHERE_SAMPLES | t_max must be finite and >
//                    1e-4 | unknown mode | any-hit writes no rays | null hits / output | count * n_samples overflows
//   bounce           unknown flag | null descriptor | t_max must be finite and > 1e-4 | without d_surface: metallic, then roughness,
//                    must be in [0, 1] | null hits / output
//   G-buffer         unknown flag | gb::cast_invalid's (gbuffer.h)
//
// HOST_LAYOUT is a flag of the array forms alone; ASYNC of both.
#pragma once
#include "mrt_internal.h"

static_assert(sizeof(mrt_light_select) == 24, "mrt_light_select must be 24 bytes");

namespace mrt {
namespace sc {

// a flag the entry does not know (array_entry: the form that takes rays and records from arrays)
inline bool unknown_flag(bool array_entry, uint32_t flags)
{
	return (flags & ~((array_entry ? (uint32_t)MRT_FLAG_HOST_LAYOUT : 0u) | (uint32_t)MRT_FLAG_ASYNC)) != 0u;
}

// The generator's seed of record i is i * 1009 + seed_add: pixel0 = the pixel index of record 0 (0 for the array forms, y0 * grid_w
// for a row band, which so draws what the whole frame draws), modulo 2^32.
inline uint32_t seed_add(uint32_t pixel0, uint32_t frame) { return pixel0 * 1009u + frame * 6529u + 7u; }

// What an entry point sets on TraceParams: the entries, the format of an output record and the mode.
struct Batch { uint64_t count; uint32_t out_fmt; int mode; };
// one byte per entry where the result is lit / shadowed, else a record in the layout of the source's input
inline uint32_t out_fmt(int src, int mode)
{
	if (lit_output(src, mode == MRT_MODE_ANY_HIT)) return OUT_BOOL8;
	return src == SRC_REFLECT_HOST || src == SRC_HEMI_HOST || src == SRC_BOUNCE_HOST ? OUT_HOST44 : OUT_HIT32;
}
inline Batch batch(int src, int mode, uint64_t count) { return Batch{count, out_fmt(src, mode), mode}; }
// (count = records; the products do not overflow in a cast that passed *_invalid)
inline Batch shadow_batch(int src, uint64_t count, uint32_t n_lights) { return batch(src, MRT_MODE_ANY_HIT, count * n_lights); }
inline Batch selected_shadow_batch(int src, uint64_t count) { return batch(src, MRT_MODE_ANY_HIT, count); }
inline Batch reflection_batch(int src, uint64_t count) { return batch(src, MRT_MODE_NEAREST, count); }
inline Batch hemisphere_batch(int src, uint64_t count, uint32_t n_samples, int mode) { return batch(src, mode, count * n_samples); }
inline Batch bounce_batch(int src, uint64_t count) { return batch(src, MRT_MODE_NEAREST, count); }

// The kernels' lights from the caller's: OFF for cast_shadows == 0, the direction of a directional light, the position of a point or
// spot light.  The types are known (*_invalid).
void fill_shadow_lights(const mrt_light *lights, uint32_t n_lights, ShadowLight *out);
// The jump of the first draw of every sample (k = first_draw + 2 * sample): one pass over the draws.
void hemisphere_jumps(uint32_t first_draw, uint32_t n_samples, HemiJump *out);

// What a cast refuses, or null, in the order of the table above.  array_entry: d_rays is required; the grid forms pass any pointer.
const char *shadow_invalid(bool array_entry, const void *d_rays, const void *d_hits, uint64_t count, const mrt_light *lights,
		uint32_t n_lights, const uint8_t *d_mask, uint32_t flags);
const char *selected_shadow_invalid(bool array_entry, const void *d_rays, const void *d_hits, const mrt_light_select *desc,
		const mrt_light *lights, uint32_t n_lights, const uint8_t *d_mask, uint32_t flags);
const char *reflection_invalid(bool array_entry, const void *d_rays, const void *d_hits, float max_distance, const void *d_out_hits,
		uint32_t flags);
const char *hemisphere_invalid(bool array_entry, const void *d_rays, const void *d_hits, uint64_t count, const mrt_hemisphere *desc,
		const void *d_out, const void *d_out_rays, int mode, uint32_t flags);
const char *bounce_invalid(bool array_entry, const void *d_rays, const void *d_hits, const mrt_bounce *desc, const void *d_out_hits,
		uint32_t flags);

// The kernels' argument of a cast that passed its *_invalid.  count = records; pixel0 as for seed_add.
void fill_shadow(const void *d_hits, uint64_t count, const mrt_light *lights, uint32_t n_lights, ShadowParams &s);
void fill_selected_shadow(const void *d_hits, const mrt_light_select *desc, const mrt_light *lights, uint32_t n_lights, uint32_t pixel0,
		SelectShadowParams &s); // n_lights >= 1
void fill_reflection(const void *d_hits, const uint8_t *d_select, float max_distance, void *d_out_rays, ReflectParams &s);
void fill_hemisphere(const void *d_hits, uint64_t count, uint32_t pixel0, const mrt_hemisphere *desc, void *d_out_rays, HemiParams &s);
void fill_bounce(const void *d_hits, uint32_t pixel0, const mrt_bounce *desc, void *d_out_rays, BounceParams &s);

} // namespace sc
} // namespace mrt
