// emitters.h -- emissive triangles as light sources (include/mrt_hip.h: mrt_build_emitters, mrt_cast_emitter_shadows,
// mrt_light_emitter_surfaces, mrt_path_step_emitters and their grid forms): the integer weights of the table as the header states them
// (one definition for the build kernels, emitter_build_kernel.h, and the host), the light kernel's argument block, what each call
// refuses before any device work (*_invalid: the reason, or null) and the kernels' arguments from the caller's (fill_*).
// host/emitter_data.cpp; no context, no device and no HIP call, so that host/emitter_data_test.cpp drives all of it alone.
//
// The order of refusals, first to last.  Every call starts with "null context" (MRT_ERR_INVALID, no text); the grid forms then make
// grid_params' refusals ("bad grid", "bad camera kind", "camera was set up for another resolution") and pass any pointer for d_rays.
//   build            null tris with n_tris > 0 | unknown flag                                  (then MRT_ERR_PENDING)
//   emitter shadow   null rays | null hits | null descriptor | null mask | null d_out_emitter | unknown flag |
//                    frame > MRT_PATH_MAX_FRAME                       (then MRT_ERR_NO_SCENE, MRT_ERR_PENDING, an empty cast MRT_OK)
//   emitter light    null rays | null hits | null rows | null descriptor | null d_out_emitter | null output | unknown flag |
//                    accumulate > 1 | frame > MRT_PATH_MAX_FRAME                               (then MRT_ERR_PENDING, an empty call MRT_OK)
//   emitter step     mrt_path_step's (path.h) | null d_prev_lobe with bounce >= 1
// HOST_LAYOUT is a flag of the array forms alone; ASYNC of both.
#pragma once
#include "mrt_internal.h"

#ifndef MRT_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define MRT_HD __host__ __device__
#else
#define MRT_HD
#endif
#endif

static_assert(sizeof(mrt_emitter_select) == 24, "mrt_emitter_select must be 24 bytes");
static_assert(sizeof(mrt_emitter64) == 64, "mrt_emitter64 must be 64 bytes: four 16-byte loads");

namespace mrt {

// Record i of an emitter light call is entry i; TraceParams::count = records, rays = the incoming rays as for a resolve (or the grid).
struct EmitterLightParams {
	const void *records;       // mrt_hit32 (SURF_RAY32, SURF_GRID) or mrt_host_hit44 (SURF_HOST)
	const void *rows;          // mrt_surface64 per record
	const uint32_t *emitter;   // the cast's words
	const uint8_t *mask;       // optional: 0 = shadowed
	void *out;                 // float4 per record
	EmitterTable table;
	uint32_t accumulate;
	uint32_t seed_add;
	HemiJump jump;
};

namespace em {

// ceil(log2(n)) for n >= 1
MRT_HD inline uint32_t ceil_log2(uint32_t n)
{
	uint32_t k = 0u;
	while (k < 32u && ((uint64_t)1u << k) < n) k++;
	return k;
}
// Q = 2^(31 - ceil_log2(n_emit)) as a float (exact), n_emit in 1 .. MRT_MAX_EMITTERS
MRT_HD inline float weight_scale(uint32_t n_emit) { return (float)(1u << (31u - ceil_log2(n_emit))); }
// q0 = max(1, (uint32)((w / w_max) * Q)): w in (0, w_max], so the product is at most 2^31
MRT_HD inline uint32_t first_weight(float w, float w_max, float Q)
{
	const uint32_t q = (uint32_t)((w / w_max) * Q);
	return q < 1u ? 1u : q;
}
// q = (q0 << 31) / T0, T0 = the sum of every q0 (>= q0, <= 2^31)
MRT_HD inline uint32_t final_weight(uint32_t q0, uint64_t t0) { return (uint32_t)(((uint64_t)q0 << 31) / t0); }

const char *build_invalid(const void *tris, uint32_t n_tris, uint32_t flags);
// array_entry: d_rays is the caller's; the grid forms pass any non-null pointer
const char *shadow_invalid(bool array_entry, const void *d_rays, const void *d_hits, const mrt_emitter_select *desc, const uint8_t *d_mask,
		uint32_t flags);
const char *light_invalid(bool array_entry, const void *d_rays, const void *d_hits, const void *d_rows, const mrt_emitter_select *desc,
		uint32_t accumulate, const mrt_light_out *out, uint32_t flags);
const char *step_invalid(const mrt_path_step_desc *desc, const uint8_t *d_prev_lobe); // after path_step_invalid found nothing

// The kernels' arguments of calls that passed their *_invalid; pixel0 = the pixel index of record 0 (source_cast.h seed_add).
void fill_shadow(const void *d_hits, const mrt_emitter_select *desc, const EmitterTable &table, uint32_t pixel0, EmitterShadowParams &s);
void fill_light(const void *d_hits, const void *d_rows, const mrt_emitter_select *desc, const uint8_t *d_mask, uint32_t accumulate,
		const mrt_light_out *out, const EmitterTable &table, uint32_t pixel0, EmitterLightParams &s);

} // namespace em
} // namespace mrt
