// lighting.h -- direct light on resolved surfaces (mrt_light_surfaces, mrt_light_grid_surfaces and their selected forms): the kernel's argument block, pow01 as
// include/mrt_hip.h defines it (one definition for the kernel, light_kernel.h, and the host, so that both hold the same bits), and the
// checks of the light list and the environment (host/light_data.cpp).  Host-only code may include this without HIP.
#pragma once
#include <cstdint>
#include "../../include/mrt_hip.h"

#ifndef MRT_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define MRT_HD __host__ __device__
#else
#define MRT_HD
#endif
#endif

static_assert(sizeof(mrt_shade_light) == 64, "mrt_shade_light must be 64 bytes");
static_assert(sizeof(mrt_environment) == 64, "mrt_environment must be 64 bytes");

namespace mrt {

// One light as the kernel reads it (uniform: a kernel argument): cos_outer = cosf(spot_angle) and 1 - cos_outer from the host.
struct KernelLight {
	uint32_t type;
	float position[3], direction[3], color[3];
	float range, attenuation, spot_attenuation, cos_outer, one_minus_cos_outer;
	uint32_t pad;
};
static_assert(sizeof(KernelLight) == 64, "KernelLight is 16 words");

// Record i of a lighting call is entry i; TraceParams::count = records, rays = the incoming rays as for a resolve (or the grid).
struct LightParams {
	const void *records;       // mrt_hit32 (SURF_RAY32, SURF_GRID) or mrt_host_hit44 (SURF_HOST)
	const void *rows;          // mrt_surface64 per record
	const uint8_t *mask;       // optional: [light * count + record], 0 = shadowed (the selected calls: [record])
	const uint8_t *selected;   // the selected calls only: the one light of each record (>= n_lights: none)
	void *out;                 // float4 per record
	uint32_t n_lights, has_env;
	float zenith[3], horizon[3], ground[3], ambient[3], ambient_energy;
	KernelLight light[MRT_MAX_LIGHTS];
};

// pow01 (include/mrt_hip.h): fp64, one operation at a time, nothing contracted.
MRT_HD inline float pow01(float b, float e)
{
	if (e == 0.0f) return 1.0f;
	if (b == 0.0f) return 0.0f;
	if (b == 1.0f) return 1.0f;
	const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10, INV_LN2 = 1.44269504088896338700e+00;
	const double RND = 6755399441055744.0;
	const double x = (double)b;
	uint64_t bits;
	__builtin_memcpy(&bits, &x, 8);
	int64_t ki = (int64_t)((bits >> 52) & 0x7FFu) - 1023;
	if (ki == 1024) return b; // (infinity, or a NaN, as it stands: outside the domain)
	bits = (bits & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
	double m;
	__builtin_memcpy(&m, &bits, 8);
	if (m > 1.4142135623730951) { m = m * 0.5; ki = ki + 1; }
	const double k = (double)ki;
	const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
	double q = 0.086956521739130432;
	q = q * s2 + 0.095238095238095233; q = q * s2 + 0.10526315789473684; q = q * s2 + 0.11764705882352941;
	q = q * s2 + 0.13333333333333333; q = q * s2 + 0.15384615384615385; q = q * s2 + 0.18181818181818182;
	q = q * s2 + 0.22222222222222221; q = q * s2 + 0.2857142857142857; q = q * s2 + 0.40000000000000002;
	q = q * s2 + 0.66666666666666663; q = q * s2 + 2.0;
	const double lg = k * LN2_HI + (s * q + k * LN2_LO);
	const double y = (double)e * lg;
	if (y < -104.0) return 0.0f;
	if (y > 89.0) return __builtin_inff();
	const double n = (y * INV_LN2 + RND) - RND;
	const double r = (y - n * LN2_HI) - n * LN2_LO;
	double p = 1.6059043836821613e-10;
	p = p * r + 2.08767569878681e-09; p = p * r + 2.505210838544172e-08; p = p * r + 2.7557319223985888e-07;
	p = p * r + 2.7557319223985893e-06; p = p * r + 2.4801587301587302e-05; p = p * r + 0.00019841269841269841;
	p = p * r + 0.0013888888888888889; p = p * r + 0.0083333333333333332; p = p * r + 0.041666666666666664;
	p = p * r + 0.16666666666666666; p = p * r + 0.5; p = p * r + 1.0; p = p * r + 1.0;
	const uint64_t sb = (uint64_t)((int64_t)n + 1023) << 52;
	double scale;
	__builtin_memcpy(&scale, &sb, 8);
	return (float)(p * scale);
}

// host/light_data.cpp (no device, no library)
// What the lighting calls refuse about their light list and environment, or null: in the order include/mrt_hip.h lists.
const char *light_list_invalid(const mrt_shade_light *lights, uint32_t n_lights, const mrt_environment *env, uint64_t count);
// The kernel's lights and environment from the caller's: cos_outer by cosf, here and nowhere else.
void fill_light_params(const mrt_shade_light *lights, uint32_t n_lights, const mrt_environment *env, LightParams &lp);
// mrt_shadow_lights
void shadow_lights(const mrt_shade_light *lights, uint32_t n, mrt_light *out);

} // namespace mrt
