// panorama.h -- the resident equirectangular panorama of a context (mrt_upload_panorama): the descriptor's checks
// (host/panorama_data.cpp), what the panorama kernels take besides their own blocks, and the sampler as include/mrt_hip.h states it --
// atan2_def, acos_def, the direction's (u, v), the four taps and their weights -- one definition for the kernels (light_kernel.h,
// path_kernel.h) and the host, so that both hold the same bits.  Host-only code may include this without HIP.
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

static_assert(sizeof(mrt_panorama) == 24, "mrt_panorama must be 24 bytes");

// MRT_PANORAMA_ANGLES=0: A/B builds of tools/bench_panorama_frame.py only (MRT_EXTRA_DEFINES) -- (u, v) from two fp32 operations each
// instead of atan2_def and acos_def (other bits, a similar spread over the image), to time the fp64 part by difference.
#ifndef MRT_PANORAMA_ANGLES
#define MRT_PANORAMA_ANGLES 1
#endif

namespace mrt {

// What a panorama kernel reads besides LightParams / PathParams (a kernel argument of its own: those blocks stay as they are).
struct PanoramaParams {
	const void *texels;        // width * height float4, row-major, top row first (device)
	uint32_t width, height;    // 1 .. MRT_PANORAMA_MAX_DIM
	float energy;
	uint32_t pad;
};
static_assert(sizeof(PanoramaParams) == 24, "PanoramaParams is 6 words");

// atan2 of doubles by + - * / alone, the signs read as bits (include/mrt_hip.h, "atan2_def"): the octant's ratio t = min / max in
// [0, 1]; above tan(pi/8) the argument is (min - max) / (min + max) = tan(atan(t) - pi/4), so that |t| <= tan(pi/8) either way and one
// division serves both; atan(t) = t * sum (-1)^k t^2k / (2k + 1), k = 0 .. 15 (the next term is below 2e-14 of the result); then the
// reflections pi/2 - r (|y| > |x|), pi - r (x negative, -0 included) and the sign of y.  Finite arguments; both infinite: NaN.
MRT_HD inline double atan2_core(double y, double x)
{
	const double PI_D = 3.141592653589793, PI_2 = 1.5707963267948966, PI_4 = 0.7853981633974483, TAN_PI_8 = 0.41421356237309503;
	uint64_t yb, xb;
	__builtin_memcpy(&yb, &y, 8);
	__builtin_memcpy(&xb, &x, 8);
	const bool yneg = (yb >> 63) != 0u, xneg = (xb >> 63) != 0u;
	const double ay = yneg ? -y : y, ax = xneg ? -x : x;
	const bool steep = ay > ax;
	const double mx = steep ? ay : ax, mn = steep ? ax : ay;
	double r = 0.0;
	if (!(mx == 0.0)) {
		double num = mn, den = mx, base = 0.0;
		if (mn > TAN_PI_8 * mx) { num = mn - mx; den = mn + mx; base = PI_4; }
		const double t = num / den, t2 = t * t;
		double q = -1.0 / 31.0;
		q = q * t2 + 1.0 / 29.0; q = q * t2 + -1.0 / 27.0; q = q * t2 + 1.0 / 25.0; q = q * t2 + -1.0 / 23.0; q = q * t2 + 1.0 / 21.0;
		q = q * t2 + -1.0 / 19.0; q = q * t2 + 1.0 / 17.0; q = q * t2 + -1.0 / 15.0; q = q * t2 + 1.0 / 13.0; q = q * t2 + -1.0 / 11.0;
		q = q * t2 + 1.0 / 9.0; q = q * t2 + -1.0 / 7.0; q = q * t2 + 1.0 / 5.0; q = q * t2 + -1.0 / 3.0; q = q * t2 + 1.0;
		r = base + t * q;
	}
	if (steep) r = PI_2 - r;
	if (xneg) r = PI_D - r;
	return yneg ? -r : r;
}

// atan2_def: C99's atan2 of two finite floats, rounded once
MRT_HD inline float atan2_def(float y, float x) { return (float)atan2_core((double)y, (double)x); }

// acos_def of c in [-1, 1]: atan2(sqrt((1 - c) * (1 + c)), c) in fp64 (both factors are exact), rounded once
MRT_HD inline float acos_def(float c)
{
	const double y = (double)c;
	return (float)atan2_core(__builtin_sqrt((1.0 - y) * (1.0 + y)), y);
}

// false: a component is an infinity or a NaN
MRT_HD inline bool finite3(float x, float y, float z)
{
	uint32_t a, b, c;
	__builtin_memcpy(&a, &x, 4);
	__builtin_memcpy(&b, &y, 4);
	__builtin_memcpy(&c, &z, 4);
	return (a & 0x7F800000u) != 0x7F800000u && (b & 0x7F800000u) != 0x7F800000u && (c & 0x7F800000u) != 0x7F800000u;
}

// direction_to_equirect_uv (shade_pass.h:233-237) of a finite direction
MRT_HD inline void equirect_uv(float dx, float dy, float dz, float &u, float &v)
{
	constexpr float PI = 3.14159265358979323846f;
	const float c = dy < -1.0f ? -1.0f : (dy > 1.0f ? 1.0f : dy);
#if MRT_PANORAMA_ANGLES
	u = atan2_def(dx, dz) * (0.5f / PI) + 0.5f;
	v = acos_def(c) * (1.0f / PI);
#else
	u = (dx + dz) * (0.5f / PI) + 0.5f;
	v = 0.5f - c * 0.5f;
#endif
}

// the cyclic wrap of a column in [-width, 2 * width) and the clamp of a row: sample_panorama's wrap_x and clamp_y where it calls them
MRT_HD inline int pano_wrap_x(int x, int width)
{
	x = x < 0 ? x + width : x;
	return x >= width ? x - width : x;
}
MRT_HD inline int pano_clamp_y(int y, int height) { return y < 0 ? 0 : (y > height - 1 ? height - 1 : y); }

// The four taps of sample_panorama (shade_pass.h:185-225) at finite (u, v): texel indices (row * width + column) and weights.
struct PanoTaps {
	uint32_t i00, i10, i01, i11;
	float w00, w10, w01, w11;
};
MRT_HD inline void panorama_taps(float u, float v, uint32_t width, uint32_t height, PanoTaps &t)
{
	u = u - __builtin_floorf(u);
	v = v < 1.0f ? v : 1.0f;
	v = v > 0.0f ? v : 0.0f;
	const float fx = u * (float)width - 0.5f, fy = v * (float)height - 0.5f;
	const float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy);
	const float sx = fx - flx, sy = fy - fly;
	int x0 = (int)flx, y0 = (int)fly; // in [-1, width - 1] and [-1, height - 1]
	const int w = (int)width, h = (int)height;
	const int x1 = pano_wrap_x(x0 + 1, w), y1 = pano_clamp_y(y0 + 1, h);
	x0 = pano_wrap_x(x0, w); y0 = pano_clamp_y(y0, h);
	t.i00 = (uint32_t)y0 * width + (uint32_t)x0; t.i10 = (uint32_t)y0 * width + (uint32_t)x1;
	t.i01 = (uint32_t)y1 * width + (uint32_t)x0; t.i11 = (uint32_t)y1 * width + (uint32_t)x1;
	const float inv_sx = 1.0f - sx, inv_sy = 1.0f - sy;
	t.w00 = inv_sx * inv_sy; t.w10 = sx * inv_sy; t.w01 = inv_sx * sy; t.w11 = sx * sy;
}

// one channel of the bilinear blend, in sample_panorama's order
MRT_HD inline float pano_blend(float p00, float p10, float p01, float p11, const PanoTaps &t)
{
	return ((p00 * t.w00 + p10 * t.w10) + p01 * t.w01) + p11 * t.w11;
}

// sample(dir) * energy of include/mrt_hip.h: texels = width * height * 4 floats; a non-finite direction reads nothing and gives zeros
MRT_HD inline void sky_panorama(const float *texels, uint32_t width, uint32_t height, float energy, float dx, float dy, float dz,
		float &r, float &g, float &b)
{
	r = g = b = 0.0f;
	if (!finite3(dx, dy, dz)) return;
	float u, v;
	equirect_uv(dx, dy, dz, u, v);
	PanoTaps t;
	panorama_taps(u, v, width, height, t);
	const float *p00 = texels + (uint64_t)t.i00 * 4u, *p10 = texels + (uint64_t)t.i10 * 4u;
	const float *p01 = texels + (uint64_t)t.i01 * 4u, *p11 = texels + (uint64_t)t.i11 * 4u;
	r = pano_blend(p00[0], p10[0], p01[0], p11[0], t) * energy;
	g = pano_blend(p00[1], p10[1], p01[1], p11[1], t) * energy;
	b = pano_blend(p00[2], p10[2], p01[2], p11[2], t) * energy;
}

// host/panorama_data.cpp (no device, no library)
// What mrt_upload_panorama refuses about its descriptor, in the order include/mrt_hip.h lists, or null.  Reads no texel.
const char *panorama_invalid(const mrt_panorama *pano);
// false: one of the first three floats of a texel is an infinity or a NaN (a host-resident image; alpha is not read)
bool panorama_texels_finite(const float *pixels, uint64_t n_texels);

} // namespace mrt
