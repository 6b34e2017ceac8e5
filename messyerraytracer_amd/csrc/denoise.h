// denoise.h -- the reflection effect's three image passes (mrt_denoise_spatial, mrt_denoise_temporal, mrt_composite_reflections,
// mrt_resolve_reflections) and mrt_reflection_guides: expn_def and every per-pixel rule as include/mrt_hip.h states them, one
// definition for the kernels (denoise_kernel.h) and the host, so that both hold the same bits; the kernel's argument block; and the
// checks of the calls (host/denoise_data.cpp).  Host-only code may include this without HIP.  pow01 is lighting.h's, unchanged.
#pragma once
#include "lighting.h"

static_assert(sizeof(mrt_denoise_params) == 112, "mrt_denoise_params must be 112 bytes");

namespace mrt {
namespace dn {

struct alignas(16) Px4 { float x, y, z, w; };
// one texel as the spatial pass uses it: the reflection's four floats, the depth and the decoded normal
struct Texel { Px4 c; float d, nx, ny, nz; };

// What the kernels read (uniform: a kernel argument).  radius is already clamped; m = the 3x3 of inv_view, m[3 c + r] = column c, row r.
struct DenoiseArgs {
	uint32_t w, h;
	int32_t radius;
	uint32_t normal_kind, has_history;
	float depth_sigma, normal_sigma, color_sigma;
	float blend, depth_threshold, roughness_threshold, intensity, f0;
	float m[9];
	float w_spatial[81]; // [(dy + radius) * (2 radius + 1) + (dx + radius)]
};

// exp(y) for y <= 0 (include/mrt_hip.h): the second half of pow01, fp64, one operation at a time, nothing contracted.
MRT_HD inline float expn_def(float yf)
{
	if (yf != yf) return yf; // a NaN as it stands (the integer conversion below is not defined for it)
	const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10, INV_LN2 = 1.44269504088896338700e+00;
	const double RND = 6755399441055744.0;
	const double y = (double)yf;
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

// std::max / std::min / their composition: a NaN first argument is kept
MRT_HD inline float max_of(float a, float b) { return a < b ? b : a; }
MRT_HD inline float min_of(float a, float b) { return b < a ? b : a; }
MRT_HD inline float clamp_of(float x, float lo, float hi) { return min_of(max_of(x, lo), hi); }
MRT_HD inline int clamp_radius(int32_t r) { return r < 1 ? 1 : (r > 4 ? 4 : r); }

// GLSL normalize as the header states it: one square root, three divisions
MRT_HD inline void normalize3(float &x, float &y, float &z)
{
	const float len = __builtin_sqrtf((x * x + y * y) + z * z);
	x = x / len; y = y / len; z = z / len;
}

// the normal and the roughness of a {x, y, z, w} guide texel
MRT_HD inline void decode_guide(uint32_t kind, const Px4 &g, float &nx, float &ny, float &nz, float &roughness)
{
	if (kind == (uint32_t)MRT_NORMAL_WORLD) { nx = g.x; ny = g.y; nz = g.z; roughness = g.w; return; }
	const float fx = g.x * 2.0f - 1.0f, fy = g.y * 2.0f - 1.0f;
	const float z = (1.0f - __builtin_fabsf(fx)) - __builtin_fabsf(fy);
	const float t = clamp_of(-z, 0.0f, 1.0f);
	nx = fx + (fx >= 0.0f ? -t : t);
	ny = fy + (fy >= 0.0f ? -t : t);
	nz = z;
	normalize3(nx, ny, nz);
	roughness = g.z;
}

// texel (x, y) of the three images, clamped to the edge
struct GlobalFetch {
	const Px4 *reflection; const float *depth; const Px4 *guide;
	uint32_t w, h, kind;
	int64_t x, y; // the centre
	MRT_HD Texel operator()(int dx, int dy) const
	{
		int64_t tx = x + dx, ty = y + dy;
		tx = tx < 0 ? 0 : (tx > (int64_t)w - 1 ? (int64_t)w - 1 : tx);
		ty = ty < 0 ? 0 : (ty > (int64_t)h - 1 ? (int64_t)h - 1 : ty);
		const uint64_t i = (uint64_t)ty * w + (uint64_t)tx;
		Texel t;
		float rough;
		t.c = reflection[i]; t.d = depth[i];
		decode_guide(kind, guide[i], t.nx, t.ny, t.nz, rough);
		return t;
	}
};

// one tap's weight: depth, normal, colour, distance
MRT_HD inline float tap_weight(const DenoiseArgs &a, const Texel &c, const Texel &s, float w_spatial)
{
	const float dd = __builtin_fabsf(c.d - s.d);
	const float w_depth = expn_def(-((dd * dd) * a.depth_sigma));
	const float dot = (c.nx * s.nx + c.ny * s.ny) + c.nz * s.nz;
	const float w_normal = pow01(max_of(dot, 0.0f), a.normal_sigma);
	const float dr = c.c.x - s.c.x, dg = c.c.y - s.c.y, db = c.c.z - s.c.z;
	const float w_color = expn_def(-(((dr * dr + dg * dg) + db * db) * a.color_sigma));
	return ((w_depth * w_normal) * w_color) * w_spatial;
}

// the spatial pass of one pixel; fetch(dx, dy) = the tap's texel, (0, 0) the centre; wsp = a.w_spatial, or a copy of it
template <class Fetch>
MRT_HD inline Px4 spatial_pixel(const DenoiseArgs &a, const float *wsp, const Fetch &fetch)
{
	const Texel c = fetch(0, 0);
	if (c.c.w <= 0.0f || c.d >= 1.0f) return Px4{0.0f, 0.0f, 0.0f, 0.0f};
	const int r = a.radius;
	float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f, ws = 0.0f;
	for (int dy = -r; dy <= r; dy++)
		for (int dx = -r; dx <= r; dx++, wsp++) {
			const Texel s = fetch(dx, dy);
			if (s.c.w <= 0.0f) continue;
			const float w = tap_weight(a, c, s, *wsp);
			sx = sx + s.c.x * w; sy = sy + s.c.y * w; sz = sz + s.c.z * w; sw = sw + s.c.w * w;
			ws = ws + w;
		}
	if (ws > 0.001f) return Px4{sx / ws, sy / ws, sz / ws, sw / ws};
	return c.c;
}

// the temporal pass of one pixel; hist is not looked at without history
MRT_HD inline Px4 temporal_pixel(const DenoiseArgs &a, const Px4 &cur, const Px4 &hist)
{
	if (!a.has_history) return cur;
	if (cur.w <= 0.0f) return Px4{hist.x * 0.9f, hist.y * 0.9f, hist.z * 0.9f, hist.w * 0.9f};
	if (hist.w <= 0.0f) return cur;
	const float dd = __builtin_fabsf(cur.w - hist.w);
	const float rej = dd < a.depth_threshold ? 0.0f : 1.0f;
	const float alpha = a.blend * (1.0f - rej) + rej;
	const float om = 1.0f - alpha;
	return Px4{hist.x * om + cur.x * alpha, hist.y * om + cur.y * alpha, hist.z * om + cur.z * alpha, hist.w * om + cur.w * alpha};
}

// the composite of pixel (x, y): false = the colour stays as it is
MRT_HD inline bool composite_pixel(const DenoiseArgs &a, uint32_t x, uint32_t y, const Px4 &refl, float depth, const Px4 &guide, Px4 &color)
{
	if (refl.w <= 0.001f || depth >= 1.0f) return false;
	float nx, ny, nz, rough;
	decode_guide(a.normal_kind, guide, nx, ny, nz, rough);
	const float u = ((float)x + 0.5f) / (float)a.w, v = ((float)y + 0.5f) / (float)a.h;
	float vx = u * 2.0f - 1.0f, vy = v * 2.0f - 1.0f, vz = -1.0f;
	normalize3(vx, vy, vz);
	float wx = (a.m[0] * vx + a.m[3] * vy) + a.m[6] * vz;
	float wy = (a.m[1] * vx + a.m[4] * vy) + a.m[7] * vz;
	float wz = (a.m[2] * vx + a.m[5] * vy) + a.m[8] * vz;
	normalize3(wx, wy, wz);
	const float n_dot_v = max_of((nx * -wx + ny * -wy) + nz * -wz, 0.001f);
	const float s = clamp_of(1.0f - n_dot_v, 0.0f, 1.0f), s2 = s * s, s4 = s2 * s2, s5 = s4 * s;
	const float fresnel = a.f0 + (1.0f - a.f0) * s5;
	const float t = clamp_of(rough / a.roughness_threshold, 0.0f, 1.0f);
	const float rw = 1.0f - (t * t) * (3.0f - 2.0f * t);
	const float blend = clamp_of(((fresnel * rw) * refl.w) * a.intensity, 0.0f, 1.0f);
	const float om = 1.0f - blend;
	color.x = color.x * om + refl.x * blend;
	color.y = color.y * om + refl.y * blend;
	color.z = color.z * om + refl.z * blend;
	return true;
}

// the two guide texels of a primary record and its surface row (mrt_reflection_guides)
MRT_HD inline void guide_texels(const mrt_hit32 &hit, const mrt_surface64 &row, float inv_depth_range, float &depth, Px4 &guide)
{
	depth = 1.0f;
	if (hit.prim_id != -1) depth = min_of(hit.t * inv_depth_range, 1.0f);
	guide = Px4{row.normal[0], row.normal[1], row.normal[2], row.roughness};
}

// w_spatial of one tap, and the table of a radius (at most 81 floats, dy outer, dx inner, both ascending)
inline float spatial_weight(int dx, int dy, int radius)
{
	return expn_def(-((float)(dx * dx + dy * dy) / (2.0f * (float)(radius * radius) + 0.001f)));
}
inline void spatial_table(int radius, float *out)
{
	for (int dy = -radius; dy <= radius; dy++)
		for (int dx = -radius; dx <= radius; dx++) *out++ = spatial_weight(dx, dy, radius);
}

// host/denoise_data.cpp (no device, no library)
enum DenoiseCall { DN_SPATIAL = 0, DN_TEMPORAL = 1, DN_COMPOSITE = 2, DN_RESOLVE = 3 };
// What a call refuses before any device work, or null, in the order include/mrt_hip.h lists.  The images in the call's own argument
// order; unused ones are not looked at.
const char *denoise_invalid(int call, const mrt_denoise_params *params, uint32_t w, uint32_t h, const void *d_reflection, const void *d_depth,
		const void *d_guide, const void *d_history, const void *d_color, const void *d_out, uint32_t flags);
const char *guides_invalid(const void *d_hits, const void *d_rows, uint64_t count, float inv_depth_range, const void *d_depth,
		const void *d_guide, uint32_t flags);
// The kernel's arguments from the caller's: the clamped radius, the 3x3 and the table.
void fill_denoise_args(const mrt_denoise_params *params, uint32_t w, uint32_t h, DenoiseArgs &a);

} // namespace dn
} // namespace mrt
