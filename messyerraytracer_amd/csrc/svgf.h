// svgf.h -- the SVGF pass chain of a path-traced frame (mrt_svgf_guides, mrt_svgf_temporal, mrt_svgf_variance, mrt_svgf_atrous,
// mrt_svgf_modulate, mrt_svgf_frame): every per-pixel rule as include/mrt_hip.h states it, one definition for the kernels
// (svgf_kernel.h) and the host, so that both hold the same bits; the kernels' argument block; and the checks of the calls
// (host/svgf_data.cpp).  Host-only code may include this without HIP.  expn_def, max_of and min_of are denoise.h's, pow01 lighting.h's,
// tonemap and path_gamma path.h's, all unchanged.
#pragma once
#include "denoise.h"
#include "channels.h"

static_assert(sizeof(mrt_svgf_params) == 48, "mrt_svgf_params must be 48 bytes");

namespace mrt {
namespace sv {

using dn::Px4;
using dn::expn_def;
using dn::max_of;
using dn::min_of;

// What the kernels read (uniform: a kernel argument).  The camera is the previous frame's; only the temporal pass looks at it.
struct SvgfArgs {
	uint32_t w, h;
	uint32_t has_history, mode;
	int32_t step;
	float white;
	float color_alpha, moments_alpha, max_history, normal_threshold, position_threshold, sigma_l, sigma_n, sigma_plane;
	float origin[3], right[3], up[3], fwd[3];
	float half_w, half_h, jitter_x, jitter_y;
};

// the images a pass reads across pixels; those a pass does not use stay null
struct Images {
	const Px4 *illum, *moments, *normal_depth, *position;
	uint32_t w, h;
	MRT_HD bool inside(int64_t x, int64_t y) const { return x >= 0 && y >= 0 && x < (int64_t)w && y < (int64_t)h; }
	MRT_HD uint64_t at(int64_t x, int64_t y) const { return (uint64_t)y * w + (uint64_t)x; }
};

MRT_HD inline float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
MRT_HD inline float lum(const Px4 &c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
// the 1-D B3 kernel {1/16, 1/4, 3/8, 1/4, 1/16} at offset k = -2 .. 2, by selects: no table is indexed
MRT_HD inline float b3(int k) { return k == 0 ? 0.375f : ((k == 1 || k == -1) ? 0.25f : 0.0625f); }

// pass 1: one record
MRT_HD inline void guides_pixel(const mrt_ray32 &ray, const mrt_hit32 &hit, const mrt_surface64 &row, const Px4 &radiance, Px4 &illum,
		Px4 &albedo, Px4 &normal_depth, Px4 &position)
{
	if (hit.prim_id == -1) {
		illum = Px4{radiance.x, radiance.y, radiance.z, 0.0f};
		albedo = Px4{1.0f, 1.0f, 1.0f, 1.0f};
		normal_depth = Px4{0.0f, 0.0f, 0.0f, 0.0f};
		position = Px4{0.0f, 0.0f, 0.0f, 0.0f};
		return;
	}
	const float ar = max_of(row.albedo[0], 0.001f), ag = max_of(row.albedo[1], 0.001f), ab = max_of(row.albedo[2], 0.001f);
	illum = Px4{radiance.x / ar, radiance.y / ag, radiance.z / ab, 0.0f};
	albedo = Px4{ar, ag, ab, 1.0f};
	normal_depth = Px4{row.normal[0], row.normal[1], row.normal[2], hit.t};
	position = Px4{ray.origin[0] + ray.direction[0] * hit.t, ray.origin[1] + ray.direction[1] * hit.t, ray.origin[2] + ray.direction[2] * hit.t, 0.0f};
}

// pass 2: the history of one pixel gathered from the previous frame; false = none
MRT_HD inline bool gather_history(const SvgfArgs &a, const Images &prev, const Px4 &nd, const Px4 &p, float &hr, float &hg, float &hb,
		float &hm1, float &hm2, float &n_prev)
{
	const float ex = p.x - a.origin[0], ey = p.y - a.origin[1], ez = p.z - a.origin[2];
	const float cx = dot3(ex, ey, ez, a.right[0], a.right[1], a.right[2]);
	const float cy = dot3(ex, ey, ez, a.up[0], a.up[1], a.up[2]);
	const float cz = dot3(ex, ey, ez, a.fwd[0], a.fwd[1], a.fwd[2]);
	if (!(cz < 0.0f)) return false;
	const float w = -cz;
	const float u = (cx / w) / a.half_w, v = (cy / w) / a.half_h;
	const float fw = (float)a.w, fh = (float)a.h;
	const float fx = ((u + 1.0f) * 0.5f) * fw - a.jitter_x;
	const float fy = ((1.0f - v) * 0.5f) * fh - a.jitter_y;
	if (!(fx >= -1.0f && fx < fw && fy >= -1.0f && fy < fh)) return false;
	const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
	const float ax = fx - x0f, ay = fy - y0f;
	const float bx = 1.0f - ax, by = 1.0f - ay;
	const int64_t x0 = (int64_t)x0f, y0 = (int64_t)y0f;
	const float bound = a.position_threshold * nd.w, bound2 = bound * bound;
	float sr = 0.0f, sg = 0.0f, sb = 0.0f, s1 = 0.0f, s2 = 0.0f, ws = 0.0f;
	bool counted = false;
	n_prev = 0.0f;
	for (int k = 0; k < 4; k++) {
		const int i = k & 1, j = k >> 1;
		const int64_t tx = x0 + i, ty = y0 + j;
		if (!prev.inside(tx, ty)) continue;
		const uint64_t at = prev.at(tx, ty);
		const Px4 pn = prev.normal_depth[at];
		if (!(pn.w > 0.0f)) continue;
		if (!(dot3(nd.x, nd.y, nd.z, pn.x, pn.y, pn.z) >= a.normal_threshold)) continue;
		const Px4 pp = prev.position[at];
		const float dx = p.x - pp.x, dy = p.y - pp.y, dz = p.z - pp.z;
		if (!(dot3(dx, dy, dz, dx, dy, dz) <= bound2)) continue;
		const float wt = (i ? ax : bx) * (j ? ay : by);
		const Px4 pi = prev.illum[at], pm = prev.moments[at];
		sr = sr + pi.x * wt; sg = sg + pi.y * wt; sb = sb + pi.z * wt;
		s1 = s1 + pm.x * wt; s2 = s2 + pm.y * wt;
		ws = ws + wt;
		n_prev = counted ? min_of(n_prev, pm.z) : pm.z;
		counted = true;
	}
	if (!(ws > 0.01f)) return false;
	hr = sr / ws; hg = sg / ws; hb = sb / ws; hm1 = s1 / ws; hm2 = s2 / ws;
	return true;
}

// pass 2: one pixel; prev is not looked at without a.has_history
MRT_HD inline void temporal_pixel(const SvgfArgs &a, const Images &prev, const Px4 &cur, const Px4 &nd, const Px4 &p, Px4 &out, Px4 &moments)
{
	if (nd.w <= 0.0f) {
		out = Px4{cur.x, cur.y, cur.z, 0.0f};
		moments = Px4{0.0f, 0.0f, 0.0f, 0.0f};
		return;
	}
	const float l = lum(cur);
	float hr, hg, hb, hm1, hm2, n_prev;
	if (a.has_history && gather_history(a, prev, nd, p, hr, hg, hb, hm1, hm2, n_prev)) {
		const float n = min_of(n_prev + 1.0f, a.max_history);
		const float inv = 1.0f / n;
		const float alpha = max_of(a.color_alpha, inv), alpha_m = max_of(a.moments_alpha, inv);
		const float om = 1.0f - alpha, omm = 1.0f - alpha_m;
		const float m1 = hm1 * omm + l * alpha_m, m2 = hm2 * omm + (l * l) * alpha_m;
		out = Px4{hr * om + cur.x * alpha, hg * om + cur.y * alpha, hb * om + cur.z * alpha, max_of(m2 - m1 * m1, 0.0f)};
		moments = Px4{m1, m2, n, 0.0f};
		return;
	}
	out = Px4{cur.x, cur.y, cur.z, 0.0f};
	moments = Px4{l, l * l, 1.0f, 0.0f};
}

// the plane and normal factors the two spatial passes share: ez = |n_c . (p_s - p_c)| / (sigma_plane * t_c)
MRT_HD inline float plane_term(const SvgfArgs &a, const Px4 &cn, const Px4 &cp, const Px4 &sp)
{
	const float dx = sp.x - cp.x, dy = sp.y - cp.y, dz = sp.z - cp.z;
	return __builtin_fabsf(dot3(cn.x, cn.y, cn.z, dx, dy, dz)) / (a.sigma_plane * cn.w);
}

// pass 3: pixel (x, y)
MRT_HD inline Px4 variance_pixel(const SvgfArgs &a, const Images &im, int64_t x, int64_t y)
{
	const uint64_t c = im.at(x, y);
	const Px4 ci = im.illum[c], cm = im.moments[c], cn = im.normal_depth[c];
	if (cn.w <= 0.0f || cm.z >= 4.0f) return ci;
	const Px4 cp = im.position[c];
	float s1 = 0.0f, s2 = 0.0f, ws = 0.0f;
	for (int dy = -3; dy <= 3; dy++)
		for (int dx = -3; dx <= 3; dx++) {
			float wt = 1.0f;
			Px4 sm = cm;
			if (dx != 0 || dy != 0) {
				const int64_t tx = x + dx, ty = y + dy;
				if (!im.inside(tx, ty)) continue;
				const uint64_t s = im.at(tx, ty);
				const Px4 sn = im.normal_depth[s];
				if (sn.w <= 0.0f) continue;
				const float dotn = dot3(cn.x, cn.y, cn.z, sn.x, sn.y, sn.z);
				if (dotn <= 0.0f) continue;
				wt = expn_def(-plane_term(a, cn, cp, im.position[s])) * pow01(dotn, a.sigma_n);
				sm = im.moments[s];
			}
			s1 = s1 + sm.x * wt; s2 = s2 + sm.y * wt;
			ws = ws + wt;
		}
	const float m1 = s1 / ws, m2 = s2 / ws;
	return Px4{ci.x, ci.y, ci.z, max_of(m2 - m1 * m1, 0.0f) * (4.0f / cm.z)};
}

// pass 4: pixel (x, y), one iteration at a.step
MRT_HD inline Px4 atrous_pixel(const SvgfArgs &a, const Images &im, int64_t x, int64_t y)
{
	const uint64_t c = im.at(x, y);
	const Px4 ci = im.illum[c], cn = im.normal_depth[c];
	if (cn.w <= 0.0f) return ci;
	const Px4 cp = im.position[c];
	float sv = 0.0f, sg = 0.0f;
	for (int dy = -1; dy <= 1; dy++)
		for (int dx = -1; dx <= 1; dx++) {
			const int64_t tx = x + dx, ty = y + dy;
			if (!im.inside(tx, ty)) continue;
			const float g = (dx == 0 && dy == 0) ? 0.25f : ((dx == 0 || dy == 0) ? 0.125f : 0.0625f);
			sv = sv + im.illum[im.at(tx, ty)].w * g;
			sg = sg + g;
		}
	const float var_c = sv / sg;
	const float denom = a.sigma_l * __builtin_sqrtf(var_c) + 1e-4f;
	const float lc = lum(ci);
	float sr = 0.0f, sgr = 0.0f, sb = 0.0f, svar = 0.0f, ws = 0.0f;
	for (int j = -2; j <= 2; j++)
		for (int i = -2; i <= 2; i++) {
			float wt = b3(0) * b3(0);
			Px4 si = ci;
			if (i != 0 || j != 0) {
				const int64_t tx = x + (int64_t)i * a.step, ty = y + (int64_t)j * a.step;
				if (!im.inside(tx, ty)) continue;
				const uint64_t s = im.at(tx, ty);
				const Px4 sn = im.normal_depth[s];
				if (sn.w <= 0.0f) continue;
				const float dotn = dot3(cn.x, cn.y, cn.z, sn.x, sn.y, sn.z);
				if (dotn <= 0.0f) continue;
				si = im.illum[s];
				const float ez = plane_term(a, cn, cp, im.position[s]);
				const float el = __builtin_fabsf(lc - lum(si)) / denom;
				wt = ((b3(i) * b3(j)) * expn_def(-(ez + el))) * pow01(dotn, a.sigma_n);
			}
			sr = sr + si.x * wt; sgr = sgr + si.y * wt; sb = sb + si.z * wt;
			svar = svar + si.w * (wt * wt);
			ws = ws + wt;
		}
	return Px4{sr / ws, sgr / ws, sb / ws, svar / (ws * ws)};
}

// pass 5: one pixel
MRT_HD inline Px4 modulate_pixel(const SvgfArgs &a, const Px4 &illum, const Px4 &albedo)
{
	return Px4{path_gamma(tonemap(illum.x * albedo.x, a.mode, a.white)), path_gamma(tonemap(illum.y * albedo.y, a.mode, a.white)),
			path_gamma(tonemap(illum.z * albedo.z, a.mode, a.white)), 1.0f};
}

// host/svgf_data.cpp (no device, no library)
enum SvgfCall { SV_TEMPORAL = 0, SV_VARIANCE = 1, SV_ATROUS = 2, SV_MODULATE = 3, SV_FRAME = 4 };
// every image of the five calls that take mrt_svgf_params, in the order the calls list them; a call leaves what it does not take null
struct SvgfImages {
	const void *illum, *albedo, *moments, *normal_depth, *position;                    // this frame's
	const void *prev_illum, *prev_moments, *prev_normal_depth, *prev_position;          // the previous frame's
	const void *out_illum, *out_moments, *scratch_a, *scratch_b, *rgba;                 // written (out_illum: d_out of the one-output calls)
};
// What a call refuses before any device work, or null, in the order include/mrt_hip.h lists.
const char *svgf_invalid(int call, const mrt_svgf_params *params, uint32_t w, uint32_t h, uint32_t step, const mrt_camera *prev_cam,
		const SvgfImages &im, uint32_t flags);
const char *svgf_guides_invalid(const void *d_rays, const void *d_hits, const void *d_rows, uint32_t source_kind, const void *d_source,
		uint64_t count, const void *d_illum, const void *d_albedo, const void *d_normal_depth, const void *d_position, uint32_t flags);
// The kernels' arguments from the caller's; prev_cam may be null (has_history == 0), white = hp(11.2f).
void fill_svgf_args(const mrt_svgf_params *params, uint32_t w, uint32_t h, uint32_t step, const mrt_camera *prev_cam, float white, SvgfArgs &a);

} // namespace sv
} // namespace mrt
