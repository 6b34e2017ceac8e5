// gbuffer.h -- the reflection effect's first pass from a rasteriser's G-buffer (mrt_cast_gbuffer_reflections, mrt_reflection_image;
// src/gpu/shaders/rt_reflections.comp.glsl:276-332): the reflection ray of a pixel from its depth and its normal-roughness texel, and
// the pixel of the reflection image from the ray's record, as include/mrt_hip.h states them, one definition for the kernels
// (gbuffer_kernel.h in the walks, gbuffer_image_kernel.h) and the host, so that both hold the same bits; and the checks of the two
// calls (host/gbuffer_data.cpp).  Host-only code may include this without HIP.  decode_guide, normalize3 and max_of are denoise.h's,
// unchanged.  Plain fp32: every multiply, add, divide and square root is rounded on its own in the order written.
#pragma once
#include "denoise.h"
#include "mrt_internal.h"

static_assert(sizeof(mrt_gbuffer) == 160, "mrt_gbuffer must be 160 bytes");

namespace mrt {
namespace gb {

using dn::Px4;

// x is neither an infinity nor a NaN
MRT_HD inline bool finite(float x) { return x - x == 0.0f; }

// A pixel's surface as the shader reconstructs it: the world position, the normalised view direction d (camera to surface), the
// decoded normal and the roughness.
struct Surface { float wx, wy, wz, dx, dy, dz, nx, ny, nz, roughness; };

// World position and view direction of pixel (x, y) of a w x h frame at `depth`; P = inv_projection, V = inv_view, both column-major
// (M[c][r] = m[4 c + r]).  Row 3 of V is not read.
MRT_HD inline void view_surface(const float *P, const float *V, uint32_t x, uint32_t y, uint32_t w, uint32_t h, float depth, Surface &s)
{
	const float u = ((float)x + 0.5f) / (float)w, v = ((float)y + 0.5f) / (float)h;
	const float cx = u * 2.0f - 1.0f, cy = v * 2.0f - 1.0f;
	const float q0 = ((P[0] * cx + P[4] * cy) + P[8] * depth) + P[12];
	const float q1 = ((P[1] * cx + P[5] * cy) + P[9] * depth) + P[13];
	const float q2 = ((P[2] * cx + P[6] * cy) + P[10] * depth) + P[14];
	const float q3 = ((P[3] * cx + P[7] * cy) + P[11] * depth) + P[15];
	const float vx = q0 / q3, vy = q1 / q3, vz = q2 / q3;
	s.wx = ((V[0] * vx + V[4] * vy) + V[8] * vz) + V[12];
	s.wy = ((V[1] * vx + V[5] * vy) + V[9] * vz) + V[13];
	s.wz = ((V[2] * vx + V[6] * vy) + V[10] * vz) + V[14];
	s.dx = s.wx - V[12]; s.dy = s.wy - V[13]; s.dz = s.wz - V[14];
	dn::normalize3(s.dx, s.dy, s.dz);
}

// Pixel (x, y): its surface from the depth and the guide texel.
MRT_HD inline void pixel_surface(uint32_t kind, const float *P, const float *V, uint32_t x, uint32_t y, uint32_t w, uint32_t h, float depth,
		const Px4 &g, Surface &s)
{
	dn::decode_guide(kind, g, s.nx, s.ny, s.nz, s.roughness);
	view_surface(P, V, x, y, w, h, depth, s);
}

// The sky test: no ray unless depth < 1 (the shader's depth >= 1, and a NaN depth)
MRT_HD inline bool sky(float depth) { return !(depth < 1.0f); }

// The reflection ray of pixel (x, y): org and dir (t_min = 0 and t_max = max_distance are the caller's).  false: no ray -- sky, too
// rough, or an origin or direction that is not finite (org and dir are then not to be used).  The normal is NOT turned towards the viewer.
MRT_HD inline bool reflection_ray(uint32_t kind, const float *P, const float *V, float roughness_threshold, uint32_t x, uint32_t y, uint32_t w,
		uint32_t h, float depth, const Px4 &g, float org[3], float dir[3])
{
	if (sky(depth)) return false;
	Surface s;
	pixel_surface(kind, P, V, x, y, w, h, depth, g, s);
	if (!(s.roughness <= roughness_threshold)) return false;
	const float k = 2.0f * ((s.nx * s.dx + s.ny * s.dy) + s.nz * s.dz);
	dir[0] = s.dx - k * s.nx; dir[1] = s.dy - k * s.ny; dir[2] = s.dz - k * s.nz;
	org[0] = s.wx + s.nx * 0.01f; org[1] = s.wy + s.ny * 0.01f; org[2] = s.wz + s.nz * 0.01f;
	return finite(org[0]) && finite(org[1]) && finite(org[2]) && finite(dir[0]) && finite(dir[1]) && finite(dir[2]);
}

// The reflection image's pixel (x, y) from the ray's record (prim_id, its normal hn) -- a miss, which every entry without a ray is:
// {0, 0, 0, 0} (depth and g are not looked at); has_lit: lit is the lit colour of the record, else the shader's grey.
MRT_HD inline Px4 image_pixel(uint32_t kind, const float *P, const float *V, float roughness_threshold, uint32_t x, uint32_t y, uint32_t w,
		uint32_t h, float depth, const Px4 &g, int32_t prim_id, float hnx, float hny, float hnz, bool has_lit, const Px4 &lit)
{
	if (prim_id == -1) return Px4{0.0f, 0.0f, 0.0f, 0.0f};
	Surface s;
	pixel_surface(kind, P, V, x, y, w, h, depth, g, s);
	const float conf = 1.0f - s.roughness / roughness_threshold;
	if (has_lit) return Px4{lit.x, lit.y, lit.z, conf};
	const float ndotl = dn::max_of((hnx * -s.dx + hny * -s.dy) + hnz * -s.dz, 0.0f);
	const float grey = 0.5f + 0.5f * ndotl;
	return Px4{grey, grey, grey, conf};
}

// The kernels' argument from the caller's descriptor (out_rays: the cast's, optional).
inline void fill_params(const mrt_gbuffer *g, uint32_t w, uint32_t h, void *out_rays, GBufferParams &s)
{
	s.depth = g->d_depth; s.guide = g->d_normal_roughness; s.out_rays = out_rays;
	s.w = w; s.h = h; s.normal_kind = g->normal_kind;
	s.roughness_threshold = g->roughness_threshold; s.max_distance = g->max_distance;
	for (int k = 0; k < 16; k++) { s.inv_projection[k] = g->inv_projection[k]; s.inv_view[k] = g->inv_view[k]; }
}

// host/gbuffer_data.cpp (no device, no library): what the two calls refuse before any device work, or null, in the order
// include/mrt_hip.h lists (the cast's flags are checked before, as every record-driven cast's: source_cast.h unknown_flag).
const char *cast_invalid(const mrt_gbuffer *g, uint32_t w, uint32_t h, const void *d_out_hits);
const char *image_invalid(const mrt_gbuffer *g, uint32_t w, uint32_t h, const void *d_hits, const void *d_reflection, uint32_t flags);

} // namespace gb
} // namespace mrt
