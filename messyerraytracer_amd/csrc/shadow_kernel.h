// shadow_kernel.h — shadow rays made in the trace kernels (mrt_cast_shadows / mrt_cast_grid_shadows).  Included by kernels.hip
// (inside namespace mrt, after source_common.h, before the kernels that use it).
//
// The second batch of the reference's frame (src/modules/graphics/ray_renderer.cpp:540-620, cpu_path_tracer.h:250-328): one
// any-hit ray per (pixel, light), built from the first batch's hit record.  A source family of source_common.h (SRC_SHADOW_*,
// any-hit only); entry g is the pair (light g / pixels, pixel g % pixels) and its result is one byte of the lit mask.  A pair without
// a ray is lit and never walks the tree.
#pragma once

// The shadow ray of record i to light L (the one text of it: selected_shadow_kernel.h makes its ray here too).  false: the pair is
// not traced (a primary miss, a light with cast_shadows == 0, or a point light on the ray's origin).  Plain float operations in the reference's order (nothing is contracted):
//   p   = position of the hit (hit44: the record's; hit32: o + d * t of the primary ray, the expression of store_hit)
//   org = p + n * 1e-3 (SHADOW_BIAS), t_min = 0
//   DIRECTIONAL: dir = the light's direction, t_max = 1000 (DIR_LIGHT_MAX_DIST)
//   POINT / SPOT: to = position - org, dist = sqrt((x*x + y*y) + z*z), dir = to / dist per component, t_max = dist
template <bool HOST, bool GRID>
__device__ __forceinline__ bool shadow_ray_to(const TraceParams &p, const void *records, uint64_t i, const ShadowLight &L, RayRegs &r)
{
	if (L.kind == SHADOW_OFF) return false;
	Surface sf;
	if (!record_surface<HOST, GRID, false>(p, records, i, sf)) return false;
	r.ox = sf.px + sf.nx * 1e-3f; r.oy = sf.py + sf.ny * 1e-3f; r.oz = sf.pz + sf.nz * 1e-3f;
	r.t_min = 0.0f;
	if (L.kind == SHADOW_DIRECTIONAL) {
		r.dx = L.v[0]; r.dy = L.v[1]; r.dz = L.v[2];
		r.t_max = 1000.0f;
		return true;
	}
	const float tx = L.v[0] - r.ox, ty = L.v[1] - r.oy, tz = L.v[2] - r.oz;
	const float dist = __builtin_sqrtf((tx * tx + ty * ty) + tz * tz);
	if (dist < 1e-6f) return false;
	r.dx = tx / dist; r.dy = ty / dist; r.dz = tz / dist;
	r.t_max = dist;
	return true;
}

// entry g = the pair (light g / pixels, pixel g % pixels)
template <int SRC>
__device__ __forceinline__ bool shadow_ray(const TraceParams &p, const ShadowParams &s, uint64_t g, RayRegs &r)
{
	uint64_t i;
	const uint64_t li = udivmod(g, s.pixels, i);
	const ShadowLight L = s.light[li];
	return shadow_ray_to<SRC == SRC_SHADOW_HOST44, SRC == SRC_SHADOW_GRID>(p, s.records, i, L, r);
}

// The shadow ray of entry g, or (false) the lit byte of a pair without one, stored.
template <int SRC, bool ANY_HIT>
__device__ __forceinline__ bool source_entry(const TraceParams &p, const ShadowParams &s, uint64_t g, RayRegs &r)
{
	static_assert(shadow_source(SRC) && ANY_HIT, "shadow sources are any-hit");
	if (shadow_ray<SRC>(p, s, g, r)) return true;
	store_lit(p, g, true);
	return false;
}
