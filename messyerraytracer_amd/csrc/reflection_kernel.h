// reflection_kernel.h — mirror-reflection rays made in the trace kernels (mrt_cast_reflections / mrt_cast_grid_reflections).
// Included by kernels.hip (inside namespace mrt, after source_common.h, before the kernels that use it).
//
// The reference's RTReflectionEffect (src/gpu/shaders/rt_reflections.comp.glsl:278-330): from each pixel's surface point and
// normal, reflect(view_dir, normal) from world_pos + normal * 0.01, traced closest-hit over [0, ray_max_distance].  A source family
// of source_common.h (SRC_REFLECT_*, closest-hit only); entry i is record i and its result is the record mrt_cast(MRT_MODE_NEAREST)
// writes for the ray.  Plain float operations in this order (nothing is contracted):
//   p   = position of the hit (host44: the record's; hit32: o + d * t of the incoming ray, the expression of store_hit)
//   n   = the record's normal; if ((nx*dx + ny*dy) + nz*dz) > 0 then n = -n      (faced against the incoming ray)
//   k   = 2 * ((nx*dx + ny*dy) + nz*dz)                                           (with the faced n)
//   dir = (dx - k*nx, dy - k*ny, dz - k*nz)                                       (GLSL reflect; not renormalised)
//   org = p + n * 0.01, t_min = 0, t_max = max_distance
// The flip changes nothing where the normal already faces the incoming ray (the reference's G-buffer normals face the camera); on
// a back face it keeps the origin in front of the surface.  dir does not depend on the sign of n (negation is exact).
// A primary miss or a record with select[i] == 0 gets no ray: it writes the record of the reference's placeholder
// Ray(0, (0,1,0), 0, 0) (t = 0 and a miss) and never walks the tree.
#pragma once

// The reflection ray of entry i (written to out_rays when asked for).  false: no ray -- r is the placeholder.
template <int SRC>
__device__ __forceinline__ bool reflection_ray(const TraceParams &p, const ReflectParams &s, uint64_t i, RayRegs &r)
{
	bool traced = s.select == nullptr || s.select[i] != 0;
	Surface sf = {};
	if (traced) traced = record_surface<SRC == SRC_REFLECT_HOST, SRC == SRC_REFLECT_GRID>(p, s.records, i, sf);
	if (traced) {
		const float k = 2.0f * face_normal(sf);
		r.dx = sf.dx - k * sf.nx; r.dy = sf.dy - k * sf.ny; r.dz = sf.dz - k * sf.nz;
		r.ox = sf.px + sf.nx * 0.01f; r.oy = sf.py + sf.ny * 0.01f; r.oz = sf.pz + sf.nz * 0.01f;
		r.t_min = 0.0f; r.t_max = s.max_distance;
	} else placeholder_ray(r);
	if (s.out_rays != nullptr) store_ray(s.out_rays, SRC == SRC_REFLECT_HOST, i, r);
	return traced;
}

// The reflection ray of entry i, or (false) the record of an entry without one, stored.
template <int SRC, bool ANY_HIT>
__device__ __forceinline__ bool source_entry(const TraceParams &p, const ReflectParams &s, uint64_t i, RayRegs &r)
{
	static_assert(reflection_source(SRC) && !ANY_HIT, "reflection sources are closest-hit");
	if (reflection_ray<SRC>(p, s, i, r)) return true;
	store_placeholder_record(p, i);
	return false;
}
