// reflection_kernel.h — mirror-reflection rays made in the trace kernels (mrt_cast_reflections / mrt_cast_grid_reflections).
// Included by kernels.hip (inside namespace mrt, after shadow_kernel.h, before the kernels that use it).
//
// The reference's RTReflectionEffect (src/gpu/shaders/rt_reflections.comp.glsl:278-330): from each pixel's surface point and
// normal, reflect(view_dir, normal) from world_pos + normal * 0.01, traced closest-hit over [0, ray_max_distance].  The lane
// kernels, persistent or not, and the two-level kernels take the source as a template parameter (SRC_REFLECT_*); entry i is
// record i and its result is the record mrt_cast(MRT_MODE_NEAREST) writes for the ray.  Plain float operations in this order
// (nothing is contracted):
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

// the reference's placeholder ray for an entry without a ray
__device__ __forceinline__ void placeholder_ray(RayRegs &r)
{
	r.ox = 0.0f; r.oy = 0.0f; r.oz = 0.0f; r.dx = 0.0f; r.dy = 1.0f; r.dz = 0.0f; r.t_min = 0.0f; r.t_max = 0.0f;
}

// The ray of entry i in the input layout: mrt_ray32, or (host) mrt_host_ray60 as Ray(o, d, t_min, t_max) fills it
// (Ray::_precompute, src/core/ray.h:78-89; the oracle's orc_make_host_rays).
__device__ __forceinline__ void store_ray(void *out, bool host, uint64_t i, const RayRegs &r)
{
	if (host) {
		float *h = reinterpret_cast<float *>(out) + i * 15u;
		int32_t *hs = reinterpret_cast<int32_t *>(h);
		const float eps = 1e-9f;
		const float d[3] = { r.dx, r.dy, r.dz };
		h[0] = r.ox; h[1] = r.oy; h[2] = r.oz; h[3] = r.dx; h[4] = r.dy; h[5] = r.dz;
#pragma unroll
		for (int k = 0; k < 3; k++) {
			h[6 + k] = __builtin_fabsf(d[k]) < eps ? (d[k] < 0.0f ? -1.0f / eps : 1.0f / eps) : 1.0f / d[k];
			hs[9 + k] = d[k] < 0.0f ? 1 : 0;
		}
		h[12] = r.t_min; h[13] = r.t_max; hs[14] = 0;
		return;
	}
	float4 *q = reinterpret_cast<float4 *>(out) + i * 2u;
	float4 a, b;
	a.x = r.ox; a.y = r.oy; a.z = r.oz; a.w = r.t_max;
	b.x = r.dx; b.y = r.dy; b.z = r.dz; b.w = r.t_min;
	q[0] = a; q[1] = b;
}

// The reflection ray of entry i (written to out_rays when asked for).  false: no ray -- r is the placeholder.
template <int SRC>
__device__ __forceinline__ bool reflection_ray(const TraceParams &p, const ReflectParams &s, uint64_t i, RayRegs &r)
{
	bool traced = s.select == nullptr || s.select[i] != 0;
	float px = 0.0f, py = 0.0f, pz = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f, dx = 0.0f, dy = 0.0f, dz = 0.0f;
	if (traced) {
		if (SRC == SRC_REFLECT_HOST) {
			const float *h = reinterpret_cast<const float *>(s.records) + i * 11u;
			if (reinterpret_cast<const uint32_t *>(h)[9] == 0xFFFFFFFFu) traced = false;
			else {
				const float *v = reinterpret_cast<const float *>(p.rays) + i * 15u;
				px = h[1]; py = h[2]; pz = h[3];
				nx = h[4]; ny = h[5]; nz = h[6];
				dx = v[3]; dy = v[4]; dz = v[5];
			}
		} else {
			const float4 *q = reinterpret_cast<const float4 *>(s.records) + i * 2u;
			const float4 a = q[0];
			if (__float_as_int(a.y) == -1) traced = false;
			else {
				const float4 b = q[1];
				RayRegs o;
				if (SRC == SRC_REFLECT_GRID) { uint64_t gx; const uint64_t gy = udivmod(i, p.grid_w, gx); grid_ray(p, (uint32_t)gx, (uint32_t)gy, o); }
				else {
					const float4 *v = reinterpret_cast<const float4 *>(p.rays) + i * 2u;
					const float4 c = v[0], d = v[1];
					o.ox = c.x; o.oy = c.y; o.oz = c.z; o.dx = d.x; o.dy = d.y; o.dz = d.z;
				}
				px = o.ox + o.dx * a.x; py = o.oy + o.dy * a.x; pz = o.oz + o.dz * a.x;
				nx = b.x; ny = b.y; nz = b.z;
				dx = o.dx; dy = o.dy; dz = o.dz;
			}
		}
	}
	if (traced) {
		float c = (nx * dx + ny * dy) + nz * dz;
		if (c > 0.0f) { nx = -nx; ny = -ny; nz = -nz; c = -c; } // (the faced n's dot product: the same sum negated, exactly)
		const float k = 2.0f * c;
		r.dx = dx - k * nx; r.dy = dy - k * ny; r.dz = dz - k * nz;
		r.ox = px + nx * 0.01f; r.oy = py + ny * 0.01f; r.oz = pz + nz * 0.01f;
		r.t_min = 0.0f; r.t_max = s.max_distance;
	} else placeholder_ray(r);
	if (s.out_rays != nullptr) store_ray(s.out_rays, SRC == SRC_REFLECT_HOST, i, r);
	return traced;
}

// The record of an entry without a ray: what mrt_cast writes for the placeholder (t_min >= t_max: a miss at t = t_max = 0).
__device__ __forceinline__ void store_no_reflection(const TraceParams &p, uint64_t i)
{
	RayRegs r;
	placeholder_ray(r);
	store_hit(p, i, r, r.t_max, -1, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u, 0xFFFFFFFFu);
}
