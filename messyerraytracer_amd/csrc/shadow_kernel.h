// shadow_kernel.h — shadow rays made in the trace kernels (mrt_cast_shadows / mrt_cast_grid_shadows).  Included by kernels.hip
// (inside namespace mrt, after the ray and record helpers, before the kernels that use it).
//
// The second batch of the reference's frame (src/modules/graphics/ray_renderer.cpp:540-620, cpu_path_tracer.h:250-328): one
// any-hit ray per (pixel, light), built from the first batch's hit record.  The lane kernels, persistent or not, and the
// two-level kernels take the source as a template parameter (SRC_SHADOW_*); entry g is the pair (light g / pixels, pixel
// g % pixels) and its result is one byte of the lit mask.  A pair without a ray is lit and never walks the tree.
#pragma once

// q = a / b, r = a % b: in 32 bits when both fit (a 64-bit division is a long software sequence on gfx950; every batch of fewer
// than 2^32 pairs takes the short one).
__device__ __forceinline__ uint64_t udivmod(uint64_t a, uint64_t b, uint64_t &r)
{
	if (((a | b) >> 32) == 0u) {
		const uint32_t q = (uint32_t)a / (uint32_t)b;
		r = (uint32_t)a - q * (uint32_t)b;
		return q;
	}
	const uint64_t q = a / b;
	r = a - q * b;
	return q;
}

// The shadow ray of entry g.  false: the pair is not traced (a primary miss, a light with cast_shadows == 0, or a point
// light on the ray's origin).  Plain float operations in the reference's order (nothing is contracted):
//   p   = position of the hit (hit44: the record's; hit32: o + d * t of the primary ray, the expression of store_hit)
//   org = p + n * 1e-3 (SHADOW_BIAS), t_min = 0
//   DIRECTIONAL: dir = the light's direction, t_max = 1000 (DIR_LIGHT_MAX_DIST)
//   POINT / SPOT: to = position - org, dist = sqrt((x*x + y*y) + z*z), dir = to / dist per component, t_max = dist
template <int SRC>
__device__ __forceinline__ bool shadow_ray(const TraceParams &p, const ShadowParams &s, uint64_t g, RayRegs &r)
{
	uint64_t i;
	const uint64_t li = udivmod(g, s.pixels, i);
	const ShadowLight L = s.light[li];
	if (L.kind == SHADOW_OFF) return false;
	float px, py, pz, nx, ny, nz;
	if (SRC == SRC_SHADOW_HOST44) {
		const float *h = reinterpret_cast<const float *>(s.records) + i * 11u;
		if (reinterpret_cast<const uint32_t *>(h)[9] == 0xFFFFFFFFu) return false;
		px = h[1]; py = h[2]; pz = h[3];
		nx = h[4]; ny = h[5]; nz = h[6];
	} else {
		const float4 *q = reinterpret_cast<const float4 *>(s.records) + i * 2u;
		const float4 a = q[0];
		if (__float_as_int(a.y) == -1) return false;
		const float4 b = q[1];
		RayRegs o;
		if (SRC == SRC_SHADOW_GRID) { uint64_t gx; const uint64_t gy = udivmod(i, p.grid_w, gx); grid_ray(p, (uint32_t)gx, (uint32_t)gy, o); }
		else {
			const float4 *v = reinterpret_cast<const float4 *>(p.rays) + i * 2u;
			const float4 c = v[0], d = v[1];
			o.ox = c.x; o.oy = c.y; o.oz = c.z; o.dx = d.x; o.dy = d.y; o.dz = d.z;
		}
		px = o.ox + o.dx * a.x; py = o.oy + o.dy * a.x; pz = o.oz + o.dz * a.x;
		nx = b.x; ny = b.y; nz = b.z;
	}
	r.ox = px + nx * 1e-3f; r.oy = py + ny * 1e-3f; r.oz = pz + nz * 1e-3f;
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

// The lit mask: 1 lit (no occluder, or no ray), 0 shadowed.
__device__ __forceinline__ void store_lit(const TraceParams &p, uint64_t g, bool lit)
{
	reinterpret_cast<uint8_t *>(p.hits)[g] = lit ? 1 : 0;
}
