// emitter_sample_kernel.h — a point of an emissive triangle sampled for a record: the one text of it for the cast that traces the
// shadow ray (emitter_shadow_kernel.h, kernels.hip) and for the light call that derives the same point again (emitter_light_kernel.h,
// shade_kernels.hip).  Included inside namespace mrt, after source_common.h.
//
// Plain float operations in the order include/mrt_hip.h states for mrt_cast_emitter_shadows (nothing is contracted):
//   state0 as hemisphere_kernel.h; state = A * state0 + C, (A, C) of draw `draw`; word = pcg_word(state), u1 = pcg_float(state'),
//   u2 = pcg_float(state'') with state' = state * mul + inc
//   target = word >> 1; target >= total: no emitter; else k = the first entry with cdf[k] > target (a binary search in device memory)
//   su = sqrt(u1), a = su * (1 - u2), b = su * u2, y = (v0 + e1 * a) + e2 * b
//   n = the record's normal faced against the incoming ray; org = p + n * 1e-3, to = y - org, dist2 = (x*x + y*y) + z*z,
//   dist = sqrt(dist2), dir = to / dist; ng = normalized(e1 x e2); refused: dist < 1e-6f, n . dir <= 0, |ng . dir| < 1e-6f
#pragma once

// The generator's state before the selecting draw of entry i.
__device__ __forceinline__ uint32_t emitter_stream(uint64_t i, uint32_t seed_add, HemiJump jump)
{
	const uint32_t state = (kPcgInc + ((uint32_t)i * 1009u + seed_add)) * kPcgMul + kPcgInc;
	return jump.a * state + jump.c;
}

// k of a selecting word, or MRT_EMITTER_NONE: the first entry of the inclusive CDF above target = word >> 1.  Up to 20 dependent loads
// per lane; the CDF stays in device memory (the walks use the LDS for their stacks).
__device__ __forceinline__ uint32_t emitter_select(const EmitterTable &t, uint32_t word)
{
	const uint32_t target = word >> 1;
	if (t.n == 0u || target >= t.total) return MRT_EMITTER_NONE;
	uint32_t lo = 0u, hi = t.n - 1u;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (t.cdf[mid] > target) hi = mid;
		else lo = mid + 1u;
	}
	return lo;
}

// What the term reads of a sampled point: the direction to it, its squared distance, n . dir, |ng . dir|, and the last three rows of
// the emitter as loaded ({e2, area}, {Le, material}; q).
struct EmitterPoint { float dx, dy, dz, dist, dist2, ndl, cy, area, ler, leg, leb; uint32_t q; };

// The point of emitter k for the stream at `state` (the state of the selecting draw) seen from a surface whose normal has been faced.
// false: refused (no ray).  ox, oy, oz = the shadow ray's origin.
__device__ __forceinline__ bool emitter_point(const EmitterTable &t, uint32_t k, uint32_t state, const Surface &sf, float &ox, float &oy,
		float &oz, EmitterPoint &e)
{
	const float4 *row = reinterpret_cast<const float4 *>(t.rows) + (size_t)k * 4u;
	const float4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
	state = state * kPcgMul + kPcgInc;
	const float u1 = pcg_float(state);
	state = state * kPcgMul + kPcgInc;
	const float u2 = pcg_float(state);
	const float su = __builtin_sqrtf(u1), a = su * (1.0f - u2), b = su * u2;
	const float yx = (r0.x + r1.x * a) + r2.x * b, yy = (r0.y + r1.y * a) + r2.y * b, yz = (r0.z + r1.z * a) + r2.z * b;
	ox = sf.px + sf.nx * 1e-3f; oy = sf.py + sf.ny * 1e-3f; oz = sf.pz + sf.nz * 1e-3f;
	const float tx = yx - ox, ty = yy - oy, tz = yz - oz;
	e.dist2 = (tx * tx + ty * ty) + tz * tz;
	e.dist = __builtin_sqrtf(e.dist2);
	e.q = __float_as_uint(r0.w); e.area = r2.w; e.ler = r3.x; e.leg = r3.y; e.leb = r3.z;
	if (e.dist < 1e-6f) return false;
	e.dx = tx / e.dist; e.dy = ty / e.dist; e.dz = tz / e.dist;
	e.ndl = (sf.nx * e.dx + sf.ny * e.dy) + sf.nz * e.dz;
	if (e.ndl <= 0.0f) return false;
	float gx = r1.y * r2.z - r1.z * r2.y, gy = r1.z * r2.x - r1.x * r2.z, gz = r1.x * r2.y - r1.y * r2.x;
	normalize3(gx, gy, gz);
	e.cy = __builtin_fabsf((gx * e.dx + gy * e.dy) + gz * e.dz);
	return !(e.cy < 1e-6f);
}
