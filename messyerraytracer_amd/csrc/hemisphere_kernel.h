// hemisphere_kernel.h — cosine-weighted hemisphere rays made in the trace kernels (mrt_cast_hemisphere / mrt_cast_grid_hemisphere).
// Included by kernels.hip (inside namespace mrt, after source_common.h, before the kernels that use it).
//
// The diffuse bounce of the reference's path tracer (cosine_hemisphere_sample, src/modules/graphics/path_trace.h:101-120, drawn
// from the PCG32 of path_state.h:40-67 seeded as PathState::init seeds it), and with a short t_max and any-hit its ambient-occlusion
// ray.  A source family of source_common.h (SRC_HEMI_*, either mode); entry g is the pair (sample g / pixels, pixel g % pixels).  Any-hit: one byte per entry, 1 - occluded.  Closest-hit: the record
// mrt_cast(MRT_MODE_NEAREST) writes for the ray.  Plain float operations in this order (nothing is contracted):
//   p, d, n  as reflection_kernel.h takes them from the record and the incoming ray; n = -n if ((nx*dx + ny*dy) + nz*dz) > 0
//   state0   = (inc + seed) * mul + inc  with seed = pixel_index * 1009 + frame * 6529 + 7           (PCG32::seed)
//   state    = A * state0 + C            (A, C) of draw first_draw + 2 * sample: HemiParams::jump
//   u1 = float(out(state)) * 2^-32, u2 = float(out(state * mul + inc)) * 2^-32                       (can be exactly 1.0)
//   r = sqrt(u1), z = sqrt(max(0, 1 - u1))
//   (cs, sn) = sincos_2pi(u2): source_common.h's pair, not a math library's                     (mrt_hip.h says why)
//   x = r * cs, y = r * sn
//   construct_onb(n): sign = copysign(1, nz), a = -1 / (sign + nz), b = (nx * ny) * a,
//       t = (1 + ((sign * nx) * nx) * a, sign * b, (-sign) * nx), bt = (b, sign + (ny * ny) * a, -ny)
//   v = (t * x + bt * y) + n * z per component, dir = v / sqrt((vx*vx + vy*vy) + vz*vz)  (0 if the sum is 0: Vector3::normalized)
//   org = p + n * 1e-3, t_min = 1e-4, t_max = the descriptor's
// No ray: a primary miss, select[pixel] == 0, or ((nx*dirx + ny*diry) + nz*dirz) <= 0 (the reference's "below surface").  Any-hit:
// the byte is 1.  Closest-hit: the placeholder ray and its record (source_common.h).  Nothing walks.
#pragma once

// The hemisphere ray of entry g (written to out_rays when asked for).  false: no ray -- r is the placeholder.
template <int SRC>
__device__ __forceinline__ bool hemisphere_ray(const TraceParams &p, const HemiParams &s, uint64_t g, RayRegs &r)
{
	uint64_t i;
	const uint64_t si = udivmod(g, s.pixels, i);
	bool traced = s.select == nullptr || s.select[i] != 0;
	Surface sf = {};
	if (traced) traced = record_surface<SRC == SRC_HEMI_HOST, SRC == SRC_HEMI_GRID>(p, s.records, i, sf);
	if (traced) {
		face_normal(sf);
		const HemiJump j = s.jump[si];
		uint32_t state = (kPcgInc + ((uint32_t)i * 1009u + s.seed_add)) * kPcgMul + kPcgInc;
		state = j.a * state + j.c;
		const float u1 = pcg_float(state), u2 = pcg_float(state * kPcgMul + kPcgInc);
		const float rr = __builtin_sqrtf(u1), z = __builtin_sqrtf(fmaxf(0.0f, 1.0f - u1));
		float vx, vy, vz;
		onb_direction(sf, rr, z, u2, vx, vy, vz);
		if ((sf.nx * vx + sf.ny * vy) + sf.nz * vz <= 0.0f) traced = false; // below the surface: an invalid sample, no ray
		else {
			r.dx = vx; r.dy = vy; r.dz = vz;
			r.ox = sf.px + sf.nx * 1e-3f; r.oy = sf.py + sf.ny * 1e-3f; r.oz = sf.pz + sf.nz * 1e-3f;
			r.t_min = 1e-4f; r.t_max = s.t_max;
		}
	}
	if (!traced) placeholder_ray(r);
	if (s.out_rays != nullptr) store_ray(s.out_rays, SRC == SRC_HEMI_HOST, g, r);
	return traced;
}

// The ray of entry g, or (false) the result of an entry without one, stored: the byte 1 (any-hit) or the placeholder's record.
template <int SRC, bool ANY_HIT>
__device__ __forceinline__ bool source_entry(const TraceParams &p, const HemiParams &s, uint64_t g, RayRegs &r)
{
	static_assert(hemisphere_source(SRC), "a hemisphere source");
	if (hemisphere_ray<SRC>(p, s, g, r)) return true;
	if (ANY_HIT) store_lit(p, g, true);
	else store_placeholder_record(p, g);
	return false;
}
