// bounce_kernel.h — the path tracer's bounce made in the trace kernels (mrt_cast_bounce / mrt_cast_grid_bounce).
// Included by kernels.hip (inside namespace mrt, after source_common.h, before the kernels that use it).
//
// PathTrace::sample_bounce of the reference (src/modules/graphics/path_trace.h:185-251): one draw chooses the lobe against a specular
// probability made from the surface's metallic and roughness, then either a GGX half vector (ggx_sample_half, :132-155) with the view
// direction reflected about it, or the cosine hemisphere of hemisphere_kernel.h.  The direction alone: weights, throughput and roulette
// are the renderer's.  A source family of source_common.h (SRC_BOUNCE_*, closest-hit only); entry i is record i and its result is the
// record mrt_cast(MRT_MODE_NEAREST) writes for the ray.  Plain float operations in this order (nothing is contracted):
//   p, d, n  as hemisphere_kernel.h takes them; n = -n if ((nx*dx + ny*dy) + nz*dz) > 0
//   m  = fminf(fmaxf(metallic, 0), 1), ro = fminf(fmaxf(roughness, 0.04f), 1)      (surface[2i], surface[2i + 1], or the constants;
//                                                                                    a NaN takes the lower bound)
//   sp = m + ((1 - m) * (1 - ro)) * 0.5f, sp = fmaxf(fminf(sp, 0.95f), 0.05f)
//   state0 as hemisphere_kernel.h; state = A * state0 + C, (A, C) of draw first_draw: BounceParams::jump
//   u0 = pcg_float(state), u1 = pcg_float(state'), u2 = pcg_float(state'') with state' = state * mul + inc
//   specular = u0 < sp
//   diffuse:  the direction of hemisphere_kernel.h from (u1, u2)
//   specular: a = ro * ro, a2 = a * a, c = sqrt((1 - u1) / ((1 + (a2 - 1) * u1) + 1e-7f)), s = sqrt(fmaxf(0, 1 - c * c)),
//             (cs, sn) = sincos_2pi(u2), lx = s * cs, ly = s * sn, h = normalized((t * lx + bt * ly) + n * c) with construct_onb(n),
//             v = normalized(-d), vh = fmaxf((vx*hx + vy*hy) + vz*hz, 0), dir = normalized(h * (2 * vh) - v)
//   normalized: l2 = (x*x + y*y) + z*z, 0 if l2 == 0, else three divisions by sqrt(l2)
//   org = p + n * 1e-3, t_min = 1e-4, t_max = the descriptor's
// No ray: a primary miss, select[i] == 0, or ((nx*dirx + ny*diry) + nz*dirz) <= 0 (the reference's "below surface").  The placeholder
// ray and its record (source_common.h); lobe byte MRT_LOBE_NONE.  Nothing walks.
#pragma once

// The bounce ray of entry i (written to out_rays when asked for, its lobe to out_lobe).  false: no ray -- r is the placeholder.
template <int SRC>
__device__ __forceinline__ bool bounce_ray(const TraceParams &p, const BounceParams &s, uint64_t i, RayRegs &r)
{
	bool traced = s.select == nullptr || s.select[i] != 0;
	Surface sf = {};
	if (traced) traced = record_surface<SRC == SRC_BOUNCE_HOST, SRC == SRC_BOUNCE_GRID>(p, s.records, i, sf);
	uint32_t lobe = MRT_LOBE_NONE;
	if (traced) {
		face_normal(sf);
		float metallic = s.metallic, roughness = s.roughness;
		if (s.surface != nullptr) { metallic = s.surface[i * 2u]; roughness = s.surface[i * 2u + 1u]; }
		uint32_t state = (kPcgInc + ((uint32_t)i * 1009u + s.seed_add)) * kPcgMul + kPcgInc;
		state = s.jump.a * state + s.jump.c;
		const BounceSample b = sample_bounce(sf, metallic, roughness, state);
		if (b.ndl <= 0.0f) traced = false; // below the surface: an invalid sample, no ray
		else {
			lobe = b.specular ? MRT_LOBE_SPECULAR : MRT_LOBE_DIFFUSE;
			r.dx = b.vx; r.dy = b.vy; r.dz = b.vz;
			r.ox = sf.px + sf.nx * 1e-3f; r.oy = sf.py + sf.ny * 1e-3f; r.oz = sf.pz + sf.nz * 1e-3f;
			r.t_min = 1e-4f; r.t_max = s.t_max;
		}
	}
	if (!traced) placeholder_ray(r);
	if (s.out_rays != nullptr) store_ray(s.out_rays, SRC == SRC_BOUNCE_HOST, i, r);
	if (s.out_lobe != nullptr) s.out_lobe[i] = (uint8_t)lobe;
	return traced;
}

// The ray of entry i, or (false) the record of an entry without one, stored.
template <int SRC, bool ANY_HIT>
__device__ __forceinline__ bool source_entry(const TraceParams &p, const BounceParams &s, uint64_t i, RayRegs &r)
{
	static_assert(bounce_source(SRC) && !ANY_HIT, "bounce sources are closest-hit");
	if (bounce_ray<SRC>(p, s, i, r)) return true;
	store_placeholder_record(p, i);
	return false;
}
