// path_kernel.h — the path tracer's per-pixel state (mrt_path_step / mrt_path_grid_step, and mrt_path_step_emitters / its grid form;
// the two small kernels of mrt_path_init and
// mrt_path_finish are path_frame_kernel.h).  Included by shade_kernels.hip (inside namespace mrt, after light_kernel.h; path.h holds PathParams).
//
// The rest of CPUPathTracer's loop body (src/modules/graphics/cpu_path_tracer.h:110-194) around the links already resident: the
// radiance accumulation, the throughput weights of PathTrace::sample_bounce (path_trace.h:213-246), Russian roulette and the `active`
// flag.  One thread per record, nothing walked: the state as two 16-byte loads, the record and
// its ray as record_surface reads them, the row as four 16-byte loads, the direct light as one, then two 16-byte stores and one or
// two bytes.  The environment, the bounce index and the generator's jump are kernel arguments: the tests of bounce == 0, bounce >= 2
// and bounce == max_bounces are uniform.  Every floating-point expression is in the order include/mrt_hip.h states (nothing is
// contracted).  No LDS, no scratch.
//
// The sampler is source_common.h's sample_bounce, the one bounce_kernel.h's bounce_ray draws its ray with; the sky, F0 and the
// diffuse albedo, Schlick and smith_g1 are light_kernel.h's.  With a panorama resident (PANO) the sky of a miss is sample(d) * energy;
// the ambient line of bounce 0 is the same line either way, as in the reference.  The panorama is a kernel argument of its own.
#pragma once

// EMIT (mrt_path_step_emitters): emitter sampling has already counted, at the previous vertex, the emission a diffuse-lobe ray finds --
// from bounce 1 on the emission line runs only where prev_lobe[i] is MRT_LOBE_SPECULAR.  prev_lobe may be s.out_lobe: the entry is read
// here, before the end of the step writes it.
template <int SRC, bool PANO, bool EMIT = false>
__device__ __forceinline__ void path_step_record(const TraceParams &p, const PathParams &s, const PanoramaParams &pano, const uint8_t *prev_lobe = nullptr)
{
	constexpr bool HOST = SRC == SURF_HOST, GRID = SRC == SURF_GRID;
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	bool alive = false; // the entry is active after this step (lanes past the end: false; every lane reaches the ballot)
	if (i < p.count) {
		float4 *st = reinterpret_cast<float4 *>(s.state) + i * 2u;
		const float4 s0 = st[0];
		uint32_t lobe = MRT_LOBE_NONE;
		if (__float_as_uint(s0.w) != 0u) {
			const float4 s1 = st[1];
			float tr = s0.x, tg = s0.y, tb = s0.z, rr = s1.x, rg = s1.y, rb = s1.z;
			Surface sf = {};
			const bool hit = record_surface<HOST, GRID>(p, s.records, i, sf);
			if (!hit) {
				float dx, dy, dz, kr, kg, kb;
				record_direction<HOST, GRID>(p, i, dx, dy, dz);
				if constexpr (PANO) panorama_sky(pano, dx, dy, dz, kr, kg, kb);
				else sky_gradient(s.zenith, s.horizon, s.ground, dy, kr, kg, kb);
				rr = rr + tr * kr; rg = rg + tg * kg; rb = rb + tb * kb;
			} else {
				const float4 *row = reinterpret_cast<const float4 *>(s.rows) + i * 4u;
				const float4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3]; // {n, n_dot_v | albedo, metallic | emission, roughness | uv, specular, material}
				const float4 dl = reinterpret_cast<const float4 *>(s.direct)[i];
				const float ndv = r0.w;
				float f0[3], df[3];
				f0_diffuse(r1, r3.z, f0, df);
				bool emits = true;
				if constexpr (EMIT) emits = s.bounce == 0u || prev_lobe[i] == MRT_LOBE_SPECULAR;
				if (emits) { rr = rr + tr * r2.x; rg = rg + tg * r2.y; rb = rb + tb * r2.z; }
				rr = rr + tr * dl.x; rg = rg + tg * dl.y; rb = rb + tb * dl.z;
				if (s.bounce == 0u) {
					rr = rr + ((tr * df[0]) * s.ambient[0]) * s.ambient_energy;
					rg = rg + ((tg * df[1]) * s.ambient[1]) * s.ambient_energy;
					rb = rb + ((tb * df[2]) * s.ambient[2]) * s.ambient_energy;
				}
				if (s.bounce != s.max_bounces) {
					face_normal(sf);
					uint32_t state = (kPcgInc + ((uint32_t)i * 1009u + s.seed_add)) * kPcgMul + kPcgInc;
					state = s.jump_a * state + s.jump_c;
					const BounceSample b = sample_bounce(sf, r1.w, r2.w, state);
					if (!(b.ndl <= 0.0f)) { // (<= 0: below the surface, an invalid sample; the throughput is not touched)
						float wr, wg, wb;
						if (b.specular) {
							const float ndh = max0((sf.nx * b.hx + sf.ny * b.hy) + sf.nz * b.hz);
							const float g_term = smith_g1(ndv, b.a2) * smith_g1(b.ndl, b.a2);
							float f[3];
							schlick(f0, b.vh, f);
							const float common = (g_term * b.vh) / (((ndv * ndh) * b.sp) + 1e-7f);
							wr = f[0] * common; wg = f[1] * common; wb = f[2] * common;
						} else {
							const float inv = 1.0f / (1.0f - b.sp);
							wr = df[0] * inv; wg = df[1] * inv; wb = df[2] * inv;
						}
						tr = tr * wr; tg = tg * wg; tb = tb * wb;
						alive = true;
						if (s.bounce >= 2u) {
							float mx = tr < tg ? tg : tr;
							mx = mx < tb ? tb : mx;
							const float surv = 0.95f < mx ? 0.95f : mx;
							const float u3 = pcg_float(state * kPcgMul + kPcgInc);
							if (u3 >= surv) alive = false;
							else { const float is = 1.0f / surv; tr = tr * is; tg = tg * is; tb = tb * is; }
						}
						if (alive) lobe = b.specular ? MRT_LOBE_SPECULAR : MRT_LOBE_DIFFUSE;
					}
				}
			}
			float4 o0, o1;
			o0.x = tr; o0.y = tg; o0.z = tb; o0.w = __uint_as_float(alive ? 1u : 0u);
			o1.x = rr; o1.y = rg; o1.z = rb; o1.w = s1.w;
			st[0] = o0; st[1] = o1;
		}
		s.out_select[i] = alive ? 1 : 0;
		if (s.out_lobe != nullptr) s.out_lobe[i] = (uint8_t)lobe;
	}
	if (s.active_count != nullptr) { // one vector atomic per wave that has an active entry
		const unsigned long long live = __ballot(alive);
		if ((threadIdx.x & 63u) == 0u && live != 0ull) atomicAdd(s.active_count, (uint32_t)__popcll(live));
	}
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void path_step_kernel(const TraceParams p, const PathParams s)
{
	path_step_record<SRC, false>(p, s, PanoramaParams{});
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void path_step_panorama_kernel(const TraceParams p, const PathParams s, const PanoramaParams pano)
{
	path_step_record<SRC, true>(p, s, pano);
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void path_step_emitters_kernel(const TraceParams p, const PathParams s, const uint8_t *prev_lobe)
{
	path_step_record<SRC, false, true>(p, s, PanoramaParams{}, prev_lobe);
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void path_step_emitters_panorama_kernel(const TraceParams p, const PathParams s, const PanoramaParams pano,
		const uint8_t *prev_lobe)
{
	path_step_record<SRC, true, true>(p, s, pano, prev_lobe);
}
