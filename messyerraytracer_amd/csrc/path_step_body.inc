// path_step_body.inc -- the body of path_step_kernel (MRT_PANO 0) and of path_step_panorama_kernel (MRT_PANO 1: `pano` is its
// PanoramaParams), both in path_kernel.h: one text, so that the two differ in nothing but the sky of a miss, and the first is compiled
// from the lines it always had.
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
#if MRT_PANO
				panorama_sky(pano, dx, dy, dz, kr, kg, kb);
#else
				sky_gradient(s.zenith, s.horizon, s.ground, dy, kr, kg, kb);
#endif
				rr = rr + tr * kr; rg = rg + tg * kg; rb = rb + tb * kb;
			} else {
				const float4 *row = reinterpret_cast<const float4 *>(s.rows) + i * 4u;
				const float4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3]; // {n, n_dot_v | albedo, metallic | emission, roughness | uv, specular, material}
				const float4 dl = reinterpret_cast<const float4 *>(s.direct)[i];
				const float ndv = r0.w, metallic = r1.w;
				const float one_m = 1.0f - metallic, dielectric = (0.04f * r3.z) * 2.0f;
				const float f0r = dielectric * one_m + r1.x * metallic, f0g = dielectric * one_m + r1.y * metallic, f0b = dielectric * one_m + r1.z * metallic;
				const float dfr = r1.x * one_m, dfg = r1.y * one_m, dfb = r1.z * one_m;
				rr = rr + tr * r2.x; rg = rg + tg * r2.y; rb = rb + tb * r2.z;
				rr = rr + tr * dl.x; rg = rg + tg * dl.y; rb = rb + tb * dl.z;
				if (s.bounce == 0u) {
					rr = rr + ((tr * dfr) * s.ambient[0]) * s.ambient_energy;
					rg = rg + ((tg * dfg) * s.ambient[1]) * s.ambient_energy;
					rb = rb + ((tb * dfb) * s.ambient[2]) * s.ambient_energy;
				}
				if (s.bounce != s.max_bounces) {
					// ---- bounce_ray's sampler (bounce_kernel.h), keeping the half vector ----
					face_normal(sf);
					const float m = fminf(fmaxf(metallic, 0.0f), 1.0f), ro = fminf(fmaxf(r2.w, 0.04f), 1.0f);
					float sp = m + ((1.0f - m) * (1.0f - ro)) * 0.5f;
					sp = fmaxf(fminf(sp, 0.95f), 0.05f);
					const uint32_t pixel = (uint32_t)i;
					uint32_t state = (kPcgInc + (pixel * 1009u + s.seed_add)) * kPcgMul + kPcgInc;
					state = s.jump_a * state + s.jump_c;
					const float u0 = pcg_float(state);
					state = state * kPcgMul + kPcgInc;
					const float u1 = pcg_float(state);
					state = state * kPcgMul + kPcgInc;
					const float u2 = pcg_float(state);
					const bool specular = u0 < sp;
					const float a = ro * ro, a2 = a * a;
					float lr, z;
					if (specular) {
						z = __builtin_sqrtf((1.0f - u1) / ((1.0f + (a2 - 1.0f) * u1) + 1e-7f));
						lr = __builtin_sqrtf(fmaxf(0.0f, 1.0f - z * z));
					} else {
						lr = __builtin_sqrtf(u1); z = __builtin_sqrtf(fmaxf(0.0f, 1.0f - u1));
					}
					float vx, vy, vz; // the direction; for the specular lobe first the half vector
					onb_direction(sf, lr, z, u2, vx, vy, vz);
					float hx = vx, hy = vy, hz = vz, vh = 0.0f;
					if (specular) {
						float wx = -sf.dx, wy = -sf.dy, wz = -sf.dz;
						normalize3(wx, wy, wz);
						vh = fmaxf((wx * vx + wy * vy) + wz * vz, 0.0f);
						const float k = 2.0f * vh;
						vx = vx * k - wx; vy = vy * k - wy; vz = vz * k - wz;
						normalize3(vx, vy, vz);
					}
					const float ndl = (sf.nx * vx + sf.ny * vy) + sf.nz * vz;
					if (!(ndl <= 0.0f)) { // (<= 0: below the surface, an invalid sample; the throughput is not touched)
						float wr, wg, wb;
						if (specular) {
							const float ndh = max0((sf.nx * hx + sf.ny * hy) + sf.nz * hz);
							const float g_term = smith_g1(ndv, a2) * smith_g1(ndl, a2);
							const float t = 1.0f - vh, t2 = t * t, t5 = (t2 * t2) * t;
							const float fr = f0r + (1.0f - f0r) * t5, fg = f0g + (1.0f - f0g) * t5, fb = f0b + (1.0f - f0b) * t5;
							const float common = (g_term * vh) / (((ndv * ndh) * sp) + 1e-7f);
							wr = fr * common; wg = fg * common; wb = fb * common;
						} else {
							const float inv = 1.0f / (1.0f - sp);
							wr = dfr * inv; wg = dfg * inv; wb = dfb * inv;
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
						if (alive) lobe = specular ? MRT_LOBE_SPECULAR : MRT_LOBE_DIFFUSE;
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
