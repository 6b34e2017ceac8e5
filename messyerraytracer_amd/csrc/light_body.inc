// light_body.inc -- the body of light_surfaces_kernel (light_kernel.h, MRT_PANO 0) and of light_panorama_surfaces_kernel
// (light_panorama_kernel.h, MRT_PANO 1: `pano` is its PanoramaParams): one text, so that the two differ in nothing but the environment's
// two lines, and the first is compiled from the lines it always had.
	constexpr bool HOST = SRC == SURF_HOST, GRID = SRC == SURF_GRID;
	constexpr float PI = 3.14159265358979323846f;
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= p.count) return;
	Surface sf = {};
	const bool hit = record_surface<HOST, GRID>(p, s.records, i, sf);
	float4 o = {0.0f, 0.0f, 0.0f, 0.0f};
#if MRT_PANO
	// sample(n) * energy of a hit, sample(d) * energy of a miss: one sampler for both, its texel loads in flight over the loop
	float er = 0.0f, eg = 0.0f, eb = 0.0f;
	if (s.has_env != 0u) {
		float qx, qy, qz;
		if (hit) { const float4 q = (reinterpret_cast<const float4 *>(s.rows) + i * 4u)[0]; qx = q.x; qy = q.y; qz = q.z; }
		else record_direction<HOST, GRID>(p, i, qx, qy, qz);
		panorama_sky(pano, qx, qy, qz, er, eg, eb);
	}
#endif
	if (hit) {
		const float4 *row = reinterpret_cast<const float4 *>(s.rows) + i * 4u;
		const float4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3]; // {n, n_dot_v | albedo, metallic | emission, roughness | uv, specular, material}
		const float nx = r0.x, ny = r0.y, nz = r0.z, ndv = r0.w, metallic = r1.w, rough = r2.w;
		float vx = -sf.dx, vy = -sf.dy, vz = -sf.dz;
		normalize3(vx, vy, vz);
		const float one_m = 1.0f - metallic, dielectric = (0.04f * r3.z) * 2.0f;
		const float f0r = dielectric * one_m + r1.x * metallic, f0g = dielectric * one_m + r1.y * metallic, f0b = dielectric * one_m + r1.z * metallic;
		const float dfr = r1.x * one_m, dfg = r1.y * one_m, dfb = r1.z * one_m;
		const float a = rough * rough, a2 = a * a;
		const float g1v = smith_g1(ndv, a2);
		const float diff_scale = 1.0f / PI;
		float cr = 0.0f, cg = 0.0f, cb = 0.0f;
		for (uint32_t l = 0; l < s.n_lights; l++) {
			const KernelLight &K = s.light[l];
			float lx, ly, lz, atten = 1.0f;
			if (K.type == MRT_LIGHT_DIRECTIONAL) { lx = K.direction[0]; ly = K.direction[1]; lz = K.direction[2]; }
			else {
				const float tx = K.position[0] - sf.px, ty = K.position[1] - sf.py, tz = K.position[2] - sf.pz;
				const float dist = __builtin_sqrtf((tx * tx + ty * ty) + tz * tz);
				if (dist < 1e-6f || dist > K.range) continue;
				lx = tx / dist; ly = ty / dist; lz = tz / dist;
				const float ratio = dist / K.range;
				atten = pow01(max0(1.0f - ratio * ratio), K.attenuation);
				if (K.type == MRT_LIGHT_SPOT) {
					const float cos_angle = (lx * K.direction[0] + ly * K.direction[1]) + lz * K.direction[2];
					float spot = 0.0f;
					if (!(cos_angle <= K.cos_outer)) spot = pow01(max0((cos_angle - K.cos_outer) / K.one_minus_cos_outer), K.spot_attenuation);
					atten = atten * spot;
				}
			}
			if (atten < 1e-6f) continue;
			const float ndl = (nx * lx + ny * ly) + nz * lz;
			if (ndl <= 0.0f) continue;
			if (s.mask != nullptr && s.mask[(uint64_t)l * p.count + i] == 0) continue;
			float hx = vx + lx, hy = vy + ly, hz = vz + lz;
			normalize3(hx, hy, hz);
			const float n_dot_h = max0((nx * hx + ny * hy) + nz * hz), v_dot_h = max0((vx * hx + vy * hy) + vz * hz);
			const float den = (n_dot_h * n_dot_h) * (a2 - 1.0f) + 1.0f;
			const float d_term = a2 / ((PI * den) * den + 1e-7f);
			const float g_term = g1v * smith_g1(ndl, a2);
			const float t = 1.0f - v_dot_h, t2 = t * t, t5 = (t2 * t2) * t;
			const float fr = f0r + (1.0f - f0r) * t5, fg = f0g + (1.0f - f0g) * t5, fb = f0b + (1.0f - f0b) * t5;
			const float spec_scale = (d_term * g_term) / ((4.0f * ndv) * ndl + 1e-7f);
			cr = cr + ((((dfr * (1.0f - fr)) * diff_scale + fr * spec_scale) * (K.color[0] * atten)) * ndl);
			cg = cg + ((((dfg * (1.0f - fg)) * diff_scale + fg * spec_scale) * (K.color[1] * atten)) * ndl);
			cb = cb + ((((dfb * (1.0f - fb)) * diff_scale + fb * spec_scale) * (K.color[2] * atten)) * ndl);
		}
		if (s.has_env != 0u) {
#if MRT_PANO
			cr = cr + ((dfr * er) * s.ambient[0]) * s.ambient_energy;
			cg = cg + ((dfg * eg) * s.ambient[1]) * s.ambient_energy;
			cb = cb + ((dfb * eb) * s.ambient[2]) * s.ambient_energy;
#else
			const float blend = ny * 0.5f + 0.5f;
			cr = cr + ((dfr * (s.ground[0] + (s.zenith[0] - s.ground[0]) * blend)) * s.ambient[0]) * s.ambient_energy;
			cg = cg + ((dfg * (s.ground[1] + (s.zenith[1] - s.ground[1]) * blend)) * s.ambient[1]) * s.ambient_energy;
			cb = cb + ((dfb * (s.ground[2] + (s.zenith[2] - s.ground[2]) * blend)) * s.ambient[2]) * s.ambient_energy;
#endif
			cr = cr + r2.x; cg = cg + r2.y; cb = cb + r2.z;
		}
		o.x = cr; o.y = cg; o.z = cb; o.w = 1.0f;
	} else if (s.has_env != 0u) {
#if MRT_PANO
		o.x = er; o.y = eg; o.z = eb;
#else
		float dx, dy, dz;
		record_direction<HOST, GRID>(p, i, dx, dy, dz);
		const float t = dy * 0.5f + 0.5f;
		if (t > 0.5f) {
			const float u = (t - 0.5f) * 2.0f;
			o.x = s.horizon[0] + (s.zenith[0] - s.horizon[0]) * u;
			o.y = s.horizon[1] + (s.zenith[1] - s.horizon[1]) * u;
			o.z = s.horizon[2] + (s.zenith[2] - s.horizon[2]) * u;
		} else {
			const float u = t * 2.0f;
			o.x = s.ground[0] + (s.horizon[0] - s.ground[0]) * u;
			o.y = s.ground[1] + (s.horizon[1] - s.ground[1]) * u;
			o.z = s.ground[2] + (s.horizon[2] - s.ground[2]) * u;
		}
#endif
	}
	reinterpret_cast<float4 *>(s.out)[i] = o;
