// light_kernel.h — direct light on resolved surfaces (mrt_light_surfaces / mrt_light_grid_surfaces; mrt_light_selected_surfaces /
// mrt_light_grid_selected_surfaces: one light per record, drawn by mrt_cast_selected_shadows), plain and with a panorama resident
// (mrt_upload_panorama), and the shading formulas the path step shares with it.  Included by shade_kernels.hip (inside namespace mrt,
// after source_common.h; lighting.h holds LightParams and pow01, panorama.h PanoramaParams and the sampler's arithmetic).
//
// ShadePass::cook_torrance_multi_light of the reference (src/modules/graphics/shade_pass.h:597-657) and the terms shade_material adds
// around it (:669-716), against the rows resolve_surfaces_kernel wrote.  One thread per record, nothing walked: the record and its ray
// as record_surface reads them, the row as four 16-byte loads, one mask byte per light at stride count (consecutive lanes read
// consecutive bytes), one 16-byte store.  The lights and the environment are kernel arguments: the loop over lights, the switch on a
// light's type and the tests of `mask` and `has_env` are uniform.  Every floating-point expression is in the order include/mrt_hip.h
// states (nothing is contracted); pow01 is fp64 and runs only for point and spot lights within range.  No LDS, no scratch.
//
// With a panorama (PANO; sky_color's and shade_material's panorama branches, shade_pass.h:248-257, :692-699) a miss writes
// sample(d) * energy and a hit's ambient factor is sample(n) * energy.  The panorama's pointer, dimensions and energy are a third
// kernel argument.  A record samples once -- the row's normal or the ray's direction -- before the loop over lights: two atan2_core in
// fp64 (about 45 fp64 operations and one division each), then four 16-byte loads whose columns x0 and x1 are neighbours except at the
// wrap.
#pragma once

// the incoming direction of record i as given, hit or miss (the sky of a miss reads it)
template <bool HOST, bool GRID>
__device__ __forceinline__ void record_direction(const TraceParams &p, uint64_t i, float &dx, float &dy, float &dz)
{
	if (HOST) {
		const float *v = reinterpret_cast<const float *>(p.rays) + i * 15u;
		dx = v[3]; dy = v[4]; dz = v[5];
	} else if (GRID) {
		RayRegs o;
		uint64_t gx; const uint64_t gy = udivmod(i, p.grid_w, gx);
		grid_ray(p, (uint32_t)gx, (uint32_t)gy, o);
		dx = o.dx; dy = o.dy; dz = o.dz;
	} else {
		const float4 d = (reinterpret_cast<const float4 *>(p.rays) + i * 2u)[1];
		dx = d.x; dy = d.y; dz = d.z;
	}
}

__device__ __forceinline__ float max0(float x) { return x < 0.0f ? 0.0f : x; }

// g1 of geometry_smith_ggx
__device__ __forceinline__ float smith_g1(float x, float a2)
{
	return (2.0f * x) / ((x + __builtin_sqrtf(a2 + ((1.0f - a2) * x) * x)) + 1e-7f);
}

// extract_surface's F0 and diffuse albedo of a row's {albedo, metallic} and its specular
__device__ __forceinline__ void f0_diffuse(const float4 &am, float specular, float (&f0)[3], float (&df)[3])
{
	const float one_m = 1.0f - am.w, dielectric = (0.04f * specular) * 2.0f;
	f0[0] = dielectric * one_m + am.x * am.w; f0[1] = dielectric * one_m + am.y * am.w; f0[2] = dielectric * one_m + am.z * am.w;
	df[0] = am.x * one_m; df[1] = am.y * one_m; df[2] = am.z * one_m;
}

// fresnel_schlick of v . h, per channel
__device__ __forceinline__ void schlick(const float (&f0)[3], float v_dot_h, float (&f)[3])
{
	const float t = 1.0f - v_dot_h, t2 = t * t, t5 = (t2 * t2) * t;
	f[0] = f0[0] + (1.0f - f0[0]) * t5; f[1] = f0[1] + (1.0f - f0[1]) * t5; f[2] = f0[2] + (1.0f - f0[2]) * t5;
}

// sky_color's analytic gradient (shade_pass.h:259-274) of a direction's y as given
__device__ __forceinline__ void sky_gradient(const float (&zenith)[3], const float (&horizon)[3], const float (&ground)[3], float dy,
		float &r, float &g, float &b)
{
	const float t = dy * 0.5f + 0.5f;
	if (t > 0.5f) {
		const float u = (t - 0.5f) * 2.0f;
		r = horizon[0] + (zenith[0] - horizon[0]) * u;
		g = horizon[1] + (zenith[1] - horizon[1]) * u;
		b = horizon[2] + (zenith[2] - horizon[2]) * u;
	} else {
		const float u = t * 2.0f;
		r = ground[0] + (horizon[0] - ground[0]) * u;
		g = ground[1] + (horizon[1] - ground[1]) * u;
		b = ground[2] + (horizon[2] - ground[2]) * u;
	}
}

// sample(dir) * energy (include/mrt_hip.h): panorama.h's sky_panorama with each texel read as one 16-byte load
__device__ __forceinline__ void panorama_sky(const PanoramaParams &pano, float dx, float dy, float dz, float &r, float &g, float &b)
{
	r = g = b = 0.0f;
	if (!finite3(dx, dy, dz)) return;
	float u, v;
	equirect_uv(dx, dy, dz, u, v);
	PanoTaps t;
	panorama_taps(u, v, pano.width, pano.height, t);
	const float4 *texels = reinterpret_cast<const float4 *>(pano.texels);
	const float4 p00 = texels[t.i00], p10 = texels[t.i10], p01 = texels[t.i01], p11 = texels[t.i11];
	r = pano_blend(p00.x, p10.x, p01.x, p11.x, t) * pano.energy;
	g = pano_blend(p00.y, p10.y, p01.y, p11.y, t) * pano.energy;
	b = pano_blend(p00.z, p10.z, p01.z, p11.z, t) * pano.energy;
}

// What every light's term reads of a hit: the position, the row's normal and n . v, the view direction, the surface's F0 and diffuse
// albedo, a2 = roughness^4 and g1(n . v).
struct LitPoint { float px, py, pz, nx, ny, nz, ndv, vx, vy, vz, a2, g1v; float f0[3], df[3]; };

// One light's pass through cook_torrance_multi_light's loop at a hit (include/mrt_hip.h): rgb.c = rgb.c + the addend of light K, the one
// text of it for the loop over all lights and for the one selected light (which enters with rgb = 0).  Nothing is added where the light
// is skipped -- out of range, attenuated away, behind the surface, or lit() == false, which is asked after ndl and before the specular
// terms (the all-lights loop reads its mask byte there).
template <class Lit>
__device__ __forceinline__ void add_light_term(const KernelLight &K, const LitPoint &q, Lit lit, float &cr, float &cg, float &cb)
{
	constexpr float PI = 3.14159265358979323846f;
	float lx, ly, lz, atten = 1.0f;
	if (K.type == MRT_LIGHT_DIRECTIONAL) { lx = K.direction[0]; ly = K.direction[1]; lz = K.direction[2]; }
	else {
		const float tx = K.position[0] - q.px, ty = K.position[1] - q.py, tz = K.position[2] - q.pz;
		const float dist = __builtin_sqrtf((tx * tx + ty * ty) + tz * tz);
		if (dist < 1e-6f || dist > K.range) return;
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
	if (atten < 1e-6f) return;
	const float ndl = (q.nx * lx + q.ny * ly) + q.nz * lz;
	if (ndl <= 0.0f) return;
	if (!lit()) return;
	float hx = q.vx + lx, hy = q.vy + ly, hz = q.vz + lz;
	normalize3(hx, hy, hz);
	const float n_dot_h = max0((q.nx * hx + q.ny * hy) + q.nz * hz), v_dot_h = max0((q.vx * hx + q.vy * hy) + q.vz * hz);
	const float den = (n_dot_h * n_dot_h) * (q.a2 - 1.0f) + 1.0f;
	const float d_term = q.a2 / ((PI * den) * den + 1e-7f);
	const float g_term = q.g1v * smith_g1(ndl, q.a2);
	float f[3];
	schlick(q.f0, v_dot_h, f);
	const float spec_scale = (d_term * g_term) / ((4.0f * q.ndv) * ndl + 1e-7f);
	const float diff_scale = 1.0f / PI;
	cr = cr + ((((q.df[0] * (1.0f - f[0])) * diff_scale + f[0] * spec_scale) * (K.color[0] * atten)) * ndl);
	cg = cg + ((((q.df[1] * (1.0f - f[1])) * diff_scale + f[1] * spec_scale) * (K.color[1] * atten)) * ndl);
	cb = cb + ((((q.df[2] * (1.0f - f[2])) * diff_scale + f[2] * spec_scale) * (K.color[2] * atten)) * ndl);
}

// ---- the light of record i: PANO = a panorama is resident (pano is read only then); SELECTED = the record's one light, s.selected[i],
// scaled by the number of lights (mrt_light_selected_surfaces), instead of the loop over all of them -------------------------------------
template <int SRC, bool PANO, bool SELECTED>
__device__ __forceinline__ void light_record(const TraceParams &p, const LightParams &s, const PanoramaParams &pano)
{
	constexpr bool HOST = SRC == SURF_HOST, GRID = SRC == SURF_GRID;
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= p.count) return;
	Surface sf = {};
	const bool hit = record_surface<HOST, GRID>(p, s.records, i, sf);
	float4 o = {0.0f, 0.0f, 0.0f, 0.0f};
	// PANO: sample(n) * energy of a hit, sample(d) * energy of a miss -- one sampler for both, its texel loads in flight over the loop
	float er = 0.0f, eg = 0.0f, eb = 0.0f;
	if constexpr (PANO) {
		if (s.has_env != 0u) {
			float qx, qy, qz;
			if (hit) { const float4 q = (reinterpret_cast<const float4 *>(s.rows) + i * 4u)[0]; qx = q.x; qy = q.y; qz = q.z; }
			else record_direction<HOST, GRID>(p, i, qx, qy, qz);
			panorama_sky(pano, qx, qy, qz, er, eg, eb);
		}
	}
	if (hit) {
		const float4 *row = reinterpret_cast<const float4 *>(s.rows) + i * 4u;
		const float4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3]; // {n, n_dot_v | albedo, metallic | emission, roughness | uv, specular, material}
		const float ny = r0.y, rough = r2.w;
		LitPoint q;
		q.px = sf.px; q.py = sf.py; q.pz = sf.pz;
		q.nx = r0.x; q.ny = r0.y; q.nz = r0.z; q.ndv = r0.w;
		q.vx = -sf.dx; q.vy = -sf.dy; q.vz = -sf.dz;
		normalize3(q.vx, q.vy, q.vz);
		f0_diffuse(r1, r3.z, q.f0, q.df);
		const float (&df)[3] = q.df;
		const float a = rough * rough;
		q.a2 = a * a;
		q.g1v = smith_g1(q.ndv, q.a2);
		float cr = 0.0f, cg = 0.0f, cb = 0.0f;
		if constexpr (SELECTED) { // the light is indexed per lane: its 16 words are read from the kernel argument where it lies
			const uint32_t k = s.selected[i];
			if (k < s.n_lights && !(s.mask != nullptr && s.mask[i] == 0)) add_light_term(s.light[k], q, [] { return true; }, cr, cg, cb);
			const float n = (float)s.n_lights;
			cr = cr * n; cg = cg * n; cb = cb * n;
		} else {
			for (uint32_t l = 0; l < s.n_lights; l++)
				add_light_term(s.light[l], q, [&] { return !(s.mask != nullptr && s.mask[(uint64_t)l * p.count + i] == 0); }, cr, cg, cb);
		}
		if (s.has_env != 0u) {
			if constexpr (!PANO) { // the ambient factor: the gradient between ground and zenith by the normal's y
				const float blend = ny * 0.5f + 0.5f;
				er = s.ground[0] + (s.zenith[0] - s.ground[0]) * blend;
				eg = s.ground[1] + (s.zenith[1] - s.ground[1]) * blend;
				eb = s.ground[2] + (s.zenith[2] - s.ground[2]) * blend;
			}
			cr = cr + ((df[0] * er) * s.ambient[0]) * s.ambient_energy;
			cg = cg + ((df[1] * eg) * s.ambient[1]) * s.ambient_energy;
			cb = cb + ((df[2] * eb) * s.ambient[2]) * s.ambient_energy;
			cr = cr + r2.x; cg = cg + r2.y; cb = cb + r2.z;
		}
		o.x = cr; o.y = cg; o.z = cb; o.w = 1.0f;
	} else if (s.has_env != 0u) {
		if constexpr (PANO) { o.x = er; o.y = eg; o.z = eb; }
		else {
			float dx, dy, dz;
			record_direction<HOST, GRID>(p, i, dx, dy, dz);
			sky_gradient(s.zenith, s.horizon, s.ground, dy, o.x, o.y, o.z);
		}
	}
	reinterpret_cast<float4 *>(s.out)[i] = o;
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void light_surfaces_kernel(const TraceParams p, const LightParams s)
{
	light_record<SRC, false, false>(p, s, PanoramaParams{});
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void light_panorama_surfaces_kernel(const TraceParams p, const LightParams s, const PanoramaParams pano)
{
	light_record<SRC, true, false>(p, s, pano);
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void light_selected_surfaces_kernel(const TraceParams p, const LightParams s)
{
	light_record<SRC, false, true>(p, s, PanoramaParams{});
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void light_selected_panorama_surfaces_kernel(const TraceParams p, const LightParams s, const PanoramaParams pano)
{
	light_record<SRC, true, true>(p, s, pano);
}
