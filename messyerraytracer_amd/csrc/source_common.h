// source_common.h — what every ray source shares (shadow_kernel.h, selected_shadow_kernel.h, reflection_kernel.h, hemisphere_kernel.h,
// bounce_kernel.h, emitter_shadow_kernel.h, and gbuffer_kernel.h, whose entries are pixels of a G-buffer, not records).  Included by kernels.hip (inside namespace mrt, after
// device_common.h, before the family headers) and, for record_surface, by shade_kernels.hip.
//
// A source family is a parameter struct (mrt_internal.h: ShadowParams, SelectShadowParams, ReflectParams, HemiParams, BounceParams, GBufferParams, EmitterShadowParams;
// SourceFamily<S> names its sources and its modes) plus one overload of
//   template <int SRC, bool ANY_HIT> bool source_entry(const TraceParams &p, const S &s, uint64_t g, RayRegs &r)
// which makes the ray of entry g (true: r is a ray to walk) or stores the result of an entry without a ray (false: the lit byte, or
// the placeholder's record; nothing walks).  The lane kernels, persistent or not, and the two-level kernels take (S, SRC, ANY_HIT) as
// template parameters and call it where a SRC_CAST kernel calls load_ray; everything else of a record-driven cast is written once.
// Every floating-point expression here is in the order its family's header states (nothing is contracted).
#pragma once

// The parameter object of a SRC_CAST kernel, whose rays come from load_ray: source_entry is declared for it so that the branch a
// SRC_CAST kernel discards still type-checks.  Never called.
struct NoSource {};
template <int SRC, bool ANY_HIT>
__device__ bool source_entry(const TraceParams &p, const NoSource &s, uint64_t g, RayRegs &r);

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

// The lit mask: 1 lit (no occluder, or no ray), 0 shadowed.
__device__ __forceinline__ void store_lit(const TraceParams &p, uint64_t g, bool lit)
{
	reinterpret_cast<uint8_t *>(p.hits)[g] = lit ? 1 : 0;
}

// The record of an entry without a ray: what mrt_cast writes for the placeholder (t_min >= t_max: a miss at t = t_max = 0).
__device__ __forceinline__ void store_placeholder_record(const TraceParams &p, uint64_t i)
{
	RayRegs r;
	placeholder_ray(r);
	store_hit(p, i, r, r.t_max, -1, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u, 0xFFFFFFFFu);
}

// The surface of record i and the ray that found it: position p, normal n, incoming direction d.  false: the record is a miss (sf is
// left as it was).  HOST: mrt_host_hit44 records, which carry the position, and mrt_host_ray60 rays, read for d alone.  Otherwise
// mrt_hit32 records: p = o + d * t of the incoming ray (the expression of store_hit), and that ray is entry i of p.rays (mrt_ray32)
// or, GRID, pixel i of the camera grid, made again.  NEED_DIR false (shadows): sf.d is not set, and a HOST source does not read
// p.rays at all.
struct Surface { float px, py, pz, nx, ny, nz, dx, dy, dz; };
template <bool HOST, bool GRID, bool NEED_DIR = true>
__device__ __forceinline__ bool record_surface(const TraceParams &p, const void *records, uint64_t i, Surface &sf)
{
	bool hit = true;
	if (HOST) {
		const float *h = reinterpret_cast<const float *>(records) + i * 11u;
		if (reinterpret_cast<const uint32_t *>(h)[9] == 0xFFFFFFFFu) hit = false;
		else {
			const float *v = NEED_DIR ? reinterpret_cast<const float *>(p.rays) + i * 15u : nullptr;
			sf.px = h[1]; sf.py = h[2]; sf.pz = h[3];
			sf.nx = h[4]; sf.ny = h[5]; sf.nz = h[6];
			if (NEED_DIR) { sf.dx = v[3]; sf.dy = v[4]; sf.dz = v[5]; }
		}
	} else {
		const float4 *q = reinterpret_cast<const float4 *>(records) + i * 2u;
		const float4 a = q[0];
		if (__float_as_int(a.y) == -1) hit = false;
		else {
			const float4 b = q[1];
			RayRegs o;
			if (GRID) { uint64_t gx; const uint64_t gy = udivmod(i, p.grid_w, gx); grid_ray(p, (uint32_t)gx, (uint32_t)gy, o); }
			else {
				const float4 *v = reinterpret_cast<const float4 *>(p.rays) + i * 2u;
				const float4 c = v[0], d = v[1];
				o.ox = c.x; o.oy = c.y; o.oz = c.z; o.dx = d.x; o.dy = d.y; o.dz = d.z;
			}
			sf.px = o.ox + o.dx * a.x; sf.py = o.oy + o.dy * a.x; sf.pz = o.oz + o.dz * a.x;
			sf.nx = b.x; sf.ny = b.y; sf.nz = b.z;
			if (NEED_DIR) { sf.dx = o.dx; sf.dy = o.dy; sf.dz = o.dz; }
		}
	}
	return hit;
}

// record i is a hit: record_surface's test alone (prim_id of either layout), for a source that has something to store for a miss
template <bool HOST>
__device__ __forceinline__ bool record_is_hit(const void *records, uint64_t i)
{
	if (HOST) return reinterpret_cast<const uint32_t *>(records)[i * 11u + 9u] != 0xFFFFFFFFu;
	return __float_as_int((reinterpret_cast<const float4 *>(records) + i * 2u)[0].y) != -1;
}

// Faces the normal against the incoming ray: n = -n if c = ((nx*dx + ny*dy) + nz*dz) > 0.  Returns the faced n's dot product with d
// (the same sum negated, exactly).
__device__ __forceinline__ float face_normal(Surface &sf)
{
	float c = (sf.nx * sf.dx + sf.ny * sf.dy) + sf.nz * sf.dz;
	if (c > 0.0f) { sf.nx = -sf.nx; sf.ny = -sf.ny; sf.nz = -sf.nz; c = -c; }
	return c;
}

// PCG32::next's output permutation of a state
__device__ __forceinline__ uint32_t pcg_word(uint32_t state)
{
	const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
	return (word >> 22u) ^ word;
}

// ... as PCG32::next_float scales it
__device__ __forceinline__ float pcg_float(uint32_t state)
{
	return (float)pcg_word(state) * 2.3283064e-10f; // 2^-32; 0xFFFFFF80 and above round to 2^32: 1.0
}

// cos and sin of 2 pi u for u in [0, 1]: the quadrant k = rint(4u) (ties to even), f = 4u - k in [-1/2, 1/2] (both exact),
// x = f * float(pi / 2), Taylor polynomials to x^10 / x^11 in Horner form with separate multiplies and adds, then the quadrant's
// swap and signs.  The same operations as messyerraytracer_amd/hemisphere.py: bit-identical on both sides.
__device__ __forceinline__ void sincos_2pi(float u, float &cs, float &sn)
{
	const float a = u * 4.0f, k = __builtin_rintf(a), f = a - k;
	const float x = f * 1.5707964e+00f, x2 = x * x;
	float s = -2.5052108e-08f;
	s = s * x2 + 2.7557319e-06f; s = s * x2 + -1.984127e-04f; s = s * x2 + 8.333334e-03f; s = s * x2 + -1.6666667e-01f;
	s = x + (x * x2) * s;
	float c = -2.755732e-07f;
	c = c * x2 + 2.4801588e-05f; c = c * x2 + -1.3888889e-03f; c = c * x2 + 4.1666668e-02f; c = c * x2 + -5.0e-01f;
	c = 1.0f + x2 * c;
	const uint32_t q = (uint32_t)(int32_t)k & 3u;
	cs = q == 0u ? c : q == 1u ? -s : q == 2u ? -c : s;
	sn = q == 0u ? s : q == 1u ? c : q == 2u ? -s : -c;
}

// Vector3::normalized: l2 = (x*x + y*y) + z*z, 0 if l2 == 0, else three divisions by sqrt(l2)
__device__ __forceinline__ void normalize3(float &x, float &y, float &z)
{
	const float l2 = (x * x + y * y) + z * z;
	if (l2 == 0.0f) { x = y = z = 0.0f; }
	else { const float l = __builtin_sqrtf(l2); x /= l; y /= l; z /= l; }
}

// The local direction (rr * cos, rr * sin, z) at angle 2 pi u2 taken through the orthonormal basis of n and normalised:
//   (cs, sn) = sincos_2pi(u2), x = rr * cs, y = rr * sn
//   construct_onb(n): sign = copysign(1, nz), a = -1 / (sign + nz), b = (nx * ny) * a,
//       t = (1 + ((sign * nx) * nx) * a, sign * b, (-sign) * nx), bt = (b, sign + (ny * ny) * a, -ny)
//   v = normalized((t * x + bt * y) + n * z) per component
// (rr, z) = (sqrt(u1), sqrt(max(0, 1 - u1))) is the cosine-weighted hemisphere sample, (sin, cos) of a GGX half vector's polar angle that vector.
__device__ __forceinline__ void onb_direction(const Surface &sf, float rr, float z, float u2, float &vx, float &vy, float &vz)
{
	const float nx = sf.nx, ny = sf.ny, nz = sf.nz;
	float cs, sn;
	sincos_2pi(u2, cs, sn);
	const float x = rr * cs, y = rr * sn;
	const float sign = __builtin_copysignf(1.0f, nz);
	const float a = -1.0f / (sign + nz), b = (nx * ny) * a;
	const float tx = 1.0f + ((sign * nx) * nx) * a, ty = sign * b, tz = (-sign) * nx;
	const float bx = b, by = sign + (ny * ny) * a, bz = -ny;
	vx = (tx * x + bx * y) + nx * z; vy = (ty * x + by * y) + ny * z; vz = (tz * x + bz * y) + nz * z;
	normalize3(vx, vy, vz);
}

// PathTrace::sample_bounce's draw (bounce_kernel.h states the operations) at a surface whose normal faces the incoming ray: the lobe,
// the direction v, n . v (<= 0: below the surface, an invalid sample), and what the renderer's weights need besides -- the specular
// probability sp, a2 = roughness^4 and, of the specular lobe, the half vector h and vh (a diffuse sample: h = v, vh = 0).  state
// enters as the generator's state of the first draw and leaves as that of the third: the next draw (the roulette's) follows from it.
struct BounceSample { bool specular; float vx, vy, vz, ndl, hx, hy, hz, vh, sp, a2; };
__device__ __forceinline__ BounceSample sample_bounce(const Surface &sf, float metallic, float roughness, uint32_t &state)
{
	BounceSample b;
	const float m = fminf(fmaxf(metallic, 0.0f), 1.0f), ro = fminf(fmaxf(roughness, 0.04f), 1.0f);
	b.sp = m + ((1.0f - m) * (1.0f - ro)) * 0.5f;
	b.sp = fmaxf(fminf(b.sp, 0.95f), 0.05f);
	const float u0 = pcg_float(state);
	state = state * kPcgMul + kPcgInc;
	const float u1 = pcg_float(state);
	state = state * kPcgMul + kPcgInc;
	const float u2 = pcg_float(state);
	b.specular = u0 < b.sp;
	const float a = ro * ro, a2 = a * a;
	b.a2 = a2;
	// the local direction before the basis: the half vector's (specular) or the ray's (diffuse)
	float rr, z;
	if (b.specular) {
		z = __builtin_sqrtf((1.0f - u1) / ((1.0f + (a2 - 1.0f) * u1) + 1e-7f));
		rr = __builtin_sqrtf(fmaxf(0.0f, 1.0f - z * z));
	} else {
		rr = __builtin_sqrtf(u1); z = __builtin_sqrtf(fmaxf(0.0f, 1.0f - u1));
	}
	onb_direction(sf, rr, z, u2, b.vx, b.vy, b.vz);
	b.hx = b.vx; b.hy = b.vy; b.hz = b.vz; b.vh = 0.0f;
	if (b.specular) { // v is the half vector: the view direction reflected about it
		float wx = -sf.dx, wy = -sf.dy, wz = -sf.dz;
		normalize3(wx, wy, wz);
		b.vh = fmaxf((wx * b.vx + wy * b.vy) + wz * b.vz, 0.0f);
		const float k = 2.0f * b.vh;
		b.vx = b.vx * k - wx; b.vy = b.vy * k - wy; b.vz = b.vz * k - wz;
		normalize3(b.vx, b.vy, b.vz);
	}
	b.ndl = (sf.nx * b.vx + sf.ny * b.vy) + sf.nz * b.vz;
	return b;
}
