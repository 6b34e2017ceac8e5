// surface_kernel.h — hit records resolved to shading surfaces (mrt_resolve_surfaces / mrt_resolve_grid_surfaces), plain and with a
// texture set resident, the steps of the resolve that the channels take too, and the row packing of shade data given as device
// arrays.  Included by shade_kernels.hip (inside namespace mrt, after source_common.h and surface_tex_kernel.h, whose sampler and
// perturb_normal the textured steps call).
//
// ShadePass::extract_surface of the reference (src/modules/graphics/shade_pass.h:509-587) without F0 and the diffuse albedo, against
// the SceneShadeData the context holds (shade_data.h).  One thread per record, nothing walked: a streaming
// gather -- the record and its ray as 16-byte loads, one 64-byte shade row and one 48-byte material as 16-byte loads, one 64-byte row
// out as four 16-byte stores (a wave writes 4 KB contiguously).  Plain float operations in this order (nothing is contracted):
//   hit, d   as record_surface gives them (source_common.h); u, v, prim_id from the record
//   in_range = prim_id < n_tris (unsigned); w = (1 - u) - v
//   n  = normals resident and in_range: normalized((n0 * w + n1 * u) + n2 * v) per component (TriangleNormals::interpolate);
//        otherwise the record's normal as it stands
//   vd = normalized(-d), ndv = (nx*vdx + ny*vdy) + nz*vdz, n_dot_v = ndv < 0.001f ? 0.001f : ndv
//   material: the defaults (0.75 x3, 0, 0.5, 0.5, emission 0, 0xFFFFFFFF); ids resident, in_range and id < n_materials: albedo,
//        metallic, specular copied, roughness = mat.roughness < 0.04f ? 0.04f : mat.roughness, emission = mat.emission *
//        mat.emission_energy if emission_energy > 0 else 0, material = id
//   uv = uvs resident and in_range: (uv0 * w + uv1 * u) + uv2 * v per component; else 0
// A miss: an all-zero row with material 0xFFFFFFFF, {0, 0.5} for the bounce pair, the record unchanged.
// The three outputs are optional, each behind a branch on a kernel argument (uniform over the launch); no LDS, no scratch.
// With a texture set (TEX) the binding, the normal map and the albedo texture as surface_tex_kernel.h states them.
#pragma once

// Rows of shade data whose per-triangle arrays are device arrays: one thread per triangle (once per upload: not a hot path).
__global__ __launch_bounds__(MRT_WG) void pack_shade_rows_kernel(const uint32_t *ids, const float *normals9, const float *uvs6,
		uint32_t n_tris, uint4 *rows)
{
	const uint64_t t = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (t >= n_tris) return;
	uint32_t w[16];
	pack_shade_row(ids, normals9, uvs6, t, w);
	uint4 *o = rows + t * 4u;
#pragma unroll
	for (int k = 0; k < 4; k++) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// ---- the steps: P is SurfaceParams or ChannelParams (shade_rows, materials, n_tris, n_materials, present) ------------------------
// The record's own words (record_surface made the same loads: the compiler keeps one of each).
struct RecordWords { float t, u, v; uint32_t prim; };
template <bool HOST>
__device__ __forceinline__ RecordWords record_words(const void *records, uint64_t i)
{
	RecordWords r;
	if (HOST) {
		const float *h = reinterpret_cast<const float *>(records) + i * 11u;
		r.t = h[0]; r.u = h[7]; r.v = h[8]; r.prim = reinterpret_cast<const uint32_t *>(h)[9];
	} else {
		const float4 ra = (reinterpret_cast<const float4 *>(records) + i * 2u)[0];
		r.t = ra.x; r.prim = __float_as_uint(ra.y); r.u = ra.z; r.v = ra.w;
	}
	return r;
}

// in_range and the 64-byte shade row of a primitive (all zero where it is not read)
struct ShadeRow { bool in_range; float4 t0, t1, t2, t3; };
template <class P>
__device__ __forceinline__ ShadeRow load_shade_row(const P &s, uint32_t prim)
{
	ShadeRow r = {};
	r.in_range = prim < s.n_tris;
	if (r.in_range && s.present != 0u) {
		const float4 *row = reinterpret_cast<const float4 *>(s.shade_rows) + (size_t)prim * 4u;
		r.t0 = row[0]; r.t1 = row[1]; r.t2 = row[2]; r.t3 = row[3];
	}
	return r;
}

// uv (left as it is where no UVs apply); returns uv_ok: a texture may be sampled there
template <class P>
__device__ __forceinline__ bool shade_uv(const P &s, const ShadeRow &r, float u, float v, float w, float &uvx, float &uvy)
{
	if (!(r.in_range && (s.present & SHADE_HAS_UVS))) return false;
	uvx = (r.t1.w * w + r.t3.x * u) + r.t3.z * v;
	uvy = (r.t2.w * w + r.t3.y * u) + r.t3.w * v;
	return fabsf(uvx) < __builtin_inff() && fabsf(uvy) < __builtin_inff(); // (false for a NaN)
}

// the smooth normal in place of the record's, where normals apply
template <class P>
__device__ __forceinline__ void smooth_normal(const P &s, const ShadeRow &r, float u, float v, float w, float &nx, float &ny, float &nz)
{
	if (!(r.in_range && (s.present & SHADE_HAS_NORMALS))) return;
	nx = (r.t0.x * w + r.t1.x * u) + r.t2.x * v;
	ny = (r.t0.y * w + r.t1.y * u) + r.t2.y * v;
	nz = (r.t0.z * w + r.t1.z * u) + r.t2.z * v;
	normalize3(nx, ny, nz);
}

// the primitive's material, if it has one, and (TEX) that material's texture binding
struct Binding { bool material; uint32_t id, albedo_tex, normal_tex; float normal_scale; };
template <bool TEX, class P>
__device__ __forceinline__ Binding material_binding(const P &s, const TextureParams &t, const ShadeRow &r)
{
	Binding b = {false, __float_as_uint(r.t0.w), MRT_NO_TEXTURE, MRT_NO_TEXTURE, 0.0f};
	b.material = r.in_range && (s.present & SHADE_HAS_IDS) && b.id < s.n_materials;
	if constexpr (TEX) {
		if (b.material && b.id < t.n_bindings) {
			const uint4 w = reinterpret_cast<const uint4 *>(t.bindings)[b.id];
			b.albedo_tex = w.x; b.normal_tex = w.y; b.normal_scale = __uint_as_float(w.z);
		}
	}
	return b;
}

// {albedo, metallic} of a material, the albedo times its texture's sample where one applies
template <bool TEX, class P>
__device__ __forceinline__ float4 material_albedo(const P &s, const TextureParams &t, const Binding &b, bool uv_ok, float uvx, float uvy)
{
	float4 m0 = (reinterpret_cast<const float4 *>(s.materials) + (size_t)b.id * 3u)[0];
	if constexpr (TEX) {
		if (b.albedo_tex != MRT_NO_TEXTURE && uv_ok) {
			float cr, cg, cb;
			sample_bilinear(t, b.albedo_tex, uvx, uvy, cr, cg, cb);
			m0.x = m0.x * cr; m0.y = m0.y * cg; m0.z = m0.z * cb;
		}
	}
	return m0;
}

// ---- the resolve of record i: TEX = a texture set is resident (t is read only then) ------------------------------------------------
template <int SRC, bool TEX>
__device__ __forceinline__ void resolve_record(const TraceParams &p, const SurfaceParams &s, const TextureParams &t)
{
	constexpr bool HOST = SRC == SURF_HOST;
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= p.count) return;
	Surface sf = {};
	const bool hit = record_surface<HOST, SRC == SURF_GRID>(p, s.records, i, sf);
	const float *h = reinterpret_cast<const float *>(s.records) + i * 11u; // HOST: the record, for out_hits
	float4 ra = {}, rb = {};                                                // otherwise
	if (!HOST) { const float4 *q = reinterpret_cast<const float4 *>(s.records) + i * 2u; ra = q[0]; rb = q[1]; }
	const RecordWords rec = record_words<HOST>(s.records, i);
	const float u = rec.u, v = rec.v;

	float4 o0 = {0.0f, 0.0f, 0.0f, 0.0f}, o1 = o0, o2 = o0, o3 = {0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu)};
	float metallic = 0.0f, roughness = 0.5f; // (a miss's bounce pair)
	float nx = sf.nx, ny = sf.ny, nz = sf.nz;
	if (hit) {
		const ShadeRow row = load_shade_row(s, rec.prim);
		const float w = (1.0f - u) - v;
		float uvx = 0.0f, uvy = 0.0f;
		const bool uv_ok = shade_uv(s, row, u, v, w, uvx, uvy);
		o3.x = uvx; o3.y = uvy;
		smooth_normal(s, row, u, v, w, nx, ny, nz);
		const Binding b = material_binding<TEX>(s, t, row);
		if constexpr (TEX) perturb_normal(t, b.normal_tex, b.normal_scale, rec.prim, uv_ok, u, v, w, uvx, uvy, nx, ny, nz);
		float vx = -sf.dx, vy = -sf.dy, vz = -sf.dz;
		normalize3(vx, vy, vz);
		const float ndv = (nx * vx + ny * vy) + nz * vz;
		o0.x = nx; o0.y = ny; o0.z = nz; o0.w = ndv < 0.001f ? 0.001f : ndv;
		o1.x = 0.75f; o1.y = 0.75f; o1.z = 0.75f; o1.w = 0.0f;
		o2.w = 0.5f; o3.z = 0.5f;
		if (b.material) {
			const float4 *m = reinterpret_cast<const float4 *>(s.materials) + (size_t)b.id * 3u;
			const float4 m1 = m[1], m2 = m[2]; // {albedo, metallic | roughness, specular, emission rg | emission b, energy, flags, -}
			o2.w = m1.x < 0.04f ? 0.04f : m1.x;
			o3.z = m1.y;
			o1 = material_albedo<TEX>(s, t, b, uv_ok, uvx, uvy); // (after the two words above: before them the row's stores come out split)
			if (m2.y > 0.0f) { o2.x = m1.z * m2.y; o2.y = m1.w * m2.y; o2.z = m2.x * m2.y; }
			o3.w = __uint_as_float(b.id);
		}
		metallic = o1.w; roughness = o2.w;
	}
	if (s.out_rows != nullptr) {
		float4 *o = reinterpret_cast<float4 *>(s.out_rows) + i * 4u;
		o[0] = o0; o[1] = o1; o[2] = o2; o[3] = o3;
	}
	if (s.out_bounce != nullptr) reinterpret_cast<float2 *>(s.out_bounce)[i] = make_float2(metallic, roughness);
	if (s.out_hits != nullptr) {
		if (HOST) {
			float *d = reinterpret_cast<float *>(s.out_hits) + i * 11u;
			float r[11];
#pragma unroll
			for (int k = 0; k < 11; k++) r[k] = h[k];
			if (hit) { r[4] = nx; r[5] = ny; r[6] = nz; }
#pragma unroll
			for (int k = 0; k < 11; k++) d[k] = r[k];
		} else {
			float4 *d = reinterpret_cast<float4 *>(s.out_hits) + i * 2u;
			if (hit) { rb.x = nx; rb.y = ny; rb.z = nz; }
			d[0] = ra; d[1] = rb;
		}
	}
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void resolve_surfaces_kernel(const TraceParams p, const SurfaceParams s)
{
	resolve_record<SRC, false>(p, s, TextureParams{});
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void resolve_textured_surfaces_kernel(const TraceParams p, const SurfaceParams s, const TextureParams t)
{
	resolve_record<SRC, true>(p, s, t);
}
