// surface_kernel.h — hit records resolved to shading surfaces (mrt_resolve_surfaces / mrt_resolve_grid_surfaces), and the row packing
// of shade data given as device arrays.  Included by shade_kernels.hip (inside namespace mrt, after source_common.h).
//
// ShadePass::extract_surface of the reference (src/modules/graphics/shade_pass.h:509-587) without textures, normal maps, F0 and the
// diffuse albedo, against the SceneShadeData the context holds (shade_data.h).  One thread per record, nothing walked: a streaming
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

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void resolve_surfaces_kernel(const TraceParams p, const SurfaceParams s)
{
	constexpr bool HOST = SRC == SURF_HOST;
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= p.count) return;
	Surface sf = {};
	const bool hit = record_surface<HOST, SRC == SURF_GRID>(p, s.records, i, sf);
	// the record's own words (the loads record_surface made, once more by name: the compiler keeps one of each)
	const float *h = reinterpret_cast<const float *>(s.records) + i * 11u;                   // HOST
	const float4 *q = reinterpret_cast<const float4 *>(s.records) + i * 2u;                  // otherwise
	float4 ra = {}, rb = {};
	float u, v; uint32_t prim;
	if (HOST) { u = h[7]; v = h[8]; prim = reinterpret_cast<const uint32_t *>(h)[9]; }
	else { ra = q[0]; rb = q[1]; prim = __float_as_uint(ra.y); u = ra.z; v = ra.w; }

	float4 o0 = {0.0f, 0.0f, 0.0f, 0.0f}, o1 = o0, o2 = o0, o3 = {0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu)};
	float metallic = 0.0f, roughness = 0.5f; // (a miss's bounce pair)
	float nx = sf.nx, ny = sf.ny, nz = sf.nz;
	if (hit) {
		const bool in_range = prim < s.n_tris;
		float4 t0 = {}, t1 = {}, t2 = {}, t3 = {};
		if (in_range && s.present != 0u) {
			const float4 *row = reinterpret_cast<const float4 *>(s.shade_rows) + (size_t)prim * 4u;
			t0 = row[0]; t1 = row[1]; t2 = row[2]; t3 = row[3];
		}
		const float w = (1.0f - u) - v;
		if (in_range && (s.present & SHADE_HAS_NORMALS)) {
			nx = (t0.x * w + t1.x * u) + t2.x * v;
			ny = (t0.y * w + t1.y * u) + t2.y * v;
			nz = (t0.z * w + t1.z * u) + t2.z * v;
			normalize3(nx, ny, nz);
		}
		float vx = -sf.dx, vy = -sf.dy, vz = -sf.dz;
		normalize3(vx, vy, vz);
		const float ndv = (nx * vx + ny * vy) + nz * vz;
		o0.x = nx; o0.y = ny; o0.z = nz; o0.w = ndv < 0.001f ? 0.001f : ndv;
		o1.x = 0.75f; o1.y = 0.75f; o1.z = 0.75f; o1.w = 0.0f;
		o2.w = 0.5f; o3.z = 0.5f;
		if (in_range && (s.present & SHADE_HAS_IDS)) {
			const uint32_t id = __float_as_uint(t0.w);
			if (id < s.n_materials) {
				const float4 *m = reinterpret_cast<const float4 *>(s.materials) + (size_t)id * 3u;
				const float4 m0 = m[0], m1 = m[1], m2 = m[2]; // {albedo, metallic | roughness, specular, emission rg | emission b, energy, flags, -}
				o1 = m0;
				o2.w = m1.x < 0.04f ? 0.04f : m1.x;
				o3.z = m1.y;
				if (m2.y > 0.0f) { o2.x = m1.z * m2.y; o2.y = m1.w * m2.y; o2.z = m2.x * m2.y; }
				o3.w = __uint_as_float(id);
			}
		}
		if (in_range && (s.present & SHADE_HAS_UVS)) {
			o3.x = (t1.w * w + t3.x * u) + t3.z * v;
			o3.y = (t2.w * w + t3.y * u) + t3.w * v;
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
