// surface_tex_kernel.h — the resolve of surface_kernel.h with a texture set resident (mrt_upload_textures; texture.h): all of
// ShadePass::extract_surface (shade_pass.h:509-587) but F0 and the diffuse albedo -- the smooth normal, perturb_normal
// (shade_pass.h:110-162) over TriangleTangents (triangle_tangents.h:21-56), the material and its albedo texture through
// TextureSampler::sample_bilinear (texture_sampler.h:45-88).  Included by shade_kernels.hip (inside namespace mrt, after source_common.h).
//
// One thread per record, 256 per workgroup, no LDS, no scratch; the gather of resolve_surfaces_kernel plus, per record and only where
// a binding applies: one 16-byte binding, three 16-byte tangent loads, per sampled texture one 16-byte descriptor and four texels.
// Plain float operations in this order (nothing is contracted), with hit, d, in_range, w, n, vd, the material and uv as
// surface_kernel.h states them, uv taken first:
//   bound = ids resident, in_range, id < n_materials, id < n_bindings; b = bindings[id]
//   uv_ok = uvs resident, in_range, uv.x and uv.y finite.  A UV that is not finite would leave u - floorf(u) NaN and the texel index
//        undefined (the reference only asserts): such a record samples neither texture -- unmultiplied albedo, the smooth normal, no
//        texel read.
//   sample(tex, u, v): u = u - floorf(u); fx = u * (float)width - 0.5f; x0 = (int)floorf(fx); sx = fx - (float)x0; x1 = x0 + 1;
//        x1 = x1 >= width ? x1 - width : x1; x0 = x0 < 0 ? x0 + width : x0 (x0 is in -1 .. width - 1 before the wrap: compares and
//        selects, no integer %); the same for y; texels (x0, y0), (x1, y0), (x0, y1), (x1, y1); an RGBA8 channel = (float)byte /
//        255.0f; lerp(a, b, t) = a + (b - a) * t: top and bot by sx, then the two by sy
//   normal map: bound, b.normal_texture != none, tangents resident, prim < n_tangent_tris, any sign != 0, uv_ok -- N = n:
//        T = (t0 * w + t1 * u) + t2 * v; l2 = (x*x + y*y) + z*z; l2 < 1e-8f ? (1, 0, 0) : T / sqrt(l2)
//        bsign = ((s0 * w + s1 * u) + s2 * v) >= 0 ? 1 : -1
//        T = normalized(T - N * ((Nx*Tx + Ny*Ty) + Nz*Tz)); B = (Ny*Tz - Nz*Ty, Nz*Tx - Nx*Tz, Nx*Ty - Ny*Tx) * bsign
//        ts = sample * 2 - 1 per channel, ts.x and ts.y times b.normal_scale
//        P = (T * ts.x + B * ts.y) + N * ts.z; l2(P) < 1e-8f ? N : P / sqrt(l2)
//        n_dot_v from the result, which is the row's normal and d_out_hits' normal
//   albedo texture: bound, b.albedo_texture != none, uv_ok: albedo.c *= sample.c (no sRGB step)
// (The row gather, uv, the smooth normal, the binding and the normal map's lines are surface_tex_steps.inc, which channel_kernel.h
// includes too.)  Misses and ids out of range as surface_kernel.h; where no binding applies the outputs equal resolve_surfaces_kernel's byte for byte.
// Every texel address lies inside the pool: u - floorf(u) of a finite u is in [0, 1], so fx is in [-0.5, width - 0.5] (width <= 16384:
// exact), x0 in -1 .. width - 1, and after the wrap x0 and x1 are in 0 .. width - 1; texture indices and sizes were checked at upload.
#pragma once

// rgb of texel (x, y); alpha is never used
__device__ __forceinline__ void load_texel(const TextureParams &t, const uint4 d, int x, int y, float &r, float &g, float &b)
{
	const uint64_t idx = (uint64_t)((uint32_t)y * d.y + (uint32_t)x); // < 2^28
	const uint4 *base = reinterpret_cast<const uint4 *>(t.texels) + d.x;
	if (d.w == MRT_TEXEL_RGBA8) {
		const uint32_t px = reinterpret_cast<const uint32_t *>(base)[idx];
		r = (float)(px & 255u) / 255.0f; g = (float)((px >> 8) & 255u) / 255.0f; b = (float)((px >> 16) & 255u) / 255.0f;
	} else {
		const float4 c = reinterpret_cast<const float4 *>(base)[idx];
		r = c.x; g = c.y; b = c.z;
	}
}

__device__ __forceinline__ float lerp1(float a, float b, float t) { return a + (b - a) * t; }

// TextureSampler::sample_bilinear on texture `tex` of the table; u and v finite
__device__ __forceinline__ void sample_bilinear(const TextureParams &t, uint32_t tex, float u, float v, float &r, float &g, float &b)
{
	const uint4 d = reinterpret_cast<const uint4 *>(t.table)[tex]; // {offset16, width, height, format}
	const int w = (int)d.y, h = (int)d.z;
	u = u - floorf(u); v = v - floorf(v);
	const float fx = u * (float)w - 0.5f, fy = v * (float)h - 0.5f;
	int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
	const float sx = fx - (float)x0, sy = fy - (float)y0;
	int x1 = x0 + 1, y1 = y0 + 1;
	x1 = x1 >= w ? x1 - w : x1; y1 = y1 >= h ? y1 - h : y1;
	x0 = x0 < 0 ? x0 + w : x0; y0 = y0 < 0 ? y0 + h : y0;
	float r00, g00, b00, r10, g10, b10, r01, g01, b01, r11, g11, b11;
	load_texel(t, d, x0, y0, r00, g00, b00); load_texel(t, d, x1, y0, r10, g10, b10);
	load_texel(t, d, x0, y1, r01, g01, b01); load_texel(t, d, x1, y1, r11, g11, b11);
	r = lerp1(lerp1(r00, r10, sx), lerp1(r01, r11, sx), sy);
	g = lerp1(lerp1(g00, g10, sx), lerp1(g01, g11, sx), sy);
	b = lerp1(lerp1(b00, b10, sx), lerp1(b01, b11, sx), sy);
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void resolve_textured_surfaces_kernel(const TraceParams p, const SurfaceParams s, const TextureParams t)
{
	constexpr bool HOST = SRC == SURF_HOST;
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= p.count) return;
	Surface sf = {};
	const bool hit = record_surface<HOST, SRC == SURF_GRID>(p, s.records, i, sf);
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
		// the row, uv, the smooth normal, the binding and perturb_normal: surface_tex_steps.inc, shared with channel_kernel.h
#define MRT_TEX_STEP 1
#include "surface_tex_steps.inc"
#undef MRT_TEX_STEP
		const float w = (1.0f - u) - v;
#define MRT_TEX_STEP 2
#include "surface_tex_steps.inc"
#undef MRT_TEX_STEP
#define MRT_TEX_STEP 3
#include "surface_tex_steps.inc"
#undef MRT_TEX_STEP
#define MRT_TEX_STEP 4
#include "surface_tex_steps.inc"
#undef MRT_TEX_STEP
#define MRT_TEX_STEP 5
#include "surface_tex_steps.inc"
#undef MRT_TEX_STEP
		float vx = -sf.dx, vy = -sf.dy, vz = -sf.dz;
		normalize3(vx, vy, vz);
		const float ndv = (nx * vx + ny * vy) + nz * vz;
		o0.x = nx; o0.y = ny; o0.z = nz; o0.w = ndv < 0.001f ? 0.001f : ndv;
		o1.x = 0.75f; o1.y = 0.75f; o1.z = 0.75f; o1.w = 0.0f;
		o2.w = 0.5f; o3.z = 0.5f;
		if (material) {
			const float4 *m = reinterpret_cast<const float4 *>(s.materials) + (size_t)id * 3u;
			const float4 m0 = m[0], m1 = m[1], m2 = m[2]; // {albedo, metallic | roughness, specular, emission rg | emission b, energy, flags, -}
			o1 = m0;
			o2.w = m1.x < 0.04f ? 0.04f : m1.x;
			o3.z = m1.y;
			if (albedo_tex != MRT_NO_TEXTURE && uv_ok) {
				float cr, cg, cb;
				sample_bilinear(t, albedo_tex, o3.x, o3.y, cr, cg, cb);
				o1.x = o1.x * cr; o1.y = o1.y * cg; o1.z = o1.z * cb;
			}
			if (m2.y > 0.0f) { o2.x = m1.z * m2.y; o2.y = m1.w * m2.y; o2.z = m2.x * m2.y; }
			o3.w = __uint_as_float(id);
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
