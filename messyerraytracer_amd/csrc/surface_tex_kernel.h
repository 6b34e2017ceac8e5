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
// Here: the sampler and perturb_normal.  The kernel, resolve_textured_surfaces_kernel, is surface_kernel.h's resolve_record with TEX set,
// next to the steps it shares with the plain resolve and the channels.  Misses and ids out of range as surface_kernel.h; where no
// binding applies the outputs equal resolve_surfaces_kernel's byte for byte.
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

// perturb_normal where a binding's normal map applies: n is the smooth normal on entry; (u, v, w) the barycentrics, (uvx, uvy) the UV
__device__ __forceinline__ void perturb_normal(const TextureParams &t, uint32_t normal_tex, float normal_scale, uint32_t prim, bool uv_ok,
		float u, float v, float w, float uvx, float uvy, float &nx, float &ny, float &nz)
{
	if (!(normal_tex != MRT_NO_TEXTURE && t.tangents != nullptr && prim < t.n_tangent_tris && uv_ok)) return;
	const float4 *tr = reinterpret_cast<const float4 *>(t.tangents) + (size_t)prim * 3u;
	const float4 a0 = tr[0], a1 = tr[1], a2 = tr[2]; // {t0 xyz, t1.x | t1 yz, t2 xy | t2.z, sign0, sign1, sign2}
	if (!(a2.y != 0.0f || a2.z != 0.0f || a2.w != 0.0f)) return;
	float tx = (a0.x * w + a0.w * u) + a1.z * v;
	float ty = (a0.y * w + a1.x * u) + a1.w * v;
	float tz = (a0.z * w + a1.y * u) + a2.x * v;
	const float tl2 = (tx * tx + ty * ty) + tz * tz;
	if (tl2 < 1e-8f) { tx = 1.0f; ty = 0.0f; tz = 0.0f; }
	else { const float l = sqrtf(tl2); tx = tx / l; ty = ty / l; tz = tz / l; }
	const float bsign = ((a2.y * w + a2.z * u) + a2.w * v) >= 0.0f ? 1.0f : -1.0f;
	const float k = (nx * tx + ny * ty) + nz * tz;
	tx = tx - nx * k; ty = ty - ny * k; tz = tz - nz * k;
	normalize3(tx, ty, tz);
	const float bx = (ny * tz - nz * ty) * bsign, by = (nz * tx - nx * tz) * bsign, bz = (nx * ty - ny * tx) * bsign;
	float cr, cg, cb;
	sample_bilinear(t, normal_tex, uvx, uvy, cr, cg, cb);
	float sx = cr * 2.0f - 1.0f, sy = cg * 2.0f - 1.0f;
	const float sz = cb * 2.0f - 1.0f;
	sx = sx * normal_scale; sy = sy * normal_scale;
	const float px = (tx * sx + bx * sy) + nx * sz, py = (ty * sx + by * sy) + ny * sz, pz = (tz * sx + bz * sy) + nz * sz;
	const float pl2 = (px * px + py * py) + pz * pz;
	if (!(pl2 < 1e-8f)) { const float l = sqrtf(pl2); nx = px / l; ny = py / l; nz = pz / l; }
}

