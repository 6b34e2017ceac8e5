// channel_kernel.h — the renderer's channels from hit records (mrt_shade_channels / mrt_shade_grid_channels): the ten channels of
// RayImage besides COLOR as ShadePass's per-channel functions write them (src/modules/graphics/shade_pass.h:337-395, :732-884), as
// float planes, as the bytes of RayImage::to_image (ray_image.cpp:22-35), or both.  Included by shade_kernels.hip (inside namespace
// mrt, after surface_kernel.h, whose steps it calls).
//
// One thread per record, 256 per workgroup, no LDS, no scratch.  The record and its ray are read once for all selected channels (16-byte
// loads, as the resolve's).  The selection is ChannelParams::mask and the plane pointers, kernel arguments: every test on them is a
// scalar branch over the launch, and one instantiation per source serves any subset.  The 64-byte shade row is gathered only when
// NORMAL, ALBEDO, UV or FRESNEL is selected; the binding, the tangents and the normal map's texels only for NORMAL, the material's
// first 16 bytes and the albedo texture's texels only for ALBEDO, each where the textured resolve would read them.  A float plane is
// one 16-byte store per record (a wave writes 1 KB contiguously), a byte plane one 4-byte store (256 B per wave).
// Plain float operations in the order include/mrt_hip.h states (nothing is contracted).  The record's words, in_range, the row, uv, uv_ok, the smooth
// normal, the binding, the perturbed normal and the albedo are the resolve's own steps, called (surface_kernel.h, surface_tex_kernel.h).
// With no texture set resident t is all zero: no binding applies, and the normal and the albedo are the plain resolve's.
#pragma once

// one record of plane k: {r, g, b, 1}, and / or its bytes
__device__ __forceinline__ void store_channel(const ChannelParams &s, int k, uint64_t i, float r, float g, float b)
{
	if (s.rgba[k] != nullptr) reinterpret_cast<float4 *>(s.rgba[k])[i] = make_float4(r, g, b, 1.0f);
	if (s.rgba8[k] != nullptr)
		reinterpret_cast<uint32_t *>(s.rgba8[k])[i] = to_rgba8(r) | (to_rgba8(g) << 8) | (to_rgba8(b) << 16) | (to_rgba8(1.0f) << 24);
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void shade_channels_kernel(const TraceParams p, const ChannelParams s, const TextureParams t)
{
	constexpr bool HOST = SRC == SURF_HOST;
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= p.count) return;
	Surface sf = {};
	const bool hit = record_surface<HOST, SRC == SURF_GRID>(p, s.records, i, sf);
	if (!hit) {
#pragma unroll
		for (int k = MRT_CHANNEL_NORMAL; k < MRT_CHANNEL_COUNT; k++)
			if (s.mask & (1u << k)) store_channel(s, k, i, 0.0f, 0.0f, 0.0f);
		return;
	}
	const RecordWords rec = record_words<HOST>(s.records, i);
	const float tt = rec.t, u = rec.u, v = rec.v, w = (1.0f - u) - v;
	const uint32_t prim = rec.prim;

	if (s.mask & (1u << MRT_CHANNEL_DEPTH)) {
		float x = 1.0f - tt * s.inv_depth_range;
		x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
		store_channel(s, MRT_CHANNEL_DEPTH, i, x, x, x);
	}
	if (s.mask & (1u << MRT_CHANNEL_BARYCENTRIC)) store_channel(s, MRT_CHANNEL_BARYCENTRIC, i, u, v, w);
	if (s.mask & (1u << MRT_CHANNEL_POSITION)) {
		float fx = sf.px * s.inv_pos_range, fy = sf.py * s.inv_pos_range, fz = sf.pz * s.inv_pos_range;
		fx = fx - floorf(fx); fy = fy - floorf(fy); fz = fz - floorf(fz);
		store_channel(s, MRT_CHANNEL_POSITION, i, fx, fy, fz);
	}
	if (s.mask & (1u << MRT_CHANNEL_PRIM_ID)) {
		uint32_t h = prim;
		h = ((h >> 16) ^ h) * 0x45d9f3bu;
		h = ((h >> 16) ^ h) * 0x45d9f3bu;
		h = (h >> 16) ^ h;
		store_channel(s, MRT_CHANNEL_PRIM_ID, i, (float)(h & 255u) / 255.0f, (float)((h >> 8) & 255u) / 255.0f, (float)((h >> 16) & 255u) / 255.0f);
	}
	if (s.mask & (1u << MRT_CHANNEL_HIT_MASK)) store_channel(s, MRT_CHANNEL_HIT_MASK, i, 1.0f, 1.0f, 1.0f);
	if (s.mask & (1u << MRT_CHANNEL_WIREFRAME)) {
		float m = w;
		if (u < m) m = u;
		if (v < m) m = v;
		float e = (m - 0.01f) / (0.03f - 0.01f);
		e = e < 0.0f ? 0.0f : (e > 1.0f ? 1.0f : e);
		e = 1.0f - (e * e) * (3.0f - 2.0f * e);
		const float x = 0.08f + e * (1.0f - 0.08f);
		store_channel(s, MRT_CHANNEL_WIREFRAME, i, x, x, x);
	}
	if (!(s.mask & CHANNELS_ROW)) return;

	// the channels that read the shade row
	float uvx = 0.0f, uvy = 0.0f;
	float nx = sf.nx, ny = sf.ny, nz = sf.nz; // the record's normal, then the smooth normal, then (NORMAL) the perturbed one
	const ShadeRow row = load_shade_row(s, prim);
	const bool uv_ok = shade_uv(s, row, u, v, w, uvx, uvy);
	if (s.mask & (1u << MRT_CHANNEL_UV)) {
		float r = 0.5f, g = 0.5f;
		if (row.in_range && (s.present & SHADE_HAS_UVS)) { r = uvx - floorf(uvx); g = uvy - floorf(uvy); }
		store_channel(s, MRT_CHANNEL_UV, i, r, g, 0.0f);
	}
	smooth_normal(s, row, u, v, w, nx, ny, nz);
	if (s.mask & (1u << MRT_CHANNEL_FRESNEL)) {
		float q = (nx * -sf.dx + ny * -sf.dy) + nz * -sf.dz;
		q = q < 0.0f ? 0.0f : (q > 1.0f ? 1.0f : q);
		store_channel(s, MRT_CHANNEL_FRESNEL, i, q, q, 0.3f + q * 0.7f);
	}
	if (!(s.mask & CHANNELS_MATERIAL)) return;

	const Binding b = material_binding<true>(s, t, row);
	if (s.mask & (1u << MRT_CHANNEL_NORMAL)) {
		perturb_normal(t, b.normal_tex, b.normal_scale, prim, uv_ok, u, v, w, uvx, uvy, nx, ny, nz);
		store_channel(s, MRT_CHANNEL_NORMAL, i, nx * 0.5f + 0.5f, ny * 0.5f + 0.5f, nz * 0.5f + 0.5f);
	}
	if (s.mask & (1u << MRT_CHANNEL_ALBEDO)) {
		float4 a = {0.75f, 0.75f, 0.75f, 0.0f};
		if (b.material) a = material_albedo<true>(s, t, b, uv_ok, uvx, uvy);
		store_channel(s, MRT_CHANNEL_ALBEDO, i, a.x, a.y, a.z);
	}
}
