// denoise_kernel.h — the kernels of the reflection effect's image passes (include/mrt_hip.h: mrt_denoise_spatial, mrt_denoise_temporal,
// mrt_composite_reflections, mrt_resolve_reflections, mrt_reflection_guides), after rt_denoise_spatial.comp.glsl,
// rt_denoise_temporal.comp.glsl and rt_composite.comp.glsl of the reference.  Included by shade_kernels.hip inside namespace mrt.  Every
// per-pixel rule is denoise.h's, shared with the host: nothing is restated here.
//
// denoise_kernel: one 16 x 16 workgroup per tile of the image, one thread per pixel.  The (16 + 2 r)^2 texels the tile's taps reach
// are read once (clamped to the edge while the tile is filled), their normals decoded once, and kept in LDS as eight planes
// {r, g, b, a, depth, nx, ny, nz} of (16 + 2 r)^2 floats (18 KB at r = 4: eight workgroups a CU); a row of 16 lanes reads consecutive
// dwords of a plane.  The plain form (every tap fetched and decoded by its pixel through L1 / L2, the same tap order and bits) was
// measured 1.24x to 1.26x slower at r = 2 and r = 4 and is not kept.  No scratch, 44 VGPRs.  FUSED: the filtered pixel stays in registers, goes through the temporal rule against the pixel's own history (updated in place)
// and is blended into the pixel's own colour; only the raw reflection and the guides are read across pixels, and neither is written.
// temporal_kernel, composite_kernel and guides_kernel are streams: one thread per pixel, 256 per workgroup, 16-byte loads and stores.
#pragma once

constexpr int DN_TILE = 16, DN_TILE_MAX = DN_TILE + 8;

struct TileFetch {
	const float *tile; // eight planes of DN_TILE_MAX^2
	int stride, at;    // the tile's row length; the centre's index
	__device__ __forceinline__ dn::Texel operator()(int dx, int dy) const
	{
		const float *p = tile + (at + dy * stride + dx);
		constexpr int P = DN_TILE_MAX * DN_TILE_MAX;
		dn::Texel t;
		t.c.x = p[0]; t.c.y = p[P]; t.c.z = p[2 * P]; t.c.w = p[3 * P];
		t.d = p[4 * P]; t.nx = p[5 * P]; t.ny = p[6 * P]; t.nz = p[7 * P];
		return t;
	}
};

template <bool FUSED>
__global__ __launch_bounds__(DN_TILE * DN_TILE) void denoise_kernel(const dn::DenoiseArgs a, uint32_t tiles_x, const dn::Px4 *reflection,
		const float *depth, const dn::Px4 *guide, dn::Px4 *history, dn::Px4 *color, dn::Px4 *out)
{
	const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
	const int lx = threadIdx.x & (DN_TILE - 1), ly = threadIdx.x / DN_TILE;
	const uint32_t x = tile_x * DN_TILE + lx, y = tile_y * DN_TILE + ly;
	const bool inside = x < a.w && y < a.h;
	// the w_spatial table into LDS: constant indices into the kernel's arguments (scalar loads; a dynamic index would put the whole
	// block into scratch), one lane keeps each, and every tap then reads its weight as an LDS broadcast
	__shared__ float wsp[81];
	{
		float mine = 0.0f;
#pragma unroll
		for (int k = 0; k < 81; k++)
			if ((int)threadIdx.x == k) mine = a.w_spatial[k];
		if (threadIdx.x < 81) wsp[threadIdx.x] = mine;
	}
	__shared__ float tile[8 * DN_TILE_MAX * DN_TILE_MAX];
	constexpr int P = DN_TILE_MAX * DN_TILE_MAX;
	const int r = a.radius, stride = DN_TILE + 2 * r;
	// the tile's first texel; taps are clamped
	const dn::GlobalFetch global = {reflection, depth, guide, a.w, a.h, a.normal_kind, (int64_t)tile_x * DN_TILE - r, (int64_t)tile_y * DN_TILE - r};
	for (int k = threadIdx.x; k < stride * stride; k += DN_TILE * DN_TILE) {
		const int ty = k / stride, tx = k - ty * stride;
		const dn::Texel t = global(tx, ty);
		tile[k] = t.c.x; tile[P + k] = t.c.y; tile[2 * P + k] = t.c.z; tile[3 * P + k] = t.c.w;
		tile[4 * P + k] = t.d; tile[5 * P + k] = t.nx; tile[6 * P + k] = t.ny; tile[7 * P + k] = t.nz;
	}
	__syncthreads();
	if (!inside) return;
	const dn::Px4 den = dn::spatial_pixel(a, wsp, TileFetch{tile, stride, (ly + r) * stride + (lx + r)});
	const uint64_t i = (uint64_t)y * a.w + x;
	if (out != nullptr) out[i] = den;
	if constexpr (FUSED) {
		dn::Px4 hist = {0.0f, 0.0f, 0.0f, 0.0f};
		if (a.has_history) hist = history[i];
		const dn::Px4 t = dn::temporal_pixel(a, den, hist);
		history[i] = t;
		const float d = depth[i];
		if (t.w <= 0.001f || d >= 1.0f) return; // (composite_pixel's own test, before the colour is fetched)
		dn::Px4 c = color[i];
		if (dn::composite_pixel(a, x, y, t, d, guide[i], c)) color[i] = c;
	}
}

__global__ __launch_bounds__(MRT_WG) void temporal_kernel(const dn::DenoiseArgs a, uint64_t count, const dn::Px4 *current, const dn::Px4 *history,
		dn::Px4 *out)
{
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= count) return;
	dn::Px4 hist = {0.0f, 0.0f, 0.0f, 0.0f};
	if (a.has_history) hist = history[i];
	out[i] = dn::temporal_pixel(a, current[i], hist);
}

__global__ __launch_bounds__(MRT_WG) void composite_kernel(const dn::DenoiseArgs a, uint64_t count, const dn::Px4 *reflection, const float *depth,
		const dn::Px4 *guide, dn::Px4 *color)
{
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= count) return;
	const dn::Px4 refl = reflection[i];
	const float d = depth[i];
	if (refl.w <= 0.001f || d >= 1.0f) return;
	const uint64_t y = i / a.w;
	dn::Px4 c = color[i];
	if (dn::composite_pixel(a, (uint32_t)(i - y * a.w), (uint32_t)y, refl, d, guide[i], c)) color[i] = c;
}

__global__ __launch_bounds__(MRT_WG) void guides_kernel(const mrt_hit32 *hits, const mrt_surface64 *rows, uint64_t count, float inv_depth_range,
		float *depth, dn::Px4 *guide)
{
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= count) return;
	float d;
	dn::Px4 g;
	dn::guide_texels(hits[i], rows[i], inv_depth_range, d, g);
	depth[i] = d;
	guide[i] = g;
}
