// svgf_kernel.h — the kernels of the SVGF pass chain (include/mrt_hip.h: mrt_svgf_guides, mrt_svgf_temporal, mrt_svgf_variance,
// mrt_svgf_atrous, mrt_svgf_modulate; mrt_svgf_frame queues them and has none of its own).  Included by shade_kernels.hip inside
// namespace mrt, after path_frame_kernel.h, whose pack_rgba8 the modulate pass calls.  Every per-pixel rule is svgf.h's, shared with
// the host: nothing is restated here.
//
// svgf_guides_kernel, svgf_temporal_kernel and svgf_modulate_kernel are streams: one thread per pixel, 256 per workgroup, 16-byte loads
// and stores (the guides read a record's 32-byte ray and hit as two and its 64-byte row as the two 16-byte words they use; KIND, an
// MRT_ACCUM_SRC_*, is a template argument as in accum_kernel.h).  The temporal pass adds four gathered 16-byte reads per previous
// image for a pixel with a reprojection inside the frame.
// svgf_variance_kernel and svgf_atrous_kernel read neighbours.  Both are the plain form: one 16 x 16 workgroup per tile of the image,
// one thread per pixel, every pixel fetching its own taps through L1 / L2 (at most 48 taps of three images; 24 of three images and a
// 3 x 3 of one).  A form that stages the tile's footprint in LDS has not been written or measured.  No LDS, no scratch.
#pragma once

constexpr int SV_TILE = 16;

template <int KIND>
__global__ __launch_bounds__(MRT_WG) void svgf_guides_kernel(const mrt_ray32 *rays, const mrt_hit32 *hits, const mrt_surface64 *rows,
		const void *source, uint64_t count, sv::Px4 *illum, sv::Px4 *albedo, sv::Px4 *normal_depth, sv::Px4 *position)
{
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= count) return;
	const float4 *rq = reinterpret_cast<const float4 *>(rays) + i * 2u, *hq = reinterpret_cast<const float4 *>(hits) + i * 2u;
	const float4 *wq = reinterpret_cast<const float4 *>(rows) + i * 4u;
	const float4 r0 = rq[0], r1 = rq[1], h0 = hq[0], w0 = wq[0], w1 = wq[1];
	const float4 s = KIND == MRT_ACCUM_SRC_PATH_STATE ? (reinterpret_cast<const float4 *>(source) + i * 2u)[1] : reinterpret_cast<const float4 *>(source)[i];
	mrt_ray32 ray;
	ray.origin[0] = r0.x; ray.origin[1] = r0.y; ray.origin[2] = r0.z; ray.t_max = r0.w;
	ray.direction[0] = r1.x; ray.direction[1] = r1.y; ray.direction[2] = r1.z; ray.t_min = r1.w;
	mrt_hit32 hit = {};
	hit.t = h0.x; hit.prim_id = __float_as_int(h0.y);
	mrt_surface64 row = {};
	row.normal[0] = w0.x; row.normal[1] = w0.y; row.normal[2] = w0.z;
	row.albedo[0] = w1.x; row.albedo[1] = w1.y; row.albedo[2] = w1.z;
	sv::Px4 il, al, nd, po;
	sv::guides_pixel(ray, hit, row, sv::Px4{s.x, s.y, s.z, s.w}, il, al, nd, po);
	illum[i] = il; albedo[i] = al; normal_depth[i] = nd; position[i] = po;
}

__global__ __launch_bounds__(MRT_WG) void svgf_temporal_kernel(const sv::SvgfArgs a, uint64_t count, const sv::Px4 *illum,
		const sv::Px4 *normal_depth, const sv::Px4 *position, const sv::Images prev, sv::Px4 *out_illum, sv::Px4 *out_moments)
{
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= count) return;
	sv::Px4 o, m;
	sv::temporal_pixel(a, prev, illum[i], normal_depth[i], position[i], o, m);
	out_illum[i] = o; out_moments[i] = m;
}

template <bool ATROUS>
__global__ __launch_bounds__(SV_TILE * SV_TILE) void svgf_spatial_kernel(const sv::SvgfArgs a, uint32_t tiles_x, const sv::Images im, sv::Px4 *out)
{
	const uint32_t tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
	const uint32_t x = tile_x * SV_TILE + (threadIdx.x & (SV_TILE - 1)), y = tile_y * SV_TILE + threadIdx.x / SV_TILE;
	if (x >= a.w || y >= a.h) return;
	out[(uint64_t)y * a.w + x] = ATROUS ? sv::atrous_pixel(a, im, (int64_t)x, (int64_t)y) : sv::variance_pixel(a, im, (int64_t)x, (int64_t)y);
}

__global__ __launch_bounds__(MRT_WG) void svgf_modulate_kernel(const sv::SvgfArgs a, uint64_t count, const sv::Px4 *illum, const sv::Px4 *albedo,
		float *rgba, uint8_t *rgba8)
{
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= count) return;
	const sv::Px4 o = sv::modulate_pixel(a, illum[i], albedo[i]);
	const float4 f = make_float4(o.x, o.y, o.z, o.w);
	reinterpret_cast<float4 *>(rgba)[i] = f;
	if (rgba8 != nullptr) reinterpret_cast<uint32_t *>(rgba8)[i] = pack_rgba8(f);
}
