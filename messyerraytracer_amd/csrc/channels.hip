// channels.hip — the renderer's channels and its 8-bit image on the device (include/mrt_hip.h: mrt_shade_channels,
// mrt_shade_grid_channels, mrt_finish_color, mrt_image_to_rgba8).  The descriptor's checks, the selection mask and Hable's white value
// are host/channel_data.cpp; the kernels are channel_kernel.h and path_frame_kernel.h (shade_kernels.hip).  Like the resolves, the
// calls wait or queue on the context's stream, write nothing to mrt_stats and read no tuner or schedule state.
#include <cstring>
#include <hip/hip_runtime.h>
#include "mrt_context.h"
#include "channels.h"
#include "texture.h"

namespace {

// Both channel passes after their own checks: p holds the incoming rays (or the grid) and the count.
int shade(mrt_ctx *ctx, int src, mrt::TraceParams &p, const void *d_hits, const mrt_channel_out *out, uint32_t flags)
{
	BEGIN_PASS(ctx, p.count);
	mrt::ChannelParams c;
	std::memset(&c, 0, sizeof(c));
	c.records = d_hits;
	shade_data_params(ctx, c);
	mrt::fill_channel_params(out, c);
	HIP_TRY(ctx, mrt::launch_shade_channels(p, c, texture_params(ctx), src, ctx->stream));
	return finish_call(ctx, flags);
}

} // namespace

extern "C" {

int mrt_shade_channels(mrt_ctx *ctx, const void *d_rays, const void *d_hits, uint64_t count, const mrt_channel_out *out, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::channel_out_invalid(d_rays, d_hits, out, flags, MRT_FLAG_HOST_LAYOUT | MRT_FLAG_ASYNC))
		return fail(ctx, MRT_ERR_INVALID, why);
	mrt::TraceParams p;
	const int src = record_params(d_rays, count, flags, p);
	return shade(ctx, src, p, d_hits, out, flags);
}

int mrt_shade_grid_channels(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1,
		const void *d_hits, const mrt_channel_out *out, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::channel_out_invalid(cam, d_hits, out, flags, MRT_FLAG_ASYNC)) return fail(ctx, MRT_ERR_INVALID, why);
	mrt::TraceParams p;
	int rc = grid_params(ctx, cam, grid_w, grid_h, y0, y1, p);
	if (rc) return rc;
	return shade(ctx, mrt::SURF_GRID, p, d_hits, out, flags);
}

int mrt_finish_color(mrt_ctx *ctx, const float *d_lit_rgba, uint64_t count, uint32_t tonemap_mode, float *d_rgba, uint8_t *d_rgba8,
		uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::image_call_invalid(d_lit_rgba, d_rgba, d_rgba8, true, flags, tonemap_mode)) return fail(ctx, MRT_ERR_INVALID, why);
	BEGIN_PASS(ctx, count);
	HIP_TRY(ctx, mrt::launch_finish_color(d_lit_rgba, count, tonemap_mode, mrt::finish_white(), d_rgba, d_rgba8, ctx->stream));
	return finish_call(ctx, flags);
}

int mrt_image_to_rgba8(mrt_ctx *ctx, const float *d_rgba, uint64_t count, uint8_t *d_rgba8, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::image_call_invalid(d_rgba, nullptr, d_rgba8, false, flags, 0u)) return fail(ctx, MRT_ERR_INVALID, why);
	BEGIN_PASS(ctx, count);
	HIP_TRY(ctx, mrt::launch_image_to_rgba8(d_rgba, count, d_rgba8, ctx->stream));
	return finish_call(ctx, flags);
}

} // extern "C"
