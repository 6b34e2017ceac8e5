// path.hip — the path tracer's per-pixel state on the device (include/mrt_hip.h: mrt_path_init, mrt_path_step, mrt_path_grid_step,
// mrt_path_finish, and the steps of a loop that samples emitters, mrt_path_step_emitters and mrt_path_grid_step_emitters).  The refusals and the kernel's copy of a descriptor are host/path_data.cpp; the kernels are path_kernel.h
// (shade_kernels.hip).
#include <cstring>
#include <hip/hip_runtime.h>
#include "mrt_context.h"
#include "path.h"
#include "panorama.h"
#include "emitters.h"

namespace {

// The steps after their own checks: p holds the incoming rays (or the grid) and the count; pixel0 = the pixel index of record 0.
// emitters: the step of a loop that samples emitters, with the lobe bytes of the step before (null at bounce 0 alone).
int step(mrt_ctx *ctx, int src, mrt::TraceParams &p, const void *d_hits, const mrt_surface64 *d_rows, uint32_t pixel0,
		const mrt_path_step_desc *desc, uint32_t flags, bool emitters = false, const uint8_t *d_prev_lobe = nullptr)
{
	BEGIN_PASS(ctx, p.count);
	mrt::PathParams s;
	std::memset(&s, 0, sizeof(s));
	s.records = d_hits; s.rows = d_rows;
	mrt::fill_path_params(desc, pixel0, s);
	const mrt::PanoramaParams pano = panorama_params(ctx);
	if (emitters) HIP_TRY(ctx, mrt::launch_path_step_emitters(p, s, ctx->pano_resident ? &pano : nullptr, d_prev_lobe, src, ctx->stream));
	else HIP_TRY(ctx, mrt::launch_path_step(p, s, ctx->pano_resident ? &pano : nullptr, src, ctx->stream));
	return finish_call(ctx, flags);
}

} // namespace

extern "C" {

int mrt_path_init(mrt_ctx *ctx, mrt_path_state *d_state, uint64_t count, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::path_frame_invalid(d_state, nullptr, false, flags, 0u)) return fail(ctx, MRT_ERR_INVALID, why);
	BEGIN_PASS(ctx, count);
	HIP_TRY(ctx, mrt::launch_path_init(d_state, count, ctx->stream));
	return finish_call(ctx, flags);
}

int mrt_path_step(mrt_ctx *ctx, const void *d_rays, const void *d_hits, const mrt_surface64 *d_rows, uint64_t count,
		const mrt_path_step_desc *desc, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::path_step_invalid(d_rays, d_hits, d_rows, desc, flags, MRT_FLAG_HOST_LAYOUT | MRT_FLAG_ASYNC))
		return fail(ctx, MRT_ERR_INVALID, why);
	mrt::TraceParams p;
	const int src = record_params(d_rays, count, flags, p);
	return step(ctx, src, p, d_hits, d_rows, 0u, desc, flags);
}

int mrt_path_grid_step(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1,
		const void *d_hits, const mrt_surface64 *d_rows, const mrt_path_step_desc *desc, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::path_step_invalid(cam, d_hits, d_rows, desc, flags, MRT_FLAG_ASYNC)) return fail(ctx, MRT_ERR_INVALID, why);
	mrt::TraceParams p;
	int rc = grid_params(ctx, cam, grid_w, grid_h, y0, y1, p);
	if (rc) return rc;
	return step(ctx, mrt::SURF_GRID, p, d_hits, d_rows, y0 * grid_w, desc, flags);
}

int mrt_path_step_emitters(mrt_ctx *ctx, const void *d_rays, const void *d_hits, const mrt_surface64 *d_rows, uint64_t count,
		const mrt_path_step_desc *desc, const uint8_t *d_prev_lobe, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	const char *why = mrt::path_step_invalid(d_rays, d_hits, d_rows, desc, flags, MRT_FLAG_HOST_LAYOUT | MRT_FLAG_ASYNC);
	if (!why) why = mrt::em::step_invalid(desc, d_prev_lobe);
	if (why) return fail(ctx, MRT_ERR_INVALID, why);
	mrt::TraceParams p;
	const int src = record_params(d_rays, count, flags, p);
	return step(ctx, src, p, d_hits, d_rows, 0u, desc, flags, true, d_prev_lobe);
}

int mrt_path_grid_step_emitters(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1,
		const void *d_hits, const mrt_surface64 *d_rows, const mrt_path_step_desc *desc, const uint8_t *d_prev_lobe, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	const char *why = mrt::path_step_invalid(cam, d_hits, d_rows, desc, flags, MRT_FLAG_ASYNC);
	if (!why) why = mrt::em::step_invalid(desc, d_prev_lobe);
	if (why) return fail(ctx, MRT_ERR_INVALID, why);
	mrt::TraceParams p;
	int rc = grid_params(ctx, cam, grid_w, grid_h, y0, y1, p);
	if (rc) return rc;
	return step(ctx, mrt::SURF_GRID, p, d_hits, d_rows, y0 * grid_w, desc, flags, true, d_prev_lobe);
}

int mrt_path_finish(mrt_ctx *ctx, const mrt_path_state *d_state, uint64_t count, uint32_t tonemap_mode, float *d_rgba, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::path_frame_invalid(d_state, d_rgba, true, flags, tonemap_mode)) return fail(ctx, MRT_ERR_INVALID, why);
	BEGIN_PASS(ctx, count);
	HIP_TRY(ctx, mrt::launch_path_finish(d_state, count, tonemap_mode, mrt::hable_partial(11.2f), d_rgba, ctx->stream));
	return finish_call(ctx, flags);
}

} // extern "C"
