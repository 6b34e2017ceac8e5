// svgf.hip — the SVGF pass chain of a path-traced frame on the device (include/mrt_hip.h: mrt_svgf_guides, mrt_svgf_temporal,
// mrt_svgf_variance, mrt_svgf_atrous, mrt_svgf_modulate, mrt_svgf_frame).  The refusals and the kernels' arguments are
// host/svgf_data.cpp and svgf.h; the kernels are svgf_kernel.h (shade_kernels.hip).  Like the other image passes, a call waits or
// queues on the context's stream, writes nothing to mrt_stats and reads no scene, tuner or schedule state.
#include <hip/hip_runtime.h>
#include "mrt_context.h"
#include "svgf.h"

namespace {

using namespace mrt::sv;

// the shared opening of the five calls with params: refusals, then the kernels' arguments
#define SVGF_BEGIN(call, step, cam, images)                                                                                 \
	if (!ctx) return MRT_ERR_INVALID;                                                                                       \
	if (const char *why = svgf_invalid(call, params, W, H, step, cam, images, flags)) return fail(ctx, MRT_ERR_INVALID, why); \
	BEGIN_PASS(ctx, (uint64_t)W * H);                                                                                       \
	SvgfArgs a;                                                                                                             \
	fill_svgf_args(params, W, H, step, cam, mrt::finish_white(), a)

} // namespace

extern "C" {

int mrt_svgf_guides(mrt_ctx *ctx, const mrt_ray32 *d_rays, const mrt_hit32 *d_hits, const mrt_surface64 *d_rows, uint32_t source_kind,
		const void *d_source, uint64_t count, float *d_illum, float *d_albedo, float *d_normal_depth, float *d_position, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = svgf_guides_invalid(d_rays, d_hits, d_rows, source_kind, d_source, count, d_illum, d_albedo, d_normal_depth, d_position, flags))
		return fail(ctx, MRT_ERR_INVALID, why);
	BEGIN_PASS(ctx, count);
	HIP_TRY(ctx, mrt::launch_svgf_guides((int)source_kind, d_rays, d_hits, d_rows, d_source, count, d_illum, d_albedo, d_normal_depth, d_position, ctx->stream));
	return finish_call(ctx, flags);
}

int mrt_svgf_temporal(mrt_ctx *ctx, const mrt_svgf_params *params, uint32_t W, uint32_t H, const float *d_illum,
		const float *d_normal_depth, const float *d_position, const mrt_camera *prev_cam, const float *d_prev_illum,
		const float *d_prev_moments, const float *d_prev_normal_depth, const float *d_prev_position, float *d_out_illum,
		float *d_out_moments, uint32_t flags)
{
	SvgfImages im = {};
	im.illum = d_illum; im.normal_depth = d_normal_depth; im.position = d_position;
	im.prev_illum = d_prev_illum; im.prev_moments = d_prev_moments; im.prev_normal_depth = d_prev_normal_depth; im.prev_position = d_prev_position;
	im.out_illum = d_out_illum; im.out_moments = d_out_moments;
	SVGF_BEGIN(SV_TEMPORAL, 0u, prev_cam, im);
	HIP_TRY(ctx, mrt::launch_svgf_temporal(a, d_illum, d_normal_depth, d_position, d_prev_illum, d_prev_moments, d_prev_normal_depth, d_prev_position,
			d_out_illum, d_out_moments, ctx->stream));
	return finish_call(ctx, flags);
}

int mrt_svgf_variance(mrt_ctx *ctx, const mrt_svgf_params *params, uint32_t W, uint32_t H, const float *d_illum, const float *d_moments,
		const float *d_normal_depth, const float *d_position, float *d_out, uint32_t flags)
{
	SvgfImages im = {};
	im.illum = d_illum; im.moments = d_moments; im.normal_depth = d_normal_depth; im.position = d_position; im.out_illum = d_out;
	SVGF_BEGIN(SV_VARIANCE, 0u, nullptr, im);
	HIP_TRY(ctx, mrt::launch_svgf_spatial(false, a, d_illum, d_moments, d_normal_depth, d_position, d_out, ctx->stream));
	return finish_call(ctx, flags);
}

int mrt_svgf_atrous(mrt_ctx *ctx, const mrt_svgf_params *params, uint32_t W, uint32_t H, uint32_t step, const float *d_illum,
		const float *d_normal_depth, const float *d_position, float *d_out, uint32_t flags)
{
	SvgfImages im = {};
	im.illum = d_illum; im.normal_depth = d_normal_depth; im.position = d_position; im.out_illum = d_out;
	SVGF_BEGIN(SV_ATROUS, step, nullptr, im);
	HIP_TRY(ctx, mrt::launch_svgf_spatial(true, a, d_illum, nullptr, d_normal_depth, d_position, d_out, ctx->stream));
	return finish_call(ctx, flags);
}

int mrt_svgf_modulate(mrt_ctx *ctx, const mrt_svgf_params *params, uint32_t W, uint32_t H, const float *d_illum, const float *d_albedo,
		float *d_rgba, uint8_t *d_rgba8, uint32_t flags)
{
	SvgfImages im = {};
	im.illum = d_illum; im.albedo = d_albedo; im.rgba = d_rgba;
	SVGF_BEGIN(SV_MODULATE, 0u, nullptr, im);
	HIP_TRY(ctx, mrt::launch_svgf_modulate(a, d_illum, d_albedo, d_rgba, d_rgba8, ctx->stream));
	return finish_call(ctx, flags);
}

int mrt_svgf_frame(mrt_ctx *ctx, const mrt_svgf_params *params, uint32_t W, uint32_t H, const float *d_illum, const float *d_albedo,
		const float *d_normal_depth, const float *d_position, const mrt_camera *prev_cam, const float *d_prev_illum,
		const float *d_prev_moments, const float *d_prev_normal_depth, const float *d_prev_position, float *d_next_illum,
		float *d_next_moments, float *d_scratch_a, float *d_scratch_b, float *d_rgba, uint8_t *d_rgba8, uint32_t flags)
{
	SvgfImages im = {};
	im.illum = d_illum; im.albedo = d_albedo; im.normal_depth = d_normal_depth; im.position = d_position;
	im.prev_illum = d_prev_illum; im.prev_moments = d_prev_moments; im.prev_normal_depth = d_prev_normal_depth; im.prev_position = d_prev_position;
	im.out_illum = d_next_illum; im.out_moments = d_next_moments; im.scratch_a = d_scratch_a; im.scratch_b = d_scratch_b; im.rgba = d_rgba;
	SVGF_BEGIN(SV_FRAME, 1u, prev_cam, im);
	HIP_TRY(ctx, mrt::launch_svgf_temporal(a, d_illum, d_normal_depth, d_position, d_prev_illum, d_prev_moments, d_prev_normal_depth, d_prev_position,
			d_scratch_a, d_next_moments, ctx->stream));
	HIP_TRY(ctx, mrt::launch_svgf_spatial(false, a, d_scratch_a, d_next_moments, d_normal_depth, d_position, d_scratch_b, ctx->stream));
	const float *in = d_scratch_b;
	float *out = d_next_illum;
	for (uint32_t k = 0; k < params->iterations; k++) {
		a.step = (int32_t)(1u << k);
		HIP_TRY(ctx, mrt::launch_svgf_spatial(true, a, in, nullptr, d_normal_depth, d_position, out, ctx->stream));
		in = out;
		out = (k & 1u) ? d_scratch_b : d_scratch_a; // after step 1: a, b, a, b
	}
	HIP_TRY(ctx, mrt::launch_svgf_modulate(a, in, d_albedo, d_rgba, d_rgba8, ctx->stream));
	return finish_call(ctx, flags);
}

} // extern "C"
