// denoise.hip — the reflection effect's image passes on the device (include/mrt_hip.h: mrt_denoise_spatial, mrt_denoise_temporal,
// mrt_composite_reflections, mrt_resolve_reflections, mrt_reflection_guides, and mrt_reflection_image of a G-buffer cast).  The
// refusals, the clamped radius and the w_spatial table are host/denoise_data.cpp and denoise.h (the image's: host/gbuffer_data.cpp and
// gbuffer.h); the kernels are denoise_kernel.h and gbuffer_image_kernel.h (shade_kernels.hip).  Like the other image passes,
// a call waits or queues on the context's stream, writes nothing to mrt_stats and reads no scene, tuner or schedule state.
#include <hip/hip_runtime.h>
#include "mrt_context.h"
#include "denoise.h"
#include "gbuffer.h"

namespace {

using namespace mrt::dn;

// the shared opening of the four image calls: refusals, then the kernel's arguments
#define DENOISE_BEGIN(call, refl, depth, guide, hist, color, out)                                                          \
	if (!ctx) return MRT_ERR_INVALID;                                                                                      \
	if (const char *why = denoise_invalid(call, params, W, H, refl, depth, guide, hist, color, out, flags))               \
		return fail(ctx, MRT_ERR_INVALID, why);                                                                            \
	BEGIN_PASS(ctx, (uint64_t)W * H);                                                                                      \
	DenoiseArgs a;                                                                                                         \
	fill_denoise_args(params, W, H, a)

} // namespace

extern "C" {

int mrt_denoise_spatial(mrt_ctx *ctx, const mrt_denoise_params *params, uint32_t W, uint32_t H, const float *d_reflection,
		const float *d_depth, const float *d_normal_roughness, float *d_out, uint32_t flags)
{
	DENOISE_BEGIN(DN_SPATIAL, d_reflection, d_depth, d_normal_roughness, nullptr, nullptr, d_out);
	HIP_TRY(ctx, mrt::launch_denoise(false, a, d_reflection, d_depth, d_normal_roughness, nullptr, nullptr, d_out, ctx->stream));
	return finish_call(ctx, flags);
}

int mrt_denoise_temporal(mrt_ctx *ctx, const mrt_denoise_params *params, uint32_t W, uint32_t H, const float *d_current,
		const float *d_history, float *d_out, uint32_t flags)
{
	DENOISE_BEGIN(DN_TEMPORAL, d_current, nullptr, nullptr, d_history, nullptr, d_out);
	HIP_TRY(ctx, mrt::launch_denoise_temporal(a, d_current, d_history, d_out, ctx->stream));
	return finish_call(ctx, flags);
}

int mrt_composite_reflections(mrt_ctx *ctx, const mrt_denoise_params *params, uint32_t W, uint32_t H, const float *d_reflection,
		const float *d_depth, const float *d_normal_roughness, float *d_color, uint32_t flags)
{
	DENOISE_BEGIN(DN_COMPOSITE, d_reflection, d_depth, d_normal_roughness, nullptr, d_color, nullptr);
	HIP_TRY(ctx, mrt::launch_composite(a, d_reflection, d_depth, d_normal_roughness, d_color, ctx->stream));
	return finish_call(ctx, flags);
}

int mrt_resolve_reflections(mrt_ctx *ctx, const mrt_denoise_params *params, uint32_t W, uint32_t H, const float *d_reflection,
		const float *d_depth, const float *d_normal_roughness, float *d_history, float *d_color, float *d_denoised, uint32_t flags)
{
	DENOISE_BEGIN(DN_RESOLVE, d_reflection, d_depth, d_normal_roughness, d_history, d_color, d_denoised);
	HIP_TRY(ctx, mrt::launch_denoise(true, a, d_reflection, d_depth, d_normal_roughness, d_history, d_color, d_denoised, ctx->stream));
	return finish_call(ctx, flags);
}

int mrt_reflection_guides(mrt_ctx *ctx, const mrt_hit32 *d_hits, const mrt_surface64 *d_rows, uint64_t count, float inv_depth_range,
		float *d_depth, float *d_normal_roughness, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = guides_invalid(d_hits, d_rows, count, inv_depth_range, d_depth, d_normal_roughness, flags))
		return fail(ctx, MRT_ERR_INVALID, why);
	BEGIN_PASS(ctx, count);
	HIP_TRY(ctx, mrt::launch_reflection_guides(d_hits, d_rows, count, inv_depth_range, d_depth, d_normal_roughness, ctx->stream));
	return finish_call(ctx, flags);
}

int mrt_reflection_image(mrt_ctx *ctx, const mrt_gbuffer *gbuffer, uint32_t W, uint32_t H, const mrt_hit32 *d_hits, const float *d_lit,
		float *d_reflection, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::gb::image_invalid(gbuffer, W, H, d_hits, d_reflection, flags)) return fail(ctx, MRT_ERR_INVALID, why);
	BEGIN_PASS(ctx, (uint64_t)W * H);
	mrt::GBufferParams s;
	mrt::gb::fill_params(gbuffer, W, H, nullptr, s);
	HIP_TRY(ctx, mrt::launch_reflection_image(s, d_hits, d_lit, d_reflection, ctx->stream));
	return finish_call(ctx, flags);
}

} // extern "C"
