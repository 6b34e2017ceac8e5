// accum.hip — the running mean of progressive frames on the device (include/mrt_hip.h: mrt_accumulate).  The refusals, 1 / (n + 1)
// and the frame policy around the call are host/accum_data.cpp and accum.h; the kernel is accum_kernel.h (shade_kernels.hip).  Like the
// image passes, the call waits or queues on the context's stream, writes nothing to mrt_stats and reads no tuner or schedule state.
#include <hip/hip_runtime.h>
#include "mrt_context.h"
#include "accum.h"

extern "C" {

int mrt_accumulate(mrt_ctx *ctx, uint32_t source_kind, const void *d_source, uint64_t count, uint32_t tonemap_mode, uint32_t n_prior,
		float *d_accum, uint8_t *d_rgba8, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::accumulate_invalid(source_kind, d_source, count, tonemap_mode, n_prior, d_accum, flags))
		return fail(ctx, MRT_ERR_INVALID, why);
	BEGIN_PASS(ctx, count);
	HIP_TRY(ctx, mrt::launch_accumulate((int)source_kind, n_prior == 0u, d_source, count, tonemap_mode, mrt::finish_white(), mrt::accum_inv(n_prior),
			d_accum, d_rgba8, ctx->stream));
	return finish_call(ctx, flags);
}

} // extern "C"
