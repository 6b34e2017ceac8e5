// panorama.hip — the panorama a context holds (include/mrt_hip.h: mrt_upload_panorama, mrt_clear_panorama).  The descriptor's checks
// and the scan of a host image are host/panorama_data.cpp; the kernels that sample it are light_kernel.h and path_kernel.h
// (shade_kernels.hip), launched by lighting.hip and path.hip while a panorama is resident.
#include <hip/hip_runtime.h>
#include "mrt_context.h"
#include "panorama.h"

namespace {

void forget_panorama(mrt_ctx *ctx)
{
	release(ctx->pano_texels);
	ctx->pano_width = ctx->pano_height = 0u;
	ctx->pano_energy = 0.0f;
	ctx->pano_resident = false;
}

} // namespace

extern "C" {

int mrt_upload_panorama(mrt_ctx *ctx, const mrt_panorama *pano)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::panorama_invalid(pano)) return fail(ctx, MRT_ERR_INVALID, why);
	const uint64_t n_texels = (uint64_t)pano->width * pano->height;
	const bool on_device = (pano->flags & MRT_PANORAMA_ON_DEVICE) != 0u;
	if (!on_device && !mrt::panorama_texels_finite(pano->pixels, n_texels)) return fail(ctx, MRT_ERR_INVALID, "a panorama texel is not finite");
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "collect the pending dispatch first");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (a queued lighting call may still read the panorama about to be replaced)
	const size_t bytes = (size_t)n_texels * 16u;
	ctx->pano_resident = false; // (nothing resident until the copy is)
	if (int rc = ensure(ctx, ctx->pano_texels, bytes)) {
		forget_panorama(ctx);
		return rc;
	}
	hipError_t e = hipMemcpyAsync(ctx->pano_texels.ptr, pano->pixels, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if (e != hipSuccess) {
		forget_panorama(ctx);
		std::snprintf(ctx->err, sizeof(ctx->err), "panorama upload failed: %s", hipGetErrorString(e));
		return MRT_ERR_HIP;
	}
	ctx->pano_width = pano->width; ctx->pano_height = pano->height; ctx->pano_energy = pano->energy;
	ctx->pano_resident = true;
	return MRT_OK;
}

int mrt_clear_panorama(mrt_ctx *ctx)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "collect the pending dispatch first");
	if (!ctx->pano_resident && !ctx->pano_texels.ptr) return MRT_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	forget_panorama(ctx);
	return MRT_OK;
}

} // extern "C"
