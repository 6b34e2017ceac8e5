// emitters.hip — emissive triangles as light sources (include/mrt_hip.h): the resident emitter table (mrt_build_emitters,
// mrt_clear_emitters, mrt_emitter_info, mrt_emitter_table), built on the device by the kernels of emitter_build_kernel.h, and the light
// call over it (mrt_light_emitter_surfaces, mrt_light_grid_emitter_surfaces; its kernel is emitter_light_kernel.h, shade_kernels.hip).
// The cast is cast.hip's (a source family of the trace kernels), the step path.hip's.  The refusals and the kernels' arguments are
// host/emitter_data.cpp.  Compiled without contraction, like every unit.
#include <cfloat>
#include <cstring>
#include <hip/hip_runtime.h>
#include "mrt_context.h"
#include "shade_data.h"
#include "emitters.h"

namespace mrt {
#include "emitter_build_kernel.h"
}

namespace {

void forget_emitters(mrt_ctx *ctx)
{
	release(ctx->emit_rows); release(ctx->emit_cdf);
	ctx->emit_n = ctx->emit_total = 0u;
}

uint32_t blocks_of(uint32_t n) { return (uint32_t)(((uint64_t)n + mrt::EM_WG - 1u) / mrt::EM_WG); }

// Both light calls after their own checks: p holds the incoming rays (or the grid) and the count; pixel0 = the pixel index of record 0.
int light(mrt_ctx *ctx, int src, mrt::TraceParams &p, const void *d_hits, const mrt_surface64 *d_rows, uint32_t pixel0,
		const mrt_emitter_select *desc, const uint8_t *d_mask, uint32_t accumulate, const mrt_light_out *out, uint32_t flags)
{
	BEGIN_PASS(ctx, p.count);
	mrt::EmitterLightParams s;
	mrt::em::fill_light(d_hits, d_rows, desc, d_mask, accumulate, out, emitter_table(ctx), pixel0, s);
	HIP_TRY(ctx, mrt::launch_light_emitter_surfaces(p, s, src, ctx->stream));
	return finish_call(ctx, flags);
}

} // namespace

extern "C" {

int mrt_build_emitters(mrt_ctx *ctx, const mrt_tri64 *tris, uint32_t n_tris, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::em::build_invalid(tris, n_tris, flags)) return fail(ctx, MRT_ERR_INVALID, why);
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "collect the pending dispatch first");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (a queued cast or light call may still read the table about to be replaced)
	// nothing can emit: no triangles, or no material ids or materials resident
	if (n_tris == 0u || !(ctx->shade_present & mrt::SHADE_HAS_IDS) || ctx->shade_n_materials == 0u) { forget_emitters(ctx); return MRT_OK; }
	int rc;
	mrt::EmitterBuildParams b;
	std::memset(&b, 0, sizeof(b));
	b.tris = tris; b.n_tris = n_tris;
	b.shade_rows = ctx->shade_rows.ptr; b.materials = ctx->shade_materials.ptr;
	b.n_shade_tris = ctx->shade_n_tris; b.n_materials = ctx->shade_n_materials; b.has_ids = 1u;
	if (!(flags & MRT_BUILD_TRIS_ON_DEVICE)) {
		if ((rc = ensure(ctx, ctx->emit_in, (size_t)n_tris * sizeof(mrt_tri64)))) return rc;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->emit_in.ptr, tris, (size_t)n_tris * sizeof(mrt_tri64), hipMemcpyHostToDevice, ctx->stream));
		b.tris = (const mrt_tri64 *)ctx->emit_in.ptr;
	}
	// the work block: the header, one count per workgroup of triangles, one sum per workgroup of emitters
	const uint32_t nb = blocks_of(n_tris), nb_emit_max = blocks_of(MRT_MAX_EMITTERS);
	const size_t hdr_bytes = mrt::EM_HDR_WORDS * sizeof(unsigned long long);
	if ((rc = ensure(ctx, ctx->emit_work, hdr_bytes + ((size_t)nb + nb_emit_max) * 4u))) return rc;
	unsigned long long *hdr = (unsigned long long *)ctx->emit_work.ptr;
	uint32_t *block_count = (uint32_t *)((char *)ctx->emit_work.ptr + hdr_bytes), *block_sum = block_count + nb;
	HIP_TRY(ctx, hipMemsetAsync(hdr, 0, hdr_bytes, ctx->stream));
	hipLaunchKernelGGL(mrt::emitter_flag_kernel, dim3(nb), dim3(mrt::EM_WG), 0, ctx->stream, b, block_count, hdr);
	hipLaunchKernelGGL(mrt::scan_words_kernel, dim3(1), dim3(mrt::EM_WG), 0, ctx->stream, block_count, nb, hdr + mrt::EM_HDR_COUNT);
	HIP_TRY(ctx, hipGetLastError());
	unsigned long long h[mrt::EM_HDR_WORDS];
	HIP_TRY(ctx, hipMemcpyAsync(h, hdr, hdr_bytes, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	if (h[mrt::EM_HDR_COUNT] > MRT_MAX_EMITTERS) return fail(ctx, MRT_ERR_UNSUPPORTED, "more than MRT_MAX_EMITTERS emitters");
	const uint32_t n_emit = (uint32_t)h[mrt::EM_HDR_COUNT];
	if (n_emit == 0u) { forget_emitters(ctx); return MRT_OK; }
	// the new table beside the resident one, which stays until this one is whole
	DevBuf rows, cdf;
	if ((rc = ensure(ctx, rows, (size_t)n_emit * sizeof(mrt_emitter64))) || (rc = ensure(ctx, cdf, (size_t)n_emit * 4u))) { release(rows); return rc; }
	const uint32_t nb_emit = blocks_of(n_emit);
	hipLaunchKernelGGL(mrt::emitter_compact_kernel, dim3(nb), dim3(mrt::EM_WG), 0, ctx->stream, b, block_count, hdr, n_emit, (uint4 *)rows.ptr);
	hipLaunchKernelGGL(mrt::emitter_weight_kernel, dim3(nb_emit), dim3(mrt::EM_WG), 0, ctx->stream, (uint4 *)rows.ptr, n_emit, hdr, (uint32_t *)cdf.ptr,
			block_sum);
	hipLaunchKernelGGL(mrt::scan_words_kernel, dim3(1), dim3(mrt::EM_WG), 0, ctx->stream, block_sum, nb_emit, hdr + mrt::EM_HDR_TOTAL);
	hipLaunchKernelGGL(mrt::emitter_cdf_kernel, dim3(nb_emit), dim3(mrt::EM_WG), 0, ctx->stream, (uint32_t *)cdf.ptr, n_emit, block_sum);
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipMemcpyAsync(h, hdr, hdr_bytes, hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if (e != hipSuccess) {
		release(rows); release(cdf);
		std::snprintf(ctx->err, sizeof(ctx->err), "emitter build failed: %s", hipGetErrorString(e));
		return MRT_ERR_HIP;
	}
	release(ctx->emit_rows); release(ctx->emit_cdf);
	ctx->emit_rows = rows; ctx->emit_cdf = cdf;
	ctx->emit_n = n_emit; ctx->emit_total = (uint32_t)h[mrt::EM_HDR_TOTAL];
	return MRT_OK;
}

int mrt_clear_emitters(mrt_ctx *ctx)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "collect the pending dispatch first");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	forget_emitters(ctx);
	return MRT_OK;
}

int mrt_emitter_info(const mrt_ctx *ctx, uint32_t *n_emitters, uint32_t *total)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (n_emitters) *n_emitters = ctx->emit_n;
	if (total) *total = ctx->emit_total;
	return MRT_OK;
}

int mrt_emitter_table(mrt_ctx *ctx, mrt_emitter64 *rows, uint32_t *cdf, uint32_t capacity)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "collect the pending dispatch first");
	const uint32_t n = capacity < ctx->emit_n ? capacity : ctx->emit_n;
	if (n == 0u) return MRT_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (rows) HIP_TRY(ctx, hipMemcpyAsync(rows, ctx->emit_rows.ptr, (size_t)n * sizeof(mrt_emitter64), hipMemcpyDeviceToHost, ctx->stream));
	if (cdf) HIP_TRY(ctx, hipMemcpyAsync(cdf, ctx->emit_cdf.ptr, (size_t)n * 4u, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return MRT_OK;
}

int mrt_light_emitter_surfaces(mrt_ctx *ctx, const void *d_rays, const void *d_hits, const mrt_surface64 *d_rows, uint64_t count,
		const mrt_emitter_select *desc, const uint8_t *d_mask, uint32_t accumulate, const mrt_light_out *out, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::em::light_invalid(true, d_rays, d_hits, d_rows, desc, accumulate, out, flags)) return fail(ctx, MRT_ERR_INVALID, why);
	mrt::TraceParams p;
	const int src = record_params(d_rays, count, flags, p);
	return light(ctx, src, p, d_hits, d_rows, 0u, desc, d_mask, accumulate, out, flags);
}

int mrt_light_grid_emitter_surfaces(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1,
		const void *d_hits, const mrt_surface64 *d_rows, const mrt_emitter_select *desc, const uint8_t *d_mask, uint32_t accumulate,
		const mrt_light_out *out, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	mrt::TraceParams p;
	int rc = grid_params(ctx, cam, grid_w, grid_h, y0, y1, p);
	if (rc) return rc;
	if (const char *why = mrt::em::light_invalid(false, cam, d_hits, d_rows, desc, accumulate, out, flags)) return fail(ctx, MRT_ERR_INVALID, why);
	return light(ctx, mrt::SURF_GRID, p, d_hits, d_rows, y0 * grid_w, desc, d_mask, accumulate, out, flags);
}

} // extern "C"
