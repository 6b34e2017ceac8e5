// surface.hip — the shade data a context holds and the resolve of hit records to shading surfaces (include/mrt_hip.h:
// mrt_upload_shade_data, mrt_clear_shade_data, mrt_resolve_surfaces, mrt_resolve_grid_surfaces).  The descriptor's checks and the
// packing of host arrays are host/shade_data.cpp; the kernels are surface_kernel.h (shade_kernels.hip), one of them for a context
// with a texture set resident (texture.hip).
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>
#include "mrt_context.h"
#include "shade_data.h"
#include "texture.h"

namespace {

void forget_shade_data(mrt_ctx *ctx)
{
	release(ctx->shade_rows); release(ctx->shade_materials);
	ctx->shade_n_tris = ctx->shade_n_materials = ctx->shade_present = 0u;
}

// Both resolves after their own checks: p holds the incoming rays (or the grid) and the count.
int resolve(mrt_ctx *ctx, int src, mrt::TraceParams &p, const void *d_hits, const mrt_surface_out *out, uint32_t flags)
{
	const uint32_t known = (src == mrt::SURF_GRID ? 0u : MRT_FLAG_HOST_LAYOUT) | MRT_FLAG_ASYNC;
	if (flags & ~known) return fail(ctx, MRT_ERR_INVALID, "unknown flag for a surface resolve");
	if (!d_hits || !out) return fail(ctx, MRT_ERR_INVALID, "null hits / outputs");
	if (!out->d_rows && !out->d_bounce_surface && !out->d_out_hits) return fail(ctx, MRT_ERR_INVALID, "no output asked for");
	BEGIN_PASS(ctx, p.count);
	mrt::SurfaceParams s;
	std::memset(&s, 0, sizeof(s));
	s.records = d_hits;
	shade_data_params(ctx, s);
	s.out_rows = out->d_rows; s.out_bounce = out->d_bounce_surface; s.out_hits = out->d_out_hits;
	const mrt::TextureParams t = texture_params(ctx); // (texture.hip) resident: extract_surface in full
	HIP_TRY(ctx, mrt::launch_resolve_surfaces(p, s, ctx->tex_resident ? &t : nullptr, src, ctx->stream));
	return finish_call(ctx, flags);
}

} // namespace

extern "C" {

int mrt_upload_shade_data(mrt_ctx *ctx, const mrt_shade_data *data)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::shade_data_invalid(data)) return fail(ctx, MRT_ERR_INVALID, why);
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "collect the pending dispatch first");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (a queued resolve may still read the rows about to be replaced)
	const uint32_t present = mrt::shade_data_present(data);
	const size_t row_bytes = present ? (size_t)data->n_tris * 64u : 0u, mat_bytes = (size_t)data->n_materials * sizeof(mrt_material);
	ctx->shade_n_tris = ctx->shade_n_materials = ctx->shade_present = 0u; // (nothing resident until everything below is)
	int rc = MRT_OK;
	if (row_bytes && (rc = ensure(ctx, ctx->shade_rows, row_bytes))) { forget_shade_data(ctx); return rc; }
	if (mat_bytes && (rc = ensure(ctx, ctx->shade_materials, mat_bytes))) { forget_shade_data(ctx); return rc; }
	hipError_t e = hipSuccess;
	std::vector<uint32_t> rows;
	if (row_bytes) {
		if (data->flags & MRT_SHADE_ARRAYS_ON_DEVICE)
			e = mrt::launch_pack_shade_rows(data->material_ids, data->normals9, data->uvs6, data->n_tris, ctx->shade_rows.ptr, ctx->stream);
		else {
			rows.resize((size_t)data->n_tris * 16u);
			mrt::pack_shade_rows_host(data, rows.data());
			e = hipMemcpyAsync(ctx->shade_rows.ptr, rows.data(), row_bytes, hipMemcpyHostToDevice, ctx->stream);
		}
	}
	if (e == hipSuccess && mat_bytes) e = hipMemcpyAsync(ctx->shade_materials.ptr, data->materials, mat_bytes, hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if (e != hipSuccess) {
		forget_shade_data(ctx);
		std::snprintf(ctx->err, sizeof(ctx->err), "shade data upload failed: %s", hipGetErrorString(e));
		return MRT_ERR_HIP;
	}
	ctx->shade_n_tris = data->n_tris; ctx->shade_n_materials = data->n_materials; ctx->shade_present = present;
	return MRT_OK;
}

int mrt_clear_shade_data(mrt_ctx *ctx)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "collect the pending dispatch first");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	forget_shade_data(ctx);
	return MRT_OK;
}

int mrt_resolve_surfaces(mrt_ctx *ctx, const void *d_rays, const void *d_hits, uint64_t count, const mrt_surface_out *out, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!d_rays) return fail(ctx, MRT_ERR_INVALID, "null rays");
	mrt::TraceParams p;
	const int src = record_params(d_rays, count, flags, p);
	return resolve(ctx, src, p, d_hits, out, flags);
}

int mrt_resolve_grid_surfaces(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1,
		const void *d_hits, const mrt_surface_out *out, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	mrt::TraceParams p;
	int rc = grid_params(ctx, cam, grid_w, grid_h, y0, y1, p);
	if (rc) return rc;
	return resolve(ctx, mrt::SURF_GRID, p, d_hits, out, flags);
}

} // extern "C"
