// texture.hip — the texture set a context holds (include/mrt_hip.h: mrt_upload_textures, mrt_clear_textures).  The descriptor's
// checks and the pool's layout are host/texture_data.cpp; the resolve that samples the set is surface_kernel.h with surface_tex_kernel.h (shade_kernels.hip),
// launched by surface.hip while a set is resident.
#include <vector>
#include <hip/hip_runtime.h>
#include "mrt_context.h"
#include "texture.h"

namespace {

void forget_textures(mrt_ctx *ctx)
{
	release(ctx->tex_texels); release(ctx->tex_table); release(ctx->tex_bindings); release(ctx->tex_tangents);
	ctx->tex_n_bindings = ctx->tex_n_tangent_tris = 0u;
	ctx->tex_resident = false;
}

} // namespace

extern "C" {

int mrt_upload_textures(mrt_ctx *ctx, const mrt_texture_set *set)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (const char *why = mrt::texture_set_invalid(set)) return fail(ctx, MRT_ERR_INVALID, why);
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "collect the pending dispatch first");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (a queued resolve may still read the set about to be replaced)
	std::vector<mrt::TextureDesc> table(set->n_textures);
	const uint64_t units = mrt::texture_pool_layout(set, table.data());
	const size_t pool_bytes = (size_t)units * 16u, table_bytes = table.size() * sizeof(mrt::TextureDesc);
	const size_t bind_bytes = (size_t)set->n_bindings * sizeof(mrt_material_textures), tan_bytes = (size_t)set->n_tangent_tris * 48u;
	ctx->tex_resident = false; // (nothing resident until everything below is)
	int rc = MRT_OK;
	if ((pool_bytes && (rc = ensure(ctx, ctx->tex_texels, pool_bytes))) || (table_bytes && (rc = ensure(ctx, ctx->tex_table, table_bytes))) ||
			(bind_bytes && (rc = ensure(ctx, ctx->tex_bindings, bind_bytes))) || (tan_bytes && (rc = ensure(ctx, ctx->tex_tangents, tan_bytes)))) {
		forget_textures(ctx);
		return rc;
	}
	const hipMemcpyKind kind = (set->flags & MRT_TEXTURES_ON_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
	hipError_t e = hipSuccess;
	// the padding between images is never read; it is zeroed so that the pool's bytes are the same from upload to upload
	if (pool_bytes) e = hipMemsetAsync(ctx->tex_texels.ptr, 0, pool_bytes, ctx->stream);
	for (uint32_t t = 0; e == hipSuccess && t < set->n_textures; t++) {
		const mrt_texture &T = set->textures[t];
		e = hipMemcpyAsync(static_cast<char *>(ctx->tex_texels.ptr) + (size_t)table[t].offset16 * 16u, T.pixels,
				(size_t)T.width * T.height * mrt::texel_bytes(T.format), kind, ctx->stream);
	}
	if (e == hipSuccess && table_bytes) e = hipMemcpyAsync(ctx->tex_table.ptr, table.data(), table_bytes, hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess && bind_bytes) e = hipMemcpyAsync(ctx->tex_bindings.ptr, set->bindings, bind_bytes, hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess && tan_bytes) e = hipMemcpyAsync(ctx->tex_tangents.ptr, set->tangents12, tan_bytes, kind, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if (e != hipSuccess) {
		forget_textures(ctx);
		std::snprintf(ctx->err, sizeof(ctx->err), "texture upload failed: %s", hipGetErrorString(e));
		return MRT_ERR_HIP;
	}
	ctx->tex_n_bindings = set->n_bindings; ctx->tex_n_tangent_tris = set->n_tangent_tris;
	ctx->tex_resident = true;
	return MRT_OK;
}

int mrt_clear_textures(mrt_ctx *ctx)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "collect the pending dispatch first");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	forget_textures(ctx);
	return MRT_OK;
}

} // extern "C"
