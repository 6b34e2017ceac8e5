// lighting.hip — direct light on resolved surfaces (include/mrt_hip.h: mrt_shadow_lights, mrt_light_surfaces,
// mrt_light_grid_surfaces, and with one light per record mrt_light_selected_surfaces, mrt_light_grid_selected_surfaces).  The checks of the light list and the environment and the kernel's copy of both are host/light_data.cpp;
// the kernels are light_kernel.h (shade_kernels.hip), one of them for a context with a panorama resident.
#include <cstring>
#include <hip/hip_runtime.h>
#include "mrt_context.h"
#include "lighting.h"
#include "panorama.h"

namespace {

// The four calls after their own checks: p holds the incoming rays (or the grid) and the count.  selected: the all-lights calls have
// no d_light (d_mask is then [light * count + record]); the selected calls require it (d_mask is [record]).
int light(mrt_ctx *ctx, int src, mrt::TraceParams &p, const void *d_hits, const mrt_surface64 *d_rows, const mrt_shade_light *lights,
		uint32_t n_lights, bool selected, const uint8_t *d_light, const uint8_t *d_mask, const mrt_environment *env, const mrt_light_out *out,
		uint32_t flags)
{
	const uint32_t known = (src == mrt::SURF_GRID ? 0u : MRT_FLAG_HOST_LAYOUT) | MRT_FLAG_ASYNC;
	if (flags & ~known) return fail(ctx, MRT_ERR_INVALID, "unknown flag for a lighting call");
	if (!d_hits || !d_rows || !out || !out->d_rgba) return fail(ctx, MRT_ERR_INVALID, "null hits / rows / output");
	if (selected && !d_light) return fail(ctx, MRT_ERR_INVALID, "null d_light");
	if (const char *why = mrt::light_list_invalid(lights, n_lights, env, p.count)) return fail(ctx, MRT_ERR_INVALID, why);
	BEGIN_PASS(ctx, p.count);
	mrt::LightParams s;
	std::memset(&s, 0, sizeof(s));
	s.records = d_hits; s.rows = d_rows; s.mask = d_mask; s.selected = selected ? d_light : nullptr; s.out = out->d_rgba;
	mrt::fill_light_params(lights, n_lights, env, s);
	const mrt::PanoramaParams pano = panorama_params(ctx); // (without an environment no kernel reads the panorama)
	HIP_TRY(ctx, mrt::launch_light_surfaces(p, s, ctx->pano_resident && env ? &pano : nullptr, src, ctx->stream));
	return finish_call(ctx, flags);
}

} // namespace

extern "C" {

int mrt_shadow_lights(const mrt_shade_light *lights, uint32_t n, mrt_light *out)
{
	if (n && (!lights || !out)) return MRT_ERR_INVALID;
	mrt::shadow_lights(lights, n, out);
	return MRT_OK;
}

int mrt_light_surfaces(mrt_ctx *ctx, const void *d_rays, const void *d_hits, const mrt_surface64 *d_rows, uint64_t count,
		const mrt_shade_light *lights, uint32_t n_lights, const uint8_t *d_mask, const mrt_environment *env,
		const mrt_light_out *out, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!d_rays) return fail(ctx, MRT_ERR_INVALID, "null rays");
	mrt::TraceParams p;
	const int src = record_params(d_rays, count, flags, p);
	return light(ctx, src, p, d_hits, d_rows, lights, n_lights, false, nullptr, d_mask, env, out, flags);
}

int mrt_light_grid_surfaces(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1,
		const void *d_hits, const mrt_surface64 *d_rows, const mrt_shade_light *lights, uint32_t n_lights,
		const uint8_t *d_mask, const mrt_environment *env, const mrt_light_out *out, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	mrt::TraceParams p;
	int rc = grid_params(ctx, cam, grid_w, grid_h, y0, y1, p);
	if (rc) return rc;
	return light(ctx, mrt::SURF_GRID, p, d_hits, d_rows, lights, n_lights, false, nullptr, d_mask, env, out, flags);
}

int mrt_light_selected_surfaces(mrt_ctx *ctx, const void *d_rays, const void *d_hits, const mrt_surface64 *d_rows, uint64_t count,
		const mrt_shade_light *lights, uint32_t n_lights, const uint8_t *d_light, const uint8_t *d_mask, const mrt_environment *env,
		const mrt_light_out *out, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!d_rays) return fail(ctx, MRT_ERR_INVALID, "null rays");
	mrt::TraceParams p;
	const int src = record_params(d_rays, count, flags, p);
	return light(ctx, src, p, d_hits, d_rows, lights, n_lights, true, d_light, d_mask, env, out, flags);
}

int mrt_light_grid_selected_surfaces(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1,
		const void *d_hits, const mrt_surface64 *d_rows, const mrt_shade_light *lights, uint32_t n_lights, const uint8_t *d_light,
		const uint8_t *d_mask, const mrt_environment *env, const mrt_light_out *out, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	mrt::TraceParams p;
	int rc = grid_params(ctx, cam, grid_w, grid_h, y0, y1, p);
	if (rc) return rc;
	return light(ctx, mrt::SURF_GRID, p, d_hits, d_rows, lights, n_lights, true, d_light, d_mask, env, out, flags);
}

} // extern "C"
