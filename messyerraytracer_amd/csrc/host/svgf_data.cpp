// svgf_data.cpp -- host side of the SVGF pass chain: the refusals of mrt_svgf_guides, mrt_svgf_temporal, mrt_svgf_variance,
// mrt_svgf_atrous, mrt_svgf_modulate and mrt_svgf_frame in the order include/mrt_hip.h lists, and the kernels' arguments.  No context,
// no device and no HIP call, so that csrc/host/svgf_data_test.cpp drives it alone.
#include "../svgf.h"

namespace mrt {
namespace sv {

namespace {

bool finite(float x) { return x - x == 0.0f; }

// the first image of `written` that equals one of `read` or an earlier written one
bool aliased(const void *const *written, int n_written, const void *const *read, int n_read)
{
	for (int k = 0; k < n_written; k++) {
		if (!written[k]) continue;
		for (int j = 0; j < n_read; j++)
			if (read[j] && written[k] == read[j]) return true;
		for (int j = 0; j < k; j++)
			if (written[k] == written[j]) return true;
	}
	return false;
}

} // namespace

const char *svgf_invalid(int call, const mrt_svgf_params *p, uint32_t w, uint32_t h, uint32_t step, const mrt_camera *prev_cam,
		const SvgfImages &im, uint32_t flags)
{
	if (!p) return "null params";
	const bool temporal = call == SV_TEMPORAL || call == SV_FRAME;
	const bool history = temporal && p->has_history != 0u;
	// the images, each in the order of the call's arguments
	if (!im.illum) return "null d_illum";
	if ((call == SV_MODULATE || call == SV_FRAME) && !im.albedo) return "null d_albedo";
	if (call == SV_VARIANCE && !im.moments) return "null d_moments";
	if (call != SV_MODULATE) {
		if (!im.normal_depth) return "null d_normal_depth";
		if (!im.position) return "null d_position";
	}
	if (history) {
		if (!im.prev_illum) return "null d_prev_illum";
		if (!im.prev_moments) return "null d_prev_moments";
		if (!im.prev_normal_depth) return "null d_prev_normal_depth";
		if (!im.prev_position) return "null d_prev_position";
	}
	if (call != SV_MODULATE && !im.out_illum)
		return call == SV_TEMPORAL ? "null d_out_illum" : (call == SV_FRAME ? "null d_next_illum" : "null d_out");
	if (temporal && !im.out_moments) return call == SV_TEMPORAL ? "null d_out_moments" : "null d_next_moments";
	if (call == SV_FRAME) {
		if (!im.scratch_a) return "null d_scratch_a";
		if (!im.scratch_b) return "null d_scratch_b";
	}
	if ((call == SV_MODULATE || call == SV_FRAME) && !im.rgba) return "null d_rgba";
	if (p->struct_size != sizeof(mrt_svgf_params)) return "struct_size is not sizeof(mrt_svgf_params)";
	if (flags & ~(uint32_t)MRT_FLAG_ASYNC) return "unknown flag for an svgf call";
	if (history) {
		if (!prev_cam) return "null prev_cam";
		if (prev_cam->kind != (uint32_t)MRT_CAMERA_PERSPECTIVE) return "prev_cam is not MRT_CAMERA_PERSPECTIVE";
	}
	if (call == SV_ATROUS && step != 1u && step != 2u && step != 4u && step != 8u && step != 16u) return "step is not 1, 2, 4, 8 or 16";
	if (call == SV_FRAME && (p->iterations < 1u || p->iterations > 5u)) return "iterations is not 1 .. 5";
	if ((call == SV_MODULATE || call == SV_FRAME) && p->tonemap_mode > 4u) return "tonemap_mode > 4";
	const float scalars[8] = {p->color_alpha, p->moments_alpha, p->max_history, p->normal_threshold, p->position_threshold, p->sigma_l,
			p->sigma_n, p->sigma_plane};
	for (float x : scalars)
		if (!finite(x)) return "a non-finite parameter";
	if (!(p->max_history >= 1.0f)) return "max_history < 1";
	for (int k = 3; k < 8; k++)
		if (!(scalars[k] > 0.0f)) return "a threshold or sigma that is not > 0";
	if (w != 0u && (uint64_t)h > UINT64_MAX / 32u / (uint64_t)w) return "W * H * 32 overflows";
	if (call == SV_TEMPORAL) {
		const void *written[2] = {im.out_illum, im.out_moments};
		const void *read[4] = {im.prev_illum, im.prev_moments, im.prev_normal_depth, im.prev_position};
		if (aliased(written, 2, read, history ? 4 : 0)) return "an output is an image read across pixels";
	}
	if (call == SV_VARIANCE || call == SV_ATROUS) {
		const void *written[1] = {im.out_illum};
		const void *read[4] = {im.illum, im.moments, im.normal_depth, im.position};
		if (aliased(written, 1, read, 4)) return "an output is an image read across pixels";
	}
	if (call == SV_FRAME) {
		const void *written[5] = {im.out_illum, im.out_moments, im.scratch_a, im.scratch_b, im.rgba};
		const void *read[8] = {im.illum, im.albedo, im.normal_depth, im.position, im.prev_illum, im.prev_moments, im.prev_normal_depth,
				im.prev_position};
		if (aliased(written, 5, read, history ? 8 : 4)) return "an output is an image read across pixels";
	}
	return nullptr;
}

const char *svgf_guides_invalid(const void *d_rays, const void *d_hits, const void *d_rows, uint32_t source_kind, const void *d_source,
		uint64_t count, const void *d_illum, const void *d_albedo, const void *d_normal_depth, const void *d_position, uint32_t flags)
{
	if (!d_rays) return "null d_rays";
	if (!d_hits) return "null d_hits";
	if (!d_rows) return "null d_rows";
	if (!d_source) return "null d_source";
	if (!d_illum) return "null d_illum";
	if (!d_albedo) return "null d_albedo";
	if (!d_normal_depth) return "null d_normal_depth";
	if (!d_position) return "null d_position";
	if (flags & ~(uint32_t)MRT_FLAG_ASYNC) return "unknown flag for mrt_svgf_guides";
	if (source_kind != (uint32_t)MRT_ACCUM_SRC_RGBA && source_kind != (uint32_t)MRT_ACCUM_SRC_PATH_STATE) return "source_kind is not RGBA or PATH_STATE";
	if (count > UINT64_MAX / 64u) return "count * 64 overflows";
	const void *written[4] = {d_illum, d_albedo, d_normal_depth, d_position};
	if (aliased(written, 4, nullptr, 0)) return "two outputs are equal";
	return nullptr;
}

void fill_svgf_args(const mrt_svgf_params *p, uint32_t w, uint32_t h, uint32_t step, const mrt_camera *cam, float white, SvgfArgs &a)
{
	a = SvgfArgs{};
	a.w = w; a.h = h;
	a.has_history = p->has_history != 0u; a.mode = p->tonemap_mode;
	a.step = (int32_t)step; a.white = white;
	a.color_alpha = p->color_alpha; a.moments_alpha = p->moments_alpha; a.max_history = p->max_history;
	a.normal_threshold = p->normal_threshold; a.position_threshold = p->position_threshold;
	a.sigma_l = p->sigma_l; a.sigma_n = p->sigma_n; a.sigma_plane = p->sigma_plane;
	if (a.has_history && cam) {
		for (int k = 0; k < 3; k++) { a.origin[k] = cam->origin[k]; a.right[k] = cam->right[k]; a.up[k] = cam->up[k]; a.fwd[k] = cam->fwd[k]; }
		a.half_w = cam->half_w; a.half_h = cam->half_h; a.jitter_x = cam->jitter_x; a.jitter_y = cam->jitter_y;
	}
}

} // namespace sv
} // namespace mrt
