// accum_data.cpp -- host side of progressive frames: mrt_halton_jitter, mrt_accum_begin_frame and mrt_accum_end_frame (the frame policy
// of RayRenderer, ray_renderer.cpp:441-504 and :804-835; the arithmetic is accum.h's) and the refusals of mrt_accumulate in the order
// include/mrt_hip.h lists.  No context, no device and no HIP call, so that csrc/host/accum_data_test.cpp drives it alone.
#include "../accum.h"

namespace mrt {

const char *accumulate_invalid(uint32_t source_kind, const void *d_source, uint64_t count, uint32_t tonemap_mode, uint32_t n_prior,
		const void *d_accum, uint32_t flags)
{
	if (!d_source || !d_accum) return "null source / accumulator";
	if (flags & ~(uint32_t)MRT_FLAG_ASYNC) return "unknown flag for mrt_accumulate";
	if (source_kind > (uint32_t)MRT_ACCUM_SRC_PATH_STATE) return "unknown source_kind";
	if (source_kind != (uint32_t)MRT_ACCUM_SRC_RGBA && tonemap_mode > 4u) return "tonemap_mode > 4";
	if (n_prior > 0x7ffffffeu) return "n_prior > 0x7ffffffe";
	if (d_accum == d_source) return "d_accum is d_source";
	if (count > UINT64_MAX / 32u) return "count * 32 overflows";
	return nullptr;
}

namespace {

const char *state_invalid(const mrt_accum_state *st)
{
	if (!st) return "null state";
	if (st->struct_size != sizeof(mrt_accum_state)) return "struct_size is not sizeof(mrt_accum_state)";
	return nullptr;
}

} // namespace

} // namespace mrt

extern "C" {

int mrt_halton_jitter(uint32_t sample_index, float jitter[2])
{
	if (!jitter) return MRT_ERR_INVALID;
	if (sample_index > 0x7ffffffeu) return MRT_ERR_INVALID;
	jitter[0] = mrt::halton2((int)(sample_index + 1u));
	jitter[1] = mrt::halton3((int)(sample_index + 1u));
	return MRT_OK;
}

int mrt_accum_begin_frame(mrt_accum_state *st, const float origin[3], const float basis[9])
{
	if (!origin || !basis || mrt::state_invalid(st)) return MRT_ERR_INVALID;
	if (st->aa_enabled == 0u || mrt::camera_changed(origin, basis, st->prev_origin, st->prev_basis)) st->count = 0u;
	for (int k = 0; k < 3; k++) st->prev_origin[k] = origin[k];
	for (int k = 0; k < 9; k++) st->prev_basis[k] = basis[k];
	st->sample_index = st->count;
	st->jitter_x = st->jitter_y = 0.5f;
	if (mrt::accum_open(st)) { // count < max_samples <= INT_MAX, so the index is one mrt_halton_jitter takes
		float j[2];
		(void)mrt_halton_jitter(st->count, j);
		st->jitter_x = j[0]; st->jitter_y = j[1];
	}
	return MRT_OK;
}

int mrt_accum_end_frame(mrt_accum_state *st, uint64_t pixels)
{
	if (mrt::state_invalid(st)) return MRT_ERR_INVALID;
	st->accumulate = 0u; st->n_prior = 0u;
	if (!mrt::accum_open(st)) return MRT_OK;
	if (pixels != st->pixels) { st->pixels = pixels; st->count = 0u; } // the resolution changed
	st->n_prior = st->count;
	st->accumulate = 1u;
	st->count++;
	return MRT_OK;
}

} // extern "C"
