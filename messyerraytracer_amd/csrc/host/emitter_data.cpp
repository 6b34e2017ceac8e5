// emitter_data.cpp -- host side of the emitter calls (emitters.h): what each refuses of its arguments, in the order the header's table
// gives, and the kernels' arguments.  No context, no device and no HIP call, so that csrc/host/emitter_data_test.cpp drives it alone.
#include "../emitters.h"
#include "../source_cast.h"

#include <cstring>

namespace mrt {
namespace em {

const char *build_invalid(const void *tris, uint32_t n_tris, uint32_t flags)
{
	if (n_tris && !tris) return "null tris";
	if (flags & ~(uint32_t)MRT_BUILD_TRIS_ON_DEVICE) return "unknown flag for an emitter build";
	return nullptr;
}

const char *shadow_invalid(bool array_entry, const void *d_rays, const void *d_hits, const mrt_emitter_select *desc, const uint8_t *d_mask,
		uint32_t flags)
{
	if (!d_rays) return "null rays";
	if (!d_hits) return "null hits";
	if (!desc) return "null descriptor";
	if (!d_mask) return "null mask";
	if (!desc->d_out_emitter) return "null d_out_emitter";
	if (sc::unknown_flag(array_entry, flags)) return "unknown flag for an emitter-shadow cast";
	if (desc->frame > MRT_PATH_MAX_FRAME) return "frame > MRT_PATH_MAX_FRAME";
	return nullptr;
}

const char *light_invalid(bool array_entry, const void *d_rays, const void *d_hits, const void *d_rows, const mrt_emitter_select *desc,
		uint32_t accumulate, const mrt_light_out *out, uint32_t flags)
{
	if (!d_rays) return "null rays";
	if (!d_hits) return "null hits";
	if (!d_rows) return "null rows";
	if (!desc) return "null descriptor";
	if (!desc->d_out_emitter) return "null d_out_emitter";
	if (!out || !out->d_rgba) return "null output";
	if (sc::unknown_flag(array_entry, flags)) return "unknown flag for an emitter lighting call";
	if (accumulate > MRT_EMITTER_ACCUMULATE) return "accumulate must be 0 or MRT_EMITTER_ACCUMULATE";
	if (desc->frame > MRT_PATH_MAX_FRAME) return "frame > MRT_PATH_MAX_FRAME";
	return nullptr;
}

const char *step_invalid(const mrt_path_step_desc *desc, const uint8_t *d_prev_lobe)
{
	if (desc->bounce >= 1u && !d_prev_lobe) return "null d_prev_lobe with bounce >= 1";
	return nullptr;
}

void fill_shadow(const void *d_hits, const mrt_emitter_select *desc, const EmitterTable &table, uint32_t pixel0, EmitterShadowParams &s)
{
	std::memset(&s, 0, sizeof(s));
	s.records = d_hits; s.select = desc->d_select; s.out_emitter = desc->d_out_emitter;
	s.table = table;
	s.seed_add = sc::seed_add(pixel0, desc->frame);
	s.jump = pcg_jump(desc->draw);
}

void fill_light(const void *d_hits, const void *d_rows, const mrt_emitter_select *desc, const uint8_t *d_mask, uint32_t accumulate,
		const mrt_light_out *out, const EmitterTable &table, uint32_t pixel0, EmitterLightParams &s)
{
	std::memset(&s, 0, sizeof(s));
	s.records = d_hits; s.rows = d_rows; s.emitter = desc->d_out_emitter; s.mask = d_mask; s.out = out->d_rgba;
	s.table = table;
	s.accumulate = accumulate;
	s.seed_add = sc::seed_add(pixel0, desc->frame);
	s.jump = pcg_jump(desc->draw);
}

} // namespace em
} // namespace mrt
