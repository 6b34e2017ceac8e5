// selected_shadow_data.cpp -- host side of mrt_cast_selected_shadows / mrt_cast_grid_selected_shadows: what the calls refuse of a
// descriptor and a light list, in the order include/mrt_hip.h lists, and the kernel's argument.  No context, no device and no HIP call,
// so that csrc/host/selected_shadow_data_test.cpp drives it alone.
#include "../selected_shadow.h"

#include <cstring>

namespace mrt {
namespace sel {

const char *cast_invalid(bool array_entry, const void *d_rays, const void *d_hits, const mrt_light_select *desc, const mrt_light *lights,
		uint32_t n_lights, const uint8_t *d_mask, uint32_t flags)
{
	if (!d_rays) return "null rays";
	if (!d_hits) return "null hits";
	if (!desc) return "null descriptor";
	if (!d_mask) return "null mask";
	if (!desc->d_out_light) return "null d_out_light";
	if (n_lights && !lights) return "n_lights > 0 with null lights";
	if (flags & ~((array_entry ? (uint32_t)MRT_FLAG_HOST_LAYOUT : 0u) | (uint32_t)MRT_FLAG_ASYNC)) return "unknown flag for a selected-shadow cast";
	if (n_lights > MRT_MAX_LIGHTS) return "more than MRT_MAX_LIGHTS lights";
	for (uint32_t l = 0; l < n_lights; l++)
		if (lights[l].type > MRT_LIGHT_SPOT) return "unknown light type";
	if (desc->frame > MRT_PATH_MAX_FRAME) return "frame > MRT_PATH_MAX_FRAME";
	return nullptr;
}

void fill_params(const void *d_hits, const mrt_light_select *desc, const mrt_light *lights, uint32_t n_lights, uint32_t pixel0,
		SelectShadowParams &s)
{
	std::memset(&s, 0, sizeof(s));
	s.records = d_hits; s.select = desc->d_select; s.out_light = desc->d_out_light;
	s.seed_add = pixel0 * 1009u + desc->frame * 6529u + 7u;
	s.jump = pcg_jump(desc->select_draw);
	s.n_lights = n_lights;
	fill_shadow_lights(lights, n_lights, s.light);
}

} // namespace sel
} // namespace mrt
