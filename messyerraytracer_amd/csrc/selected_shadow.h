// selected_shadow.h -- host side of mrt_cast_selected_shadows / mrt_cast_grid_selected_shadows (include/mrt_hip.h): what the calls
// refuse before any device work, in the order the header lists, and the kernel's argument from the caller's descriptor and lights
// (host/selected_shadow_data.cpp).  The shadow half of a light as the kernels read it is made here for mrt_cast_shadows too.  Host-only
// code may include this without HIP.
#pragma once
#include "mrt_internal.h"

static_assert(sizeof(mrt_light_select) == 24, "mrt_light_select must be 24 bytes");

namespace mrt {
namespace sel {

// The kernels' lights from the caller's: OFF for cast_shadows == 0, the direction of a directional light, the position of a point or
// spot light.  An unknown type is refused (the lights before it are filled).
inline const char *fill_shadow_lights(const mrt_light *lights, uint32_t n_lights, ShadowLight *out)
{
	for (uint32_t l = 0; l < n_lights; l++) {
		const mrt_light &L = lights[l];
		if (L.type > MRT_LIGHT_SPOT) return "unknown light type";
		ShadowLight &d = out[l];
		d.kind = !L.cast_shadows ? SHADOW_OFF : (L.type == MRT_LIGHT_DIRECTIONAL ? SHADOW_DIRECTIONAL : SHADOW_POINT);
		const float *v = L.type == MRT_LIGHT_DIRECTIONAL ? L.direction : L.position;
		d.v[0] = v[0]; d.v[1] = v[1]; d.v[2] = v[2];
	}
	return nullptr;
}

// host/selected_shadow_data.cpp (no device, no library)
// What a selected-shadow cast refuses, or null.  array_entry: mrt_cast_selected_shadows (d_rays is required and HOST_LAYOUT is a flag
// it knows); the grid form passes any non-null d_rays.
const char *cast_invalid(bool array_entry, const void *d_rays, const void *d_hits, const mrt_light_select *desc, const mrt_light *lights,
		uint32_t n_lights, const uint8_t *d_mask, uint32_t flags);
// The kernel's argument of a cast that passed cast_invalid, n_lights >= 1.  pixel0: the pixel index of record 0 (a row band: y0 * grid_w).
void fill_params(const void *d_hits, const mrt_light_select *desc, const mrt_light *lights, uint32_t n_lights, uint32_t pixel0,
		SelectShadowParams &s);

} // namespace sel
} // namespace mrt
