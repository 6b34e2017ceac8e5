// light_data.cpp -- host side of mrt_light_surfaces / mrt_light_grid_surfaces: the checks of the light list and the environment, the
// kernel's copy of both (cos_outer = cosf(spot_angle): the one libm call of the formula, made here) and mrt_shadow_lights (lighting.h).
// No device and no HIP call, so that csrc/host/light_data_test.cpp drives it alone.
#include "../lighting.h"

#include <cmath>
#include <cstring>

namespace mrt {

const char *light_list_invalid(const mrt_shade_light *lights, uint32_t n_lights, const mrt_environment *env, uint64_t count)
{
	if (n_lights > MRT_MAX_LIGHTS) return "more than MRT_MAX_LIGHTS lights";
	if (n_lights && !lights) return "n_lights > 0 with null lights";
	for (uint32_t l = 0; l < n_lights; l++) {
		const mrt_shade_light &L = lights[l];
		if (L.type > MRT_LIGHT_SPOT) return "unknown light type";
		if (L.reserved != 0u) return "a light's reserved word is not 0";
		const float f[13] = { L.position[0], L.position[1], L.position[2], L.direction[0], L.direction[1], L.direction[2],
			L.color[0], L.color[1], L.color[2], L.range, L.attenuation, L.spot_angle, L.spot_angle_attenuation };
		for (float x : f)
			if (!std::isfinite(x)) return "a light holds a value that is not finite";
		if (L.type != MRT_LIGHT_DIRECTIONAL && !(L.range > 0.0f)) return "a point or spot light's range is not > 0";
		if (L.attenuation < 0.0f || L.spot_angle_attenuation < 0.0f) return "a light's attenuation exponent is negative";
	}
	if (env) {
		const float f[13] = { env->sky_zenith[0], env->sky_zenith[1], env->sky_zenith[2], env->sky_horizon[0], env->sky_horizon[1],
			env->sky_horizon[2], env->sky_ground[0], env->sky_ground[1], env->sky_ground[2], env->ambient[0], env->ambient[1],
			env->ambient[2], env->ambient_energy };
		for (float x : f)
			if (!std::isfinite(x)) return "the environment holds a value that is not finite";
	}
	if (n_lights && count > UINT64_MAX / n_lights) return "count * n_lights overflows";
	return nullptr;
}

void fill_light_params(const mrt_shade_light *lights, uint32_t n_lights, const mrt_environment *env, LightParams &lp)
{
	lp.n_lights = n_lights;
	lp.has_env = env ? 1u : 0u;
	if (env) {
		for (int k = 0; k < 3; k++) {
			lp.zenith[k] = env->sky_zenith[k]; lp.horizon[k] = env->sky_horizon[k]; lp.ground[k] = env->sky_ground[k];
			lp.ambient[k] = env->ambient[k];
		}
		lp.ambient_energy = env->ambient_energy;
	}
	for (uint32_t l = 0; l < n_lights; l++) {
		const mrt_shade_light &L = lights[l];
		KernelLight &K = lp.light[l];
		K.type = L.type;
		for (int k = 0; k < 3; k++) { K.position[k] = L.position[k]; K.direction[k] = L.direction[k]; K.color[k] = L.color[k]; }
		K.range = L.range; K.attenuation = L.attenuation; K.spot_attenuation = L.spot_angle_attenuation;
		K.cos_outer = cosf(L.spot_angle);
		K.one_minus_cos_outer = 1.0f - K.cos_outer;
		K.pad = 0u;
	}
}

void shadow_lights(const mrt_shade_light *lights, uint32_t n, mrt_light *out)
{
	static_assert(sizeof(mrt_light) == 32, "mrt_light is the first 32 bytes of mrt_shade_light");
	for (uint32_t l = 0; l < n; l++) std::memcpy(&out[l], &lights[l], sizeof(mrt_light));
}

} // namespace mrt
