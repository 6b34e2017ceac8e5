// path_data.cpp -- host side of mrt_path_init / mrt_path_step / mrt_path_grid_step / mrt_path_finish: the refusals in the order
// include/mrt_hip.h lists, the generator's jump to a bounce's first draw and the kernel's copy of a descriptor (path.h).  No device and
// no HIP call, so that csrc/host/path_data_test.cpp drives it alone.
#include "../path.h"
#include "../source_cast.h"

#include <cmath>

namespace mrt {

void path_jump(uint32_t k, uint32_t &A, uint32_t &C)
{
	uint32_t a = 747796405u, c = 2891336453u; // the reference's PCG32 (path_state.h): state' = state * a + c
	A = 1u; C = 0u;
	for (; k != 0u; k >>= 1) { // by squaring: the step (a, c) applied twice is (a * a, a * c + c)
		if (k & 1u) { A = a * A; C = a * C + c; }
		c = a * c + c; a = a * a;
	}
}

const char *path_step_invalid(const void *d_rays_or_cam, const void *d_hits, const void *d_rows, const mrt_path_step_desc *desc,
		uint32_t flags, uint32_t known)
{
	if (!d_rays_or_cam || !d_hits || !d_rows || !desc) return "null rays / hits / rows / descriptor";
	if (!desc->d_direct || !desc->d_state || !desc->env || !desc->d_out_select) return "null d_direct / d_state / env / d_out_select";
	if (flags & ~known) return "unknown flag for a path step";
	if (desc->bounce > desc->max_bounces) return "bounce > max_bounces";
	if (desc->frame > MRT_PATH_MAX_FRAME) return "frame > MRT_PATH_MAX_FRAME";
	if (desc->max_bounces > MRT_PATH_MAX_BOUNCES) return "max_bounces > MRT_PATH_MAX_BOUNCES";
	const mrt_environment *env = desc->env;
	const float f[13] = { env->sky_zenith[0], env->sky_zenith[1], env->sky_zenith[2], env->sky_horizon[0], env->sky_horizon[1],
		env->sky_horizon[2], env->sky_ground[0], env->sky_ground[1], env->sky_ground[2], env->ambient[0], env->ambient[1],
		env->ambient[2], env->ambient_energy };
	for (float x : f)
		if (!std::isfinite(x)) return "the environment holds a value that is not finite";
	return nullptr;
}

const char *path_frame_invalid(const void *d_state, const void *d_out, bool need_out, uint32_t flags, uint32_t tonemap_mode)
{
	if (!d_state || (need_out && !d_out)) return "null state / output";
	if (flags & ~(uint32_t)MRT_FLAG_ASYNC) return "unknown flag for a path state call";
	if (tonemap_mode > 4u) return "tonemap_mode > 4";
	return nullptr;
}

void fill_path_params(const mrt_path_step_desc *desc, uint32_t pixel0, PathParams &s)
{
	s.direct = desc->d_direct; s.state = desc->d_state;
	s.out_select = desc->d_out_select; s.out_lobe = desc->d_out_lobe; s.active_count = desc->d_active_count;
	s.bounce = desc->bounce; s.max_bounces = desc->max_bounces;
	s.seed_add = sc::seed_add(pixel0, desc->frame); // the seed rule of every record-driven cast
	path_jump(path_first_draw(desc->bounce), s.jump_a, s.jump_c);
	const mrt_environment *env = desc->env;
	for (int k = 0; k < 3; k++) {
		s.zenith[k] = env->sky_zenith[k]; s.horizon[k] = env->sky_horizon[k]; s.ground[k] = env->sky_ground[k];
		s.ambient[k] = env->ambient[k];
	}
	s.ambient_energy = env->ambient_energy;
}

} // namespace mrt
