// path.h -- the path tracer's per-pixel state (mrt_path_init, mrt_path_step, mrt_path_grid_step, mrt_path_finish): the step kernel's
// argument block, the tone mappers as include/mrt_hip.h states them (one definition for the kernel, path_kernel.h, and the host, which
// evaluates Hable's white value once per call), and the checks of the calls (host/path_data.cpp).  Host-only code may include this
// without HIP.
#pragma once
#include "lighting.h"

static_assert(sizeof(mrt_path_state) == 32, "mrt_path_state must be 32 bytes");

namespace mrt {

// Record i of a step is entry i; TraceParams::count = records, rays = the incoming rays as for a resolve (or the grid).
struct PathParams {
	const void *records;       // mrt_hit32 (SURF_RAY32, SURF_GRID) or mrt_host_hit44 (SURF_HOST)
	const void *rows;          // mrt_surface64 per record
	const float *direct;       // float4 per record
	mrt_path_state *state;
	uint8_t *out_select;
	uint8_t *out_lobe;         // optional
	uint32_t *active_count;    // optional
	uint32_t bounce, max_bounces;
	uint32_t seed_add;         // frame * 6529 + 7 (+ y0 * grid_w * 1009 for a row band): seed = record * 1009 + seed_add
	uint32_t jump_a, jump_c;   // the generator's state before draw first_draw = jump_a * state0 + jump_c
	float zenith[3], horizon[3], ground[3], ambient[3], ambient_energy;
};

// _hable_partial
MRT_HD inline float hable_partial(float x)
{
	const float A = 0.15f, B = 0.50f, CB = 0.10f * 0.50f, DE = 0.20f * 0.02f, DF = 0.20f * 0.30f, EF = 0.02f / 0.30f;
	return ((x * (A * x + CB) + DE) / (x * (A * x + B) + DF)) - EF;
}

// tonemap_rgb's operator for one channel: mode 0 .. 4, white = hable_partial(11.2f)
MRT_HD inline float tonemap(float c, uint32_t mode, float white)
{
	switch (mode) {
		case 1: return c / (c + 1.0f);
		case 2: return hable_partial(c) / white;
		case 3: {
			const float m = (c * (2.51f * c + 0.03f)) / (c * (2.43f * c + 0.59f) + 0.14f);
			return m < 0.0f ? 0.0f : (m > 1.0f ? 1.0f : m);
		}
		case 4: {
			const float x = c < 0.0f ? 0.0f : c, x2 = x * x;
			const float m = x2 / ((x2 + 0.09f * x) + 0.0009f);
			return m > 1.0f ? 1.0f : m;
		}
		default: return c;
	}
}

// the display transfer after it: pow(max(c, 0), 1 / 2.2f)
MRT_HD inline float path_gamma(float c) { return pow01(c < 0.0f ? 0.0f : c, 1.0f / 2.2f); }

// host/path_data.cpp (no device, no library)
// draws of a pixel's stream before the lobe draw of bounce b: three per bounce, one more for every roulette before it
inline uint32_t path_first_draw(uint32_t bounce) { return 3u * bounce + (bounce > 2u ? bounce - 2u : 0u); }
// (A, C) with: PCG32 state before draw k = A * state0 + C, modulo 2^32
void path_jump(uint32_t k, uint32_t &a, uint32_t &c);
// What a step refuses, or null, in the order include/mrt_hip.h lists; known = the flags of the form.
const char *path_step_invalid(const void *d_rays_or_cam, const void *d_hits, const void *d_rows, const mrt_path_step_desc *desc,
		uint32_t flags, uint32_t known);
// The same for mrt_path_init (d_out null) and mrt_path_finish.
const char *path_frame_invalid(const void *d_state, const void *d_out, bool need_out, uint32_t flags, uint32_t tonemap_mode);
// The kernel's block from a checked descriptor; pixel0 = the pixel index of record 0.
void fill_path_params(const mrt_path_step_desc *desc, uint32_t pixel0, PathParams &s);

} // namespace mrt
