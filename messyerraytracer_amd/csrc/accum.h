// accum.h -- progressive frames (mrt_halton_jitter, mrt_accum_begin_frame, mrt_accum_end_frame, mrt_accumulate): the Halton pair, the
// camera-motion test and the running-mean step as include/mrt_hip.h states them (one definition for the kernel, accum_kernel.h, and the
// host), and the checks of the device call (host/accum_data.cpp).  Host-only code may include this without HIP.
#pragma once
#include "channels.h"

static_assert(sizeof(mrt_accum_state) == 96, "mrt_accum_state must be 96 bytes");

namespace mrt {

// RayRenderer's two lambdas (ray_renderer.cpp:480-501); idx > 0 is the caller's to see to
MRT_HD inline float halton2(int idx)
{
	float f = 1.0f, r = 0.0f;
	int i = idx;
	while (i > 0) {
		f = f * 0.5f;
		r = r + f * (float)(i & 1);
		i >>= 1;
	}
	return r;
}
MRT_HD inline float halton3(int idx)
{
	const float INV3 = 1.0f / 3.0f;
	float f = 1.0f, r = 0.0f;
	int i = idx;
	while (i > 0) {
		f = f * INV3;
		r = r + f * (float)(i % 3);
		i /= 3;
	}
	return r;
}

// Vector3::length_squared of a - b
MRT_HD inline float diff_length_squared(float ax, float ay, float az, float bx, float by, float bz)
{
	const float x = ax - bx, y = ay - by, z = az - bz;
	return (x * x + y * y) + z * z;
}

// moved || rotated of :452-459 (a NaN compares false); basis row-major, column c = {b[c], b[3 + c], b[6 + c]}
inline bool camera_changed(const float origin[3], const float basis[9], const float prev_origin[3], const float prev_basis[9])
{
	const float POS_EPS = 1e-4f, ROT_EPS = 1e-3f;
	const bool moved = diff_length_squared(origin[0], origin[1], origin[2], prev_origin[0], prev_origin[1], prev_origin[2]) > POS_EPS * POS_EPS;
	bool rotated = false;
	if (!moved)
		for (int c = 0; c < 3 && !rotated; c++)
			rotated = diff_length_squared(basis[c], basis[3 + c], basis[6 + c], prev_basis[c], prev_basis[3 + c], prev_basis[6 + c]) > ROT_EPS * ROT_EPS;
	return moved || rotated;
}

// set_aa_max_samples' clamp, applied where the value is read
inline int32_t accum_max_samples(const mrt_accum_state *st) { return st->max_samples > 1 ? st->max_samples : 1; }
inline bool accum_open(const mrt_accum_state *st) { return st->aa_enabled != 0u && (int64_t)st->count < (int64_t)accum_max_samples(st); }

// one component of the running mean (:824-827): three separately rounded operations
MRT_HD inline float accum_step(float acc, float s, float inv)
{
	const float d = s - acc;
	const float p = d * inv;
	return acc + p;
}
// 1 / (n + 1) as :818 computes it
inline float accum_inv(uint32_t n_prior) { return 1.0f / (float)(int)(n_prior + 1u); }

// host/accum_data.cpp (no device, no library)
// What mrt_accumulate refuses before any device work, or null, in the order include/mrt_hip.h lists.
const char *accumulate_invalid(uint32_t source_kind, const void *d_source, uint64_t count, uint32_t tonemap_mode, uint32_t n_prior,
		const void *d_accum, uint32_t flags);

} // namespace mrt
