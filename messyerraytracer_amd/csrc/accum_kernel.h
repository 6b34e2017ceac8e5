// accum_kernel.h — mrt_accumulate's kernel: the running mean of RayRenderer::_convert_output (src/modules/graphics/ray_renderer.cpp
// :812-827) and the bytes of the mean (:850-857), with the frame's last pass fused in for a lit frame or a path state.  Included by
// shade_kernels.hip inside namespace mrt, after path_frame_kernel.h, whose pack_rgba8 it calls; tonemap and path_gamma are path.h's,
// accum_step accum.h's, to_rgba8 channels.h's: nothing is restated.
// One thread per pixel, 256 per workgroup, no LDS, no scratch.  One 16-byte load of the source (KIND 2: the second 16 bytes of the
// 32-byte state), one 16-byte load of the accumulator unless FIRST, one 16-byte store of it and one 4-byte store of the bytes.  KIND
// (an MRT_ACCUM_SRC_*) and FIRST (n_prior == 0: the reference's memcpy, nothing is read from the accumulator and no arithmetic
// touches the sample) are template arguments; the optional byte plane is a scalar branch over the launch.
#pragma once

template <int KIND, bool FIRST>
__global__ __launch_bounds__(MRT_WG) void accumulate_kernel(const void *source, uint64_t count, uint32_t mode, float white, float inv,
		float *accum, uint8_t *rgba8)
{
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= count) return;
	float4 s;
	if (KIND == MRT_ACCUM_SRC_PATH_STATE) {
		s = (reinterpret_cast<const float4 *>(source) + i * 2u)[1];
		s.x = path_gamma(tonemap(s.x, mode, white));
		s.y = path_gamma(tonemap(s.y, mode, white));
		s.z = path_gamma(tonemap(s.z, mode, white));
		s.w = 1.0f;
	} else {
		s = reinterpret_cast<const float4 *>(source)[i];
		if (KIND == MRT_ACCUM_SRC_LIT) {
			if (s.w != 0.0f) { // a hit; a miss keeps the sky as it is
				s.x = path_gamma(tonemap(s.x, mode, white));
				s.y = path_gamma(tonemap(s.y, mode, white));
				s.z = path_gamma(tonemap(s.z, mode, white));
			}
			s.w = 1.0f;
		}
	}
	float4 *acc = reinterpret_cast<float4 *>(accum) + i;
	if (!FIRST) {
		const float4 a = *acc;
		s.x = accum_step(a.x, s.x, inv);
		s.y = accum_step(a.y, s.y, inv);
		s.z = accum_step(a.z, s.z, inv);
		s.w = accum_step(a.w, s.w, inv);
	}
	*acc = s;
	if (rgba8 != nullptr) reinterpret_cast<uint32_t *>(rgba8)[i] = pack_rgba8(s);
}
