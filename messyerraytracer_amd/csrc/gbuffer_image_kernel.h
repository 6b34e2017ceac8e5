// gbuffer_image_kernel.h — the kernel of mrt_reflection_image (include/mrt_hip.h): the reflection image of the effect's first pass
// (rt_reflections.comp.glsl:321-331) from the records of mrt_cast_gbuffer_reflections.  Included by shade_kernels.hip inside namespace
// mrt.  The per-pixel rule is gbuffer.h's image_pixel, shared with the host: nothing is restated here.
// A stream: one thread per pixel, 256 per workgroup; reads 32 bytes of record and, for a hit, 20 bytes of G-buffer (and 16 of the lit
// buffer), writes 16.  A miss reads nothing else.  The matrices arrive in the kernel argument (scalar loads).
#pragma once

__global__ __launch_bounds__(MRT_WG) void reflection_image_kernel(const GBufferParams s, uint64_t count, const mrt_hit32 *hits, const dn::Px4 *lit,
		dn::Px4 *out)
{
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= count) return;
	const float4 a = reinterpret_cast<const float4 *>(hits)[i * 2u];
	const int32_t prim_id = __float_as_int(a.y);
	dn::Px4 px = {0.0f, 0.0f, 0.0f, 0.0f};
	if (prim_id != -1) {
		const float4 b = reinterpret_cast<const float4 *>(hits)[i * 2u + 1u];
		uint64_t x;
		const uint64_t y = udivmod(i, s.w, x);
		dn::Px4 l = {0.0f, 0.0f, 0.0f, 0.0f};
		if (lit != nullptr) l = lit[i];
		px = gb::image_pixel(s.normal_kind, s.inv_projection, s.inv_view, s.roughness_threshold, (uint32_t)x, (uint32_t)y, s.w, s.h, s.depth[i],
				reinterpret_cast<const dn::Px4 *>(s.guide)[i], prim_id, b.x, b.y, b.z, lit != nullptr, l);
	}
	out[i] = px;
}
