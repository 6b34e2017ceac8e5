// path_frame_kernel.h — the small kernels around a frame: mrt_path_init's and mrt_path_finish's (the path-traced frame's last pass,
// src/modules/graphics/cpu_path_tracer.h:202-222: tone mapping and gamma; path.h holds both, shared with the host), and after them
// mrt_finish_color's and mrt_image_to_rgba8's.  Included by
// shade_kernels.hip inside namespace mrt, ahead of surface_kernel.h.  The order matters to nothing outside that unit: plain kernels
// are laid out in source order and the last one carries the padding that ends the section, which tools/isa_symbols.py leaves out.
// One thread per entry, 16-byte loads and stores; pow01 is fp64.
#pragma once

__global__ __launch_bounds__(MRT_WG) void path_init_kernel(mrt_path_state *state, uint64_t count)
{
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= count) return;
	float4 *st = reinterpret_cast<float4 *>(state) + i * 2u;
	float4 a, b;
	a.x = 1.0f; a.y = 1.0f; a.z = 1.0f; a.w = __uint_as_float(1u);
	b.x = 0.0f; b.y = 0.0f; b.z = 0.0f; b.w = __uint_as_float(0u);
	st[0] = a; st[1] = b;
}

__global__ __launch_bounds__(MRT_WG) void path_finish_kernel(const mrt_path_state *state, uint64_t count, uint32_t mode, float white, float *rgba)
{
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= count) return;
	const float4 r = (reinterpret_cast<const float4 *>(state) + i * 2u)[1];
	float4 o;
	o.x = path_gamma(tonemap(r.x, mode, white));
	o.y = path_gamma(tonemap(r.y, mode, white));
	o.z = path_gamma(tonemap(r.z, mode, white));
	o.w = 1.0f;
	reinterpret_cast<float4 *>(rgba)[i] = o;
}

// The same last pass for a lit frame (mrt_finish_color: shade_pass.h:669-675, :718-725) and RayImage::to_image (mrt_image_to_rgba8:
// ray_image.cpp:22-35; to_rgba8 is channels.h's).  One 16-byte load per entry, one 16-byte and / or one 4-byte store; rgba may be lit.
__device__ __forceinline__ uint32_t pack_rgba8(const float4 o)
{
	return to_rgba8(o.x) | (to_rgba8(o.y) << 8) | (to_rgba8(o.z) << 16) | (to_rgba8(o.w) << 24);
}

__global__ __launch_bounds__(MRT_WG) void finish_color_kernel(const float *lit, uint64_t count, uint32_t mode, float white, float *rgba, uint8_t *rgba8)
{
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= count) return;
	float4 o = reinterpret_cast<const float4 *>(lit)[i];
	if (o.w != 0.0f) { // a hit; a miss keeps the sky as it is
		o.x = path_gamma(tonemap(o.x, mode, white));
		o.y = path_gamma(tonemap(o.y, mode, white));
		o.z = path_gamma(tonemap(o.z, mode, white));
	}
	o.w = 1.0f;
	if (rgba != nullptr) reinterpret_cast<float4 *>(rgba)[i] = o;
	if (rgba8 != nullptr) reinterpret_cast<uint32_t *>(rgba8)[i] = pack_rgba8(o);
}

__global__ __launch_bounds__(MRT_WG) void image_to_rgba8_kernel(const float *rgba, uint64_t count, uint8_t *rgba8)
{
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= count) return;
	reinterpret_cast<uint32_t *>(rgba8)[i] = pack_rgba8(reinterpret_cast<const float4 *>(rgba)[i]);
}
