// light_kernel.h — direct light on resolved surfaces (mrt_light_surfaces / mrt_light_grid_surfaces).  Included by shade_kernels.hip (inside
// namespace mrt, after source_common.h; lighting.h holds LightParams and pow01).
//
// ShadePass::cook_torrance_multi_light of the reference (src/modules/graphics/shade_pass.h:597-657) and the terms shade_material adds
// around it (:669-716), against the rows resolve_surfaces_kernel wrote.  One thread per record, nothing walked: the record and its ray
// as record_surface reads them, the row as four 16-byte loads, one mask byte per light at stride count (consecutive lanes read
// consecutive bytes), one 16-byte store.  The lights and the environment are kernel arguments: the loop over lights, the switch on a
// light's type and the tests of `mask` and `has_env` are uniform.  Every floating-point expression is in the order include/mrt_hip.h
// states (nothing is contracted); pow01 is fp64 and runs only for point and spot lights within range.  No LDS, no scratch.  The kernel's
// body is light_body.inc, which light_panorama_kernel.h includes as well.
#pragma once

// the incoming direction of record i as given, hit or miss (the sky gradient of a miss reads it)
template <bool HOST, bool GRID>
__device__ __forceinline__ void record_direction(const TraceParams &p, uint64_t i, float &dx, float &dy, float &dz)
{
	if (HOST) {
		const float *v = reinterpret_cast<const float *>(p.rays) + i * 15u;
		dx = v[3]; dy = v[4]; dz = v[5];
	} else if (GRID) {
		RayRegs o;
		uint64_t gx; const uint64_t gy = udivmod(i, p.grid_w, gx);
		grid_ray(p, (uint32_t)gx, (uint32_t)gy, o);
		dx = o.dx; dy = o.dy; dz = o.dz;
	} else {
		const float4 d = (reinterpret_cast<const float4 *>(p.rays) + i * 2u)[1];
		dx = d.x; dy = d.y; dz = d.z;
	}
}

__device__ __forceinline__ float max0(float x) { return x < 0.0f ? 0.0f : x; }

// g1 of geometry_smith_ggx
__device__ __forceinline__ float smith_g1(float x, float a2)
{
	return (2.0f * x) / ((x + __builtin_sqrtf(a2 + ((1.0f - a2) * x) * x)) + 1e-7f);
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void light_surfaces_kernel(const TraceParams p, const LightParams s)
{
#define MRT_PANO 0
#include "light_body.inc"
#undef MRT_PANO
}
