// light_panorama_kernel.h — direct light on resolved surfaces with a panorama resident (mrt_upload_panorama): what the lighting calls
// launch instead of light_surfaces_kernel when an environment is given.  Included by shade_kernels.hip (inside namespace mrt, after
// light_kernel.h and before path_kernel.h; panorama.h holds PanoramaParams and the sampler's arithmetic).
//
// sky_color's and shade_material's panorama branches (shade_pass.h:248-257, :692-699): a miss writes sample(d) * energy, a hit's
// ambient factor is sample(n) * energy.  The kernel is light_surfaces_kernel's text (light_body.inc) with those two places exchanged;
// the panorama's pointer, dimensions and energy are a third kernel argument, so that LightParams and light_surfaces_kernel stay as
// they are.  A record samples once -- the row's normal or the ray's direction -- before the loop over lights: two atan2_core in fp64
// (about 45 fp64 operations and one division each), then four 16-byte loads whose columns x0 and x1 are neighbours except at the
// wrap.  No LDS, no scratch.
#pragma once

// sample(dir) * energy (include/mrt_hip.h): panorama.h's sky_panorama with each texel read as one 16-byte load
__device__ __forceinline__ void panorama_sky(const PanoramaParams &pano, float dx, float dy, float dz, float &r, float &g, float &b)
{
	r = g = b = 0.0f;
	if (!finite3(dx, dy, dz)) return;
	float u, v;
	equirect_uv(dx, dy, dz, u, v);
	PanoTaps t;
	panorama_taps(u, v, pano.width, pano.height, t);
	const float4 *texels = reinterpret_cast<const float4 *>(pano.texels);
	const float4 p00 = texels[t.i00], p10 = texels[t.i10], p01 = texels[t.i01], p11 = texels[t.i11];
	r = pano_blend(p00.x, p10.x, p01.x, p11.x, t) * pano.energy;
	g = pano_blend(p00.y, p10.y, p01.y, p11.y, t) * pano.energy;
	b = pano_blend(p00.z, p10.z, p01.z, p11.z, t) * pano.energy;
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void light_panorama_surfaces_kernel(const TraceParams p, const LightParams s, const PanoramaParams pano)
{
#define MRT_PANO 1
#include "light_body.inc"
#undef MRT_PANO
}
