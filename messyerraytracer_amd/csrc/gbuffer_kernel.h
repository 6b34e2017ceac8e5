// gbuffer_kernel.h — reflection rays made in the trace kernels from a rasteriser's G-buffer (mrt_cast_gbuffer_reflections).
// Included by kernels.hip (inside namespace mrt, after source_common.h, before the kernels that use it); gbuffer.h, which holds the
// formula for host and device, is included by kernels.hip before the namespace opens.
//
// Pass 1 of the reference's RTReflectionEffect (src/gpu/shaders/rt_reflections.comp.glsl:276-332) as it runs inside a rasterised
// frame: the world position from the depth buffer through inv_projection and inv_view, the view direction reflected about the
// decoded normal, traced closest-hit over [0, max_distance] from world + n * 0.01.  A source family of source_common.h with one source
// (SRC_GBUFFER, closest-hit only); entry i is pixel (i % w, i / w) and its result is the record mrt_cast(MRT_MODE_NEAREST) writes for
// the ray.  Every operation is gbuffer.h's reflection_ray, in the order include/mrt_hip.h states.  Unlike the record-driven family
// (reflection_kernel.h) the normal is not turned towards the viewer: a rasteriser's normals face the camera, and the shader does not
// turn them.  A sky pixel (its guide texel is not read), a pixel above the roughness threshold and a pixel whose origin or direction
// is not finite get no ray: the placeholder Ray(0, (0,1,0), 0, 0) and its record (t = 0 and a miss); they never walk the tree.
// The two matrices are read from the kernel argument with constant indices: 28 scalar loads, no vector memory instruction.
#pragma once

// The ray of pixel i, or (false) the record of a pixel without one, stored.
template <int SRC, bool ANY_HIT>
__device__ __forceinline__ bool source_entry(const TraceParams &p, const GBufferParams &s, uint64_t i, RayRegs &r)
{
	static_assert(gbuffer_source(SRC) && !ANY_HIT, "the G-buffer source is closest-hit");
	bool traced = false;
	const float depth = s.depth[i];
	if (!gb::sky(depth)) {
		const dn::Px4 g = reinterpret_cast<const dn::Px4 *>(s.guide)[i];
		uint64_t x;
		const uint64_t y = udivmod(i, s.w, x);
		float org[3], dir[3];
		traced = gb::reflection_ray(s.normal_kind, s.inv_projection, s.inv_view, s.roughness_threshold, (uint32_t)x, (uint32_t)y, s.w, s.h,
				depth, g, org, dir);
		if (traced) {
			r.ox = org[0]; r.oy = org[1]; r.oz = org[2]; r.dx = dir[0]; r.dy = dir[1]; r.dz = dir[2];
			r.t_min = 0.0f; r.t_max = s.max_distance;
		}
	}
	if (!traced) placeholder_ray(r);
	if (s.out_rays != nullptr) store_ray(s.out_rays, false, i, r);
	if (traced) return true;
	store_placeholder_record(p, i);
	return false;
}
