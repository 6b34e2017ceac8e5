// shade_kernels.hip — gfx950 kernels of the shading passes over hit records: the resolve to shading surfaces (plain and textured), the
// direct light and the path tracer's per-pixel state (the lighting and the step also with a resident panorama), the renderer's
// channels with the two image passes, the running mean of progressive frames, the reflection effect's image passes, the SVGF pass chain, and the packing of shade rows.  None of them walks a scene; they share the ray and record helpers of device_common.h and record_surface of
// source_common.h with the walks of kernels.hip, and are compiled apart from them.  The arithmetic is the canonical form of DESIGN.md
// ("Arithmetic"), as in kernels.hip.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <type_traits>
#include "mrt_internal.h"
#include "shade_data.h"
#include "texture.h"
#include "lighting.h"
#include "path.h"
#include "panorama.h"
#include "channels.h"
#include "accum.h"
#include "denoise.h"
#include "svgf.h"
#include "emitters.h"
#include "gbuffer.h"
#include "lane_map.h"
#include "walk_steps.h"

namespace mrt {

#include "device_common.h"
#include "dispatch.h"
#include "source_common.h"

#include "path_frame_kernel.h"
#include "accum_kernel.h"
#include "denoise_kernel.h"
#include "svgf_kernel.h"
#include "surface_tex_kernel.h"
#include "surface_kernel.h"
#include "light_kernel.h"
#include "emitter_sample_kernel.h"
#include "emitter_light_kernel.h"
#include "path_kernel.h"
#include "channel_kernel.h"
#include "gbuffer_image_kernel.h"

// ---- launch wrappers (called from surface.hip, lighting.hip and path.hip); src = a SurfaceSrc; t / pano null: none resident --------
hipError_t launch_resolve_surfaces(const TraceParams &p, const SurfaceParams &s, const TextureParams *t, int src, hipStream_t stream)
{
	if (t == nullptr) return launch_surface_pass([](auto SRC) { return resolve_surfaces_kernel<SRC>; }, src, p, stream, s);
	return launch_surface_pass([](auto SRC) { return resolve_textured_surfaces_kernel<SRC>; }, src, p, stream, s, *t);
}
hipError_t launch_light_surfaces(const TraceParams &p, const LightParams &s, const PanoramaParams *pano, int src, hipStream_t stream)
{
	if (s.selected != nullptr) { // one light per record (mrt_light_selected_surfaces)
		if (pano == nullptr) return launch_surface_pass([](auto SRC) { return light_selected_surfaces_kernel<SRC>; }, src, p, stream, s);
		return launch_surface_pass([](auto SRC) { return light_selected_panorama_surfaces_kernel<SRC>; }, src, p, stream, s, *pano);
	}
	if (pano == nullptr) return launch_surface_pass([](auto SRC) { return light_surfaces_kernel<SRC>; }, src, p, stream, s);
	return launch_surface_pass([](auto SRC) { return light_panorama_surfaces_kernel<SRC>; }, src, p, stream, s, *pano);
}
hipError_t launch_path_step(const TraceParams &p, const PathParams &s, const PanoramaParams *pano, int src, hipStream_t stream)
{
	if (pano == nullptr) return launch_surface_pass([](auto SRC) { return path_step_kernel<SRC>; }, src, p, stream, s);
	return launch_surface_pass([](auto SRC) { return path_step_panorama_kernel<SRC>; }, src, p, stream, s, *pano);
}
// mrt_path_step_emitters: prev_lobe may be null at bounce 0 alone (the kernel reads it from bounce 1 on)
hipError_t launch_path_step_emitters(const TraceParams &p, const PathParams &s, const PanoramaParams *pano, const uint8_t *prev_lobe, int src, hipStream_t stream)
{
	if (pano == nullptr) return launch_surface_pass([](auto SRC) { return path_step_emitters_kernel<SRC>; }, src, p, stream, s, prev_lobe);
	return launch_surface_pass([](auto SRC) { return path_step_emitters_panorama_kernel<SRC>; }, src, p, stream, s, *pano, prev_lobe);
}
// the diffuse term of a sampled emitter point (emitter_light_kernel.h), called from emitters.hip
hipError_t launch_light_emitter_surfaces(const TraceParams &p, const EmitterLightParams &s, int src, hipStream_t stream)
{
	return launch_surface_pass([](auto SRC) { return light_emitter_surfaces_kernel<SRC>; }, src, p, stream, s);
}
hipError_t launch_path_init(mrt_path_state *state, uint64_t count, hipStream_t stream)
{
	return launch_per_entry<true>(path_init_kernel, count, stream, state, count);
}
hipError_t launch_path_finish(const mrt_path_state *state, uint64_t count, uint32_t mode, float white, float *rgba, hipStream_t stream)
{
	return launch_per_entry<true>(path_finish_kernel, count, stream, state, count, mode, white, rgba);
}
// the renderer's channels (channel_kernel.h) and the two image passes (path_frame_kernel.h), called from channels.hip
hipError_t launch_shade_channels(const TraceParams &p, const ChannelParams &c, const TextureParams &t, int src, hipStream_t stream)
{
	return launch_surface_pass([](auto SRC) { return shade_channels_kernel<SRC>; }, src, p, stream, c, t);
}
hipError_t launch_finish_color(const float *lit, uint64_t count, uint32_t mode, float white, float *rgba, uint8_t *rgba8, hipStream_t stream)
{
	return launch_per_entry<true>(finish_color_kernel, count, stream, lit, count, mode, white, rgba, rgba8);
}
hipError_t launch_image_to_rgba8(const float *rgba, uint64_t count, uint8_t *rgba8, hipStream_t stream)
{
	return launch_per_entry<true>(image_to_rgba8_kernel, count, stream, rgba, count, rgba8);
}
// the running mean of progressive frames (accum_kernel.h), called from accum.hip; kind = an MRT_ACCUM_SRC_*, first: n_prior == 0
hipError_t launch_accumulate(int kind, bool first, const void *source, uint64_t count, uint32_t mode, float white, float inv, float *accum,
		uint8_t *rgba8, hipStream_t stream)
{
	hipError_t e = count ? hipErrorInvalidValue : hipSuccess;
	dispatch([&](auto KIND, auto FIRST) { e = launch_per_entry<true>(accumulate_kernel<KIND, FIRST>, count, stream, source, count, mode, white, inv, accum, rgba8); },
			Among<(int)MRT_ACCUM_SRC_RGBA, (int)MRT_ACCUM_SRC_LIT, (int)MRT_ACCUM_SRC_PATH_STATE>{kind}, Among<false, true>{first});
	return e;
}
// the reflection effect's image passes (denoise_kernel.h), called from denoise.hip
hipError_t launch_denoise(bool fused, const dn::DenoiseArgs &a, const float *reflection, const float *depth, const float *guide, float *history,
		float *color, float *out, hipStream_t stream)
{
	const uint64_t tiles_x = ((uint64_t)a.w + DN_TILE - 1) / DN_TILE, tiles = tiles_x * (((uint64_t)a.h + DN_TILE - 1) / DN_TILE);
	if (tiles == 0) return hipSuccess;
	if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
	const auto *r = reinterpret_cast<const dn::Px4 *>(reflection), *g = reinterpret_cast<const dn::Px4 *>(guide);
	auto *h = reinterpret_cast<dn::Px4 *>(history), *c = reinterpret_cast<dn::Px4 *>(color), *o = reinterpret_cast<dn::Px4 *>(out);
	if (fused) hipLaunchKernelGGL(denoise_kernel<true>, dim3((uint32_t)tiles), dim3(DN_TILE * DN_TILE), 0, stream, a, (uint32_t)tiles_x, r, depth, g, h, c, o);
	else hipLaunchKernelGGL(denoise_kernel<false>, dim3((uint32_t)tiles), dim3(DN_TILE * DN_TILE), 0, stream, a, (uint32_t)tiles_x, r, depth, g, h, c, o);
	return hipGetLastError();
}
hipError_t launch_denoise_temporal(const dn::DenoiseArgs &a, const float *current, const float *history, float *out, hipStream_t stream)
{
	const uint64_t count = (uint64_t)a.w * a.h;
	return launch_per_entry<true>(temporal_kernel, count, stream, a, count, reinterpret_cast<const dn::Px4 *>(current),
			reinterpret_cast<const dn::Px4 *>(history), reinterpret_cast<dn::Px4 *>(out));
}
hipError_t launch_composite(const dn::DenoiseArgs &a, const float *reflection, const float *depth, const float *guide, float *color, hipStream_t stream)
{
	const uint64_t count = (uint64_t)a.w * a.h;
	return launch_per_entry<true>(composite_kernel, count, stream, a, count, reinterpret_cast<const dn::Px4 *>(reflection), depth,
			reinterpret_cast<const dn::Px4 *>(guide), reinterpret_cast<dn::Px4 *>(color));
}
hipError_t launch_reflection_guides(const mrt_hit32 *hits, const mrt_surface64 *rows, uint64_t count, float inv_depth_range, float *depth,
		float *guide, hipStream_t stream)
{
	return launch_per_entry<true>(guides_kernel, count, stream, hits, rows, count, inv_depth_range, depth, reinterpret_cast<dn::Px4 *>(guide));
}
// the reflection image of a G-buffer cast (gbuffer_image_kernel.h), called from denoise.hip; lit may be null
hipError_t launch_reflection_image(const GBufferParams &s, const mrt_hit32 *hits, const float *lit, float *out, hipStream_t stream)
{
	const uint64_t count = (uint64_t)s.w * s.h;
	return launch_per_entry<true>(reflection_image_kernel, count, stream, s, count, hits, reinterpret_cast<const dn::Px4 *>(lit),
			reinterpret_cast<dn::Px4 *>(out));
}
// the SVGF pass chain (svgf_kernel.h), called from svgf.hip
hipError_t launch_svgf_guides(int kind, const mrt_ray32 *rays, const mrt_hit32 *hits, const mrt_surface64 *rows, const void *source, uint64_t count,
		float *illum, float *albedo, float *normal_depth, float *position, hipStream_t stream)
{
	hipError_t e = count ? hipErrorInvalidValue : hipSuccess;
	dispatch([&](auto KIND) { e = launch_per_entry<true>(svgf_guides_kernel<KIND>, count, stream, rays, hits, rows, source, count, reinterpret_cast<sv::Px4 *>(illum),
				reinterpret_cast<sv::Px4 *>(albedo), reinterpret_cast<sv::Px4 *>(normal_depth), reinterpret_cast<sv::Px4 *>(position)); },
			Among<(int)MRT_ACCUM_SRC_RGBA, (int)MRT_ACCUM_SRC_PATH_STATE>{kind});
	return e;
}
static sv::Images svgf_images(const sv::SvgfArgs &a, const float *illum, const float *moments, const float *normal_depth, const float *position)
{
	return sv::Images{reinterpret_cast<const sv::Px4 *>(illum), reinterpret_cast<const sv::Px4 *>(moments), reinterpret_cast<const sv::Px4 *>(normal_depth),
			reinterpret_cast<const sv::Px4 *>(position), a.w, a.h};
}
hipError_t launch_svgf_temporal(const sv::SvgfArgs &a, const float *illum, const float *normal_depth, const float *position, const float *prev_illum,
		const float *prev_moments, const float *prev_normal_depth, const float *prev_position, float *out_illum, float *out_moments, hipStream_t stream)
{
	const uint64_t count = (uint64_t)a.w * a.h;
	return launch_per_entry<true>(svgf_temporal_kernel, count, stream, a, count, reinterpret_cast<const sv::Px4 *>(illum),
			reinterpret_cast<const sv::Px4 *>(normal_depth), reinterpret_cast<const sv::Px4 *>(position),
			svgf_images(a, prev_illum, prev_moments, prev_normal_depth, prev_position), reinterpret_cast<sv::Px4 *>(out_illum),
			reinterpret_cast<sv::Px4 *>(out_moments));
}
hipError_t launch_svgf_spatial(bool atrous, const sv::SvgfArgs &a, const float *illum, const float *moments, const float *normal_depth,
		const float *position, float *out, hipStream_t stream)
{
	const uint64_t tiles_x = ((uint64_t)a.w + SV_TILE - 1) / SV_TILE, tiles = tiles_x * (((uint64_t)a.h + SV_TILE - 1) / SV_TILE);
	if (tiles == 0) return hipSuccess;
	if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
	const sv::Images im = svgf_images(a, illum, moments, normal_depth, position);
	auto *o = reinterpret_cast<sv::Px4 *>(out);
	if (atrous) hipLaunchKernelGGL(svgf_spatial_kernel<true>, dim3((uint32_t)tiles), dim3(SV_TILE * SV_TILE), 0, stream, a, (uint32_t)tiles_x, im, o);
	else hipLaunchKernelGGL(svgf_spatial_kernel<false>, dim3((uint32_t)tiles), dim3(SV_TILE * SV_TILE), 0, stream, a, (uint32_t)tiles_x, im, o);
	return hipGetLastError();
}
hipError_t launch_svgf_modulate(const sv::SvgfArgs &a, const float *illum, const float *albedo, float *rgba, uint8_t *rgba8, hipStream_t stream)
{
	const uint64_t count = (uint64_t)a.w * a.h;
	return launch_per_entry<true>(svgf_modulate_kernel, count, stream, a, count, reinterpret_cast<const sv::Px4 *>(illum),
			reinterpret_cast<const sv::Px4 *>(albedo), rgba, rgba8);
}
hipError_t launch_pack_shade_rows(const uint32_t *ids, const float *normals9, const float *uvs6, uint32_t n_tris, void *rows, hipStream_t stream)
{
	return launch_per_entry<false>(pack_shade_rows_kernel, n_tris, stream, ids, normals9, uvs6, n_tris, reinterpret_cast<uint4 *>(rows));
}

} // namespace mrt
