// path_kernel.h — the path tracer's per-pixel state (mrt_path_step / mrt_path_grid_step; the two small kernels of mrt_path_init and
// mrt_path_finish are path_frame_kernel.h).  Included by shade_kernels.hip (inside namespace mrt, after light_panorama_kernel.h; path.h holds PathParams).
//
// The rest of CPUPathTracer's loop body (src/modules/graphics/cpu_path_tracer.h:110-194) around the links already resident: the
// radiance accumulation, the throughput weights of PathTrace::sample_bounce (path_trace.h:213-246), Russian roulette and the `active`
// flag.  One thread per record, nothing walked: the state as two 16-byte loads, the record and
// its ray as record_surface reads them, the row as four 16-byte loads, the direct light as one, then two 16-byte stores and one or
// two bytes.  The environment, the bounce index and the generator's jump are kernel arguments: the tests of bounce == 0, bounce >= 2
// and bounce == max_bounces are uniform.  Every floating-point expression is in the order include/mrt_hip.h states (nothing is
// contracted).  No LDS, no scratch.
//
// The sampler is bounce_kernel.h's bounce_ray restated operation for operation (its face_normal, clamps, stream, three draws, lobe
// test, local direction, onb_direction, reflection and "below the surface" test), because the weights also need the half vector and
// vh, which bounce_ray does not keep: the trace kernels that inline bounce_ray stay as they are.  The sky gradient is restated for the
// same reason: light_surfaces_kernel calling a shared function came out as other machine code (tools/isa_symbols.py), so it keeps its
// own lines and this is their copy, operation for operation.  The step's body is path_step_body.inc, included once per kernel below.
#pragma once

// sky_color's analytic gradient (shade_pass.h:259-274) of a direction's y as given: light_kernel.h's lines for a miss
__device__ __forceinline__ void sky_gradient(const float (&zenith)[3], const float (&horizon)[3], const float (&ground)[3], float dy,
		float &r, float &g, float &b)
{
	const float t = dy * 0.5f + 0.5f;
	if (t > 0.5f) {
		const float u = (t - 0.5f) * 2.0f;
		r = horizon[0] + (zenith[0] - horizon[0]) * u;
		g = horizon[1] + (zenith[1] - horizon[1]) * u;
		b = horizon[2] + (zenith[2] - horizon[2]) * u;
	} else {
		const float u = t * 2.0f;
		r = ground[0] + (horizon[0] - ground[0]) * u;
		g = ground[1] + (horizon[1] - ground[1]) * u;
		b = ground[2] + (horizon[2] - ground[2]) * u;
	}
}

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void path_step_kernel(const TraceParams p, const PathParams s)
{
#define MRT_PANO 0
#include "path_step_body.inc"
#undef MRT_PANO
}

// The same with a panorama resident (mrt_upload_panorama): the sky of a miss is sample(d) * energy (light_panorama_kernel.h's
// panorama_sky); the ambient line of bounce 0 is the same line, as in the reference.  The panorama is an argument of its own.
template <int SRC>
__global__ __launch_bounds__(MRT_WG) void path_step_panorama_kernel(const TraceParams p, const PathParams s, const PanoramaParams pano)
{
#define MRT_PANO 1
#include "path_step_body.inc"
#undef MRT_PANO
}
