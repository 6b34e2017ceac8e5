// kernels.hip — gfx950 (CDNA4, wave64) kernels of the batch ray-cast path: the walks.  The shading passes over hit records are
// shade_kernels.hip and the kernels that prepare a cast or a scene (rows, grid rays, tokens, detection, keys) prep_kernels.hip; the
// three share device_common.h and are compiled apart.
//
// Replaces the reference's GLSL compute shader
// src/gpu/shaders/bvh_traverse.comp.glsl (one thread = one ray, stack-based
// ordered BVH2 traversal over 64-byte dual-AABB nodes, slab test, Moller-
// Trumbore) and the two host conversion loops around it
// (src/gpu/gpu_ray_caster.cpp:639-650, 442-456), which run on the device here.
//
// Arithmetic is the canonical form documented in DESIGN.md ("Arithmetic"):
// compiled with -ffp-contract=off, every fused operation is an explicit
// __builtin_fmaf, so results are bit-identical to oracle/mrt_oracle.c.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "mrt_internal.h"
#include "launch_policy.h"
#include "lane_map.h"
#include "walk_steps.h"
#include "gbuffer.h"

namespace mrt {

#include "device_common.h"
#include "dispatch.h"

#include "source_common.h"
#include "shadow_kernel.h"
#include "selected_shadow_kernel.h"
#include "reflection_kernel.h"
#include "hemisphere_kernel.h"
#include "bounce_kernel.h"
#include "gbuffer_kernel.h"
#include "emitter_sample_kernel.h"
#include "emitter_shadow_kernel.h"

// ---- the traversal kernel: one lane = one ray (lane_walk.h) -------------------------------------
#include "lane_walk.h"
template <bool ANY_HIT, bool COUNT>
__global__ __launch_bounds__(MRT_WG) void trace_lane_kernel(const TraceParams p) { lane_walk<SRC_CAST, ANY_HIT, COUNT>(p, NoSource{}); }

#include "lane_persistent_kernel.h"
#include "packet_kernel.h"
#include "packet_asm_kernel.h"
#include "packet_rows_kernel.h"
#ifdef MRT_WITH_QUAD   // the four-wide packet walk: measured, not faster; build.py MRT_WITH_QUAD=1 compiles it in
#include "packet_quad_kernel.h"
#endif
#include "two_level_kernel.h"

// ---- record-driven casts (source_common.h): the lane kernels a non-coherent batch can get, with a ray source -------------------
// S = the source family's parameters (its own kernel argument: ShadowParams and HemiParams are large, and a union of the five would
// grow every family's argument block), SRC one of its sources, ANY_HIT a mode its source_entry accepts.  The walks are the
// ones of trace_lane_kernel, trace_two_level_kernel and trace_lane_persistent_kernel, called with SRC set.
template <class S, int SRC, bool ANY_HIT>
__global__ __launch_bounds__(MRT_WG) void trace_source_lane_kernel(const TraceParams p, const S s) { lane_walk<SRC, ANY_HIT, false>(p, s); }
template <class S, int SRC, bool ANY_HIT>
__global__ __launch_bounds__(MRT_WG) void trace_source_two_level_kernel(const TraceParams p, const S s) { two_level_walk<SRC, ANY_HIT>(p, s); }
template <class S, int SRC, bool ANY_HIT, int WIDTH, bool TL>
__global__ __launch_bounds__(MRT_WG) MRT_PERSIST_ATTR void trace_source_persistent_kernel(const TraceParams p, const PersistParams q, const S s)
{
	constexpr bool COUNT = false;
#include "persistent_walk.inc" // (in scope: the names its first lines check; kept as a textual body: DESIGN.md 4.2a)
}

// ---- launch wrappers (called from api.hip / cast.hip) -------------------------------------------
bool quad_kernel_built()
{
#ifdef MRT_WITH_QUAD
	return true;
#else
	return false;
#endif
}
// The instantiation the last launch_trace / launch_trace_persistent / launch_source of this thread put on a stream, spelled by
// format_variant (launch_policy.h) from the very TraceVariant that selected the kernel: mrt_last_kernel_variant, which bench.py uses
// to accept committed counter passes only for the kernel the run used.
static thread_local char g_variant[96] = "";
const char *last_trace_variant() { return g_variant; }
#ifndef MRT_ROWS_WG_LARGE
#define MRT_ROWS_WG_LARGE MRT_WG // threads per workgroup of the rows kernel on large scenes
#endif

// launch_policy.cpp resolve_trace decides everything -- the kernel, its template arguments, the grid --; this is the lookup.
hipError_t launch_trace(const TraceParams &p_in, bool any_hit, bool count, hipStream_t stream)
{
	const TraceLaunch l = resolve_trace(p_in, any_hit, count, quad_kernel_built(), MRT_ROWS_WG_LARGE);
	if (l.error) return hipErrorInvalidValue;
	if (l.blocks == 0) return hipSuccess;
	TraceParams p = p_in;
	p.tile_group = l.tile_group;
	const TraceVariant &v = l.v;
	p.rows_fast = kFastNo;
	if (v.kernel == TraceKernel::PACKET_ROWS) { // whole-tile pairs take the short map (lane_map.h)
		FastLaunch f;
		f.packets = v.packets; f.counting = v.count; f.lane_map = p.lane_map;
		f.k = p.tile_w_log2; f.order = p.tile_order; f.quarter_all = p.quarter_all;
		f.sched = p.tile_sched != nullptr; f.perm = p.perm != nullptr; f.tile_cost = p.tile_cost != nullptr;
		f.ray32_in = p.in_fmt == IN_RAY32; f.hit32_out = p.out_fmt == OUT_HIT32;
		f.auto_grid = p.auto_grid != nullptr;
		f.skip = p.skip_flag == nullptr ? 0 : (p.auto_grid != nullptr && p.skip_flag == p.auto_grid + 3 ? 1 : 2);
		p.rows_fast = fast_launch(f);
	}
	const Bool a{v.any_hit}, c{v.count};
	const auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(l.blocks), dim3(l.threads), l.lds, stream, p); };
	switch (v.kernel) {
		case TraceKernel::TWO_LEVEL_PACKET: dispatch([&](auto A) { go(trace_two_level_packet_kernel<A>); }, a); break;
		case TraceKernel::TWO_LEVEL: dispatch([&](auto A) { go(trace_two_level_kernel<A>); }, a); break;
#ifdef MRT_WITH_QUAD
		case TraceKernel::PACKET_QUAD: dispatch([&](auto C, auto A) { go(trace_packet_quad_kernel<A, C>); }, c, a); break;
#endif
		case TraceKernel::PACKET_ROWS:
			if (v.packets == 2u)
				dispatch([&](auto W, auto F, auto C, auto A) { go(trace_packet_rows_kernel<A, C, 2, W, F>); },
						Among<64, MRT_ROWS_WG_LARGE>{(int)v.wg}, Bool{v.cull}, c, a);
			else dispatch([&](auto C, auto A) { go(trace_packet_rows_kernel<A, C, 1, MRT_WG, false>); }, c, a);
			break;
		case TraceKernel::PACKET_ASM:
			dispatch([&](auto C, auto KPF, auto A) { if constexpr (!(C && KPF)) go(trace_packet_asm_kernel<A, C, KPF>); }, c, Bool{v.prefetch}, a);
			break;
		case TraceKernel::PACKET: dispatch([&](auto A, auto C) { go(trace_packet_kernel<A, C>); }, a, c); break;
		case TraceKernel::LANE: dispatch([&](auto A, auto C) { go(trace_lane_kernel<A, C>); }, a, c); break;
		default: return hipErrorInvalidValue; // (resolve_trace names no other; the persistent walk is launch_trace_persistent's)
	}
	format_variant(g_variant, sizeof(g_variant), v);
	return hipGetLastError();
}

static PersistParams persist_params(const TraceParams &p, unsigned long long *next_ray, uint32_t *overflow,
		uint32_t lds_depth, uint32_t refill, uint32_t leaf_wait, uint32_t blocks)
{
	PersistParams q;
	q.next_ray = next_ray; q.overflow = overflow; q.overflow_stride = blocks * MRT_WG;
	q.lds_depth = lds_depth; q.refill = refill; q.leaf_wait = leaf_wait ? leaf_wait : 1u;
	// about 32 chunks per wave, between one wave's worth of rays and MRT_RAY_CHUNK
	const uint64_t per_wave = p.count / ((uint64_t)blocks * (MRT_WG / MRT_WAVE)) / 32u;
	q.chunk = per_wave >= MRT_RAY_CHUNK ? MRT_RAY_CHUNK : (per_wave <= MRT_WAVE ? MRT_WAVE : (uint32_t)(per_wave & ~63ull));
	return q;
}

// Persistent lane kernel: `blocks` workgroups stay resident and pull rays from *next_ray (resolve_persistent: which walk).
hipError_t launch_trace_persistent(const TraceParams &p, unsigned long long *next_ray, uint32_t *overflow,
		uint32_t lds_depth, uint32_t refill, uint32_t leaf_wait, uint32_t blocks, bool any_hit, bool count, hipStream_t stream)
{
	const TraceLaunch l = resolve_persistent(p, lds_depth, blocks, any_hit, count);
	if (l.blocks == 0) return hipSuccess;
	const PersistParams q = persist_params(p, next_ray, overflow, lds_depth, refill, leaf_wait, blocks);
	const TraceVariant &v = l.v;
	dispatch([&](auto TL, auto C, auto W, auto A) {
		if constexpr (!TL || (W != 4 && !C)) // (the two-level walk is 8- or 2-wide and does not count)
			hipLaunchKernelGGL((trace_lane_persistent_kernel<A, W, TL, C>), dim3(l.blocks), dim3(l.threads), l.lds, stream, p, q);
	}, Bool{v.two_level}, Bool{v.count}, Among<8, 4, 2>{v.width}, Bool{v.any_hit});
	format_variant(g_variant, sizeof(g_variant), v);
	return hipGetLastError();
}

// Record-driven casts: p.kernel is the lane kernel the plan chose (launch_policy.cpp plan_source); p.count = entries.  persistent:
// blocks != 0 (as launch_trace_persistent), else the plain kernel with p.sparse_lanes (resolve_source).  src = one of the family's
// three sources; any_hit = a mode the family has (shadows, selected, to an emitter or neither, any-hit, reflections and bounces closest-hit, hemispheres either: the other
// instantiations do not compile, source_entry).  Anything else is hipErrorInvalidValue.
template <class S>
hipError_t launch_source(const TraceParams &p, const void *params, int src, bool any_hit, unsigned long long *next_ray, uint32_t *overflow,
		uint32_t lds_depth, uint32_t refill, uint32_t leaf_wait, uint32_t blocks, hipStream_t stream)
{
	using F = SourceFamily<S>;
	const S &s = *static_cast<const S *>(params);
	const TraceLaunch l = resolve_source(p, lds_depth, blocks, any_hit);
	if (l.error) return hipErrorInvalidValue;
	if (l.blocks == 0) return hipSuccess;
	if ((src != F::ray32 && src != F::host && src != F::grid) || !(any_hit ? F::any_hit : F::nearest)) return hipErrorInvalidValue;
	const TraceVariant &v = l.v;
	const dim3 grid(l.blocks), wg(l.threads);
	const PersistParams q = blocks ? persist_params(p, next_ray, overflow, lds_depth, refill, leaf_wait, blocks) : PersistParams{};
	dispatch([&](auto A, auto SRC, auto TL, auto W) {
		if constexpr ((A ? F::any_hit : F::nearest) && (!TL || W != 4)) { // (the plain kernels take neither TL nor W: a variant's defaults)
			if (v.kernel == TraceKernel::TWO_LEVEL) hipLaunchKernelGGL((trace_source_two_level_kernel<S, SRC, A>), grid, wg, l.lds, stream, p, s);
			else if (v.kernel == TraceKernel::LANE) hipLaunchKernelGGL((trace_source_lane_kernel<S, SRC, A>), grid, wg, l.lds, stream, p, s);
			else hipLaunchKernelGGL((trace_source_persistent_kernel<S, SRC, A, W, TL>), grid, wg, l.lds, stream, p, q, s);
		}
	}, Bool{any_hit}, Among<F::ray32, F::host, F::grid>{src}, Bool{v.two_level}, Among<8, 4, 2>{v.width});
	format_variant(g_variant, sizeof(g_variant), v, F::name, src, F::any_hit && F::nearest);
	return hipGetLastError();
}
template hipError_t launch_source<ShadowParams>(const TraceParams &, const void *, int, bool, unsigned long long *, uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t);
template hipError_t launch_source<SelectShadowParams>(const TraceParams &, const void *, int, bool, unsigned long long *, uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t);
template hipError_t launch_source<ReflectParams>(const TraceParams &, const void *, int, bool, unsigned long long *, uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t);
template hipError_t launch_source<HemiParams>(const TraceParams &, const void *, int, bool, unsigned long long *, uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t);
template hipError_t launch_source<BounceParams>(const TraceParams &, const void *, int, bool, unsigned long long *, uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t);
template hipError_t launch_source<GBufferParams>(const TraceParams &, const void *, int, bool, unsigned long long *, uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t);
template hipError_t launch_source<EmitterShadowParams>(const TraceParams &, const void *, int, bool, unsigned long long *, uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t);

} // namespace mrt
