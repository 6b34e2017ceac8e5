// api.hip — the C-ABI of include/mrt_hip.h: context, scene upload and build, the small entry points (the casts: cast.hip).
//
// Mirrors GPURayCaster (src/gpu/gpu_ray_caster.{h,cpp}) and the GPU half of
// RayDispatcher's policy (src/dispatch/ray_dispatcher.h:124-356): grow-only
// per-dispatch buffers (cpp:776-817), one pending async dispatch (cpp:538),
// upload drains a pending dispatch (cpp:198-202), Morton sort for incoherent
// batches of >= 256 rays (ray_dispatcher.h:135,427) — the sort, the gather and
// the unshuffle all run on the device (radix sort + permuted load/store inside
// the trace kernel) instead of std::sort + three host copies.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <new>
#include <thread>
#include <vector>
#include <hip/hip_runtime.h>
#include "mrt_context.h"

size_t ray_stride(uint32_t flags) { return (flags & MRT_FLAG_HOST_LAYOUT) ? sizeof(mrt_host_ray60) : sizeof(mrt_ray32); }
// hit tokens: 4 bytes (flat scenes: the winning triangle's slot), 8 for a two-level scene ({triangle slot, instance row})
size_t token_bytes(const mrt_ctx *ctx) { return ctx->two_level ? 8 : 4; }
size_t hit_stride(const mrt_ctx *ctx, uint32_t flags, int mode)
{
	if ((flags & MRT_FLAG_BOOL_OUT) && mode == MRT_MODE_ANY_HIT) return 1;
	if (flags & MRT_FLAG_TOKEN_OUT) return token_bytes(ctx);
	return (flags & MRT_FLAG_HOST_LAYOUT) ? sizeof(mrt_host_hit44) : sizeof(mrt_hit32);
}

uint32_t out_format(const mrt_ctx *ctx, uint32_t flags, int mode)
{
	if ((flags & MRT_FLAG_BOOL_OUT) && mode == MRT_MODE_ANY_HIT) return mrt::OUT_BOOL8;
	if (flags & MRT_FLAG_TOKEN_OUT) return ctx->two_level ? mrt::OUT_TOKEN8 : mrt::OUT_TOKEN4;
	return (flags & MRT_FLAG_HOST_LAYOUT) ? mrt::OUT_HOST44 : mrt::OUT_HIT32;
}

void base_params(mrt_ctx *ctx, mrt::TraceParams &p)
{
	std::memset(&p, 0, sizeof(p));
	p.nodes = ctx->d_nodes; p.nodes4 = ctx->d_nodes4; p.nodes8 = ctx->d_nodes8; p.leaf_box = ctx->d_leaf_box; p.instances = ctx->d_instances; p.tri_hot = ctx->d_hot; p.tri_cold = ctx->d_cold; p.row_array = ctx->d_rows; p.row_array4 = ctx->d_rows4; p.tri_unit_base4 = 2u * ctx->n_nodes4;
	p.stack_depth = ctx->stack_depth; p.n_tris = ctx->n_tris; p.n_nodes = ctx->n_nodes;
	p.n_instances = ctx->two_level ? ctx->two_level->n_inst : 0u;
	if (ctx->opts.stack_override >= ctx->depth && ctx->opts.stack_override <= 64) p.stack_depth = ctx->opts.stack_override;
	p.counters = ctx->d_counters;
	p.xcd_swizzle = ctx->opts.xcd_swizzle ? 1 : 0;
	p.tile_w_log2 = mrt::tile_w_log2(ctx->opts);
	// Z-order tiles keep the packets in flight on a compact image region.  That pays once the scene no longer
	// fits the 256 MB Infinity Cache (C5, 1.3 GB of nodes + triangles: 24.6 -> 23.5 ms) and costs 3-5 % while it
	// does (C2, C3), so the default goes by the size of the scene.
	const size_t scene_bytes = (size_t)ctx->n_nodes * sizeof(mrt::DevNode) + (size_t)ctx->n_tris * (sizeof(mrt::TriHot) + sizeof(mrt::TriCold));
	p.tile_order = ctx->opts.tile_order == 2 || (ctx->opts.tile_order == 0 && scene_bytes > (size_t)256 << 20) ? 1u : 0u;
	if (ctx->opts.tile_order == 3) p.tile_order = 2u; // 32x32-tile super-tiles (C5: 23.3 against 23.5 ms; not the default)
	if (ctx->opts.tile_order == 4) p.tile_order = 3u; // column strips per XCD (device_common.h, xcd_strips)
	p.extra_lds = ctx->opts.extra_lds <= 60000u ? ctx->opts.extra_lds : 60000u;
	p.count_mode = ctx->opts.count_visits;
	// packet-level frustum culling in the 128-ray walk (packet_rows_kernel.h): 0 off, 1 on, 2 = by where the rays come from
	// (launch_trace): on for rays generated in the kernel (C3 1.84 against 1.86 ms, C5 20.4 against 21.1), off for rays read from
	// memory, where the walk with the scalar-cache prefetch waits less (C3 1.89 against 1.93 ms; profiles/r03_cull_cast_vs_fused.txt)
	p.rows_cull = ctx->opts.packet_cull == 1u ? 0u : (ctx->opts.packet_cull == 2u ? 1u : 2u);
	p.scene_abs_max = 0.0f;
	for (int c = 0; c < 3; c++) p.scene_abs_max = std::fmax(p.scene_abs_max, std::fmax(std::fabs(ctx->bounds_lo[c]), std::fabs(ctx->bounds_hi[c])));
	p.rows_wg = ctx->opts.packet_wg == 64u || ctx->opts.packet_wg == 256u ? ctx->opts.packet_wg : (scene_bytes > (size_t)256 << 20 ? 256u : 64u);
	p.kernel = MRT_KERNEL_LANE; // the cast's plan picks per batch (launch_policy.cpp)
}

int grid_params(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1, mrt::TraceParams &p)
{
	if (!cam || grid_w == 0 || grid_h == 0 || y0 > y1 || y1 > grid_h) return fail(ctx, MRT_ERR_INVALID, "bad grid");
	if (cam->kind > MRT_CAMERA_ORTHOGRAPHIC) return fail(ctx, MRT_ERR_INVALID, "bad camera kind");
	// RayCamera::generate_rays asserts the resolution the camera was set up for (ray_camera.h:150-152)
	if (cam->kind != MRT_CAMERA_DEBUG_GRID && (cam->inv_w != 1.0f / (float)grid_w || cam->inv_h != 1.0f / (float)grid_h))
		return fail(ctx, MRT_ERR_INVALID, "camera was set up for another resolution");
	base_params(ctx, p);
	p.cam = *cam; p.grid_w = grid_w; p.grid_h = grid_h; p.y0 = y0; p.rows = y1 - y0;
	p.tiles_x = (grid_w + (1u << p.tile_w_log2) - 1u) >> p.tile_w_log2;
	p.count = (uint64_t)grid_w * (y1 - y0);
	p.in_fmt = mrt::IN_GRID;
	return MRT_OK;
}

void free_scene(mrt_ctx *ctx)
{
	if (ctx->d_nodes) (void)hipFree(ctx->d_nodes);
	if (ctx->d_hot) (void)hipFree(ctx->d_hot);
	if (ctx->d_cold) (void)hipFree(ctx->d_cold);
	if (ctx->d_nodes4) (void)hipFree(ctx->d_nodes4);
	if (ctx->d_nodes8) (void)hipFree(ctx->d_nodes8);
	if (ctx->d_leaf_box) (void)hipFree(ctx->d_leaf_box);
	ctx->d_leaf_box = nullptr;
	if (ctx->d_rows) (void)hipFree(ctx->d_rows);
	ctx->d_rows = nullptr;
	if (ctx->d_rows4) (void)hipFree(ctx->d_rows4);
	ctx->d_rows4 = nullptr;
	if (ctx->d_instances) (void)hipFree(ctx->d_instances);
	ctx->d_instances = nullptr;
	if (ctx->two_level) { mrt::free_two_level(ctx->two_level); delete ctx->two_level; ctx->two_level = nullptr; }
	if (ctx->d_slot_src) (void)hipFree(ctx->d_slot_src);
	if (ctx->d_parent) (void)hipFree(ctx->d_parent);
	ctx->d_slot_src = nullptr; ctx->d_parent = nullptr;
	release(ctx->tlas_inst_tab); release(ctx->tlas_blas_tab); // the device top level's tables (tlas_device.hip) belong to the scene
	ctx->tlas_inst_ok = ctx->tlas_blas_ok = false;
	ctx->d_nodes = nullptr; ctx->d_hot = nullptr; ctx->d_cold = nullptr; ctx->d_nodes4 = nullptr; ctx->d_nodes8 = nullptr;
	ctx->n_nodes8 = ctx->stack8 = 0;
	ctx->scene = false; ctx->n_nodes = ctx->n_tris = 0;
	for (int k = 0; k < mrt::GridStates::kCount; k++) { // what was learnt about the old scene's grids
		ctx->sched[k].forget(); ctx->grids.e[k].tune.phase = 0; ctx->grids.e[k].tune.mode = -1;
	}
}

namespace {

// Flat scenes: the unified row array of the assembly packet walk, built on the device from the arrays just
// uploaded / built.  Optional: a scene too large for its 26-bit row index, or a device short of memory, goes
// without (coherent batches then take trace_packet_asm_kernel).
int build_rows(mrt_ctx *ctx)
{
	// the 4-wide rows: when the 4-wide layout is resident and its worst-case stack fits the wave's 64 entries
	const bool wanted4 = ctx->opts.kernel == MRT_KERNEL_PACKET_QUAD && mrt::quad_kernel_built(); // (AUTO never picks the four-wide walk: it is no faster)
	const uint64_t n_units4 = (uint64_t)2u * ctx->n_nodes4 + ctx->n_tris;
	if (wanted4 && ctx->d_nodes4 && ctx->n_nodes4 && ctx->stack4 <= 64u && n_units4 < mrt::kAsmNodeLimit) {
		if (hipMalloc(&ctx->d_rows4, (size_t)n_units4 * 64u) != hipSuccess) { ctx->d_rows4 = nullptr; (void)hipGetLastError(); }
		else {
			HIP_TRY(ctx, mrt::launch_build_rows4(ctx->d_nodes4, ctx->d_hot, ctx->d_cold, ctx->n_nodes4, ctx->n_tris, ctx->d_rows4, ctx->stream));
			HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		}
	}
	const bool wanted = ctx->opts.kernel == MRT_KERNEL_AUTO || ctx->opts.kernel == MRT_KERNEL_PACKET_DUAL || ctx->opts.kernel == MRT_KERNEL_PACKET_ROWS;
	const uint64_t n_rows = (uint64_t)ctx->n_nodes + ctx->n_tris;
	if (!wanted || n_rows >= mrt::kAsmNodeLimit) return MRT_OK;
	if (hipMalloc(&ctx->d_rows, (size_t)n_rows * 64u) != hipSuccess) { ctx->d_rows = nullptr; (void)hipGetLastError(); return MRT_OK; }
	HIP_TRY(ctx, mrt::launch_build_rows(ctx->d_nodes, ctx->d_hot, ctx->d_cold, ctx->n_nodes, ctx->n_tris, ctx->d_rows, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return MRT_OK;
}

int drain_pending(mrt_ctx *ctx)
{
	if (ctx->pending) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); ctx->pending = false; }
	return MRT_OK;
}

} // namespace

extern "C" {

uint32_t mrt_version(void) { return (MRT_VERSION_MAJOR << 16) | MRT_VERSION_MINOR; }

uint32_t mrt_struct_size(uint32_t which)
{
	switch (which) {
		case 0: return (uint32_t)sizeof(mrt_options);
		case 1: return (uint32_t)sizeof(mrt_camera);
		case 2: return (uint32_t)sizeof(mrt_stats);
		case 3: return (uint32_t)sizeof(mrt_instance);
		case 4: return (uint32_t)sizeof(mrt_light);
		case 6: return (uint32_t)sizeof(mrt_material); // (5: not a struct)
		case 7: return (uint32_t)sizeof(mrt_shade_data);
		case 8: return (uint32_t)sizeof(mrt_surface64);
		case 9: return (uint32_t)sizeof(mrt_surface_out);
		case 11: return (uint32_t)sizeof(mrt_shade_light); // (10: not a struct)
		case 12: return (uint32_t)sizeof(mrt_environment);
		case 13: return (uint32_t)sizeof(mrt_light_out);
		case 15: return (uint32_t)sizeof(mrt_path_state); // (14: not a struct)
		case 16: return (uint32_t)sizeof(mrt_path_step_desc);
		case 18: return (uint32_t)sizeof(mrt_texture); // (17: not a struct)
		case 19: return (uint32_t)sizeof(mrt_material_textures);
		case 20: return (uint32_t)sizeof(mrt_texture_set);
		case 22: return (uint32_t)sizeof(mrt_panorama); // (21: not a struct)
		case 24: return (uint32_t)sizeof(mrt_channel_out); // (23: not a struct)
		case 26: return (uint32_t)sizeof(mrt_accum_state); // (25: not a struct)
		case 28: return (uint32_t)sizeof(mrt_denoise_params); // (27: not a struct)
		case 30: return (uint32_t)sizeof(mrt_gbuffer); // (29: not a struct)
		case 32: return (uint32_t)sizeof(mrt_svgf_params); // (31: not a struct)
		case 34: return (uint32_t)sizeof(mrt_light_select); // (33: not a struct)
		case 36: return (uint32_t)sizeof(mrt_emitter_select); // (35: not a struct)
		case 38: return (uint32_t)sizeof(mrt_emitter64); // (37: not a struct)
		default: return 0u;
	}
}

const char *mrt_status_string(int s)
{
	switch (s) {
		case MRT_OK: return "ok";
		case MRT_ERR_INVALID: return "invalid argument";
		case MRT_ERR_NO_DEVICE: return "no such HIP device";
		case MRT_ERR_HIP: return "HIP runtime error";
		case MRT_ERR_NO_SCENE: return "no scene uploaded";
		case MRT_ERR_PENDING: return "an async dispatch is already pending";
		case MRT_ERR_NOT_PENDING: return "no async dispatch pending";
		case MRT_ERR_OOM: return "out of memory";
		case MRT_ERR_UNSUPPORTED: return "unsupported";
		case MRT_ERR_BAD_BVH: return "BVH failed validation";
		default: return "unknown status";
	}
}

const char *mrt_kernel_name(uint32_t kernel)
{
	switch (kernel) {
		case MRT_KERNEL_LANE: return "trace_lane_kernel";
		case MRT_KERNEL_PACKET: return "trace_packet_kernel";
		case MRT_KERNEL_PACKET_ASM: return "trace_packet_asm_kernel";
		case MRT_KERNEL_PACKET_DUAL: return "trace_packet_rows_kernel<2>";
		case MRT_KERNEL_PACKET_ROWS: return "trace_packet_rows_kernel<1>";
		case MRT_KERNEL_PACKET_QUAD: return "trace_packet_quad_kernel";
		case MRT_KERNEL_LANE_PERSISTENT: return "trace_lane_persistent_kernel<2>";
		case MRT_KERNEL_LANE4_PERSISTENT: return "trace_lane_persistent_kernel<4>";
		case MRT_KERNEL_LANE8_PERSISTENT: return "trace_lane_persistent_kernel<8>";
		case MRT_KERNEL_TWO_LEVEL: return "trace_two_level_kernel";
		case MRT_KERNEL_TWO_LEVEL_PACKET: return "trace_two_level_packet_kernel";
		case MRT_KERNEL_TWO_LEVEL_PERSISTENT: return "trace_lane_persistent_kernel<2, two-level>";
		case MRT_KERNEL_TWO_LEVEL_PERSISTENT8: return "trace_lane_persistent_kernel<8, two-level>";
		default: return "?";
	}
}

// 1 if this build of the library contains the kernel (everything but MRT_KERNEL_PACKET_QUAD always; the four-wide packet
// walk only in builds made with MRT_WITH_QUAD)
int mrt_kernel_available(uint32_t kernel)
{
	if (kernel == MRT_KERNEL_PACKET_QUAD) return mrt::quad_kernel_built() ? 1 : 0;
	return std::strcmp(mrt_kernel_name(kernel), "?") != 0 || kernel == MRT_KERNEL_AUTO ? 1 : 0;
}

const char *mrt_last_error(const mrt_ctx *ctx) { return ctx ? ctx->err : "null context"; }

int mrt_create(int device_ordinal, const mrt_options *opts, mrt_ctx **out)
{
	if (!out) return MRT_ERR_INVALID;
	*out = nullptr;
	if (opts && opts->struct_size != sizeof(mrt_options)) return MRT_ERR_INVALID;
	if (opts && opts->kernel == MRT_KERNEL_PACKET_QUAD && !mrt::quad_kernel_built()) return MRT_ERR_UNSUPPORTED; // not in this build (MRT_WITH_QUAD)
	if (opts && ((opts->packet_wg != 0u && opts->packet_wg != 64u && opts->packet_wg != 256u) || opts->packet_cull > 2u || opts->tile_schedule > 2u || opts->kernel > MRT_KERNEL_PACKET_QUAD || opts->kernel == 3u || opts->kernel == 4u)) return MRT_ERR_INVALID; // 3, 4: retired ids
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || device_ordinal < 0 || device_ordinal >= n) return MRT_ERR_NO_DEVICE;
	mrt_ctx *ctx = new (std::nothrow) mrt_ctx();
	if (!ctx) return MRT_ERR_OOM;
	ctx->device = device_ordinal;
	if (opts) ctx->opts = *opts;
	ctx->opts.struct_size = sizeof(mrt_options);
	// tuning knobs of the tile schedule (tools/bench_resolutions.py; the tests schedule smaller grids): read once, here
	if (const char *e = std::getenv("MRT_SCHEDULE_MIN_LOG2")) {
		const int k = std::atoi(e);
		ctx->knobs.schedule_min_rays = ctx->knobs.tune_min_rays = 1ull << (k >= 12 && k <= 24 ? k : 17);
	}
	if (const char *e = std::getenv("MRT_SCHED_SPLIT_PCT")) { const int v = std::atoi(e); if (v >= 0 && v <= 50) ctx->knobs.split_pct = (uint32_t)v; }
	ctx->knobs.dump = std::getenv("MRT_SCHED_DUMP") != nullptr;
	ctx->knobs.poison = std::getenv("MRT_POISON_OUTPUT") != nullptr;
	auto bail = [&](int code) { mrt_destroy(ctx); return code; };
	if (hipSetDevice(device_ordinal) != hipSuccess) return bail(MRT_ERR_NO_DEVICE);
	if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) return bail(MRT_ERR_HIP);
	{
		int cus = 0;
		if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_ordinal) == hipSuccess && cus > 0) ctx->cu_count = cus;
	}
	ctx->stream = ctx->own_stream;
	for (auto &e : ctx->ev) if (hipEventCreate(&e) != hipSuccess) return bail(MRT_ERR_HIP);
	// visit counters, detected grid, detect_grid_kernel scratch, ray counters: the layout is in mrt_internal.h
	if (hipMalloc(&ctx->d_counters, mrt::kCounterWords * sizeof(unsigned long long)) != hipSuccess) return bail(MRT_ERR_OOM);
	if (hipMemset(ctx->d_counters, 0, mrt::kCounterWords * sizeof(unsigned long long)) != hipSuccess) return bail(MRT_ERR_HIP);
	if (hipHostMalloc((void **)&ctx->h_auto, 64, hipHostMallocMapped) != hipSuccess) return bail(MRT_ERR_OOM);
	std::memset(ctx->h_auto, 0, 64);
	if (hipHostGetDevicePointer((void **)&ctx->d_auto_host, ctx->h_auto, 0) != hipSuccess) return bail(MRT_ERR_HIP);
	*out = ctx;
	return MRT_OK;
}

void mrt_destroy(mrt_ctx *ctx)
{
	if (!ctx) return;
	(void)hipSetDevice(ctx->device);
	if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
	free_scene(ctx);
	release(ctx->rays); release(ctx->hits); release(ctx->keys_in); release(ctx->keys_out);
	release(ctx->idx_in); release(ctx->idx_out); release(ctx->sort_tmp); release(ctx->overflow); release(ctx->refit_in);
	release(ctx->tlas_work);
	release(ctx->shade_rows); release(ctx->shade_materials);
	release(ctx->tex_texels); release(ctx->tex_table); release(ctx->tex_bindings); release(ctx->tex_tangents);
	release(ctx->pano_texels);
	release(ctx->emit_rows); release(ctx->emit_cdf); release(ctx->emit_in); release(ctx->emit_work);
	for (auto &sc : ctx->sched) {
		if (sc.side) { (void)hipStreamSynchronize(sc.side); (void)hipStreamDestroy(sc.side); }
		if (sc.traced) (void)hipEventDestroy(sc.traced);
		for (int k = 0; k < 2; k++) { if (sc.ready[k]) (void)hipEventDestroy(sc.ready[k]); release(sc.cost[k]); release(sc.order[k]); release(sc.slots[k]); release(sc.hdr[k]); }
		release(sc.cost_sorted); release(sc.iota); release(sc.tmp);
	}
	if (ctx->d_counters) (void)hipFree(ctx->d_counters);
	if (ctx->build_arena.ptr) (void)hipFree(ctx->build_arena.ptr);
	if (ctx->build_arena.pinned) (void)hipHostFree(ctx->build_arena.pinned);
	if (ctx->h_auto) (void)hipHostFree(ctx->h_auto);
	if (ctx->h_small_in) (void)hipHostFree(ctx->h_small_in);
	if (ctx->h_small_out) (void)hipHostFree(ctx->h_small_out);
	for (auto &e : ctx->ev) if (e) (void)hipEventDestroy(e);
	for (auto &e : ctx->pipe_ev) (void)hipEventDestroy(e);
	if (ctx->up_stream) (void)hipStreamDestroy(ctx->up_stream);
	if (ctx->dn_stream) (void)hipStreamDestroy(ctx->dn_stream);
	if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
	delete ctx;
}

int mrt_set_stream(mrt_ctx *ctx, void *hip_stream)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "cannot switch streams with a dispatch pending");
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
	return MRT_OK;
}

int mrt_synchronize(mrt_ctx *ctx)
{
	if (!ctx) return MRT_ERR_INVALID;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	ctx->detect.waited(ctx->h_auto);
	return MRT_OK;
}

int mrt_upload_scene(mrt_ctx *ctx, const mrt_tri64 *tris, uint32_t n_tris,
		const mrt_bvh_node32 *nodes, uint32_t used_nodes, const uint32_t *prim_idx)
{
	if (!ctx) return MRT_ERR_INVALID;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = drain_pending(ctx); // gpu_ray_caster.cpp:198-202
	if (rc) return rc;
	mrt::DeviceSceneHost h;
	h.want8 = ctx->opts.kernel == MRT_KERNEL_LANE8_PERSISTENT || ctx->opts.kernel == MRT_KERNEL_AUTO;
	rc = mrt::prepare_scene(tris, n_tris, nodes, used_nodes, prim_idx, &h, ctx->err, sizeof(ctx->err));
	if (rc) return rc;
	auto cleanup = [&] { std::free(h.nodes); std::free(h.nodes4); std::free(h.nodes8); std::free(h.leaf_box); std::free(h.hot); std::free(h.cold); };
	if (h.depth > 64 || h.stack4 > 128) { cleanup(); return fail(ctx, MRT_ERR_UNSUPPORTED, "BVH deeper than the 64-entry traversal stack"); }
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	free_scene(ctx);
	hipError_t e;
	// the 4-wide layout is resident only when a kernel that walks it is asked for
	const bool want4 = ctx->opts.kernel == MRT_KERNEL_LANE4_PERSISTENT || ctx->opts.kernel == MRT_KERNEL_PACKET_QUAD || ctx->opts.kernel == MRT_KERNEL_AUTO;
	if ((e = hipMalloc(&ctx->d_nodes, (size_t)h.n_nodes * sizeof(mrt::DevNode))) != hipSuccess ||
			// +16 B of slack: a 64-B scalar fetch at the last 48-B triangle stays inside the allocation
			(e = hipMalloc(&ctx->d_hot, (size_t)h.n_tris * sizeof(mrt::TriHot) + 16)) != hipSuccess ||
			(e = hipMalloc(&ctx->d_cold, (size_t)h.n_tris * sizeof(mrt::TriCold))) != hipSuccess ||
			(want4 && (e = hipMalloc(&ctx->d_nodes4, (size_t)h.n_nodes4 * sizeof(mrt::Dev4Node))) != hipSuccess) ||
			(h.nodes8 && ((e = hipMalloc(&ctx->d_nodes8, (size_t)h.n_nodes8 * sizeof(mrt::Dev8Node))) != hipSuccess ||
					(e = hipMalloc(&ctx->d_leaf_box, (size_t)h.n_tris * 32)) != hipSuccess)) ||
			(e = hipMalloc(&ctx->d_slot_src, (size_t)h.n_tris * 4)) != hipSuccess) {
		cleanup(); free_scene(ctx);
		return fail(ctx, MRT_ERR_OOM, "scene does not fit in device memory");
	}
	e = hipMemcpy(ctx->d_nodes, h.nodes, (size_t)h.n_nodes * sizeof(mrt::DevNode), hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMemcpy(ctx->d_hot, h.hot, (size_t)h.n_tris * sizeof(mrt::TriHot), hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMemcpy(ctx->d_cold, h.cold, (size_t)h.n_tris * sizeof(mrt::TriCold), hipMemcpyHostToDevice);
	if (e == hipSuccess && want4) e = hipMemcpy(ctx->d_nodes4, h.nodes4, (size_t)h.n_nodes4 * sizeof(mrt::Dev4Node), hipMemcpyHostToDevice);
	if (e == hipSuccess && h.nodes8) e = hipMemcpy(ctx->d_nodes8, h.nodes8, (size_t)h.n_nodes8 * sizeof(mrt::Dev8Node), hipMemcpyHostToDevice);
	if (e == hipSuccess && h.nodes8) e = hipMemcpy(ctx->d_leaf_box, h.leaf_box, (size_t)h.n_tris * 32, hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMemcpy(ctx->d_slot_src, prim_idx, (size_t)h.n_tris * 4, hipMemcpyHostToDevice); // slot k holds triangle prim_idx[k]
	ctx->n_nodes4 = want4 ? h.n_nodes4 : 0;
	ctx->n_nodes8 = h.nodes8 ? h.n_nodes8 : 0; ctx->stack8 = h.stack8;
	for (int c = 0; c < 3; c++) { ctx->bounds_lo[c] = h.bounds_lo[c]; ctx->bounds_hi[c] = h.bounds_hi[c]; }
	cleanup();
	if (e != hipSuccess) { free_scene(ctx); std::snprintf(ctx->err, sizeof(ctx->err), "scene upload failed: %s", hipGetErrorString(e)); return MRT_ERR_HIP; }
	ctx->n_nodes = h.n_nodes; ctx->n_tris = h.n_tris; ctx->depth = h.depth; ctx->stack4 = h.stack4;
	// LDS stack entries per lane: what this BVH can need, rounded up to 8, at most 64.
	ctx->stack_depth = ((h.depth + 7u) / 8u) * 8u;
	if (ctx->stack_depth < 8) ctx->stack_depth = 8;
	if ((rc = build_rows(ctx))) { free_scene(ctx); return rc; }
	ctx->scene = true;
	return MRT_OK;
}

int mrt_build_scene_device(mrt_ctx *ctx, const mrt_tri64 *tris, uint32_t n_tris, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!tris || n_tris == 0) return fail(ctx, MRT_ERR_INVALID, "build_scene_device: no triangles");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	int rc = drain_pending(ctx);
	if (rc) return rc;
	const bool on_device = (flags & MRT_BUILD_TRIS_ON_DEVICE) != 0;
	if (n_tris < 2) {
		// a one-triangle scene has no radix tree: the host path wraps the root leaf (scene_prep.cpp)
		mrt_tri64 t;
		if (on_device) { // read in stream order: the caller's work on the context's stream may still be writing the triangle
			HIP_TRY(ctx, hipMemcpyAsync(&t, tris, sizeof(t), hipMemcpyDeviceToHost, ctx->stream));
			HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		} else t = tris[0];
		float verts[12] = { t.v0[0], t.v0[1], t.v0[2], 0.0f, t.v0[0] + t.edge1[0], t.v0[1] + t.edge1[1], t.v0[2] + t.edge1[2], 0.0f,
			t.v0[0] + t.edge2[0], t.v0[1] + t.edge2[1], t.v0[2] + t.edge2[2], 0.0f };
		mrt_bvh_node32 nodes[2]; uint32_t prim = 0, used = 0;
		if ((rc = mrt_bvh2_build(verts, 1, nodes, &prim, &used, 1))) return fail(ctx, rc, "build_scene_device: host build failed");
		return mrt_upload_scene(ctx, &t, 1, nodes, used, &prim);
	}
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	hipEvent_t e0 = ctx->ev[0], e1 = ctx->ev[1];
	HIP_TRY(ctx, hipEventRecord(e0, ctx->stream));
	const mrt_tri64 *d_tris = tris;
	void *staged = nullptr;
	if (!on_device) {
		if (hipMalloc(&staged, (size_t)n_tris * sizeof(mrt_tri64)) != hipSuccess) return fail(ctx, MRT_ERR_OOM, "scene does not fit in device memory");
		hipError_t e = hipMemcpyAsync(staged, tris, (size_t)n_tris * sizeof(mrt_tri64), hipMemcpyHostToDevice, ctx->stream);
		if (e != hipSuccess) { (void)hipFree(staged); return fail(ctx, MRT_ERR_HIP, hipGetErrorString(e)); }
		d_tris = (const mrt_tri64 *)staged;
	}
	mrt::DeviceBuildResult b;
	if (hipMalloc(&b.slot_src, (size_t)n_tris * 4) != hipSuccess) {
		if (staged) (void)hipFree(staged);
		return fail(ctx, MRT_ERR_OOM, "scene does not fit in device memory");
	}
	const bool want4 = ctx->opts.kernel == MRT_KERNEL_LANE4_PERSISTENT || ctx->opts.kernel == MRT_KERNEL_PACKET_QUAD || ctx->opts.kernel == MRT_KERNEL_AUTO;
	const bool want8 = ctx->opts.kernel == MRT_KERNEL_LANE8_PERSISTENT || ctx->opts.kernel == MRT_KERNEL_AUTO;
	rc = mrt::device_build_lbvh(d_tris, n_tris, want4, want8, (flags & MRT_BUILD_SAFE_HANDOFF) != 0, (flags & MRT_BUILD_SAH) ? 2 : (flags & MRT_BUILD_PLOC) ? 1 : 0, &ctx->build_arena, (void *)ctx->stream, &b,
			ctx->err, sizeof(ctx->err));
	if (staged) (void)hipFree(staged);
	if (rc) { (void)hipFree(b.slot_src); return rc; }
	auto drop_build = [&] { // the build's arrays are ours until the context takes them over below
		(void)hipFree(b.nodes); (void)hipFree(b.hot); (void)hipFree(b.cold); (void)hipFree(b.slot_src);
		if (b.nodes4) (void)hipFree(b.nodes4);
		if (b.nodes8) (void)hipFree(b.nodes8);
		if (b.leaf_box) (void)hipFree(b.leaf_box);
	};
	if (b.depth > 64) { // the packet kernels keep 64 stack entries per wave
		drop_build();
		return fail(ctx, MRT_ERR_UNSUPPORTED, "device-built BVH deeper than the 64-entry traversal stack: build on the host");
	}
	float ms = 0.0f;
	hipError_t te = hipEventRecord(e1, ctx->stream);
	if (te == hipSuccess) te = hipEventSynchronize(e1);
	if (te == hipSuccess) te = hipEventElapsedTime(&ms, e0, e1);
	if (te != hipSuccess) { drop_build(); return fail(ctx, MRT_ERR_HIP, hipGetErrorString(te)); }
	free_scene(ctx);
	ctx->d_nodes = b.nodes; ctx->d_hot = b.hot; ctx->d_cold = b.cold; ctx->d_slot_src = b.slot_src;
	ctx->d_nodes4 = b.nodes4; ctx->n_nodes4 = b.nodes4 ? b.n_nodes : 0; ctx->stack4 = b.stack4;
	ctx->d_nodes8 = b.nodes8; ctx->d_leaf_box = b.leaf_box; ctx->n_nodes8 = b.nodes8 ? b.n_nodes : 0; ctx->stack8 = b.stack8;
	ctx->n_nodes = b.n_nodes; ctx->n_tris = b.n_tris; ctx->depth = b.depth;
	for (int c = 0; c < 3; c++) { ctx->bounds_lo[c] = b.bounds_lo[c]; ctx->bounds_hi[c] = b.bounds_hi[c]; }
	ctx->stack_depth = ((b.depth + 7u) / 8u) * 8u;
	if (ctx->stack_depth < 8) ctx->stack_depth = 8;
	ctx->stats.last_build_ms = ms;
	if ((rc = build_rows(ctx))) { free_scene(ctx); return rc; }
	ctx->scene = true;
	return MRT_OK;
}

// validates the instances, uploads what is on the host, flattens into d_out (device); *total = sum(n_tris)
static int flatten_instances(mrt_ctx *ctx, const float *verts9, uint32_t n_mesh_tris, const mrt_instance *instances,
		uint32_t n_instances, uint32_t flags, mrt_tri64 *d_out_or_null, mrt_tri64 **d_out_alloc, uint32_t *total)
{
	if (!verts9 || !instances || n_instances == 0) return fail(ctx, MRT_ERR_INVALID, "flatten_instances: no instances");
	std::vector<uint32_t> first(n_instances);
	uint64_t sum = 0; uint32_t max_tris = 0;
	for (uint32_t i = 0; i < n_instances; i++) {
		const mrt_instance &in = instances[i];
		if ((uint64_t)in.first_tri + in.n_tris > n_mesh_tris) return fail(ctx, MRT_ERR_INVALID, "flatten_instances: instance outside the mesh array");
		first[i] = (uint32_t)sum; sum += in.n_tris;
		if (in.n_tris > max_tris) max_tris = in.n_tris;
	}
	if (sum == 0 || sum > 0x7FFFFFFFull) return fail(ctx, MRT_ERR_INVALID, "flatten_instances: triangle count out of range");
	*total = (uint32_t)sum;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	void *d_inst = nullptr, *d_first = nullptr, *d_verts = nullptr, *d_out = d_out_or_null;
	auto drop = [&] {
		if (d_inst) (void)hipFree(d_inst);
		if (d_first) (void)hipFree(d_first);
		if (d_verts) (void)hipFree(d_verts);
	};
	const bool on_device = (flags & MRT_BUILD_TRIS_ON_DEVICE) != 0;
	hipError_t e = hipMalloc(&d_inst, (size_t)n_instances * sizeof(mrt_instance));
	if (e == hipSuccess) e = hipMalloc(&d_first, (size_t)n_instances * 4);
	if (e == hipSuccess && !on_device) e = hipMalloc(&d_verts, (size_t)n_mesh_tris * 36);
	if (e == hipSuccess && !d_out) { e = hipMalloc(&d_out, (size_t)sum * sizeof(mrt_tri64)); if (e == hipSuccess) *d_out_alloc = (mrt_tri64 *)d_out; }
	if (e != hipSuccess) { drop(); return fail(ctx, MRT_ERR_OOM, "flatten_instances: out of device memory"); }
	e = hipMemcpyAsync(d_inst, instances, (size_t)n_instances * sizeof(mrt_instance), hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess) e = hipMemcpyAsync(d_first, first.data(), (size_t)n_instances * 4, hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess && !on_device) e = hipMemcpyAsync(d_verts, verts9, (size_t)n_mesh_tris * 36, hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess) e = mrt::launch_flatten_instances(on_device ? verts9 : (const float *)d_verts, (const mrt_instance *)d_inst,
			(const uint32_t *)d_first, n_instances, max_tris, (mrt_tri64 *)d_out, (void *)ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream); // `first` and the staging buffers go out of scope
	drop();
	if (e != hipSuccess) {
		if (*d_out_alloc) { (void)hipFree(*d_out_alloc); *d_out_alloc = nullptr; }
		std::snprintf(ctx->err, sizeof(ctx->err), "flatten_instances failed: %s", hipGetErrorString(e));
		return MRT_ERR_HIP;
	}
	return MRT_OK;
}

int mrt_flatten_instances(mrt_ctx *ctx, const float *verts9, uint32_t n_mesh_tris, const mrt_instance *instances,
		uint32_t n_instances, uint32_t flags, mrt_tri64 *d_out)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!d_out) return fail(ctx, MRT_ERR_INVALID, "flatten_instances: null output");
	mrt_tri64 *unused = nullptr; uint32_t total = 0;
	return flatten_instances(ctx, verts9, n_mesh_tris, instances, n_instances, flags, d_out, &unused, &total);
}

int mrt_build_instanced_scene_device(mrt_ctx *ctx, const float *verts9, uint32_t n_mesh_tris, const mrt_instance *instances,
		uint32_t n_instances, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	mrt_tri64 *d_world = nullptr; uint32_t total = 0;
	int rc = flatten_instances(ctx, verts9, n_mesh_tris, instances, n_instances, flags, nullptr, &d_world, &total);
	if (rc) return rc;
	rc = mrt_build_scene_device(ctx, d_world, total, MRT_BUILD_TRIS_ON_DEVICE | (flags & (MRT_BUILD_PLOC | MRT_BUILD_SAH | MRT_BUILD_SAFE_HANDOFF)));
	(void)hipFree(d_world);
	return rc;
}

// Device-built BLASes for a two-level scene: every distinct mesh goes through device_build_lbvh on its own and
// is moved to its place in the scene's arrays (node refs + node_base, leaf slots + tri_base).  h comes from
// prepare_two_level(build_blas = false); on success the device arrays of ctx hold every BLAS and h knows
// their boxes and depths.
static int build_blases_on_device(mrt_ctx *ctx, mrt::TwoLevelHost *h, const float *verts9, int form)
{
	uint32_t max_tris = 0;
	for (uint32_t k = 0; k < h->n_blas; k++) if (h->blas[k].n_tris > max_tris) max_tris = h->blas[k].n_tris;
	mrt_tri64 *staged = nullptr;
	if (hipMalloc(&staged, (size_t)max_tris * sizeof(mrt_tri64)) != hipSuccess) return fail(ctx, MRT_ERR_OOM, "scene does not fit in device memory");
	std::vector<mrt_tri64> tris(max_tris);
	uint32_t tri_base = 0;
	int rc = MRT_OK;
	for (uint32_t k = 0; k < h->n_blas && rc == MRT_OK; k++) {
		mrt::TwoLevelBlas &bl = h->blas[k];
		rc = mrt_make_triangles(verts9 + (size_t)9 * bl.first_tri, nullptr, nullptr, bl.n_tris, tris.data()); // mesh-local ids, all layers
		if (rc) { fail(ctx, rc, "two-level scene: bad mesh triangles"); break; }
		hipError_t e = hipMemcpy(staged, tris.data(), (size_t)bl.n_tris * sizeof(mrt_tri64), hipMemcpyHostToDevice);
		if (e != hipSuccess) { rc = fail(ctx, MRT_ERR_HIP, hipGetErrorString(e)); break; }
		mrt::DeviceBuildResult b;
		rc = mrt::device_build_lbvh(staged, bl.n_tris, false, h->wide8, false, form, &ctx->build_arena, (void *)ctx->stream, &b, ctx->err, sizeof(ctx->err));
		if (rc) break;
		e = mrt::launch_offset_refs(ctx->d_nodes + bl.root, b.nodes, b.n_nodes, bl.root, tri_base, (void *)ctx->stream);
		if (h->wide8 && !(b.nodes8 && b.leaf_box)) h->wide8 = false; // a mesh whose boxes fit no grid: the scene goes without the 8-wide layout
		if (h->wide8) {
			if (e == hipSuccess) e = mrt::launch_offset_refs8(ctx->d_nodes8 + bl.root8, b.nodes8, b.n_nodes, bl.root8, tri_base, (void *)ctx->stream);
			if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_leaf_box + (size_t)tri_base * 8, b.leaf_box, (size_t)bl.n_tris * 32, hipMemcpyDeviceToDevice, ctx->stream);
			bl.stack8 = b.stack8;
		}
		if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_hot + tri_base, b.hot, (size_t)bl.n_tris * sizeof(mrt::TriHot), hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_cold + tri_base, b.cold, (size_t)bl.n_tris * sizeof(mrt::TriCold), hipMemcpyDeviceToDevice, ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
		(void)hipFree(b.nodes); (void)hipFree(b.hot); (void)hipFree(b.cold);
		if (b.nodes8) (void)hipFree(b.nodes8);
		if (b.leaf_box) (void)hipFree(b.leaf_box);
		if (e != hipSuccess) { rc = fail(ctx, MRT_ERR_HIP, hipGetErrorString(e)); break; }
		// (the scene's node array holds n_tris - 1 rows per mesh: what the radix tree fills; the SAH form, with leaves of several triangles, fewer)
		if (b.n_nodes == 0u || b.n_nodes > bl.n_tris - 1u) { rc = fail(ctx, MRT_ERR_BAD_BVH, "two-level scene: unexpected BLAS size"); break; }
		bl.depth = b.depth; bl.n_nodes = b.n_nodes;
		for (int c = 0; c < 3; c++) { bl.lo[c] = b.bounds_lo[c]; bl.hi[c] = b.bounds_hi[c]; }
		tri_base += bl.n_tris;
	}
	(void)hipFree(staged);
	return rc;
}

// SceneTLAS::build_tlas + every MeshBLAS::build (scene_tlas.h:140-176, mesh_blas.h:86-138): nothing is flattened
int mrt_upload_two_level_scene(mrt_ctx *ctx, const float *verts9, uint32_t n_mesh_tris, const mrt_instance *instances,
		uint32_t n_instances, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!verts9 || !instances || n_instances == 0 || n_mesh_tris == 0) return fail(ctx, MRT_ERR_INVALID, "two-level scene: null or empty argument");
	if (flags & ~(uint32_t)(MRT_BUILD_BLAS_ON_DEVICE | MRT_BUILD_SAH)) return fail(ctx, MRT_ERR_INVALID, "two-level scene: unknown flag");
	if ((flags & MRT_BUILD_SAH) && !(flags & MRT_BUILD_BLAS_ON_DEVICE)) return fail(ctx, MRT_ERR_INVALID, "two-level scene: MRT_BUILD_SAH goes with MRT_BUILD_BLAS_ON_DEVICE (the host builder's trees are SAH trees)");
	const bool on_device = (flags & MRT_BUILD_BLAS_ON_DEVICE) != 0;
	int rc = drain_pending(ctx);
	if (rc) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	mrt::TwoLevelHost *h = new (std::nothrow) mrt::TwoLevelHost();
	if (!h) return fail(ctx, MRT_ERR_OOM, "two-level scene: out of host memory");
	auto drop = [&] { mrt::free_two_level(h); delete h; };
	unsigned n_thr = std::thread::hardware_concurrency();
	rc = mrt::prepare_two_level(verts9, n_mesh_tris, instances, n_instances, n_thr ? n_thr : 1u, !on_device, h, ctx->err, sizeof(ctx->err));
	if (rc) { drop(); return rc; }
	if (!on_device && h->depth > 64u) { drop(); return fail(ctx, MRT_ERR_UNSUPPORTED, "two-level scene: trees too deep for the traversal stack"); }
	hipError_t e = hipStreamSynchronize(ctx->stream);
	if (e != hipSuccess) { drop(); return fail(ctx, MRT_ERR_HIP, hipGetErrorString(e)); }
	free_scene(ctx);
	if ((e = hipMalloc(&ctx->d_nodes, (size_t)h->n_nodes * sizeof(mrt::DevNode))) != hipSuccess ||
			(e = hipMalloc(&ctx->d_hot, (size_t)h->n_tris * sizeof(mrt::TriHot) + 16)) != hipSuccess ||
			(e = hipMalloc(&ctx->d_cold, (size_t)h->n_tris * sizeof(mrt::TriCold))) != hipSuccess ||
			(e = hipMalloc(&ctx->d_instances, (size_t)h->n_inst * sizeof(mrt::DevInstance))) != hipSuccess) {
		drop(); free_scene(ctx);
		return fail(ctx, MRT_ERR_OOM, "scene does not fit in device memory");
	}
	if (on_device) { h->wide8 = true; h->n_nodes8 = h->n_nodes - h->tlas_cap; } // wanted; build_blases_on_device takes it back if a mesh has none
	if (h->wide8 && (hipMalloc(&ctx->d_nodes8, (size_t)h->n_nodes8 * sizeof(mrt::Dev8Node)) != hipSuccess ||
			hipMalloc(&ctx->d_leaf_box, (size_t)h->n_tris * 32) != hipSuccess)) { // an optional layout: go without it
		if (ctx->d_nodes8) (void)hipFree(ctx->d_nodes8);
		ctx->d_nodes8 = nullptr; ctx->d_leaf_box = nullptr; h->wide8 = false;
	}
	if (on_device) {
		hipEvent_t e0 = ctx->ev[0], e1 = ctx->ev[1]; // the context's own events: nothing to create or to leak here
		(void)hipEventRecord(e0, ctx->stream);
		rc = build_blases_on_device(ctx, h, verts9, (flags & MRT_BUILD_SAH) ? 2 : 0);
		if (!rc) rc = mrt::refit_two_level(h, instances, n_instances, ctx->err, sizeof(ctx->err));
		if (!rc && h->depth > 64u) rc = fail(ctx, MRT_ERR_UNSUPPORTED, "two-level scene: device-built trees too deep for the traversal stack: build on the host");
		if (rc) { drop(); free_scene(ctx); return rc; }
		e = hipMemcpy(ctx->d_nodes, h->nodes, (size_t)h->n_tlas_nodes * sizeof(mrt::DevNode), hipMemcpyHostToDevice);
		(void)hipEventRecord(e1, ctx->stream);
		(void)hipEventSynchronize(e1);
		float ms = 0.0f;
		if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ctx->stats.last_build_ms = ms;
	} else {
		e = hipMemcpy(ctx->d_nodes, h->nodes, (size_t)h->n_nodes * sizeof(mrt::DevNode), hipMemcpyHostToDevice);
		if (e == hipSuccess) e = hipMemcpy(ctx->d_hot, h->hot, (size_t)h->n_tris * sizeof(mrt::TriHot), hipMemcpyHostToDevice);
		if (e == hipSuccess) e = hipMemcpy(ctx->d_cold, h->cold, (size_t)h->n_tris * sizeof(mrt::TriCold), hipMemcpyHostToDevice);
		if (e == hipSuccess && h->wide8) e = hipMemcpy(ctx->d_nodes8, h->nodes8, (size_t)h->n_nodes8 * sizeof(mrt::Dev8Node), hipMemcpyHostToDevice);
		if (e == hipSuccess && h->wide8) e = hipMemcpy(ctx->d_leaf_box, h->leaf_box, (size_t)h->n_tris * 32, hipMemcpyHostToDevice);
	}
	if (!h->wide8 && ctx->d_nodes8) { // taken back during the device builds
		(void)hipFree(ctx->d_nodes8); (void)hipFree(ctx->d_leaf_box);
		ctx->d_nodes8 = nullptr; ctx->d_leaf_box = nullptr;
	}
	if (e == hipSuccess) e = hipMemcpy(ctx->d_instances, h->inst, (size_t)h->n_inst * sizeof(mrt::DevInstance), hipMemcpyHostToDevice);
	if (e != hipSuccess) { drop(); free_scene(ctx); return fail(ctx, MRT_ERR_HIP, hipGetErrorString(e)); }
	std::free(h->hot); std::free(h->cold); h->hot = nullptr; h->cold = nullptr; // the device has them; a refit only needs nodes + instances
	std::free(h->nodes8); std::free(h->leaf_box); h->nodes8 = nullptr; h->leaf_box = nullptr;
	ctx->n_nodes8 = h->wide8 ? h->n_nodes8 : 0; ctx->stack8 = h->wide8 ? h->depth8 : 0;
	ctx->two_level = h;
	ctx->n_nodes = h->n_nodes; ctx->n_tris = h->n_tris; ctx->depth = h->depth;
	ctx->stack_depth = ((h->depth + 7u) / 8u) * 8u;
	if (ctx->stack_depth < 8) ctx->stack_depth = 8;
	ctx->n_nodes4 = 0; ctx->stack4 = 0;
	// sort keys (origin Morton) are quantised on the scene box: the union of the TLAS root's children
	for (int c = 0; c < 3; c++) {
		ctx->bounds_lo[c] = std::fmin(h->nodes[0].lmin[c], h->nodes[0].rmin[c]);
		ctx->bounds_hi[c] = std::fmax(h->nodes[0].lmax[c], h->nodes[0].rmax[c]);
	}
	ctx->scene = true;
	return MRT_OK;
}

// SceneTLAS::set_instance_transform + refit_tlas (scene_tlas.h:118-134,178-196): instances moved, meshes unchanged
int mrt_update_instances(mrt_ctx *ctx, const mrt_instance *instances, uint32_t n_instances)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!ctx->scene || !ctx->two_level) return fail(ctx, MRT_ERR_NO_SCENE, "no two-level scene uploaded");
	if (!instances) return fail(ctx, MRT_ERR_INVALID, "null instances");
	int rc = drain_pending(ctx);
	if (rc) return rc;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	mrt::TwoLevelHost *h = ctx->two_level;
	if ((rc = mrt::refit_two_level(h, instances, n_instances, ctx->err, sizeof(ctx->err)))) return rc;
	if (h->depth > 64u) return fail(ctx, MRT_ERR_UNSUPPORTED, "two-level scene: trees too deep for the per-lane stack");
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	HIP_TRY(ctx, hipMemcpy(ctx->d_nodes, h->nodes, (size_t)h->n_tlas_nodes * sizeof(mrt::DevNode), hipMemcpyHostToDevice));
	HIP_TRY(ctx, hipMemcpy(ctx->d_instances, h->inst, (size_t)h->n_inst * sizeof(mrt::DevInstance), hipMemcpyHostToDevice));
	ctx->depth = h->depth; ctx->stack8 = h->wide8 ? h->depth8 : 0;
	ctx->stack_depth = ((h->depth + 7u) / 8u) * 8u;
	if (ctx->stack_depth < 8) ctx->stack_depth = 8;
	for (int c = 0; c < 3; c++) {
		ctx->bounds_lo[c] = std::fmin(h->nodes[0].lmin[c], h->nodes[0].rmin[c]);
		ctx->bounds_hi[c] = std::fmax(h->nodes[0].lmax[c], h->nodes[0].rmax[c]);
	}
	return MRT_OK;
}

int mrt_is_available(const mrt_ctx *ctx) { return ctx && ctx->scene ? 1 : 0; }

int mrt_scene_info(const mrt_ctx *ctx, uint32_t *n_tris, uint32_t *n_wide_nodes, uint32_t *bvh_depth)
{
	if (!ctx || !ctx->scene) return MRT_ERR_NO_SCENE;
	if (n_tris) *n_tris = ctx->n_tris;
	if (n_wide_nodes) *n_wide_nodes = ctx->n_nodes;
	if (bvh_depth) *bvh_depth = ctx->depth;
	return MRT_OK;
}

// The resident scene's arrays as they stand, for a validator on the host (include/mrt_hip.h).  Reads only: plain copies on the
// context's stream into the caller's buffers, one wait at the end; no allocation, no tuner, schedule or counter state touched.
int mrt_debug_snapshot(mrt_ctx *ctx, mrt_debug_snapshot_info *info, void *const *buffers)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!info || info->struct_size != sizeof(mrt_debug_snapshot_info)) return fail(ctx, MRT_ERR_INVALID, "debug_snapshot: null info or bad struct_size");
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "debug_snapshot: collect the pending dispatch first");
	if (!ctx->scene) return fail(ctx, MRT_ERR_NO_SCENE, "debug_snapshot: no scene uploaded");
	const mrt::TwoLevelHost *tl = ctx->two_level;
	std::memset(info, 0, sizeof(*info));
	info->struct_size = sizeof(*info);
	info->two_level = tl ? 1u : 0u;
	info->n_nodes = ctx->n_nodes; info->n_tris = ctx->n_tris; info->n_nodes4 = ctx->d_nodes4 ? ctx->n_nodes4 : 0u; info->n_nodes8 = ctx->d_nodes8 ? ctx->n_nodes8 : 0u;
	info->depth = ctx->depth; info->stack_depth = ctx->stack_depth; info->stack4 = ctx->stack4; info->stack8 = ctx->stack8;
	info->n_tlas_nodes = tl ? tl->n_tlas_nodes : 0u; info->tlas_cap = tl ? tl->tlas_cap : 0u; info->n_instances = tl ? tl->n_inst : 0u;
	for (int c = 0; c < 3; c++) {
		info->bounds_lo[c] = ctx->bounds_lo[c]; info->bounds_hi[c] = ctx->bounds_hi[c];
		info->scene_abs_max = std::fmax(info->scene_abs_max, std::fmax(std::fabs(ctx->bounds_lo[c]), std::fabs(ctx->bounds_hi[c])));
	}
	const void *src[MRT_SNAP_COUNT] = { ctx->d_nodes, ctx->d_hot, ctx->d_cold, ctx->d_nodes4, ctx->d_nodes8, ctx->d_leaf_box, ctx->d_slot_src,
		ctx->d_parent, ctx->d_rows, ctx->d_rows4, ctx->d_instances };
	static const uint32_t elem[MRT_SNAP_COUNT] = { sizeof(mrt::DevNode), sizeof(mrt::TriHot), sizeof(mrt::TriCold), sizeof(mrt::Dev4Node),
		sizeof(mrt::Dev8Node), 32u, 4u, 4u, 64u, 64u, sizeof(mrt::DevInstance) };
	const uint64_t count[MRT_SNAP_COUNT] = { ctx->n_nodes, ctx->n_tris, ctx->n_tris, ctx->n_nodes4, ctx->n_nodes8, ctx->n_tris, ctx->n_tris,
		(uint64_t)ctx->n_nodes - (tl ? tl->tlas_cap : 0u), (uint64_t)ctx->n_nodes + ctx->n_tris, (uint64_t)2u * ctx->n_nodes4 + ctx->n_tris, tl ? tl->n_inst : 0u };
	for (int a = 0; a < MRT_SNAP_COUNT; a++) { info->count[a] = src[a] ? count[a] : 0u; info->elem_bytes[a] = elem[a]; }
	if (!buffers) return MRT_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	for (int a = 0; a < MRT_SNAP_COUNT; a++)
		if (buffers[a] && info->count[a])
			HIP_TRY(ctx, hipMemcpyAsync(buffers[a], src[a], (size_t)info->count[a] * elem[a], hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return MRT_OK;
}

int mrt_generate_grid(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h,
		uint32_t y0, uint32_t y1, mrt_ray32 *d_rays)
{
	if (!ctx || !d_rays) return MRT_ERR_INVALID;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	mrt::TraceParams p;
	int rc = grid_params(ctx, cam, grid_w, grid_h, y0, y1, p);
	if (rc) return rc;
	HIP_TRY(ctx, mrt::launch_grid_rays(p, d_rays, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return MRT_OK;
}

int mrt_expand_tokens(mrt_ctx *ctx, const void *d_rays, const uint32_t *d_tokens, void *d_hits, uint64_t count,
		uint32_t flags, void *hip_stream)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!ctx->scene) return fail(ctx, MRT_ERR_NO_SCENE, "no scene uploaded");
	if (count == 0) return MRT_OK;
	if (!d_rays || !d_tokens || !d_hits) return fail(ctx, MRT_ERR_INVALID, "null rays / tokens / hits");
	if (flags & (MRT_FLAG_BOOL_OUT | MRT_FLAG_TOKEN_OUT)) return fail(ctx, MRT_ERR_INVALID, "tokens expand to hit records only");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	mrt::TraceParams p;
	base_params(ctx, p);
	p.rays = d_rays; p.hits = d_hits; p.count = count;
	p.in_fmt = (flags & MRT_FLAG_HOST_LAYOUT) ? mrt::IN_HOST60 : mrt::IN_RAY32;
	p.out_fmt = (flags & MRT_FLAG_HOST_LAYOUT) ? mrt::OUT_HOST44 : mrt::OUT_HIT32;
	HIP_TRY(ctx, mrt::launch_expand_tokens(p, d_tokens, hip_stream ? (hipStream_t)hip_stream : ctx->stream));
	return MRT_OK;
}

int mrt_expand_grid_tokens(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h,
		uint32_t y0, uint32_t y1, const uint32_t *d_tokens, mrt_hit32 *d_hits, void *hip_stream)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!ctx->scene) return fail(ctx, MRT_ERR_NO_SCENE, "no scene uploaded");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	mrt::TraceParams p;
	int rc = grid_params(ctx, cam, grid_w, grid_h, y0, y1, p);
	if (rc) return rc;
	if (p.count == 0) return MRT_OK;
	if (!d_tokens || !d_hits) return fail(ctx, MRT_ERR_INVALID, "null tokens / hits");
	p.hits = d_hits; p.out_fmt = mrt::OUT_HIT32;
	HIP_TRY(ctx, mrt::launch_expand_tokens(p, d_tokens, hip_stream ? (hipStream_t)hip_stream : ctx->stream));
	return MRT_OK;
}

int mrt_morton_keys(mrt_ctx *ctx, const mrt_ray32 *d_rays, uint64_t count, uint32_t *d_keys)
{
	if (!ctx || !d_rays || !d_keys) return MRT_ERR_INVALID;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, mrt::launch_morton_keys(d_rays, mrt::IN_RAY32, count, d_keys, nullptr, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return MRT_OK;
}

uint32_t mrt_token_bytes(mrt_ctx *ctx)
{
	return ctx ? (uint32_t)token_bytes(ctx) : 0u;
}

const char *mrt_last_kernel_variant(mrt_ctx *ctx)
{
	return ctx ? ctx->last_variant : "";
}

int mrt_get_stats(mrt_ctx *ctx, mrt_stats *out)
{
	if (!ctx || !out) return MRT_ERR_INVALID;
	*out = ctx->stats;
	return MRT_OK;
}

int mrt_schedule_counts(mrt_ctx *ctx, uint64_t out[3])
{
	if (!ctx || !out) return MRT_ERR_INVALID;
	for (int k = 0; k < 3; k++) out[k] = ctx->sched_counts[k];
	return MRT_OK;
}

int mrt_debug_sort_order(mrt_ctx *ctx, uint32_t *out, uint64_t count)
{
	if (!ctx || !out) return MRT_ERR_INVALID;
	if (!ctx->idx_out.ptr || count == 0 || count > ctx->idx_out.cap / 4) return fail(ctx, MRT_ERR_INVALID, "no sorted cast of that many rays");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(out, ctx->idx_out.ptr, count * 4, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return MRT_OK;
}

int mrt_device_alloc(mrt_ctx *ctx, size_t bytes, void **d_ptr)
{
	if (!ctx || !d_ptr) return MRT_ERR_INVALID;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (hipMalloc(d_ptr, bytes ? bytes : 16) != hipSuccess) { *d_ptr = nullptr; return fail(ctx, MRT_ERR_OOM, "device allocation failed"); }
	return MRT_OK;
}
int mrt_device_free(mrt_ctx *ctx, void *d_ptr)
{
	if (!ctx) return MRT_ERR_INVALID;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	if (d_ptr) HIP_TRY(ctx, hipFree(d_ptr));
	return MRT_OK;
}
int mrt_memcpy_h2d(mrt_ctx *ctx, void *d_dst, const void *h_src, size_t bytes)
{
	if (!ctx || (bytes && (!d_dst || !h_src))) return MRT_ERR_INVALID;
	HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return MRT_OK;
}
int mrt_memcpy_d2h(mrt_ctx *ctx, void *h_dst, const void *d_src, size_t bytes)
{
	if (!ctx || (bytes && (!h_dst || !d_src))) return MRT_ERR_INVALID;
	HIP_TRY(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return MRT_OK;
}

} // extern "C"
