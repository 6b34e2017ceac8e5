// cast.hip — the casts of the C-ABI: mrt_cast / mrt_submit / mrt_collect (rays from arrays), mrt_cast_grid (rays made in the
// kernel), mrt_cast_tiled, and the record-driven casts (rays made in the kernel from resident records: their entry points; what they
// refuse and how their arguments are filled is source_cast.h's).  launch_policy.cpp plans every cast (which kernel, how launched);
// launch_planned runs the plan.
#include <cstdio>
#include <cstring>
#include <atomic>
#include <thread>
#include <utility>
#include <vector>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "mrt_context.h"
#include "gbuffer.h"
#include "source_cast.h"
#include "emitters.h"

namespace {

// Sorts ray indices by direction Morton key on the device; returns the permutation in idx_out.
int device_sort(mrt_ctx *ctx, const void *d_rays, uint32_t in_fmt, uint64_t count, const uint32_t **perm)
{
	if (count > 0xFFFFFFFFull) return fail(ctx, MRT_ERR_UNSUPPORTED, "sorted batches are limited to 2^32-1 rays");
	int rc;
	if ((rc = ensure(ctx, ctx->keys_in, count * 4)) || (rc = ensure(ctx, ctx->keys_out, count * 4)) ||
			(rc = ensure(ctx, ctx->idx_in, count * 4)) || (rc = ensure(ctx, ctx->idx_out, count * 4))) return rc;
	uint32_t *ki = (uint32_t *)ctx->keys_in.ptr, *ko = (uint32_t *)ctx->keys_out.ptr;
	uint32_t *ii = (uint32_t *)ctx->idx_in.ptr, *io = (uint32_t *)ctx->idx_out.ptr;
	if (ctx->opts.sort_key == 1) // the reference's direction-only key (ray_sort.h:64-76)
		HIP_TRY(ctx, mrt::launch_morton_keys(d_rays, in_fmt, count, ki, ii, ctx->stream));
	else // origin cell first, then direction: groups rays whose origins are scattered too
		HIP_TRY(ctx, mrt::launch_origin_dir_keys(d_rays, in_fmt, count, ctx->bounds_lo, ctx->bounds_hi, ki, ii, ctx->stream));
	size_t tmp_bytes = 0;
	HIP_TRY(ctx, rocprim::radix_sort_pairs(nullptr, tmp_bytes, ki, ko, ii, io, (size_t)count, 0, 30, ctx->stream));
	if ((rc = ensure(ctx, ctx->sort_tmp, tmp_bytes ? tmp_bytes : 16))) return rc;
	HIP_TRY(ctx, rocprim::radix_sort_pairs(ctx->sort_tmp.ptr, tmp_bytes, ki, ko, ii, io, (size_t)count, 0, 30, ctx->stream));
	*perm = io;
	return MRT_OK;
}

// bytes of one output record (mrt::OutFmt)
size_t out_bytes(uint32_t out_fmt)
{
	switch (out_fmt) {
		case mrt::OUT_HOST44: return sizeof(mrt_host_hit44);
		case mrt::OUT_BOOL8: return 1;
		case mrt::OUT_TOKEN4: return 4;
		case mrt::OUT_TOKEN8: return 8;
		default: return sizeof(mrt_hit32);
	}
}

mrt::SceneFacts scene_facts(const mrt_ctx *ctx)
{
	mrt::SceneFacts s;
	s.two_level = ctx->two_level != nullptr; s.rows = ctx->d_rows != nullptr; s.rows4 = ctx->d_rows4 != nullptr;
	s.nodes4 = ctx->d_nodes4 != nullptr; s.nodes8 = ctx->d_nodes8 != nullptr;
	s.n_nodes = ctx->n_nodes; s.depth = ctx->depth; s.stack4 = ctx->stack4; s.stack8 = ctx->stack8;
	s.cu_count = (uint32_t)ctx->cu_count;
	return s;
}

mrt::CastPlan plan(mrt_ctx *ctx, const mrt::CastRequest &r)
{
	// (never h_auto itself: a detect queued before this cast may not have run yet; the memo's pair is the one of the last wait)
	return mrt::plan_cast(ctx->opts, scene_facts(ctx), r, ctx->detect.prev(), ctx->knobs, ctx->grids);
}

void note_queued(mrt_ctx *ctx, uint32_t kernel)
{
	ctx->queued_kernel = kernel;
	std::snprintf(ctx->queued_variant, sizeof(ctx->queued_variant), "%s", mrt::last_trace_variant());
}

// The end of an ASYNC cast: no kernel is named (mrt_stats.last_kernel, mrt_last_kernel_variant) -- which one does the work of a
// batch declared coherent is known only once the stream has been waited for -- and there is no timing: the four times are 0, not
// those of an earlier blocking cast.
int queued_async(mrt_ctx *ctx)
{
	ctx->stats.last_trace_ms = ctx->stats.last_sort_ms = ctx->stats.last_h2d_ms = ctx->stats.last_d2h_ms = 0.0f;
	ctx->stats.last_kernel = 0;
	ctx->last_variant[0] = '\0';
	return MRT_OK;
}

// A cast whose rays are made in the kernel launches its source family's instantiation of the same lane kernels: the family's launcher
// (mrt::launch_source<S>), its parameters (an S) and which of its three sources.  launch_planned and launch_lane pass it through.
struct SourceLaunch {
	hipError_t (*launch)(const mrt::TraceParams &, const void *, int, bool, unsigned long long *, uint32_t *, uint32_t, uint32_t, uint32_t, uint32_t, hipStream_t);
	const void *params;
	int src;
};

int launch_lane(mrt_ctx *ctx, const mrt::LaneLaunch &l, mrt::TraceParams &p, uint64_t count, bool any_hit, const SourceLaunch *sh = nullptr)
{
	int rc;
	p.kernel = l.kernel;
	if (!l.persistent) {
		p.sparse_lanes = l.sparse_lanes;
		if (sh) HIP_TRY(ctx, sh->launch(p, sh->params, sh->src, any_hit, nullptr, nullptr, 0u, 0u, 0u, 0u, ctx->stream));
		else HIP_TRY(ctx, mrt::launch_trace(p, any_hit, l.count, ctx->stream));
		note_queued(ctx, p.kernel);
		return MRT_OK;
	}
	uint32_t *ovf = nullptr;
	if (l.spill) { // deeper entries spill to [depth - lds_depth][thread] in HBM
		if ((rc = ensure(ctx, ctx->overflow, (size_t)l.spill * l.blocks * 256u * 4u))) return rc;
		ovf = (uint32_t *)ctx->overflow.ptr;
	}
	// eight ray counters (one per region of the batch), 128 bytes apart
	unsigned long long *next_ray = ctx->d_counters + mrt::kNextRayOff;
	HIP_TRY(ctx, hipMemsetAsync(next_ray, 0, 128 * sizeof(unsigned long long), ctx->stream));
	if (sh) HIP_TRY(ctx, sh->launch(p, sh->params, sh->src, any_hit, next_ray, ovf, l.lds_depth, l.refill, l.leaf_wait, l.blocks, ctx->stream));
	else HIP_TRY(ctx, mrt::launch_trace_persistent(p, next_ray, ovf, l.lds_depth, l.refill, l.leaf_wait, l.blocks, any_hit, l.count, ctx->stream));
	note_queued(ctx, p.kernel);
	return MRT_OK;
}

// Runs a plan on the context's stream: pre-processing of rays from an array (sort, detect) from ev[2] to ev[3] (last_sort_ms), the
// trace launches from ev[3] to ev[4] (last_trace_ms), then the sort of a measuring frame's tile costs on the side stream.  p holds
// the batch (rays, hits, formats, grid); the plan decides the rest.
int launch_planned(mrt_ctx *ctx, const mrt::CastPlan &c, const mrt::CastRequest &r, mrt::TraceParams &p, const SourceLaunch *sh = nullptr)
{
	int rc;
	const bool rays = mrt::ray_entry(r.entry), any = r.mode == MRT_MODE_ANY_HIT;
	const auto zero_counters = [&] { return hipMemsetAsync(ctx->d_counters, 0, mrt::kNumCounters * sizeof(unsigned long long), ctx->stream); };
	p.kernel = c.kernel; p.lane_map = c.lane_map; p.quarter_all = c.quarter_all;
	// (tests: a record no launch writes keeps the pattern; the mapped small-cast buffer is filled on the host, mrt_cast)
	if (ctx->knobs.poison && p.hits != ctx->d_small_out)
		HIP_TRY(ctx, hipMemsetAsync(p.hits, mrt::kPoisonByte, p.count * out_bytes(p.out_fmt), ctx->stream));
	if (rays) HIP_TRY(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
	if (c.sort) {
		const uint32_t *perm = nullptr;
		if ((rc = device_sort(ctx, p.rays, p.in_fmt, r.count, &perm))) return rc;
		p.perm = perm;
	}
	if (c.detect) {
		uint32_t *d_auto = reinterpret_cast<uint32_t *>(ctx->d_counters + mrt::kAutoGridOff);
		HIP_TRY(ctx, mrt::launch_detect_grid(p.rays, p.in_fmt, r.count, p.tile_w_log2, ctx->d_counters + mrt::kDetectScratchOff, d_auto, ctx->d_auto_host, ctx->stream));
		p.auto_grid = d_auto;
	}
	if (rays) ctx->detect.queued(c.detect, r.count);
	if (rays && ctx->opts.count_visits) HIP_TRY(ctx, zero_counters());
	if (c.scheduled && (rc = schedule_grid(ctx, c, p))) return rc;
	HIP_TRY(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
	if (!rays && ctx->opts.count_visits) HIP_TRY(ctx, zero_counters());
	ctx->queued_detect = c.detect; ctx->queued_alt_kernel = 0;
	if (c.launch == mrt::CastPlan::DUAL) {
		p.skip_flag = p.auto_grid + 3; p.skip_when = 1u;
		HIP_TRY(ctx, mrt::launch_trace(p, any, c.count, ctx->stream));
		note_queued(ctx, p.kernel);
		mrt::TraceParams lp = p;
		lp.lane_map = mrt::MAP_LINEAR; lp.auto_grid = nullptr; lp.skip_when = 0u; lp.quarter_all = 0u;
		std::swap(ctx->queued_kernel, ctx->queued_alt_kernel); std::swap(ctx->queued_variant, ctx->queued_alt_variant);
		if ((rc = launch_lane(ctx, c.lane, lp, r.count, any))) return rc; // runs if the batch is judged incoherent
		std::swap(ctx->queued_kernel, ctx->queued_alt_kernel); std::swap(ctx->queued_variant, ctx->queued_alt_variant);
	} else if (c.launch == mrt::CastPlan::LANE) {
		if ((rc = launch_lane(ctx, c.lane, p, r.count, any, sh))) return rc;
	} else {
		HIP_TRY(ctx, mrt::launch_trace(p, any, c.count, ctx->stream));
		note_queued(ctx, p.kernel);
	}
	HIP_TRY(ctx, hipEventRecord(ctx->ev[4], ctx->stream));
	if (c.scheduled && (rc = schedule_sort(ctx))) return rc;
	if (c.launches) ctx->stats.last_kernel_launches = c.launches;
	ctx->stats.rays_cast += r.count;
	return MRT_OK;
}

// Enqueue H2D (if needed) + optional sort + trace.  On return the kernels are queued on ctx->stream.
int enqueue_cast(mrt_ctx *ctx, mrt::Entry entry, const void *rays, void *hits_dev_or_null, uint64_t count, uint32_t query_mask,
		int mode, uint32_t flags, void **d_hits_out)
{
	if (!ctx->scene) return fail(ctx, MRT_ERR_NO_SCENE, "no scene uploaded (is_available() == false)");
	if (mode != MRT_MODE_NEAREST && mode != MRT_MODE_ANY_HIT) return fail(ctx, MRT_ERR_INVALID, "bad mode");
	if ((flags & MRT_FLAG_BOOL_OUT) && mode != MRT_MODE_ANY_HIT) return fail(ctx, MRT_ERR_INVALID, "BOOL_OUT needs any-hit mode");
	if ((flags & MRT_FLAG_BOOL_OUT) && (flags & MRT_FLAG_TOKEN_OUT)) return fail(ctx, MRT_ERR_INVALID, "BOOL_OUT and TOKEN_OUT exclude each other");
	const size_t rs = ray_stride(flags), hs = hit_stride(ctx, flags, mode);
	int rc;
	const void *d_rays = rays;
	ctx->stats.last_h2d_ms = ctx->stats.last_d2h_ms = ctx->stats.last_sort_ms = 0.0f;
	if (!(flags & MRT_FLAG_RAYS_ON_DEVICE)) {
		if ((rc = ensure(ctx, ctx->rays, count * rs))) return rc;
		HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
		HIP_TRY(ctx, hipMemcpyAsync(ctx->rays.ptr, rays, count * rs, hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
		d_rays = ctx->rays.ptr;
	}
	void *d_hits = hits_dev_or_null;
	if (!d_hits) {
		if ((rc = ensure(ctx, ctx->hits, count * hs))) return rc;
		d_hits = ctx->hits.ptr;
	}
	mrt::TraceParams p;
	base_params(ctx, p);
	p.rays = d_rays; p.hits = d_hits; p.count = count; p.query_mask = query_mask;
	p.in_fmt = (flags & MRT_FLAG_HOST_LAYOUT) ? mrt::IN_HOST60 : mrt::IN_RAY32;
	p.out_fmt = out_format(ctx, flags, mode);
	const mrt::CastRequest r{entry, count, flags, mode};
	if ((rc = launch_planned(ctx, plan(ctx, r), r, p))) return rc;
	*d_hits_out = d_hits;
	return MRT_OK;
}

constexpr uint64_t kSmallCast = 1024; // rays: host-array casts up to this size take the mapped-memory path of mrt_cast

int finish_timing(mrt_ctx *ctx, bool h2d, bool sorted, bool d2h)
{
	float ms = 0.0f;
	if (h2d) { HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1])); ctx->stats.last_h2d_ms = ms; }
	if (sorted) { HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3])); ctx->stats.last_sort_ms = ms; }
	HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[3], ctx->ev[4])); ctx->stats.last_trace_ms = ms;
	if (d2h) { HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5])); ctx->stats.last_d2h_ms = ms; }
	// which kernel did the work: the stream has been waited for, so detect_grid_kernel's words are in h_auto
	ctx->detect.waited(ctx->h_auto);
	ctx->stats.detected_grid_w = ctx->queued_detect ? ctx->h_auto[0] : 0u;
	ctx->stats.reserved = ctx->queued_detect ? ctx->h_auto[3] : 0u; // 1: the "coherent" batch was judged incoherent
	const bool alt_ran = ctx->queued_detect && ctx->queued_alt_kernel && ctx->h_auto[3];
	ctx->stats.last_kernel = alt_ran ? ctx->queued_alt_kernel : ctx->queued_kernel;
	std::snprintf(ctx->last_variant, sizeof(ctx->last_variant), "%s", alt_ran ? ctx->queued_alt_variant : ctx->queued_variant);
	if (ctx->opts.count_visits) {
		unsigned long long c[mrt::kNumCounters];
		HIP_TRY(ctx, hipMemcpy(c, ctx->d_counters, sizeof(c), hipMemcpyDeviceToHost));
		ctx->stats.tri_tests += c[mrt::kCntTris]; ctx->stats.bvh_nodes_visited += c[mrt::kCntNodes]; ctx->stats.hits += c[mrt::kCntHits];
		if ((uint32_t)c[mrt::kCntMaxStack] > ctx->stats.max_stack_depth) ctx->stats.max_stack_depth = (uint32_t)c[mrt::kCntMaxStack];
		ctx->stats.dead_pops += c[mrt::kCntDeadPops];
		ctx->stats.wave_node_fetches += c[mrt::kCntWaveNodeFetch]; ctx->stats.wave_tri_fetches += c[mrt::kCntWaveTriFetch];
		ctx->stats.leaf_box_checks += c[mrt::kCntLeafBoxChecks];
		ctx->stats.fetch_wait_cycles += c[mrt::kCntFetchWaitCycles]; ctx->stats.wave_cycles += c[mrt::kCntWaveCycles];
		ctx->stats.waves += c[mrt::kCntWaves];
	}
	return MRT_OK;
}

// Host arrays in, host arrays out (the reference's cast_rays contract), large batch: upload, trace and
// download run as a pipeline over 2^20-ray chunks.  A pageable copy occupies the host thread that
// issues it, so uploads are issued from the calling thread and downloads from a helper thread: both
// PCIe directions then move data at once, and the trace of a chunk hides between them.
constexpr uint64_t kPipeChunk = 1ull << 20;

int cast_host_pipelined(mrt_ctx *ctx, const void *rays, void *hits, uint64_t count, uint32_t query_mask, int mode, uint32_t flags)
{
	const size_t rs = ray_stride(flags), hs = hit_stride(ctx, flags, mode);
	const uint32_t n_chunks = (uint32_t)((count + kPipeChunk - 1) / kPipeChunk);
	int rc;
	if ((rc = ensure(ctx, ctx->rays, count * rs)) || (rc = ensure(ctx, ctx->hits, count * hs))) return rc;
	if (!ctx->up_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->up_stream, hipStreamNonBlocking));
	if (!ctx->dn_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->dn_stream, hipStreamNonBlocking));
	while (ctx->pipe_ev.size() < 2u * n_chunks) {
		hipEvent_t e;
		HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
		ctx->pipe_ev.push_back(e);
	}
	char *d_rays = (char *)ctx->rays.ptr, *d_hits = (char *)ctx->hits.ptr;
	std::atomic<uint32_t> traced{0};      // chunks whose trace has been queued (their event is recorded)
	std::atomic<int> stop{0}, down_err{0};
	std::thread down([&] {
		if (hipSetDevice(ctx->device) != hipSuccess) { down_err = (int)hipErrorInvalidDevice; return; }
		for (uint32_t k = 0; k < n_chunks; k++) {
			while (traced.load(std::memory_order_acquire) <= k) { if (stop.load()) return; std::this_thread::yield(); }
			const uint64_t off = (uint64_t)k * kPipeChunk, n = count - off < kPipeChunk ? count - off : kPipeChunk;
			hipError_t e = hipEventSynchronize(ctx->pipe_ev[2 * k + 1]);
			if (e == hipSuccess) e = hipMemcpyAsync((char *)hits + off * hs, d_hits + off * hs, n * hs, hipMemcpyDeviceToHost, ctx->dn_stream);
			if (e == hipSuccess) e = hipStreamSynchronize(ctx->dn_stream);
			if (e != hipSuccess) { down_err = (int)e; return; }
		}
	});
	const uint32_t dev_flags = flags | MRT_FLAG_RAYS_ON_DEVICE | MRT_FLAG_HITS_ON_DEVICE;
	hipError_t e = hipSuccess;
	uint32_t launches = 0;
	for (uint32_t k = 0; k < n_chunks && e == hipSuccess && rc == MRT_OK && !down_err.load(); k++) {
		const uint64_t off = (uint64_t)k * kPipeChunk, n = count - off < kPipeChunk ? count - off : kPipeChunk;
		e = hipMemcpyAsync(d_rays + off * rs, (const char *)rays + off * rs, n * rs, hipMemcpyHostToDevice, ctx->up_stream);
		if (e == hipSuccess) e = hipEventRecord(ctx->pipe_ev[2 * k], ctx->up_stream);
		if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->pipe_ev[2 * k], 0);
		if (e != hipSuccess) break;
		void *unused = nullptr;
		rc = enqueue_cast(ctx, mrt::ENTRY_CHUNK, d_rays + off * rs, d_hits + off * hs, n, query_mask, mode, dev_flags, &unused);
		if (rc) break;
		if (ctx->stats.last_kernel_launches > launches) launches = ctx->stats.last_kernel_launches;
		e = hipEventRecord(ctx->pipe_ev[2 * k + 1], ctx->stream);
		if (e == hipSuccess) traced.store(k + 1, std::memory_order_release);
	}
	if (e != hipSuccess || rc != MRT_OK) stop = 1;
	down.join();
	(void)hipStreamSynchronize(ctx->stream);
	if (rc) return rc;
	if (e != hipSuccess || down_err.load()) {
		std::snprintf(ctx->err, sizeof(ctx->err), "pipelined cast failed: %s", hipGetErrorString(e != hipSuccess ? e : (hipError_t)down_err.load()));
		return MRT_ERR_HIP;
	}
	ctx->stats.last_kernel_launches = launches;
	ctx->stats.last_h2d_ms = ctx->stats.last_d2h_ms = 0.0f; // overlapped: not separable (last_trace_ms is the last chunk's)
	return finish_timing(ctx, false, launches >= 2, false);
}

// What every record-driven cast checks before it touches the device, after its entry point's opening (array_params, grid_source_params):
// why (what the family's *_invalid finds of the arguments and the flags, or null: source_cast.h, whose table has the order), the scene, a
// pending dispatch.  MRT_OK: go on (an empty cast is OK only after all of those: run_source_cast).
int source_cast_check(mrt_ctx *ctx, const char *why)
{
	if (why) return fail(ctx, MRT_ERR_INVALID, why);
	if (!ctx->scene) return fail(ctx, MRT_ERR_NO_SCENE, "no scene uploaded");
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "collect the pending dispatch first");
	return MRT_OK;
}

// The opening of an array form: the scene and the incoming rays.  host_rays: they are mrt_host_ray60 and the source reads them (a
// shadow source does not: the record has the position).  A null d_rays is the family's first refusal.
void array_params(mrt_ctx *ctx, const void *d_rays, bool host_rays, mrt::TraceParams &p)
{
	base_params(ctx, p);
	p.rays = d_rays;
	p.in_fmt = host_rays ? mrt::IN_HOST60 : mrt::IN_RAY32;
}

// The opening of a grid form: grid_params' refusals, then the lanes linear over the entries (the kernel regenerates the primary or
// incoming ray of an entry from p.cam itself).  p.count = the records of the band.
int grid_source_params(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1, mrt::TraceParams &p)
{
	int rc = grid_params(ctx, cam, grid_w, grid_h, y0, y1, p);
	if (rc) return rc;
	p.in_fmt = mrt::IN_RAY32;
	return MRT_OK;
}

// Plans and runs a record-driven cast of family S: p holds the scene, the batch (count = entries, hits = the output, out_fmt) and what
// the source reads of the incoming rays (rays or the grid); s the family's parameters.  Blocking unless ASYNC.  No entries (no
// records, or no lights or samples for them): MRT_OK, nothing is touched.
template <class S>
int run_source_cast(mrt_ctx *ctx, mrt::Entry entry, int src, int mode, mrt::TraceParams &p, const S &s, uint32_t flags)
{
	if (p.count == 0) return MRT_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// (the plan reads neither the detected grid nor the grid states: an empty PrevDetect)
	const mrt::CastRequest r{entry, p.count, flags, mode};
	const mrt::CastPlan c = mrt::plan_cast(ctx->opts, scene_facts(ctx), r, mrt::PrevDetect{}, ctx->knobs, ctx->grids);
	const SourceLaunch sl{&mrt::launch_source<S>, &s, src};
	int rc = launch_planned(ctx, c, r, p, &sl);
	if (rc) return rc;
	if (flags & MRT_FLAG_ASYNC) return queued_async(ctx);
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	ctx->stats.last_h2d_ms = ctx->stats.last_sort_ms = ctx->stats.last_d2h_ms = 0.0f;
	return finish_timing(ctx, false, false, false); // (no tune_record: the grid tuner times primary casts only)
}

// Runs a family's batch (source_cast.h): out = its output, one b.out_fmt record per entry.
template <class S>
int cast_batch(mrt_ctx *ctx, mrt::Entry entry, int src, mrt::TraceParams &p, const mrt::sc::Batch &b, void *out, uint32_t query_mask,
		const S &s, uint32_t flags)
{
	p.hits = out; p.count = b.count; p.query_mask = query_mask;
	p.out_fmt = b.out_fmt;
	return run_source_cast(ctx, entry, src, b.mode, p, s, flags);
}

// The families' casts, array and grid form (ENTRY_X / ENTRY_GRID_X): p comes from the form's opening and holds the scene, the grid (grid
// source) and the primary or incoming rays (array sources); count = records, pixel0 = the pixel index of record 0.

int cast_shadows(mrt_ctx *ctx, mrt::Entry entry, int src, mrt::TraceParams &p, const void *d_hits, uint64_t count,
		const mrt_light *lights, uint32_t n_lights, uint8_t *d_mask, uint32_t query_mask, uint32_t flags)
{
	if (int rc = source_cast_check(ctx, mrt::sc::shadow_invalid(entry == mrt::ENTRY_SHADOW, p.rays, d_hits, count, lights, n_lights, d_mask, flags)))
		return rc;
	mrt::ShadowParams s;
	mrt::sc::fill_shadow(d_hits, count, lights, n_lights, s);
	return cast_batch(ctx, entry, src, p, mrt::sc::shadow_batch(src, count, n_lights), d_mask, query_mask, s, flags);
}

// (d_rays: the grid form passes any non-null pointer; the family checks it before its other pointers)
int cast_selected_shadows(mrt_ctx *ctx, mrt::Entry entry, int src, mrt::TraceParams &p, const void *d_rays, const void *d_hits, uint64_t count,
		uint32_t pixel0, const mrt_light_select *desc, const mrt_light *lights, uint32_t n_lights, uint8_t *d_mask, uint32_t query_mask, uint32_t flags)
{
	if (int rc = source_cast_check(ctx, mrt::sc::selected_shadow_invalid(entry == mrt::ENTRY_SELECTED_SHADOW, d_rays, d_hits, desc, lights,
			n_lights, d_mask, flags))) return rc;
	if (n_lights == 0) return MRT_OK; // (nothing to select from: nothing written, as a shadow cast without lights)
	mrt::SelectShadowParams s;
	mrt::sc::fill_selected_shadow(d_hits, desc, lights, n_lights, pixel0, s);
	return cast_batch(ctx, entry, src, p, mrt::sc::selected_shadow_batch(src, count), d_mask, query_mask, s, flags);
}

// (an empty table: every record gets MRT_EMITTER_NONE and a lit byte, in the kernel, so that the outputs are always written)
int cast_emitter_shadows(mrt_ctx *ctx, mrt::Entry entry, int src, mrt::TraceParams &p, const void *d_rays, const void *d_hits, uint64_t count,
		uint32_t pixel0, const mrt_emitter_select *desc, uint8_t *d_mask, uint32_t query_mask, uint32_t flags)
{
	if (int rc = source_cast_check(ctx, mrt::em::shadow_invalid(entry == mrt::ENTRY_EMITTER_SHADOW, d_rays, d_hits, desc, d_mask, flags))) return rc;
	mrt::EmitterShadowParams s;
	mrt::em::fill_shadow(d_hits, desc, emitter_table(ctx), pixel0, s);
	return cast_batch(ctx, entry, src, p, mrt::sc::batch(src, MRT_MODE_ANY_HIT, count), d_mask, query_mask, s, flags);
}

int cast_reflections(mrt_ctx *ctx, mrt::Entry entry, int src, mrt::TraceParams &p, const void *d_hits, uint64_t count,
		const uint8_t *d_select, float max_distance, void *d_out_hits, void *d_out_rays, uint32_t query_mask, uint32_t flags)
{
	if (int rc = source_cast_check(ctx, mrt::sc::reflection_invalid(entry == mrt::ENTRY_REFLECTION, p.rays, d_hits, max_distance, d_out_hits, flags)))
		return rc;
	mrt::ReflectParams s;
	mrt::sc::fill_reflection(d_hits, d_select, max_distance, d_out_rays, s);
	return cast_batch(ctx, entry, src, p, mrt::sc::reflection_batch(src, count), d_out_hits, query_mask, s, flags);
}

int cast_hemisphere(mrt_ctx *ctx, mrt::Entry entry, int src, mrt::TraceParams &p, const void *d_hits, uint64_t count, uint32_t pixel0,
		const mrt_hemisphere *desc, void *d_out, void *d_out_rays, uint32_t query_mask, int mode, uint32_t flags)
{
	if (int rc = source_cast_check(ctx, mrt::sc::hemisphere_invalid(entry == mrt::ENTRY_HEMISPHERE, p.rays, d_hits, count, desc, d_out, d_out_rays,
			mode, flags))) return rc;
	mrt::HemiParams s;
	mrt::sc::fill_hemisphere(d_hits, count, pixel0, desc, d_out_rays, s);
	return cast_batch(ctx, entry, src, p, mrt::sc::hemisphere_batch(src, count, desc->n_samples, mode), d_out, query_mask, s, flags);
}

int cast_bounce(mrt_ctx *ctx, mrt::Entry entry, int src, mrt::TraceParams &p, const void *d_hits, uint64_t count, uint32_t pixel0,
		const mrt_bounce *desc, void *d_out_hits, void *d_out_rays, uint32_t query_mask, uint32_t flags)
{
	if (int rc = source_cast_check(ctx, mrt::sc::bounce_invalid(entry == mrt::ENTRY_BOUNCE, p.rays, d_hits, desc, d_out_hits, flags))) return rc;
	mrt::BounceParams s;
	mrt::sc::fill_bounce(d_hits, pixel0, desc, d_out_rays, s);
	return cast_batch(ctx, entry, src, p, mrt::sc::bounce_batch(src, count), d_out_hits, query_mask, s, flags);
}

} // namespace

extern "C" {

int mrt_cast(mrt_ctx *ctx, const void *rays, void *hits, uint64_t count, uint32_t query_mask, int mode, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (count == 0) return ctx->scene ? MRT_OK : fail(ctx, MRT_ERR_NO_SCENE, "no scene uploaded"); // cpp:419: silent no-op
	if (!rays || !hits) return fail(ctx, MRT_ERR_INVALID, "null rays / hits");
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "collect the pending dispatch first");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	void *d_hits = nullptr;
	const bool hits_dev = (flags & MRT_FLAG_HITS_ON_DEVICE) != 0;
	if ((flags & MRT_FLAG_ASYNC) && !(hits_dev && (flags & MRT_FLAG_RAYS_ON_DEVICE)))
		return fail(ctx, MRT_ERR_INVALID, "ASYNC needs device-resident rays and hits");
	if (!hits_dev && !(flags & MRT_FLAG_RAYS_ON_DEVICE) && count >= 2 * kPipeChunk && !ctx->opts.count_visits) {
		if (!ctx->scene) return fail(ctx, MRT_ERR_NO_SCENE, "no scene uploaded (is_available() == false)");
		return cast_host_pipelined(ctx, rays, hits, count, query_mask, mode, flags);
	}
	// Latency path: host arrays of at most kSmallCast rays skip both DMA copies: the kernel reads the rays from, and
	// writes the records to, pinned host memory mapped into the device (one ray: 85 -> 55 us per blocking call,
	// tools/bench_latency.py).  The same kernels, the same records.
	if (!hits_dev && !(flags & (MRT_FLAG_RAYS_ON_DEVICE | MRT_FLAG_ASYNC)) && count <= kSmallCast && !ctx->opts.count_visits) {
		const size_t rs_ = ray_stride(flags), hs_ = hit_stride(ctx, flags, mode);
		if (!ctx->h_small_in) {
			if (hipHostMalloc(&ctx->h_small_in, kSmallCast * 64, hipHostMallocMapped) != hipSuccess ||
					hipHostMalloc(&ctx->h_small_out, kSmallCast * 64, hipHostMallocMapped) != hipSuccess ||
					hipHostGetDevicePointer(&ctx->d_small_in, ctx->h_small_in, 0) != hipSuccess ||
					hipHostGetDevicePointer(&ctx->d_small_out, ctx->h_small_out, 0) != hipSuccess) {
				if (ctx->h_small_in) (void)hipHostFree(ctx->h_small_in);
				if (ctx->h_small_out) (void)hipHostFree(ctx->h_small_out);
				ctx->h_small_in = ctx->h_small_out = ctx->d_small_in = ctx->d_small_out = nullptr;
				(void)hipGetLastError();
			}
		}
		if (ctx->h_small_in) {
			std::memcpy(ctx->h_small_in, rays, count * rs_);
			if (ctx->knobs.poison) std::memset(ctx->h_small_out, mrt::kPoisonByte, count * hs_); // (no cast is in flight: mrt_cast waits for each)
			int rc2 = enqueue_cast(ctx, mrt::ENTRY_CAST, ctx->d_small_in, ctx->d_small_out, count, query_mask, mode, flags | MRT_FLAG_RAYS_ON_DEVICE, &d_hits);
			if (rc2) return rc2;
			HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
			std::memcpy(hits, ctx->h_small_out, count * hs_);
			return finish_timing(ctx, false, ctx->stats.last_kernel_launches >= 2, false);
		}
	}
	int rc = enqueue_cast(ctx, mrt::ENTRY_CAST, rays, hits_dev ? hits : nullptr, count, query_mask, mode, flags, &d_hits);
	if (rc) return rc;
	if (flags & MRT_FLAG_ASYNC) return queued_async(ctx); // queued on the context's stream; no timing
	if (!hits_dev) {
		HIP_TRY(ctx, hipMemcpyAsync(hits, d_hits, count * hit_stride(ctx, flags, mode), hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipEventRecord(ctx->ev[5], ctx->stream));
	}
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	rc = finish_timing(ctx, !(flags & MRT_FLAG_RAYS_ON_DEVICE), ctx->stats.last_kernel_launches >= 2, !hits_dev);
	if (rc == MRT_OK) mrt::tune_record(ctx->grids.tune(), ctx->stats.last_trace_ms);
	return rc;
}

int mrt_submit(mrt_ctx *ctx, const void *rays, uint64_t count, uint32_t query_mask, int mode, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "submit while a dispatch is pending (gpu_ray_caster.cpp:538)");
	if (!ctx->scene) return fail(ctx, MRT_ERR_NO_SCENE, "no scene uploaded");
	if (count == 0) return MRT_OK;
	if (!rays) return fail(ctx, MRT_ERR_INVALID, "null rays");
	if (flags & (MRT_FLAG_HITS_ON_DEVICE | MRT_FLAG_ASYNC)) return fail(ctx, MRT_ERR_INVALID, "submit keeps results in the context; use mrt_cast for device outputs");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	void *d_hits = nullptr;
	int rc = enqueue_cast(ctx, mrt::ENTRY_SUBMIT, rays, nullptr, count, query_mask, mode, flags, &d_hits);
	if (rc) return rc;
	ctx->pending = true; ctx->pending_count = count; ctx->pending_flags = flags; ctx->pending_mode = mode;
	ctx->pending_dev_hits = d_hits;
	return MRT_OK;
}

int mrt_collect(mrt_ctx *ctx, void *hits, uint64_t count)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!ctx->pending) return fail(ctx, MRT_ERR_NOT_PENDING, "collect without a pending dispatch");
	if (!hits) return fail(ctx, MRT_ERR_INVALID, "null hits");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint64_t n = count < ctx->pending_count ? count : ctx->pending_count; // cpp:573
	HIP_TRY(ctx, hipMemcpyAsync(hits, ctx->pending_dev_hits, n * hit_stride(ctx, ctx->pending_flags, ctx->pending_mode),
			hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipEventRecord(ctx->ev[5], ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	ctx->pending = false;
	return finish_timing(ctx, !(ctx->pending_flags & MRT_FLAG_RAYS_ON_DEVICE), ctx->stats.last_kernel_launches >= 2, true);
}

int mrt_has_pending(const mrt_ctx *ctx) { return ctx && ctx->pending ? 1 : 0; }

int mrt_cast_grid(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h,
		uint32_t y0, uint32_t y1, void *hits, uint32_t query_mask, int mode, uint32_t flags)
{
	if (!ctx || !hits) return MRT_ERR_INVALID;
	if (!ctx->scene) return fail(ctx, MRT_ERR_NO_SCENE, "no scene uploaded");
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "collect the pending dispatch first");
	if (flags & MRT_FLAG_HOST_LAYOUT) return fail(ctx, MRT_ERR_UNSUPPORTED, "grid casts write packed hits");
	if ((flags & MRT_FLAG_BOOL_OUT) && (flags & MRT_FLAG_TOKEN_OUT)) return fail(ctx, MRT_ERR_INVALID, "BOOL_OUT and TOKEN_OUT exclude each other");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	mrt::TraceParams p;
	int rc = grid_params(ctx, cam, grid_w, grid_h, y0, y1, p);
	if (rc) return rc;
	if (p.count == 0) return MRT_OK;
	const size_t hs = hit_stride(ctx, flags, mode);
	const bool hits_dev = (flags & MRT_FLAG_HITS_ON_DEVICE) != 0;
	if ((flags & MRT_FLAG_ASYNC) && !hits_dev) return fail(ctx, MRT_ERR_INVALID, "ASYNC needs device-resident hits");
	void *d_hits = hits;
	if (!hits_dev) { if ((rc = ensure(ctx, ctx->hits, p.count * hs))) return rc; d_hits = ctx->hits.ptr; }
	p.hits = d_hits; p.query_mask = query_mask;
	p.out_fmt = out_format(ctx, flags, mode);
	const mrt::CastRequest r{mrt::ENTRY_GRID, p.count, flags, mode, grid_w, grid_h, y0, p.rows};
	if ((rc = launch_planned(ctx, plan(ctx, r), r, p))) return rc;
	if (flags & MRT_FLAG_ASYNC) return queued_async(ctx);
	if (!hits_dev) {
		HIP_TRY(ctx, hipMemcpyAsync(hits, d_hits, p.count * hs, hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipEventRecord(ctx->ev[5], ctx->stream));
	}
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	ctx->stats.last_h2d_ms = ctx->stats.last_sort_ms = ctx->stats.last_d2h_ms = 0.0f;
	rc = finish_timing(ctx, false, false, !hits_dev);
	if (rc == MRT_OK) mrt::tune_record(ctx->grids.tune(), ctx->stats.last_trace_ms);
	return rc;
}

int mrt_cast_tiled(mrt_ctx *ctx, const mrt_ray32 *d_rays, mrt_hit32 *d_hits,
		uint32_t grid_w, uint32_t rows, uint32_t query_mask, int mode)
{
	if (!ctx || !d_rays || !d_hits || grid_w == 0) return MRT_ERR_INVALID;
	if (!ctx->scene) return fail(ctx, MRT_ERR_NO_SCENE, "no scene uploaded");
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "collect the pending dispatch first");
	if (rows == 0) return MRT_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	mrt::TraceParams p;
	base_params(ctx, p);
	p.rays = d_rays; p.hits = d_hits; p.count = (uint64_t)grid_w * rows; p.query_mask = query_mask;
	p.in_fmt = mrt::IN_RAY32; p.out_fmt = mrt::OUT_HIT32;
	p.grid_w = grid_w; p.grid_h = rows; p.y0 = 0; p.rows = rows;
	const mrt::CastRequest r{mrt::ENTRY_TILED, p.count, 0u, mode, grid_w, rows, 0u, rows};
	const mrt::CastPlan c = plan(ctx, r);
	p.tiles_x = c.tiles_x;
	int rc = launch_planned(ctx, c, r, p);
	if (rc) return rc;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	ctx->stats.last_h2d_ms = ctx->stats.last_sort_ms = ctx->stats.last_d2h_ms = 0.0f;
	return finish_timing(ctx, false, false, false);
}

// ---- the record-driven casts: each entry point is its form's opening (array_params / grid_source_params), its source and its family --------

int mrt_cast_shadows(mrt_ctx *ctx, const void *d_rays, const void *d_hits, uint64_t count,
		const mrt_light *lights, uint32_t n_lights, uint8_t *d_mask, uint32_t query_mask, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	mrt::TraceParams p;
	array_params(ctx, d_rays, false, p);
	const int src = (flags & MRT_FLAG_HOST_LAYOUT) ? mrt::SRC_SHADOW_HOST44 : mrt::SRC_SHADOW_RAY32;
	return cast_shadows(ctx, mrt::ENTRY_SHADOW, src, p, d_hits, count, lights, n_lights, d_mask, query_mask, flags);
}

int mrt_cast_grid_shadows(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1,
		const mrt_hit32 *d_hits, const mrt_light *lights, uint32_t n_lights, uint8_t *d_mask, uint32_t query_mask, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	mrt::TraceParams p;
	if (int rc = grid_source_params(ctx, cam, grid_w, grid_h, y0, y1, p)) return rc;
	return cast_shadows(ctx, mrt::ENTRY_GRID_SHADOW, mrt::SRC_SHADOW_GRID, p, d_hits, p.count, lights, n_lights, d_mask, query_mask, flags);
}

int mrt_cast_selected_shadows(mrt_ctx *ctx, const void *d_rays, const void *d_hits, uint64_t count, const mrt_light_select *desc,
		const mrt_light *lights, uint32_t n_lights, uint8_t *d_mask, uint32_t query_mask, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	mrt::TraceParams p;
	array_params(ctx, d_rays, false, p);
	const int src = (flags & MRT_FLAG_HOST_LAYOUT) ? mrt::SRC_SELSHADOW_HOST44 : mrt::SRC_SELSHADOW_RAY32;
	return cast_selected_shadows(ctx, mrt::ENTRY_SELECTED_SHADOW, src, p, d_rays, d_hits, count, 0u, desc, lights, n_lights, d_mask, query_mask, flags);
}

int mrt_cast_grid_selected_shadows(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1,
		const mrt_hit32 *d_hits, const mrt_light_select *desc, const mrt_light *lights, uint32_t n_lights, uint8_t *d_mask,
		uint32_t query_mask, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	mrt::TraceParams p;
	if (int rc = grid_source_params(ctx, cam, grid_w, grid_h, y0, y1, p)) return rc;
	return cast_selected_shadows(ctx, mrt::ENTRY_GRID_SELECTED_SHADOW, mrt::SRC_SELSHADOW_GRID, p, cam, d_hits, p.count, y0 * grid_w, desc, lights,
			n_lights, d_mask, query_mask, flags);
}

int mrt_cast_emitter_shadows(mrt_ctx *ctx, const void *d_rays, const void *d_hits, uint64_t count, const mrt_emitter_select *desc,
		uint8_t *d_mask, uint32_t query_mask, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	const bool host = (flags & MRT_FLAG_HOST_LAYOUT) != 0;
	mrt::TraceParams p;
	array_params(ctx, d_rays, host, p); // (the incoming rays are read: the normal is faced)
	return cast_emitter_shadows(ctx, mrt::ENTRY_EMITTER_SHADOW, host ? mrt::SRC_EMITSHADOW_HOST44 : mrt::SRC_EMITSHADOW_RAY32, p, d_rays, d_hits,
			count, 0u, desc, d_mask, query_mask, flags);
}

int mrt_cast_grid_emitter_shadows(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1,
		const mrt_hit32 *d_hits, const mrt_emitter_select *desc, uint8_t *d_mask, uint32_t query_mask, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	mrt::TraceParams p;
	if (int rc = grid_source_params(ctx, cam, grid_w, grid_h, y0, y1, p)) return rc;
	return cast_emitter_shadows(ctx, mrt::ENTRY_GRID_EMITTER_SHADOW, mrt::SRC_EMITSHADOW_GRID, p, cam, d_hits, p.count, y0 * grid_w, desc, d_mask,
			query_mask, flags);
}

int mrt_cast_reflections(mrt_ctx *ctx, const void *d_rays, const void *d_hits, uint64_t count, const uint8_t *d_select,
		float max_distance, void *d_out_hits, void *d_out_rays, uint32_t query_mask, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	const bool host = (flags & MRT_FLAG_HOST_LAYOUT) != 0;
	mrt::TraceParams p;
	array_params(ctx, d_rays, host, p);
	return cast_reflections(ctx, mrt::ENTRY_REFLECTION, host ? mrt::SRC_REFLECT_HOST : mrt::SRC_REFLECT_RAY32, p, d_hits, count,
			d_select, max_distance, d_out_hits, d_out_rays, query_mask, flags);
}

int mrt_cast_grid_reflections(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1,
		const mrt_hit32 *d_hits, const uint8_t *d_select, float max_distance, mrt_hit32 *d_out_hits, mrt_ray32 *d_out_rays,
		uint32_t query_mask, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	mrt::TraceParams p;
	if (int rc = grid_source_params(ctx, cam, grid_w, grid_h, y0, y1, p)) return rc;
	return cast_reflections(ctx, mrt::ENTRY_GRID_REFLECTION, mrt::SRC_REFLECT_GRID, p, d_hits, p.count, d_select, max_distance,
			d_out_hits, d_out_rays, query_mask, flags);
}

int mrt_cast_hemisphere(mrt_ctx *ctx, const void *d_rays, const void *d_hits, uint64_t count, const mrt_hemisphere *desc,
		void *d_out, void *d_out_rays, uint32_t query_mask, int mode, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	const bool host = (flags & MRT_FLAG_HOST_LAYOUT) != 0;
	mrt::TraceParams p;
	array_params(ctx, d_rays, host, p);
	return cast_hemisphere(ctx, mrt::ENTRY_HEMISPHERE, host ? mrt::SRC_HEMI_HOST : mrt::SRC_HEMI_RAY32, p, d_hits, count, 0u, desc,
			d_out, d_out_rays, query_mask, mode, flags);
}

int mrt_cast_grid_hemisphere(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1,
		const void *d_hits, const mrt_hemisphere *desc, void *d_out, void *d_out_rays, uint32_t query_mask, int mode, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	mrt::TraceParams p;
	if (int rc = grid_source_params(ctx, cam, grid_w, grid_h, y0, y1, p)) return rc;
	return cast_hemisphere(ctx, mrt::ENTRY_GRID_HEMISPHERE, mrt::SRC_HEMI_GRID, p, d_hits, p.count, y0 * grid_w, desc, d_out, d_out_rays,
			query_mask, mode, flags);
}

int mrt_cast_bounce(mrt_ctx *ctx, const void *d_rays, const void *d_hits, uint64_t count, const mrt_bounce *desc, void *d_out_hits,
		void *d_out_rays, uint32_t query_mask, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	const bool host = (flags & MRT_FLAG_HOST_LAYOUT) != 0;
	mrt::TraceParams p;
	array_params(ctx, d_rays, host, p);
	return cast_bounce(ctx, mrt::ENTRY_BOUNCE, host ? mrt::SRC_BOUNCE_HOST : mrt::SRC_BOUNCE_RAY32, p, d_hits, count, 0u, desc, d_out_hits,
			d_out_rays, query_mask, flags);
}

int mrt_cast_grid_bounce(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1,
		const void *d_hits, const mrt_bounce *desc, void *d_out_hits, void *d_out_rays, uint32_t query_mask, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	mrt::TraceParams p;
	if (int rc = grid_source_params(ctx, cam, grid_w, grid_h, y0, y1, p)) return rc;
	return cast_bounce(ctx, mrt::ENTRY_GRID_BOUNCE, mrt::SRC_BOUNCE_GRID, p, d_hits, p.count, y0 * grid_w, desc, d_out_hits, d_out_rays,
			query_mask, flags);
}

// Reflection rays from a rasteriser's G-buffer (gbuffer_kernel.h): a whole frame, count = W * H; no ray is read (the lanes are linear
// over the pixels).  The family's pair is gbuffer.h's.
int mrt_cast_gbuffer_reflections(mrt_ctx *ctx, const mrt_gbuffer *gbuffer, uint32_t W, uint32_t H, mrt_hit32 *d_out_hits,
		mrt_ray32 *d_out_rays, uint32_t query_mask, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (int rc = source_cast_check(ctx, mrt::sc::unknown_flag(false, flags) ? "unknown flag for a G-buffer reflection cast"
			: mrt::gb::cast_invalid(gbuffer, W, H, d_out_hits))) return rc;
	mrt::TraceParams p;
	base_params(ctx, p);
	p.in_fmt = mrt::IN_RAY32; // (the lanes are linear over the pixels)
	mrt::GBufferParams s;
	mrt::gb::fill_params(gbuffer, W, H, d_out_rays, s);
	return cast_batch(ctx, mrt::ENTRY_GBUFFER_REFLECTION, mrt::SRC_GBUFFER, p, mrt::sc::batch(mrt::SRC_GBUFFER, MRT_MODE_NEAREST, (uint64_t)W * H),
			d_out_hits, query_mask, s, flags);
}

} // extern "C"
