// schedule.hip — the frame-coherent tile schedule of grid casts: per-unit costs of a measuring frame, sorted on a side
// stream into the launch order of the next frames of the same grid.
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "mrt_context.h"

// ---- frame-coherent tile schedule -------------------------------------------------------------------------------------
// A grid cast ends with its slowest wave: packets differ 25-fold in cost (27 .. 667 rows at C3), and at renderer sizes
// (1 - 2 M rays = 2 - 4 rounds of waves) the last round's long walks leave most of the chip idle: 1920x1080 ran at 3.8 Grays/s
// against 9 at 4096^2.  Which tiles are expensive barely changes from one frame to the next, so every wave notes the
// shader cycles its tile(s) took (TraceParams::tile_cost), a radix sort on a side stream turns that into a launch order,
// longest first, and the next cast of the same grid (same size and rows; any camera: the order is only a permutation,
// results never depend on it) launches in that order: the long walks start first and the short ones fill the gaps behind
// them (longest-processing-time-first).  The first cast of a grid runs in the plain order.  mrt_options.tile_schedule = 1
// turns it off.  For batches of 2^19 up to (not including) 2^24 rays: 1280x720 -17 %, 1920x1080 -18 %, 3840x2160 -13 %; at 4096^2
// and above the gain is 2-4 % in kernel time and less than what the bookkeeping costs a blocking call; 640x360 measured 7 %
// slower with it (too few tiles to reorder).  The order is renewed every kScheduleRenew-th frame, not every frame: which
// tiles are expensive changes slowly, and a sort that runs beside the start of the next frame delays exactly the long walks
// that frame launches first (1920x1080: 0.52 against 0.44 ms with a sort per frame).  A batch whose row width is found on the device
// (mrt_cast with MRT_FLAG_COHERENT) is scheduled from the width the previous cast of the same size found.
// The launch list of a generation: the sorted order, with the units whose cost says they would end the frame alone launched in
// pieces (TraceParams::tile_sched).  A frame of 1-2 M rays is one or two rounds of waves, so it lasts as long as its longest
// walk, and the cost arrays say the longest walks are few and far out: at 1920x1080 on the C3 scene one pair of tiles takes
// 1.4 M cycles, the 99th percentile 0.57 M, and all pairs together 0.68 M per wave slot.  A unit above BOTH the work per wave
// slot and the cost of rank n / 100 goes in quarter tiles (4x4 pixels in 16 lanes; eight of them for a pair: each takes
// 0.18 of the pair, all eight 1.5 x the pair); pieces first, so the longest things still start first.  Whether that pays
// depends on how many rounds of waves the frame is: 1920x1080 (two rounds of pairs) 0.60 -> 0.37 ms, 1280x960 (1.2 rounds)
// 0.323 -> 0.337 ms -- every extra wave pushes a whole unit into the second round, and the pieces' work is half again their
// unit's; a deeper cut (the work per wave slot alone as the bound) 0.378 ms, only far outliers (1.25 x the 99th percentile)
// nothing at 1280x960 and 0.43 ms at 1920x1080.  So the rule stays simple and the kernel tuner MEASURES it: a grid's frames
// 3-5 run the 128-ray walk with pieces, 6-8 without, and the faster way is kept (tune_grid_kernel).
// hdr = {units in quarters, units in single tiles (unused: 0), slots}.  MRT_SCHED_SPLIT_PCT: the rank, in percent (default 1).
__global__ __launch_bounds__(1024) void schedule_plan_kernel(const uint32_t *cost_sorted, uint32_t n_units, uint32_t unit, uint32_t n_extra, uint32_t rank, uint32_t *hdr)
{
	__shared__ unsigned long long part[16];
	unsigned long long sum = 0ull;
	for (uint32_t i = threadIdx.x; i < n_units; i += 1024u) sum += cost_sorted[i];
	for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
	if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = sum;
	__syncthreads();
	if (threadIdx.x != 0u) return;
	sum = 0ull;
	for (int w = 0; w < 16; w++) sum += part[w];
	unsigned long long thr = sum / mrt::kWaveSlots;
	if (rank < n_units && (unsigned long long)cost_sorted[rank] > thr) thr = cost_sorted[rank];
	// cost_sorted is descending: how many lie above the bound
	uint32_t lo = 0u, hi = n_units;
	while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if ((unsigned long long)cost_sorted[mid] > thr) lo = mid + 1u; else hi = mid; }
	const uint32_t per_quartered = unit == 2u ? 7u : 3u; // extra slots of a unit in quarters
	uint32_t quartered = sum == 0ull ? 0u : lo;
	// fewer units than wave slots: the frame is one round of waves and lasts as long as its longest walk; the most expensive units
	// go in quarters until the round is full (C3 scene, 64-ray kernel: 512^2 0.305 -> 0.248 ms, 640x360 0.284 -> 0.227, 960x540
	// 0.378 -> 0.309; filling to 1.25 or 1.5 rounds instead: 0.293 / 0.317 at 512^2)
	if (sum != 0ull && n_units < mrt::kWaveSlots && (mrt::kWaveSlots - n_units) / per_quartered > quartered) quartered = (mrt::kWaveSlots - n_units) / per_quartered;
	if (quartered > n_units) quartered = n_units;
	if ((unsigned long long)quartered * per_quartered > n_extra) quartered = n_extra / per_quartered;
	hdr[0] = quartered; hdr[1] = 0u; hdr[2] = n_units + quartered * per_quartered;
}
__global__ __launch_bounds__(256) void schedule_fill_kernel(const uint32_t *order, uint32_t n_units, uint32_t unit, const uint32_t *hdr, uint32_t *slots)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n_units) return;
	const uint32_t quartered = hdr[0], halved = hdr[1], u = order[i], pieces = unit == 2u ? 8u : 4u;
	if (i < quartered) {
		for (uint32_t k = 0; k < pieces; k++) slots[i * pieces + k] = ((2u + (k & 3u)) << 28) | (u * unit + (k >> 2));
	} else if (i < quartered + halved) {
		const uint32_t at = quartered * pieces + (i - quartered) * 2u;
		slots[at] = (1u << 28) | (u * 2u); slots[at + 1u] = (1u << 28) | (u * 2u + 1u);
	} else slots[quartered * pieces + halved * 2u + (i - quartered - halved)] = u;
}

// Before the launch: the units of this grid, the newest finished order of the same grid, and -- on a measuring frame -- a
// zeroed cost array.  Two generations of (cost, order): generation g is sorted on the side stream while later frames already
// run in the order of generation g - 1; no frame waits for a running sort.
constexpr uint32_t kScheduleRenew = 8;
int schedule_grid(mrt_ctx *ctx, const mrt::CastPlan &c, mrt::TraceParams &p)
{
	auto &s = ctx->sched[ctx->grids.cur];
	const uint32_t th = 64u >> p.tile_w_log2;
	const uint32_t tiles_y = (c.rows + th - 1u) / th;
	const uint32_t unit = c.kernel == MRT_KERNEL_PACKET_DUAL ? 2u : 1u;
	const uint32_t n_units = (uint32_t)(((uint64_t)c.tiles_x * tiles_y + unit - 1u) / unit);
	const bool pieces = c.pieces;
	const bool same = s.grid_w == c.grid_w && s.grid_h == c.grid_h && s.y0 == c.y0 && s.rows == c.rows && s.unit == unit &&
			s.n_units == n_units && s.tile_w_log2 == p.tile_w_log2 && s.pieces == pieces;
	int rc;
	if (!s.side) {
		HIP_TRY(ctx, hipStreamCreateWithFlags(&s.side, hipStreamNonBlocking));
		HIP_TRY(ctx, hipEventCreateWithFlags(&s.traced, hipEventDisableTiming));
		for (int k = 0; k < 2; k++) HIP_TRY(ctx, hipEventCreateWithFlags(&s.ready[k], hipEventDisableTiming));
	}
	if (!same) {
		HIP_TRY(ctx, hipStreamSynchronize(s.side)); // no sort of the old grid may still use the arrays
		// room for pieces: half as many extra slots as there are units, or what fills one round of waves (schedule_plan_kernel)
		s.n_slots_max = mrt::schedule_slots(n_units, pieces);
		for (int k = 0; k < 2; k++)
			if ((rc = ensure(ctx, s.cost[k], ((size_t)n_units + s.n_slots_max) * 4)) || (rc = ensure(ctx, s.order[k], (size_t)n_units * 4)) ||
					(rc = ensure(ctx, s.slots[k], (size_t)s.n_slots_max * 4)) || (rc = ensure(ctx, s.hdr[k], 16))) return rc;
		if ((rc = ensure(ctx, s.cost_sorted, (size_t)n_units * 4)) || (rc = ensure(ctx, s.iota, (size_t)n_units * 4))) return rc;
		std::vector<uint32_t> iota(n_units);
		for (uint32_t i = 0; i < n_units; i++) iota[i] = i;
		HIP_TRY(ctx, hipMemcpyAsync(s.iota.ptr, iota.data(), (size_t)n_units * 4, hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (the host vector goes out of scope)
		s.forget();
		s.frame = 0; s.gen = 0;
	}
	s.grid_w = c.grid_w; s.grid_h = c.grid_h; s.y0 = c.y0; s.rows = c.rows; s.unit = unit; s.n_units = n_units; s.tile_w_log2 = p.tile_w_log2; s.pieces = pieces;
	const uint32_t cur = s.gen & 1u, newest = cur ^ 1u;     // the slot the next generation goes to, the slot of the last one
	// the order to launch in: the last generation's if its sort is done, else the one before (still intact in slot `cur`:
	// that slot's ORDER array is rewritten only by the next sort, which runs after this frame's trace)
	if (c.wait_sorts) HIP_TRY(ctx, hipStreamSynchronize(s.side));
	const uint32_t *order = nullptr, *hdr = nullptr;
	if (s.have_order[newest] && hipEventQuery(s.ready[newest]) == hipSuccess) { order = (const uint32_t *)s.slots[newest].ptr; hdr = (const uint32_t *)s.hdr[newest].ptr; }
	(void)hipGetLastError(); // (hipErrorNotReady is not an error)
	if (!order && s.have_order[cur] && hipEventQuery(s.ready[cur]) == hipSuccess) { order = (const uint32_t *)s.slots[cur].ptr; hdr = (const uint32_t *)s.hdr[cur].ptr; }
	(void)hipGetLastError();
	// a measuring frame: the first two of a grid, then every kScheduleRenew-th -- if the slot's previous sort is done
	s.measuring = (s.gen < 2u || s.frame % kScheduleRenew == 0u) && (!s.have_order[cur] || hipEventQuery(s.ready[cur]) == hipSuccess);
	(void)hipGetLastError();
	if (s.measuring) HIP_TRY(ctx, hipMemsetAsync(s.cost[cur].ptr, 0, (size_t)n_units * 4, ctx->stream));
	p.tile_sched = order; p.sched_hdr = hdr; p.n_slots_max = order ? s.n_slots_max : 0u;
	p.tile_cost = s.measuring ? (uint32_t *)s.cost[cur].ptr : nullptr;
	p.tile_unit = unit; p.n_units = n_units;
	ctx->sched_counts[0]++;
	if (order) ctx->sched_counts[1]++;
	return MRT_OK;
}

// After the launch (ev[4] recorded on the context's stream): on a measuring frame, sort its units by cost, descending, on the
// side stream.
int schedule_sort(mrt_ctx *ctx)
{
	auto &s = ctx->sched[ctx->grids.cur];
	s.frame++;
	if (!s.measuring) return MRT_OK;
	const uint32_t cur = s.gen & 1u;
	HIP_TRY(ctx, hipEventRecord(s.traced, ctx->stream));
	HIP_TRY(ctx, hipStreamWaitEvent(s.side, s.traced, 0));
	size_t tmp_bytes = 0;
	uint32_t *ki = (uint32_t *)s.cost[cur].ptr, *ko = (uint32_t *)s.cost_sorted.ptr, *vi = (uint32_t *)s.iota.ptr, *vo = (uint32_t *)s.order[cur].ptr;
	HIP_TRY(ctx, rocprim::radix_sort_pairs_desc(nullptr, tmp_bytes, ki, ko, vi, vo, (size_t)s.n_units, 0, 32, s.side));
	int rc;
	if (s.tmp.cap < tmp_bytes) { HIP_TRY(ctx, hipStreamSynchronize(s.side)); if ((rc = ensure(ctx, s.tmp, tmp_bytes))) return rc; }
	HIP_TRY(ctx, rocprim::radix_sort_pairs_desc(s.tmp.ptr, tmp_bytes, ki, ko, vi, vo, (size_t)s.n_units, 0, 32, s.side));
	hipLaunchKernelGGL(schedule_plan_kernel, dim3(1), dim3(1024), 0, s.side, ko, s.n_units, s.unit, s.n_slots_max - s.n_units, (uint32_t)((uint64_t)s.n_units * ctx->knobs.split_pct / 100u),
			(uint32_t *)s.hdr[cur].ptr);
	hipLaunchKernelGGL(schedule_fill_kernel, dim3((s.n_units + 255u) / 256u), dim3(256), 0, s.side, vo, s.n_units, s.unit, (const uint32_t *)s.hdr[cur].ptr, (uint32_t *)s.slots[cur].ptr);
	HIP_TRY(ctx, hipGetLastError());
	HIP_TRY(ctx, hipEventRecord(s.ready[cur], s.side));
	s.have_order[cur] = true;
	s.gen++;
	ctx->sched_counts[2]++;
	if (ctx->knobs.dump) { // diagnosis: what the schedule was made of (tools/bench_resolutions.py with MRT_SCHED_DUMP=1)
		std::vector<uint32_t> c(s.n_units);
		uint32_t hdr[3] = {0, 0, 0};
		HIP_TRY(ctx, hipStreamSynchronize(s.side));
		HIP_TRY(ctx, hipMemcpy(c.data(), s.cost_sorted.ptr, (size_t)s.n_units * 4, hipMemcpyDeviceToHost));
		HIP_TRY(ctx, hipMemcpy(hdr, s.hdr[cur].ptr, sizeof(hdr), hipMemcpyDeviceToHost));
		unsigned long long sum = 0; for (uint32_t v : c) sum += v;
		std::fprintf(stderr, "[mrt schedule] %ux%u unit %u: %u units, cycles sum %llu, max %u, p99 %u, median %u, min %u; next launch: %u units in quarter tiles, %u slots\n", s.grid_w, s.rows, s.unit,
				s.n_units, sum, c.empty() ? 0u : c[0], c.empty() ? 0u : c[s.n_units / 100], c.empty() ? 0u : c[s.n_units / 2], c.empty() ? 0u : c[s.n_units - 1], hdr[0], hdr[2]);
	}
	return MRT_OK;
}
