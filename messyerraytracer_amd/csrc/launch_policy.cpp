// launch_policy.cpp — the cast launch policy (launch_policy.h): plain host code, no HIP.
#include <cstdint>
#include <cstdio>
#include "../../include/mrt_hip.h"
#include "mrt_internal.h"
#include "launch_policy.h"

namespace mrt {
namespace {

bool persistent_lane_kernel(uint32_t k)
{
	return k == MRT_KERNEL_LANE_PERSISTENT || k == MRT_KERNEL_LANE4_PERSISTENT || k == MRT_KERNEL_LANE8_PERSISTENT;
}
bool lane_kernel(uint32_t k) { return k == MRT_KERNEL_LANE || k == MRT_KERNEL_TWO_LEVEL; }

// MRT_KERNEL_AUTO: packets for batches the caller declares coherent (RayQuery::coherent,
// primary-ray grids), one lane per ray for everything else (sorted / incoherent batches).
uint32_t pick_kernel(const mrt_options &o, const SceneFacts &s, bool coherent, uint64_t count)
{
	// a two-level scene has its own pair of kernels (two_level_kernel.h)
	// Packets pay once there are enough of them: a wave that walks for 64 rays is a long serial chain (0.3 - 0.7 ms on a
	// 1 M-triangle scene, the longer the wider its 8x8 tile opens), and a small batch is over when its slowest wave is.
	// Coherent grids on the C3 scene (tools/bench_small_batches.py, profiles/r02d_small_batches.txt): 64^2 rays 0.69 ms by
	// packets, 0.32 ms one lane per ray; 128^2 0.56 / 0.40; 256^2 0.40 / 0.43; 512^2 0.35 / 0.59 (C2 scene: even at 128^2).
	// (Batches whose tiling is known or found -- grids, tiled casts, mrt_cast(COHERENT) -- leave this rule from 2^11 rays on:
	// the quarter rule of plan_cast runs them by packets of 16 rays, faster than either.)
	const bool few = o.kernel == MRT_KERNEL_AUTO && count < (1ull << 15);
	if (s.two_level) return coherent && !few && o.kernel != MRT_KERNEL_LANE ? MRT_KERNEL_TWO_LEVEL_PACKET : MRT_KERNEL_TWO_LEVEL;
	if (o.kernel == MRT_KERNEL_PACKET_DUAL || o.kernel == MRT_KERNEL_PACKET_ROWS)
		return !coherent ? MRT_KERNEL_LANE : (s.rows ? o.kernel : MRT_KERNEL_PACKET_ASM);
	if (o.kernel == MRT_KERNEL_PACKET_QUAD)
		return !coherent ? MRT_KERNEL_LANE : (s.rows4 ? MRT_KERNEL_PACKET_QUAD : MRT_KERNEL_PACKET_ASM);
	if (o.kernel >= MRT_KERNEL_LANE && o.kernel <= MRT_KERNEL_LANE8_PERSISTENT) return o.kernel;
	if (!coherent || few) return MRT_KERNEL_LANE;
	// Coherent batches: the 128-ray shared walk over the row array (packet_rows_kernel.h) once the batch is large
	// enough to fill the chip with half as many waves (C3 2.16 -> 2.06 ms, C5 23.2 -> 21.2 ms; C2's 2^20 rays are
	// 7 % faster with one packet per wave: 0.188 against 0.202 ms), else the 64-ray packet kernel with the
	// hand-written node loop.
	return (s.rows && count >= (1ull << 22)) ? MRT_KERNEL_PACKET_DUAL : MRT_KERNEL_PACKET_ASM;
}

bool schedule_applies(const mrt_options &o, const SceneFacts &s, const Knobs &k, uint32_t lane_map, uint64_t count, uint32_t kernel)
{
	if (o.tile_schedule == 1u || o.count_visits) return false;
	if ((lane_map != MAP_TILE8X8 && lane_map != MAP_AUTO) || count < k.schedule_min_rays || count >= kScheduleMaxRays) return false;
	return kernel == MRT_KERNEL_PACKET_ASM || (kernel == MRT_KERNEL_PACKET_DUAL && s.rows);
}

// The kernel of a mid-size grid cast, by measurement (GridTune).  Only for MRT_KERNEL_AUTO on flat scenes, blocking
// casts (a timing is needed), grids the schedule applies to.
uint32_t tune_grid_kernel(GridTune &t, const mrt_options &o, const SceneFacts &s, const Knobs &k, const GridKey &g, uint64_t count,
		uint32_t lane_map, uint32_t quarter_all, uint32_t kernel, uint32_t flags)
{
	t.armed = false; t.no_pieces = false;
	if (o.kernel != MRT_KERNEL_AUTO || s.two_level || !s.rows || o.count_visits || o.tile_schedule == 1u) return kernel;
	// (from 2^22 rays on the 128-ray walk won every measurement -- 2560x1440 .. 7680x4320, C5's row blocks --: no frames are spent on the other one)
	if (lane_map != MAP_TILE8X8 || quarter_all || count < k.schedule_min_rays || count < k.tune_min_rays || count >= kScheduleMaxRays || count >= (1ull << 22)) return kernel;
	if (kernel != MRT_KERNEL_PACKET_ASM && kernel != MRT_KERNEL_PACKET_DUAL) return kernel;
	const bool same = t.grid_w == g.w && t.grid_h == g.h && t.y0 == g.y0 && t.rows == g.rows && t.mode == g.mode;
	if (!same) { t.grid_w = g.w; t.grid_h = g.h; t.y0 = g.y0; t.rows = g.rows; t.mode = g.mode; t.phase = 0; t.t_asm = t.t_dual = t.t_whole = 0.0f; }
	// frames 0-3: the 64-ray kernel; 4-7: the 128-ray walk, its most expensive units in pieces (schedule_plan_kernel); 8-11: the
	// same with every unit whole; then the fastest of the three (each by the faster of its last two frames)
	if (t.phase < kTuneFrames) kernel = MRT_KERNEL_PACKET_ASM;
	else if (t.phase < 2 * kTuneFrames) kernel = MRT_KERNEL_PACKET_DUAL;
	else if (t.phase < 3 * kTuneFrames) { kernel = MRT_KERNEL_PACKET_DUAL; t.no_pieces = true; }
	else {
		const bool whole = t.t_whole <= t.t_dual * 1.03f; // (pieces must win by more than the noise of two timings)
		const float best_dual = whole ? t.t_whole : t.t_dual;
		kernel = best_dual < t.t_asm ? MRT_KERNEL_PACKET_DUAL : MRT_KERNEL_PACKET_ASM;
		t.no_pieces = kernel == MRT_KERNEL_PACKET_DUAL && whole;
	}
	t.armed = t.phase < 3 * kTuneFrames && !(flags & MRT_FLAG_ASYNC);   // an ASYNC cast has no timing: the phase waits for a blocking one
	return kernel;
}

// Lane kernel launch: plain (one fixed ray per lane) or persistent (resident waves pulling rays
// from a counter, short LDS stack with HBM spill).
LaneLaunch lane_launch(const mrt_options &o, const SceneFacts &s, uint64_t count, uint32_t lane_map, bool persistent)
{
	LaneLaunch l;
	// The wide walks exist in persistent form only.  For large incoherent batches MRT_KERNEL_AUTO takes the
	// 8-wide compressed layout when the scene has it (6.1 ms at C4), else the 4-wide one (7.7 ms), else the
	// 2-wide persistent kernel (11.0 ms).
	const bool wide4 = s.nodes4 && (o.kernel == MRT_KERNEL_LANE4_PERSISTENT || (o.kernel == MRT_KERNEL_AUTO && persistent));
	const bool wide8 = s.nodes8 && (o.kernel == MRT_KERNEL_LANE8_PERSISTENT || (o.kernel == MRT_KERNEL_AUTO && persistent));
	// counting builds: the persistent kernels count for flat scenes; two-level scenes take the plain lane kernel
	const bool can_count = !o.count_visits || !s.two_level;
	if ((wide4 || wide8) && can_count) persistent = true;
	if (!persistent || !can_count) {
		l.kernel = s.two_level ? MRT_KERNEL_TWO_LEVEL : MRT_KERNEL_LANE;
		// A small batch on more, emptier waves: with fewer rays than the device has wave slots (8 192) every ray gets a wave of its
		// own, up to 2^15 rays two or four share one.  A wave's walk is as long as its longest ray's and every step costs as many
		// memory requests as it has rays; a batch this small ends with its longest wave (blocking mrt_cast of incoherent rays in
		// host arrays: 256 rays 190 -> 97 us, 1 024 rays 247 -> 125, 4 096 rays 317 -> 210; 2^14 device-resident rays 503 -> 338;
		// on the C5 two-level scene 256 rays 1 649 -> 319 us, 4 096 rays 2 272 -> 646; profiles/r03_latency.txt)
		if (lane_map == MAP_LINEAR && count <= (kWaveSlots << 2)) {
			l.sparse_lanes = 1u;
			while ((count + l.sparse_lanes - 1u) / l.sparse_lanes > kWaveSlots) l.sparse_lanes <<= 1;
		}
		l.count = o.count_visits != 0;
		return l;
	}
	l.persistent = true;
	l.lds_depth = o.stack_override >= 4 && o.stack_override <= 64 ? o.stack_override : 16u;
	const uint32_t lds_bytes = 4u * l.lds_depth * 64u * 4u; // per 256-thread workgroup
	uint32_t wg_per_cu = (160u * 1024u) / lds_bytes; if (wg_per_cu > 8u) wg_per_cu = 8u;
	const uint64_t blocks = (uint64_t)s.cu_count * wg_per_cu, needed = (count + 255u) / 256u;
	l.blocks = (uint32_t)(blocks > needed ? needed : blocks);
	const uint32_t need = wide8 ? s.stack8 : (wide4 ? s.stack4 : s.depth); // entries one ray can have pending
	l.spill = need > l.lds_depth ? need - l.lds_depth : 0u; // deeper entries spill to [depth - lds_depth][thread] in HBM
	l.kernel = wide8 ? MRT_KERNEL_LANE8_PERSISTENT : (wide4 ? MRT_KERNEL_LANE4_PERSISTENT : MRT_KERNEL_LANE_PERSISTENT);
	if (s.two_level) l.kernel = wide8 ? MRT_KERNEL_TWO_LEVEL_PERSISTENT8 : MRT_KERNEL_TWO_LEVEL_PERSISTENT; // need = stack8 (= depth8) / depth
	l.refill = o.refill ? o.refill : 16u;
	l.leaf_wait = o.leaf_wait ? o.leaf_wait : (wide8 ? 8u : 16u);
	l.count = o.count_visits != 0 && !s.two_level;
	return l;
}

// Small grids of known width (mrt_cast_grid, mrt_cast_tiled; flat scenes, MRT_KERNEL_AUTO; mrt_cast(COHERENT) does the same for a
// width found on the device): the 64-ray packet kernel with EVERY tile launched in pieces (TraceParams::quarter_all) -- up to 512
// tiles as its sixteen 2x2-pixel sixteenths (4 rays in lanes 0..3 of a wave), up to 3 600 tiles as its four 4x4-pixel quarters (16
// rays).  Such a grid has fewer tiles than the device has wave slots (8 192), so it lasts as long as its longest walk whatever the
// order, and a walk for 16 rays is about half as long as its tile's, one for 4 rays a third.  C3 scene, kernel time in ms (whole
// tiles by packets / one lane per ray / quarters / sixteenths): 16x12 - / 0.23 / - / 0.15, 32^2 1.22 / 0.34 / 0.36 / 0.15, 64^2 0.67 /
// 0.31 / 0.26 / 0.12, 128^2 0.53 / 0.37 / 0.20 / 0.18, 192^2 0.46 / 0.45 / 0.25 / 0.22, 256^2 0.37 / 0.40 / 0.24 / 0.25, 384^2 0.34 / 0.47 /
// 0.25, 640x360 0.38 / 0.55 / 0.29; sixteen times as many waves are two rounds of them from 1 024 tiles on, four times as many from
// 4 096 (512^2: 0.32 / 0.55 / 0.32), and nothing is gained.  The C2 scene draws the same lines (64^2 0.38 / 0.27 / 0.18 / 0.09;
// 192^2 - / - / 0.10 / 0.10; 256^2 - / - / 0.09 / 0.15).  Between 2 048 and 8 192 tiles the cost history picks the tiles (schedule_plan_kernel).
// Two-level scenes go the same way with their own packet kernel (whose walks are longer still: a ray crosses several instances):
// C5 as a two-level scene, 64^2 2.56 -> 0.95 ms, 128^2 2.78 -> 0.83, 256^2 4.14 -> 1.73, 640x360 2.10 -> 1.79.
// Two rules that look alike: `units` are the tiles of a grid of known width, but rays / 64 (rounded up) for a width found on the
// device, whose grid is not known when the kernel is chosen -- a grid with clipped tiles has more tiles than that.
void quarter_rule(const mrt_options &o, const SceneFacts &s, uint64_t count, uint64_t units, CastPlan &c)
{
	if (o.kernel != MRT_KERNEL_AUTO || o.count_visits || tile_w_log2(o) != 3u || s.n_nodes >= kAsmNodeLimit) return;
	if (count < kQuarterMinRays || units > kQuarterMaxTiles) return;
	c.kernel = s.two_level ? MRT_KERNEL_TWO_LEVEL_PACKET : MRT_KERNEL_PACKET_ASM; // (a two-level scene: its packet kernel maps lanes the same way)
	c.quarter_all = units <= kSixteenthMaxTiles ? 2u : 1u;
}

} // namespace

uint32_t tile_w_log2(const mrt_options &o) { return o.tile_w_log2 >= 1 && o.tile_w_log2 <= 6 ? o.tile_w_log2 : 3u; }

int select_grid_state(GridStates &g, const GridKey &k)
{
	int pick = -1, oldest = 0;
	for (int i = 0; i < GridStates::kCount; i++) {
		const GridKey &q = g.e[i].key;
		if (q.mode == k.mode && q.w == k.w && q.h == k.h && q.y0 == k.y0 && q.rows == k.rows) { pick = i; break; }
		if (g.e[i].stamp < g.e[oldest].stamp) oldest = i;
	}
	if (pick < 0) { pick = oldest; g.e[pick].key = k; }
	g.e[pick].stamp = ++g.clock;
	return g.cur = pick;
}

void DetectMemo::waited(const volatile uint32_t *words)
{
	if (!queued_since_wait) return; // nothing queued since the last wait: the words have not changed
	seen.pending = false;
	seen.count = queued_count;
	for (int i = 0; i < 4; i++) seen.word[i] = queued_count ? words[i] : 0u;
	queued_since_wait = false;
}

void tune_record(GridTune &t, float trace_ms)
{
	if (!t.armed) return;
	// the faster of a candidate's last two frames (both launched in a measured order: schedule_grid waits for the sorts behind them)
	const int cand = t.phase / kTuneFrames, at = t.phase % kTuneFrames;
	float &slot = cand == 0 ? t.t_asm : (cand == 1 ? t.t_dual : t.t_whole);
	if (at == kTuneFrames - 2) slot = trace_ms;
	if (at == kTuneFrames - 1 && trace_ms < slot) slot = trace_ms;
	t.phase++;
	t.armed = false;
}

// Record-driven casts (shadow, selected shadow, reflection, hemisphere, bounce: record_cast_entry): count rays made in the kernel from resident hit records
// -- pixels * lights any-hit shadow rays or one per record to a drawn light, one closest-hit mirror or bounce ray per record, pixels * samples hemisphere rays in either
// mode -- in entry order (which already groups nearby origins, though hemisphere and bounce rays are far less coherent than the
// others).  A G-buffer reflection cast (ENTRY_GBUFFER_REFLECTION: one mirror ray per pixel from depth and normal buffers, in pixel order)
// is the same kind of batch.  One plan for all of them, since neither the family nor the mode enters it:
//   - never sorted: the rays never exist in memory, so there is nothing to sort; no detection and no tiling;
//   - the lane kernels as for any incoherent batch: the plain one below 2^16 rays (small batches on emptier waves), the persistent ones
//     from 2^16 (8-, 4- or 2-wide, two-level scenes their own);
//   - the packet kernels have no ray source: a forced one means the policy's own lane kernel;
//   - there is no counting variant;
//   - nothing of the grid state (detected widths, the grid tuner, tile schedules) is read or changed: a renderer that alternates primary
//     casts with these keeps its primary grid's plan exactly as it is without them.
static CastPlan plan_source(const mrt_options &o, const SceneFacts &s, const CastRequest &r)
{
	CastPlan c;
	mrt_options so = o;
	so.count_visits = 0;
	if (so.kernel != MRT_KERNEL_LANE && !persistent_lane_kernel(so.kernel)) so.kernel = MRT_KERNEL_AUTO;
	const uint32_t kernel = pick_kernel(so, s, false, r.count);
	const bool persistent = persistent_lane_kernel(kernel) || (so.kernel == MRT_KERNEL_AUTO && r.count >= 65536);
	c.launch = CastPlan::LANE;
	c.lane = lane_launch(so, s, r.count, MAP_LINEAR, persistent);
	c.kernel = c.lane.kernel;
	c.launches = (r.flags & MRT_FLAG_ASYNC) ? 0 : 1;
	return c;
}

CastPlan plan_cast(const mrt_options &o, const SceneFacts &s, const CastRequest &r, const PrevDetect &prev, const Knobs &k, GridStates &gs)
{
	if (record_cast_entry(r.entry)) return plan_source(o, s, r);
	CastPlan c;
	const uint64_t n = r.count;
	const bool auto_k = o.kernel == MRT_KERNEL_AUTO, coherent = (r.flags & MRT_FLAG_COHERENT) != 0;
	const uint32_t tw = tile_w_log2(o), th = 64u >> tw;
	gs.tune().armed = false; // (the grid tuner times a cast only if THIS cast asks it to)
	if (ray_entry(r.entry)) {
		const uint32_t thr = o.sort_threshold ? o.sort_threshold : 256u; // MIN_BATCH_FOR_SORTING
		// (a batch of at most 8 192 rays runs one ray per wave in the lane kernel, lane_launch: there is no wave whose rays a sort could
		// bring together, and its three launches are a third of such a cast's time)
		const bool one_ray_waves = auto_k && n <= kWaveSlots && !(r.flags & MRT_FLAG_FORCE_SORT);
		c.sort = !coherent && !one_ray_waves && (n >= thr || (r.flags & MRT_FLAG_FORCE_SORT));
		c.kernel = pick_kernel(o, s, !c.sort && coherent, n);
		const bool persistent_kind = persistent_lane_kernel(c.kernel);
		// Coherent batch without a declared width: look for the row width on the device and let the
		// trace kernel tile its lanes (no host round trip: the kernel reads the answer from HBM).
		// Timed with the sort as pre-processing (last_sort_ms); last_trace_ms is the trace kernel alone.
		c.detect = !c.sort && coherent && n >= 256 && o.grid_tile != 1 && !persistent_kind;
		c.lane_map = c.detect ? MAP_AUTO : MAP_LINEAR;
		// a small batch whose width the device finds: sixteenth or quarter tiles (if no width is found the lanes stay linear and the
		// waves past the batch have nothing to do)
		if (c.detect && (c.kernel == MRT_KERNEL_PACKET_ASM || lane_kernel(c.kernel) || c.kernel == MRT_KERNEL_TWO_LEVEL_PACKET))
			quarter_rule(o, s, n, n / 64u + (n % 64u != 0u), c);
		// the tile schedule for a batch whose width the device finds: sized from what the previous cast of as many rays found ...
		if (c.detect && !prev.pending && prev.count == n && prev.word[0] != 0u && prev.word[3] == 0u &&
				schedule_applies(o, s, k, c.lane_map, n, c.kernel) && !(c.quarter_all && n <= kQuarterAllRays)) {
			c.scheduled = true; c.quarter_all = 0u;
			c.grid_w = prev.word[0]; c.rows = c.grid_h = prev.word[1]; c.tiles_x = prev.word[2];
			// ... and so is the way it is cast: the grid tuner's candidates, as for a grid cast of that width (mrt_cast records the timing)
			const GridKey key{c.grid_w, c.grid_h, 0u, c.rows, r.mode};
			select_grid_state(gs, key);
			c.kernel = tune_grid_kernel(gs.tune(), o, s, k, key, n, MAP_TILE8X8, 0u, c.kernel, r.flags);
		}
		c.launches = c.sort ? 3 : (c.detect ? 2 : 1);
		if (c.detect && auto_k && !o.count_visits && !lane_kernel(c.kernel)) {
			// The caller said "coherent"; the device checks.  Packet launch first, lane launch behind it:
			// detect_grid_kernel's verdict (auto_grid[3]) makes exactly one of them do the work.  The lane launch is
			// persistent from 2^16 rays, the bound below, but its lanes are linear whatever the device finds (a two-level
			// scene: its own lane kernels).
			c.launch = CastPlan::DUAL;
			c.lane = lane_launch(o, s, n, MAP_LINEAR, n >= 65536);
		} else if (persistent_kind || lane_kernel(c.kernel)) {
			// large incoherent batches: resident waves that pull rays from a counter (no counting variant)
			const bool persistent = c.lane_map == MAP_LINEAR && (persistent_kind || (auto_k && n >= 65536));
			c.launch = CastPlan::LANE;
			c.lane = lane_launch(o, s, n, c.lane_map, persistent);
			c.kernel = c.lane.kernel;
		}
	} else {
		// a grid of known width: mrt_cast_grid, mrt_cast_tiled
		c.grid_w = r.grid_w; c.grid_h = r.grid_h; c.y0 = r.y0; c.rows = r.rows;
		c.tiles_x = (r.grid_w + (1u << tw) - 1u) >> tw;
		c.lane_map = o.grid_tile == 1 ? MAP_LINEAR : MAP_TILE8X8;
		c.kernel = pick_kernel(o, s, true, n);
		if (c.lane_map == MAP_TILE8X8) quarter_rule(o, s, n, (uint64_t)c.tiles_x * ((r.rows + 7u) / 8u), c);
		if (r.entry == ENTRY_GRID) {
			const GridKey key{r.grid_w, r.grid_h, r.y0, r.rows, r.mode};
			if (n >= k.schedule_min_rays) select_grid_state(gs, key);
			c.kernel = tune_grid_kernel(gs.tune(), o, s, k, key, n, c.lane_map, c.quarter_all, c.kernel, r.flags);
			// (from 2 048 tiles on the cost history says WHICH tiles go in quarters)
			c.scheduled = schedule_applies(o, s, k, c.lane_map, n, c.kernel) && !(c.quarter_all && n <= kQuarterAllRays);
			if (c.scheduled) c.quarter_all = 0u;
		}
		c.launches = r.entry == ENTRY_GRID && (r.flags & MRT_FLAG_ASYNC) ? 0 : 1; // (an ASYNC grid cast leaves the count as it was)
	}
	c.count = o.count_visits != 0;
	const GridTune &t = gs.tune();
	if (c.scheduled) {
		// pieces: 8x8 tiles only, ids within the entry's 28 bits, not while the kernel tuner tries (or has chosen) the frames without
		const uint64_t tiles = (uint64_t)c.tiles_x * ((c.rows + th - 1u) / th);
		c.pieces = tw == 3u && o.tile_schedule != 2u && tiles < (1ull << 28) && !t.no_pieces;
		// the frame the kernel tuner times (the third of a kernel) waits for the sorts behind it: it is launched the way later frames will be
		c.wait_sorts = t.armed && t.phase % kTuneFrames >= kTuneFrames - 2;
	}
	// only a blocking mrt_cast / mrt_cast_grid records its time (a submitted cast is collected later, pipeline chunks are not timed
	// one by one)
	c.arms_tuner = t.armed && (r.entry == ENTRY_CAST || r.entry == ENTRY_GRID);
	gs.tune().armed = c.arms_tuner;
	return c;
}

// ---- plan -> variant -> launch -> label (launch_policy.h) ------------------------------------------------------------------------
namespace {

constexpr uint32_t kWg = 256, kWave = 64; // MRT_WG and MRT_WAVE of kernels.hip: every kernel's workgroup but the 128-ray walk's

// the per-lane LDS stack of the lane kernels: entry d of lane l at dword d * 64 + l of its wave's region
size_t lane_stack_lds(uint32_t depth) { return (size_t)(kWg / kWave) * depth * kWave * sizeof(uint32_t); }
uint32_t pieces_per_tile(uint32_t quarter_all) { return quarter_all == 2u ? 16u : (quarter_all ? 4u : 1u); }
uint64_t linear_lanes(const TraceParams &p) { return p.sparse_lanes ? (p.count + p.sparse_lanes - 1u) / p.sparse_lanes * 64u : p.count; }

// The lanes a plain or packet launch covers (one per ray, or 64 per piece of a tile): at least the batch's rays.
uint64_t launch_lanes(const TraceParams &p)
{
	if (p.tile_sched != nullptr && p.sched_hdr != nullptr && p.n_slots_max != 0u) {
		const uint64_t lanes = (uint64_t)p.n_slots_max * p.tile_unit * 64u; // (slots past sched_hdr[2] have nothing to do)
		// a width found on the device was scheduled from an earlier cast's: should this batch's grid differ, the kernel ignores the
		// schedule and maps tiles in plain order, a lane per ray (a schedule of the batch's own grid covers that already)
		return p.lane_map == MAP_AUTO && lanes < p.count ? p.count : lanes;
	}
	if (p.lane_map == MAP_TILE8X8) {
		const uint32_t th = 64u >> p.tile_w_log2;
		return (uint64_t)p.tiles_x * ((p.rows + th - 1u) / th) * 64u * pieces_per_tile(p.quarter_all);
	}
	if (p.lane_map == MAP_LINEAR) return linear_lanes(p);
	return p.count * (p.lane_map == MAP_AUTO ? pieces_per_tile(p.quarter_all) : 1u); // (a width found on the device: whole tiles, count / 64 of them)
}

// The asm kernel's scalar-cache prefetch of both children pays where the launch is about one round of waves (packet_asm_kernel.h).
// A scheduled launch covers the slots the list MAY use: what counts is the units, or the one round the fill rule makes of fewer.
bool prefetch_pays(const TraceParams &p, uint64_t lanes)
{
	uint64_t waves = p.tile_sched != nullptr && p.n_slots_max != 0u
			? (p.n_units > kWaveSlots ? p.n_units : (p.n_slots_max < kWaveSlots ? p.n_slots_max : kWaveSlots)) : lanes / kWave;
	if (p.lane_map == MAP_AUTO && waves < (p.count + kWave - 1u) / kWave) waves = (p.count + kWave - 1u) / kWave; // (as in launch_lanes)
	return waves <= kPrefetchMaxWaves;
}

// The persistent walk of p.kernel: 8- or 4-wide where the id asks for it and the layout is resident, else 2-wide.
void persistent_launch(TraceLaunch &l, const TraceParams &p, bool two_level, uint32_t lds_depth, uint32_t blocks)
{
	TraceVariant &v = l.v;
	v.kernel = TraceKernel::LANE_PERSISTENT; v.two_level = two_level;
	if (two_level) v.width = p.kernel == MRT_KERNEL_TWO_LEVEL_PERSISTENT8 && p.nodes8 != nullptr && p.leaf_box != nullptr ? 8 : 2;
	else v.width = p.kernel == MRT_KERNEL_LANE8_PERSISTENT && p.nodes8 != nullptr ? 8 : (p.kernel == MRT_KERNEL_LANE4_PERSISTENT && p.nodes4 != nullptr ? 4 : 2);
	l.blocks = blocks; l.lds = lane_stack_lds(lds_depth);
}

} // namespace

TraceLaunch resolve_trace(const TraceParams &p, bool any_hit, bool count, bool quad_built, uint32_t rows_wg_large)
{
	TraceLaunch l;
	TraceVariant &v = l.v;
	const uint64_t lanes = launch_lanes(p);
	if (lanes == 0) return l;
	if ((lanes + kWg - 1) / kWg > 0x7FFFFFFFull) { l.error = true; return l; }
	const bool rows_id = p.kernel == MRT_KERNEL_PACKET_DUAL || p.kernel == MRT_KERNEL_PACKET_ROWS;
	const bool packet_id = p.kernel == MRT_KERNEL_PACKET_ASM || rows_id || p.kernel == MRT_KERNEL_PACKET_QUAD;
	uint64_t per_block = kWg; // lanes a workgroup covers
	v.any_hit = any_hit; v.count = count;
	if (p.kernel == MRT_KERNEL_TWO_LEVEL_PACKET) { // two-level scene, coherent batch: one wave per packet
		v.kernel = TraceKernel::TWO_LEVEL_PACKET; v.count = false; l.lds = p.extra_lds;
	} else if (p.kernel == MRT_KERNEL_TWO_LEVEL) { // two-level scene: one lane per ray, per-lane LDS stack
		v.kernel = TraceKernel::TWO_LEVEL; v.count = false; l.lds = lane_stack_lds(p.stack_depth);
	} else if (quad_built && p.kernel == MRT_KERNEL_PACKET_QUAD && p.row_array4 != nullptr) {
		// the 128-ray walk over 4-wide node rows: two packets per wave (half the waves)
		v.kernel = TraceKernel::PACKET_QUAD; l.lds = p.extra_lds; per_block = 2u * kWg;
	} else if (rows_id && p.row_array != nullptr) {
		// the walk over the unified row array: one or two packets per wave (two: half the waves, rows_wg / 64 waves of two tiles each
		// per workgroup, culling by where the rays come from unless forced)
		v.kernel = TraceKernel::PACKET_ROWS; l.lds = p.extra_lds;
		v.packets = p.kernel == MRT_KERNEL_PACKET_DUAL ? 2u : 1u;
		if (v.packets == 2u) {
			v.wg = p.rows_wg == 64u ? 64u : rows_wg_large;
			v.cull = p.rows_cull == 1u || (p.rows_cull == 2u && p.in_fmt == IN_GRID);
			l.tile_group = 2u * (v.wg / kWave);
		}
		l.threads = v.wg; per_block = (uint64_t)v.packets * v.wg;
	} else if (packet_id && p.n_nodes < kAsmNodeLimit) {
		v.kernel = TraceKernel::PACKET_ASM; l.lds = p.extra_lds;
		v.prefetch = !count && prefetch_pays(p, lanes);
	} else if (p.kernel == MRT_KERNEL_PACKET || packet_id) { // (scenes whose node offsets pass the asm loop's 32 bits)
		v.kernel = TraceKernel::PACKET;
	} else l.lds = lane_stack_lds(p.stack_depth);
	l.blocks = (uint32_t)((lanes + per_block - 1) / per_block);
	return l;
}

TraceLaunch resolve_persistent(const TraceParams &p, uint32_t lds_depth, uint32_t blocks, bool any_hit, bool count)
{
	TraceLaunch l;
	if (p.count == 0 || blocks == 0) return l;
	const bool tl = p.kernel == MRT_KERNEL_TWO_LEVEL_PERSISTENT || p.kernel == MRT_KERNEL_TWO_LEVEL_PERSISTENT8;
	persistent_launch(l, p, tl, lds_depth, blocks);
	l.v.any_hit = any_hit; l.v.count = count && !tl; // (the counting form exists for flat scenes)
	return l;
}

TraceLaunch resolve_source(const TraceParams &p, uint32_t lds_depth, uint32_t blocks, bool any_hit)
{
	TraceLaunch l;
	if (p.count == 0) return l;
	const bool tl = p.kernel == MRT_KERNEL_TWO_LEVEL || p.kernel == MRT_KERNEL_TWO_LEVEL_PERSISTENT || p.kernel == MRT_KERNEL_TWO_LEVEL_PERSISTENT8;
	l.v.any_hit = any_hit;
	if (blocks != 0) { persistent_launch(l, p, tl, lds_depth, blocks); return l; }
	const uint64_t n = (linear_lanes(p) + kWg - 1) / kWg;
	if (n > 0x7FFFFFFFull) { l.error = true; return l; }
	l.v.kernel = tl ? TraceKernel::TWO_LEVEL : TraceKernel::LANE;
	l.blocks = (uint32_t)n; l.lds = lane_stack_lds(p.stack_depth);
	return l;
}

void format_variant(char *out, size_t n, const TraceVariant &v, const char *family, int src, bool with_mode)
{
	static const char *const names[] = {"lane", "two_level", "two_level_packet", "packet", "packet_asm", "packet_rows", "packet_quad", "lane_persistent"};
	const auto b = [](bool x) { return x ? "true" : "false"; };
	const char *name = names[(uint32_t)v.kernel], *a = b(v.any_hit), *c = b(v.count);
	if (family != nullptr) { // not a symbol of the library: (family, source, mode where the family has two, width, two-level)
		const char *mode = !with_mode ? "" : (v.any_hit ? ", true" : ", false");
		if (v.kernel == TraceKernel::LANE_PERSISTENT) std::snprintf(out, n, "trace_%s_persistent_kernel<%d%s, %d, %s>", family, src, mode, v.width, b(v.two_level));
		else std::snprintf(out, n, "trace_%s_%s_kernel<%d%s>", family, name, src, mode);
		return;
	}
	switch (v.kernel) {
		case TraceKernel::TWO_LEVEL: case TraceKernel::TWO_LEVEL_PACKET: std::snprintf(out, n, "trace_%s_kernel<%s>", name, a); break;
		case TraceKernel::PACKET_ROWS: std::snprintf(out, n, "trace_%s_kernel<%s, %s, %u, %u, %s>", name, a, c, v.packets, v.wg, b(v.cull)); break;
		case TraceKernel::LANE_PERSISTENT: std::snprintf(out, n, "trace_%s_kernel<%s, %d, %s, %s>", name, a, v.width, b(v.two_level), c); break;
		// (the asm kernel's KPF is spelled only where it is not the default, and then COUNT is false)
		default: std::snprintf(out, n, v.prefetch ? "trace_%s_kernel<%s, false, true>" : "trace_%s_kernel<%s, %s>", name, a, c); break;
	}
}

} // namespace mrt
