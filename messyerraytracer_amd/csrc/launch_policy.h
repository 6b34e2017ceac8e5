// launch_policy.h — which kernel a cast gets and how it is launched, as plain host code (no HIP calls, no allocation), in two steps:
//   plan_cast:      the cast -> a CastPlan (kernel id, lane map, sort / detect / schedule, the lane launch); cast.hip launch_planned
//                   executes it and fills a TraceParams per launch;
//   resolve_trace / resolve_persistent / resolve_source: that TraceParams -> a TraceLaunch, the one instantiation (TraceVariant) with
//                   its grid, workgroup, LDS and tile_group.  kernels.hip looks the instantiation up from the variant, launches it
//                   with that geometry and prints the label of mrt_last_kernel_variant from the same value (format_variant).
// csrc/host/launch_policy_test.cpp pins both steps on the CPU: every plan with the label and the geometry it resolves to.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/mrt_hip.h"
#include "mrt_internal.h"

namespace mrt {

// Grid casts of 2^19 .. 2^24 rays are scheduled (schedule.hip): see the comment there.
#ifndef MRT_SCHEDULE_MAX_LOG2
#define MRT_SCHEDULE_MAX_LOG2 24
#endif
constexpr uint64_t kScheduleMaxRays = 1ull << MRT_SCHEDULE_MAX_LOG2;
constexpr uint64_t kQuarterMinRays = 64, kQuarterMaxTiles = 3600, kSixteenthMaxTiles = 512; // small grids in quarter / sixteenth tiles
constexpr uint64_t kQuarterAllRays = 2048ull * 64ull; // up to here four quarters per tile still fit one round of waves: no schedule needed
constexpr int kTuneFrames = 4; // frames per candidate of the grid kernel tuner (tune_grid_kernel): the last two are timed

// Settings read from the environment once, when the context is created (mrt_create).
struct Knobs {
	// From 2^17 rays (2 048 tiles: below, all tiles go in quarter tiles anyway, quarter rule).  With the order alone 640x360
	// measured 7 % slower scheduled than not; with the most expensive tiles in quarter tiles until the chip is full
	// (schedule_plan_kernel) it is 20 % faster.  MRT_SCHEDULE_MIN_LOG2 moves the bound (the tests schedule smaller grids)
	uint64_t schedule_min_rays = 1ull << 17;
	// the grid tuner: from 2^19 rays on the 128-ray walk is a candidate (below, the 64-ray kernel won every measurement); a test that
	// moves the schedule's bound moves this one with it
	uint64_t tune_min_rays = 1ull << 19;
	uint32_t split_pct = 1;  // MRT_SCHED_SPLIT_PCT: the rank, in percent, above which a unit goes in pieces (schedule_plan_kernel)
	bool dump = false;       // MRT_SCHED_DUMP: print what every schedule was made of (tools/bench_resolutions.py)
	// MRT_POISON_OUTPUT (tests): every cast first fills its output range with kPoisonByte on the context's stream, so that a record
	// no launch wrote shows up as one (0xA5: t < 0, prim_id and token out of range, a bool neither 0 nor 1); off, nothing is queued
	bool poison = false;
};
constexpr uint8_t kPoisonByte = 0xA5;

// What the cast path needs to know about the scene (and the device).
struct SceneFacts {
	bool two_level = false, rows = false, rows4 = false, nodes4 = false, nodes8 = false; // which layouts are resident
	uint32_t n_nodes = 0, depth = 0, stack4 = 0, stack8 = 0; // stack entries one ray can need in the 2-, 4- and 8-wide walks
	uint32_t cu_count = 256;
};

// ENTRY_CHUNK: a chunk of cast_host_pipelined.  ENTRY_SHADOW / ENTRY_GRID_SHADOW: mrt_cast_shadows / mrt_cast_grid_shadows, count =
// pixels * lights (shadow rays made in the kernel from hit records: an unsorted, non-coherent any-hit batch).  ENTRY_REFLECTION /
// ENTRY_GRID_REFLECTION: mrt_cast_reflections / mrt_cast_grid_reflections, count = records (mirror rays made in the kernel: an
// unsorted, non-coherent closest-hit batch).  ENTRY_HEMISPHERE / ENTRY_GRID_HEMISPHERE: mrt_cast_hemisphere / mrt_cast_grid_hemisphere,
// count = pixels * samples (cosine-weighted hemisphere rays made in the kernel: an unsorted, non-coherent batch in either mode).
// ENTRY_BOUNCE / ENTRY_GRID_BOUNCE: mrt_cast_bounce / mrt_cast_grid_bounce, count = records (the path tracer's bounce rays made in the
// kernel: an unsorted, non-coherent closest-hit batch).  ENTRY_GBUFFER_REFLECTION: mrt_cast_gbuffer_reflections, count = pixels of the
// frame (mirror rays made in the kernel from a rasteriser's depth and normal buffers: the plan of a reflection cast of as many rays).
// ENTRY_SELECTED_SHADOW / ENTRY_GRID_SELECTED_SHADOW: mrt_cast_selected_shadows / mrt_cast_grid_selected_shadows, count = records (one
// shadow ray per record to the light it draws: an unsorted any-hit batch, less coherent than a shadow cast's since neighbours differ in light)
// ENTRY_EMITTER_SHADOW / ENTRY_GRID_EMITTER_SHADOW: mrt_cast_emitter_shadows / mrt_cast_grid_emitter_shadows, count = records (one shadow
// ray per record to a sampled point of a sampled emissive triangle: the same kind of batch, neighbours differing in emitter and point)
enum Entry : uint32_t { ENTRY_CAST, ENTRY_SUBMIT, ENTRY_CHUNK, ENTRY_GRID, ENTRY_TILED, ENTRY_SHADOW, ENTRY_GRID_SHADOW,
	ENTRY_REFLECTION, ENTRY_GRID_REFLECTION, ENTRY_HEMISPHERE, ENTRY_GRID_HEMISPHERE, ENTRY_BOUNCE, ENTRY_GRID_BOUNCE,
	ENTRY_GBUFFER_REFLECTION, ENTRY_SELECTED_SHADOW, ENTRY_GRID_SELECTED_SHADOW, ENTRY_EMITTER_SHADOW, ENTRY_GRID_EMITTER_SHADOW };
inline bool ray_entry(Entry e) { return e <= ENTRY_CHUNK; } // rays from an array, through enqueue_cast
// rays made in the kernel, from hit records or (ENTRY_GBUFFER_REFLECTION) from a G-buffer
inline bool record_cast_entry(Entry e) { return e >= ENTRY_SHADOW && e <= ENTRY_GRID_EMITTER_SHADOW; }

struct CastRequest {
	Entry entry = ENTRY_CAST;
	uint64_t count = 0;
	uint32_t flags = 0;
	int mode = MRT_MODE_NEAREST;
	uint32_t grid_w = 0, grid_h = 0, y0 = 0, rows = 0; // grid / tiled casts
};

// What detect_grid_kernel found for the previous cast ({row width, rows, tiles_x, verdict}), and for how many rays.
struct PrevDetect {
	bool pending = false;  // the words may still be written (a planner that cannot tell: no schedule)
	uint64_t count = 0;    // rays of the last cast that ran detect_grid_kernel (0: none)
	uint32_t word[4] = {0, 0, 0, 0};
};

// The PrevDetect a cast is planned from, as a consistent pair.  detect_grid_kernel writes its words to host-mapped memory when it
// RUNS, but a cast is planned when it is QUEUED: ASYNC casts, pipeline chunks and a submit queue behind others, and a count noted at
// queue time next to words read at plan time may belong to two different casts (the count of the cast just queued, the width of
// one before it: a schedule of the wrong grid, whose launch covers too few rays).  So every cast from an array notes, as it is
// queued, whether it runs a detect and for how many rays (queued), and only after the host has waited for the stream -- when the
// words are those of the last detect queued -- are count and words taken together (waited).  Casts queued since then are planned
// from the pair of the last wait (prev).  Plain host code: cast.hip calls it, launch_policy_test.cpp runs it through sequences.
struct DetectMemo {
	uint64_t queued_count = 0;   // rays of the last cast queued from an array if it ran detect_grid_kernel (0: it did not)
	bool queued_since_wait = false;
	PrevDetect seen;             // taken at the last wait after a queued cast
	void queued(bool detect, uint64_t count) { queued_count = detect ? count : 0u; queued_since_wait = true; }
	void waited(const volatile uint32_t *words); // the host has waited for the stream: words = what the last queued detect wrote
	const PrevDetect &prev() const { return seen; }
};

// How a mid-size grid is cast is MEASURED per grid (tune_grid_kernel): four frames with the 64-ray kernel, four with the 128-ray
// walk and its most expensive units launched in pieces, four with the 128-ray walk and every unit whole; from frame 12 on the
// fastest of the three, each judged by the faster of its last two frames.  What wins flips with the number of rounds a grid
// makes on the chip (C3 scene: 1280x720 the 64-ray kernel, 1280x960 the 128-ray walk whole, 1920x1080 the 128-ray walk in pieces).
struct GridTune { uint32_t grid_w = 0, grid_h = 0, y0 = 0, rows = 0; int mode = -1; int phase = 0; float t_asm = 0.0f, t_dual = 0.0f, t_whole = 0.0f; bool armed = false, no_pieces = false; };
// What has been learnt about a grid (its tile schedule, how it is cast fastest) is kept per grid AND cast mode, for the last few
// of them: a renderer that casts two views, or closest-hit and any-hit rays of one view, or the row-block chunks of a sharded
// frame, in turn, keeps every one's state (with one state each change of grid threw the other's away, and cost a stream
// synchronisation and an upload to start over).  select_grid_state() picks the entry of a cast; the least recently used one goes.
// The context keeps the tile schedule of entry k in its own array at k.
struct GridKey { uint32_t w = 0, h = 0, y0 = 0, rows = 0; int mode = -1; };
struct GridStates {
	static constexpr int kCount = 8;
	struct Entry { GridKey key; GridTune tune; uint64_t stamp = 0; } e[kCount];
	uint64_t clock = 0;
	int cur = 0;
	GridTune &tune() { return e[cur].tune; }
};
int select_grid_state(GridStates &g, const GridKey &k); // returns (and makes current) the entry of k
void tune_record(GridTune &t, float trace_ms);          // after a blocking cast the tuner armed: note its time, next phase

// One launch of the lane kernels (launch_lane): plain, one fixed ray per lane, or persistent, resident waves pulling rays from
// a counter with a short LDS stack that spills to HBM.
struct LaneLaunch {
	bool persistent = false;
	uint32_t kernel = MRT_KERNEL_LANE;
	uint32_t sparse_lanes = 0;              // plain: rays per wave (0 = 64)
	uint32_t lds_depth = 0, blocks = 0;     // persistent: LDS stack entries per lane, workgroups
	uint32_t spill = 0;                     // persistent: stack entries per lane past lds_depth (in HBM)
	uint32_t refill = 0, leaf_wait = 0;
	bool count = false;                     // the counting variant
};

struct CastPlan {
	bool sort = false, detect = false;
	uint32_t kernel = MRT_KERNEL_LANE, lane_map = MAP_LINEAR, quarter_all = 0;
	enum Launch : uint32_t { PLAIN, LANE, DUAL } launch = PLAIN; // DUAL: the packet kernel, then `lane` queued behind it
	bool count = false;                     // PLAIN / DUAL packet launch: the counting variant
	LaneLaunch lane;                        // LANE, DUAL
	bool scheduled = false;                 // a frame-coherent tile schedule (schedule_grid / schedule_sort) ...
	uint32_t grid_w = 0, grid_h = 0, y0 = 0, rows = 0, tiles_x = 0; // ... of this grid (mrt_cast(COHERENT): the detected one)
	bool pieces = false;                    // ... with its most expensive units in pieces
	bool wait_sorts = false;                // ... launched in a measured order (the tuner times this frame)
	bool arms_tuner = false;                // the cast's timing goes to tune_record
	uint32_t launches = 0;                  // mrt_stats.last_kernel_launches (0: left as it is)
};

// Launch slots of a tile schedule of n_units units (schedule_grid): with pieces, room for half as many again or for what fills one
// round of waves (schedule_plan_kernel).  A launch from the schedule covers slots * unit * 64 lanes: at least the batch's rays.
inline uint32_t schedule_slots(uint32_t n_units, bool pieces)
{
	return pieces ? (n_units + n_units / 2u > kWaveSlots ? n_units + n_units / 2u : kWaveSlots) : n_units;
}

// ---- plan -> variant -> launch -> label ---------------------------------------------------------------------------------------
// One instantiation of the trace kernels.  The template arguments a kernel does not have stay at their defaults here.
enum class TraceKernel : uint32_t { LANE, TWO_LEVEL, TWO_LEVEL_PACKET, PACKET, PACKET_ASM, PACKET_ROWS, PACKET_QUAD, LANE_PERSISTENT };
struct TraceVariant {
	TraceKernel kernel = TraceKernel::LANE;
	bool any_hit = false, count = false;
	uint32_t packets = 1, wg = 256; bool cull = false; // PACKET_ROWS: packets per wave, threads per workgroup, the frustum cull
	bool prefetch = false;                             // PACKET_ASM: the scalar-cache prefetch of both children (never with count)
	int width = 2; bool two_level = false;             // LANE_PERSISTENT: children per node step, the two-level walk
};
// A variant with its launch.  blocks == 0: nothing to launch (no rays; the label stays as it was); error: more than 0x7FFFFFFF
// workgroups of 256 lanes (hipErrorInvalidValue).
struct TraceLaunch {
	TraceVariant v;
	bool error = false;
	uint32_t blocks = 0, threads = 256;  // workgroups, threads per workgroup
	size_t lds = 0;                      // dynamic LDS bytes per workgroup
	uint32_t tile_group = 4;             // plain and packet launches: the TraceParams::tile_group the kernel must see (tiles per workgroup)
	uint32_t packets_per_wave() const { return v.kernel == TraceKernel::PACKET_QUAD ? 2u : (v.kernel == TraceKernel::PACKET_ROWS ? v.packets : 1u); }
};
constexpr uint32_t kPrefetchMaxWaves = kWaveSlots + kWaveSlots / 4u; // the asm kernel prefetches up to 1.25 rounds of the device's wave slots

// A plain or packet launch of a primary cast (launch_trace): p as launch_planned filled it.  Fallbacks, in this order: a two-level id
// takes its own kernel; PACKET_QUAD without row_array4 (or a build without the kernel: quad_built) and PACKET_DUAL / PACKET_ROWS
// without row_array take the asm kernel; any of the four packet ids with n_nodes >= kAsmNodeLimit takes the C++ packet kernel.
// rows_wg_large: threads per workgroup of the 128-ray walk where p.rows_wg != 64 (the build's MRT_ROWS_WG_LARGE).
TraceLaunch resolve_trace(const TraceParams &p, bool any_hit, bool count, bool quad_built, uint32_t rows_wg_large = 256);
// A persistent launch of a primary cast (launch_trace_persistent): `blocks` resident workgroups with lds_depth stack entries per lane.
TraceLaunch resolve_persistent(const TraceParams &p, uint32_t lds_depth, uint32_t blocks, bool any_hit, bool count);
// A record-driven cast (launch_source): persistent as above if blocks != 0, else the plain lane kernel with p.sparse_lanes; LANE,
// TWO_LEVEL or LANE_PERSISTENT.  There is no counting variant.
TraceLaunch resolve_source(const TraceParams &p, uint32_t lds_depth, uint32_t blocks, bool any_hit);
// The name mrt_last_kernel_variant reports.  family == nullptr: the kernel's symbol as rocprofv3 prints it,
// "trace_packet_rows_kernel<false, false, 2, 64, true>".  A record-driven cast: its family, source (a RaySrc) and, where the family
// has two modes (with_mode), the mode: "trace_shadow_lane_kernel<3>", "trace_hemisphere_persistent_kernel<9, true, 8, false>".
void format_variant(char *out, size_t n, const TraceVariant &v, const char *family = nullptr, int src = 0, bool with_mode = false);

uint32_t tile_w_log2(const mrt_options &o);
// Plans a cast.  May select (and reset) the grid state of the cast in `gs` (never for a shadow, reflection, hemisphere or bounce entry: those
// read neither `prev` nor `gs`).
CastPlan plan_cast(const mrt_options &o, const SceneFacts &s, const CastRequest &r, const PrevDetect &prev, const Knobs &k, GridStates &gs);

} // namespace mrt
