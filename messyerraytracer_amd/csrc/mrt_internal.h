// mrt_internal.h — shared between the host-side scene preparation and the HIP
// kernels of libmrt_hip.so.  Not part of the C-ABI.
#pragma once
#include <cstdint>
#include "../../include/mrt_hip.h"

static_assert(sizeof(mrt_ray32) == 32, "GPURayPacked must be 32 bytes (src/api/gpu_types.h:70)");
static_assert(sizeof(mrt_hit32) == 32, "GPUIntersectionPacked must be 32 bytes (src/api/gpu_types.h:93)");
static_assert(sizeof(mrt_tri64) == 64, "GPUTrianglePacked must be 64 bytes (src/api/gpu_types.h:51)");
static_assert(sizeof(mrt_bvh_node32) == 32, "GPUBVHNodePacked must be 32 bytes (src/api/gpu_types.h:127)");
static_assert(sizeof(mrt_bvh_node_wide64) == 64, "GPUBVHNodeWide must be 64 bytes (src/gpu/gpu_structs.h:47)");
static_assert(sizeof(mrt_host_ray60) == 60, "Ray must be 60 bytes (src/core/ray.h:25-51, precision=single)");
static_assert(sizeof(mrt_host_hit44) == 44, "Intersection must be 44 bytes (src/core/intersection.h:16-40)");
static_assert(sizeof(mrt_host_tri80) == 80, "Triangle must be 80 bytes (src/core/triangle.h:22-39)");
static_assert(sizeof(mrt_light) == 32, "mrt_light must be 32 bytes");

namespace mrt {

// ---- device scene layout (HBM) ------------------------------------------------
// Node: the reference's 64-byte dual-AABB node with the child encoding folded
// into one 32-bit reference per child:
//   ref <  0x7FFFFFFF : index of a wide node
//   ref == 0x7FFFFFFF : sentinel (bottom of every traversal stack)
//   ref >= 0x80000000 : leaf; low 31 bits = first slot in the leaf-ordered
//                       triangle arrays; the leaf's last triangle carries
//                       kLastInLeaf in TriHot::flags.
struct alignas(16) DevNode {
	float lmin[3]; uint32_t left_ref;
	float lmax[3]; uint32_t right_ref;
	float rmin[3]; uint32_t left_count;   // counts kept for validation / stats only
	float rmax[3]; uint32_t right_count;
};
static_assert(sizeof(DevNode) == 64, "DevNode must be 64 bytes");

// Triangle, split hot/cold: traversal reads 48 B per test, the 16-byte normal
// row is read once per ray for the winning triangle.
struct alignas(16) TriHot {
	float v0[3]; uint32_t id;
	float e1[3]; uint32_t layers;
	float e2[3]; uint32_t flags;
};
static_assert(sizeof(TriHot) == 48, "TriHot must be 48 bytes");
struct alignas(16) TriCold { float normal[3]; uint32_t pad; };

// 4-wide node for the persistent lane kernel: two levels of the BVH2 collapsed into one 128-byte
// line, halving the chain of dependent fetches a ray walks.
// Built on the host from the same binned-SAH BVH2 (greedy: keep opening the child with
// the largest surface area until there are 4).  Child refs use the DevNode encoding with
// wide4 indices; an unused slot has ref == kSentinel.
struct alignas(16) Dev4Node {
	float box[4][6];      // child c: min.xyz, max.xyz
	uint32_t ref[4];
	uint32_t n_children, pad[3];
};
static_assert(sizeof(Dev4Node) == 128, "Dev4Node must be 128 bytes");

// 8-wide compressed node (Ylitie, Karras, Laine 2017, the layout idea of the
// reference's cwbvh_traverse.comp.glsl, re-cut for one 128-byte cache line and explicit child refs):
// child boxes are 8-bit coordinates on a per-node grid, lo = fma(q, 2^(exp-127), org) per axis.  The
// builder rounds outwards and checks the DECODED value in float, so a decoded box contains the exact
// one and the slab test on it (same formula as for exact boxes, monotone in the box coordinate)
// passes whenever the test on the exact box does: the walk visits a superset of what the 2-wide walk
// visits, and every triangle is still tested with the exact arithmetic.  A hit is accepted only if
// the ray also passes the slab test on the leaf's EXACT box (leaf_box[], 32 bytes per leaf, read on
// that rare path only): boxes nest and the slab arithmetic is monotone, so passing the leaf's box is
// passing every ancestor's, and the 8-wide walk reports exactly what the 2-wide walk reports -- also
// for rays that lie in a face plane of a box, where a looser box would let an edge hit through.
struct alignas(16) Dev8Node {
	float org[3];
	uint8_t exp[3];       // float exponent byte of the grid step per axis
	uint8_t n_children;
	uint8_t qlo[3][8];    // [axis][child]
	uint8_t qhi[3][8];
	uint32_t ref[8];      // DevNode encoding with wide8 indices; unused slots kSentinel
	uint32_t pad[8];
};
static_assert(sizeof(Dev8Node) == 128, "Dev8Node must be 128 bytes");

// ---- the context's counter block (unsigned long long words; mrt_ctx::d_counters) ----
// [0, kNumCounters): visit counters of the counting kernel variants (mrt_options.count_visits)
constexpr int kCntRays = 0, kCntTris = 1, kCntNodes = 2, kCntHits = 3, kCntMaxStack = 4, kCntDeadPops = 5;
constexpr int kCntWaveNodeFetch = 6; // node fetches as the hardware sees them: one per wave step (packet kernels), one per lane step
                                     // = one divergent 64-/128-byte line (lane kernels)
constexpr int kCntWaveTriFetch = 7;  // triangle rows fetched: one per wave step (packet kernels), one per lane test (lane kernels)
constexpr int kCntLeafBoxChecks = 8; // 8-wide kernel: exact leaf boxes read for candidate hits
constexpr int kCntFetchWaitCycles = 9, kCntWaveCycles = 10, kCntWaves = 11; // trace_packet_rows_kernel<.., 1>: s_memtime clock
constexpr int kNumCounters = 16;
constexpr int kAutoGridOff = kNumCounters;         // 8 words: what detect_grid_kernel found (4 x u32 used)
constexpr int kDetectScratchOff = kAutoGridOff + 8; // 1026 words: jump masks + ticket + wide-neighbour count
constexpr int kNextRayOff = kDetectScratchOff + 1026; // 128 words: 8 ray counters of the persistent kernels, 16 words apart
constexpr int kCounterWords = kNextRayOff + 128;

// wave slots of the device (256 CUs x 4 SIMDs x 8 waves): what a launch's work is spread over in one round
constexpr uint32_t kWaveSlots = 8192u;

constexpr uint32_t kSentinel = 0x7FFFFFFFu;
constexpr uint32_t kLeafBit = 0x80000000u;
constexpr uint32_t kLastInLeaf = 1u;

enum InFmt : uint32_t { IN_RAY32 = 0, IN_HOST60 = 1, IN_GRID = 2 };
// OUT_TOKEN4: one u32 per ray = leaf-order slot of the winning triangle (0xFFFFFFFF = miss); the
// full record is rebuilt from (ray, slot) by expand_tokens_kernel, bit for bit
// OUT_TOKEN8 (two-level scenes): two u32 per ray = {slot of the winning triangle in its mesh's arrays (0xFFFFFFFF =
// miss), DevInstance row of the instance it was hit in}: the record is a function of (ray, triangle, instance)
enum OutFmt : uint32_t { OUT_HIT32 = 0, OUT_HOST44 = 1, OUT_BOOL8 = 2, OUT_TOKEN4 = 3, OUT_TOKEN8 = 4 };
enum LaneMap : uint32_t { MAP_LINEAR = 0, MAP_TILE8X8 = 1, MAP_AUTO = 2 };

struct DevInstance;
struct TraceParams {
	const DevNode *nodes;
	const Dev4Node *nodes4;    // 4-wide layout of the persistent lane kernel (may be null)
	const Dev8Node *nodes8;    // 8-wide compressed layout (may be null)
	const float *leaf_box;     // with nodes8: exact box {min xyz, -, max xyz, -} of the leaf that starts at a slot
	const DevInstance *instances; // two-level scenes (kernel == MRT_KERNEL_TWO_LEVEL)
	const TriHot *tri_hot;
	const TriCold *tri_cold;
	const void *row_array;     // nodes + triangles as one array of 64-byte rows (packet_rows_kernel.h; may be null)
	const void *row_array4;    // 4-wide node rows (128 bytes) + triangle rows, in 64-byte units (packet_quad_kernel.h; may be null)
	uint32_t rows_wg;          // trace_packet_rows_kernel<.., 2>: threads per workgroup, 64 or 256
	uint32_t rows_cull;        // ... 1: packet-level frustum culling in the 128-ray walk
	float scene_abs_max;       // largest |coordinate| of the scene's bounds (error bound of the culling test)
	uint32_t tri_unit_base4;   // row_array4: the unit of triangle slot 0 (= 2 * number of 4-wide nodes)
	const void *rays;          // IN_RAY32 / IN_HOST60 (device)
	void *hits;                // device
	const uint32_t *perm;      // optional: lane g traces ray perm[g], writes hits[perm[g]]
	unsigned long long *counters; // COUNT variants: the kCnt* words above
	const uint32_t *auto_grid; // MAP_AUTO: {row width (0 = none), rows, tiles_x, incoherent} written by detect_grid_kernel
	const uint32_t *skip_flag; // optional: the whole launch returns at once when *skip_flag == skip_when
	uint32_t skip_when;        // (a "coherent" batch that is not: the packet launch yields to the lane launch)
	uint64_t count;            // number of rays
	uint32_t query_mask;
	uint32_t in_fmt, out_fmt, lane_map;
	uint32_t grid_w, grid_h, y0, rows; // IN_GRID / MAP_TILE8X8: rows [y0, y0+rows) of a grid_w x grid_h grid
	uint32_t tiles_x;          // ceil(grid_w / tile width)
	uint32_t tile_w_log2;      // lane tile: 2^k wide, 64 / 2^k high
	uint32_t tile_order;       // 0: tiles row-major, 1: Z-order inside 16x16-tile super-tiles, 2: 32x32, 3: column strips per XCD
	uint32_t tile_group;       // tile_order 3: consecutive tiles per workgroup (set by launch_trace)
	// Frame-coherent tile schedule of grid casts (schedule.hip; mrt_ctx::TileSchedule): launch slot u runs schedule unit tile_sched[u]
	// (a unit = tile_unit consecutive tiles: 1, or 2 for the 128-ray walk) and leaves the shader cycles it took in
	// tile_cost[unit]; the next cast of the same grid launches the units longest first.  Both may be null.
	// An entry of tile_sched: bits 0-27 an id, bits 28-31 what the slot's wave works on -- 0: schedule unit `id`; 1: the one tile
	// `id` (in the wave's first group; a second group stays empty); 2 + q: quarter q of tile `id`, 4x4 pixels in lanes 0..15.
	// The most expensive units of the last measured frame are launched in such pieces (schedule.hip schedule_plan_kernel): a frame of a
	// million rays ends with its longest walk, and the longest one is 2-3 x the 99th percentile.  sched_hdr[2] = slots in use
	// (the launch covers n_slots_max); a piece parks its start time in tile_cost[n_units + slot] and ADDS its share to its unit.
	const uint32_t *tile_sched;
	uint32_t *tile_cost;
	uint32_t tile_unit, n_units;
	const uint32_t *sched_hdr;
	uint32_t n_slots_max;
	// Small grids (launch_policy.cpp quarter_rule): EVERY tile is launched as its four quarter tiles (launch slot s = quarter s & 3 of
	// tile s >> 2, 16 rays in lanes 0..15) -- a grid of fewer tiles than the device has wave slots lasts as long as its longest
	// walk, and a quarter tile's walk is about half as long as its tile's.
	uint32_t quarter_all;
	uint32_t sparse_lanes;     // linear lane map of the lane kernel: rays per wave, in lanes 0 .. sparse_lanes - 1 (0 = 64): a small batch on more, emptier waves (launch_policy.cpp lane_launch)
	uint32_t kernel;           // MRT_KERNEL_LANE / MRT_KERNEL_PACKET
	uint32_t stack_depth;      // LDS stack entries per lane
	uint32_t xcd_swizzle;      // 1: remap blockIdx so each XCD owns a contiguous band
	uint32_t n_tris;           // rows in tri_hot / tri_cold (token validation)
	uint32_t n_instances;      // rows in instances (two-level scenes; token validation)
	uint32_t n_nodes;          // rows in nodes (the hand-written node loop addresses them with a 32-bit byte offset)
	uint32_t count_mode;       // COUNT variants: mrt_options.count_visits (1: visit counters, 2: only the sampled clock of the rows kernel)
	uint32_t extra_lds;        // experiments: dynamic LDS bytes added per workgroup of the packet kernels (occupancy sweeps)
	uint32_t rows_fast;        // trace_packet_rows_kernel<.., 2>: lane_map.h fast_launch of this launch (set by launch_trace)
	mrt_camera cam;
};

// ---- shadow rays (shadow_kernel.h): made in the trace kernel from the hit records of a cast -----------------------------
// Entry g of a shadow cast is the pair (light g / pixels, pixel g % pixels); TraceParams::count = pixels * lights, hits = the
// lit mask (one byte per entry), rays = the primary rays (SRC_SHADOW_RAY32).  The ray source is a template parameter of the
// kernels (SRC_CAST: the rays of an ordinary cast, the instantiations that existed before); source_common.h says what a family is.
enum RaySrc : int { SRC_CAST = 0, SRC_SHADOW_RAY32 = 1, SRC_SHADOW_HOST44 = 2, SRC_SHADOW_GRID = 3,
	SRC_REFLECT_RAY32 = 4, SRC_REFLECT_HOST = 5, SRC_REFLECT_GRID = 6,
	SRC_HEMI_RAY32 = 7, SRC_HEMI_HOST = 8, SRC_HEMI_GRID = 9,
	SRC_BOUNCE_RAY32 = 10, SRC_BOUNCE_HOST = 11, SRC_BOUNCE_GRID = 12,
	SRC_GBUFFER = 13,
	SRC_SELSHADOW_RAY32 = 14, SRC_SELSHADOW_HOST44 = 15, SRC_SELSHADOW_GRID = 16,
	SRC_EMITSHADOW_RAY32 = 17, SRC_EMITSHADOW_HOST44 = 18, SRC_EMITSHADOW_GRID = 19 };
constexpr bool shadow_source(int src) { return src >= SRC_SHADOW_RAY32 && src <= SRC_SHADOW_GRID; }
constexpr bool reflection_source(int src) { return src >= SRC_REFLECT_RAY32 && src <= SRC_REFLECT_GRID; }
constexpr bool hemisphere_source(int src) { return src >= SRC_HEMI_RAY32 && src <= SRC_HEMI_GRID; }
constexpr bool bounce_source(int src) { return src >= SRC_BOUNCE_RAY32 && src <= SRC_BOUNCE_GRID; }
constexpr bool gbuffer_source(int src) { return src == SRC_GBUFFER; }
constexpr bool selected_shadow_source(int src) { return src >= SRC_SELSHADOW_RAY32 && src <= SRC_SELSHADOW_GRID; }
constexpr bool emitter_shadow_source(int src) { return src >= SRC_EMITSHADOW_RAY32 && src <= SRC_EMITSHADOW_GRID; }
// the result of an entry is one byte (1 = no occluder, or no ray): every shadow cast, selected, to an emitter or neither, and a hemisphere cast in any-hit mode
constexpr bool lit_output(int src, bool any_hit)
{
	return shadow_source(src) || selected_shadow_source(src) || emitter_shadow_source(src) || (hemisphere_source(src) && any_hit);
}
enum ShadowKind : uint32_t { SHADOW_OFF = 0, SHADOW_DIRECTIONAL = 1, SHADOW_POINT = 2 }; // OFF: cast_shadows == 0 (lit)
struct ShadowLight { uint32_t kind; float v[3]; }; // DIRECTIONAL: direction towards the light; POINT (point and spot): position
struct ShadowParams {
	const void *records;       // mrt_hit32 (SRC_SHADOW_RAY32, SRC_SHADOW_GRID) or mrt_host_hit44 (SRC_SHADOW_HOST44), `pixels` of them
	uint64_t pixels;
	ShadowLight light[MRT_MAX_LIGHTS];
};

// ---- mirror-reflection rays (reflection_kernel.h): one closest-hit ray per hit record of a cast --------------------------------
// Entry i of a reflection cast is record i; TraceParams::count = records, hits = the output records (out_fmt OUT_HIT32 or OUT_HOST44),
// rays = the incoming rays (SRC_REFLECT_RAY32: mrt_ray32, SRC_REFLECT_HOST: mrt_host_ray60; SRC_REFLECT_GRID regenerates them).
struct ReflectParams {
	const void *records;       // mrt_hit32 (SRC_REFLECT_RAY32, SRC_REFLECT_GRID) or mrt_host_hit44 (SRC_REFLECT_HOST)
	const uint8_t *select;     // optional: 0 = no ray for this record
	void *out_rays;            // optional: the rays made, mrt_ray32 (or mrt_host_ray60 for SRC_REFLECT_HOST)
	float max_distance;        // t_max of every ray
};

// ---- cosine-weighted hemisphere rays (hemisphere_kernel.h): n_samples rays per hit record of a cast ----------------------------
// Entry g of a hemisphere cast is the pair (sample g / pixels, pixel g % pixels); TraceParams::count = pixels * n_samples, hits = one
// byte per entry (any-hit) or one record per entry (closest-hit), rays = the incoming rays as for reflections.  The generator's state
// before a sample's first draw is jump[sample].a * state0 + jump[sample].c (hemisphere_jumps, source_cast.h).
constexpr uint32_t kPcgMul = 747796405u, kPcgInc = 2891336453u; // the reference's PCG32 (path_state.h): state' = state * mul + inc
struct HemiJump { uint32_t a, c; };
// (A, C) with: PCG32 state before draw k = A * state0 + C, modulo 2^32, by squaring: the step (a, c) applied twice is (a * a, a * c + c).
// Once per call on the host, so that the kernel has no loop over draws.
inline HemiJump pcg_jump(uint32_t first_draw)
{
	uint32_t A = 1u, C = 0u, a = kPcgMul, c = kPcgInc;
	for (uint32_t k = first_draw; k != 0u; k >>= 1) {
		if (k & 1u) { A = a * A; C = a * C + c; }
		c = a * c + c; a = a * a;
	}
	return HemiJump{A, C};
}
struct HemiParams {
	const void *records;       // mrt_hit32 (SRC_HEMI_RAY32, SRC_HEMI_GRID) or mrt_host_hit44 (SRC_HEMI_HOST)
	const uint8_t *select;     // optional: 0 = no ray for this pixel
	void *out_rays;            // optional (closest-hit only): the rays made, mrt_ray32 (or mrt_host_ray60 for SRC_HEMI_HOST)
	uint64_t pixels;
	uint32_t seed_add;         // frame * 6529 + 7 (+ y0 * grid_w * 1009 for a row band): seed = pixel * 1009 + seed_add
	float t_max;               // t_max of every ray
	HemiJump jump[MRT_MAX_HEMISPHERE_SAMPLES];
};

// ---- the path tracer's bounce (bounce_kernel.h): one closest-hit ray per hit record, lobe chosen and sampled in the kernel ---------
// Entry i of a bounce cast is record i; TraceParams::count = records, hits = the output records, rays = the incoming rays as for
// reflections.  The generator's state before the lobe draw is jump.a * state0 + jump.c (pcg_jump).
struct BounceParams {
	const void *records;       // mrt_hit32 (SRC_BOUNCE_RAY32, SRC_BOUNCE_GRID) or mrt_host_hit44 (SRC_BOUNCE_HOST)
	const uint8_t *select;     // optional: 0 = no ray for this record
	const float *surface;      // optional: {metallic, roughness} per record; null: the two constants below for every record
	void *out_rays;            // optional: the rays made, mrt_ray32 (or mrt_host_ray60 for SRC_BOUNCE_HOST)
	uint8_t *out_lobe;         // optional: MRT_LOBE_* per record
	uint32_t seed_add;         // frame * 6529 + 7 (+ y0 * grid_w * 1009 for a row band): seed = record * 1009 + seed_add
	float t_max;               // t_max of every ray
	float metallic, roughness; // as the descriptor gave them (clamped in the kernel like a record's pair)
	HemiJump jump;             // (A, C) of draw first_draw
};

// ---- one shadow ray per record, to the light the record draws (selected_shadow_kernel.h; source_cast.h fills this) ------------------
// Entry i of a selected-shadow cast is record i; TraceParams::count = records, hits = the lit mask (one byte per record), rays = the
// primary rays (SRC_SELSHADOW_RAY32).  The generator's state before the selecting draw is jump.a * state0 + jump.c, as for a bounce.
struct SelectShadowParams {
	const void *records;       // mrt_hit32 (SRC_SELSHADOW_RAY32, SRC_SELSHADOW_GRID) or mrt_host_hit44 (SRC_SELSHADOW_HOST44)
	const uint8_t *select;     // optional: 0 = the record selects no light
	uint8_t *out_light;        // the light selected per record, or MRT_LIGHT_NONE
	uint32_t seed_add;         // frame * 6529 + 7 (+ y0 * grid_w * 1009 for a row band): seed = record * 1009 + seed_add
	HemiJump jump;             // (A, C) of draw select_draw
	uint32_t n_lights;         // >= 1
	ShadowLight light[MRT_MAX_LIGHTS];
};

// ---- one shadow ray per record, to a sampled point of a sampled emissive triangle (emitter_shadow_kernel.h; emitters.h fills this) ------
// The resident emitter table (emitters.hip): n rows of 64 bytes {v0, q | edge1, prim id | edge2, area | Le, material} and the inclusive
// uint32 CDF of q, both in device memory; total = cdf[n - 1] (0 with n == 0).
struct EmitterTable {
	const void *rows;
	const uint32_t *cdf;
	uint32_t n, total;
};
// Entry i of an emitter-shadow cast is record i; TraceParams::count = records, hits = the lit mask (one byte per record), rays = the
// incoming rays as for a bounce (the normal is faced).  The generator's state before the selecting draw is jump.a * state0 + jump.c;
// the two floats of the point are the next two draws.
struct EmitterShadowParams {
	const void *records;       // mrt_hit32 (SRC_EMITSHADOW_RAY32, SRC_EMITSHADOW_GRID) or mrt_host_hit44 (SRC_EMITSHADOW_HOST44)
	const uint8_t *select;     // optional: 0 = the record samples no emitter
	uint32_t *out_emitter;     // the emitter sampled per record, or MRT_EMITTER_NONE
	EmitterTable table;
	uint32_t seed_add;         // frame * 6529 + 7 (+ y0 * grid_w * 1009 for a row band): seed = record * 1009 + seed_add
	HemiJump jump;             // (A, C) of draw `draw`
};

// ---- reflection rays from a rasteriser's G-buffer (gbuffer_kernel.h, gbuffer.h): one closest-hit ray per pixel of a whole frame -----
// Entry i of a G-buffer cast is pixel (i % w, i / w); TraceParams::count = w * h, hits = the output records (OUT_HIT32); rays is not
// read.  The matrices are part of the kernel argument: uniform, read with constant indices before the walk (scalar loads).
struct GBufferParams {
	const float *depth;        // w * h
	const void *guide;         // w * h normal-roughness texels, 4 floats each
	void *out_rays;            // optional: the rays made, mrt_ray32
	uint32_t w, h, normal_kind; // MRT_NORMAL_*
	float roughness_threshold;
	float max_distance;        // t_max of every ray
	float inv_projection[16], inv_view[16]; // column-major, as mrt_gbuffer gives them
};

// ---- shading surfaces (surface_kernel.h): one mrt_surface64 row per hit record, nothing walked ---------------------------------
// Record i of a resolve is entry i; TraceParams::count = records, rays = the incoming rays as for reflections (or the grid).  The
// resident shade data (shade_data.h): n_tris rows of 64 bytes, n_materials rows of 48; an absent per-triangle array is a bit not set
// in `present` (SHADE_HAS_*), never a per-row sentinel.
enum SurfaceSrc : int { SURF_RAY32 = 0, SURF_HOST = 1, SURF_GRID = 2 };
struct SurfaceParams {
	const void *records;       // mrt_hit32 (SURF_RAY32, SURF_GRID) or mrt_host_hit44 (SURF_HOST)
	const void *shade_rows;    // n_tris x 64 bytes (null when no per-triangle array is resident)
	const void *materials;     // n_materials x mrt_material
	uint32_t n_tris, n_materials, present;
	void *out_rows;            // optional: mrt_surface64 per record
	float *out_bounce;         // optional: {metallic, roughness} per record
	void *out_hits;            // optional: the records in the input layout, shading normal in place of the normal
};

// ---- the renderer's channels (channel_kernel.h): up to ten RGBA planes per hit record, floats and / or bytes, nothing walked -------
// Record i of a channel pass is entry i, as for a resolve; the shade data as in SurfaceParams.  mask: bit c set = channel c is
// selected (one of its two planes is given); a launch may carry a subset of a call's selection (channels.hip).
struct ChannelParams {
	const void *records;       // mrt_hit32 (SURF_RAY32, SURF_GRID) or mrt_host_hit44 (SURF_HOST)
	const void *shade_rows;    // n_tris x 64 bytes (null when no per-triangle array is resident)
	const void *materials;     // n_materials x mrt_material
	uint32_t n_tris, n_materials, present;
	uint32_t mask;
	float inv_depth_range, inv_pos_range;
	float *rgba[MRT_CHANNEL_COUNT];    // float4 per record, or null
	uint8_t *rgba8[MRT_CHANNEL_COUNT]; // 4 bytes per record, or null
};
// the channels that read the shade row, and those that read the material, the binding, the tangents and the texels
constexpr uint32_t CHANNELS_ROW = (1u << MRT_CHANNEL_NORMAL) | (1u << MRT_CHANNEL_ALBEDO) | (1u << MRT_CHANNEL_UV) | (1u << MRT_CHANNEL_FRESNEL);
constexpr uint32_t CHANNELS_MATERIAL = (1u << MRT_CHANNEL_NORMAL) | (1u << MRT_CHANNEL_ALBEDO);

// What the one launcher and the one set of kernels need to know of a source family, by its parameter struct: its three sources
// (RaySrc values: they are printed in mrt_last_kernel_variant; a family with one source names it three times), the modes it has (a
// family with one does not print it) and its name.
template <class S> struct SourceFamily;
template <> struct SourceFamily<ShadowParams> {
	static constexpr int ray32 = SRC_SHADOW_RAY32, host = SRC_SHADOW_HOST44, grid = SRC_SHADOW_GRID;
	static constexpr bool any_hit = true, nearest = false;
	static constexpr const char *name = "shadow";
};
template <> struct SourceFamily<ReflectParams> {
	static constexpr int ray32 = SRC_REFLECT_RAY32, host = SRC_REFLECT_HOST, grid = SRC_REFLECT_GRID;
	static constexpr bool any_hit = false, nearest = true;
	static constexpr const char *name = "reflection";
};
template <> struct SourceFamily<HemiParams> {
	static constexpr int ray32 = SRC_HEMI_RAY32, host = SRC_HEMI_HOST, grid = SRC_HEMI_GRID;
	static constexpr bool any_hit = true, nearest = true;
	static constexpr const char *name = "hemisphere";
};
template <> struct SourceFamily<BounceParams> {
	static constexpr int ray32 = SRC_BOUNCE_RAY32, host = SRC_BOUNCE_HOST, grid = SRC_BOUNCE_GRID;
	static constexpr bool any_hit = false, nearest = true;
	static constexpr const char *name = "bounce";
};
template <> struct SourceFamily<GBufferParams> {
	static constexpr int ray32 = SRC_GBUFFER, host = SRC_GBUFFER, grid = SRC_GBUFFER;
	static constexpr bool any_hit = false, nearest = true;
	static constexpr const char *name = "gbuffer";
};
template <> struct SourceFamily<SelectShadowParams> {
	static constexpr int ray32 = SRC_SELSHADOW_RAY32, host = SRC_SELSHADOW_HOST44, grid = SRC_SELSHADOW_GRID;
	static constexpr bool any_hit = true, nearest = false;
	static constexpr const char *name = "selected_shadow";
};

template <> struct SourceFamily<EmitterShadowParams> {
	static constexpr int ray32 = SRC_EMITSHADOW_RAY32, host = SRC_EMITSHADOW_HOST44, grid = SRC_EMITSHADOW_GRID;
	static constexpr bool any_hit = true, nearest = false;
	static constexpr const char *name = "emitter_shadow";
};

// host-side preparation (scene_prep.cpp)
struct DeviceSceneHost {
	DevNode *nodes = nullptr; uint32_t n_nodes = 0;
	Dev4Node *nodes4 = nullptr; uint32_t n_nodes4 = 0;
	uint32_t stack4 = 0;        // per-wave stack entries the 4-wide walk can need
	bool want8 = false;         // in: also build the 8-wide compressed collapse
	Dev8Node *nodes8 = nullptr; uint32_t n_nodes8 = 0; uint32_t stack8 = 0;
	float *leaf_box = nullptr;  // with nodes8: 8 floats per triangle slot, filled at the first slot of every leaf
	float bounds_lo[3] = {0, 0, 0}, bounds_hi[3] = {0, 0, 0}; // scene AABB (sort key quantisation)
	TriHot *hot = nullptr; TriCold *cold = nullptr; uint32_t n_tris = 0;
	uint32_t depth = 0;         // max stack entries any traversal can need (incl. sentinel)
};
// Returns MRT_OK or an error; on success arrays are malloc'ed (free with free()).
int prepare_scene(const mrt_tri64 *tris, uint32_t n_tris, const mrt_bvh_node32 *nodes, uint32_t used_nodes,
		const uint32_t *prim_idx, DeviceSceneHost *out, char *err, size_t err_len);

// device-side build (device_build.hip): LBVH over n >= 2 device-resident triangles (or boxes: boxes_in), written in the
// layout above.  Arrays are hipMalloc'ed and belong to the caller on success.  `stream` is a hipStream_t.
struct DeviceBuildResult {
	DevNode *nodes = nullptr; TriHot *hot = nullptr; TriCold *cold = nullptr;
	Dev4Node *nodes4 = nullptr;  // optional: one 4-wide node per binary node, at the binary node's index
	Dev8Node *nodes8 = nullptr;  // optional: likewise for the 8-wide compressed layout
	float *leaf_box = nullptr;   // with nodes8: exact leaf boxes, 8 floats per slot
	uint32_t n_nodes = 0, n_tris = 0, depth = 0, stack4 = 0, stack8 = 0;
	float bounds_lo[3] = {0, 0, 0}, bounds_hi[3] = {0, 0, 0};
	uint32_t *slot_src = nullptr; // in, optional: n device words, filled with the input triangle of every slot (what a refit rewrites slot k from)
	const float *boxes_in = nullptr; // in, with d_tris == nullptr: n device boxes {min xyz, max xyz} to build over (a top level over world boxes)
};
struct BuildArena { void *ptr = nullptr; size_t cap = 0; uint32_t *pinned = nullptr; }; // the builder's temporaries: owned by the context, grown on demand (pinned: 64 host bytes the per-level counters are read back into)
// form: 0 the radix tree over the Morton keys (fastest build), 1 PLOC, 2 binned SAH (the host builder's tree; leaves of several triangles)
int device_build_lbvh(const mrt_tri64 *d_tris, uint32_t n, bool want4, bool want8, bool safe_handoff, int form, BuildArena *arena, void *stream,
		DeviceBuildResult *out, char *err, size_t err_len);

// ---- two-level scene: SceneTLAS / MeshBLAS / BLASInstance
// (src/accel/scene_tlas.h:140-251, mesh_blas.h:86-138, blas_instance.h:47-107) -------------
// One node array: TLAS nodes at [0, tlas_cap) (rebuilt in place when instances move), the BLAS
// of every distinct mesh behind them, node and leaf refs already global.  A TLAS leaf ref is the
// first slot of a run of DevInstance rows (leaf order; the last row of a leaf has flags & 1).
constexpr uint32_t kAsmNodeLimit = 1u << 26;     // packet_asm_kernel.h: node index * 64 must fit 32 bits
constexpr uint32_t kInstanceReturn = 0x7FFFFFFEu; // stack marker: back from a BLAS to the TLAS walk
// kernel ids of two-level scenes (TraceParams.kernel; the values of the public enum, include/mrt_hip.h):
// MRT_KERNEL_TWO_LEVEL one lane per ray, _PACKET one wave per 64-ray packet (coherent batches), _PERSISTENT
// resident waves with node / leaf phases (large incoherent batches), _PERSISTENT8 the same with 8-wide BLAS nodes
using ::MRT_KERNEL_TWO_LEVEL; using ::MRT_KERNEL_TWO_LEVEL_PACKET; using ::MRT_KERNEL_TWO_LEVEL_PERSISTENT;
using ::MRT_KERNEL_TWO_LEVEL_PERSISTENT8;
struct alignas(16) DevInstance {
	float inv[12];      // world -> object, rows {m00 m01 m02 tx}: o' = M o + t, d' = M d (no renormalisation: t stays world-parameterised)
	float basis[9];     // object -> world 3x3 (normals: normalize(basis n))
	uint32_t root;      // BLAS root node (global index)
	uint32_t id_base;   // flat id of the instance's first triangle (running offset in registration order)
	uint32_t layers;    // the mesh's layer mask
	uint32_t flags;     // 1 = last instance of its TLAS leaf
	uint32_t index;     // registration index
	uint32_t root8;     // BLAS root in the 8-wide layout (scenes that have it)
	uint32_t pad[5];
};
static_assert(sizeof(DevInstance) == 128, "DevInstance must be 128 bytes");

// n_nodes: the rows the BLAS fills from root (a device SAH tree leaves the rest of its n_tris - 1 rows unused)
struct TwoLevelBlas { uint32_t first_tri, n_tris, root, depth; float lo[3], hi[3]; uint32_t root8, stack8, n_nodes; };
struct TwoLevelHost {
	DevNode *nodes = nullptr; uint32_t n_nodes = 0, tlas_cap = 0, n_tlas_nodes = 0;
	TriHot *hot = nullptr; TriCold *cold = nullptr; uint32_t n_tris = 0;   // all BLAS triangles, mesh-space
	DevInstance *inst = nullptr; uint32_t n_inst = 0;
	TwoLevelBlas *blas = nullptr; uint32_t n_blas = 0;
	uint32_t *inst_blas = nullptr;   // per registered instance: its BLAS
	uint32_t depth = 0;              // stack entries one ray can need
	// optional 8-wide compressed layout of every BLAS (the persistent kernel's walk for incoherent rays)
	Dev8Node *nodes8 = nullptr; uint32_t n_nodes8 = 0; float *leaf_box = nullptr;
	bool wide8 = false;              // every BLAS has it (set by the builder of the BLASes)
	uint32_t depth8 = 0;             // stack entries with 8-wide BLAS walks
	uint64_t flat_tris = 0;          // triangles of the flattened scene (sum over instances)
};
void free_two_level(TwoLevelHost *h);
// Builds every BLAS (binned SAH, as MeshBLAS::build) and the TLAS over the instances' world boxes.
// build_blas = false: only groups the instances by mesh and lays the BLAS roots out (device-built BLASes).
int prepare_two_level(const float *verts9, uint32_t n_mesh_tris, const mrt_instance *instances, uint32_t n_instances,
		uint32_t n_threads, bool build_blas, TwoLevelHost *out, char *err, size_t err_len);

// New transforms for the same instances: inverse, world box, TLAS rebuilt into nodes[0, tlas_cap) and inst[].
int refit_two_level(TwoLevelHost *h, const mrt_instance *instances, uint32_t n_instances, char *err, size_t err_len);
// What refit_two_level would refuse (instance count, mesh ranges, singular transforms) and a mesh range outside n_mesh_tris,
// checked without touching h: mrt_refit_two_level_scene refuses before any device write.  instances == nullptr (instances on the
// device): the count and the meshes' ranges only; the per-instance checks run on the device (tlas_device.hip).
int check_two_level_refit(const TwoLevelHost *h, const mrt_instance *instances, uint32_t n_instances, uint32_t n_mesh_tris,
		char *err, size_t err_len);

} // namespace mrt
