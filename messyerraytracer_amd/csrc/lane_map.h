// lane_map.h -- which ray a lane of a launch traces (lane_ray_index_g, device_common.h), in two parts: what the 64 lanes of a group
// share (its tile, and which piece of the tile) and what differs between them (the pixel inside the tile, the clip test).  The first
// part divides and takes remainders, all of wave-uniform values: a kernel that keeps its group index in scalar registers gets it
// done on the scalar unit, once per group, in 32-bit arithmetic whenever the numbers fit.  No HIP types: csrc/host/lane_map_test.cpp
// compiles this for the CPU and holds both parts to the one-function form they replace.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define MRT_LM_HD __host__ __device__ __forceinline__
#else
#define MRT_LM_HD inline
#endif

namespace mrt {

// What the map needs of a launch with a tiled grid (MAP_TILE8X8, or MAP_AUTO with a grid found), every word wave-uniform.
struct TileGrid {
	uint32_t grid_w, rows;       // the clip rectangle
	uint32_t tiles_x, tiles_y;   // tiles_y = ceil(rows / tile height)
	uint32_t k;                  // tile_w_log2: a tile is 2^k wide, 64 / 2^k high
	uint32_t order;              // tile_order
	uint32_t group;              // tile_group (tile_order 3)
	uint32_t quarter_all;
	const uint32_t *sched;       // the tile schedule, or null: none, or not one of this grid (sched_matches)
	uint32_t unit, sched_slots;  // with sched: tile_unit, launch slots in use
};

// The piece of its tile a group works on: 0..15 = that 2x2 sixteenth in lanes 0..3, 16..19 = that 4x4 quarter in lanes 0..15,
// kPieceTile = the whole tile, kPieceTile16 = the whole tile's map in lanes 0..15 only (a schedule entry above 5: no quarter),
// kPieceNone = nothing.
constexpr uint32_t kPieceTile = 20u, kPieceTile16 = 21u, kPieceNone = 0xFFu;
// How the NEXT group's tile follows from this one's (wave_tile_next): kNextSame = the next piece of the same tile, kNextRight = the
// tile to the right, kNextRowMajor = the same with a wrap to the next tile row, kNextNone = nothing, kNextAnew = mapped from scratch.
constexpr uint32_t kNextAnew = 0u, kNextSame = 1u, kNextRight = 2u, kNextRowMajor = 3u, kNextNone = 4u;
struct WaveTile {
	uint32_t tx, ty;   // the tile's column and row
	uint32_t code;     // piece | next << 8
};

MRT_LM_HD uint32_t tile_rows_of(uint32_t rows, uint32_t k) { return (rows + (64u >> k) - 1u) >> (6u - k); }

// ceil(total / unit) == n_units without dividing: a schedule sized for another grid is not used.  unit >= 1.
MRT_LM_HD bool sched_matches(uint64_t total, uint32_t unit, uint32_t n_units)
{
	if (n_units == 0u) return total == 0u;
	return (uint64_t)(n_units - 1u) * unit < total && total <= (uint64_t)n_units * unit;
}

// tile_order 3 (device_common.h, xcd_strips): every XCD works down its own column strips.  T = uint32_t or uint64_t.
template <class T>
MRT_LM_HD bool strip_tile(const TileGrid &g, T tile, uint32_t &tx, uint32_t &ty)
{
	const uint32_t tg = g.group ? g.group : 1u;
	uint32_t m = (g.tiles_x + 128u) >> 8;
	if (m == 0u) m = 1u;
	const uint32_t S = g.tiles_x / (8u * m);
	if (S == 0u || S * 8u * m != g.tiles_x || S % tg != 0u) return false;
	const T wg = tile / tg;
	const uint32_t x = (uint32_t)wg & 7u;
	const T j = (wg >> 3) * tg + (tile - wg * tg); // the tile's place in its XCD's own sequence
	const T per_strip = (T)S * g.tiles_y;
	const T q = j / per_strip;
	const uint32_t sl = (uint32_t)q, r = (uint32_t)(j - q * per_strip);
	ty = r / S;
	tx = (sl * 8u + x) * S + r % S;
	return true;
}

template <class T>
MRT_LM_HD WaveTile wave_tile_t(const TileGrid &g, T group)
{
	WaveTile w; w.tx = 0u; w.ty = 0u; w.code = kPieceNone;
	const T total = (T)g.tiles_x * g.tiles_y;
	T tile = group;
	uint32_t piece = kPieceTile, next = kNextAnew;
	bool plus1 = false; // the next group's tile is tile + 1
	if (g.quarter_all == 2u) {
		piece = (uint32_t)tile & 15u; tile >>= 4;
		if (tile >= total) return w;
		if (piece < 15u) next = kNextSame;
	} else if (g.quarter_all) {
		piece = 16u + ((uint32_t)tile & 3u); tile >>= 2;
		if (tile >= total) return w;
		if (piece < 19u) next = kNextSame;
	} else if (g.sched != nullptr) {
		const T slot = g.unit == 1u ? tile : (g.unit == 2u ? tile >> 1 : tile / g.unit); // (the units in use: 1, and 2 for the 128-ray walk)
		const uint32_t rem = (uint32_t)(tile - slot * g.unit);
		if (slot >= g.sched_slots) return w;
		const uint32_t e = g.sched[slot], what = e >> 28, id = e & 0x0FFFFFFFu;
		if (what == 0u) { tile = (T)id * g.unit + rem; plus1 = rem + 1u < g.unit; }
		else {
			if (rem != 0u) return w; // a piece is (part of) one tile: a second group of the wave has nothing to do
			tile = id;
			if (what >= 2u) piece = what - 2u < 4u ? 16u + (what - 2u) : kPieceTile16;
			if (g.unit > 1u) next = kNextNone;
		}
	} else plus1 = true;
	const bool even = ((uint32_t)tile & 1u) == 0u;
	if (g.order == 1u && (g.tiles_x & 15u) == 0u && (g.tiles_y & 15u) == 0u) {
		// 16x16-tile super-tiles in row-major order, Z-order inside
		const uint32_t st = (uint32_t)(tile >> 8), in = (uint32_t)tile & 255u;
		uint32_t mx = in & 0x55u, my = (in >> 1) & 0x55u; // de-interleave 4+4 bits
		mx = (mx | (mx >> 1)) & 0x33u; mx = (mx | (mx >> 2)) & 0x0Fu;
		my = (my | (my >> 1)) & 0x33u; my = (my | (my >> 2)) & 0x0Fu;
		const uint32_t sx = g.tiles_x >> 4, sty = st / sx;
		w.tx = ((st - sty * sx) << 4) + mx; w.ty = (sty << 4) + my;
		if (plus1 && even) next = kNextRight; // (bit 0 of a Z-order index is bit 0 of the column)
	} else if (g.order == 2u && (g.tiles_x & 31u) == 0u && (g.tiles_y & 31u) == 0u) {
		const uint32_t st = (uint32_t)(tile >> 10), in = (uint32_t)tile & 1023u;
		uint32_t mx = in & 0x155u, my = (in >> 1) & 0x155u; // de-interleave 5+5 bits
		mx = (mx | (mx >> 1)) & 0x133u; mx = (mx | (mx >> 2)) & 0x10Fu; mx = (mx | (mx >> 4)) & 0x1Fu;
		my = (my | (my >> 1)) & 0x133u; my = (my | (my >> 2)) & 0x10Fu; my = (my | (my >> 4)) & 0x1Fu;
		const uint32_t sx = g.tiles_x >> 5, sty = st / sx;
		w.tx = ((st - sty * sx) << 5) + mx; w.ty = (sty << 5) + my;
		if (plus1 && even) next = kNextRight;
	} else if (g.order == 3u && strip_tile<T>(g, tile, w.tx, w.ty)) {
		// an even tile of an even tile_group has its successor in the same workgroup, strip and row (a strip is S tiles wide, S a multiple
		// of the group): one column on
		if (plus1 && even && g.group != 0u && (g.group & 1u) == 0u) next = kNextRight;
	} else {
		const T y = tile / g.tiles_x;
		w.tx = (uint32_t)(tile - y * g.tiles_x); w.ty = (uint32_t)y;
		if (plus1) next = kNextRowMajor;
	}
	w.code = piece | next << 8;
	return w;
}

// The tile of group `group` (= g >> 6 of lane_ray_index_g).  The narrow form holds whenever nothing it computes can pass 2^32: the
// group index, the tile count, and a schedule entry's 28-bit id times the unit.
MRT_LM_HD WaveTile wave_tile(const TileGrid &g, uint64_t group)
{
	const bool narrow = (group >> 32) == 0u && (((uint64_t)g.tiles_x * g.tiles_y) >> 32) == 0u && (g.sched == nullptr || g.unit <= 16u);
	return narrow ? wave_tile_t<uint32_t>(g, (uint32_t)group) : wave_tile_t<uint64_t>(g, group);
}

// The tile of group + 1, given the one of `group`.
MRT_LM_HD WaveTile wave_tile_next(const TileGrid &g, const WaveTile &a, uint64_t group)
{
	WaveTile b = a;
	const uint32_t piece = a.code & 0xFFu, next = piece == kPieceNone ? kNextAnew : a.code >> 8;
	b.code = piece | kNextAnew << 8; // (only a tile mapped from scratch says how its successor follows)
	if (next == kNextSame) { b.code += 1u; return b; }
	if (next == kNextNone) { b.code = kPieceNone; return b; }
	if (next == kNextRight) { b.tx = a.tx + 1u; return b; }
	if (next == kNextRowMajor) {
		b.tx = a.tx + 1u;
		if (b.tx == g.tiles_x) { b.tx = 0u; b.ty = a.ty + 1u; }
		return b;
	}
	return wave_tile(g, group + 1u);
}

// The lane's pixel in its group's tile, and its ray; false = no ray (a lane outside the piece, a pixel outside the grid).
MRT_LM_HD bool tile_lane(const TileGrid &g, const WaveTile &w, uint32_t l, uint64_t &ray_idx, uint32_t &px, uint32_t &py)
{
	const uint32_t piece = w.code & 0xFFu;
	if (piece == kPieceNone) return false;
	if (piece < 16u) {
		if (l >= 4u) return false;
		px = (w.tx << 3) + ((piece & 3u) << 1) + (l & 1u);
		py = (w.ty << 3) + ((piece >> 2) << 1) + (l >> 1);
	} else if (piece < kPieceTile) { // (schedule pieces exist for 8x8 tiles only: k == 3)
		if (l >= 16u) return false;
		px = (w.tx << 3) + ((piece & 1u) << 2) + (l & 3u);
		py = (w.ty << 3) + (((piece >> 1) & 1u) << 2) + (l >> 2);
	} else {
		if (piece == kPieceTile16 && l >= 16u) return false;
		px = (w.tx << g.k) + (l & ((1u << g.k) - 1u));
		py = (w.ty << (6u - g.k)) + (l >> g.k);
	}
	if (px >= g.grid_w || py >= g.rows) return false;
	ray_idx = (uint64_t)py * g.grid_w + px;
	return true;
}

// ---- whole-tile pairs: the launches whose map needs none of the above -------------------------------------------------------------
// A wave of two groups (the 128-ray walk) that casts whole 8x8 tiles in row-major pairs, reads 32-byte rays and writes 32-byte
// records takes a short form of the map (packet_rows_kernel.h): one 32-bit division per wave, two shifts and two adds per lane, no
// validity flags (every lane has a ray), group B = A's right-hand neighbour.  The test is in two parts.  fast_launch: what the host
// knows of a launch (launch_trace asks it once and leaves the answer in TraceParams::rows_fast); fast_grid: the grid's size, which
// a MAP_AUTO launch learns on the device.  csrc/host/lane_map_fast_test.cpp holds both to a listed expectation and the short map to
// wave_tile + wave_tile_next + tile_lane.
struct FastLaunch {
	uint32_t packets;            // groups per wave
	bool counting;               // a counting build
	uint32_t lane_map;           // LaneMap (mrt_internal.h): 0 linear, 1 tiled, 2 the grid is found on the device
	uint32_t k, order, quarter_all;
	bool sched, perm, tile_cost; // the launch has a tile schedule / a sort permutation / tile-cost notes (the pointer is set)
	bool ray32_in, hit32_out;    // 32-byte rays in, 32-byte records out
	bool auto_grid;              // the device's grid words are there (the pointer is set)
	int skip;                    // the launch's skip word: 0 none, 1 word 3 of the grid words, 2 anywhere else
};
// 0: the general map.  Else how the kernel gets the grid and the skip word: 1 = the launch's own grid, no skip word; 2 = the device's
// four words {width, rows, tiles_x, skip word}; 3 = the device's first three, no skip word.
constexpr uint32_t kFastNo = 0u, kFastOwnGrid = 1u, kFastAutoSkip = 2u, kFastAuto = 3u;
MRT_LM_HD uint32_t fast_launch(const FastLaunch &f)
{
	if (f.packets != 2u || f.counting || f.k != 3u || f.order != 0u || f.quarter_all != 0u) return kFastNo;
	if (f.sched || f.perm || f.tile_cost || !f.ray32_in || !f.hit32_out) return kFastNo;
	if (f.lane_map == 1u) return f.skip == 0 ? kFastOwnGrid : kFastNo;
	if (f.lane_map == 2u && f.auto_grid) return f.skip == 1 ? kFastAutoSkip : (f.skip == 0 ? kFastAuto : kFastNo);
	return kFastNo;
}
// The grid's part: whole tiles in pairs on every tile row (no clipped tile, no wave without a group B, no pair across two tile rows),
// tiles_x what the width says, and rays -- so tiles too -- below 2^32.  width 0 = no grid was found.
MRT_LM_HD bool fast_grid(uint32_t grid_w, uint32_t rows, uint32_t tiles_x)
{
	return grid_w != 0u && rows != 0u && (grid_w & 15u) == 0u && (rows & 7u) == 0u && tiles_x == grid_w >> 3 && (((uint64_t)grid_w * rows) >> 32) == 0u;
}
// Wave `pair` of such a launch (its groups are 2 pair and 2 pair + 1): group A's tile; false = past the grid's last pair.
MRT_LM_HD bool fast_wave_tile(uint32_t grid_w, uint32_t rows, uint32_t pair, uint32_t &tx, uint32_t &ty)
{
	const uint32_t pairs_x = grid_w >> 4;
	ty = pair / pairs_x;
	tx = (pair - ty * pairs_x) << 1;
	return ty < rows >> 3;
}
// What such a wave keeps of its tiles: the ray of tile A's first pixel ...
MRT_LM_HD uint32_t fast_tile_ray(uint32_t grid_w, uint32_t tx, uint32_t ty) { return (ty << 3) * grid_w + (tx << 3); }
// ... from which lane l's ray in group A follows; in group B it is 8 more.
MRT_LM_HD uint32_t fast_lane_ray(uint32_t grid_w, uint32_t tile_ray, uint32_t l) { return tile_ray + (l >> 3) * grid_w + (l & 7u); }
// Lane l's pixel in group A (rays made from a camera need it); in group B px is 8 more.
MRT_LM_HD void fast_lane_pixel(uint32_t tx, uint32_t ty, uint32_t l, uint32_t &px, uint32_t &py)
{
	px = (tx << 3) + (l & 7u); py = (ty << 3) + (l >> 3);
}

// The linear map: lane l of group `group` takes entry group * 64 + l, or with sparse_lanes = n (rays in lanes 0 .. n - 1 only)
// entry group * n + l.  false = no entry.
MRT_LM_HD bool linear_lane(uint64_t group, uint32_t l, uint32_t sparse_lanes, uint64_t count, uint64_t &entry)
{
	if (sparse_lanes) { if (l >= sparse_lanes) return false; entry = group * sparse_lanes + l; }
	else entry = (group << 6) + l;
	return entry < count;
}

} // namespace mrt
