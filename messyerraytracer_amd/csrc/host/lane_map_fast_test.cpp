// lane_map_fast_test.cpp -- the short map of whole-tile pairs (lane_map.h: fast_launch, fast_grid, fast_wave_tile, fast_tile_ray,
// fast_lane_ray, fast_lane_pixel).  Two things, for listed, boundary and random launches: the test's answer against an expectation
// written down here, and, where it says yes, {ray index, px, py} of every lane of both groups of a wave against the general map
// (wave_tile + wave_tile_next + tile_lane).  Host code alone: no device, no library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../lane_map.h"

using namespace mrt;

namespace {

uint64_t rng_state = 0x2545F4914F6CDD1Dull;
uint64_t rnd() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

long checks = 0, failures = 0;
void expect(bool ok, const char *what, uint32_t a = 0u, uint32_t b = 0u, uint32_t c = 0u)
{
	checks++;
	if (!ok && failures++ < 20) printf("FAIL %s (%u, %u, %u)\n", what, a, b, c);
}

// a launch the short map takes: two groups, not counting, 8x8 tiles row-major, no pieces, schedule, permutation or cost notes,
// 32-byte rays and records, its own grid, no skip word
FastLaunch yes_launch()
{
	FastLaunch f;
	f.packets = 2u; f.counting = false; f.lane_map = 1u; f.k = 3u; f.order = 0u; f.quarter_all = 0u;
	f.sched = f.perm = f.tile_cost = false; f.ray32_in = f.hit32_out = true; f.auto_grid = false; f.skip = 0;
	return f;
}

void launches()
{
	FastLaunch f = yes_launch();
	expect(fast_launch(f) == kFastOwnGrid, "a tiled launch with its own grid");
	f.auto_grid = true; expect(fast_launch(f) == kFastOwnGrid, "... the device's grid words set but not asked for");
	f = yes_launch(); f.skip = 1; expect(fast_launch(f) == kFastNo, "a tiled launch with a skip word");
	f.skip = 2; expect(fast_launch(f) == kFastNo, "a tiled launch with a skip word elsewhere");
	f = yes_launch(); f.lane_map = 2u; f.auto_grid = true; f.skip = 1; expect(fast_launch(f) == kFastAutoSkip, "a grid found on the device, skip word 3");
	f.skip = 0; expect(fast_launch(f) == kFastAuto, "a grid found on the device, no skip word");
	f.skip = 2; expect(fast_launch(f) == kFastNo, "a grid found on the device, a skip word elsewhere");
	f.skip = 1; f.auto_grid = false; expect(fast_launch(f) == kFastNo, "MAP_AUTO without the device's words");
	f = yes_launch(); f.lane_map = 0u; expect(fast_launch(f) == kFastNo, "the linear map");
	f.lane_map = 3u; expect(fast_launch(f) == kFastNo, "no map at all");
	// every other word, one at a time, on all three forms of yes
	for (int form = 0; form < 3; form++) {
		FastLaunch y = yes_launch();
		if (form) { y.lane_map = 2u; y.auto_grid = true; y.skip = form == 1 ? 1 : 0; }
		const uint32_t want = form == 0 ? kFastOwnGrid : (form == 1 ? kFastAutoSkip : kFastAuto);
		expect(fast_launch(y) == want, "the form itself", (uint32_t)form);
		f = y; f.packets = 1u; expect(fast_launch(f) == kFastNo, "one group per wave", (uint32_t)form);
		f = y; f.packets = 4u; expect(fast_launch(f) == kFastNo, "four groups per wave", (uint32_t)form);
		f = y; f.counting = true; expect(fast_launch(f) == kFastNo, "a counting build", (uint32_t)form);
		for (uint32_t k = 0u; k <= 6u; k++) { f = y; f.k = k; expect((fast_launch(f) != kFastNo) == (k == 3u), "tile_w_log2", (uint32_t)form, k); }
		for (uint32_t o = 0u; o <= 4u; o++) { f = y; f.order = o; expect((fast_launch(f) != kFastNo) == (o == 0u), "tile_order", (uint32_t)form, o); }
		for (uint32_t q = 0u; q <= 2u; q++) { f = y; f.quarter_all = q; expect((fast_launch(f) != kFastNo) == (q == 0u), "quarter_all", (uint32_t)form, q); }
		f = y; f.sched = true; expect(fast_launch(f) == kFastNo, "a schedule", (uint32_t)form);
		f = y; f.perm = true; expect(fast_launch(f) == kFastNo, "a permutation", (uint32_t)form);
		f = y; f.tile_cost = true; expect(fast_launch(f) == kFastNo, "tile-cost notes", (uint32_t)form);
		f = y; f.ray32_in = false; expect(fast_launch(f) == kFastNo, "rays of another format", (uint32_t)form);
		f = y; f.hit32_out = false; expect(fast_launch(f) == kFastNo, "records of another format", (uint32_t)form);
	}
}

// the grid's part as the task states it, written apart from fast_grid: whole 8x8 tiles, an even number per tile row, tiles_x what the
// width gives, fewer than 2^32 rays
bool want_grid(uint32_t w, uint32_t rows, uint32_t tiles_x)
{
	if (w == 0u || rows == 0u) return false;
	if (w % 16u != 0u || rows % 8u != 0u) return false;
	if (tiles_x != (w + 7u) / 8u) return false;
	return (uint64_t)w * (uint64_t)rows <= 0xFFFFFFFFull;
}

// every lane of both groups of waves [first, first + n) of a grid the short map takes, against the general map
void check_waves(uint32_t w, uint32_t rows, uint32_t first, uint32_t n)
{
	TileGrid g;
	g.grid_w = w; g.rows = rows; g.tiles_x = w >> 3; g.k = 3u; g.tiles_y = tile_rows_of(rows, 3u);
	g.order = 0u; g.group = 2u; g.quarter_all = 0u; g.sched = nullptr; g.unit = 1u; g.sched_slots = 0u;
	const uint64_t pairs = (uint64_t)g.tiles_x * g.tiles_y / 2u;
	for (uint64_t pair = first; pair < (uint64_t)first + n; pair++) {
		uint32_t tx = 0u, ty = 0u;
		const bool in = fast_wave_tile(w, rows, (uint32_t)pair, tx, ty);
		expect(in == (pair < pairs), "fast_wave_tile: the last pair", w, rows, (uint32_t)pair);
		if (!in || pair >= pairs) continue;
		const WaveTile ta = wave_tile(g, pair * 2u), tb = wave_tile_next(g, ta, pair * 2u);
		expect(ta.tx == tx && ta.ty == ty && tb.tx == tx + 1u && tb.ty == ty, "the wave's tiles", w, rows, (uint32_t)pair);
		const uint32_t ray0 = fast_tile_ray(w, tx, ty);
		for (uint32_t l = 0u; l < 64u; l++) {
			uint64_t ia = 0, ib = 0; uint32_t ax = 0, ay = 0, bx = 0, by = 0, px = 0, py = 0;
			const bool va = tile_lane(g, ta, l, ia, ax, ay), vb = tile_lane(g, tb, l, ib, bx, by);
			fast_lane_pixel(tx, ty, l, px, py);
			const uint32_t ray = fast_lane_ray(w, ray0, l);
			expect(va && ia == ray && ax == px && ay == py, "group A's lane", w, rows, (uint32_t)pair * 64u + l);
			expect(vb && ib == (uint64_t)ray + 8u && bx == px + 8u && by == py, "group B's lane", w, rows, (uint32_t)pair * 64u + l);
		}
	}
}

void one_grid(uint32_t w, uint32_t rows, uint32_t tiles_x, int listed)
{
	const bool want = want_grid(w, rows, tiles_x), got = fast_grid(w, rows, tiles_x);
	expect(got == want, "fast_grid against the statement", w, rows, tiles_x);
	if (listed >= 0) expect(got == (listed != 0), "fast_grid against the list", w, rows, tiles_x);
	if (!got || !want) return;
	const uint64_t pairs = (uint64_t)(w >> 4) * (rows >> 3);
	if (pairs <= 600u) { check_waves(w, rows, 0u, (uint32_t)pairs + 3u); return; }
	check_waves(w, rows, 0u, 200u);
	check_waves(w, rows, (uint32_t)(pairs - 200u), 203u);
	check_waves(w, rows, (w >> 4) > 2u ? (w >> 4) - 2u : 0u, 4u); // around the end of the first tile row
	for (int it = 0; it < 60; it++) check_waves(w, rows, (uint32_t)(rnd() % (pairs - 2u)), 3u);
}

} // namespace

int main()
{
	launches();
	// listed grids: {width, rows, tiles_x, the answer}
	const uint32_t listed[][4] = {
		{32u, 8u, 4u, 1u}, {16u, 16u, 2u, 1u}, {48u, 8u, 6u, 1u}, {64u, 16u, 8u, 1u}, {16u, 8u, 2u, 1u},   // the smallest, a division that is no shift, two tile rows
		{24u, 8u, 3u, 0u}, {16u, 12u, 2u, 0u}, {40u, 8u, 5u, 0u}, {8u, 8u, 1u, 0u}, {17u, 9u, 3u, 0u},     // an odd tile count, clipped rows, a width off 16
		{0u, 8u, 0u, 0u}, {16u, 0u, 2u, 0u}, {0u, 0u, 0u, 0u},                                              // no grid found
		{16u, 8u, 3u, 0u}, {32u, 8u, 2u, 0u}, {32u, 8u, 0u, 0u},                                            // tiles_x of another width
		{4096u, 4096u, 512u, 1u}, {1920u, 1080u, 240u, 1u}, {1920u, 1084u, 240u, 0u}, {3840u, 2160u, 480u, 1u}, {2048u, 40u, 256u, 1u},
		{65536u, 65536u, 8192u, 0u}, {65536u, 65528u, 8192u, 1u}, {0x80000000u, 8u, 0x10000000u, 0u},      // 2^32 rays, and just below
		{0xFFFFFFF0u, 8u, 0x1FFFFFFEu, 0u}, {0x10000000u, 8u, 0x2000000u, 1u}, {16u, 0xFFFFFFF8u, 2u, 0u}, {16u, 0x0FFFFFF8u, 2u, 1u},
	};
	for (auto &l : listed) one_grid(l[0], l[1], l[2], (int)l[3]);
	// boundary launches: widths and row counts around the multiples, tiles_x right, one off, and of the width rounded down
	for (uint32_t w = 0u; w <= 130u; w++) for (uint32_t rows = 0u; rows <= 34u; rows++) {
		one_grid(w, rows, (w + 7u) >> 3, -1);
		if ((w & 15u) == 0u && (rows & 7u) == 0u) { one_grid(w, rows, ((w + 7u) >> 3) + 1u, -1); one_grid(w, rows, (w >> 3) - 1u, -1); }
	}
	// random launches: mostly on the multiples, sometimes off them, sometimes large
	for (int it = 0; it < 6000; it++) {
		uint32_t w = (1u + below(it % 10 == 0 ? 4096u : 40u)) * 16u, rows = (1u + below(it % 10 == 1 ? 2048u : 30u)) * 8u;
		if (it % 4 == 1) w += below(16);
		if (it % 4 == 2) rows += below(8);
		if (it % 50 == 3) { w = (uint32_t)(rnd() >> 40) & ~15u; rows = (uint32_t)(rnd() >> 44) & ~7u; }
		uint32_t tiles_x = (w + 7u) >> 3;
		if (it % 9 == 4) tiles_x += below(3) - 1u;
		one_grid(w, rows, tiles_x, -1);
	}
	if (failures) { printf("%ld of %ld checks FAIL\n", failures, checks); return 1; }
	printf("lane_map_fast_test: %ld checks hold (the short map = the general map where the test says yes)\n", checks);
	return 0;
}
