// lane_map_test.cpp -- the two-part lane map of lane_map.h (wave_tile / wave_tile_next / tile_lane, linear_lane, sched_matches)
// against the one function it replaces, restated here as it stood: every lane of every group, for random grids, tile shapes, tile
// orders, schedules with pieces and quarter modes, for the edge widths and row counts, and for a tile count above 2^32.  Host code
// alone: no device, no library.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../lane_map.h"

using namespace mrt;

namespace {

struct Params { // the words of TraceParams the map reads
	uint32_t grid_w, rows, tiles_x, tile_w_log2, tile_order, tile_group, quarter_all;
	const uint32_t *tile_sched; uint32_t tile_unit, n_units; const uint32_t *sched_hdr;
	uint32_t sparse_lanes; uint64_t count;
};

bool ref_strips(const Params &p, uint64_t tile, uint32_t tiles_x, uint32_t tiles_y, uint32_t &tx, uint32_t &ty)
{
	const uint32_t tg = p.tile_group ? p.tile_group : 1u;
	uint32_t m = (tiles_x + 128u) >> 8;
	if (m == 0u) m = 1u;
	const uint32_t S = tiles_x / (8u * m);
	if (S == 0u || S * 8u * m != tiles_x || S % tg != 0u) return false;
	const uint64_t wg = tile / tg;
	const uint32_t k = (uint32_t)wg & 7u;
	const uint64_t j = (wg >> 3) * tg + tile % tg;
	const uint64_t per_strip = (uint64_t)S * tiles_y;
	const uint32_t sl = (uint32_t)(j / per_strip), r = (uint32_t)(j % per_strip);
	ty = r / S;
	tx = (sl * 8u + k) * S + r % S;
	return true;
}

// the tiled branch of lane_ray_index_g as it was
bool ref_tiled(const Params &p, uint64_t g, uint64_t &ray_idx, uint32_t &px, uint32_t &py)
{
	const uint32_t grid_w = p.grid_w, rows = p.rows, tiles_x = p.tiles_x;
	uint64_t tile = g >> 6;
	const uint32_t l = (uint32_t)g & 63u;
	uint32_t tx, ty;
	const uint32_t k = p.tile_w_log2;
	const uint32_t tiles_y = (rows + (64u >> k) - 1u) >> (6u - k);
	uint32_t quarter = 4u, sixteenth = 16u;
	if (p.quarter_all == 2u) { sixteenth = (uint32_t)tile & 15u; tile >>= 4; if (l >= 4u || tile >= (uint64_t)tiles_x * tiles_y) return false; }
	else if (p.quarter_all) { quarter = (uint32_t)tile & 3u; tile >>= 2; if (l >= 16u || tile >= (uint64_t)tiles_x * tiles_y) return false; }
	else if (p.tile_sched != nullptr && ((uint64_t)tiles_x * tiles_y + p.tile_unit - 1u) / p.tile_unit == p.n_units) {
		const uint64_t slot = tile / p.tile_unit;
		if (slot >= (p.sched_hdr ? p.sched_hdr[2] : p.n_units)) return false;
		const uint32_t e = p.tile_sched[slot], what = e >> 28, id = e & 0x0FFFFFFFu;
		if (what == 0u) tile = (uint64_t)id * p.tile_unit + tile % p.tile_unit;
		else {
			if (tile % p.tile_unit != 0u) return false;
			tile = id;
			if (what >= 2u) { quarter = what - 2u; if (l >= 16u) return false; }
		}
	}
	if (p.tile_order == 1u && (tiles_x & 15u) == 0u && (tiles_y & 15u) == 0u) {
		const uint32_t st = (uint32_t)(tile >> 8), in = (uint32_t)tile & 255u;
		uint32_t mx = in & 0x55u, my = (in >> 1) & 0x55u;
		mx = (mx | (mx >> 1)) & 0x33u; mx = (mx | (mx >> 2)) & 0x0Fu;
		my = (my | (my >> 1)) & 0x33u; my = (my | (my >> 2)) & 0x0Fu;
		const uint32_t stx = st % (tiles_x >> 4), sty = st / (tiles_x >> 4);
		tx = (stx << 4) + mx; ty = (sty << 4) + my;
	} else if (p.tile_order == 2u && (tiles_x & 31u) == 0u && (tiles_y & 31u) == 0u) {
		const uint32_t st = (uint32_t)(tile >> 10), in = (uint32_t)tile & 1023u;
		uint32_t mx = in & 0x155u, my = (in >> 1) & 0x155u;
		mx = (mx | (mx >> 1)) & 0x133u; mx = (mx | (mx >> 2)) & 0x10Fu; mx = (mx | (mx >> 4)) & 0x1Fu;
		my = (my | (my >> 1)) & 0x133u; my = (my | (my >> 2)) & 0x10Fu; my = (my | (my >> 4)) & 0x1Fu;
		const uint32_t stx = st % (tiles_x >> 5), sty = st / (tiles_x >> 5);
		tx = (stx << 5) + mx; ty = (sty << 5) + my;
	} else if (p.tile_order == 3u && ref_strips(p, tile, tiles_x, tiles_y, tx, ty)) {
	} else { tx = (uint32_t)(tile % tiles_x); ty = (uint32_t)(tile / tiles_x); }
	if (sixteenth < 16u) {
		px = (tx << 3) + ((sixteenth & 3u) << 1) + (l & 1u);
		py = (ty << 3) + ((sixteenth >> 2) << 1) + (l >> 1);
	} else if (quarter < 4u) {
		px = (tx << 3) + ((quarter & 1u) << 2) + (l & 3u);
		py = (ty << 3) + ((quarter >> 1) << 2) + (l >> 2);
	} else {
		px = (tx << k) + (l & ((1u << k) - 1u));
		py = (ty << (6u - k)) + (l >> k);
	}
	if (px >= grid_w || py >= rows) return false;
	ray_idx = (uint64_t)py * grid_w + px;
	return true;
}
// and the linear branch, up to the entry (perm and the camera pixel follow it unchanged)
bool ref_linear(const Params &p, uint64_t g, uint64_t &entry)
{
	if (p.sparse_lanes) { const uint32_t l = (uint32_t)g & 63u; if (l >= p.sparse_lanes) return false; g = (g >> 6) * p.sparse_lanes + l; }
	if (g >= p.count) return false;
	entry = g;
	return true;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

long checks = 0, failures = 0;

TileGrid grid_of(const Params &p)
{
	TileGrid g;
	g.grid_w = p.grid_w; g.rows = p.rows; g.tiles_x = p.tiles_x; g.k = p.tile_w_log2; g.tiles_y = tile_rows_of(p.rows, p.tile_w_log2);
	g.order = p.tile_order; g.group = p.tile_group; g.quarter_all = p.quarter_all;
	g.sched = nullptr; g.unit = 1u; g.sched_slots = 0u;
	if (!p.quarter_all && p.tile_sched != nullptr && sched_matches((uint64_t)g.tiles_x * g.tiles_y, p.tile_unit, p.n_units)) {
		g.sched = p.tile_sched; g.unit = p.tile_unit; g.sched_slots = p.sched_hdr ? p.sched_hdr[2] : p.n_units;
	}
	return g;
}

// groups [first, first + n) of one launch: every lane through wave_tile + tile_lane, and through wave_tile_next from its predecessor
void check_groups(const Params &p, uint64_t first, uint64_t n, const char *what)
{
	const TileGrid g = grid_of(p);
	WaveTile prev = {0u, 0u, kPieceNone};
	for (uint64_t group = first; group < first + n; group++) {
		const WaveTile w = wave_tile(g, group);
		const WaveTile wn = group > first ? wave_tile_next(g, prev, group - 1u) : w;
		prev = w;
		for (uint32_t l = 0; l < 64u; l++) {
			uint64_t ri = 0, i1 = 0, i2 = 0; uint32_t rx = 0, ry = 0, x1 = 0, y1 = 0, x2 = 0, y2 = 0;
			const bool rv = ref_tiled(p, group * 64u + l, ri, rx, ry);
			const bool v1 = tile_lane(g, w, l, i1, x1, y1), v2 = tile_lane(g, wn, l, i2, x2, y2);
			checks += 2;
			const bool ok1 = rv == v1 && (!rv || (ri == i1 && rx == x1 && ry == y1)), ok2 = rv == v2 && (!rv || (ri == i2 && rx == x2 && ry == y2));
			if (!ok1 || !ok2) {
				if (failures++ < 20)
					printf("FAIL %s: grid %ux%u tiles_x %u k %u order %u group %u quarter_all %u unit %u sched %d: group %llu lane %u: was %d (%u, %u), "
							"is %d (%u, %u), from the predecessor %d (%u, %u)\n", what, p.grid_w, p.rows, p.tiles_x, p.tile_w_log2, p.tile_order,
							p.tile_group, p.quarter_all, p.tile_unit, g.sched != nullptr, (unsigned long long)group, l, rv, rx, ry, v1, x1, y1, v2, x2, y2);
			}
		}
	}
}

void one_grid(uint32_t grid_w, uint32_t rows, uint32_t k, uint32_t order, uint32_t quarter_all, uint32_t unit, int sched_kind, uint32_t tile_group, bool sample = false)
{
	Params p = {};
	p.grid_w = grid_w; p.rows = rows; p.tile_w_log2 = k; p.tiles_x = (grid_w + (1u << k) - 1u) >> k;
	p.tile_order = order; p.tile_group = tile_group; p.quarter_all = quarter_all; p.tile_unit = unit;
	const uint64_t total = (uint64_t)p.tiles_x * tile_rows_of(rows, k);
	const uint32_t n_units = (uint32_t)((total + unit - 1u) / unit);
	std::vector<uint32_t> sched; uint32_t hdr[3] = {0u, 0u, 0u};
	uint64_t groups = total;
	if (quarter_all == 2u) groups = total * 16u; else if (quarter_all) groups = total * 4u;
	if (sched_kind) { // 1: a schedule of this grid, 2: one sized for another grid (must be ignored), 3: without a header
		p.n_units = sched_kind == 2 ? n_units + 1u + below(3) : n_units;
		const uint32_t slots = n_units + below(n_units / 2u + 2u); // pieces take extra slots
		sched.resize(slots + 4u);
		for (auto &e : sched) {
			const uint32_t r = below(8);
			const uint32_t what = r < 4u ? 0u : (r < 5u ? 1u : (r < 7u ? 2u + below(4) : below(16)));
			const uint32_t id = below(what == 0u ? n_units + 1u : (uint32_t)(total < 0x0FFFFFFFu ? total + 1u : 0x0FFFFFFFu));
			e = what << 28 | id;
		}
		p.tile_sched = sched.data();
		hdr[2] = slots - below(2);
		p.sched_hdr = sched_kind == 3 ? nullptr : hdr;
		if (sched_kind == 3) sched.resize(p.n_units + 4u, 0u), p.tile_sched = sched.data();
		groups = (uint64_t)(slots + 2u) * unit;
	}
	if (!sample || groups < 1000u) { check_groups(p, 0u, groups + 3u, "grid"); return; }
	check_groups(p, 0u, 300u, "grid, first groups");
	check_groups(p, groups - 300u, 303u, "grid, last groups");
	for (int it = 0; it < 100; it++) check_groups(p, rnd() % (groups - 2u), 3u, "grid, anywhere");
}

} // namespace

int main()
{
	const uint32_t edge[] = {1u, 7u, 8u, 9u, 4095u, 4097u};
	// the edge widths and row counts, in every tile shape, order and quarter mode (the large ones once per mode, sampled rows)
	for (uint32_t w : edge) for (uint32_t h : edge) {
		const bool large = true; // (launches of 1000 groups and more are sampled: the first and the last groups, and groups anywhere)
		for (uint32_t k = 0u; k <= 6u; k++)
			for (uint32_t order = 0; order <= 3u; order++)
				for (uint32_t q = 0; q <= 2u; q++) one_grid(w, h, k, order, q, 1u, 0, 8u, large);
		for (uint32_t unit = 1; unit <= 3u; unit++) for (int sk = 1; sk <= 3; sk++) one_grid(w, h, 3u, below(4), 0u, unit, sk, 2u, large);
	}
	// widths whose tile counts take the super-tile and the strip orders (multiples of 16, 32 and 64 tiles), with and without a schedule
	const uint32_t wide[][2] = {{128u, 128u}, {256u, 256u}, {512u, 64u}, {512u, 256u}, {1024u, 96u}, {2048u, 40u}, {520u, 250u}};
	for (auto &wh : wide)
		for (uint32_t order = 0; order <= 3u; order++)
			for (uint32_t tgp : {0u, 1u, 2u, 3u, 4u, 8u})
				for (int sk = 0; sk <= 1; sk++) one_grid(wh[0], wh[1], 3u, order, 0u, sk ? 2u : 1u, sk, tgp);
	// random launches
	for (int it = 0; it < 1500; it++) {
		const uint32_t k = below(7), w = 1u + below(it % 8 == 0 ? 700u : 90u), h = 1u + below(it % 8 == 1 ? 500u : 70u);
		const uint32_t q = below(6) == 0u ? 1u + below(2) : 0u;
		const int sk = q == 0u && below(2) ? 1 + (int)below(3) : 0;
		one_grid(w, h, sk ? 3u : k, below(4), q, sk ? 1u + below(4) : 1u, sk, below(9));
	}
	// a tile count above 2^32: 2^17 x 2^17 tiles of 1 x 64 pixels ... the first groups, the groups around 2^32, and the last ones
	{
		Params p = {};
		p.tile_w_log2 = 0u; p.grid_w = 1u << 17; p.rows = 1u << 23; p.tiles_x = 1u << 17; // tiles_y = 2^17: 2^34 tiles
		for (uint32_t order = 0; order <= 3u; order++) {
			p.tile_order = order; p.tile_group = 8u;
			for (uint32_t q = 0; q <= 2u; q++) {
				p.quarter_all = q;
				const uint64_t total = 1ull << 34, groups = q == 2u ? total << 4 : (q ? total << 2 : total);
				check_groups(p, 0u, 300u, "2^34 tiles, first");
				check_groups(p, (1ull << 32) - 150u, 300u, "2^34 tiles, around 2^32");
				check_groups(p, groups - 150u, 300u, "2^34 tiles, last");
				for (int it = 0; it < 200; it++) check_groups(p, rnd() % groups, 3u, "2^34 tiles, anywhere");
			}
		}
		// ... and a schedule over them (units of 2^8 tiles: 2^26 units would be a large table, so one that does not match, and a
		// narrow grid with a unit above 16, which takes the wide form too)
		p.quarter_all = 0u; p.tile_order = 0u; p.tile_unit = 256u; p.n_units = 5u;
		std::vector<uint32_t> sched(8, 3u); p.tile_sched = sched.data();
		check_groups(p, (1ull << 33) - 5u, 10u, "2^34 tiles, a schedule of another grid");
		one_grid(64u, 64u, 3u, 0u, 0u, 17u, 1, 2u);
		one_grid(256u, 256u, 3u, 3u, 0u, 32u, 1, 2u);
	}
	// sched_matches against the division it replaces
	for (int it = 0; it < 200000; it++) {
		const uint64_t total = it % 3 == 0 ? rnd() >> below(64) : below(5000);
		const uint32_t unit = it % 5 == 0 ? 1u + (uint32_t)(rnd() >> (32 + below(32))) : 1u + below(40);
		const uint64_t want = (total + unit - 1u) / unit; // (no overflow: total + unit < 2^64 for the values drawn, checked next)
		if (total + unit < total) continue;
		const uint32_t cand[] = {(uint32_t)want, (uint32_t)want + 1u, (uint32_t)want - 1u, 0u, (uint32_t)rnd()};
		for (uint32_t n : cand) { checks++; if (sched_matches(total, unit, n) != (want == n)) { if (failures++ < 20) printf("FAIL sched_matches(%llu, %u, %u)\n", (unsigned long long)total, unit, n); } }
	}
	// the linear map
	for (int it = 0; it < 4000; it++) {
		Params p = {};
		p.sparse_lanes = below(3) ? 0u : 1u + below(64);
		p.count = it % 7 == 0 ? (1ull << 32) + below(300) : below(400);
		const uint64_t first = it % 7 == 0 && below(2) ? (p.count >> 6) - 3u : 0u;
		for (uint64_t group = first; group < first + 8u; group++) for (uint32_t l = 0; l < 64u; l++) {
			uint64_t er = 0, e = 0;
			const bool rv = ref_linear(p, group * 64u + l, er), v = linear_lane(group, l, p.sparse_lanes, p.count, e);
			checks++;
			if (rv != v || (rv && er != e)) { if (failures++ < 20) printf("FAIL linear: sparse %u count %llu group %llu lane %u\n", p.sparse_lanes, (unsigned long long)p.count, (unsigned long long)group, l); }
		}
	}
	if (failures) { printf("%ld of %ld checks FAIL\n", failures, checks); return 1; }
	printf("lane_map_test: %ld checks hold (the two-part map = the one-function map)\n", checks);
	return 0;
}
