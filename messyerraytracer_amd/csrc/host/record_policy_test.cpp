// record_policy_test.cpp — pins the plans of the record-driven casts (launch_policy.cpp plan_source: shadow, selected shadow, reflection,
// hemisphere, bounce and G-buffer reflection) without a device.  One table of casts and the plan each one must get, applied to every
// family in every mode it has (the plan reads neither: unsorted, non-coherent, the plain lane kernel below 2^16 rays and the persistent
// ones from 2^16, a forced packet kernel meaning the policy's lane kernel), and for every case: the plan leaves the grid states and the
// detected-grid words byte for byte as they were, is the plan of the family's sibling for as many rays, and is the plan made without a
// detected grid.  Then a renderer's frame loop -- a primary grid cast, the grid tuner's timing, the family's cast -- against the same
// loop without the family's casts: the primary grid's plans must be the same, frame by frame.
// record_policy_test <family> runs one family, record_policy_test all of them; one line per failure and one per family, the last line
// "N of M checks hold (K table cases)".  Exit status 0 iff every check holds.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../launch_policy.h"

using namespace mrt;

namespace {

int failures = 0, checks = 0;
void expect(bool ok, const std::string &what)
{
	checks++;
	if (!ok) { failures++; std::printf("FAIL %s\n", what.c_str()); }
}

const char *kname(uint32_t k)
{
	switch (k) {
		case MRT_KERNEL_LANE: return "lane";
		case MRT_KERNEL_PACKET_ASM: return "asm";
		case MRT_KERNEL_LANE_PERSISTENT: return "lp";
		case MRT_KERNEL_LANE4_PERSISTENT: return "l4p";
		case MRT_KERNEL_LANE8_PERSISTENT: return "l8p";
		case MRT_KERNEL_PACKET_DUAL: return "dual";
		case MRT_KERNEL_TWO_LEVEL: return "tl";
		case MRT_KERNEL_TWO_LEVEL_PACKET: return "tlpkt";
		case MRT_KERNEL_TWO_LEVEL_PERSISTENT: return "tlp";
		case MRT_KERNEL_TWO_LEVEL_PERSISTENT8: return "tlp8";
		default: return "?";
	}
}

// k=<kernel> <launch>(<lane launch>) [sort] [detect] [sched] [arms] n=<launches> [cnt]
std::string describe(const CastPlan &c)
{
	char b[256];
	int n = std::snprintf(b, sizeof(b), "k=%s ", kname(c.kernel));
	if (c.launch == CastPlan::PLAIN) n += std::snprintf(b + n, sizeof(b) - n, "plain");
	else {
		const LaneLaunch &l = c.lane;
		n += std::snprintf(b + n, sizeof(b) - n, "%s(%s ", c.launch == CastPlan::DUAL ? "dual" : "lane", kname(l.kernel));
		if (l.persistent) n += std::snprintf(b + n, sizeof(b) - n, "pers blocks=%u lds=%u spill=%u wait=%u", l.blocks, l.lds_depth, l.spill, l.leaf_wait);
		else n += std::snprintf(b + n, sizeof(b) - n, "sparse=%u", l.sparse_lanes);
		n += std::snprintf(b + n, sizeof(b) - n, "%s)", l.count ? " cnt" : "");
	}
	if (c.lane_map != MAP_LINEAR || c.quarter_all) n += std::snprintf(b + n, sizeof(b) - n, " map=%u q=%u", c.lane_map, c.quarter_all);
	if (c.sort) n += std::snprintf(b + n, sizeof(b) - n, " sort");
	if (c.detect) n += std::snprintf(b + n, sizeof(b) - n, " detect");
	if (c.scheduled) n += std::snprintf(b + n, sizeof(b) - n, " sched%s", c.pieces ? "+pieces" : "");
	if (c.arms_tuner) n += std::snprintf(b + n, sizeof(b) - n, " arms");
	n += std::snprintf(b + n, sizeof(b) - n, " n=%u%s", c.launches, c.count ? " cnt" : "");
	return b;
}

// scenes as in launch_policy_test.cpp: flat with every layout, without the 8-wide one, 2-wide only; two-level with / without 8-wide BLASes
enum { FLAT, NO8, BARE, TL, TL_NO8 };
SceneFacts scene(int k)
{
	SceneFacts s;
	s.rows = s.nodes4 = s.nodes8 = true; s.n_nodes = 40000; s.depth = 20; s.stack4 = 12; s.stack8 = 10;
	if (k == NO8) s.nodes8 = false;
	if (k == BARE) s.rows = s.nodes4 = s.nodes8 = false;
	if (k == TL || k == TL_NO8) { s.two_level = true; s.rows = s.nodes4 = false; s.nodes8 = k == TL; s.depth = 30; s.stack8 = 14; }
	return s;
}

mrt_options options(uint32_t kernel, uint32_t count_visits = 0)
{
	mrt_options o;
	std::memset(&o, 0, sizeof(o));
	o.struct_size = sizeof(o); o.kernel = kernel; o.count_visits = count_visits;
	return o;
}

// ---- the families ---------------------------------------------------------------------------------------------------------------------

constexpr uint64_t kPixels = 1280ull * 960ull; // the alternation loop's primary grid
enum { SHADOW, SELECTED_SHADOW, REFLECTION, HEMISPHERE, BOUNCE, GBUFFER, N_FAMILIES, NONE = -1 };
const int ANY = MRT_MODE_ANY_HIT, NEAREST = MRT_MODE_NEAREST;

// The cast after the primary grid of frame f of the alternation loop (array / grid: the family's entries).
CastRequest request(Entry entry, uint64_t count, int mode, uint32_t flags = 0u)
{
	CastRequest r;
	r.entry = entry; r.count = count; r.mode = mode; r.flags = flags;
	return r;
}
CastRequest shadow_frame(Entry array, Entry grid, int f) { return request(f & 1 ? array : grid, 2ull * kPixels, ANY); }                       // 2 lights
CastRequest selected_frame(Entry array, Entry grid, int f) { return request(f & 1 ? array : grid, kPixels, ANY); }                           // one light per record
CastRequest nearest_frame(Entry array, Entry grid, int f) { return request(f & 1 ? array : grid, kPixels, NEAREST); }
// a four-sample ambient-occlusion cast (even frames) or a diffuse bounce (odd frames)
CastRequest hemisphere_frame(Entry array, Entry grid, int f) { return request(f & 2 ? array : grid, kPixels * (f & 1 ? 1u : 4u), f & 1 ? NEAREST : ANY); }
CastRequest bounce_frame(Entry array, Entry grid, int f) { return request(f & 2 ? array : grid, kPixels, NEAREST, f & 1 ? MRT_FLAG_ASYNC : 0u); }

// One row per family: its entries (a family without an array form has the same entry twice), its modes, the family whose plan of as
// many rays it must match in each mode (NONE: shadow, which the others are held to), and its cast in the alternation loop.
struct Family { const char *name; Entry array, grid; int modes[2], n_modes, sibling[2]; CastRequest (*frame)(Entry, Entry, int); };
const Family kFamilies[N_FAMILIES] = {
	{"shadow", ENTRY_SHADOW, ENTRY_GRID_SHADOW, {ANY, 0}, 1, {NONE, NONE}, shadow_frame},
	{"selected_shadow", ENTRY_SELECTED_SHADOW, ENTRY_GRID_SELECTED_SHADOW, {ANY, 0}, 1, {SHADOW, NONE}, selected_frame},
	{"reflection", ENTRY_REFLECTION, ENTRY_GRID_REFLECTION, {NEAREST, 0}, 1, {SHADOW, NONE}, nearest_frame},
	{"hemisphere", ENTRY_HEMISPHERE, ENTRY_GRID_HEMISPHERE, {ANY, NEAREST}, 2, {SHADOW, REFLECTION}, hemisphere_frame},
	{"bounce", ENTRY_BOUNCE, ENTRY_GRID_BOUNCE, {NEAREST, 0}, 1, {REFLECTION, NONE}, bounce_frame},
	{"gbuffer", ENTRY_GBUFFER_REFLECTION, ENTRY_GBUFFER_REFLECTION, {NEAREST, 0}, 1, {REFLECTION, NONE}, nearest_frame},
};

// ---- the cases ------------------------------------------------------------------------------------------------------------------------

struct Case { const char *name; int scene; uint32_t kernel, count_visits; bool grid; uint64_t count; uint32_t flags; const char *want; };
// count = rays (pixels * lights, records, pixels * samples, pixels); grid: the case goes to the family's grid entry.  HOST_LAYOUT is
// given to an array form only.  Persistent: 16 LDS entries per lane -> 8 workgroups per CU -> 2 048 blocks (fewer for a small batch).
const Case kCases[] = {
	{"1k rays: one ray per wave", FLAT, MRT_KERNEL_AUTO, 0, false, 1000, 0, "k=lane lane(lane sparse=1) n=1"},
	{"67 x 35: one ray per wave", FLAT, MRT_KERNEL_AUTO, 0, true, 67 * 35, 0, "k=lane lane(lane sparse=1) n=1"},
	{"20k rays: four rays per wave", FLAT, MRT_KERNEL_AUTO, 0, true, 20000, 0, "k=lane lane(lane sparse=4) n=1"},
	{"40k rays: full waves", FLAT, MRT_KERNEL_AUTO, 0, false, 40000, 0, "k=lane lane(lane sparse=0) n=1"},
	{"2^16 - 1 rays: still plain", FLAT, MRT_KERNEL_AUTO, 0, true, 65535, 0, "k=lane lane(lane sparse=0) n=1"},
	{"2^16 rays: 8-wide persistent", FLAT, MRT_KERNEL_AUTO, 0, true, 65536, 0, "k=l8p lane(l8p pers blocks=256 lds=16 spill=0 wait=8) n=1"},
	{"2^20 rays, async", FLAT, MRT_KERNEL_AUTO, 0, true, 1u << 20, MRT_FLAG_ASYNC, "k=l8p lane(l8p pers blocks=2048 lds=16 spill=0 wait=8) n=0"},
	{"2^20 rays, no 8-wide nodes", NO8, MRT_KERNEL_AUTO, 0, false, 1u << 20, 0, "k=l4p lane(l4p pers blocks=2048 lds=16 spill=0 wait=16) n=1"},
	{"2^20 rays, 2-wide nodes only", BARE, MRT_KERNEL_AUTO, 0, false, 1u << 20, MRT_FLAG_HOST_LAYOUT, "k=lp lane(lp pers blocks=2048 lds=16 spill=4 wait=16) n=1"},
	{"two-level, 1k rays", TL, MRT_KERNEL_AUTO, 0, true, 1000, 0, "k=tl lane(tl sparse=1) n=1"},
	{"two-level, 2^20 rays", TL, MRT_KERNEL_AUTO, 0, true, 1u << 20, 0, "k=tlp8 lane(tlp8 pers blocks=2048 lds=16 spill=0 wait=8) n=1"},
	{"two-level without 8-wide BLASes", TL_NO8, MRT_KERNEL_AUTO, 0, false, 1u << 20, 0, "k=tlp lane(tlp pers blocks=2048 lds=16 spill=14 wait=16) n=1"},
	{"forced 64-ray packets: the policy's lane kernel", FLAT, MRT_KERNEL_PACKET_ASM, 0, true, 1u << 20, 0, "k=l8p lane(l8p pers blocks=2048 lds=16 spill=0 wait=8) n=1"},
	{"forced 128-ray walk, small", FLAT, MRT_KERNEL_PACKET_DUAL, 0, false, 1000, 0, "k=lane lane(lane sparse=1) n=1"},
	{"forced generic packets", FLAT, MRT_KERNEL_PACKET, 0, false, 40000, 0, "k=lane lane(lane sparse=0) n=1"},
	{"forced packets, two-level", TL, MRT_KERNEL_PACKET_ASM, 0, true, 1u << 20, 0, "k=tlp8 lane(tlp8 pers blocks=2048 lds=16 spill=0 wait=8) n=1"},
	{"forced lane kernel", FLAT, MRT_KERNEL_LANE, 0, true, 1u << 20, 0, "k=lane lane(lane sparse=0) n=1"},
	{"forced 4-wide persistent, small", FLAT, MRT_KERNEL_LANE4_PERSISTENT, 0, false, 1000, 0, "k=l4p lane(l4p pers blocks=4 lds=16 spill=0 wait=16) n=1"},
	{"forced 8-wide persistent", FLAT, MRT_KERNEL_LANE8_PERSISTENT, 0, false, 40000, 0, "k=l8p lane(l8p pers blocks=157 lds=16 spill=0 wait=8) n=1"},
	{"counting build: no counting variant", FLAT, MRT_KERNEL_AUTO, 1, true, 1u << 20, 0, "k=l8p lane(l8p pers blocks=2048 lds=16 spill=0 wait=8) n=1"},
	{"counting build, small", FLAT, MRT_KERNEL_AUTO, 1, false, 1000, 0, "k=lane lane(lane sparse=1) n=1"},
	{"counting build, two-level", TL, MRT_KERNEL_AUTO, 1, true, 1u << 20, 0, "k=tlp8 lane(tlp8 pers blocks=2048 lds=16 spill=0 wait=8) n=1"},
};

std::vector<unsigned char> bytes_of(const GridStates &gs)
{
	std::vector<unsigned char> b(sizeof(GridStates));
	std::memcpy(b.data(), &gs, sizeof(gs));
	return b;
}

void table(const Family &f)
{
	expect(record_cast_entry(f.array) && !ray_entry(f.array) && record_cast_entry(f.grid) && !ray_entry(f.grid), std::string(f.name) + ": the entries go through plan_source");
	for (const Case &k : kCases) for (int m = 0; m < f.n_modes; m++) {
		const int mode = f.modes[m];
		const std::string name = std::string(f.name) + ", " + k.name + (mode == ANY ? " (any-hit)" : " (closest-hit)");
		const mrt_options o = options(k.kernel, k.count_visits);
		GridStates gs;
		PrevDetect prev;   // a detected grid of as many rays: the plan must not take it
		prev.count = k.count; prev.word[0] = 1024; prev.word[1] = (uint32_t)(k.count / 1024u); prev.word[2] = 128; prev.word[3] = 0;
		const PrevDetect prev_before = prev;
		const bool array_form = !k.grid && f.array != f.grid;
		const CastRequest r = request(k.grid ? f.grid : f.array, k.count, mode, array_form ? k.flags : k.flags & ~(uint32_t)MRT_FLAG_HOST_LAYOUT);
		const std::vector<unsigned char> before = bytes_of(gs);
		const CastPlan c = plan_cast(o, scene(k.scene), r, prev, Knobs(), gs);
		const std::string got = describe(c);
		expect(got == k.want, name + ": got \"" + got + "\", want \"" + k.want + "\"");
		expect(before == bytes_of(gs), name + ": the plan changed the grid states");
		expect(prev.count == prev_before.count && std::memcmp(prev.word, prev_before.word, sizeof(prev.word)) == 0, name + ": the plan changed the detected-grid words");
		expect(!c.sort && !c.detect && !c.scheduled && !c.arms_tuner && !c.count && c.lane_map == MAP_LINEAR && c.quarter_all == 0u,
				name + ": not an unsorted, untiled, non-counting plan: " + got);
		// the plan of the sibling's cast of as many rays (the mode does not enter it), and the same plan whatever was detected before
		if (f.sibling[m] != NONE) {
			const Family &s = kFamilies[f.sibling[m]];
			CastRequest sr = r;
			sr.entry = k.grid ? s.grid : s.array; sr.mode = s.modes[0];
			const std::string sibling = describe(plan_cast(o, scene(k.scene), sr, prev, Knobs(), gs));
			expect(got == sibling, name + ": plan \"" + got + "\", " + s.name + " plan \"" + sibling + "\"");
		}
		const std::string blind = describe(plan_cast(o, scene(k.scene), r, PrevDetect(), Knobs(), gs));
		expect(got == blind, name + ": plan \"" + got + "\" with a detected grid, \"" + blind + "\" without");
	}
}

// A renderer's frame: the primary grid (blocking, so the grid tuner times it), then, if `with`, the family's cast of the grid's records.
// The primary plans of 14 frames must not depend on the casts between them.
std::vector<std::string> frames(const Family &f, int scn, bool with)
{
	GridStates gs;
	const mrt_options o = options(MRT_KERNEL_AUTO);
	std::vector<std::string> out;
	const float ms[14] = {0.50f, 0.48f, 0.47f, 0.46f, 0.45f, 0.44f, 0.40f, 0.41f, 0.43f, 0.42f, 0.44f, 0.45f, 0.40f, 0.40f};
	for (int fr = 0; fr < 14; fr++) {
		CastRequest g = request(ENTRY_GRID, kPixels, NEAREST);
		g.grid_w = 1280; g.grid_h = 960; g.y0 = 0; g.rows = 960;
		out.push_back(describe(plan_cast(o, scene(scn), g, PrevDetect(), Knobs(), gs)));
		tune_record(gs.tune(), ms[fr]);
		if (!with) continue;
		const std::vector<unsigned char> before = bytes_of(gs);
		const CastPlan sc = plan_cast(o, scene(scn), f.frame(f.array, f.grid, fr), PrevDetect(), Knobs(), gs);
		const std::string name = std::string(f.name) + ", frame " + std::to_string(fr);
		expect(before == bytes_of(gs), name + ": the family's plan changed the grid states");
		expect(!sc.sort && !sc.detect && !sc.scheduled && !sc.arms_tuner && sc.lane_map == MAP_LINEAR, name + ": plan " + describe(sc));
	}
	return out;
}

void alternation(const Family &f)
{
	for (int scn : {FLAT, TL}) {
		const std::vector<std::string> a = frames(f, scn, false), b = frames(f, scn, true);
		for (size_t fr = 0; fr < a.size(); fr++)
			expect(a[fr] == b[fr], std::string(f.name) + ", scene " + std::to_string(scn) + " frame " + std::to_string(fr) + ": primary plan \"" + b[fr] + "\" with the family's casts, \"" + a[fr] + "\" without");
		if (scn == FLAT) { // (the tuner does run here: its three candidates over the first twelve frames)
			bool dual = false, asm_ = false;
			for (const std::string &d : a) { dual |= d.rfind("k=dual", 0) == 0; asm_ |= d.rfind("k=asm", 0) == 0; }
			expect(dual && asm_, std::string(f.name) + ", flat scene: the grid tuner tried both packet kernels");
		}
	}
}

// G-buffer: where the entry stands, and the label of every form the family has (format_variant, as launch_source calls it for a
// family with one mode)
void gbuffer_extras()
{
	expect(ENTRY_GBUFFER_REFLECTION == ENTRY_GRID_BOUNCE + 1, "gbuffer: the entry is appended after the bounce entries");
	struct L { TraceKernel k; int width; bool tl; const char *want; };
	const L kLabels[] = {
		{TraceKernel::LANE, 2, false, "trace_gbuffer_lane_kernel<13>"},
		{TraceKernel::TWO_LEVEL, 2, true, "trace_gbuffer_two_level_kernel<13>"},
		{TraceKernel::LANE_PERSISTENT, 2, false, "trace_gbuffer_persistent_kernel<13, 2, false>"},
		{TraceKernel::LANE_PERSISTENT, 4, false, "trace_gbuffer_persistent_kernel<13, 4, false>"},
		{TraceKernel::LANE_PERSISTENT, 8, false, "trace_gbuffer_persistent_kernel<13, 8, false>"},
		{TraceKernel::LANE_PERSISTENT, 2, true, "trace_gbuffer_persistent_kernel<13, 2, true>"},
		{TraceKernel::LANE_PERSISTENT, 8, true, "trace_gbuffer_persistent_kernel<13, 8, true>"},
	};
	for (const L &l : kLabels) {
		TraceVariant v;
		v.kernel = l.k; v.width = l.width; v.two_level = l.tl;
		char b[96];
		format_variant(b, sizeof(b), v, SourceFamily<GBufferParams>::name, SRC_GBUFFER, SourceFamily<GBufferParams>::any_hit && SourceFamily<GBufferParams>::nearest);
		expect(std::string(b) == l.want, std::string("gbuffer label: got \"") + b + "\", want \"" + l.want + "\"");
	}
}

} // namespace

int main(int argc, char **argv)
{
	const size_t n_cases = sizeof(kCases) / sizeof(kCases[0]);
	int ran = 0;
	for (int i = 0; i < N_FAMILIES; i++) {
		const Family &f = kFamilies[i];
		if (argc > 1 && std::strcmp(argv[1], f.name) != 0) continue;
		const int checks0 = checks, failures0 = failures;
		table(f);
		alternation(f);
		if (i == GBUFFER) gbuffer_extras();
		std::printf("%s: %d of %d checks hold (%zu table cases)\n", f.name, (checks - checks0) - (failures - failures0), checks - checks0, n_cases);
		ran++;
	}
	if (!ran) { std::printf("FAIL no family named \"%s\"\n", argv[1]); return 2; }
	if (ran > 1) std::printf("%d of %d checks hold (%zu table cases)\n", checks - failures, checks, n_cases);
	return failures ? 1 : 0;
}
