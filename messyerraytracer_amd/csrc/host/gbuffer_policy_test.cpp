// gbuffer_policy_test.cpp — pins the plans of G-buffer reflection casts (launch_policy.cpp, ENTRY_GBUFFER_REFLECTION) without a device:
// a table of casts and the plan each one must get (the same as a reflection cast of as many rays: unsorted, non-coherent, the plain
// lane kernel below 2^16 pixels and the persistent ones from 2^16), then a hybrid renderer's frame loop -- a primary grid cast, the grid
// tuner's timing, a G-buffer cast -- against the same loop without the G-buffer casts: the primary grid's plans must be the same, frame
// by frame, and a G-buffer plan must leave the grid states byte for byte as they were.  Exit status 0 iff every check holds; one line
// per failure.
#include "record_policy_test.h"

namespace {

struct Case { const char *name; int scene; uint32_t kernel, count_visits; uint64_t count; uint32_t flags; const char *want; };
// count = pixels.  Persistent: 16 LDS entries per lane -> 8 workgroups per CU -> 2 048 blocks (fewer for a small frame).
const Case kCases[] = {
	{"1k pixels: one ray per wave", FLAT, MRT_KERNEL_AUTO, 0, 1000, 0, "k=lane lane(lane sparse=1) n=1"},
	{"67 x 35: one ray per wave", FLAT, MRT_KERNEL_AUTO, 0, 67 * 35, 0, "k=lane lane(lane sparse=1) n=1"},
	{"20k pixels: four rays per wave", FLAT, MRT_KERNEL_AUTO, 0, 20000, 0, "k=lane lane(lane sparse=4) n=1"},
	{"40k pixels: full waves", FLAT, MRT_KERNEL_AUTO, 0, 40000, 0, "k=lane lane(lane sparse=0) n=1"},
	{"2^16 - 1 pixels: still plain", FLAT, MRT_KERNEL_AUTO, 0, 65535, 0, "k=lane lane(lane sparse=0) n=1"},
	{"2^16 pixels: 8-wide persistent", FLAT, MRT_KERNEL_AUTO, 0, 65536, 0, "k=l8p lane(l8p pers blocks=256 lds=16 spill=0 wait=8) n=1"},
	{"2^20 pixels, async", FLAT, MRT_KERNEL_AUTO, 0, 1u << 20, MRT_FLAG_ASYNC, "k=l8p lane(l8p pers blocks=2048 lds=16 spill=0 wait=8) n=0"},
	{"2^20 pixels, no 8-wide nodes", NO8, MRT_KERNEL_AUTO, 0, 1u << 20, 0, "k=l4p lane(l4p pers blocks=2048 lds=16 spill=0 wait=16) n=1"},
	{"2^20 pixels, 2-wide nodes only", BARE, MRT_KERNEL_AUTO, 0, 1u << 20, 0, "k=lp lane(lp pers blocks=2048 lds=16 spill=4 wait=16) n=1"},
	{"two-level, 1k pixels", TL, MRT_KERNEL_AUTO, 0, 1000, 0, "k=tl lane(tl sparse=1) n=1"},
	{"two-level, 2^20 pixels", TL, MRT_KERNEL_AUTO, 0, 1u << 20, 0, "k=tlp8 lane(tlp8 pers blocks=2048 lds=16 spill=0 wait=8) n=1"},
	{"two-level without 8-wide BLASes", TL_NO8, MRT_KERNEL_AUTO, 0, 1u << 20, 0, "k=tlp lane(tlp pers blocks=2048 lds=16 spill=14 wait=16) n=1"},
	{"forced 64-ray packets: the policy's lane kernel", FLAT, MRT_KERNEL_PACKET_ASM, 0, 1u << 20, 0, "k=l8p lane(l8p pers blocks=2048 lds=16 spill=0 wait=8) n=1"},
	{"forced 128-ray walk, small", FLAT, MRT_KERNEL_PACKET_DUAL, 0, 1000, 0, "k=lane lane(lane sparse=1) n=1"},
	{"forced generic packets", FLAT, MRT_KERNEL_PACKET, 0, 40000, 0, "k=lane lane(lane sparse=0) n=1"},
	{"forced packets, two-level", TL, MRT_KERNEL_PACKET_ASM, 0, 1u << 20, 0, "k=tlp8 lane(tlp8 pers blocks=2048 lds=16 spill=0 wait=8) n=1"},
	{"forced lane kernel", FLAT, MRT_KERNEL_LANE, 0, 1u << 20, 0, "k=lane lane(lane sparse=0) n=1"},
	{"forced 4-wide persistent, small", FLAT, MRT_KERNEL_LANE4_PERSISTENT, 0, 1000, 0, "k=l4p lane(l4p pers blocks=4 lds=16 spill=0 wait=16) n=1"},
	{"forced 8-wide persistent", FLAT, MRT_KERNEL_LANE8_PERSISTENT, 0, 40000, 0, "k=l8p lane(l8p pers blocks=157 lds=16 spill=0 wait=8) n=1"},
	{"counting build: no counting variant", FLAT, MRT_KERNEL_AUTO, 1, 1u << 20, 0, "k=l8p lane(l8p pers blocks=2048 lds=16 spill=0 wait=8) n=1"},
	{"counting build, small", FLAT, MRT_KERNEL_AUTO, 1, 1000, 0, "k=lane lane(lane sparse=1) n=1"},
	{"counting build, two-level", TL, MRT_KERNEL_AUTO, 1, 1u << 20, 0, "k=tlp8 lane(tlp8 pers blocks=2048 lds=16 spill=0 wait=8) n=1"},
};

void table()
{
	expect(record_cast_entry(ENTRY_GBUFFER_REFLECTION) && !ray_entry(ENTRY_GBUFFER_REFLECTION), "the entry goes through plan_source");
	expect(ENTRY_GBUFFER_REFLECTION == ENTRY_GRID_BOUNCE + 1, "the entry is appended after the existing ones");
	for (const Case &k : kCases) {
		GridStates gs;
		PrevDetect prev;   // a detected grid of as many rays: a G-buffer plan must not take it
		prev.count = k.count; prev.word[0] = 1024; prev.word[1] = (uint32_t)(k.count / 1024u); prev.word[2] = 128; prev.word[3] = 0;
		CastRequest r;
		r.entry = ENTRY_GBUFFER_REFLECTION; r.count = k.count; r.flags = k.flags; r.mode = MRT_MODE_NEAREST;
		std::vector<unsigned char> before(sizeof(GridStates)), after(sizeof(GridStates));
		std::memcpy(before.data(), &gs, sizeof(gs));
		const CastPlan c = plan_cast(options(k.kernel, k.count_visits), scene(k.scene), r, prev, Knobs(), gs);
		std::memcpy(after.data(), &gs, sizeof(gs));
		const std::string got = describe(c);
		expect(got == k.want, std::string(k.name) + ": got \"" + got + "\", want \"" + k.want + "\"");
		expect(before == after, std::string(k.name) + ": the plan changed the grid states");
		expect(!c.sort && !c.detect && !c.scheduled && !c.arms_tuner && !c.count && c.lane_map == MAP_LINEAR && c.quarter_all == 0u,
				std::string(k.name) + ": not an unsorted, untiled, non-counting plan: " + got);
		// the same plan as a reflection cast of as many records
		CastRequest rr = r;
		rr.entry = ENTRY_REFLECTION;
		const std::string reflection = describe(plan_cast(options(k.kernel, k.count_visits), scene(k.scene), rr, prev, Knobs(), gs));
		expect(got == reflection, std::string(k.name) + ": G-buffer plan \"" + got + "\", reflection plan \"" + reflection + "\"");
	}
}

// A hybrid renderer's frame: the primary grid (blocking, so the grid tuner times it), then, if `gbuffer`, a G-buffer cast of as many
// pixels.  The primary plans of 14 frames must not depend on the G-buffer casts between them.
std::vector<std::string> frames(int scn, bool gbuffer)
{
	GridStates gs;
	const mrt_options o = options(MRT_KERNEL_AUTO);
	std::vector<std::string> out;
	const float ms[14] = {0.50f, 0.48f, 0.47f, 0.46f, 0.45f, 0.44f, 0.40f, 0.41f, 0.43f, 0.42f, 0.44f, 0.45f, 0.40f, 0.40f};
	for (int f = 0; f < 14; f++) {
		CastRequest g;
		g.entry = ENTRY_GRID; g.count = 1280ull * 960ull; g.mode = MRT_MODE_NEAREST;
		g.grid_w = 1280; g.grid_h = 960; g.y0 = 0; g.rows = 960;
		const CastPlan c = plan_cast(o, scene(scn), g, PrevDetect(), Knobs(), gs);
		out.push_back(describe(c));
		tune_record(gs.tune(), ms[f]);
		if (!gbuffer) continue;
		std::vector<unsigned char> before(sizeof(GridStates)), after(sizeof(GridStates));
		std::memcpy(before.data(), &gs, sizeof(gs));
		CastRequest s;
		s.entry = ENTRY_GBUFFER_REFLECTION; s.count = 1280ull * 960ull; s.mode = MRT_MODE_NEAREST;
		const CastPlan sc = plan_cast(o, scene(scn), s, PrevDetect(), Knobs(), gs);
		std::memcpy(after.data(), &gs, sizeof(gs));
		expect(before == after, "frame " + std::to_string(f) + ": a G-buffer plan changed the grid states");
		expect(!sc.sort && !sc.detect && !sc.scheduled && !sc.arms_tuner && sc.lane_map == MAP_LINEAR, "frame " + std::to_string(f) + ": G-buffer plan " + describe(sc));
	}
	return out;
}

void alternation()
{
	for (int scn : {FLAT, TL}) {
		const std::vector<std::string> a = frames(scn, false), b = frames(scn, true);
		for (size_t f = 0; f < a.size(); f++)
			expect(a[f] == b[f], "scene " + std::to_string(scn) + " frame " + std::to_string(f) + ": primary plan \"" + b[f] + "\" with G-buffer casts, \"" + a[f] + "\" without");
		if (scn == FLAT) { // (the tuner does run here: its three candidates over the first twelve frames)
			bool dual = false, asm_ = false;
			for (const std::string &d : a) { dual |= d.rfind("k=dual", 0) == 0; asm_ |= d.rfind("k=asm", 0) == 0; }
			expect(dual && asm_, "flat scene: the grid tuner tried both packet kernels");
		}
	}
}

// the label of every form the family has (format_variant, as launch_source calls it for a family with one mode)
void labels()
{
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
		expect(std::string(b) == l.want, std::string("label: got \"") + b + "\", want \"" + l.want + "\"");
	}
}

} // namespace

int main()
{
	table();
	alternation();
	labels();
	std::printf("%d of %d checks hold (%zu table cases)\n", checks - failures, checks, sizeof(kCases) / sizeof(kCases[0]));
	return failures ? 1 : 0;
}
