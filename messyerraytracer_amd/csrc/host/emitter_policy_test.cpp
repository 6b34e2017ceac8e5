// emitter_policy_test.cpp — pins the plans of the emitter-shadow casts (launch_policy.cpp plan_source: ENTRY_EMITTER_SHADOW and
// ENTRY_GRID_EMITTER_SHADOW) without a device: for every scene kind of record_policy_test.cpp's table, every kernel a context may
// force, with and without the counting option, blocking and ASYNC, and a ladder of record counts around every bound of the policy, the
// two entries get ENTRY_SELECTED_SHADOW's plan for as many records, field for field; the plan leaves the grid states as they were; the
// entries stand after the selected-shadow entries; the labels of the family's forms.
// One line per failure, the last line "N of M checks hold (K plans)".  Exit status 0 iff every check holds.
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
	if (!ok) { failures++; if (failures <= 40) std::printf("FAIL %s\n", what.c_str()); }
}

// scenes as in record_policy_test.cpp: flat with every layout, without the 8-wide one, 2-wide only; two-level with / without 8-wide BLASes
enum { FLAT, NO8, BARE, TL, TL_NO8, N_SCENES };
SceneFacts scene(int k)
{
	SceneFacts s;
	s.rows = s.nodes4 = s.nodes8 = true; s.n_nodes = 40000; s.depth = 20; s.stack4 = 12; s.stack8 = 10;
	if (k == NO8) s.nodes8 = false;
	if (k == BARE) s.rows = s.nodes4 = s.nodes8 = false;
	if (k == TL || k == TL_NO8) { s.two_level = true; s.rows = s.nodes4 = false; s.nodes8 = k == TL; s.depth = 30; s.stack8 = 14; }
	return s;
}

bool same_lane(const LaneLaunch &a, const LaneLaunch &b)
{
	return a.persistent == b.persistent && a.kernel == b.kernel && a.sparse_lanes == b.sparse_lanes && a.lds_depth == b.lds_depth &&
			a.blocks == b.blocks && a.spill == b.spill && a.refill == b.refill && a.leaf_wait == b.leaf_wait && a.count == b.count;
}
bool same_plan(const CastPlan &a, const CastPlan &b)
{
	return a.sort == b.sort && a.detect == b.detect && a.kernel == b.kernel && a.lane_map == b.lane_map && a.quarter_all == b.quarter_all &&
			a.launch == b.launch && a.count == b.count && same_lane(a.lane, b.lane) && a.scheduled == b.scheduled && a.grid_w == b.grid_w &&
			a.grid_h == b.grid_h && a.y0 == b.y0 && a.rows == b.rows && a.tiles_x == b.tiles_x && a.pieces == b.pieces &&
			a.wait_sorts == b.wait_sorts && a.arms_tuner == b.arms_tuner && a.launches == b.launches;
}

} // namespace

int main()
{
	expect(ENTRY_EMITTER_SHADOW == ENTRY_GRID_SELECTED_SHADOW + 1 && ENTRY_GRID_EMITTER_SHADOW == ENTRY_EMITTER_SHADOW + 1,
			"the entries are appended after the selected-shadow entries");
	for (Entry e : {ENTRY_EMITTER_SHADOW, ENTRY_GRID_EMITTER_SHADOW})
		expect(record_cast_entry(e) && !ray_entry(e), "the entries go through plan_source");
	const uint32_t kernels[] = {MRT_KERNEL_AUTO, MRT_KERNEL_LANE, MRT_KERNEL_PACKET, MRT_KERNEL_PACKET_ASM, MRT_KERNEL_LANE_PERSISTENT,
		MRT_KERNEL_LANE4_PERSISTENT, MRT_KERNEL_LANE8_PERSISTENT, MRT_KERNEL_PACKET_DUAL, MRT_KERNEL_PACKET_ROWS, MRT_KERNEL_PACKET_QUAD};
	const uint64_t counts[] = {1, 63, 64, 65, 1000, 8192, 8193, 16384, 16385, 20000, 32768, 32769, 40000, 65535, 65536, 65537, 77000,
		1u << 20, 1920ull * 1080ull, (1ull << 32) + 5u};
	int plans = 0;
	for (int scn = 0; scn < N_SCENES; scn++) for (uint32_t kernel : kernels) for (uint32_t cv : {0u, 1u}) for (uint32_t fl : {0u, (uint32_t)MRT_FLAG_ASYNC})
		for (uint64_t n : counts) for (int grid = 0; grid < 2; grid++) {
			mrt_options o;
			std::memset(&o, 0, sizeof(o));
			o.struct_size = sizeof(o); o.kernel = kernel; o.count_visits = cv;
			CastRequest r;
			r.count = n; r.mode = MRT_MODE_ANY_HIT; r.flags = fl | (grid ? 0u : (uint32_t)MRT_FLAG_HOST_LAYOUT);
			GridStates gs;
			std::vector<unsigned char> before(sizeof(gs));
			std::memcpy(before.data(), &gs, sizeof(gs));
			r.entry = grid ? ENTRY_GRID_EMITTER_SHADOW : ENTRY_EMITTER_SHADOW;
			const CastPlan mine = plan_cast(o, scene(scn), r, PrevDetect(), Knobs(), gs);
			expect(std::memcmp(before.data(), &gs, sizeof(gs)) == 0, "the plan changed the grid states");
			r.entry = grid ? ENTRY_GRID_SELECTED_SHADOW : ENTRY_SELECTED_SHADOW;
			const CastPlan theirs = plan_cast(o, scene(scn), r, PrevDetect(), Knobs(), gs);
			plans++;
			expect(same_plan(mine, theirs), "scene " + std::to_string(scn) + " kernel " + std::to_string(kernel) + " count_visits " + std::to_string(cv) +
					" flags " + std::to_string(fl) + " records " + std::to_string(n) + (grid ? " grid" : " array") + ": not the selected-shadow cast's plan");
			expect(mine.launch == CastPlan::LANE && !mine.sort && !mine.detect && !mine.scheduled && !mine.count && mine.lane_map == MAP_LINEAR,
					"not an unsorted, untiled, non-counting lane plan");
		}
	// the labels of the family's forms (format_variant, as launch_source calls it for a family with one mode)
	struct L { TraceKernel k; int width; bool tl; int src; const char *want; };
	const L kLabels[] = {
		{TraceKernel::LANE, 2, false, SRC_EMITSHADOW_RAY32, "trace_emitter_shadow_lane_kernel<17>"},
		{TraceKernel::LANE, 2, false, SRC_EMITSHADOW_HOST44, "trace_emitter_shadow_lane_kernel<18>"},
		{TraceKernel::TWO_LEVEL, 2, true, SRC_EMITSHADOW_GRID, "trace_emitter_shadow_two_level_kernel<19>"},
		{TraceKernel::LANE_PERSISTENT, 2, false, SRC_EMITSHADOW_RAY32, "trace_emitter_shadow_persistent_kernel<17, 2, false>"},
		{TraceKernel::LANE_PERSISTENT, 4, false, SRC_EMITSHADOW_RAY32, "trace_emitter_shadow_persistent_kernel<17, 4, false>"},
		{TraceKernel::LANE_PERSISTENT, 8, false, SRC_EMITSHADOW_GRID, "trace_emitter_shadow_persistent_kernel<19, 8, false>"},
		{TraceKernel::LANE_PERSISTENT, 2, true, SRC_EMITSHADOW_RAY32, "trace_emitter_shadow_persistent_kernel<17, 2, true>"},
		{TraceKernel::LANE_PERSISTENT, 8, true, SRC_EMITSHADOW_GRID, "trace_emitter_shadow_persistent_kernel<19, 8, true>"},
	};
	using Fam = SourceFamily<EmitterShadowParams>;
	expect(Fam::any_hit && !Fam::nearest && Fam::ray32 == SRC_EMITSHADOW_RAY32 && Fam::host == SRC_EMITSHADOW_HOST44 && Fam::grid == SRC_EMITSHADOW_GRID,
			"the family: any-hit, its three sources");
	expect(SRC_EMITSHADOW_RAY32 == SRC_SELSHADOW_GRID + 1, "the sources are appended after the selected-shadow sources");
	for (int src = 0; src <= SRC_EMITSHADOW_GRID; src++)
		expect(lit_output(src, true) == (shadow_source(src) || selected_shadow_source(src) || hemisphere_source(src) || emitter_shadow_source(src)),
				"lit_output of source " + std::to_string(src));
	for (const L &l : kLabels) {
		TraceVariant v;
		v.kernel = l.k; v.width = l.width; v.two_level = l.tl; v.any_hit = true;
		char b[96];
		format_variant(b, sizeof(b), v, Fam::name, l.src, Fam::any_hit && Fam::nearest);
		expect(std::string(b) == l.want, std::string("label: got \"") + b + "\", want \"" + l.want + "\"");
	}
	std::printf("%d of %d checks hold (%d plans)\n", checks - failures, checks, plans);
	return failures ? 1 : 0;
}
