// record_policy_test.h — what the four policy tests of record-driven casts share (shadow_policy_test.cpp, reflection_policy_test.cpp,
// hemisphere_policy_test.cpp, bounce_policy_test.cpp): the check counter, a plan written as one line, the scenes and the options.
// Each test keeps its own case table and alternation loop.
#pragma once
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

} // namespace
