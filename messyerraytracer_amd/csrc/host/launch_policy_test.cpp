// launch_policy_test.cpp — pins the cast launch policy (launch_policy.cpp) without a device: a table of casts, the plan each one
// must get and what that plan runs (the instantiation's name and its launch geometry, resolve_trace / resolve_persistent), a second
// table of hand-made TraceParams on both sides of every branch the resolvers have, the labels of record-driven casts, then the
// grid kernel tuner over fifteen frames with fake timings, the per-grid state LRU and the detected width across sequences of
// blocking, ASYNC, pipelined and submitted casts (DetectMemo).
// Exit status 0 iff every check holds; one line per failure.
#include <array>
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
		case MRT_KERNEL_PACKET_ROWS: return "rows";
		case MRT_KERNEL_PACKET_QUAD: return "quad";
		case MRT_KERNEL_TWO_LEVEL: return "tl";
		case MRT_KERNEL_TWO_LEVEL_PACKET: return "tlpkt";
		case MRT_KERNEL_TWO_LEVEL_PERSISTENT: return "tlp";
		case MRT_KERNEL_TWO_LEVEL_PERSISTENT8: return "tlp8";
		default: return "?";
	}
}

// one line per plan: k=<kernel> map=<lanes> q=<quarter_all> <launch>(<lane launch>) [sort] [detect] [sched=WxR/tiles_x[+pieces][+wait]] [arms] n=<launches> [cnt]
std::string describe(const CastPlan &c)
{
	static const char *maps[] = {"lin", "tile", "auto"};
	char b[256];
	int n = std::snprintf(b, sizeof(b), "k=%s map=%s q=%u ", kname(c.kernel), maps[c.lane_map], c.quarter_all);
	if (c.launch == CastPlan::PLAIN) n += std::snprintf(b + n, sizeof(b) - n, "plain");
	else {
		const LaneLaunch &l = c.lane;
		n += std::snprintf(b + n, sizeof(b) - n, "%s(%s ", c.launch == CastPlan::DUAL ? "dual" : "lane", kname(l.kernel));
		if (l.persistent) n += std::snprintf(b + n, sizeof(b) - n, "pers blocks=%u lds=%u spill=%u wait=%u", l.blocks, l.lds_depth, l.spill, l.leaf_wait);
		else n += std::snprintf(b + n, sizeof(b) - n, "sparse=%u", l.sparse_lanes);
		n += std::snprintf(b + n, sizeof(b) - n, "%s)", l.count ? " cnt" : "");
	}
	if (c.sort) n += std::snprintf(b + n, sizeof(b) - n, " sort");
	if (c.detect) n += std::snprintf(b + n, sizeof(b) - n, " detect");
	if (c.scheduled) n += std::snprintf(b + n, sizeof(b) - n, " sched=%ux%u/%u%s%s", c.grid_w, c.rows, c.tiles_x, c.pieces ? "+pieces" : "", c.wait_sorts ? "+wait" : "");
	if (c.arms_tuner) n += std::snprintf(b + n, sizeof(b) - n, " arms");
	n += std::snprintf(b + n, sizeof(b) - n, " n=%u%s", c.launches, c.count ? " cnt" : "");
	return b;
}

// scenes: a flat one with every layout, without the row array, with nothing but the 2-wide nodes, with 2-wide nodes only
// and no 8-wide ones, past the 32-bit node offsets of the hand-written loop; two-level with and without 8-wide BLASes
enum { FLAT, NO_ROWS, BARE, NO8, BIG, TL, TL_NO8 };
SceneFacts scene(int k)
{
	SceneFacts s;
	s.rows = s.nodes4 = s.nodes8 = true; s.n_nodes = 40000; s.depth = 20; s.stack4 = 12; s.stack8 = 10;
	if (k == NO_ROWS) s.rows = false;
	if (k == BARE) s.rows = s.nodes4 = s.nodes8 = false;
	if (k == NO8) s.nodes8 = false;
	if (k == BIG) { s.rows = false; s.n_nodes = kAsmNodeLimit; }
	if (k == TL || k == TL_NO8) { s.two_level = true; s.rows = s.nodes4 = false; s.nodes8 = k == TL; s.depth = 30; s.stack8 = 14; }
	return s;
}

struct Opt { uint32_t kernel = MRT_KERNEL_AUTO, count_visits = 0, grid_tile = 0, tile_schedule = 0, tile_w_log2 = 0, stack_override = 0; };
mrt_options options(const Opt &x)
{
	mrt_options o;
	std::memset(&o, 0, sizeof(o));
	o.struct_size = sizeof(o);
	o.kernel = x.kernel; o.count_visits = x.count_visits; o.grid_tile = x.grid_tile; o.tile_schedule = x.tile_schedule;
	o.tile_w_log2 = x.tile_w_log2; o.stack_override = x.stack_override;
	return o;
}

enum { NONE, SAME, OTHER_COUNT, INCOHERENT, PENDING, NO_WIDTH }; // the previous detect
struct Case {
	const char *name;
	Opt opt;
	int scene;
	Entry entry;
	uint64_t count;   // rays of an array cast; ignored for grids (w x rows)
	uint32_t flags;
	uint32_t w, h, y0, rows; // grids; for a previous detect (array casts): what it found, {w, h, w / 8}
	int prev;
	const char *want;
	const char *runs; // what launch_planned puts on the stream for the plan: runs()
};

constexpr uint32_t COH = MRT_FLAG_COHERENT, FORCE = MRT_FLAG_FORCE_SORT, ASYNC = MRT_FLAG_ASYNC | MRT_FLAG_RAYS_ON_DEVICE | MRT_FLAG_HITS_ON_DEVICE;
constexpr uint32_t HOST = MRT_FLAG_HOST_LAYOUT, TOKEN = MRT_FLAG_TOKEN_OUT, BOOL = MRT_FLAG_BOOL_OUT;
const Opt AUTO{};
Opt kernel(uint32_t k) { Opt o; o.kernel = k; return o; }
Opt with(Opt o, uint32_t Opt::*f, uint32_t v) { o.*f = v; return o; }

const Case kCases[] = {
	// ---- rays from an array, not declared coherent: the lane kernels; a sort from 256 rays unless one ray per wave (<= 8 192 rays)
	{"incoherent 1", AUTO, FLAT, ENTRY_CAST, 1, 0, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) n=1",
		"trace_lane_kernel<false, false> 1x256 lds=24576"},
	{"incoherent 63", AUTO, FLAT, ENTRY_CAST, 63, 0, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) n=1",
		"trace_lane_kernel<false, false> 16x256 lds=24576"},
	{"incoherent 255", AUTO, FLAT, ENTRY_CAST, 255, 0, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) n=1",
		"trace_lane_kernel<false, false> 64x256 lds=24576"},
	{"incoherent 256", AUTO, FLAT, ENTRY_CAST, 256, 0, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) n=1",
		"trace_lane_kernel<false, false> 64x256 lds=24576"},
	{"incoherent 8192", AUTO, FLAT, ENTRY_CAST, 8192, 0, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) n=1",
		"trace_lane_kernel<false, false> 2048x256 lds=24576"},
	{"incoherent 8193", AUTO, FLAT, ENTRY_CAST, 8193, 0, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=2) sort n=3",
		"trace_lane_kernel<false, false> 1025x256 lds=24576"},
	{"incoherent 2^15-1", AUTO, FLAT, ENTRY_CAST, 32767, 0, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=4) sort n=3",
		"trace_lane_kernel<false, false> 2048x256 lds=24576"},
	{"incoherent 2^15", AUTO, FLAT, ENTRY_CAST, 32768, 0, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=4) sort n=3",
		"trace_lane_kernel<false, false> 2048x256 lds=24576"},
	{"incoherent 2^15+1", AUTO, FLAT, ENTRY_CAST, 32769, 0, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=0) sort n=3",
		"trace_lane_kernel<false, false> 129x256 lds=24576"},
	{"incoherent 65535", AUTO, FLAT, ENTRY_CAST, 65535, 0, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=0) sort n=3",
		"trace_lane_kernel<false, false> 256x256 lds=24576"},
	{"incoherent 65536", AUTO, FLAT, ENTRY_CAST, 65536, 0, 0, 0, 0, 0, NONE, "k=l8p map=lin q=0 lane(l8p pers blocks=256 lds=16 spill=0 wait=8) sort n=3",
		"trace_lane_persistent_kernel<false, 8, false, false> 256x256 lds=16384"},
	{"incoherent 2^17", AUTO, FLAT, ENTRY_CAST, 1u << 17, 0, 0, 0, 0, 0, NONE, "k=l8p map=lin q=0 lane(l8p pers blocks=512 lds=16 spill=0 wait=8) sort n=3",
		"trace_lane_persistent_kernel<false, 8, false, false> 512x256 lds=16384"},
	{"incoherent 2^22", AUTO, FLAT, ENTRY_CAST, 1u << 22, 0, 0, 0, 0, 0, NONE, "k=l8p map=lin q=0 lane(l8p pers blocks=2048 lds=16 spill=0 wait=8) sort n=3",
		"trace_lane_persistent_kernel<false, 8, false, false> 2048x256 lds=16384"},
	{"incoherent 2^24", AUTO, FLAT, ENTRY_CAST, 1u << 24, 0, 0, 0, 0, 0, NONE, "k=l8p map=lin q=0 lane(l8p pers blocks=2048 lds=16 spill=0 wait=8) sort n=3",
		"trace_lane_persistent_kernel<false, 8, false, false> 2048x256 lds=16384"},
	{"FORCE_SORT 1", AUTO, FLAT, ENTRY_CAST, 1, FORCE, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) sort n=3",
		"trace_lane_kernel<false, false> 1x256 lds=24576"},
	{"TOKEN_OUT 100000", AUTO, FLAT, ENTRY_CAST, 100000, TOKEN, 0, 0, 0, 0, NONE, "k=l8p map=lin q=0 lane(l8p pers blocks=391 lds=16 spill=0 wait=8) sort n=3",
		"trace_lane_persistent_kernel<false, 8, false, false> 391x256 lds=16384"},
	{"BOOL_OUT 10", AUTO, FLAT, ENTRY_CAST, 10, BOOL, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) n=1",
		"trace_lane_kernel<false, false> 3x256 lds=24576"},
	{"ASYNC 65536", AUTO, FLAT, ENTRY_CAST, 65536, ASYNC, 0, 0, 0, 0, NONE, "k=l8p map=lin q=0 lane(l8p pers blocks=256 lds=16 spill=0 wait=8) sort n=3",
		"trace_lane_persistent_kernel<false, 8, false, false> 256x256 lds=16384"},
	{"no 8-wide 65536", AUTO, NO8, ENTRY_CAST, 65536, 0, 0, 0, 0, 0, NONE, "k=l4p map=lin q=0 lane(l4p pers blocks=256 lds=16 spill=0 wait=16) sort n=3",
		"trace_lane_persistent_kernel<false, 4, false, false> 256x256 lds=16384"},
	{"2-wide only 65536", AUTO, BARE, ENTRY_CAST, 65536, 0, 0, 0, 0, 0, NONE, "k=lp map=lin q=0 lane(lp pers blocks=256 lds=16 spill=4 wait=16) sort n=3",
		"trace_lane_persistent_kernel<false, 2, false, false> 256x256 lds=16384"},
	{"stack_override 8", with(AUTO, &Opt::stack_override, 8), FLAT, ENTRY_CAST, 65536, 0, 0, 0, 0, 0, NONE, "k=l8p map=lin q=0 lane(l8p pers blocks=256 lds=8 spill=2 wait=8) sort n=3",
		"trace_lane_persistent_kernel<false, 8, false, false> 256x256 lds=8192"},
	{"stack_override 32", with(AUTO, &Opt::stack_override, 32), FLAT, ENTRY_CAST, 1u << 22, 0, 0, 0, 0, 0, NONE, "k=l8p map=lin q=0 lane(l8p pers blocks=1280 lds=32 spill=0 wait=8) sort n=3",
		"trace_lane_persistent_kernel<false, 8, false, false> 1280x256 lds=32768"},
	{"pipelined chunk 2^20", AUTO, FLAT, ENTRY_CHUNK, 1u << 20, MRT_FLAG_RAYS_ON_DEVICE | MRT_FLAG_HITS_ON_DEVICE, 0, 0, 0, 0, NONE, "k=l8p map=lin q=0 lane(l8p pers blocks=2048 lds=16 spill=0 wait=8) sort n=3",
		"trace_lane_persistent_kernel<false, 8, false, false> 2048x256 lds=16384"},
	// ---- declared coherent: the width is looked for on the device from 256 rays; packets with the lane launch queued behind
	{"coherent 63", AUTO, FLAT, ENTRY_CAST, 63, COH, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) n=1",
		"trace_lane_kernel<false, false> 16x256 lds=24576"},
	{"coherent 64", AUTO, FLAT, ENTRY_CAST, 64, COH, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) n=1",
		"trace_lane_kernel<false, false> 16x256 lds=24576"},
	{"coherent 255", AUTO, FLAT, ENTRY_CAST, 255, COH, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) n=1",
		"trace_lane_kernel<false, false> 64x256 lds=24576"},
	{"coherent 256", AUTO, FLAT, ENTRY_CAST, 256, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=2 dual(lane sparse=1) detect n=2",
		"trace_packet_asm_kernel<false, false, true> 16x256 lds=0 | trace_lane_kernel<false, false> 64x256 lds=24576"},
	{"coherent 2^15", AUTO, FLAT, ENTRY_CAST, 32768, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=2 dual(lane sparse=4) detect n=2",
		"trace_packet_asm_kernel<false, false, true> 2048x256 lds=0 | trace_lane_kernel<false, false> 2048x256 lds=24576"},
	{"coherent 2^15+1", AUTO, FLAT, ENTRY_CAST, 32769, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=1 dual(lane sparse=0) detect n=2",
		"trace_packet_asm_kernel<false, false, true> 513x256 lds=0 | trace_lane_kernel<false, false> 129x256 lds=24576"},
	{"coherent 65535", AUTO, FLAT, ENTRY_CAST, 65535, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=1 dual(lane sparse=0) detect n=2",
		"trace_packet_asm_kernel<false, false, true> 1024x256 lds=0 | trace_lane_kernel<false, false> 256x256 lds=24576"},
	{"coherent 65536", AUTO, FLAT, ENTRY_CAST, 65536, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=1 dual(l8p pers blocks=256 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_asm_kernel<false, false, true> 1024x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 256x256 lds=16384"},
	{"coherent 3600 tiles of rays", AUTO, FLAT, ENTRY_CAST, 230400, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=1 dual(l8p pers blocks=900 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_asm_kernel<false, false> 3600x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 900x256 lds=16384"},
	{"coherent 3600 tiles + 1 ray", AUTO, FLAT, ENTRY_CAST, 230401, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=0 dual(l8p pers blocks=901 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_asm_kernel<false, false, true> 901x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 901x256 lds=16384"},
	{"coherent 2^19", AUTO, FLAT, ENTRY_CAST, 1u << 19, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=0 dual(l8p pers blocks=2048 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_asm_kernel<false, false, true> 2048x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 2048x256 lds=16384"},
	{"coherent 2^22-1", AUTO, FLAT, ENTRY_CAST, (1u << 22) - 1, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=0 dual(l8p pers blocks=2048 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_asm_kernel<false, false> 16384x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 2048x256 lds=16384"},
	{"coherent 2^22", AUTO, FLAT, ENTRY_CAST, 1u << 22, COH, 0, 0, 0, 0, NONE, "k=dual map=auto q=0 dual(l8p pers blocks=2048 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_rows_kernel<false, false, 2, 64, false> 32768x64 lds=0 group=2 | trace_lane_persistent_kernel<false, 8, false, false> 2048x256 lds=16384"},
	{"coherent 2^22+1", AUTO, FLAT, ENTRY_CAST, (1u << 22) + 1, COH, 0, 0, 0, 0, NONE, "k=dual map=auto q=0 dual(l8p pers blocks=2048 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_rows_kernel<false, false, 2, 64, false> 32769x64 lds=0 group=2 | trace_lane_persistent_kernel<false, 8, false, false> 2048x256 lds=16384"},
	{"coherent 2^24", AUTO, FLAT, ENTRY_CAST, 1u << 24, COH, 0, 0, 0, 0, NONE, "k=dual map=auto q=0 dual(l8p pers blocks=2048 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_rows_kernel<false, false, 2, 64, false> 131072x64 lds=0 group=2 | trace_lane_persistent_kernel<false, 8, false, false> 2048x256 lds=16384"},
	{"coherent + FORCE_SORT 300", AUTO, FLAT, ENTRY_CAST, 300, COH | FORCE, 0, 0, 0, 0, NONE, "k=asm map=auto q=2 dual(lane sparse=1) detect n=2",
		"trace_packet_asm_kernel<false, false, true> 19x256 lds=0 | trace_lane_kernel<false, false> 75x256 lds=24576"},
	{"coherent HOST_LAYOUT 1024", AUTO, FLAT, ENTRY_CAST, 1024, COH | HOST, 0, 0, 0, 0, NONE, "k=asm map=auto q=2 dual(lane sparse=1) detect n=2",
		"trace_packet_asm_kernel<false, false, true> 64x256 lds=0 | trace_lane_kernel<false, false> 256x256 lds=24576"},
	{"coherent submit 4096", AUTO, FLAT, ENTRY_SUBMIT, 4096, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=2 dual(lane sparse=1) detect n=2",
		"trace_packet_asm_kernel<false, false, true> 256x256 lds=0 | trace_lane_kernel<false, false> 1024x256 lds=24576"},
	{"coherent grid_tile 1", with(AUTO, &Opt::grid_tile, 1), FLAT, ENTRY_CAST, 4096, COH, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) n=1",
		"trace_lane_kernel<false, false> 1024x256 lds=24576"},
	{"coherent count_visits", with(AUTO, &Opt::count_visits, 1), FLAT, ENTRY_CAST, 4096, COH, 0, 0, 0, 0, NONE, "k=lane map=auto q=0 lane(lane sparse=0 cnt) detect n=2 cnt",
		"trace_lane_kernel<false, true> 16x256 lds=24576"},
	{"coherent tile_w_log2 2", with(AUTO, &Opt::tile_w_log2, 2), FLAT, ENTRY_CAST, 4096, COH, 0, 0, 0, 0, NONE, "k=lane map=auto q=0 lane(lane sparse=0) detect n=2",
		"trace_lane_kernel<false, false> 16x256 lds=24576"},
	{"coherent 2^22 no rows", AUTO, BARE, ENTRY_CAST, 1u << 22, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=0 dual(lp pers blocks=2048 lds=16 spill=4 wait=16) detect n=2",
		"trace_packet_asm_kernel<false, false> 16384x256 lds=0 | trace_lane_persistent_kernel<false, 2, false, false> 2048x256 lds=16384"},
	{"coherent 4096 past kAsmNodeLimit", AUTO, BIG, ENTRY_CAST, 4096, COH, 0, 0, 0, 0, NONE, "k=lane map=auto q=0 lane(lane sparse=0) detect n=2",
		"trace_lane_kernel<false, false> 16x256 lds=24576"},
	{"coherent 65536 past kAsmNodeLimit", AUTO, BIG, ENTRY_CAST, 65536, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=0 dual(l8p pers blocks=256 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_kernel<false, false> 256x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 256x256 lds=16384"},
	// ---- two-level scenes
	{"two-level incoherent 1", AUTO, TL, ENTRY_CAST, 1, 0, 0, 0, 0, 0, NONE, "k=tl map=lin q=0 lane(tl sparse=1) n=1",
		"trace_two_level_kernel<false> 1x256 lds=32768"},
	{"two-level incoherent 65536", AUTO, TL, ENTRY_CAST, 65536, 0, 0, 0, 0, 0, NONE, "k=tlp8 map=lin q=0 lane(tlp8 pers blocks=256 lds=16 spill=0 wait=8) sort n=3",
		"trace_lane_persistent_kernel<false, 8, true, false> 256x256 lds=16384"},
	{"two-level no 8-wide 65536", AUTO, TL_NO8, ENTRY_CAST, 65536, 0, 0, 0, 0, 0, NONE, "k=tlp map=lin q=0 lane(tlp pers blocks=256 lds=16 spill=14 wait=16) sort n=3",
		"trace_lane_persistent_kernel<false, 2, true, false> 256x256 lds=16384"},
	{"two-level count_visits 65536", with(AUTO, &Opt::count_visits, 1), TL, ENTRY_CAST, 65536, 0, 0, 0, 0, 0, NONE, "k=tl map=lin q=0 lane(tl sparse=0 cnt) sort n=3 cnt",
		"trace_two_level_kernel<false> 256x256 lds=32768"},
	{"two-level coherent 4096", AUTO, TL, ENTRY_CAST, 4096, COH, 0, 0, 0, 0, NONE, "k=tlpkt map=auto q=2 dual(tl sparse=1) detect n=2",
		"trace_two_level_packet_kernel<false> 256x256 lds=0 | trace_two_level_kernel<false> 1024x256 lds=32768"},
	{"two-level coherent 2^17", AUTO, TL, ENTRY_CAST, 1u << 17, COH, 0, 0, 0, 0, NONE, "k=tlpkt map=auto q=1 dual(tlp8 pers blocks=512 lds=16 spill=0 wait=8) detect n=2",
		"trace_two_level_packet_kernel<false> 2048x256 lds=0 | trace_lane_persistent_kernel<false, 8, true, false> 512x256 lds=16384"},
	{"two-level coherent 2^19", AUTO, TL, ENTRY_CAST, 1u << 19, COH, 0, 0, 0, 0, NONE, "k=tlpkt map=auto q=0 dual(tlp8 pers blocks=2048 lds=16 spill=0 wait=8) detect n=2",
		"trace_two_level_packet_kernel<false> 2048x256 lds=0 | trace_lane_persistent_kernel<false, 8, true, false> 2048x256 lds=16384"},
	// ---- explicit kernels
	{"ASM coherent", kernel(MRT_KERNEL_PACKET_ASM), FLAT, ENTRY_CAST, 4096, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=0 plain detect n=2",
		"trace_packet_asm_kernel<false, false, true> 16x256 lds=0"},
	{"ASM incoherent", kernel(MRT_KERNEL_PACKET_ASM), FLAT, ENTRY_CAST, 4096, 0, 0, 0, 0, 0, NONE, "k=asm map=lin q=0 plain sort n=3",
		"trace_packet_asm_kernel<false, false, true> 16x256 lds=0"},
	{"LANE 255", kernel(MRT_KERNEL_LANE), FLAT, ENTRY_CAST, 255, 0, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) n=1",
		"trace_lane_kernel<false, false> 64x256 lds=24576"},
	{"LANE 256", kernel(MRT_KERNEL_LANE), FLAT, ENTRY_CAST, 256, 0, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) sort n=3",
		"trace_lane_kernel<false, false> 64x256 lds=24576"},
	{"LANE coherent", kernel(MRT_KERNEL_LANE), FLAT, ENTRY_CAST, 4096, COH, 0, 0, 0, 0, NONE, "k=lane map=auto q=0 lane(lane sparse=0) detect n=2",
		"trace_lane_kernel<false, false> 16x256 lds=24576"},
	{"LANE_PERSISTENT incoherent", kernel(MRT_KERNEL_LANE_PERSISTENT), FLAT, ENTRY_CAST, 1000, 0, 0, 0, 0, 0, NONE, "k=lp map=lin q=0 lane(lp pers blocks=4 lds=16 spill=4 wait=16) sort n=3",
		"trace_lane_persistent_kernel<false, 2, false, false> 4x256 lds=16384"},
	{"LANE_PERSISTENT coherent", kernel(MRT_KERNEL_LANE_PERSISTENT), FLAT, ENTRY_CAST, 1000, COH, 0, 0, 0, 0, NONE, "k=lp map=lin q=0 lane(lp pers blocks=4 lds=16 spill=4 wait=16) n=1",
		"trace_lane_persistent_kernel<false, 2, false, false> 4x256 lds=16384"},
	{"LANE4_PERSISTENT", kernel(MRT_KERNEL_LANE4_PERSISTENT), FLAT, ENTRY_CAST, 100, 0, 0, 0, 0, 0, NONE, "k=l4p map=lin q=0 lane(l4p pers blocks=1 lds=16 spill=0 wait=16) n=1",
		"trace_lane_persistent_kernel<false, 4, false, false> 1x256 lds=16384"},
	{"LANE8_PERSISTENT", kernel(MRT_KERNEL_LANE8_PERSISTENT), FLAT, ENTRY_CAST, 100, 0, 0, 0, 0, 0, NONE, "k=l8p map=lin q=0 lane(l8p pers blocks=1 lds=16 spill=0 wait=8) n=1",
		"trace_lane_persistent_kernel<false, 8, false, false> 1x256 lds=16384"},
	{"LANE8_PERSISTENT without 8-wide", kernel(MRT_KERNEL_LANE8_PERSISTENT), BARE, ENTRY_CAST, 100, 0, 0, 0, 0, 0, NONE, "k=lp map=lin q=0 lane(lp pers blocks=1 lds=16 spill=4 wait=16) n=1",
		"trace_lane_persistent_kernel<false, 2, false, false> 1x256 lds=16384"},
	{"PACKET_DUAL coherent", kernel(MRT_KERNEL_PACKET_DUAL), FLAT, ENTRY_CAST, 4096, COH, 0, 0, 0, 0, NONE, "k=dual map=auto q=0 plain detect n=2",
		"trace_packet_rows_kernel<false, false, 2, 64, false> 32x64 lds=0 group=2"},
	{"PACKET_DUAL coherent no rows", kernel(MRT_KERNEL_PACKET_DUAL), NO_ROWS, ENTRY_CAST, 4096, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=0 plain detect n=2",
		"trace_packet_asm_kernel<false, false, true> 16x256 lds=0"},
	{"PACKET_DUAL incoherent", kernel(MRT_KERNEL_PACKET_DUAL), FLAT, ENTRY_CAST, 4096, 0, 0, 0, 0, 0, NONE, "k=lane map=lin q=0 lane(lane sparse=1) sort n=3",
		"trace_lane_kernel<false, false> 1024x256 lds=24576"},
	{"PACKET_ROWS coherent", kernel(MRT_KERNEL_PACKET_ROWS), FLAT, ENTRY_CAST, 4096, COH, 0, 0, 0, 0, NONE, "k=rows map=auto q=0 plain detect n=2",
		"trace_packet_rows_kernel<false, false, 1, 256, false> 16x256 lds=0 group=4"},
	{"PACKET_QUAD coherent no 4-wide rows", kernel(MRT_KERNEL_PACKET_QUAD), FLAT, ENTRY_CAST, 4096, COH, 0, 0, 0, 0, NONE, "k=asm map=auto q=0 plain detect n=2",
		"trace_packet_asm_kernel<false, false, true> 16x256 lds=0"},
	{"LANE two-level coherent", kernel(MRT_KERNEL_LANE), TL, ENTRY_CAST, 1u << 17, COH, 0, 0, 0, 0, NONE, "k=tl map=auto q=0 lane(tl sparse=0) detect n=2",
		"trace_two_level_kernel<false> 512x256 lds=32768"},
	{"LANE_PERSISTENT two-level", kernel(MRT_KERNEL_LANE_PERSISTENT), TL, ENTRY_CAST, 1000, 0, 0, 0, 0, 0, NONE, "k=tl map=lin q=0 lane(tl sparse=1) sort n=3",
		"trace_two_level_kernel<false> 250x256 lds=32768"},
	{"LANE8_PERSISTENT two-level", kernel(MRT_KERNEL_LANE8_PERSISTENT), TL, ENTRY_CAST, 1000, 0, 0, 0, 0, 0, NONE, "k=tlp8 map=lin q=0 lane(tlp8 pers blocks=4 lds=16 spill=0 wait=8) sort n=3",
		"trace_lane_persistent_kernel<false, 8, true, false> 4x256 lds=16384"},
	// ---- the width found by the previous cast of as many rays: a tile schedule (and the tuner) as for a grid of that width
	{"prev detect 640x360", AUTO, FLAT, ENTRY_CAST, 230400, COH, 640, 360, 0, 0, SAME, "k=asm map=auto q=0 dual(l8p pers blocks=900 lds=16 spill=0 wait=8) detect sched=640x360/80+pieces n=2",
		"trace_packet_asm_kernel<false, false, true> 2048x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 900x256 lds=16384"},
	{"prev detect other count", AUTO, FLAT, ENTRY_CAST, 230400, COH, 640, 360, 0, 0, OTHER_COUNT, "k=asm map=auto q=1 dual(l8p pers blocks=900 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_asm_kernel<false, false> 3600x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 900x256 lds=16384"},
	{"prev detect incoherent", AUTO, FLAT, ENTRY_CAST, 230400, COH, 640, 360, 0, 0, INCOHERENT, "k=asm map=auto q=1 dual(l8p pers blocks=900 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_asm_kernel<false, false> 3600x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 900x256 lds=16384"},
	{"prev detect pending", AUTO, FLAT, ENTRY_CAST, 230400, COH, 640, 360, 0, 0, PENDING, "k=asm map=auto q=1 dual(l8p pers blocks=900 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_asm_kernel<false, false> 3600x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 900x256 lds=16384"},
	{"prev detect no width", AUTO, FLAT, ENTRY_CAST, 230400, COH, 640, 360, 0, 0, NO_WIDTH, "k=asm map=auto q=1 dual(l8p pers blocks=900 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_asm_kernel<false, false> 3600x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 900x256 lds=16384"},
	{"prev detect 512x256 (all in quarters)", AUTO, FLAT, ENTRY_CAST, 131072, COH, 512, 256, 0, 0, SAME, "k=asm map=auto q=1 dual(l8p pers blocks=512 lds=16 spill=0 wait=8) detect n=2",
		"trace_packet_asm_kernel<false, false, true> 2048x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 512x256 lds=16384"},
	{"prev detect 1280x960", AUTO, FLAT, ENTRY_CAST, 1228800, COH, 1280, 960, 0, 0, SAME, "k=asm map=auto q=0 dual(l8p pers blocks=2048 lds=16 spill=0 wait=8) detect sched=1280x960/160+pieces arms n=2",
		"trace_packet_asm_kernel<false, false> 7200x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 2048x256 lds=16384"},
	{"prev detect 1280x960 submit", AUTO, FLAT, ENTRY_SUBMIT, 1228800, COH, 1280, 960, 0, 0, SAME, "k=asm map=auto q=0 dual(l8p pers blocks=2048 lds=16 spill=0 wait=8) detect sched=1280x960/160+pieces n=2",
		"trace_packet_asm_kernel<false, false> 7200x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 2048x256 lds=16384"},
	{"prev detect 1280x960 ASYNC", AUTO, FLAT, ENTRY_CAST, 1228800, COH | ASYNC, 1280, 960, 0, 0, SAME, "k=asm map=auto q=0 dual(l8p pers blocks=2048 lds=16 spill=0 wait=8) detect sched=1280x960/160+pieces n=2",
		"trace_packet_asm_kernel<false, false> 7200x256 lds=0 | trace_lane_persistent_kernel<false, 8, false, false> 2048x256 lds=16384"},
	{"prev detect count_visits", with(AUTO, &Opt::count_visits, 1), FLAT, ENTRY_CAST, 230400, COH, 640, 360, 0, 0, SAME, "k=asm map=auto q=0 plain detect n=2 cnt",
		"trace_packet_asm_kernel<false, true> 900x256 lds=0"},
	// ---- grids of known width (mrt_cast_grid): quarter / sixteenth tiles up to 3 600 / 512 tiles, the schedule from 2^17 rays
	{"grid 7x5", AUTO, FLAT, ENTRY_GRID, 0, 0, 7, 5, 0, 5, NONE, "k=lane map=tile q=0 plain n=1",
		"trace_lane_kernel<false, false> 1x256 lds=24576"},
	{"grid 8x8", AUTO, FLAT, ENTRY_GRID, 0, 0, 8, 8, 0, 8, NONE, "k=asm map=tile q=2 plain n=1",
		"trace_packet_asm_kernel<false, false, true> 4x256 lds=0"},
	{"grid 16x12", AUTO, FLAT, ENTRY_GRID, 0, 0, 16, 12, 0, 12, NONE, "k=asm map=tile q=2 plain n=1",
		"trace_packet_asm_kernel<false, false, true> 16x256 lds=0"},
	{"grid 184x176 (506 tiles)", AUTO, FLAT, ENTRY_GRID, 0, 0, 184, 176, 0, 176, NONE, "k=asm map=tile q=2 plain n=1",
		"trace_packet_asm_kernel<false, false, true> 2024x256 lds=0"},
	{"grid 192x176 (528 tiles)", AUTO, FLAT, ENTRY_GRID, 0, 0, 192, 176, 0, 176, NONE, "k=asm map=tile q=1 plain n=1",
		"trace_packet_asm_kernel<false, false, true> 528x256 lds=0"},
	{"grid 512x255", AUTO, FLAT, ENTRY_GRID, 0, 0, 512, 255, 0, 255, NONE, "k=asm map=tile q=1 plain n=1",
		"trace_packet_asm_kernel<false, false, true> 2048x256 lds=0"},
	{"grid 512x256 (2^17, all in quarters)", AUTO, FLAT, ENTRY_GRID, 0, 0, 512, 256, 0, 256, NONE, "k=asm map=tile q=1 plain n=1",
		"trace_packet_asm_kernel<false, false, true> 2048x256 lds=0"},
	{"grid 640x360 (3600 tiles)", AUTO, FLAT, ENTRY_GRID, 0, 0, 640, 360, 0, 360, NONE, "k=asm map=tile q=0 plain sched=640x360/80+pieces n=1",
		"trace_packet_asm_kernel<false, false, true> 2048x256 lds=0"},
	{"grid 648x360 (3645 tiles)", AUTO, FLAT, ENTRY_GRID, 0, 0, 648, 360, 0, 360, NONE, "k=asm map=tile q=0 plain sched=648x360/81+pieces n=1",
		"trace_packet_asm_kernel<false, false, true> 2048x256 lds=0"},
	{"grid 1280x960", AUTO, FLAT, ENTRY_GRID, 0, 0, 1280, 960, 0, 960, NONE, "k=asm map=tile q=0 plain sched=1280x960/160+pieces arms n=1",
		"trace_packet_asm_kernel<false, false> 7200x256 lds=0"},
	{"grid 1280x960 ASYNC", AUTO, FLAT, ENTRY_GRID, 0, ASYNC, 1280, 960, 0, 960, NONE, "k=asm map=tile q=0 plain sched=1280x960/160+pieces n=0",
		"trace_packet_asm_kernel<false, false> 7200x256 lds=0"},
	{"grid row block 1280x[100,300)", AUTO, FLAT, ENTRY_GRID, 0, 0, 1280, 960, 100, 200, NONE, "k=asm map=tile q=0 plain sched=1280x200/160+pieces n=1",
		"trace_packet_asm_kernel<false, false, true> 2048x256 lds=0"},
	{"grid 2048x2048 (2^22)", AUTO, FLAT, ENTRY_GRID, 0, 0, 2048, 2048, 0, 2048, NONE, "k=dual map=tile q=0 plain sched=2048x2048/256+pieces n=1",
		"trace_packet_rows_kernel<false, false, 2, 64, true> 49152x64 lds=0 group=2"},
	{"grid 4096x4096 (2^24)", AUTO, FLAT, ENTRY_GRID, 0, 0, 4096, 4096, 0, 4096, NONE, "k=dual map=tile q=0 plain n=1",
		"trace_packet_rows_kernel<false, false, 2, 64, true> 131072x64 lds=0 group=2"},
	{"grid grid_tile 1", with(AUTO, &Opt::grid_tile, 1), FLAT, ENTRY_GRID, 0, 0, 640, 360, 0, 360, NONE, "k=asm map=lin q=0 plain n=1",
		"trace_packet_asm_kernel<false, false, true> 900x256 lds=0"},
	{"grid tile_schedule 1", with(AUTO, &Opt::tile_schedule, 1), FLAT, ENTRY_GRID, 0, 0, 648, 360, 0, 360, NONE, "k=asm map=tile q=0 plain n=1",
		"trace_packet_asm_kernel<false, false, true> 912x256 lds=0"},
	{"grid tile_schedule 2", with(AUTO, &Opt::tile_schedule, 2), FLAT, ENTRY_GRID, 0, 0, 648, 360, 0, 360, NONE, "k=asm map=tile q=0 plain sched=648x360/81 n=1",
		"trace_packet_asm_kernel<false, false, true> 912x256 lds=0"},
	{"grid count_visits", with(AUTO, &Opt::count_visits, 1), FLAT, ENTRY_GRID, 0, 0, 648, 360, 0, 360, NONE, "k=asm map=tile q=0 plain n=1 cnt",
		"trace_packet_asm_kernel<false, true> 912x256 lds=0"},
	{"grid count_visits 64x64", with(AUTO, &Opt::count_visits, 1), FLAT, ENTRY_GRID, 0, 0, 64, 64, 0, 64, NONE, "k=lane map=tile q=0 plain n=1 cnt",
		"trace_lane_kernel<false, true> 16x256 lds=24576"},
	{"grid tile_w_log2 4", with(AUTO, &Opt::tile_w_log2, 4), FLAT, ENTRY_GRID, 0, 0, 648, 360, 0, 360, NONE, "k=asm map=tile q=0 plain sched=648x360/41 n=1",
		"trace_packet_asm_kernel<false, false, true> 923x256 lds=0"},
	{"grid past kAsmNodeLimit", AUTO, BIG, ENTRY_GRID, 0, 0, 640, 360, 0, 360, NONE, "k=asm map=tile q=0 plain sched=640x360/80+pieces n=1",
		"trace_packet_kernel<false, false> 2048x256 lds=0"},
	{"grid two-level 64x64", AUTO, TL, ENTRY_GRID, 0, 0, 64, 64, 0, 64, NONE, "k=tlpkt map=tile q=2 plain n=1",
		"trace_two_level_packet_kernel<false> 256x256 lds=0"},
	{"grid two-level 1280x960", AUTO, TL, ENTRY_GRID, 0, 0, 1280, 960, 0, 960, NONE, "k=tlpkt map=tile q=0 plain n=1",
		"trace_two_level_packet_kernel<false> 4800x256 lds=0"},
	{"grid ASM 648x360", kernel(MRT_KERNEL_PACKET_ASM), FLAT, ENTRY_GRID, 0, 0, 648, 360, 0, 360, NONE, "k=asm map=tile q=0 plain sched=648x360/81+pieces n=1",
		"trace_packet_asm_kernel<false, false, true> 2048x256 lds=0"},
	{"grid ASM 64x64", kernel(MRT_KERNEL_PACKET_ASM), FLAT, ENTRY_GRID, 0, 0, 64, 64, 0, 64, NONE, "k=asm map=tile q=0 plain n=1",
		"trace_packet_asm_kernel<false, false, true> 16x256 lds=0"},
	{"grid PACKET_DUAL 648x360", kernel(MRT_KERNEL_PACKET_DUAL), FLAT, ENTRY_GRID, 0, 0, 648, 360, 0, 360, NONE, "k=dual map=tile q=0 plain sched=648x360/81+pieces n=1",
		"trace_packet_rows_kernel<false, false, 2, 64, true> 8192x64 lds=0 group=2"},
	{"grid PACKET_DUAL no rows", kernel(MRT_KERNEL_PACKET_DUAL), NO_ROWS, ENTRY_GRID, 0, 0, 648, 360, 0, 360, NONE, "k=asm map=tile q=0 plain sched=648x360/81+pieces n=1",
		"trace_packet_asm_kernel<false, false, true> 2048x256 lds=0"},
	{"grid LANE 648x360", kernel(MRT_KERNEL_LANE), FLAT, ENTRY_GRID, 0, 0, 648, 360, 0, 360, NONE, "k=lane map=tile q=0 plain n=1",
		"trace_lane_kernel<false, false> 912x256 lds=24576"},
	{"grid LANE_PERSISTENT 648x360", kernel(MRT_KERNEL_LANE_PERSISTENT), FLAT, ENTRY_GRID, 0, 0, 648, 360, 0, 360, NONE, "k=lp map=tile q=0 plain n=1",
		"trace_lane_kernel<false, false> 912x256 lds=24576"},
	// ---- tiled casts (mrt_cast_tiled): the grid rules without schedule or tuner
	{"tiled 64x64", AUTO, FLAT, ENTRY_TILED, 0, 0, 64, 64, 0, 64, NONE, "k=asm map=tile q=2 plain n=1",
		"trace_packet_asm_kernel<false, false, true> 256x256 lds=0"},
	{"tiled 648x360", AUTO, FLAT, ENTRY_TILED, 0, 0, 648, 360, 0, 360, NONE, "k=asm map=tile q=0 plain n=1",
		"trace_packet_asm_kernel<false, false, true> 912x256 lds=0"},
	{"tiled 1280x960", AUTO, FLAT, ENTRY_TILED, 0, 0, 1280, 960, 0, 960, NONE, "k=asm map=tile q=0 plain n=1",
		"trace_packet_asm_kernel<false, false> 4800x256 lds=0"},
	{"tiled 2048x2048", AUTO, FLAT, ENTRY_TILED, 0, 0, 2048, 2048, 0, 2048, NONE, "k=dual map=tile q=0 plain n=1",
		"trace_packet_rows_kernel<false, false, 2, 64, false> 32768x64 lds=0 group=2"},
	{"tiled grid_tile 1", with(AUTO, &Opt::grid_tile, 1), FLAT, ENTRY_TILED, 0, 0, 64, 64, 0, 64, NONE, "k=lane map=lin q=0 plain n=1",
		"trace_lane_kernel<false, false> 16x256 lds=24576"},
};

// ---- what a plan runs ---------------------------------------------------------------------------------------------------------
// <name> <workgroups>x<threads> lds=<bytes> [group=<tile_group>]; "nothing" for a launch without rays, "error" past 2^31 - 1 workgroups
std::string describe(const TraceLaunch &l, const char *family = nullptr, int src = 0, bool with_mode = false)
{
	if (l.error) return "error";
	if (l.blocks == 0) return "nothing";
	char name[96], b[192];
	format_variant(name, sizeof(name), l.v, family, src, with_mode);
	int n = std::snprintf(b, sizeof(b), "%s %ux%u lds=%zu", name, l.blocks, l.threads, l.lds);
	if (l.v.kernel == TraceKernel::PACKET_ROWS) std::snprintf(b + n, sizeof(b) - n, " group=%u", l.tile_group);
	return b;
}

// The lanes a plain or packet launch must cover: a lane per ray and piece of a tile; a lane per ray where the width is found on the device
uint64_t lanes_needed(const TraceParams &p)
{
	return p.lane_map == MAP_TILE8X8 ? p.count * (p.quarter_all == 2u ? 16u : (p.quarter_all ? 4u : 1u)) : p.count;
}
void covers(const std::string &name, const TraceParams &p, const TraceLaunch &l)
{
	if (l.error || l.v.kernel == TraceKernel::LANE_PERSISTENT) return; // (resident waves pull their rays from a counter)
	expect((uint64_t)l.blocks * l.threads * l.packets_per_wave() >= lanes_needed(p), name + ": the launch covers the batch (" + describe(l) + ")");
}

const uint32_t kResidentWords[4] = {0, 0, 0, 0};
template <class T> const T *resident() { return reinterpret_cast<const T *>(kResidentWords); } // an array the resolvers only test for null

// TraceParams as api.hip base_params makes them for a scene that fits the Infinity Cache (64-thread workgroups for the 128-ray
// walk, culling by where the rays come from)
TraceParams scene_params(const SceneFacts &s, const mrt_options &o)
{
	TraceParams p;
	std::memset(&p, 0, sizeof(p));
	if (s.rows) p.row_array = resident<void>();
	if (s.rows4) p.row_array4 = resident<void>();
	if (s.nodes4) p.nodes4 = resident<Dev4Node>();
	if (s.nodes8) { p.nodes8 = resident<Dev8Node>(); p.leaf_box = resident<float>(); }
	p.n_nodes = s.n_nodes; p.stack_depth = (s.depth + 7u) / 8u * 8u;
	p.tile_w_log2 = tile_w_log2(o); p.rows_wg = 64u; p.rows_cull = 2u; p.kernel = MRT_KERNEL_LANE;
	return p;
}

// What cast.hip launch_planned (with launch_lane, and schedule.hip schedule_grid once the grid has an order) puts on the stream
// for a plan, closest hit: the packet launch, the lane launch, or "packet | lane" where both are queued
std::string runs(const Case &t, const CastPlan &c)
{
	const mrt_options o = options(t.opt);
	TraceParams p = scene_params(scene(t.scene), o);
	if (ray_entry(t.entry)) { p.count = t.count; p.in_fmt = (t.flags & HOST) ? IN_HOST60 : IN_RAY32; }
	else {
		p.count = (uint64_t)t.w * t.rows; p.in_fmt = t.entry == ENTRY_GRID ? IN_GRID : IN_RAY32;
		p.grid_w = t.w; p.grid_h = t.h; p.y0 = t.y0; p.rows = t.rows; p.tiles_x = c.tiles_x;
	}
	p.kernel = c.kernel; p.lane_map = c.lane_map; p.quarter_all = c.quarter_all;
	if (c.scheduled) {
		const uint32_t th = 64u >> p.tile_w_log2;
		p.tile_unit = c.kernel == MRT_KERNEL_PACKET_DUAL ? 2u : 1u;
		p.n_units = (uint32_t)(((uint64_t)c.tiles_x * ((c.rows + th - 1u) / th) + p.tile_unit - 1u) / p.tile_unit);
		p.tile_sched = p.sched_hdr = resident<uint32_t>(); p.n_slots_max = schedule_slots(p.n_units, c.pieces);
	}
	const auto traced = [&](const TraceParams &q, const TraceLaunch &l) { covers(t.name, q, l); return describe(l); };
	const auto lane = [&](TraceParams q) {
		const LaneLaunch &l = c.lane;
		q.kernel = l.kernel;
		if (l.persistent) return describe(resolve_persistent(q, l.lds_depth, l.blocks, false, l.count));
		q.sparse_lanes = l.sparse_lanes;
		return traced(q, resolve_trace(q, false, l.count, false));
	};
	if (c.launch == CastPlan::LANE) return lane(p);
	const std::string packet = traced(p, resolve_trace(p, false, c.count, false));
	if (c.launch == CastPlan::PLAIN) return packet;
	TraceParams lp = p;
	lp.lane_map = MAP_LINEAR; lp.quarter_all = 0u;
	return packet + " | " + lane(lp);
}

CastPlan plan(const Case &t, GridStates &gs, const Knobs &k = Knobs())
{
	CastRequest r;
	r.entry = t.entry; r.flags = t.flags; r.mode = MRT_MODE_NEAREST;
	PrevDetect prev;
	if (ray_entry(t.entry)) {
		r.count = t.count;
		if (t.prev != NONE) {
			prev.count = t.prev == OTHER_COUNT ? t.count + 64 : t.count;
			prev.pending = t.prev == PENDING;
			prev.word[0] = t.prev == NO_WIDTH ? 0u : t.w; prev.word[1] = t.h; prev.word[2] = (t.w + 7u) / 8u;
			prev.word[3] = t.prev == INCOHERENT ? 1u : 0u;
		}
	} else {
		r.count = (uint64_t)t.w * t.rows; r.grid_w = t.w; r.grid_h = t.h; r.y0 = t.y0; r.rows = t.rows;
	}
	return plan_cast(options(t.opt), scene(t.scene), r, prev, k, gs);
}

// A batch whose width is found on the device and scheduled from a consistent pair (the width of a cast of as many rays) gets a
// launch of at least a lane per ray (launch_trace), and the prefetch rule counts at least a wave per 64 rays
void schedule_covers(const Case &t, const CastPlan &c)
{
	if (!c.scheduled || c.lane_map != MAP_AUTO) return;
	const uint32_t tw = tile_w_log2(options(t.opt)), th = 64u >> tw, unit = c.kernel == MRT_KERNEL_PACKET_DUAL ? 2u : 1u;
	const uint32_t n_units = (uint32_t)(((uint64_t)c.tiles_x * ((c.rows + th - 1u) / th) + unit - 1u) / unit);
	const uint32_t slots = schedule_slots(n_units, c.pieces);
	const uint64_t waves = n_units > kWaveSlots ? n_units : (slots < kWaveSlots ? slots : kWaveSlots);
	expect((uint64_t)slots * unit * 64u >= t.count && (unit != 1u || waves * 64u >= t.count), std::string(t.name) + ": the schedule's launch covers the batch");
}

void table()
{
	for (const Case &t : kCases) {
		GridStates gs;
		const CastPlan c = plan(t, gs);
		const std::string got = describe(c);
		expect(got == t.want, std::string(t.name) + ": got \"" + got + "\", want \"" + t.want + "\"");
		schedule_covers(t, c);
		const std::string ran = runs(t, c);
		expect(ran == t.runs, std::string(t.name) + ": runs \"" + ran + "\", want \"" + t.runs + "\"");
	}
	// the schedule's bound from the environment (MRT_SCHEDULE_MIN_LOG2 = 15) moves the tuner's with it
	Knobs k; k.schedule_min_rays = k.tune_min_rays = 1ull << 15;
	GridStates gs;
	const Case t{"grid ASM 256x128 with the bound at 2^15", kernel(MRT_KERNEL_PACKET_ASM), FLAT, ENTRY_GRID, 0, 0, 256, 128, 0, 128, NONE, ""};
	expect(describe(plan(t, gs, k)) == "k=asm map=tile q=0 plain sched=256x128/32+pieces n=1", "schedule bound 2^15: " + describe(plan(t, gs, k)));
	expect(describe(plan(t, gs)) == "k=asm map=tile q=0 plain n=1", "schedule bound 2^17: " + describe(plan(t, gs)));
}

// ---- every branch of the resolvers, on TraceParams made by hand -------------------------------------------------------------------
// a flat scene of 40 000 nodes with nothing but the 2-wide nodes resident; the setters add the rest
struct P : TraceParams {
	P(uint32_t k, uint32_t map, uint64_t n)
	{
		std::memset(static_cast<TraceParams *>(this), 0, sizeof(TraceParams));
		kernel = k; lane_map = map; count = n; in_fmt = IN_RAY32;
		n_nodes = 40000; stack_depth = 24; tile_w_log2 = 3; rows_wg = 64; rows_cull = 2;
	}
	P &with_rows() { row_array = resident<void>(); return *this; }
	P &with_rows4() { row_array4 = resident<void>(); return *this; }
	P &with_nodes4() { nodes4 = resident<Dev4Node>(); return *this; }
	P &with_nodes8(bool boxes = true) { nodes8 = resident<Dev8Node>(); if (boxes) leaf_box = resident<float>(); return *this; }
	P &grid(uint32_t w, uint32_t r) { grid_w = w; grid_h = rows = r; tiles_x = (w + 7u) / 8u; count = (uint64_t)w * r; in_fmt = IN_GRID; return *this; }
	P &from(uint32_t fmt) { in_fmt = fmt; return *this; }
	P &wg(uint32_t w) { rows_wg = w; return *this; }
	P &cull(uint32_t c) { rows_cull = c; return *this; }
	P &quarter(uint32_t q) { quarter_all = q; return *this; }
	P &sparse(uint32_t l) { sparse_lanes = l; return *this; }
	P &nodes(uint32_t n) { n_nodes = n; return *this; }
	P &lds(uint32_t bytes) { extra_lds = bytes; return *this; }
	// a tile schedule with an order (schedule.hip schedule_grid); hdr = false: the list without its header
	P &sched(uint32_t units, uint32_t unit, bool pieces, bool hdr = true)
	{
		tile_sched = resident<uint32_t>(); sched_hdr = hdr ? resident<uint32_t>() : nullptr;
		tile_unit = unit; n_units = units; n_slots_max = schedule_slots(units, pieces);
		return *this;
	}
};
constexpr uint32_t LIN = MAP_LINEAR, TILE = MAP_TILE8X8, FOUND = MAP_AUTO;
constexpr uint32_t K_LANE = MRT_KERNEL_LANE, K_PKT = MRT_KERNEL_PACKET, K_ASM = MRT_KERNEL_PACKET_ASM, K_ROWS = MRT_KERNEL_PACKET_ROWS,
	K_DUAL = MRT_KERNEL_PACKET_DUAL, K_QUAD = MRT_KERNEL_PACKET_QUAD, K_LP = MRT_KERNEL_LANE_PERSISTENT, K_L4P = MRT_KERNEL_LANE4_PERSISTENT,
	K_L8P = MRT_KERNEL_LANE8_PERSISTENT, K_TL = MRT_KERNEL_TWO_LEVEL, K_TLPKT = MRT_KERNEL_TWO_LEVEL_PACKET,
	K_TLP = MRT_KERNEL_TWO_LEVEL_PERSISTENT, K_TLP8 = MRT_KERNEL_TWO_LEVEL_PERSISTENT8;
constexpr uint64_t kPrefetchRays = (uint64_t)kPrefetchMaxWaves * 64u; // 10 240 waves of rays
constexpr uint64_t kMaxBlockRays = 0x7FFFFFFFull * 256u;

struct Launch {
	const char *name;
	P p;
	bool any_hit, count;
	const char *want;
	bool quad_built = false;
};
// launch_trace: closest hit without counters unless the row says otherwise
const Launch kTrace[] = {
	// ---- the rows kernels, and what takes their place without a row array
	{"DUAL grid", P(K_DUAL, TILE, 0).with_rows().grid(64, 64), false, false, "trace_packet_rows_kernel<false, false, 2, 64, true> 32x64 lds=0 group=2"},
	{"DUAL grid any-hit counting", P(K_DUAL, TILE, 0).with_rows().grid(64, 64), true, true, "trace_packet_rows_kernel<true, true, 2, 64, true> 32x64 lds=0 group=2"},
	{"DUAL grid without rows", P(K_DUAL, TILE, 0).grid(64, 64), false, false, "trace_packet_asm_kernel<false, false, true> 16x256 lds=0"},
	{"ROWS grid", P(K_ROWS, TILE, 0).with_rows().grid(64, 64), false, false, "trace_packet_rows_kernel<false, false, 1, 256, false> 16x256 lds=0 group=4"},
	{"ROWS grid any-hit", P(K_ROWS, TILE, 0).with_rows().grid(64, 64), true, false, "trace_packet_rows_kernel<true, false, 1, 256, false> 16x256 lds=0 group=4"},
	{"ROWS grid without rows", P(K_ROWS, TILE, 0).grid(64, 64), false, true, "trace_packet_asm_kernel<false, true> 16x256 lds=0"},
	{"DUAL workgroups of 256", P(K_DUAL, TILE, 0).with_rows().grid(64, 64).wg(256), false, false, "trace_packet_rows_kernel<false, false, 2, 256, true> 8x256 lds=0 group=8"},
	{"DUAL workgroups of 256, 130x66", P(K_DUAL, TILE, 0).with_rows().grid(130, 66).wg(256), false, false, "trace_packet_rows_kernel<false, false, 2, 256, true> 20x256 lds=0 group=8"},
	{"ROWS ignores rows_wg", P(K_ROWS, TILE, 0).with_rows().grid(64, 64).wg(64), false, false, "trace_packet_rows_kernel<false, false, 1, 256, false> 16x256 lds=0 group=4"},
	{"DUAL cull 0 grid", P(K_DUAL, TILE, 0).with_rows().grid(64, 64).cull(0), false, false, "trace_packet_rows_kernel<false, false, 2, 64, false> 32x64 lds=0 group=2"},
	{"DUAL cull 0 rays", P(K_DUAL, FOUND, 4096).with_rows().cull(0), false, false, "trace_packet_rows_kernel<false, false, 2, 64, false> 32x64 lds=0 group=2"},
	{"DUAL cull 1 grid", P(K_DUAL, TILE, 0).with_rows().grid(64, 64).cull(1), false, false, "trace_packet_rows_kernel<false, false, 2, 64, true> 32x64 lds=0 group=2"},
	{"DUAL cull 1 rays", P(K_DUAL, FOUND, 4096).with_rows().cull(1), false, false, "trace_packet_rows_kernel<false, false, 2, 64, true> 32x64 lds=0 group=2"},
	{"DUAL cull 2 grid", P(K_DUAL, TILE, 0).with_rows().grid(64, 64).cull(2), false, false, "trace_packet_rows_kernel<false, false, 2, 64, true> 32x64 lds=0 group=2"},
	{"DUAL cull 2 rays", P(K_DUAL, FOUND, 4096).with_rows().cull(2), false, false, "trace_packet_rows_kernel<false, false, 2, 64, false> 32x64 lds=0 group=2"},
	{"DUAL cull 2 host rays", P(K_DUAL, FOUND, 4096).with_rows().cull(2).from(IN_HOST60), false, false, "trace_packet_rows_kernel<false, false, 2, 64, false> 32x64 lds=0 group=2"},
	{"ROWS never culls", P(K_ROWS, TILE, 0).with_rows().grid(64, 64).cull(1), false, false, "trace_packet_rows_kernel<false, false, 1, 256, false> 16x256 lds=0 group=4"},
	{"DUAL with rows past kAsmNodeLimit", P(K_DUAL, TILE, 0).with_rows().grid(64, 64).nodes(kAsmNodeLimit), false, false, "trace_packet_rows_kernel<false, false, 2, 64, true> 32x64 lds=0 group=2"},
	// ---- the four-wide walk: only with its rows, only in a build that has it
	{"QUAD", P(K_QUAD, TILE, 0).with_rows4().grid(64, 64), false, false, "trace_packet_quad_kernel<false, false> 8x256 lds=0", true},
	{"QUAD any-hit counting", P(K_QUAD, TILE, 0).with_rows4().grid(130, 66), true, true, "trace_packet_quad_kernel<true, true> 20x256 lds=0", true},
	{"QUAD not built", P(K_QUAD, TILE, 0).with_rows4().grid(64, 64), false, false, "trace_packet_asm_kernel<false, false, true> 16x256 lds=0", false},
	{"QUAD without row_array4", P(K_QUAD, TILE, 0).with_rows().grid(64, 64), false, false, "trace_packet_asm_kernel<false, false, true> 16x256 lds=0", true},
	{"QUAD without row_array4, not built", P(K_QUAD, TILE, 0).grid(64, 64), true, false, "trace_packet_asm_kernel<true, false, true> 16x256 lds=0", false},
	{"QUAD not built past kAsmNodeLimit", P(K_QUAD, TILE, 0).with_rows4().grid(64, 64).nodes(kAsmNodeLimit), false, false, "trace_packet_kernel<false, false> 16x256 lds=0", false},
	// ---- node offsets past the asm loop's 32 bits: the C++ packet kernel
	{"ASM one node below kAsmNodeLimit", P(K_ASM, TILE, 0).grid(64, 64).nodes(kAsmNodeLimit - 1u), false, false, "trace_packet_asm_kernel<false, false, true> 16x256 lds=0"},
	{"ASM at kAsmNodeLimit", P(K_ASM, TILE, 0).grid(64, 64).nodes(kAsmNodeLimit), false, false, "trace_packet_kernel<false, false> 16x256 lds=0"},
	{"DUAL without rows at kAsmNodeLimit", P(K_DUAL, TILE, 0).grid(64, 64).nodes(kAsmNodeLimit), true, true, "trace_packet_kernel<true, true> 16x256 lds=0"},
	{"ROWS without rows at kAsmNodeLimit", P(K_ROWS, TILE, 0).grid(64, 64).nodes(kAsmNodeLimit), false, true, "trace_packet_kernel<false, true> 16x256 lds=0"},
	{"PACKET", P(K_PKT, TILE, 0).grid(64, 64), false, false, "trace_packet_kernel<false, false> 16x256 lds=0"},
	{"PACKET any-hit counting", P(K_PKT, LIN, 4096), true, true, "trace_packet_kernel<true, true> 16x256 lds=0"},
	// ---- the asm kernel's prefetch: up to kPrefetchMaxWaves waves, counted three ways; never when counting
	{"ASM linear, kPrefetchMaxWaves", P(K_ASM, LIN, kPrefetchRays + 63u), false, false, "trace_packet_asm_kernel<false, false, true> 2561x256 lds=0"},
	{"ASM linear, one wave more", P(K_ASM, LIN, kPrefetchRays + 64u), false, false, "trace_packet_asm_kernel<false, false> 2561x256 lds=0"},
	{"ASM grid, kPrefetchMaxWaves tiles", P(K_ASM, TILE, 0).grid(1280, 512), true, false, "trace_packet_asm_kernel<true, false, true> 2560x256 lds=0"},
	{"ASM grid, one column of tiles more", P(K_ASM, TILE, 0).grid(1288, 512), true, false, "trace_packet_asm_kernel<true, false> 2576x256 lds=0"},
	{"ASM width found, kPrefetchMaxWaves", P(K_ASM, FOUND, kPrefetchRays), false, false, "trace_packet_asm_kernel<false, false, true> 2560x256 lds=0"},
	{"ASM width found, one ray more", P(K_ASM, FOUND, kPrefetchRays + 1u), false, false, "trace_packet_asm_kernel<false, false> 2561x256 lds=0"},
	{"ASM scheduled, kPrefetchMaxWaves units", P(K_ASM, TILE, 0).grid(1280, 512).sched(kPrefetchMaxWaves, 1, false), false, false, "trace_packet_asm_kernel<false, false, true> 2560x256 lds=0"},
	{"ASM scheduled, one unit more", P(K_ASM, TILE, 0).grid(616, 1064).sched(kPrefetchMaxWaves + 1u, 1, false), false, false, "trace_packet_asm_kernel<false, false> 2561x256 lds=0"},
	{"ASM scheduled in pieces, a round of slots", P(K_ASM, TILE, 0).grid(640, 360).sched(3600, 1, true), false, false, "trace_packet_asm_kernel<false, false, true> 2048x256 lds=0"},
	{"ASM scheduled in pieces, units past a round", P(K_ASM, TILE, 0).grid(1280, 512).sched(kPrefetchMaxWaves, 1, true), false, false, "trace_packet_asm_kernel<false, false, true> 3840x256 lds=0"},
	{"ASM scheduled, width found, kPrefetchMaxWaves", P(K_ASM, FOUND, kPrefetchRays).sched(kPrefetchMaxWaves, 1, false), false, false, "trace_packet_asm_kernel<false, false, true> 2560x256 lds=0"},
	{"ASM scheduled, width found, one ray more", P(K_ASM, FOUND, kPrefetchRays + 1u).sched(kPrefetchMaxWaves, 1, false), false, false, "trace_packet_asm_kernel<false, false> 2561x256 lds=0"},
	{"ASM counting", P(K_ASM, TILE, 0).grid(64, 64), false, true, "trace_packet_asm_kernel<false, true> 16x256 lds=0"},
	{"ASM any-hit counting", P(K_ASM, TILE, 0).grid(64, 64), true, true, "trace_packet_asm_kernel<true, true> 16x256 lds=0"},
	// ---- every tile in quarters or sixteenths
	{"quarters, grid", P(K_ASM, TILE, 0).grid(64, 64).quarter(1), false, false, "trace_packet_asm_kernel<false, false, true> 64x256 lds=0"},
	{"sixteenths, grid", P(K_ASM, TILE, 0).grid(64, 64).quarter(2), false, false, "trace_packet_asm_kernel<false, false, true> 256x256 lds=0"},
	{"quarters, clipped grid", P(K_ASM, TILE, 0).grid(130, 66).quarter(1), false, false, "trace_packet_asm_kernel<false, false, true> 153x256 lds=0"},
	{"quarters, width found", P(K_ASM, FOUND, 4096).quarter(1), false, false, "trace_packet_asm_kernel<false, false, true> 64x256 lds=0"},
	{"sixteenths, width found", P(K_ASM, FOUND, 4096).quarter(2), false, false, "trace_packet_asm_kernel<false, false, true> 256x256 lds=0"},
	{"sixteenths, two-level packets", P(K_TLPKT, TILE, 0).grid(64, 64).quarter(2), false, false, "trace_two_level_packet_kernel<false> 256x256 lds=0"},
	{"quarters mean nothing to linear lanes", P(K_LANE, LIN, 4096).quarter(1), false, false, "trace_lane_kernel<false, false> 16x256 lds=24576"},
	// ---- a small batch on emptier waves
	{"sparse lanes 1", P(K_LANE, LIN, 1000).sparse(1), false, false, "trace_lane_kernel<false, false> 250x256 lds=24576"},
	{"sparse lanes 2", P(K_LANE, LIN, 1000).sparse(2), false, false, "trace_lane_kernel<false, false> 125x256 lds=24576"},
	{"sparse lanes 4", P(K_LANE, LIN, 1001).sparse(4), true, false, "trace_lane_kernel<true, false> 63x256 lds=24576"},
	{"sparse lanes 4, two-level", P(K_TL, LIN, 1001).sparse(4), false, false, "trace_two_level_kernel<false> 63x256 lds=24576"},
	{"sparse lanes mean nothing to tiles", P(K_LANE, TILE, 0).grid(64, 64).sparse(4), false, true, "trace_lane_kernel<false, true> 16x256 lds=24576"},
	// ---- launches from a tile schedule: schedule_slots slots of tile_unit tiles
	{"scheduled 640x360, whole units", P(K_ASM, TILE, 0).grid(640, 360).sched(3600, 1, false), false, false, "trace_packet_asm_kernel<false, false, true> 900x256 lds=0"},
	{"scheduled 640x360, pieces", P(K_ASM, TILE, 0).grid(640, 360).sched(3600, 1, true), true, false, "trace_packet_asm_kernel<true, false, true> 2048x256 lds=0"},
	{"scheduled 2048x2048 DUAL, whole units", P(K_DUAL, TILE, 0).with_rows().grid(2048, 2048).sched(32768, 2, false), false, false, "trace_packet_rows_kernel<false, false, 2, 64, true> 32768x64 lds=0 group=2"},
	{"scheduled 2048x2048 DUAL, pieces", P(K_DUAL, TILE, 0).with_rows().grid(2048, 2048).sched(32768, 2, true), false, false, "trace_packet_rows_kernel<false, false, 2, 64, true> 49152x64 lds=0 group=2"},
	{"a schedule without its header is not used", P(K_ASM, TILE, 0).grid(640, 360).sched(100, 1, false, false), false, false, "trace_packet_asm_kernel<false, false, true> 900x256 lds=0"},
	{"scheduled from a narrower grid, width found", P(K_ASM, FOUND, 230400).sched(100, 1, false), false, false, "trace_packet_asm_kernel<false, false, true> 900x256 lds=0"},
	{"scheduled from this grid, width found", P(K_DUAL, FOUND, 2048u * 2048u).with_rows().sched(32768, 2, true), false, false, "trace_packet_rows_kernel<false, false, 2, 64, false> 49152x64 lds=0 group=2"},
	// ---- two-level scenes, the lane kernel
	{"two-level packets", P(K_TLPKT, TILE, 0).grid(64, 64).lds(4096), true, true, "trace_two_level_packet_kernel<true> 16x256 lds=4096"},
	{"two-level lanes", P(K_TL, FOUND, 4096), false, true, "trace_two_level_kernel<false> 16x256 lds=24576"},
	{"lanes", P(K_LANE, LIN, 4097), false, false, "trace_lane_kernel<false, false> 17x256 lds=24576"},
	{"lanes any-hit counting", P(K_LANE, FOUND, 4096), true, true, "trace_lane_kernel<true, true> 16x256 lds=24576"},
	{"a persistent id launched plain", P(K_LP, TILE, 0).grid(64, 64), false, false, "trace_lane_kernel<false, false> 16x256 lds=24576"},
	// ---- nothing to launch; too much to launch
	{"no rays", P(K_LANE, LIN, 0), false, false, "nothing"},
	{"no rows", P(K_ASM, TILE, 0).grid(64, 0), false, false, "nothing"},
	{"2^31 - 1 workgroups", P(K_LANE, LIN, kMaxBlockRays), false, false, "trace_lane_kernel<false, false> 2147483647x256 lds=24576"},
	{"2^31 workgroups", P(K_LANE, LIN, kMaxBlockRays + 1u), false, false, "error"},
	{"2^31 - 1 workgroups of lanes, half the waves", P(K_DUAL, LIN, kMaxBlockRays).with_rows(), false, false, "trace_packet_rows_kernel<false, false, 2, 64, false> 4294967294x64 lds=0 group=2"},
	{"2^31 workgroups of sparse lanes", P(K_LANE, LIN, 1ull << 33).sparse(1), false, false, "error"},
	{"2^31 workgroups of sixteenths", P(K_ASM, FOUND, 1ull << 35).quarter(2), false, false, "error"},
};

// launch_trace_persistent (kPersistent) and launch_source (kSource: named as a hemisphere cast from a grid, the family with both modes)
struct Resident {
	const char *name;
	P p;
	uint32_t lds_depth, blocks;
	bool any_hit, count;
	const char *want;
};
const Resident kPersistent[] = {
	{"LP", P(K_LP, LIN, 100000), 16, 391, false, false, "trace_lane_persistent_kernel<false, 2, false, false> 391x256 lds=16384"},
	{"LP any-hit counting", P(K_LP, LIN, 100000).with_nodes4().with_nodes8(), 16, 391, true, true, "trace_lane_persistent_kernel<true, 2, false, true> 391x256 lds=16384"},
	{"L4P", P(K_L4P, LIN, 100000).with_nodes4().with_nodes8(), 16, 391, true, false, "trace_lane_persistent_kernel<true, 4, false, false> 391x256 lds=16384"},
	{"L4P counting", P(K_L4P, LIN, 100000).with_nodes4(), 8, 2048, false, true, "trace_lane_persistent_kernel<false, 4, false, true> 2048x256 lds=8192"},
	{"L4P without the 4-wide nodes", P(K_L4P, LIN, 100000).with_nodes8(), 16, 391, false, false, "trace_lane_persistent_kernel<false, 2, false, false> 391x256 lds=16384"},
	{"L8P", P(K_L8P, LIN, 100000).with_nodes4().with_nodes8(), 32, 1280, false, false, "trace_lane_persistent_kernel<false, 8, false, false> 1280x256 lds=32768"},
	{"L8P any-hit counting", P(K_L8P, LIN, 100000).with_nodes8(false), 16, 391, true, true, "trace_lane_persistent_kernel<true, 8, false, true> 391x256 lds=16384"},
	{"L8P without the 8-wide nodes", P(K_L8P, LIN, 100000).with_nodes4(), 16, 391, false, true, "trace_lane_persistent_kernel<false, 2, false, true> 391x256 lds=16384"},
	{"TLP", P(K_TLP, LIN, 100000).with_nodes8(), 16, 391, false, false, "trace_lane_persistent_kernel<false, 2, true, false> 391x256 lds=16384"},
	{"TLP any-hit, no counting form", P(K_TLP, LIN, 100000), 16, 391, true, true, "trace_lane_persistent_kernel<true, 2, true, false> 391x256 lds=16384"},
	{"TLP8", P(K_TLP8, LIN, 100000).with_nodes8(), 16, 391, false, false, "trace_lane_persistent_kernel<false, 8, true, false> 391x256 lds=16384"},
	{"TLP8 any-hit, no counting form", P(K_TLP8, LIN, 100000).with_nodes8(), 16, 391, true, true, "trace_lane_persistent_kernel<true, 8, true, false> 391x256 lds=16384"},
	{"TLP8 without leaf boxes", P(K_TLP8, LIN, 100000).with_nodes8(false), 16, 391, false, false, "trace_lane_persistent_kernel<false, 2, true, false> 391x256 lds=16384"},
	{"TLP8 without the 8-wide nodes", P(K_TLP8, LIN, 100000), 16, 391, true, false, "trace_lane_persistent_kernel<true, 2, true, false> 391x256 lds=16384"},
	{"a plain id launched persistent", P(K_TL, LIN, 100000).with_nodes8(), 16, 391, false, true, "trace_lane_persistent_kernel<false, 2, false, true> 391x256 lds=16384"},
	{"no rays", P(K_LP, LIN, 0), 16, 391, false, false, "nothing"},
	{"no workgroups", P(K_LP, LIN, 100000), 16, 0, false, false, "nothing"},
};
const Resident kSource[] = {
	{"lanes", P(K_LANE, LIN, 40000), 0, 0, true, false, "trace_hemisphere_lane_kernel<9, true> 157x256 lds=24576"},
	{"sparse lanes", P(K_LANE, LIN, 1001).sparse(4), 0, 0, false, false, "trace_hemisphere_lane_kernel<9, false> 63x256 lds=24576"},
	{"two-level lanes", P(K_TL, LIN, 40000), 0, 0, true, false, "trace_hemisphere_two_level_kernel<9, true> 157x256 lds=24576"},
	{"LP", P(K_LP, LIN, 100000), 16, 391, false, false, "trace_hemisphere_persistent_kernel<9, false, 2, false> 391x256 lds=16384"},
	{"L4P", P(K_L4P, LIN, 100000).with_nodes4(), 16, 391, true, false, "trace_hemisphere_persistent_kernel<9, true, 4, false> 391x256 lds=16384"},
	{"L4P without the 4-wide nodes", P(K_L4P, LIN, 100000), 16, 391, true, false, "trace_hemisphere_persistent_kernel<9, true, 2, false> 391x256 lds=16384"},
	{"L8P", P(K_L8P, LIN, 100000).with_nodes8(), 16, 391, true, false, "trace_hemisphere_persistent_kernel<9, true, 8, false> 391x256 lds=16384"},
	{"L8P without the 8-wide nodes", P(K_L8P, LIN, 100000).with_nodes4(), 16, 391, false, false, "trace_hemisphere_persistent_kernel<9, false, 2, false> 391x256 lds=16384"},
	{"TLP", P(K_TLP, LIN, 100000).with_nodes8(), 16, 391, false, false, "trace_hemisphere_persistent_kernel<9, false, 2, true> 391x256 lds=16384"},
	{"TLP8", P(K_TLP8, LIN, 100000).with_nodes8(), 16, 391, true, false, "trace_hemisphere_persistent_kernel<9, true, 8, true> 391x256 lds=16384"},
	{"TLP8 without leaf boxes", P(K_TLP8, LIN, 100000).with_nodes8(false), 16, 391, false, false, "trace_hemisphere_persistent_kernel<9, false, 2, true> 391x256 lds=16384"},
	{"a plain two-level id launched persistent", P(K_TL, LIN, 100000).with_nodes8(), 16, 391, false, false, "trace_hemisphere_persistent_kernel<9, false, 2, true> 391x256 lds=16384"},
	{"no entries", P(K_LANE, LIN, 0), 16, 391, false, false, "nothing"},
	{"2^31 - 1 workgroups", P(K_LANE, LIN, kMaxBlockRays), 0, 0, false, false, "trace_hemisphere_lane_kernel<9, false> 2147483647x256 lds=24576"},
	{"2^31 workgroups", P(K_LANE, LIN, kMaxBlockRays + 1u), 0, 0, false, false, "error"},
	{"2^31 workgroups of sparse lanes", P(K_TL, LIN, 1ull << 33).sparse(1), 0, 0, false, false, "error"},
	{"2^31 workgroups of entries, persistent", P(K_LP, LIN, kMaxBlockRays + 1u), 16, 2048, false, false, "trace_hemisphere_persistent_kernel<9, false, 2, false> 2048x256 lds=16384"},
};

void launches()
{
	for (const Launch &t : kTrace) {
		const TraceLaunch l = resolve_trace(t.p, t.any_hit, t.count, t.quad_built);
		const std::string got = describe(l);
		expect(got == t.want, std::string("launch_trace, ") + t.name + ": got \"" + got + "\", want \"" + t.want + "\"");
		covers(std::string("launch_trace, ") + t.name, t.p, l);
	}
	for (const Resident &t : kPersistent) {
		const std::string got = describe(resolve_persistent(t.p, t.lds_depth, t.blocks, t.any_hit, t.count));
		expect(got == t.want, std::string("launch_trace_persistent, ") + t.name + ": got \"" + got + "\", want \"" + t.want + "\"");
	}
	for (const Resident &t : kSource) {
		const TraceLaunch l = resolve_source(t.p, t.lds_depth, t.blocks, t.any_hit);
		const std::string got = describe(l, "hemisphere", SRC_HEMI_GRID, true);
		expect(got == t.want, std::string("launch_source, ") + t.name + ": got \"" + got + "\", want \"" + t.want + "\"");
		covers(std::string("launch_source, ") + t.name, t.p, l);
	}
	// a build with MRT_ROWS_WG_LARGE = 64 has one workgroup size
	const P dual = P(K_DUAL, TILE, 0).with_rows().grid(64, 64).wg(256);
	expect(describe(resolve_trace(dual, false, false, false, 64u)) == "trace_packet_rows_kernel<false, false, 2, 64, true> 32x64 lds=0 group=2", "launch_trace, MRT_ROWS_WG_LARGE 64: " + describe(resolve_trace(dual, false, false, false, 64u)));
	// the names of record-driven casts: a family with one mode does not print it
	const auto name = [](const TraceLaunch &l, const char *family, int src, bool with_mode) {
		char b[96];
		format_variant(b, sizeof(b), l.v, family, src, with_mode);
		return std::string(b);
	};
	const TraceLaunch plain = resolve_source(P(K_LANE, LIN, 4096), 0, 0, true), tl = resolve_source(P(K_TL, LIN, 4096), 0, 0, false);
	const TraceLaunch wide = resolve_source(P(K_L8P, LIN, 100000).with_nodes8(), 16, 391, true), tlp = resolve_source(P(K_TLP, LIN, 100000), 16, 391, false);
	expect(name(plain, "shadow", SRC_SHADOW_GRID, false) == "trace_shadow_lane_kernel<3>", "names: " + name(plain, "shadow", SRC_SHADOW_GRID, false));
	expect(name(tl, "reflection", SRC_REFLECT_RAY32, false) == "trace_reflection_two_level_kernel<4>", "names: " + name(tl, "reflection", SRC_REFLECT_RAY32, false));
	expect(name(wide, "hemisphere", SRC_HEMI_GRID, true) == "trace_hemisphere_persistent_kernel<9, true, 8, false>", "names: " + name(wide, "hemisphere", SRC_HEMI_GRID, true));
	expect(name(tlp, "bounce", SRC_BOUNCE_HOST, false) == "trace_bounce_persistent_kernel<11, 2, true>", "names: " + name(tlp, "bounce", SRC_BOUNCE_HOST, false));
	expect(name(wide, "shadow", SRC_SHADOW_RAY32, false) == "trace_shadow_persistent_kernel<1, 8, false>", "names: " + name(wide, "shadow", SRC_SHADOW_RAY32, false));
	expect(name(tl, "hemisphere", SRC_HEMI_HOST, true) == "trace_hemisphere_two_level_kernel<8, false>", "names: " + name(tl, "hemisphere", SRC_HEMI_HOST, true));
	// a name that does not fit is cut, never written past its buffer
	char small[16];
	format_variant(small, sizeof(small), wide.v, "hemisphere", SRC_HEMI_GRID, true);
	expect(std::string(small) == "trace_hemispher", std::string("names: cut to the buffer: ") + small);
}

// 15 frames of one 1280x960 grid: frames 0-3 the 64-ray kernel, 4-7 the 128-ray walk in pieces, 8-11 whole; the last two of every
// candidate are timed, waiting for the sorts; from frame 12 the fastest (the faster of its two timed frames)
void tuner(const char *name, const float ms[12], const char *final_want)
{
	GridStates gs;
	const Case grid{name, AUTO, FLAT, ENTRY_GRID, 0, 0, 1280, 960, 0, 960, NONE, ""};
	static const char *want[12] = {"asm+pieces", "asm+pieces", "asm+pieces+wait", "asm+pieces+wait", "dual+pieces", "dual+pieces",
		"dual+pieces+wait", "dual+pieces+wait", "dual", "dual", "dual+wait", "dual+wait"};
	for (int f = 0; f < 15; f++) {
		const CastPlan c = plan(grid, gs);
		char got[64];
		std::snprintf(got, sizeof(got), "%s%s%s", kname(c.kernel), c.pieces ? "+pieces" : "", c.wait_sorts ? "+wait" : "");
		const std::string w = f < 12 ? want[f] : final_want;
		expect(got == w && c.arms_tuner == (f < 12) && c.scheduled, std::string(name) + " frame " + std::to_string(f) + ": got " + got + ", want " + w);
		tune_record(gs.tune(), f < 12 ? ms[f] : 0.1f);
		if (f == 5) { // an ASYNC frame has no timing: it takes the phase's kernel and leaves the phase where it is
			Case a = grid; a.flags = ASYNC;
			const CastPlan ca = plan(a, gs);
			expect(!ca.arms_tuner && ca.kernel == MRT_KERNEL_PACKET_DUAL && gs.tune().phase == 6, std::string(name) + ": ASYNC frame");
			tune_record(gs.tune(), 9.0f);
			expect(gs.tune().phase == 6, std::string(name) + ": ASYNC frame advanced the phase");
		}
	}
}

// per grid and mode: eight states, the least recently used one goes
void lru()
{
	GridStates gs;
	const Case a{"lru", AUTO, FLAT, ENTRY_GRID, 0, 0, 1280, 960, 0, 960, NONE, ""};
	auto other = [&](uint32_t k) { Case c = a; c.w = 1280 + 8 * k; return c; };
	for (int f = 0; f < 5; f++) { plan(a, gs); tune_record(gs.tune(), 1.0f); } // phase 5
	for (uint32_t k = 1; k <= 7; k++) plan(other(k), gs);                      // seven more grids: a is still held
	CastPlan c = plan(a, gs);
	expect(c.kernel == MRT_KERNEL_PACKET_DUAL && c.pieces && gs.tune().phase == 5, "lru: grid a kept among eight");
	Case any = a; // the same grid in any-hit mode is a state of its own
	CastRequest r; r.entry = ENTRY_GRID; r.count = 1280u * 960u; r.grid_w = 1280; r.grid_h = 960; r.rows = 960; r.mode = MRT_MODE_ANY_HIT;
	c = plan_cast(options(any.opt), scene(FLAT), r, PrevDetect(), Knobs(), gs);
	expect(c.kernel == MRT_KERNEL_PACKET_ASM && gs.tune().phase == 0 && gs.e[gs.cur].key.mode == MRT_MODE_ANY_HIT, "lru: any-hit mode has its own state");
	const int slot_of_other1 = [&] { for (int i = 0; i < GridStates::kCount; i++) if (gs.e[i].key.w == 1288) return i; return -1; }();
	expect(slot_of_other1 < 0, "lru: the any-hit state evicted the oldest (grid 1)");
	plan(a, gs); // a: most recent again
	for (uint32_t k = 10; k <= 17; k++) plan(other(k), gs); // eight new grids: a is the oldest by the eighth
	c = plan(a, gs);
	expect(c.kernel == MRT_KERNEL_PACKET_ASM && gs.tune().phase == 0, "lru: grid a evicted after eight others");
	GridStates g2;
	for (uint32_t k = 0; k < 8; k++) select_grid_state(g2, GridKey{100 + k, 1, 0, 1, 0});
	select_grid_state(g2, GridKey{100, 1, 0, 1, 0});
	const int at = select_grid_state(g2, GridKey{200, 1, 0, 1, 0});
	expect(at == 1 && g2.e[0].key.w == 100, "lru: select_grid_state evicts the least recently used");
}

// Sequences of casts against a fake stream: a queued detect writes its words only when the host waits (the worst case for the
// planner: ASYNC casts, pipeline chunks and submits queued behind a long cast).  Rays are w x h grids (COHERENT), or not a grid.
struct Seq {
	GridStates gs;
	DetectMemo memo;
	Knobs k;
	uint32_t h_auto[4] = {0, 0, 0, 0};               // what the device has written so far
	std::vector<std::array<uint32_t, 4>> in_flight;  // detects queued, not run
	CastRequest req(Entry e, uint64_t n, uint32_t flags) const
	{
		CastRequest r; r.entry = e; r.count = n; r.flags = flags; r.mode = MRT_MODE_NEAREST;
		return r;
	}
	// the plan the rule before DetectMemo made: the count of the last cast queued, the words as they are now
	PrevDetect racy() const
	{
		PrevDetect p; p.count = memo.queued_count;
		for (int i = 0; i < 4; i++) p.word[i] = h_auto[i];
		return p;
	}
	CastPlan cast(Entry e, uint32_t w, uint32_t h, uint32_t flags = COH, bool grid = true)
	{
		const CastRequest r = req(e, (uint64_t)w * h, flags);
		const CastPlan c = plan_cast(options(AUTO), scene(FLAT), r, memo.prev(), k, gs);
		memo.queued(c.detect, r.count);
		if (c.detect) in_flight.push_back(grid ? std::array<uint32_t, 4>{w, h, w / 8u, 0u} : std::array<uint32_t, 4>{0u, 0u, 0u, 1u});
		return c;
	}
	void wait()
	{
		for (const auto &q : in_flight) std::memcpy(h_auto, q.data(), sizeof(h_auto));
		in_flight.clear();
		memo.waited(h_auto);
	}
	CastPlan blocking(uint32_t w, uint32_t h) { const CastPlan c = cast(ENTRY_CAST, w, h); wait(); return c; }
};

std::string sched(const CastPlan &c)
{
	if (!c.scheduled) return "-";
	return std::to_string(c.grid_w) + "x" + std::to_string(c.rows) + "/" + std::to_string(c.tiles_x);
}

void memo()
{
	constexpr uint32_t DEV = MRT_FLAG_RAYS_ON_DEVICE | MRT_FLAG_HITS_ON_DEVICE;
	{   // blocking A until scheduled, then two ASYNC casts B1, B2 of another grid and as many rays as each other
		Seq s;
		expect(sched(s.blocking(640, 360)) == "-", "memo: the first cast of A has no width to go by");
		const CastPlan a = s.blocking(640, 360);
		expect(sched(a) == "640x360/80", "memo: A from A's width: " + sched(a));
		expect(sched(s.cast(ENTRY_CAST, 1280, 960, COH | ASYNC)) == "-", "memo: ASYNC B1");
		// B1's detect has not run: the count is B's, the words are still A's
		expect(s.racy().count == 1228800u && s.racy().word[0] == 640u, "memo: the race is set up");
		GridStates g2 = s.gs;
		const CastPlan old = plan_cast(options(AUTO), scene(FLAT), s.req(ENTRY_CAST, 1228800, COH | ASYNC), s.racy(), s.k, g2);
		expect(sched(old) == "640x360/80", "memo: the rule it replaces scheduled B2 from A's width: " + sched(old));
		const CastPlan b2 = s.cast(ENTRY_CAST, 1280, 960, COH | ASYNC);
		expect(sched(b2) == "-", "memo: ASYNC B2 is not scheduled from A: " + sched(b2));
		s.wait(); // mrt_synchronize
		expect(s.memo.prev().count == 1228800u && s.memo.prev().word[0] == 1280u && s.memo.prev().word[1] == 960u, "memo: after the wait, B's pair");
		expect(sched(s.cast(ENTRY_CAST, 1280, 960, COH | ASYNC)) == "1280x960/160", "memo: ASYNC B3 from B's own width");
		expect(sched(s.cast(ENTRY_CAST, 1280, 960, COH | ASYNC)) == "1280x960/160", "memo: ASYNC B4 from the same pair");
		s.wait();
		expect(sched(s.blocking(640, 360)) == "-", "memo: A after B: B's count");
		expect(sched(s.blocking(640, 360)) == "640x360/80", "memo: A again");
	}
	{   // blocking 1024x576 casts, then a host cast of 2048x1152 in 2^20-ray chunks (2048 x 512, 2048 x 512, 2048 x 128)
		Seq s;
		for (int f = 0; f < 3; f++) s.blocking(1024, 576);
		const uint32_t rows[3] = {512, 512, 128};
		for (int k = 0; k < 3; k++) {
			GridStates g2 = s.gs;
			const CastPlan old = plan_cast(options(AUTO), scene(FLAT), s.req(ENTRY_CHUNK, 2048ull * rows[k], COH | DEV), s.racy(), s.k, g2);
			if (k == 1) expect(sched(old) == "1024x576/128", "memo: the rule it replaces scheduled chunk 1 from 1024x576: " + sched(old));
			const CastPlan c = s.cast(ENTRY_CHUNK, 2048, rows[k], COH | DEV);
			expect(c.detect && sched(c) == "-", "memo: chunk " + std::to_string(k) + " not scheduled from a width of the queue: " + sched(c));
		}
		s.wait(); // the end of the pipelined cast
		expect(s.memo.prev().count == 262144u && s.memo.prev().word[0] == 2048u && s.memo.prev().word[1] == 128u, "memo: after the pipeline, the tail chunk's pair");
		expect(sched(s.cast(ENTRY_CHUNK, 2048, 128, COH | DEV)) == "2048x128/256", "memo: a chunk of the tail's size from the tail's width");
		s.wait();
	}
	{   // submit and collect between blocking casts of other sizes
		Seq s;
		s.blocking(1280, 960);
		const CastPlan sub = s.cast(ENTRY_SUBMIT, 640, 360);
		expect(sched(sub) == "-", "memo: a submit of A after B");
		expect(s.memo.prev().word[0] == 1280u, "memo: a submit in flight leaves the pair of the last wait");
		s.wait(); // mrt_collect
		expect(sched(s.cast(ENTRY_SUBMIT, 640, 360)) == "640x360/80", "memo: the next submit from the collected one's width");
		s.wait();
		expect(sched(s.blocking(640, 360)) == "640x360/80", "memo: a blocking cast after a collect");
	}
	{   // casts without a detect between: an incoherent batch queued last leaves no width; grid casts and shadow casts queue none
		Seq s;
		s.blocking(640, 360); s.blocking(640, 360);
		const CastPlan inc = s.cast(ENTRY_CAST, 640, 360, 0u);
		expect(!inc.detect && inc.sort, "memo: an incoherent batch runs no detect");
		s.wait();
		expect(s.memo.prev().count == 0u, "memo: the last cast queued had no detect: no width");
		expect(sched(s.blocking(640, 360)) == "-", "memo: A after the incoherent batch");
		expect(sched(s.blocking(640, 360)) == "640x360/80", "memo: A after A");
		s.cast(ENTRY_CAST, 640, 360, ASYNC);                        // queued without a detect, no wait: the pair stays A's
		expect(sched(s.cast(ENTRY_CAST, 640, 360, COH | ASYNC)) == "640x360/80", "memo: ASYNC A behind a cast without detect");
		s.wait();
		s.memo.waited(s.h_auto);                                     // a grid cast (no detect queued) waits: nothing changes
		expect(s.memo.prev().count == 230400u && s.memo.prev().word[0] == 640u, "memo: a wait with nothing queued changes nothing");
		s.cast(ENTRY_CAST, 640, 360, COH | ASYNC, false);             // not a grid after all
		s.wait();
		expect(s.memo.prev().count == 230400u && s.memo.prev().word[0] == 0u && s.memo.prev().word[3] == 1u, "memo: no width found");
		expect(sched(s.blocking(640, 360)) == "-", "memo: no schedule from a batch in which no width was found");
	}
}

} // namespace

int main()
{
	table();
	launches();
	const float pieces_win[12] = {0, 0, 0.40f, 0.38f, 0, 0, 0.35f, 0.36f, 0, 0, 0.37f, 0.38f};   // whole 0.37 > 1.03 x 0.35
	const float whole_wins[12] = {0, 0, 0.40f, 0.38f, 0, 0, 0.35f, 0.36f, 0, 0, 0.36f, 0.361f};  // whole 0.36 <= 1.03 x 0.35
	const float asm_wins[12] = {0, 0, 0.30f, 0.31f, 0, 0, 0.35f, 0.36f, 0, 0, 0.36f, 0.37f};
	tuner("tuner, pieces win", pieces_win, "dual+pieces");
	tuner("tuner, whole wins", whole_wins, "dual");
	tuner("tuner, 64-ray kernel wins", asm_wins, "asm+pieces");
	lru();
	memo();
	std::printf("%d of %d checks hold (%zu table cases)\n", checks - failures, checks, sizeof(kCases) / sizeof(kCases[0]));
	return failures ? 1 : 0;
}
