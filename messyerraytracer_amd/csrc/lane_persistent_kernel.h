// lane_persistent_kernel.h — one lane = one ray, persistent waves with ray refill.
// Included by kernels.hip (inside namespace mrt, after the common helpers).
//
// For incoherent batches (config C4).  profiles/r01_c4lane: with one fixed ray per lane a
// wave executes ~540 loop iterations for rays that need ~89 (16 % SIMD efficiency: the
// wave runs until its slowest ray ends) at 5 waves per SIMD (LDS stack), 74 % of the time
// waiting on the divergent node fetches.  This kernel
//   * keeps the grid resident (waves x CUs that fit) and lets every wave pull rays from
//     one global counter: when at least `refill` lanes have finished, the wave stores
//     their hits and hands them new rays (ballot + mbcnt prefix, one atomicAdd per refill);
//   * keeps only the top `lds_depth` stack entries per lane in LDS ([depth][lane] layout)
//     and spills deeper entries to a per-lane slice of an HBM scratch buffer, so LDS no
//     longer limits occupancy (16 entries = 4 KB per wave);
//   * alternates a NODE phase and a LEAF phase under wave-uniform control: the node phase
//     steps every lane that stands at an inner node and ends as soon as `leaf_wait` lanes
//     stand at a leaf (or nobody is at an inner node); the leaf phase then intersects those
//     leaves.  The plain while-while loop of trace_lane_kernel keeps a lane that reached its
//     leaf waiting until the LAST lane of the wave has reached one: PMC counters put its node
//     steps at 11 busy lanes of 64.  Node steps are 93 % of the arithmetic of a ray and leaf
//     tests 7 %, so it pays to run the cheap leaf phase often, at low occupancy, to keep the
//     expensive node phase dense.
// The arithmetic is trace_lane_kernel's (same operations, same tie rule).
//
// WIDE4: the same walk over the 4-wide collapse of the BVH (Dev4Node, one 128-byte cache line
// per node; tools/ubench/tcp_rate.hip: a divergent fetch is paid per cache line, so a 4-wide
// node costs what a 2-wide node costs and a ray needs half as many).  Children are visited
// nearest first (sorting network on packed distance|slot keys); the order never changes a
// result.
//
// WIDTH 8: the 8-wide compressed collapse (Dev8Node: 8-bit child boxes on a per-node grid, decoded
// with fma(q, step, origin) to boxes that contain the exact ones).  Still one line per step, and a
// ray needs fewer again; the price is the decode arithmetic.
#pragma once

#define MRT_RAY_CHUNK 256u // most rays a wave reserves per atomic on a ray counter (PersistParams::chunk)

struct PersistParams {
	unsigned long long *next_ray; // 8 ray counters, one per region of the batch, 16 u64 apart (zeroed before the launch)
	uint32_t *overflow;           // [depth - lds_depth][global thread] spill area
	uint32_t overflow_stride;     // = total threads of the launch
	uint32_t lds_depth;           // stack entries per lane kept in LDS
	uint32_t refill;              // refill when at least this many lanes are idle
	uint32_t leaf_wait;           // leave the node phase when this many lanes stand at a leaf
	uint32_t chunk;               // rays a wave reserves at a time: MRT_RAY_CHUNK, less for batches that would
	                              // otherwise give a wave only a few chunks (the last ones finish unevenly)
};

// Waves per SIMD the register allocator has to leave room for.  The flat forms need 75-92 VGPRs (5-6 waves) by
// themselves; the two-level forms come to 118-125 (4 waves) and gain 6 % when held to 96 (2^22 incoherent rays
// on C5: 8.35 -> 7.8 ms).  Asking for 6 costs every form (C4 8-wide: +3 %, two-level: +8 %).
#ifndef MRT_PERSIST_WPE
#define MRT_PERSIST_WPE 5
#endif
#define MRT_PERSIST_ATTR __attribute__((amdgpu_waves_per_eu(MRT_PERSIST_WPE, 8)))

// byte k of a packed word as a float (v_cvt_f32_ubyteK)
__device__ __forceinline__ float ubyte_f(uint32_t w, int k) { return (float)((w >> (8 * k)) & 0xFFu); }

// TL: a two-level scene (two_level_kernel.h): p.nodes holds the TLAS and every BLAS, a TLAS leaf is a run of
// DevInstance rows, a lane inside an instance walks with its mesh-space ray and the marker kInstanceReturn on
// its stack takes it back to the world ray.  WIDTH 2: both levels 2-wide.  WIDTH 8: the TLAS 2-wide, every
// BLAS in the 8-wide compressed layout (p.nodes8, p.leaf_box; DevInstance::root8).
// sum of a per-lane count over the wave (counting builds)
__device__ __forceinline__ unsigned long long wave_sum(uint32_t v)
{
	unsigned long long s = v;
	for (int m = 1; m < MRT_WAVE; m <<= 1) s += __shfl_xor(s, m);
	return s;
}

// COUNT: the counting build (mrt_options.count_visits): per ray node steps (= cache lines fetched: one 64- or 128-byte
// line per step whatever the width), triangle rows tested and, for the 8-wide walk, exact leaf boxes read.
template <bool ANY_HIT, int WIDTH, bool TL = false, bool COUNT = false> // WIDTH: children per node step = 2 (DevNode), 4 (Dev4Node) or 8 (Dev8Node)
__global__ __launch_bounds__(MRT_WG) MRT_PERSIST_ATTR void trace_lane_persistent_kernel(const TraceParams p, const PersistParams q)
{
	constexpr int SRC = SRC_CAST;
	const NoSource s{};
#include "persistent_walk.inc" // (in scope: the names its first lines check)
}
