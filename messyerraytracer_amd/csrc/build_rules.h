// build_rules.h -- the rules of scene construction that the host path (host/scene_prep.cpp, host/two_level_prep.cpp) and the device
// path (device_build.hip, refit.hip, tlas_device.hip) both apply, each written once and compiled for both sides, so that the arrays
// either path writes agree bit for bit: the triangle made of three vertices, its box, the union of boxes, the re-basing of a ref, the
// greedy widening of a binary node to 4 or 8 children, the 8-bit grid of a Dev8Node.  Every operation is spelled out in the order it
// is evaluated and nothing is contracted into an fma.  csrc/host/build_rules_test.cpp holds each function to the host text it
// replaced, on random and edge inputs.
// Internal linkage (an unnamed namespace): every unit compiles its own copy, and a kernel that takes a Box keeps its name.
#pragma once
#include <cfloat>
#include <cstring>
#include <math.h>
#include "mrt_internal.h"
#ifdef __HIPCC__
#include <hip/hip_runtime.h> // for the device-only part at the end
#endif

#define MRT_NO_CONTRACT _Pragma("clang fp contract(off)") // first in a function: nothing in it is contracted into an fma
#ifndef MRT_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define MRT_HD __host__ __device__
#else
#define MRT_HD
#endif
#endif

namespace mrt {

namespace {

struct Box { float mn[3], mx[3]; };

// left then right: every union is taken in this order, so a pass that boxes a node and a pass that checks it agree bit for bit
MRT_HD inline Box unite(const Box &l, const Box &r)
{
	Box u;
	for (int k = 0; k < 3; k++) { u.mn[k] = fminf(l.mn[k], r.mn[k]); u.mx[k] = fmaxf(l.mx[k], r.mx[k]); }
	return u;
}

// the box a node row holds for its left (0) or right (1) child
MRT_HD inline Box get_side(const DevNode *row, int side)
{
	const float *mn = side ? row->rmin : row->lmin, *mx = side ? row->rmax : row->lmax;
	Box b;
	for (int k = 0; k < 3; k++) { b.mn[k] = mn[k]; b.mx[k] = mx[k]; }
	return b;
}

// order-preserving float <-> uint (for atomicMin / atomicMax on floats of either sign)
MRT_HD inline uint32_t f2ord(float f) { const uint32_t u = __builtin_bit_cast(uint32_t, f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
MRT_HD inline float ord2f(uint32_t o) { return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

// one float step towards -inf / +inf (0 -> -+FLT_MIN)
MRT_HD inline float ulp_down(float f) { return f == 0.0f ? -FLT_MIN : __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) + (f > 0.0f ? -1 : 1)); }
MRT_HD inline float ulp_up(float f) { return f == 0.0f ? FLT_MIN : __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) + (f > 0.0f ? 1 : -1)); }

MRT_HD inline size_t align256(size_t bytes) { return (bytes + 255u) & ~(size_t)255u; } // arenas are carved in 256-byte steps

// The Triangle ctor (src/core/triangle.h:41-51): v0, the two edges, their cross product normalized() as godot::Vector3 does it (zero
// stays zero, otherwise divide by the length), the id and the layer mask; both pads zero.
MRT_HD inline mrt_tri64 make_tri64(const float a[3], const float b[3], const float c[3], uint32_t id, uint32_t layers)
{
	MRT_NO_CONTRACT
	mrt_tri64 t;
	for (int k = 0; k < 3; k++) { t.v0[k] = a[k]; t.edge1[k] = b[k] - a[k]; t.edge2[k] = c[k] - a[k]; }
	float *n = t.normal;
	n[0] = t.edge1[1] * t.edge2[2] - t.edge1[2] * t.edge2[1];
	n[1] = t.edge1[2] * t.edge2[0] - t.edge1[0] * t.edge2[2];
	n[2] = t.edge1[0] * t.edge2[1] - t.edge1[1] * t.edge2[0];
	const float l2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
	if (l2 == 0.0f) { n[0] = n[1] = n[2] = 0.0f; }
	else { const float l = __builtin_sqrtf(l2); n[0] /= l; n[1] /= l; n[2] /= l; }
	t.id = id; t.layers = layers; t.pad2 = 0.0f; t.pad3 = 0.0f;
	return t;
}

// The box of a triangle on the device: the vertices v0, v0 + e1, v0 + e2 as the intersection test sees them, one ulp outwards
// (v0 + e1 is a rounded sum, the true vertex may lie half an ulp outside it).
MRT_HD inline Box tri_box(const float v0[3], const float e1[3], const float e2[3])
{
	MRT_NO_CONTRACT
	Box bx;
	for (int k = 0; k < 3; k++) {
		const float p1 = v0[k] + e1[k], p2 = v0[k] + e2[k];
		bx.mn[k] = ulp_down(fminf(v0[k], fminf(p1, p2)));
		bx.mx[k] = ulp_up(fmaxf(v0[k], fmaxf(p1, p2)));
	}
	return bx;
}

// A ref of a tree built on its own (nodes and slots from 0) at its place in a larger array; the sentinel stays.
MRT_HD inline uint32_t rebase_ref(uint32_t ref, uint32_t node_base, uint32_t tri_base) { return ref < kSentinel ? ref + node_base : (ref >= kLeafBit ? (kLeafBit | ((ref & 0x7FFFFFFFu) + tri_base)) : ref); }

// The children of a wide node while it is put together: box[i] = child i's exact box {min xyz, max xyz}, ref[i] its DevNode ref (two
// arrays, not one of structs: the device compiler keeps each in registers).  The two children of node g into the slots at_l, at_r:
MRT_HD inline void take_children(const DevNode &g, float (*box)[6], uint32_t *ref, uint32_t at_l, uint32_t at_r)
{
	for (int c = 0; c < 3; c++) {
		box[at_l][c] = g.lmin[c]; box[at_l][3 + c] = g.lmax[c];
		box[at_r][c] = g.rmin[c]; box[at_r][3 + c] = g.rmax[c];
	}
	ref[at_l] = g.left_ref; ref[at_r] = g.right_ref;
}

// The widening of a binary node to N children: slots 0 and 1 hold its two children; keep opening the internal child with the
// largest half-area (the first of equals; its left child takes its slot, its right child the next free one) until there are N or
// only leaves remain.  node_of(ref) is the binary node ref.  Returns the number of children.
template <uint32_t N, class F> MRT_HD inline uint32_t open_widest(float (&box)[N][6], uint32_t (&ref)[N], F node_of)
{
	MRT_NO_CONTRACT
	uint32_t n = 2;
	while (n < N) {
		int best = -1; float best_a = -1.0f;
		for (uint32_t i = 0; i < n; i++) {
			if (ref[i] >= kSentinel) continue; // a leaf
			const float e0 = box[i][3] - box[i][0], e1 = box[i][4] - box[i][1], e2 = box[i][5] - box[i][2];
			const float a = e0 * e1 + e1 * e2 + e2 * e0;
			if (a > best_a) { best_a = a; best = (int)i; }
		}
		if (best < 0) break;
		take_children(node_of(ref[best]), box, ref, (uint32_t)best, n);
		n++;
	}
	return n;
}

// The grid of a Dev8Node and its n children's boxes on it (refs as given; unused slots the sentinel): per axis the origin is the
// smallest child minimum and the step the smallest power of two with extent / step <= 254 (one step of headroom for the outward
// rounding); every coordinate is rounded outwards and checked on the value the walk will decode, fmaf(q, step, origin).  false for a
// box that fits no grid, an extent that is infinite or NaN: the layout is optional, the scene then goes without it, out is not to be
// used.  Origin and extent are taken by comparison, the first child first, as the host always took them: of a +0 and a -0 the earlier
// stays; a NaN coordinate counts only in the first child, in a later one it is passed over and its q is 0 (no builder makes one).
MRT_HD inline bool quantise8(const float (*box)[6], const uint32_t *ref, uint32_t n, Dev8Node &out)
{
	MRT_NO_CONTRACT
	memset(&out, 0, sizeof(out));
	out.n_children = (uint8_t)n;
	float step[3] = { 1.0f, 1.0f, 1.0f };
	bool ok = true;
	for (int a = 0; a < 3; a++) {
		float lo = box[0][a], hi = box[0][3 + a];
		for (uint32_t i = 1; i < n; i++) { lo = box[i][a] < lo ? box[i][a] : lo; hi = hi < box[i][3 + a] ? box[i][3 + a] : hi; }
		out.org[a] = lo;
		const double ext = (double)hi - (double)lo;
		if (!(ext >= 0.0) || !__builtin_isfinite(ext)) { ok = false; continue; } // NaN / infinite box
		int e = 1;
		if (ext > 0.0) { e = (int)ceil(log2(ext / 254.0)) + 127; if (e < 1) e = 1; if (e > 254) e = 254; }
		for (;;) { // guard against log2 rounding: make sure the extent fits
			const float s = __builtin_bit_cast(float, (uint32_t)e << 23);
			if ((double)s * 254.0 >= ext || e >= 254) { step[a] = s; break; }
			e++;
		}
		out.exp[a] = (uint8_t)e;
	}
	for (uint32_t i = 0; i < 8; i++) {
		if (i >= n) { out.ref[i] = kSentinel; continue; }
		out.ref[i] = ref[i];
		for (int a = 0; a < 3 && ok; a++) {
			// (clamped before the conversion: a quotient that is no int, from a box that is none, converts alike on host and device)
			const double tl = floor(((double)box[i][a] - (double)out.org[a]) / (double)step[a]);
			int ql = !(tl > 0.0) ? 0 : (tl > 255.0 ? 255 : (int)tl);
			while (ql > 0 && __builtin_fmaf((float)ql, step[a], out.org[a]) > box[i][a]) ql--;
			const double th = ceil(((double)box[i][3 + a] - (double)out.org[a]) / (double)step[a]);
			int qh = !(th > 0.0) ? 0 : (th > 255.0 ? 255 : (int)th);
			while (qh < 255 && __builtin_fmaf((float)qh, step[a], out.org[a]) < box[i][3 + a]) qh++;
			// cannot happen for finite boxes (one step of headroom); never ship a box that does not contain its child
			if (__builtin_fmaf((float)ql, step[a], out.org[a]) > box[i][a] || __builtin_fmaf((float)qh, step[a], out.org[a]) < box[i][3 + a]) ok = false;
			out.qlo[a][i] = (uint8_t)ql; out.qhi[a][i] = (uint8_t)qh;
		}
	}
	return ok;
}

#ifdef __HIPCC__
// ---- device only ----

// The bounds every thread of a block of WG threads has gathered (mn / mx: its own minimum and maximum, FLT_MAX / -FLT_MAX if it saw
// nothing) into bounds[0..2] = min (ordered uint), bounds[3..5] = max: shuffles within a wave, partials through LDS, then one atomic
// per block and component (one per wave made the bounds pass 1 ms per million triangles).  Every thread of the block calls it.
template <uint32_t WG> __device__ __forceinline__ void block_bounds(const float mn[3], const float mx[3], uint32_t *bounds)
{
	__shared__ float part[WG / 64][6];
	for (int k = 0; k < 3; k++) {
		float lo = mn[k], hi = mx[k];
		for (int off = 32; off > 0; off >>= 1) { lo = fminf(lo, __shfl_xor(lo, off)); hi = fmaxf(hi, __shfl_xor(hi, off)); }
		if ((threadIdx.x & 63u) == 0u) { part[threadIdx.x >> 6][k] = lo; part[threadIdx.x >> 6][3 + k] = hi; }
	}
	__syncthreads();
	if (threadIdx.x < 6u) {
		const bool is_min = threadIdx.x < 3u;
		float v = part[0][threadIdx.x];
		for (uint32_t w = 1; w < WG / 64; w++) v = is_min ? fminf(v, part[w][threadIdx.x]) : fmaxf(v, part[w][threadIdx.x]);
		if (is_min) atomicMin(&bounds[threadIdx.x], f2ord(v)); else atomicMax(&bounds[threadIdx.x], f2ord(v));
	}
}
#endif

} // namespace

} // namespace mrt
