// refit.hip — new triangles for the resident tree of a flat scene (mrt_refit_scene, mrt_refit_instanced_scene) and for the
// BLASes of a two-level scene (mrt_refit_two_level_scene).
//
// A refit keeps the tree's topology -- every node's refs and counts, every leaf's slot range -- and recomputes the boxes
// from the new triangles.  Casts return what they return against a fresh build of the new triangles, because results do
// not depend on which valid BVH is walked; the tree only walks worse as the motion grows.  Both scene kinds
// run one pipeline over a table of BLASes (a flat scene is one BLAS over all its nodes), on the context's stream, in order:
//   1. the box of every slot's new triangle, the scene bounds and a non-finite flag  (refit_boxes_kernel; read back:
//      a refused refit has written nothing of the scene)
//   2. the triangle rows: slot k <- input triangle slot_src[k], leaf-end flags kept    (refit_rows_kernel)
//   3. every node's parent, once per scene                                              (refit_parents_kernel)
//   4. the boxes bottom-up                                                              (refit_climb_kernel)
//   5. a check that every box a node holds is its child's own union                     (refit_verify_kernel)
//   6. the wide layouts and the row arrays, as a build derives them                     (device_build.hip, prep_kernels.hip)
// DESIGN.md 4.8 has the pipeline and the measurements.  A two-level scene adds kernels of its own where a pass needs
// the mesh array (refit2_tris_kernel, refit2_slots_kernel, refit2_roots_kernel), then rebuilds its TLAS.
#include <cfloat>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>
#include "mrt_context.h"
#include "build_rules.h"

namespace mrt {

namespace {

#define REFIT_WG 256
#define REFIT_BOXES_BLOCKS 1024u

// the union of the slots [first, first + count) (a host SAH leaf holds several; the root leaf of a tiny scene is wrapped
// as two children over the halves of one range)
__device__ __forceinline__ Box leaf_union(const Box *boxes, uint32_t first, uint32_t count)
{
	Box u = boxes[first];
	for (uint32_t j = 1; j < count; j++) u = unite(u, boxes[first + j]);
	return u;
}

__device__ __forceinline__ void put_side(DevNode *row, int side, const Box &b)
{
	float *mn = side ? row->rmin : row->lmin, *mx = side ? row->rmax : row->lmax;
	for (int k = 0; k < 3; k++) { mn[k] = b.mn[k]; mx[k] = b.mx[k]; }
}
// the same, write-through (sc1: agent-scope relaxed atomic stores, 8 + 4 bytes per corner), for a box another thread reads in the launch
typedef __attribute__((address_space(1))) unsigned long long refit_gu64;
typedef __attribute__((address_space(1))) unsigned int refit_gu32;
#define REFIT_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
__device__ __forceinline__ void put_side_sc1(DevNode *row, int side, const Box &b)
{
	float *mn = side ? row->rmin : row->lmin, *mx = side ? row->rmax : row->lmax;
	__hip_atomic_store((refit_gu64 *)mn, (unsigned long long)__float_as_uint(b.mn[0]) | ((unsigned long long)__float_as_uint(b.mn[1]) << 32), REFIT_RLX);
	__hip_atomic_store((refit_gu32 *)(mn + 2), __float_as_uint(b.mn[2]), REFIT_RLX);
	__hip_atomic_store((refit_gu64 *)mx, (unsigned long long)__float_as_uint(b.mx[0]) | ((unsigned long long)__float_as_uint(b.mx[1]) << 32), REFIT_RLX);
	__hip_atomic_store((refit_gu32 *)(mx + 2), __float_as_uint(b.mx[2]), REFIT_RLX);
}

// One row per BLAS, in blas[] order: its node rows [root, root + n_nodes), its slots [slot_base, slot_base + n_tris), its triangles
// [first_tri, first_tri + n_tris) of the mesh array.  Roots and slot bases grow with the index.  A flat scene is the one row
// {0, n_nodes, 0, n_tris, 0}.
struct RefitBlas { uint32_t root, n_nodes, slot_base, n_tris, first_tri; };

// the last BLAS whose first node (by_node) or first slot starts at or before key
__device__ __forceinline__ RefitBlas blas_of(const RefitBlas *blas, uint32_t n_blas, uint32_t key, bool by_node)
{
	uint32_t lo = 0u, hi = n_blas;
	while (hi - lo > 1u) {
		const uint32_t mid = (lo + hi) >> 1;
		if ((by_node ? blas[mid].root : blas[mid].slot_base) <= key) lo = mid; else hi = mid;
	}
	return blas[lo];
}

// 1. boxes[k] = box of input triangle slot_src[k] (slot order: a leaf's boxes are contiguous); scal[0..5] = the bounds
//    (ordered uint: min, max), scal[6] != 0 if any coordinate is not finite.  Grid-stride, one atomic per block and component.
__global__ __launch_bounds__(REFIT_WG) void refit_boxes_kernel(const mrt_tri64 *tris, const uint32_t *slot_src, uint32_t n, Box *boxes, uint32_t *scal)
{
	float mn[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, mx[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
	bool finite = true;
	for (uint32_t k = blockIdx.x * REFIT_WG + threadIdx.x; k < n; k += gridDim.x * REFIT_WG) {
		const float4 *t = reinterpret_cast<const float4 *>(tris + slot_src[k]);
		const float4 a = t[0], b = t[1], c = t[2];
		const float v0[3] = { a.x, a.y, a.z }, e1[3] = { b.x, b.y, b.z }, e2[3] = { c.x, c.y, c.z };
		const Box bx = tri_box(v0, e1, e2);
		for (int i = 0; i < 3; i++) {
			finite = finite && __builtin_isfinite(v0[i]) && __builtin_isfinite(e1[i]) && __builtin_isfinite(e2[i]) &&
					__builtin_isfinite(v0[i] + e1[i]) && __builtin_isfinite(v0[i] + e2[i]);
			mn[i] = fminf(mn[i], bx.mn[i]); mx[i] = fmaxf(mx[i], bx.mx[i]);
		}
		boxes[k] = bx;
	}
	if (!finite) atomicOr(&scal[6], 1u);
	block_bounds<REFIT_WG>(mn, mx, scal);
}

// 2. slot k <- input triangle slot_src[k]: the whole row (v0, edges, id, layers, normal) but the leaf-end flag, which is the tree's
__global__ __launch_bounds__(REFIT_WG) void refit_rows_kernel(const mrt_tri64 *tris, const uint32_t *slot_src, uint32_t n, TriHot *hot, TriCold *cold)
{
	const uint32_t k = blockIdx.x * REFIT_WG + threadIdx.x;
	if (k >= n) return;
	const float4 *t = reinterpret_cast<const float4 *>(tris + slot_src[k]);
	const float4 a = t[0], b = t[1], d = t[3];
	float4 c = t[2];
	c.w = __uint_as_float(hot[k].flags & kLastInLeaf);
	float4 *h = reinterpret_cast<float4 *>(hot + k);
	h[0] = a; h[1] = b; h[2] = c;
	float4 nn = d; nn.w = 0.0f;
	reinterpret_cast<float4 *>(cold)[k] = nn;
}

// 3. Parents, once per scene, of the node rows [lo, hi), numbered from lo as refit_climb_kernel sees them (it runs on nodes + lo):
//    parent[c - lo] = b - lo for the left child c of node b, | 1 << 31 for the right one.  Every BLAS root keeps the 0xFFFFFFFF of
//    the memset before, so each climb ends at its BLAS's root.  The rows a BLAS leaves unused (a device SAH tree fills fewer than
//    n_tris - 1) are zeroed: without leaf refs, the climb starts nothing there.
__global__ __launch_bounds__(REFIT_WG) void refit_parents_kernel(DevNode *nodes, uint32_t lo, uint32_t hi, const RefitBlas *blas, uint32_t n_blas,
		uint32_t *parent)
{
	const uint32_t b = lo + blockIdx.x * REFIT_WG + threadIdx.x;
	if (b >= hi) return;
	const RefitBlas bl = blas_of(blas, n_blas, b, true);
	const uint32_t end = bl.root + bl.n_nodes;
	if (b >= end) { DevNode z; memset(&z, 0, sizeof(z)); nodes[b] = z; return; }
	const uint32_t l = nodes[b].left_ref, r = nodes[b].right_ref;
	if (l > bl.root && l < end) parent[l - lo] = b - lo;
	if (r > bl.root && r < end) parent[r - lo] = (b - lo) | 0x80000000u;
}

// 4. The climb.  A node whose children are both leaves boxes them and owns itself; a node with one leaf child boxes it and
//    arrives at itself with it, as a finished child would.  A thread that finishes a node writes the node's box into its
//    parent's row (its own side only: refs and counts stay) and adds one to the parent's arrival counter; the second to
//    arrive owns the parent, reads the other side and climbs on.  The hand-off crosses CUs and XCDs (per-XCD L2s are not
//    coherent with each other, a CU's L1 is never refreshed by another CU's stores), so it is the write-through form with
//    an acquire (MI355X guide, inter-workgroup visibility; the R1 recipe): the box is stored sc1, the storing thread drains
//    its stores (s_waitcnt vmcnt(0)) before its agent-scope add to the counter, and the owner takes an agent acquire
//    (buffer_inv sc1: its CU's L1) before its plain loads of the other side.  No release fence: an agent release writes back
//    the XCD's whole L2, and one per wave and level made this pass 4x slower.
__global__ __launch_bounds__(REFIT_WG) void refit_climb_kernel(DevNode *nodes, uint32_t n_nodes, const Box *boxes, uint32_t n_tris,
		const uint32_t *parent, uint32_t *arrivals)
{
	const uint32_t b = blockIdx.x * REFIT_WG + threadIdx.x;
	if (b >= n_nodes) return;
	const DevNode g = nodes[b];
	const bool ll = (g.left_ref & kLeafBit) != 0u, rl = (g.right_ref & kLeafBit) != 0u;
	if (!ll && !rl) return;
	// (a leaf range outside the triangle arrays cannot come from a builder of this library; the check pass reports it)
	auto leaf = [&](uint32_t ref, uint32_t count) {
		const uint32_t first = (ref & 0x7FFFFFFFu) < n_tris ? (ref & 0x7FFFFFFFu) : n_tris - 1u;
		return leaf_union(boxes, first, count == 0u ? 1u : (count <= n_tris - first ? count : n_tris - first));
	};
	Box have;
	uint32_t node = b;
	int side = ll ? 0 : 1;
	bool owned = ll && rl;
	if (owned) {
		const Box lb = leaf(g.left_ref, g.left_count), rb = leaf(g.right_ref, g.right_count);
		put_side(nodes + b, 0, lb); put_side(nodes + b, 1, rb);
		have = unite(lb, rb);
	} else have = ll ? leaf(g.left_ref, g.left_count) : leaf(g.right_ref, g.right_count);
	for (;;) {
		if (!owned) {
			put_side_sc1(nodes + node, side, have);
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the box is out before the counter moves
			const uint32_t before = __hip_atomic_fetch_add(&arrivals[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (before == 0u) return; // the other side is not finished: its thread climbs on
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
			const Box other = get_side(nodes + node, side ^ 1);
			have = side ? unite(other, have) : unite(have, other);
		}
		owned = false;
		const uint32_t p = parent[node];
		if (p == 0xFFFFFFFFu) return;
		node = p & 0x7FFFFFFFu; side = (int)(p >> 31);
		if (node >= n_nodes) return;
	}
}

// 5. After the kernel boundary: every box a node of [lo, hi) holds must be what its child says -- the union of a leaf's slot boxes,
//    the union of an inner child's two boxes; inner refs must lie in [lo, hi).  A row past its BLAS's n_nodes is unused (the parents
//    pass zeroed it) and has nothing to check.  A stale hand-off (or a broken tree) shows as a count in *bad.
__global__ __launch_bounds__(REFIT_WG) void refit_verify_kernel(const DevNode *nodes, uint32_t lo, uint32_t hi, const RefitBlas *blas, uint32_t n_blas,
		const Box *boxes, uint32_t n_tris, uint32_t *bad)
{
	const uint32_t b = lo + blockIdx.x * REFIT_WG + threadIdx.x;
	if (b >= hi) return;
	const RefitBlas bl = blas_of(blas, n_blas, b, true);
	if (b >= bl.root + bl.n_nodes) return;
	const DevNode g = nodes[b];
	bool ok = true;
	for (int side = 0; side < 2; side++) {
		const uint32_t ref = side ? g.right_ref : g.left_ref;
		Box want;
		if (ref & kLeafBit) {
			const uint32_t first = ref & 0x7FFFFFFFu, cnt = side ? g.right_count : g.left_count;
			if (cnt == 0u || first >= n_tris || cnt > n_tris - first) { ok = false; continue; }
			want = leaf_union(boxes, first, cnt);
		} else {
			if (ref < lo || ref >= hi) { ok = false; continue; }
			want = unite(get_side(nodes + ref, 0), get_side(nodes + ref, 1));
		}
		const Box have = get_side(&g, side);
		for (int k = 0; k < 3; k++)
			ok = ok && __float_as_uint(have.mn[k]) == __float_as_uint(want.mn[k]) && __float_as_uint(have.mx[k]) == __float_as_uint(want.mx[k]);
	}
	if (!ok) atomicAdd(bad, 1u);
}

// ---- two-level scenes (mrt_refit_two_level_scene).  The node array holds the TLAS in [0, tlas_cap) and every BLAS behind it,
// with global refs: inner refs are node indices, leaf refs slots of d_hot / d_cold, whose ids are mesh-local.  The passes above run
// over the BLAS rows [lo, hi) = [tlas_cap, n_nodes) only (TLAS leaves hold instance slots, not triangles); the TLAS is rebuilt on
// the host from the new mesh boxes, as mrt_update_instances rebuilds it.

// 0. the triangles of every BLAS by make_tri64 (build_rules.h), as an upload makes them: mesh-local id, all layers -- BLAS after
//    BLAS: row slot_base + j is triangle first_tri + j of the mesh array.
__global__ __launch_bounds__(REFIT_WG) void refit2_tris_kernel(const float *verts9, const RefitBlas *blas, uint32_t n_blas, uint32_t n, mrt_tri64 *out)
{
	const uint32_t s = blockIdx.x * REFIT_WG + threadIdx.x;
	if (s >= n) return;
	const RefitBlas bl = blas_of(blas, n_blas, s, false);
	const uint32_t j = s - bl.slot_base;
	const float *a = verts9 + 9u * (size_t)(bl.first_tri + j);
	out[s] = make_tri64(a, a + 3, a + 6, j, 0xFFFFFFFFu);
}

// the slot map, once per scene: slot k holds triangle hot[k].id of its BLAS, staged at slot_base + id.  (An id beyond its mesh
// cannot come from a builder of this library; it is held inside the BLAS's rows.)
__global__ __launch_bounds__(REFIT_WG) void refit2_slots_kernel(const TriHot *hot, const RefitBlas *blas, uint32_t n_blas, uint32_t n, uint32_t *slot_src)
{
	const uint32_t k = blockIdx.x * REFIT_WG + threadIdx.x;
	if (k >= n) return;
	const RefitBlas bl = blas_of(blas, n_blas, k, false);
	const uint32_t id = hot[k].id;
	slot_src[k] = bl.slot_base + (id < bl.n_tris ? id : 0u);
}

// 6. every mesh's new box: the union of its root's two sides (what the TLAS rebuild and later mrt_update_instances calls box)
__global__ __launch_bounds__(REFIT_WG) void refit2_roots_kernel(const DevNode *nodes, const RefitBlas *blas, uint32_t n_blas, Box *out)
{
	const uint32_t k = blockIdx.x * REFIT_WG + threadIdx.x;
	if (k >= n_blas) return;
	const DevNode *g = nodes + blas[k].root;
	out[k] = unite(get_side(g, 0), get_side(g, 1));
}

// One refit, flat or two-level: the node rows [lo, hi) of the n_blas BLASes of a table, over n slots, on the context's stream.
// What a scene's first refit allocates -- the slot map (two-level scenes), the parents, and a host-uploaded scene's wide layouts at
// binary-node indices (its compact host collapse has no map from binary nodes to wide nodes) -- starts as the scene's own array;
// one that differs is new, and is dropped on a failure before the scene adopts it.
struct Refit {
	mrt_ctx *ctx;
	uint32_t n, lo, hi, n_blas;
	// in the build arena: the slot boxes, the arrival counters, 256 bytes of scalars (bounds[6], non-finite, verification failures,
	// collapse8 "bad"), the table, then the caller's extra bytes
	Box *boxes = nullptr; uint32_t *arrivals = nullptr, *scal = nullptr; RefitBlas *table = nullptr; char *extra = nullptr;
	uint32_t *slot_src, *parent; Dev4Node *nodes4; Dev8Node *nodes8;
	uint32_t h[10]; // the scalars as last read back
	std::vector<uint32_t> head; // the scalars' start values and the table, as start uploads them (read until box_pass syncs)

	Refit(mrt_ctx *c, uint32_t n_slots, uint32_t first, uint32_t end, uint32_t blases) : ctx(c), n(n_slots), lo(first), hi(end), n_blas(blases),
			slot_src(c->d_slot_src), parent(c->d_parent), nodes4(c->d_nodes4), nodes8(c->d_nodes8) {}

	int arena(size_t extra_bytes)
	{
		const size_t box_bytes = align256((size_t)n * sizeof(Box)), arr_bytes = align256((size_t)(hi - lo) * 4u),
				tab_bytes = align256((size_t)n_blas * sizeof(RefitBlas)), need = box_bytes + arr_bytes + 256u + tab_bytes + extra_bytes;
		const hipError_t arena_sync = grow_arena(&ctx->build_arena, need, ctx->stream);
		if (arena_sync == hipErrorOutOfMemory) return fail(ctx, MRT_ERR_OOM, "refit: out of device memory");
		HIP_TRY(ctx, arena_sync);
		boxes = (Box *)ctx->build_arena.ptr;
		arrivals = (uint32_t *)((char *)boxes + box_bytes);
		scal = (uint32_t *)((char *)arrivals + arr_bytes);
		table = (RefitBlas *)((char *)scal + 256u);
		extra = (char *)table + tab_bytes;
		return MRT_OK;
	}
	// (a failed allocation leaves the pointer null: drop frees nothing that is the scene's)
	template <class T> static bool alloc(T *&p, uint32_t count) { if (hipMalloc((void **)&p, (size_t)count * sizeof(T)) == hipSuccess) return true; p = nullptr; return false; }
	int out_of_memory() { drop(); return fail(ctx, MRT_ERR_OOM, "refit: out of device memory"); }
	void drop() const
	{
		if (slot_src != ctx->d_slot_src) (void)hipFree(slot_src);
		if (parent != ctx->d_parent) (void)hipFree(parent);
		if (nodes4 != ctx->d_nodes4) (void)hipFree(nodes4);
		if (nodes8 != ctx->d_nodes8) (void)hipFree(nodes8);
	}
	// (after finish has adopted the new arrays they are the scene's, and free_scene's to release)
	int bail(hipError_t e, const char *what, bool written)
	{
		if (written) free_scene(ctx); // part of the scene may be new, part old: released rather than kept wrong
		std::snprintf(ctx->err, sizeof(ctx->err), "refit: %s failed: %s%s", what, hipGetErrorString(e), written ? "; the scene was released" : "");
		return MRT_ERR_HIP;
	}

	// event 0, then the scalars' start values (the bounds' min at the top of the ordered range, zeros) and the table behind them, in
	// one copy; a front-end may enqueue passes of its own behind it
	hipError_t start(const RefitBlas *host_table)
	{
		head.assign(64u + n_blas * sizeof(RefitBlas) / 4u, 0u);
		head[0] = head[1] = head[2] = 0xFFFFFFFFu;
		std::memcpy(head.data() + 64, host_table, (size_t)n_blas * sizeof(RefitBlas));
		hipError_t e = hipEventRecord(ctx->ev[0], ctx->stream);
		if (e == hipSuccess) e = hipMemcpyAsync(scal, head.data(), head.size() * 4u, hipMemcpyHostToDevice, ctx->stream);
		return e;
	}
	// 1. after what was enqueued since start (e its status): the boxes of the slots' new triangles tris[slot_src[k]], the bounds and the
	//    non-finite flag, read back (event 1, a sync) before anything of the scene is written.  A failure, or a non-finite coordinate
	//    (refused with the message non_finite), leaves the scene as it was.
	int box_pass(hipError_t e, const mrt_tri64 *tris, const char *non_finite)
	{
		const uint32_t blocks = (n + REFIT_WG - 1u) / REFIT_WG;
		if (e == hipSuccess) {
			hipLaunchKernelGGL(refit_boxes_kernel, dim3(blocks < REFIT_BOXES_BLOCKS ? blocks : REFIT_BOXES_BLOCKS), dim3(REFIT_WG), 0, ctx->stream, tris, slot_src, n, boxes, scal);
			e = hipGetLastError();
		}
		if (e == hipSuccess) e = hipMemcpyAsync(h, scal, sizeof(h), hipMemcpyDeviceToHost, ctx->stream);
		if (e == hipSuccess) e = hipEventRecord(ctx->ev[1], ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
		if (e != hipSuccess) { drop(); return bail(e, "the box pass", false); }
		if (h[6] != 0u) { drop(); return fail(ctx, MRT_ERR_INVALID, non_finite); }
		return MRT_OK;
	}
	// 2-5. from event 2: the triangle rows, the parents (first refit), the climb and the check.  Only enqueues.
	hipError_t tree_pass(const mrt_tri64 *tris)
	{
		const uint32_t nb = hi - lo, blocks = (n + REFIT_WG - 1u) / REFIT_WG, node_blocks = (nb + REFIT_WG - 1u) / REFIT_WG;
		hipError_t e = hipEventRecord(ctx->ev[2], ctx->stream);
		if (e == hipSuccess) { hipLaunchKernelGGL(refit_rows_kernel, dim3(blocks), dim3(REFIT_WG), 0, ctx->stream, tris, slot_src, n, ctx->d_hot, ctx->d_cold); e = hipGetLastError(); }
		if (e == hipSuccess && parent != ctx->d_parent) {
			e = hipMemsetAsync(parent, 0xFF, (size_t)nb * 4u, ctx->stream);
			if (e == hipSuccess) { hipLaunchKernelGGL(refit_parents_kernel, dim3(node_blocks), dim3(REFIT_WG), 0, ctx->stream, ctx->d_nodes, lo, hi, table, n_blas, parent); e = hipGetLastError(); }
		}
		if (e == hipSuccess) e = hipMemsetAsync(arrivals, 0, (size_t)nb * 4u, ctx->stream);
		if (e == hipSuccess) { hipLaunchKernelGGL(refit_climb_kernel, dim3(node_blocks), dim3(REFIT_WG), 0, ctx->stream, ctx->d_nodes + lo, nb, boxes, n, parent, arrivals); e = hipGetLastError(); }
		if (e == hipSuccess) { hipLaunchKernelGGL(refit_verify_kernel, dim3(node_blocks), dim3(REFIT_WG), 0, ctx->stream, ctx->d_nodes, lo, hi, table, n_blas, boxes, n, scal + 7); e = hipGetLastError(); }
		return e;
	}
	// after what was enqueued behind the tree pass (e its status): the scalars read back (event 3, a sync), the new arrays adopted (a
	// new wide layout covers the hi - lo binary nodes).  From here on a failure releases the scene.
	int finish(hipError_t e)
	{
		if (e == hipSuccess) e = hipMemcpyAsync(h, scal, sizeof(h), hipMemcpyDeviceToHost, ctx->stream);
		if (e == hipSuccess) e = hipEventRecord(ctx->ev[3], ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
		if (e != hipSuccess) { drop(); return bail(e, "the refit", true); }
		ctx->d_slot_src = slot_src; ctx->d_parent = parent;
		if (nodes4 != ctx->d_nodes4) { (void)hipFree(ctx->d_nodes4); ctx->d_nodes4 = nodes4; ctx->n_nodes4 = hi - lo; }
		if (nodes8 != ctx->d_nodes8) { (void)hipFree(ctx->d_nodes8); ctx->d_nodes8 = nodes8; ctx->n_nodes8 = hi - lo; }
		if (h[7] != 0u) {
			// boxes that are not what the tree needs could make casts miss: the scene is released rather than kept wrong
			free_scene(ctx);
			std::snprintf(ctx->err, sizeof(ctx->err), "refit: the tree failed its verification pass (%u nodes); the scene was released", h[7]);
			return MRT_ERR_HIP;
		}
		return MRT_OK;
	}
	// the end of a refit that succeeded: last_build_ms is the device time from event 0 to 1 and from 2 to 3
	int done()
	{
		float ms0 = 0.0f, ms1 = 0.0f;
		if (hipEventElapsedTime(&ms0, ctx->ev[0], ctx->ev[1]) == hipSuccess && hipEventElapsedTime(&ms1, ctx->ev[2], ctx->ev[3]) == hipSuccess) ctx->stats.last_build_ms = ms0 + ms1;
		return MRT_OK;
	}
};

// The refit of the resident flat scene, one BLAS over all its nodes, from n_tris = ctx->n_tris device triangles (checked by the
// callers); then the wide layouts and the row arrays, as a build derives them.  Blocks until it is done.
int refit_flat_scene(mrt_ctx *ctx, const mrt_tri64 *d_tris)
{
	const uint32_t n = ctx->n_tris, nn = ctx->n_nodes;
	const RefitBlas table{ 0u, nn, 0u, n, 0u };
	Refit r(ctx, n, 0u, nn, 1u);
	int rc = r.arena(0u);
	if (rc) return rc;
	bool ok = r.parent || Refit::alloc(r.parent, nn);
	if (ok && r.nodes4 && ctx->n_nodes4 != nn) ok = Refit::alloc(r.nodes4, nn);
	if (ok && r.nodes8 && ctx->n_nodes8 != nn) ok = Refit::alloc(r.nodes8, nn);
	if (!ok) return r.out_of_memory();
	if ((rc = r.box_pass(r.start(&table), d_tris, "refit: a triangle has a non-finite coordinate (the scene is unchanged)"))) return rc;
	hipError_t e = r.tree_pass(d_tris);
	const bool new4 = r.nodes4 != ctx->d_nodes4;
	if (e == hipSuccess && r.nodes4) e = launch_collapse4(ctx->d_nodes, nn, r.nodes4, ctx->stream);
	if (e == hipSuccess && r.nodes8) e = launch_collapse8(ctx->d_nodes, nn, r.nodes8, ctx->d_leaf_box, r.scal + 8, ctx->stream);
	if (e == hipSuccess && ctx->d_rows) e = launch_build_rows(ctx->d_nodes, ctx->d_hot, ctx->d_cold, nn, n, ctx->d_rows, ctx->stream);
	if (e == hipSuccess && ctx->d_rows4 && !new4) e = launch_build_rows4(r.nodes4, ctx->d_hot, ctx->d_cold, ctx->n_nodes4, n, ctx->d_rows4, ctx->stream);
	if ((rc = r.finish(e))) return rc;
	// the walks' stack bounds by the builder's rule (device_build.hip): every 4-wide node on a path leaves at most 3 entries pending
	// and descends at least one binary level, every 8-wide node at most 7
	const uint32_t levels = ctx->depth - 1u;
	if (ctx->d_nodes4) ctx->stack4 = 3u * levels + 1u;
	if (ctx->d_nodes8) ctx->stack8 = 7u * levels + 1u;
	if (ctx->d_nodes8 && r.h[8] != 0u) { // a box that fits no grid: the scene goes without the 8-wide layout, as a build does
		(void)hipFree(ctx->d_nodes8); (void)hipFree(ctx->d_leaf_box);
		ctx->d_nodes8 = nullptr; ctx->d_leaf_box = nullptr; ctx->n_nodes8 = ctx->stack8 = 0;
	}
	if (new4 && ctx->d_rows4) {
		// the 4-wide rows (builds with the four-wide packet walk) of a host-uploaded scene's first refit: sized by the new layout,
		// under build_rows' conditions (api.hip), else the scene goes without them as an upload would
		(void)hipFree(ctx->d_rows4); ctx->d_rows4 = nullptr;
		const uint64_t n_units4 = (uint64_t)2u * nn + n;
		if (ctx->stack4 <= 64u && n_units4 < kAsmNodeLimit) {
			if (hipMalloc(&ctx->d_rows4, (size_t)n_units4 * 64u) != hipSuccess) { ctx->d_rows4 = nullptr; (void)hipGetLastError(); }
			else {
				e = launch_build_rows4(ctx->d_nodes4, ctx->d_hot, ctx->d_cold, nn, n, ctx->d_rows4, ctx->stream);
				if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
				if (e != hipSuccess) return r.bail(e, "the 4-wide rows", true);
			}
		}
	}
	for (int c = 0; c < 3; c++) { ctx->bounds_lo[c] = ord2f(r.h[c]); ctx->bounds_hi[c] = ord2f(r.h[3 + c]); }
	return r.done();
}

// The refit of the resident two-level scene from the mesh array d_verts9 (on the device), for instances checked by
// check_two_level_refit: every BLAS in the node rows [tlas_cap, n_nodes), then the mesh boxes, the 8-wide layout per BLAS and the
// TLAS.  Blocks until it is done.
int refit_two_level_scene(mrt_ctx *ctx, const float *d_verts9, const mrt_instance *instances, uint32_t n_instances, bool inst_on_device)
{
	TwoLevelHost *tl = ctx->two_level;
	const uint32_t n = ctx->n_tris, lo = tl->tlas_cap, nb = ctx->n_nodes - lo, n_blas = tl->n_blas;
	std::vector<RefitBlas> table(n_blas);
	uint32_t slot_base = 0, max_nodes = 0;
	bool binary8 = ctx->n_nodes8 == nb; // the 8-wide layout sits at binary-node indices (device-built BLASes, or refit before)
	for (uint32_t k = 0; k < n_blas; k++) {
		const TwoLevelBlas &b = tl->blas[k];
		table[k] = RefitBlas{ b.root, b.n_nodes, slot_base, b.n_tris, b.first_tri };
		slot_base += b.n_tris;
		if (b.n_nodes > max_nodes) max_nodes = b.n_nodes;
		binary8 = binary8 && b.root8 == b.root - lo;
	}
	const bool wide8 = tl->wide8 && ctx->d_nodes8 && ctx->d_leaf_box;
	// behind the table in the arena: the mesh boxes, and scratch for the largest BLAS's collapse
	const size_t root_bytes = align256((size_t)n_blas * sizeof(Box)), scr_bytes = wide8 ? align256((size_t)max_nodes * sizeof(DevNode)) : 0u,
			scr8_bytes = wide8 ? align256((size_t)max_nodes * sizeof(Dev8Node)) : 0u;
	Refit r(ctx, n, lo, ctx->n_nodes, n_blas);
	int rc = r.arena(root_bytes + scr_bytes + scr8_bytes);
	if (rc) return rc;
	Box *d_roots = (Box *)r.extra;
	DevNode *scr = (DevNode *)(r.extra + root_bytes);
	Dev8Node *scr8 = (Dev8Node *)(r.extra + root_bytes + scr_bytes);
	mrt_tri64 *staged = (mrt_tri64 *)ctx->refit_in.ptr; // (sized by the caller)
	bool ok = r.slot_src || Refit::alloc(r.slot_src, n);
	if (ok && !r.parent) ok = Refit::alloc(r.parent, nb);
	if (ok && wide8 && !binary8) ok = Refit::alloc(r.nodes8, nb);
	if (!ok) return r.out_of_memory();

	// 0. the new triangle rows staged and the slot map (first refit), ahead of the box pass
	const uint32_t blocks = (n + REFIT_WG - 1u) / REFIT_WG, blas_blocks = (n_blas + REFIT_WG - 1u) / REFIT_WG;
	hipError_t e = r.start(table.data());
	if (e == hipSuccess) { hipLaunchKernelGGL(refit2_tris_kernel, dim3(blocks), dim3(REFIT_WG), 0, ctx->stream, d_verts9, r.table, n_blas, n, staged); e = hipGetLastError(); }
	if (e == hipSuccess && r.slot_src != ctx->d_slot_src) { hipLaunchKernelGGL(refit2_slots_kernel, dim3(blocks), dim3(REFIT_WG), 0, ctx->stream, ctx->d_hot, r.table, n_blas, n, r.slot_src); e = hipGetLastError(); }
	if ((rc = r.box_pass(e, staged, "refit: a mesh triangle has a non-finite coordinate (the scene is unchanged)"))) return rc;

	// 6. after the tree pass: the mesh boxes, the 8-wide layout per BLAS
	std::vector<Box> roots(n_blas);
	e = r.tree_pass(staged);
	if (e == hipSuccess) { hipLaunchKernelGGL(refit2_roots_kernel, dim3(blas_blocks), dim3(REFIT_WG), 0, ctx->stream, ctx->d_nodes, r.table, n_blas, d_roots); e = hipGetLastError(); }
	// the builder's collapse wants a tree from node 0 with local refs: each BLAS is localised into scratch (offset_refs adds modulo
	// 2^32), collapsed with its exact leaf boxes, and put back at root - tlas_cap with global refs, as build_blases_on_device places it
	for (uint32_t k = 0; wide8 && k < n_blas && e == hipSuccess; k++) {
		const RefitBlas &b = table[k];
		const uint32_t root8 = b.root - lo;
		e = launch_offset_refs(scr, ctx->d_nodes + b.root, b.n_nodes, 0u - b.root, 0u - b.slot_base, (void *)ctx->stream);
		if (e == hipSuccess) e = launch_collapse8(scr, b.n_nodes, scr8, ctx->d_leaf_box + (size_t)b.slot_base * 8u, r.scal + 8, ctx->stream);
		if (e == hipSuccess) e = launch_offset_refs8(r.nodes8 + root8, scr8, b.n_nodes, root8, b.slot_base, (void *)ctx->stream);
	}
	if (e == hipSuccess) e = hipMemcpyAsync(roots.data(), d_roots, (size_t)n_blas * sizeof(Box), hipMemcpyDeviceToHost, ctx->stream);
	if ((rc = r.finish(e))) return rc;
	// the mesh boxes every TLAS build (here and in later mrt_update_instances calls) boxes the instances by; where the 8-wide layout
	// moved to binary indices, its size, roots and stack bounds by the builder's rule (device_build.hip: 7 entries per binary level)
	if (wide8 && !binary8) tl->n_nodes8 = nb;
	for (uint32_t k = 0; k < n_blas; k++) {
		TwoLevelBlas &b = tl->blas[k];
		for (int c = 0; c < 3; c++) { b.lo[c] = roots[k].mn[c]; b.hi[c] = roots[k].mx[c]; }
		if (wide8 && !binary8) { b.root8 = b.root - lo; b.stack8 = 7u * (b.depth - 1u) + 1u; }
	}
	if (wide8 && r.h[8] != 0u) { // a box that fits no grid: the scene goes without the 8-wide layout, as upload and build do
		(void)hipFree(ctx->d_nodes8); (void)hipFree(ctx->d_leaf_box);
		ctx->d_nodes8 = nullptr; ctx->d_leaf_box = nullptr; ctx->n_nodes8 = ctx->stack8 = 0;
		tl->wide8 = false; tl->n_nodes8 = 0;
	}
	ctx->tlas_blas_ok = false; // the mesh table of device top-level builds (tlas_device.hip) holds the old boxes and roots
	if (inst_on_device) {
		// the TLAS built on the device from the device instances (checked on the device before the refit) and the new mesh boxes,
		// in the radix form; a refusal here leaves new meshes behind an old top level, so the scene is released as below
		r.done();
		const float refit_ms = ctx->stats.last_build_ms;
		float tlas_ms = 0.0f;
		rc = device_update_tlas(ctx, instances, n_instances, true, 0, false, &tlas_ms);
		if (rc) { if (ctx->scene) free_scene(ctx); return rc; }
		ctx->stats.last_build_ms = refit_ms + tlas_ms;
		return MRT_OK;
	}
	// the TLAS over the new world boxes, uploaded as mrt_update_instances does.  (The host's copy of the BLAS rows, tl->nodes beyond
	// the TLAS range of a host-built scene, is stale from here on: nothing reads it after the upload.)
	rc = refit_two_level(tl, instances, n_instances, ctx->err, sizeof(ctx->err));
	if (!rc && tl->depth > 64u) rc = fail(ctx, MRT_ERR_UNSUPPORTED, "refit: the new top level is too deep for the per-lane stack");
	if (rc) { free_scene(ctx); return rc; } // (checked before; a new TLAS that cannot be used leaves new meshes behind an old one)
	e = hipMemcpy(ctx->d_nodes, tl->nodes, (size_t)tl->n_tlas_nodes * sizeof(DevNode), hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMemcpy(ctx->d_instances, tl->inst, (size_t)tl->n_inst * sizeof(DevInstance), hipMemcpyHostToDevice);
	if (e != hipSuccess) return r.bail(e, "the top-level upload", true);
	ctx->depth = tl->depth; ctx->stack8 = tl->wide8 ? tl->depth8 : 0;
	ctx->stack_depth = ((tl->depth + 7u) / 8u) * 8u;
	if (ctx->stack_depth < 8) ctx->stack_depth = 8;
	for (int c = 0; c < 3; c++) {
		ctx->bounds_lo[c] = std::fmin(tl->nodes[0].lmin[c], tl->nodes[0].rmin[c]);
		ctx->bounds_hi[c] = std::fmax(tl->nodes[0].lmax[c], tl->nodes[0].rmax[c]);
	}
	return r.done();
}

} // namespace

} // namespace mrt

extern "C" {

// refusals that leave the scene as it is, in the order the header lists them, for a refit of a two-level scene or of a flat one
static int refit_precheck(mrt_ctx *ctx, uint32_t flags, bool two_level)
{
	const uint32_t known = MRT_BUILD_TRIS_ON_DEVICE | (two_level ? (uint32_t)MRT_BUILD_INSTANCES_ON_DEVICE : 0u);
	if (flags & ~known) return fail(ctx, MRT_ERR_INVALID, "refit: unknown flag");
	if (ctx->pending) return fail(ctx, MRT_ERR_PENDING, "refit: collect the pending dispatch first");
	if (!ctx->scene) return fail(ctx, MRT_ERR_NO_SCENE, "refit: no scene uploaded");
	if (two_level && !ctx->two_level) return fail(ctx, MRT_ERR_UNSUPPORTED, "refit: a flat scene (mrt_refit_scene / mrt_refit_instanced_scene refit it)");
	if (!two_level && ctx->two_level) return fail(ctx, MRT_ERR_UNSUPPORTED, "refit: a two-level scene (mrt_update_instances moves its instances)");
	if (!ctx->d_slot_src && !two_level) return fail(ctx, MRT_ERR_UNSUPPORTED, "refit: the scene has no slot map");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	return MRT_OK;
}

int mrt_refit_scene(mrt_ctx *ctx, const mrt_tri64 *tris, uint32_t n_tris, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!tris) return fail(ctx, MRT_ERR_INVALID, "refit: null triangles");
	int rc = refit_precheck(ctx, flags, false);
	if (rc) return rc;
	if (n_tris != ctx->n_tris) return fail(ctx, MRT_ERR_INVALID, "refit: the triangle count differs from the scene's");
	const mrt_tri64 *d_tris = tris;
	if (!(flags & MRT_BUILD_TRIS_ON_DEVICE)) {
		if ((rc = ensure(ctx, ctx->refit_in, (size_t)n_tris * sizeof(mrt_tri64)))) return rc;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->refit_in.ptr, tris, (size_t)n_tris * sizeof(mrt_tri64), hipMemcpyHostToDevice, ctx->stream));
		d_tris = (const mrt_tri64 *)ctx->refit_in.ptr;
	}
	return mrt::refit_flat_scene(ctx, d_tris);
}

int mrt_refit_instanced_scene(mrt_ctx *ctx, const float *verts9, uint32_t n_mesh_tris, const mrt_instance *instances,
		uint32_t n_instances, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!verts9 || !instances || n_instances == 0) return fail(ctx, MRT_ERR_INVALID, "refit: no instances");
	int rc = refit_precheck(ctx, flags, false);
	if (rc) return rc;
	uint64_t total = 0;
	for (uint32_t i = 0; i < n_instances; i++) total += instances[i].n_tris;
	if (total != ctx->n_tris) return fail(ctx, MRT_ERR_INVALID, "refit: the instances' triangle count differs from the scene's");
	if ((rc = ensure(ctx, ctx->refit_in, (size_t)total * sizeof(mrt_tri64)))) return rc;
	if ((rc = mrt_flatten_instances(ctx, verts9, n_mesh_tris, instances, n_instances, flags, (mrt_tri64 *)ctx->refit_in.ptr))) return rc;
	return mrt::refit_flat_scene(ctx, (const mrt_tri64 *)ctx->refit_in.ptr);
}

int mrt_refit_two_level_scene(mrt_ctx *ctx, const float *verts9, uint32_t n_mesh_tris, const mrt_instance *instances,
		uint32_t n_instances, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!verts9 || !instances || n_instances == 0 || n_mesh_tris == 0) return fail(ctx, MRT_ERR_INVALID, "refit: null or empty argument");
	int rc = refit_precheck(ctx, flags, true);
	if (rc) return rc;
	const bool inst_on_device = (flags & MRT_BUILD_INSTANCES_ON_DEVICE) != 0;
	if ((rc = mrt::check_two_level_refit(ctx->two_level, inst_on_device ? nullptr : instances, n_instances, n_mesh_tris, ctx->err, sizeof(ctx->err)))) return rc;
	// device instances: their mesh ranges and transforms checked on the device, before any row of the scene is written
	if (inst_on_device && (rc = mrt::device_update_tlas(ctx, instances, n_instances, true, 0, true, nullptr))) return rc;
	// the staged triangle rows, then (host vertices) a copy of the mesh array behind them
	const size_t tri_bytes = (size_t)ctx->n_tris * sizeof(mrt_tri64), vert_bytes = (size_t)n_mesh_tris * 9u * sizeof(float);
	const bool on_device = (flags & MRT_BUILD_TRIS_ON_DEVICE) != 0;
	if ((rc = ensure(ctx, ctx->refit_in, tri_bytes + (on_device ? 0u : vert_bytes)))) return rc;
	const float *d_verts9 = verts9;
	if (!on_device) {
		float *dst = (float *)((char *)ctx->refit_in.ptr + tri_bytes);
		HIP_TRY(ctx, hipMemcpyAsync(dst, verts9, vert_bytes, hipMemcpyHostToDevice, ctx->stream));
		d_verts9 = dst;
	}
	return mrt::refit_two_level_scene(ctx, d_verts9, instances, n_instances, inst_on_device);
}

} // extern "C"
