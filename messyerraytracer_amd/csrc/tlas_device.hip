// tlas_device.hip — the top level of a two-level scene built on the device (mrt_update_instances_device, and
// mrt_refit_two_level_scene with MRT_BUILD_INSTANCES_ON_DEVICE).  DESIGN.md 4.10.
//
// mrt_update_instances does this step on the host (two_level_prep.cpp refit_two_level): inverse transforms, world boxes, a binned-SAH
// BVH2 over the boxes, then an upload of the TLAS rows and the DevInstance rows.  Here, on the context's stream:
//   1. one thread per instance: its mesh range against the scene's tables, the inverse and the world box with the host's arithmetic
//      (instance_math.h, bit for bit), its registration row into scratch, errors into a status block  (tlas_instances_kernel)
//   2. the status block read back: a refused update has written nothing of the scene
//   3. a tree over the world boxes themselves by device_build_lbvh (radix tree, PLOC or binned SAH; a box input, not triangles)
//   4. the TLAS rows into d_nodes[0, n_rows) and the DevInstance rows in leaf order, with the leaf-end flag  (tlas_commit_kernel)
//   5. the root row read back: the host updates depth, stack bounds and the scene box the sort keys are quantised on
// Casts return the same records after either path: results do not depend on which valid BVH is walked, and the
// DevInstance rows are the host's rows (only their order, the TLAS leaf order, may differ).
#include <cfloat>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>
#include "mrt_context.h"
#include "instance_math.h"
#include "build_rules.h"

namespace mrt {

namespace {

#define TLAS_WG 256

struct TlasInst { uint32_t blas, id_base; };                          // per registered instance: its mesh, the flat id of its first triangle
struct TlasBlas { uint32_t first_tri, n_tris, root, root8; float lo[3], hi[3]; }; // per mesh: range, BLAS roots, mesh-space box

// status block words (in scratch, read back after step 1 and after step 4)
constexpr uint32_t kStBad = 0, kStFirst = 1, kStRoot = 4; // error bits, the first instance with an error, the committed root row (16 words)
constexpr uint32_t kBadMesh = 1u, kBadTransform = 2u, kBadBox = 4u;

// 1. registration row i of instance i (what refit_two_level writes into reg[i]) and its world box
__global__ __launch_bounds__(TLAS_WG) void tlas_instances_kernel(const mrt_instance *in, uint32_t n, const TlasInst *inst_tab, const TlasBlas *blas_tab,
		uint32_t n_blas, DevInstance *reg, Box *wbox, uint32_t *status)
{
	const uint32_t i = blockIdx.x * TLAS_WG + threadIdx.x;
	if (i >= n) return;
	const mrt_instance m = in[i];
	const TlasInst ti = inst_tab[i];
	const TlasBlas b = blas_tab[ti.blas < n_blas ? ti.blas : 0u];
	uint32_t bad = 0u;
	if (m.first_tri != b.first_tri || m.n_tris != b.n_tris) bad |= kBadMesh;
	DevInstance d;
	memset(&d, 0, sizeof(d));
	if (!invert_affine(m.basis, m.origin, d.inv)) bad |= kBadTransform;
	for (int k = 0; k < 9; k++) d.basis[k] = m.basis[k];
	d.root = b.root; d.root8 = b.root8; d.id_base = ti.id_base; d.layers = m.layers; d.index = i;
	Box w;
	world_box(b.lo, b.hi, m.basis, m.origin, w.mn, w.mx);
	for (int k = 0; k < 3; k++)
		if (!__builtin_isfinite(w.mn[k]) || !__builtin_isfinite(w.mx[k])) bad |= kBadBox;
	reg[i] = d;
	wbox[i] = w;
	if (bad) { atomicOr(&status[kStBad], bad); atomicMin(&status[kStFirst], i); }
}

// 4. the TLAS rows (built == nullptr: one instance, the host's wrapped root leaf -- one row whose two sides are the leaf) and slot k
//    of the DevInstance rows = registration row leaf[k].id with the leaf-end flag; row 0 also into the status block
__global__ __launch_bounds__(TLAS_WG) void tlas_commit_kernel(const DevNode *built, uint32_t n_rows, const TriHot *leaf, const DevInstance *reg,
		const Box *wbox, uint32_t n, DevNode *nodes, DevInstance *instances, uint32_t *status)
{
	const uint32_t k = blockIdx.x * TLAS_WG + threadIdx.x;
	if (k < n_rows) {
		DevNode g;
		if (built) g = built[k];
		else {
			const Box w = wbox[0];
			for (int c = 0; c < 3; c++) { g.lmin[c] = g.rmin[c] = w.mn[c]; g.lmax[c] = g.rmax[c] = w.mx[c]; }
			g.left_ref = g.right_ref = kLeafBit; g.left_count = g.right_count = 1u;
		}
		nodes[k] = g;
		if (k == 0u) *reinterpret_cast<DevNode *>(status + kStRoot) = g;
	}
	if (k < n) {
		const uint32_t src = built ? leaf[k].id : 0u;
		DevInstance d = reg[src < n ? src : 0u];
		d.flags = built ? (leaf[k].flags & kLastInLeaf) : kLastInLeaf;
		instances[k] = d;
	}
}

// the scene's tables, from the host copy (two_level); the instance table once per scene, the mesh table after every refit
int upload_tables(mrt_ctx *ctx)
{
	const TwoLevelHost *tl = ctx->two_level;
	if (!ctx->tlas_inst_ok) {
		std::vector<TlasInst> t(tl->n_inst);
		uint64_t id_base = 0;
		for (uint32_t i = 0; i < tl->n_inst; i++) {
			t[i] = TlasInst{ tl->inst_blas[i], (uint32_t)id_base };
			id_base += tl->blas[tl->inst_blas[i]].n_tris;
		}
		int rc = ensure(ctx, ctx->tlas_inst_tab, t.size() * sizeof(TlasInst));
		if (rc) return rc;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->tlas_inst_tab.ptr, t.data(), t.size() * sizeof(TlasInst), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // (t goes out of scope)
		ctx->tlas_inst_ok = true;
	}
	if (!ctx->tlas_blas_ok) {
		std::vector<TlasBlas> t(tl->n_blas);
		for (uint32_t k = 0; k < tl->n_blas; k++) {
			const TwoLevelBlas &b = tl->blas[k];
			t[k] = TlasBlas{ b.first_tri, b.n_tris, b.root, b.root8, { b.lo[0], b.lo[1], b.lo[2] }, { b.hi[0], b.hi[1], b.hi[2] } };
		}
		int rc = ensure(ctx, ctx->tlas_blas_tab, t.size() * sizeof(TlasBlas));
		if (rc) return rc;
		HIP_TRY(ctx, hipMemcpyAsync(ctx->tlas_blas_tab.ptr, t.data(), t.size() * sizeof(TlasBlas), hipMemcpyHostToDevice, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		ctx->tlas_blas_ok = true;
	}
	return MRT_OK;
}

} // namespace

int device_update_tlas(mrt_ctx *ctx, const mrt_instance *instances, uint32_t n, bool on_device, int form, bool check_only, float *ms)
{
	TwoLevelHost *tl = ctx->two_level;
	if (n != tl->n_inst) return fail(ctx, MRT_ERR_INVALID, "two-level scene: the instance count of an update must match the upload");
	int rc = upload_tables(ctx);
	if (rc) return rc;
	// scratch: the status block, the registration rows, the world boxes, the staged instances (host input)
	const size_t o_reg = 256u, o_box = o_reg + align256((size_t)n * sizeof(DevInstance)), o_in = o_box + align256((size_t)n * sizeof(Box)),
			need = o_in + (on_device ? 0u : (size_t)n * sizeof(mrt_instance));
	if ((rc = ensure(ctx, ctx->tlas_work, need))) return rc;
	char *S = (char *)ctx->tlas_work.ptr;
	uint32_t *status = (uint32_t *)S;
	DevInstance *reg = (DevInstance *)(S + o_reg);
	Box *wbox = (Box *)(S + o_box);
	const mrt_instance *d_in = on_device ? instances : (const mrt_instance *)(S + o_in);
	static const uint32_t init[4] = { 0u, 0xFFFFFFFFu, 0u, 0u };
	uint32_t h[4 + 16];
	const uint32_t blocks = (n + TLAS_WG - 1u) / TLAS_WG;

	// 1-2. the rows and boxes into scratch, the verdict read back
	HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
	HIP_TRY(ctx, hipMemcpyAsync(status, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
	if (!on_device) HIP_TRY(ctx, hipMemcpyAsync((void *)d_in, instances, (size_t)n * sizeof(mrt_instance), hipMemcpyHostToDevice, ctx->stream));
	hipLaunchKernelGGL(tlas_instances_kernel, dim3(blocks), dim3(TLAS_WG), 0, ctx->stream, d_in, n, (const TlasInst *)ctx->tlas_inst_tab.ptr,
			(const TlasBlas *)ctx->tlas_blas_tab.ptr, tl->n_blas, reg, wbox, status);
	HIP_TRY(ctx, hipGetLastError());
	HIP_TRY(ctx, hipMemcpyAsync(h, status, 16, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	const uint32_t bad = h[kStBad] & (check_only ? (kBadMesh | kBadTransform) : (kBadMesh | kBadTransform | kBadBox));
	if (bad) {
		std::snprintf(ctx->err, sizeof(ctx->err), "two-level scene: instance %u: %s", h[kStFirst],
				(bad & kBadMesh) ? "an update may move instances, not change their meshes" :
				(bad & kBadTransform) ? "singular or non-finite instance transform" : "non-finite world box");
		return MRT_ERR_INVALID;
	}
	if (check_only) return MRT_OK;

	// 3. the tree over the world boxes (device_build_lbvh wants two or more; one instance is the host's wrapped leaf)
	DeviceBuildResult b;
	uint32_t n_rows = 1u, depth_t = 2u;
	auto drop = [&] {
		if (b.nodes) (void)hipFree(b.nodes);
		if (b.hot) (void)hipFree(b.hot);
		if (b.cold) (void)hipFree(b.cold);
		b.nodes = nullptr; b.hot = nullptr; b.cold = nullptr;
	};
	if (n >= 2u) {
		b.boxes_in = (const float *)wbox;
		if ((rc = device_build_lbvh(nullptr, n, false, false, false, form, &ctx->build_arena, (void *)ctx->stream, &b, ctx->err, sizeof(ctx->err)))) return rc;
		n_rows = b.n_nodes; depth_t = b.depth;
	}
	if (n_rows == 0u || n_rows > tl->tlas_cap) { drop(); return fail(ctx, MRT_ERR_BAD_BVH, "two-level scene: TLAS larger than its reserved range"); }
	uint32_t max_blas = 0, max_blas8 = 0;
	for (uint32_t k = 0; k < tl->n_blas; k++) {
		if (tl->blas[k].depth > max_blas) max_blas = tl->blas[k].depth;
		if (tl->blas[k].stack8 > max_blas8) max_blas8 = tl->blas[k].stack8;
	}
	// pending entries, as refit_two_level counts them: TLAS path + the rest of a TLAS leaf + the return marker + a BLAS path
	const uint32_t depth = depth_t + 2u + max_blas, depth8 = depth_t + 2u + max_blas8;
	if (depth > 64u) { drop(); return fail(ctx, MRT_ERR_UNSUPPORTED, "two-level scene: trees too deep for the per-lane stack"); }

	// 4-5. commit; the root row comes back with the sync
	const uint32_t cover = n_rows > n ? n_rows : n;
	hipLaunchKernelGGL(tlas_commit_kernel, dim3((cover + TLAS_WG - 1u) / TLAS_WG), dim3(TLAS_WG), 0, ctx->stream, b.nodes, n_rows, b.hot, reg, wbox, n,
			ctx->d_nodes, ctx->d_instances, status);
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipMemcpyAsync(h, status, sizeof(h), hipMemcpyDeviceToHost, ctx->stream);
	if (e == hipSuccess) e = hipEventRecord(ctx->ev[1], ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	drop();
	if (e != hipSuccess) {
		free_scene(ctx); // rows may be half written: released rather than kept wrong
		std::snprintf(ctx->err, sizeof(ctx->err), "two-level scene: the top-level commit failed: %s; the scene was released", hipGetErrorString(e));
		return MRT_ERR_HIP;
	}
	// the host copy's TLAS rows (nodes[0, tlas_cap)) and instance rows (inst) are not updated: refit_two_level rewrites both whole
	// before it reads either, and nothing else reads them after an upload
	tl->n_tlas_nodes = n_rows; tl->depth = depth; tl->depth8 = depth8;
	ctx->depth = depth; ctx->stack8 = tl->wide8 ? depth8 : 0;
	ctx->stack_depth = ((depth + 7u) / 8u) * 8u;
	if (ctx->stack_depth < 8) ctx->stack_depth = 8;
	DevNode root;
	std::memcpy(&root, h + kStRoot, sizeof(root));
	for (int c = 0; c < 3; c++) {
		ctx->bounds_lo[c] = std::fmin(root.lmin[c], root.rmin[c]);
		ctx->bounds_hi[c] = std::fmax(root.lmax[c], root.rmax[c]);
	}
	float t = 0.0f;
	if (ms && hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]) == hipSuccess) *ms = t;
	return MRT_OK;
}

} // namespace mrt

extern "C" {

int mrt_update_instances_device(mrt_ctx *ctx, const mrt_instance *instances, uint32_t n_instances, uint32_t flags)
{
	if (!ctx) return MRT_ERR_INVALID;
	if (!ctx->scene || !ctx->two_level) return fail(ctx, MRT_ERR_NO_SCENE, "no two-level scene uploaded");
	if (!instances) return fail(ctx, MRT_ERR_INVALID, "null instances");
	if (flags & ~(uint32_t)(MRT_BUILD_INSTANCES_ON_DEVICE | MRT_BUILD_PLOC | MRT_BUILD_SAH)) return fail(ctx, MRT_ERR_INVALID, "update_instances_device: unknown flag");
	if ((flags & MRT_BUILD_PLOC) && (flags & MRT_BUILD_SAH)) return fail(ctx, MRT_ERR_INVALID, "update_instances_device: one tree form (MRT_BUILD_PLOC or MRT_BUILD_SAH)");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (ctx->pending) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); ctx->pending = false; } // as mrt_update_instances: drained
	float ms = 0.0f;
	const int rc = mrt::device_update_tlas(ctx, instances, n_instances, (flags & MRT_BUILD_INSTANCES_ON_DEVICE) != 0,
			(flags & MRT_BUILD_SAH) ? 2 : (flags & MRT_BUILD_PLOC) ? 1 : 0, false, &ms);
	if (rc == MRT_OK) ctx->stats.last_build_ms = ms;
	return rc;
}

} // extern "C"
