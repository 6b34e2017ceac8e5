// prep_kernels.hip — gfx950 kernels that prepare a scene or a cast and walk nothing: the row arrays of the packet walks, standalone ray
// generation, hit tokens back to records, the row-width detection of coherent batches and the two sort keys, each with its launcher
// (called from api.hip, cast.hip and refit.hip).  They share device_common.h with the walks of kernels.hip and are compiled apart
// from them.  The arithmetic is the canonical form of DESIGN.md ("Arithmetic"), as in kernels.hip.
#include <hip/hip_runtime.h>
#include <cfloat>
#include <type_traits>
#include "mrt_internal.h"
#include "lane_map.h"
#include "walk_steps.h"

namespace mrt {

#include "device_common.h"
#include "dispatch.h"

// ---- the unified row array of packet_rows_kernel.h ------------------------------------------------------------
// rows[0, n_nodes) = the wide nodes with leaf refs rebased to row indices (0x80000000 | (n_nodes + first slot));
// rows[n_nodes + s] = triangle slot s as {v0,id | e1,layers | e2,flags | normal}: the hot and the cold row of the
// triangle in one 64-byte line, which is the reference's GPUTrianglePacked row (src/api/gpu_types.h:44-51).
__global__ __launch_bounds__(MRT_WG) void build_rows_kernel(const DevNode *nodes, const TriHot *hot, const TriCold *cold,
		uint32_t n_nodes, uint32_t n_tris, float4 *rows)
{
	const uint64_t g = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (g >= (uint64_t)n_nodes + n_tris) return;
	float4 *out = rows + g * 4u;
	if (g < n_nodes) {
		const float4 *n = reinterpret_cast<const float4 *>(nodes) + g * 4u;
		float4 a = n[0], b = n[1];
		uint32_t l = __float_as_uint(a.w), r = __float_as_uint(b.w);
		if (l >= kLeafBit) l = kLeafBit | (n_nodes + (l & 0x7FFFFFFFu));
		if (r >= kLeafBit) r = kLeafBit | (n_nodes + (r & 0x7FFFFFFFu));
		a.w = __uint_as_float(l); b.w = __uint_as_float(r);
		out[0] = a; out[1] = b; out[2] = n[2]; out[3] = n[3];
	} else {
		const uint64_t s = g - n_nodes;
		const float4 *t = reinterpret_cast<const float4 *>(hot) + s * 3u;
		out[0] = t[0]; out[1] = t[1]; out[2] = t[2];
		out[3] = reinterpret_cast<const float4 *>(cold)[s];
	}
}

hipError_t launch_build_rows(const DevNode *nodes, const TriHot *hot, const TriCold *cold, uint32_t n_nodes, uint32_t n_tris,
		void *rows, hipStream_t stream)
{
	return launch_per_entry<false>(build_rows_kernel, (uint64_t)n_nodes + n_tris, stream, nodes, hot, cold, n_nodes, n_tris, reinterpret_cast<float4 *>(rows));
}

// ---- the row array of packet_quad_kernel.h: units of 64 bytes; 4-wide node i = the 128-byte row at unit 2i with
// its boxes as {min, max} pairs per axis and its refs rebased (inner -> 2 * index, leaf -> 0x80000000 |
// (2 * n_nodes4 + first slot)); triangle slot s = the
// 64-byte row at unit 2 * n_nodes4 + s ----
__global__ __launch_bounds__(MRT_WG) void build_rows4_kernel(const Dev4Node *nodes4, const TriHot *hot, const TriCold *cold,
		uint32_t n_nodes4, uint32_t n_tris, float4 *rows)
{
	const uint64_t g = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (g >= (uint64_t)n_nodes4 + n_tris) return;
	if (g < n_nodes4) {
		const Dev4Node &n = nodes4[g];
		float *out = reinterpret_cast<float *>(rows + g * 8u);
		for (int k = 0; k < 4; k++)
			for (int c = 0; c < 3; c++) { out[6 * k + 2 * c] = n.box[k][c]; out[6 * k + 2 * c + 1] = n.box[k][3 + c]; } // {min, max} per axis
		uint32_t *oref = reinterpret_cast<uint32_t *>(out) + 24;
		for (int i = 0; i < 4; i++) {
			const uint32_t ref = n.ref[i];
			oref[i] = ref == kSentinel ? ref : (ref >= kLeafBit ? (kLeafBit | (2u * n_nodes4 + (ref & 0x7FFFFFFFu))) : 2u * ref);
		}
		oref[4] = n.n_children; oref[5] = 0u; oref[6] = 0u; oref[7] = 0u;
	} else {
		const uint64_t s = g - n_nodes4;
		float4 *out = rows + ((uint64_t)2u * n_nodes4 + s) * 4u;
		const float4 *t = reinterpret_cast<const float4 *>(hot) + s * 3u;
		out[0] = t[0]; out[1] = t[1]; out[2] = t[2];
		out[3] = reinterpret_cast<const float4 *>(cold)[s];
	}
}

hipError_t launch_build_rows4(const Dev4Node *nodes4, const TriHot *hot, const TriCold *cold, uint32_t n_nodes4, uint32_t n_tris,
		void *rows, hipStream_t stream)
{
	return launch_per_entry<false>(build_rows4_kernel, (uint64_t)n_nodes4 + n_tris, stream, nodes4, hot, cold, n_nodes4, n_tris, reinterpret_cast<float4 *>(rows));
}

// ---- standalone ray generation (mrt_generate_grid) ---------------------------------
__global__ __launch_bounds__(MRT_WG) void grid_rays_kernel(const TraceParams p, mrt_ray32 *out)
{
	const uint64_t g = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (g >= p.count) return;
	RayRegs r;
	grid_ray(p, (uint32_t)(g % p.grid_w), (uint32_t)(g / p.grid_w), r);
	float4 *q = reinterpret_cast<float4 *>(out) + g * 2u;
	float4 a, b;
	a.x = r.ox; a.y = r.oy; a.z = r.oz; a.w = r.t_max;
	b.x = r.dx; b.y = r.dy; b.z = r.dz; b.w = r.t_min;
	q[0] = a; q[1] = b;
}

hipError_t launch_grid_rays(const TraceParams &p, mrt_ray32 *out, hipStream_t stream)
{
	return launch_per_entry<false>(grid_rays_kernel, p.count, stream, p, out);
}

// ---- hit tokens -> full hit records (mrt_expand_tokens) -----------------------------------
// A token names the winning triangle of a ray (leaf-order slot, 0xFFFFFFFF = miss).  Everything
// else in the record is a function of (ray, triangle): t, u, v come out of one Moller-Trumbore
// evaluation, the walks' form without its rejections (walk_steps.h tri_tuv), so the rebuilt record is the record
// the trace would have stored, bit for bit.  This is what lets a multi-GPU gather move 4 bytes
// per ray over xGMI instead of 32 (sharded.py): the root rebuilds the records from its own copy
// of the scene and the sender's camera.
__global__ __launch_bounds__(MRT_WG) void expand_tokens_kernel(const TraceParams p, const uint32_t *tokens)
{
	const uint64_t g = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (g >= p.count) return;
	RayRegs r;
	uint32_t px = 0, py = 0;
	if (p.in_fmt == IN_GRID) { px = (uint32_t)(g % p.grid_w); py = (uint32_t)(g / p.grid_w); }
	load_ray(p, g, px, py, r);
	const uint32_t slot = tokens[g];
	if (slot >= p.n_tris) { // miss (0xFFFFFFFF), or a token that is not from this scene: never read out of bounds
		store_hit(p, g, r, r.t_max, -1, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0u, slot);
		return;
	}
	const float4 *t3 = reinterpret_cast<const float4 *>(p.tri_hot) + (size_t)slot * 3u;
	const float4 q0 = t3[0], q1 = t3[1], q2 = t3[2];
	float t, u, v;
	tri_tuv(r.o(), r.d(), q0, q1, q2, t, u, v);
	const float4 nn = reinterpret_cast<const float4 *>(p.tri_cold)[slot];
	store_hit(p, g, r, t, (int32_t)__float_as_uint(q0.w), u, v, nn.x, nn.y, nn.z, __float_as_uint(q1.w), slot);
}

// The same for a two-level scene: a token is {triangle slot in the mesh arrays, DevInstance row}.  The ray goes to the
// instance's mesh space as in the walks (walk_steps.h to_instance_space), Moller-Trumbore runs there, and
// finish_two_level_ray writes the record: flat id = the instance's id base + the mesh-local id, the instance's layer mask,
// normalize(basis * n), position on the world ray.
__global__ __launch_bounds__(MRT_WG) void expand_two_level_tokens_kernel(const TraceParams p, const uint2 *tokens)
{
	const uint64_t g = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (g >= p.count) return;
	RayRegs r;
	uint32_t px = 0, py = 0;
	if (p.in_fmt == IN_GRID) { px = (uint32_t)(g % p.grid_w); py = (uint32_t)(g / p.grid_w); }
	load_ray(p, g, px, py, r);
	const uint2 tok = tokens[g];
	const uint32_t slot = tok.x, inst = tok.y;
	if (slot >= p.n_tris || inst >= p.n_instances) { // miss, or a token that is not from this scene: never read out of bounds
		finish_two_level_ray(p, g, r, r.t_max, 0.0f, 0.0f, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u);
		return;
	}
	const float4 *row = reinterpret_cast<const float4 *>(p.instances) + (size_t)inst * 8u;
	const float4 m0 = row[0], m1 = row[1], m2 = row[2], meta = row[5];
	V3 o, d;
	to_instance_space(m0, m1, m2, r.o(), r.d(), o, d);
	const float4 *t3 = reinterpret_cast<const float4 *>(p.tri_hot) + (size_t)slot * 3u;
	const float4 q0 = t3[0], q1 = t3[1], q2 = t3[2];
	float t, u, v;
	tri_tuv(o, d, q0, q1, q2, t, u, v);
	finish_two_level_ray(p, g, r, t, u, v, slot, __float_as_uint(meta.z) + __float_as_uint(q0.w), inst);
}

hipError_t launch_expand_tokens(const TraceParams &p, const uint32_t *tokens, hipStream_t stream)
{
	if (p.instances != nullptr) // a two-level scene: 8-byte tokens {triangle slot, instance row}
		return launch_per_entry<false>(expand_two_level_tokens_kernel, p.count, stream, p, reinterpret_cast<const uint2 *>(tokens));
	return launch_per_entry<false>(expand_tokens_kernel, p.count, stream, p, tokens);
}

// ---- row-width detection for coherent batches ------------------------------------------
// RayQuery::coherent (src/api/ray_query.h:69-76) says "these are primary camera rays" but
// the reference's cast_rays(rays, results, count) carries no image width, and a wave of 64
// consecutive rays is a 64x1 pixel strip.  One small block looks at the first rows: inside
// a row consecutive directions differ by one pixel step, at a row end they jump back by a
// whole row.  If the first two jumps sit at w and 2w and w x rows tiles the batch exactly,
// the trace kernel maps its lanes to 2^k x 64/2^k pixel tiles instead.  Purely a speed
// decision: any lane -> ray mapping gives the same results.
#define MRT_DETECT_THREADS 1024
#define MRT_DETECT_MAX_RAYS 65536u
// scratch layout (uint64 words): [0 .. 1023] jump bit masks, [1024] finished-block ticket
__device__ __forceinline__ void ray_dir(const void *rays, uint32_t in_fmt, uint64_t i, float &x, float &y, float &z)
{
	if (in_fmt == IN_HOST60) {
		const float *h = reinterpret_cast<const float *>(rays) + i * 15u;
		x = h[3]; y = h[4]; z = h[5];
	} else {
		const float4 b = reinterpret_cast<const float4 *>(rays)[i * 2u + 1u];
		x = b.x; y = b.y; z = b.z;
	}
}
__global__ __launch_bounds__(MRT_DETECT_THREADS) void detect_grid_kernel(const void *rays, uint32_t in_fmt, uint64_t count,
		uint32_t tile_w_log2, unsigned long long *scratch, uint32_t *out, uint32_t *host_out)
{
	__shared__ uint32_t first, second, is_last;
	const uint32_t m = (uint32_t)(count < (uint64_t)MRT_DETECT_MAX_RAYS ? count : (uint64_t)MRT_DETECT_MAX_RAYS);
	float ax, ay, az, bx, by, bz;
	ray_dir(rays, in_fmt, 0, ax, ay, az);
	ray_dir(rays, in_fmt, 1, bx, by, bz);
	const float step2 = (bx - ax) * (bx - ax) + (by - ay) * (by - ay) + (bz - az) * (bz - az);
	const float thr = 36.0f * step2; // a jump of more than 6 pixel steps
	// phase 1: every thread looks at one pair (i-1, i); one 64-bit jump mask per wave
	const uint32_t i = blockIdx.x * MRT_DETECT_THREADS + threadIdx.x;
	bool jump = false, wide = false;
	if (i >= 1 && i < m) {
		ray_dir(rays, in_fmt, i - 1, ax, ay, az);
		ray_dir(rays, in_fmt, i, bx, by, bz);
		const float d2 = (bx - ax) * (bx - ax) + (by - ay) * (by - ay) + (bz - az) * (bz - az);
		jump = d2 > thr;
		wide = !(d2 <= 0.01f); // neighbours more than ~6 degrees apart (or NaN): not what a packet wants
	}
	const unsigned long long mask = __ballot(jump);
	const unsigned long long wmask_dir = __ballot(wide);
	if ((threadIdx.x & 63u) == 0u) {
		__hip_atomic_store(&scratch[i >> 6], mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (wmask_dir) atomicAdd(&scratch[1025], (unsigned long long)__builtin_popcountll(wmask_dir));
	}
	// hand-off to the block that finishes last (agent-scope release / acquire, guide G16)
	__threadfence();
	__syncthreads();
	if (threadIdx.x == 0) {
		const unsigned long long t = atomicAdd(&scratch[1024], 1ull);
		is_last = (t == (unsigned long long)gridDim.x - 1ull) ? 1u : 0u;
		first = 0xFFFFFFFFu; second = 0xFFFFFFFFu;
	}
	__syncthreads();
	if (!is_last) return;
	__threadfence();
	// phase 2 (one block): first and second jump over the <= 1024 mask words
	const uint32_t words = (m + 63u) >> 6;
	unsigned long long wmask = 0ull;
	if (threadIdx.x < words) wmask = __hip_atomic_load(&scratch[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	if (wmask) atomicMin(&first, threadIdx.x * 64u + (uint32_t)__builtin_ctzll(wmask));
	__syncthreads();
	const uint32_t f = first;
	if (f != 0xFFFFFFFFu && threadIdx.x >= (f >> 6)) {
		unsigned long long rest = wmask;
		if (threadIdx.x == (f >> 6)) rest &= ~((2ull << (f & 63u)) - 1ull); // clear bits <= f
		if (rest) atomicMin(&second, threadIdx.x * 64u + (uint32_t)__builtin_ctzll(rest));
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t w = first, rows = 0, tiles_x = 0;
		const uint32_t tw = 1u << tile_w_log2, th = 64u >> tile_w_log2;
		bool ok = step2 > 0.0f && w != 0xFFFFFFFFu && w >= 16u && (w % tw) == 0u && (count % w) == 0ull;
		if (ok) {
			const uint64_t r = count / w;
			ok = r <= 0xFFFFFFFFull && (r % th) == 0ull && (2ull * w >= m || second == 2u * w);
			rows = (uint32_t)r; tiles_x = w >> tile_w_log2;
		}
		out[0] = ok ? w : 0u; out[1] = ok ? rows : 0u; out[2] = ok ? tiles_x : 0u;
		// "coherent" was only the caller's word: if more than 1 in 8 neighbouring rays point
		// somewhere else, the batch goes to the lane kernel (out[3] = 1) instead of packets
		const unsigned long long n_wide = __hip_atomic_load(&scratch[1025], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		// ... and so does a small batch in which no row width was found: packets of 64 consecutive rays are no match for one lane
		// per ray there (with a width, small batches go in pieces of 4 or 16 rays: launch_policy.cpp quarter_rule)
		out[3] = (n_wide * 8ull > (unsigned long long)m || (!ok && count < 32768ull)) ? 1u : 0u;
		// the same four words to host-mapped memory: read by the host after it has waited for the stream
		if (host_out) { host_out[0] = out[0]; host_out[1] = out[1]; host_out[2] = out[2]; host_out[3] = out[3]; }
		scratch[1024] = 0ull; scratch[1025] = 0ull; // ticket / counter for the next launch (stream ordered)
	}
}

hipError_t launch_detect_grid(const void *rays, uint32_t in_fmt, uint64_t count, uint32_t tile_w_log2,
		unsigned long long *scratch, uint32_t *out, uint32_t *host_out, hipStream_t stream)
{
	const uint32_t m = (uint32_t)(count < (uint64_t)MRT_DETECT_MAX_RAYS ? count : (uint64_t)MRT_DETECT_MAX_RAYS);
	const uint32_t blocks = (m + MRT_DETECT_THREADS - 1) / MRT_DETECT_THREADS;
	hipLaunchKernelGGL(detect_grid_kernel, dim3(blocks), dim3(MRT_DETECT_THREADS), 0, stream, rays, in_fmt, count, tile_w_log2, scratch, out, host_out);
	return hipGetLastError();
}

// ---- Morton keys: src/dispatch/ray_sort.h:41-76 -------------------------------------
__device__ __forceinline__ uint32_t spread10(uint32_t v)
{
	v &= 0x000003FFu;
	v = (v | (v << 16)) & 0x030000FFu;
	v = (v | (v << 8)) & 0x0300F00Fu;
	v = (v | (v << 4)) & 0x030C30C3u;
	v = (v | (v << 2)) & 0x09249249u;
	return v;
}
__device__ __forceinline__ uint32_t quant10(float v)
{
	float n = (v + 1.0f) * 0.5f;
	n = fmaxf(0.0f, fminf(1.0f, n));
	return (uint32_t)(n * 1023.0f);
}
__global__ __launch_bounds__(MRT_WG) void morton_keys_kernel(const void *rays, uint32_t in_fmt, uint64_t count,
		uint32_t *keys, uint32_t *index)
{
	const uint64_t g = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (g >= count) return;
	float dx, dy, dz;
	if (in_fmt == IN_HOST60) {
		const float *h = reinterpret_cast<const float *>(rays) + g * 15u;
		dx = h[3]; dy = h[4]; dz = h[5];
	} else {
		const float4 b = reinterpret_cast<const float4 *>(rays)[g * 2u + 1u];
		dx = b.x; dy = b.y; dz = b.z;
	}
	keys[g] = (spread10(quant10(dx)) << 2) | (spread10(quant10(dy)) << 1) | spread10(quant10(dz));
	if (index) index[g] = (uint32_t)g;
}

hipError_t launch_morton_keys(const void *rays, uint32_t in_fmt, uint64_t count, uint32_t *keys, uint32_t *index, hipStream_t stream)
{
	return launch_per_entry<false>(morton_keys_kernel, count, stream, rays, in_fmt, count, keys, index);
}

// ---- sort key for incoherent batches --------------------------------------------------
// The reference sorts by direction only (ray_sort.h:64-76), which groups nothing when the
// origins are scattered (config C4).  Results do not depend on the order, so the sort that
// feeds the lane kernel uses origin first: 6 bits per axis of the origin inside the scene
// bounds (Morton, 18 bits) above 4 bits per axis of the direction (Morton, 12 bits).
// Rays that start in the same ~1/64-of-the-scene cell and point the same way share a wave.
__global__ __launch_bounds__(MRT_WG) void origin_dir_keys_kernel(const void *rays, uint32_t in_fmt, uint64_t count,
		float bx, float by, float bz, float sx, float sy, float sz, uint32_t *keys, uint32_t *index)
{
	const uint64_t g = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (g >= count) return;
	float ox, oy, oz, dx, dy, dz;
	if (in_fmt == IN_HOST60) {
		const float *h = reinterpret_cast<const float *>(rays) + g * 15u;
		ox = h[0]; oy = h[1]; oz = h[2]; dx = h[3]; dy = h[4]; dz = h[5];
	} else {
		const float4 a = reinterpret_cast<const float4 *>(rays)[g * 2u], b = reinterpret_cast<const float4 *>(rays)[g * 2u + 1u];
		ox = a.x; oy = a.y; oz = a.z; dx = b.x; dy = b.y; dz = b.z;
	}
	auto q = [](float v, float lo, float scale, float top) { // clamp handles NaN / out-of-scene origins
		const float n = fmaxf(0.0f, fminf(top, (v - lo) * scale));
		return (uint32_t)n;
	};
	const uint32_t qx = q(ox, bx, sx, 63.0f), qy = q(oy, by, sy, 63.0f), qz = q(oz, bz, sz, 63.0f);
	const uint32_t ex = q(dx, -1.0f, 8.0f, 15.0f), ey = q(dy, -1.0f, 8.0f, 15.0f), ez = q(dz, -1.0f, 8.0f, 15.0f);
	const uint32_t ko = (spread10(qx) << 2) | (spread10(qy) << 1) | spread10(qz); // 18 bits
	const uint32_t kd = (spread10(ex) << 2) | (spread10(ey) << 1) | spread10(ez); // 12 bits
	keys[g] = (ko << 12) | kd;
	if (index) index[g] = (uint32_t)g;
}

hipError_t launch_origin_dir_keys(const void *rays, uint32_t in_fmt, uint64_t count, const float lo[3], const float hi[3],
		uint32_t *keys, uint32_t *index, hipStream_t stream)
{
	float s[3];
	for (int k = 0; k < 3; k++) { const float e = hi[k] - lo[k]; s[k] = e > 0.0f ? 64.0f / e : 0.0f; }
	return launch_per_entry<false>(origin_dir_keys_kernel, count, stream, rays, in_fmt, count, lo[0], lo[1], lo[2], s[0], s[1], s[2], keys, index);
}

} // namespace mrt
