// emitter_build_kernel.h — the resident emitter table built on the device (mrt_build_emitters).  Included by emitters.hip (inside
// namespace mrt).
//
// Five small kernels over the caller's triangles, once per build (not a hot path; a build of 11 076 triangles is a few launches of
// 44 workgroups).  What makes a triangle an emitter, its weight and its row are the header's, one fp32 operation at a time (the unit
// is compiled without contraction); everything summed is an integer, so that the table is the same words whatever the launch's
// block structure:
//   emitter_flag_kernel     per triangle: w, the flag; per workgroup the number of flags; the largest w by an integer atomic max on
//                           its bits (positive floats order as their bits)
//   scan_words_kernel       one workgroup: the exclusive scan of the per-workgroup counts in place, the total to a header word
//   emitter_compact_kernel  per triangle: the flag again, its place = its workgroup's offset + an exclusive scan of the flags within the
//                           workgroup (input order kept); the row with q0 in the place of q; T0 += q0 (64-bit integer atomic)
//   emitter_weight_kernel   per emitter: q = (q0 << 31) / T0 into the row; the inclusive scan of q within the workgroup to the CDF;
//                           the workgroup's sum
//   (scan_words_kernel over those sums, the total to a header word)
//   emitter_cdf_kernel      per emitter: cdf[k] += its workgroup's offset
// Every thread of a workgroup reaches the scans; a thread past the end contributes 0 and reads and writes nothing.
#pragma once

constexpr uint32_t EM_WG = 256u, EM_WAVE = 64u;
// words of the header block (unsigned long long each)
constexpr int EM_HDR_WMAX = 0, EM_HDR_COUNT = 1, EM_HDR_T0 = 2, EM_HDR_TOTAL = 3, EM_HDR_WORDS = 8;

struct EmitterBuildParams {
	const mrt_tri64 *tris;
	uint32_t n_tris;
	const void *shade_rows;    // n_shade_tris x 64 bytes: word 3 of a row is the triangle's material id
	const void *materials;     // n_materials x mrt_material
	uint32_t n_shade_tris, n_materials;
	uint32_t has_ids;          // the material ids are resident
};

// The exclusive scan of v over the workgroup's EM_WG threads, and the workgroup's sum.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t &total)
{
	__shared__ uint32_t wave_sum[EM_WG / EM_WAVE];
	const uint32_t lane = threadIdx.x & (EM_WAVE - 1u), wave = threadIdx.x / EM_WAVE;
	uint32_t inc = v;
#pragma unroll
	for (uint32_t off = 1u; off < EM_WAVE; off <<= 1) {
		const uint32_t below = __shfl_up(inc, off);
		if (lane >= off) inc += below;
	}
	if (lane == EM_WAVE - 1u) wave_sum[wave] = inc;
	__syncthreads();
	uint32_t base = 0u;
	total = 0u;
#pragma unroll
	for (uint32_t w = 0u; w < EM_WG / EM_WAVE; w++) {
		if (w < wave) base += wave_sum[w];
		total += wave_sum[w];
	}
	__syncthreads(); // (the next scan of this workgroup writes wave_sum again)
	return base + (inc - v);
}

// Le, the area and w of triangle t (include/mrt_hip.h); returns w, or 0 where the triangle is no emitter.
struct EmitterFacts { float ler, leg, leb, area; uint32_t material; };
__device__ __forceinline__ float emitter_weight(const EmitterBuildParams &b, const float4 &t0, const float4 &t1, const float4 &t2, EmitterFacts &f)
{
	f.ler = f.leg = f.leb = 0.0f; f.material = 0xFFFFFFFFu;
	const uint32_t id = __float_as_uint(t0.w);
	if (b.has_ids != 0u && id < b.n_shade_tris) {
		const uint32_t mid = reinterpret_cast<const uint32_t *>(b.shade_rows)[(size_t)id * 16u + 3u];
		if (mid < b.n_materials) {
			const float4 *m = reinterpret_cast<const float4 *>(b.materials) + (size_t)mid * 3u;
			const float4 m1 = m[1], m2 = m[2]; // {roughness, specular, emission rg | emission b, energy, flags, -}
			f.material = mid;
			if (m2.y > 0.0f) { f.ler = m1.z * m2.y; f.leg = m1.w * m2.y; f.leb = m2.x * m2.y; }
		}
	}
	const float cx = t1.y * t2.z - t1.z * t2.y, cy = t1.z * t2.x - t1.x * t2.z, cz = t1.x * t2.y - t1.y * t2.x;
	f.area = 0.5f * __builtin_sqrtf((cx * cx + cy * cy) + cz * cz);
	const float w = f.area * ((0.2126f * f.ler + 0.7152f * f.leg) + 0.0722f * f.leb);
	return w > 0.0f && w <= FLT_MAX ? w : 0.0f; // (false for a NaN)
}

__global__ __launch_bounds__(EM_WG) void emitter_flag_kernel(const EmitterBuildParams b, uint32_t *block_count, unsigned long long *hdr)
{
	const uint64_t t = (uint64_t)blockIdx.x * EM_WG + threadIdx.x;
	float w = 0.0f;
	if (t < b.n_tris) {
		const float4 *row = reinterpret_cast<const float4 *>(b.tris) + t * 4u;
		EmitterFacts f;
		w = emitter_weight(b, row[0], row[1], row[2], f);
	}
	uint32_t total;
	block_exclusive_scan(w > 0.0f ? 1u : 0u, total);
	uint32_t bits = __float_as_uint(w); // (w >= 0: the bits order as the floats)
#pragma unroll
	for (uint32_t off = EM_WAVE / 2u; off != 0u; off >>= 1) {
		const uint32_t other = __shfl_xor(bits, off);
		bits = other > bits ? other : bits;
	}
	if ((threadIdx.x & (EM_WAVE - 1u)) == 0u && bits != 0u) atomicMax(reinterpret_cast<uint32_t *>(hdr + EM_HDR_WMAX), bits);
	if (threadIdx.x == 0u) block_count[blockIdx.x] = total;
}

// One workgroup: v[0 .. n) becomes its exclusive scan; *total = the sum.
__global__ __launch_bounds__(EM_WG) void scan_words_kernel(uint32_t *v, uint32_t n, unsigned long long *total)
{
	unsigned long long carry = 0ull;
	for (uint64_t base = 0; base < n; base += EM_WG) {
		const uint64_t k = base + threadIdx.x;
		const uint32_t x = k < n ? v[k] : 0u;
		uint32_t sum;
		const uint32_t ex = block_exclusive_scan(x, sum);
		if (k < n) v[k] = (uint32_t)carry + ex;
		carry += sum;
	}
	if (threadIdx.x == 0u) *total = carry;
}

__global__ __launch_bounds__(EM_WG) void emitter_compact_kernel(const EmitterBuildParams b, const uint32_t *block_offset, unsigned long long *hdr,
		uint32_t n_emit, uint4 *rows)
{
	__shared__ unsigned long long block_t0;
	if (threadIdx.x == 0u) block_t0 = 0ull;
	const uint64_t t = (uint64_t)blockIdx.x * EM_WG + threadIdx.x;
	float w = 0.0f;
	float4 t0 = {}, t1 = {}, t2 = {};
	EmitterFacts f = {};
	if (t < b.n_tris) {
		const float4 *row = reinterpret_cast<const float4 *>(b.tris) + t * 4u;
		t0 = row[0]; t1 = row[1]; t2 = row[2];
		w = emitter_weight(b, t0, t1, t2, f);
	}
	uint32_t total;
	const uint32_t at = block_offset[blockIdx.x] + block_exclusive_scan(w > 0.0f ? 1u : 0u, total); // (the scan's barriers order block_t0 = 0)
	if (w > 0.0f && at < n_emit) {
		const float w_max = __uint_as_float((uint32_t)hdr[EM_HDR_WMAX]);
		const uint32_t q0 = em::first_weight(w, w_max, em::weight_scale(n_emit));
		uint4 *o = rows + (size_t)at * 4u;
		o[0] = make_uint4(__float_as_uint(t0.x), __float_as_uint(t0.y), __float_as_uint(t0.z), q0);
		o[1] = make_uint4(__float_as_uint(t1.x), __float_as_uint(t1.y), __float_as_uint(t1.z), __float_as_uint(t0.w));
		o[2] = make_uint4(__float_as_uint(t2.x), __float_as_uint(t2.y), __float_as_uint(t2.z), __float_as_uint(f.area));
		o[3] = make_uint4(__float_as_uint(f.ler), __float_as_uint(f.leg), __float_as_uint(f.leb), f.material);
		atomicAdd(&block_t0, (unsigned long long)q0);
	}
	__syncthreads();
	if (threadIdx.x == 0u && block_t0 != 0ull) atomicAdd(hdr + EM_HDR_T0, block_t0);
}

__global__ __launch_bounds__(EM_WG) void emitter_weight_kernel(uint4 *rows, uint32_t n_emit, const unsigned long long *hdr, uint32_t *cdf,
		uint32_t *block_sum)
{
	const uint64_t k = (uint64_t)blockIdx.x * EM_WG + threadIdx.x;
	uint32_t q = 0u;
	if (k < n_emit) {
		uint32_t *word = reinterpret_cast<uint32_t *>(rows + (size_t)k * 4u) + 3;
		q = em::final_weight(*word, hdr[EM_HDR_T0]);
		*word = q;
	}
	uint32_t total;
	const uint32_t ex = block_exclusive_scan(q, total);
	if (k < n_emit) cdf[k] = ex + q;
	if (threadIdx.x == 0u) block_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(EM_WG) void emitter_cdf_kernel(uint32_t *cdf, uint32_t n_emit, const uint32_t *block_offset)
{
	const uint64_t k = (uint64_t)blockIdx.x * EM_WG + threadIdx.x;
	if (k < n_emit) cdf[k] += block_offset[blockIdx.x];
}
