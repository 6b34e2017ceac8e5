// lane_walk.h -- the walk of trace_lane_kernel and trace_source_lane_kernel (kernels.hip): one lane = one ray, a per-lane stack in LDS
// (entry d of lane l at dword d*64 + l of the wave's region: the 64 lanes of a push or a pop hit 64 consecutive dwords).  Included by
// kernels.hip inside namespace mrt, after source_common.h.  The arithmetic is the canonical form, written out here: called from
// walk_steps.h the same steps measured 1 to 4 % slower.
// p = the cast, s = the parameters of the kernel's source family (source_common.h; NoSource in a SRC_CAST kernel).  SRC_CAST: the
// batch's rays (load_ray); else the family's source_entry makes the ray of an entry or stores its result.
#pragma once

template <int SRC, bool ANY_HIT, bool COUNT, class S>
__device__ __forceinline__ void lane_walk(const TraceParams &p, const S &s)
{
	static_assert((SRC == SRC_CAST) == std::is_same<S, NoSource>::value, "lane_walk: s is NoSource exactly for SRC_CAST");
	static_assert(SRC == SRC_CAST || !COUNT, "lane_walk: no ray source counts (source_entry checks the family's modes)");
	extern __shared__ uint32_t lds_stack[];
	if (skip_launch(p)) return;
	uint32_t block = blockIdx.x;
	if (p.xcd_swizzle) { // contiguous band of the batch per XCD (blocks are dealt round-robin over 8 XCDs)
		const uint32_t per = gridDim.x >> 3;
		if (block < (per << 3)) block = (block & 7u) * per + (block >> 3);
	}
	uint64_t ray_idx = 0; uint32_t px = 0, py = 0;
	if (!lane_ray_index(p, block, ray_idx, px, py)) return;
	RayRegs r;
	if constexpr (SRC == SRC_CAST) load_ray(p, ray_idx, px, py, r);
	else if (!source_entry<SRC, ANY_HIT>(p, s, ray_idx, r)) return;

	float best_t = r.t_max, best_u = 0.0f, best_v = 0.0f;
	uint32_t best_slot = 0xFFFFFFFFu, best_id = 0xFFFFFFFFu;
	uint32_t n_nodes = 0, n_tris = 0, max_sp = 0;

	if (!(r.t_min >= r.t_max)) { // degenerate rays are misses, glsl:214-222
		const float ix = safe_inv(r.dx), iy = safe_inv(r.dy), iz = safe_inv(r.dz);
		const float nrx = -(r.ox * ix), nry = -(r.oy * iy), nrz = -(r.oz * iz);
		const uint32_t lane = threadIdx.x & (MRT_WAVE - 1);
		const uint32_t wave = threadIdx.x / MRT_WAVE;
		uint32_t sp = wave * (p.stack_depth * MRT_WAVE) + lane; // dword index of this lane's stack bottom
		lds_stack[sp] = kSentinel; sp += MRT_WAVE;
		uint32_t cur = 0; // the root is always a wide node (root leaves are wrapped on the host)
		const float4 *nodes = reinterpret_cast<const float4 *>(p.nodes);
		const float4 *hot = reinterpret_cast<const float4 *>(p.tri_hot);

		while (cur != kSentinel) {
			// ---- inner nodes: glsl:243-318 ----
			while (cur < kSentinel) {
				const float4 *n = nodes + (size_t)cur * 4u;
				const float4 a = n[0], b = n[1], c = n[2], d = n[3];
				if (COUNT) n_nodes++;
				// ray_aabb (glsl:84-99) for both children, clamped to [t_min, best_t]
				const float l0x = fma_(a.x, ix, nrx), l1x = fma_(b.x, ix, nrx);
				const float l0y = fma_(a.y, iy, nry), l1y = fma_(b.y, iy, nry);
				const float l0z = fma_(a.z, iz, nrz), l1z = fma_(b.z, iz, nrz);
				const float r0x = fma_(c.x, ix, nrx), r1x = fma_(d.x, ix, nrx);
				const float r0y = fma_(c.y, iy, nry), r1y = fma_(d.y, iy, nry);
				const float r0z = fma_(c.z, iz, nrz), r1z = fma_(d.z, iz, nrz);
				const float tl = fmaxf(fmaxf(fminf(l0x, l1x), fminf(l0y, l1y)), fmaxf(fminf(l0z, l1z), r.t_min));
				const float tlx = fminf(fminf(fmaxf(l0x, l1x), fmaxf(l0y, l1y)), fminf(fmaxf(l0z, l1z), best_t));
				const float tr = fmaxf(fmaxf(fminf(r0x, r1x), fminf(r0y, r1y)), fmaxf(fminf(r0z, r1z), r.t_min));
				const float trx = fminf(fminf(fmaxf(r0x, r1x), fmaxf(r0y, r1y)), fminf(fmaxf(r0z, r1z), best_t));
				const bool hl = tl <= tlx, hr = tr <= trx;
				const uint32_t lref = __float_as_uint(a.w), rref = __float_as_uint(b.w);
				if (hl && hr) { // near child first, far child pushed (glsl:290-305)
					const bool left_near = tl < tr;
					cur = left_near ? lref : rref;
					lds_stack[sp] = left_near ? rref : lref; sp += MRT_WAVE;
					if (COUNT) { const uint32_t dpt = (sp - lane) / MRT_WAVE - wave * p.stack_depth; max_sp = dpt > max_sp ? dpt : max_sp; }
				} else if (hl) cur = lref;
				else if (hr) cur = rref;
				else { sp -= MRT_WAVE; cur = lds_stack[sp]; }
			}
			// ---- leaves: INTERSECT_LEAF, glsl:166-192 ----
			while (cur >= kLeafBit) {
				uint32_t slot = cur & 0x7FFFFFFFu;
				bool last;
				do {
					const float4 *t3 = hot + (size_t)slot * 3u;
					const float4 q0 = t3[0], q1 = t3[1], q2 = t3[2];
					last = (__float_as_uint(q2.w) & kLastInLeaf) != 0u;
					if ((__float_as_uint(q1.w) & p.query_mask) != 0u) {
						if (COUNT) n_tris++;
						// ray_triangle, glsl:105-131 == Triangle::intersect, src/core/triangle.h:56-105
						const float pvx = fma_(r.dy, q2.z, -(r.dz * q2.y));
						const float pvy = fma_(r.dz, q2.x, -(r.dx * q2.z));
						const float pvz = fma_(r.dx, q2.y, -(r.dy * q2.x));
						const float det = dot3(q1.x, q1.y, q1.z, pvx, pvy, pvz);
						if (!(__builtin_fabsf(det) < 1e-8f)) {
							const float inv_det = 1.0f / det;
							const float tvx = r.ox - q0.x, tvy = r.oy - q0.y, tvz = r.oz - q0.z;
							const float u = dot3(tvx, tvy, tvz, pvx, pvy, pvz) * inv_det;
							if (!(u < 0.0f || u > 1.0f)) {
								const float qvx = fma_(tvy, q1.z, -(tvz * q1.y));
								const float qvy = fma_(tvz, q1.x, -(tvx * q1.z));
								const float qvz = fma_(tvx, q1.y, -(tvy * q1.x));
								const float v = dot3(r.dx, r.dy, r.dz, qvx, qvy, qvz) * inv_det;
								if (!(v < 0.0f || u + v > 1.0f)) {
									const float t = dot3(q2.x, q2.y, q2.z, qvx, qvy, qvz) * inv_det;
									// glsl:124 accepts t_min <= t < best_t; an exact tie goes to the lower
									// triangle id so the answer does not depend on the visiting order
									const uint32_t id = __float_as_uint(q0.w);
									if (!(t < r.t_min) && (t < best_t || (t == best_t && best_slot != 0xFFFFFFFFu && id < best_id))) {
										best_t = t; best_u = u; best_v = v; best_slot = slot; best_id = id;
										if (ANY_HIT) last = true;
									}
								}
							}
						}
					}
					slot++;
				} while (!last);
				if (ANY_HIT && best_slot != 0xFFFFFFFFu) { cur = kSentinel; break; }
				sp -= MRT_WAVE; cur = lds_stack[sp];
			}
		}
	}

	// ---- result: glsl:322-327 ----
	if constexpr (!lit_output(SRC, ANY_HIT)) finish_ray(p, ray_idx, r, best_t, best_u, best_v, best_slot); // (a reflection, a bounce: r is its ray)
	else store_lit(p, ray_idx, best_slot == 0xFFFFFFFFu);

	if (COUNT) {
		atomicAdd(&p.counters[kCntRays], 1ull);
		atomicAdd(&p.counters[kCntTris], (unsigned long long)n_tris);
		atomicAdd(&p.counters[kCntNodes], (unsigned long long)n_nodes);
		if (best_slot != 0xFFFFFFFFu) atomicAdd(&p.counters[kCntHits], 1ull);
		atomicMax(&p.counters[kCntMaxStack], (unsigned long long)max_sp);
		// one lane = one ray: every node step is a (divergent) node fetch, every test a triangle row
		atomicAdd(&p.counters[kCntWaveNodeFetch], (unsigned long long)n_nodes);
		atomicAdd(&p.counters[kCntWaveTriFetch], (unsigned long long)n_tris);
	}
}
