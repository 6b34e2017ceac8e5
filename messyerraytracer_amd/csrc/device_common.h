// device_common.h — what every kernel unit shares (kernels.hip, shade_kernels.hip, prep_kernels.hip): the
// lane -> ray map's glue, the camera's rays, and the load of a ray and the store of a record.  Included inside namespace mrt, after
// mrt_internal.h, lane_map.h and walk_steps.h (the canonical arithmetic).  Every function is __forceinline__, so a unit gets the same code whichever unit it is.
#pragma once

#define MRT_WG 256
#define MRT_WAVE 64

// ---- canonical arithmetic: walk_steps.h (fma_, dot3, safe_inv and the steps of a walk), which the unit includes before namespace mrt ----

struct RayRegs {
	float ox, oy, oz, dx, dy, dz, t_min, t_max;
	__device__ __forceinline__ V3 o() const { return {ox, oy, oz}; }
	__device__ __forceinline__ V3 d() const { return {dx, dy, dz}; }
};

// Two launches are queued for a batch declared coherent: the packet kernel and, behind it, the
// lane kernel.  detect_grid_kernel decides on the device which one does the work; the other
// returns here (a few microseconds for an empty grid, no host round trip).
__device__ __forceinline__ bool skip_launch(const TraceParams &p)
{
	return p.skip_flag != nullptr && *p.skip_flag == p.skip_when;
}

// ---- lane -> ray mapping ---------------------------------------------------------
// MAP_LINEAR: thread g traces ray g (or perm[g]).  MAP_TILE8X8: a wave owns an
// 8x8 pixel tile of the row-major grid so its 64 rays share most of their path.
__device__ __forceinline__ bool lane_ray_index_g(const TraceParams &p, uint64_t g, uint64_t &ray_idx, uint32_t &px, uint32_t &py);
__device__ __forceinline__ bool lane_ray_index(const TraceParams &p, uint32_t block, uint64_t &ray_idx, uint32_t &px, uint32_t &py)
{
	return lane_ray_index_g(p, (uint64_t)block * MRT_WG + threadIdx.x, ray_idx, px, py);
}
// The map itself is lane_map.h: what a group's 64 lanes share (the tile: wave_tile) and what differs between them (tile_lane).
//
// tile_order 3: every XCD works on its own column strips of the image.  Workgroups are dealt to the 8 XCDs round-robin
// (workgroup i runs on XCD i & 7), and each XCD has its own 4 MB L2: in row-major launch order every XCD sees every
// tile column, so the rows a band of tiles needs are fetched into all eight L2s (C5: 13 GB of L2 fills per launch for a
// 1.8 GB scene).  Here the image is cut into 8 m strips (about 256 pixels wide), XCD k takes strips k, k + 8, ..., one
// after the other, each from top to bottom: the ~1000 waves an XCD has in flight cover one compact region, and the
// strips of every XCD are spread evenly over the image, so cheap and expensive regions balance (a contiguous band per
// XCD, xcd_swizzle = 1, measured 6 % slower for that reason).  tile_group = consecutive tiles per workgroup.  Row-major
// order when the width does not split into 8 m strips of whole workgroups.

// The launch's grid as lane_map.h takes it; false = the linear map.  The schedule of the previous frame (launch slot -> unit of
// tile_unit consecutive tiles) counts only if it is a schedule of THIS grid (a batch whose row width is found on the device,
// MAP_AUTO, was scheduled from the last cast's width).
__device__ __forceinline__ bool tile_grid(const TraceParams &p, TileGrid &g)
{
	uint32_t lane_map = p.lane_map;
	g.grid_w = p.grid_w; g.rows = p.rows; g.tiles_x = p.tiles_x;
	if (lane_map == MAP_AUTO) { // row width found on the device by detect_grid_kernel (0 = not a grid)
		const uint32_t w = p.auto_grid[0];
		lane_map = w ? MAP_TILE8X8 : MAP_LINEAR;
		g.grid_w = w; g.rows = p.auto_grid[1]; g.tiles_x = p.auto_grid[2];
	}
	g.k = p.tile_w_log2; g.tiles_y = tile_rows_of(g.rows, g.k);
	g.order = p.tile_order; g.group = p.tile_group; g.quarter_all = p.quarter_all;
	g.sched = nullptr; g.unit = 1u; g.sched_slots = 0u;
	if (lane_map != MAP_TILE8X8) return false;
	if (!p.quarter_all && p.tile_sched != nullptr && sched_matches((uint64_t)g.tiles_x * g.tiles_y, p.tile_unit, p.n_units)) {
		g.sched = p.tile_sched; g.unit = p.tile_unit; g.sched_slots = p.sched_hdr ? p.sched_hdr[2] : p.n_units;
	}
	return true;
}
// the linear map's lane: entry -> ray (perm), and its pixel for rays made from a camera
__device__ __forceinline__ bool linear_ray(const TraceParams &p, uint64_t group, uint32_t l, uint64_t &ray_idx, uint32_t &px, uint32_t &py)
{
	uint64_t e = 0;
	if (!linear_lane(group, l, p.sparse_lanes, p.count, e)) return false;
	ray_idx = p.perm ? (uint64_t)p.perm[e] : e;
	if (p.in_fmt == IN_GRID) { px = (uint32_t)(ray_idx % p.grid_w); py = (uint32_t)(ray_idx / p.grid_w); }
	return true;
}

// g = virtual thread index: 64 consecutive g form one wave-sized group of rays
__device__ __forceinline__ bool lane_ray_index_g(const TraceParams &p, uint64_t g, uint64_t &ray_idx, uint32_t &px, uint32_t &py)
{
	TileGrid tg;
	if (tile_grid(p, tg)) return tile_lane(tg, wave_tile(tg, g >> 6), (uint32_t)g & 63u, ray_idx, px, py);
	return linear_ray(p, g >> 6, (uint32_t)g & 63u, ray_idx, px, py);
}

// What a wave's schedule unit cost (shader cycles, modulo 2^32), for the next frame's longest-first launch order.  The
// start time is parked in the cost word itself (note_tile_start) and replaced by the difference at the end
// (note_tile_cost): nothing stays in registers across the walk.  One lane per wave calls; a unit belongs to one wave.
__device__ __forceinline__ bool tile_cost_word(const TraceParams &p, uint64_t g_first, uint32_t *&park, uint32_t *&sum, uint32_t &what)
{
	if (p.tile_cost == nullptr) return false;
	uint32_t rows = p.rows, tiles_x = p.tiles_x;
	if (p.lane_map == MAP_AUTO) { if (p.auto_grid[0] == 0u) return false; rows = p.auto_grid[1]; tiles_x = p.auto_grid[2]; }
	else if (p.lane_map != MAP_TILE8X8) return false;
	const uint32_t k = p.tile_w_log2, tiles_y = (rows + (64u >> k) - 1u) >> (6u - k);
	if (!sched_matches((uint64_t)tiles_x * tiles_y, p.tile_unit, p.n_units)) return false; // not the grid the arrays were sized for
	const uint64_t group = g_first >> 6;
	const uint64_t slot = p.tile_unit == 1u ? group : (p.tile_unit == 2u ? group >> 1 : group / p.tile_unit);
	what = 0u;
	if (p.tile_sched == nullptr) { if (slot >= p.n_units) return false; park = sum = p.tile_cost + slot; return true; }
	if (slot >= (p.sched_hdr ? p.sched_hdr[2] : p.n_units)) return false;
	const uint32_t e = p.tile_sched[slot], id = e & 0x0FFFFFFFu;
	what = e >> 28;
	if (what == 0u) { park = sum = p.tile_cost + id; return true; }
	park = p.tile_cost + p.n_units + slot; // a piece of a unit: its own word for the start time, its share added to the unit's
	sum = p.tile_cost + id / p.tile_unit;
	return true;
}
__device__ __forceinline__ void note_tile_start(const TraceParams &p, uint64_t g_first)
{
	uint32_t *park, *sum, what;
	if (tile_cost_word(p, g_first, park, sum, what)) *park = (uint32_t)__builtin_amdgcn_s_memtime();
}
// A unit launched in pieces notes what it would have cost in one piece, as well as that can be said: two single tiles take
// about 1.3 x their pair, the eight quarter tiles of a pair 1.5 x the pair, the four of a tile 1.15 x the tile (MRT_SCHED_DUMP
// of consecutive renewals of one grid, 1920x1080 on the C3 scene: the same pair 1.43 M cycles whole, 1.82 M as two tiles,
// 2.1 M as eight quarters) -- so that a unit is ranked as what it is, not as the sum of its pieces.
__device__ __forceinline__ void note_tile_cost(const TraceParams &p, uint64_t g_first)
{
	uint32_t *park, *sum, what;
	if (!tile_cost_word(p, g_first, park, sum, what)) return;
	uint32_t d = (uint32_t)__builtin_amdgcn_s_memtime() - *park;
	if (park == sum) { *sum = d ? d : 1u; return; }
	if (what == 1u) d = d - (d >> 2);                                  // x 3/4
	else d = p.tile_unit == 2u ? (d >> 1) + (d >> 3) + (d >> 4) : d - (d >> 3); // quarters: x 11/16 of a pair's eight, x 7/8 of a tile's four
	atomicAdd(sum, d ? d : 1u);
}

// Primary-ray grids.  MRT_CAMERA_DEBUG_GRID: RayTracerDebug::cast_debug_rays, src/godot/raytracer_debug.cpp:585-596
// (basis / half extents precomputed on the host, mrt_camera_look, :573-583).  MRT_CAMERA_PERSPECTIVE /
// _ORTHOGRAPHIC: RayCamera::_generate_perspective / _generate_orthographic, src/modules/graphics/
// ray_camera.h:234-273 (v flipped; Basis::xform = one dot product per row, summed left to right; the
// jittered form of :106-122 with the pixel centre 0.5 as the default offset).  Plain float operations in the
// reference's order (nothing is contracted): bit-identical to the host loops.
__device__ __forceinline__ void grid_ray(const TraceParams &p, uint32_t px, uint32_t py, RayRegs &r)
{
	const mrt_camera &c = p.cam;
	float dx, dy, dz;
	r.ox = c.origin[0]; r.oy = c.origin[1]; r.oz = c.origin[2];
	if (c.kind == MRT_CAMERA_DEBUG_GRID) {
		const float u = (2.0f * ((float)px + 0.5f) / (float)p.grid_w - 1.0f) * c.half_w;
		const float v = (2.0f * ((float)(py + p.y0) + 0.5f) / (float)p.grid_h - 1.0f) * c.half_h;
		dx = c.fwd[0] + c.right[0] * u + c.up[0] * v;
		dy = c.fwd[1] + c.right[1] * u + c.up[1] * v;
		dz = c.fwd[2] + c.right[2] * u + c.up[2] * v;
	} else {
		const float u = (2.0f * ((float)px + c.jitter_x) * c.inv_w) - 1.0f;
		const float v = 1.0f - (2.0f * ((float)(py + p.y0) + c.jitter_y) * c.inv_h);
		if (c.kind == MRT_CAMERA_PERSPECTIVE) {
			const float vx = u * c.half_w, vy = v * c.half_h; // view_dir = (vx, vy, -1)
			dx = c.right[0] * vx + c.up[0] * vy + c.fwd[0] * -1.0f;
			dy = c.right[1] * vx + c.up[1] * vy + c.fwd[1] * -1.0f;
			dz = c.right[2] * vx + c.up[2] * vy + c.fwd[2] * -1.0f;
		} else { // parallel rays: the direction is -column 2 as it stands (Ray(ray_origin, forward_): not normalised)
			const float sv = v * c.half_h, su = u * c.half_w;
			r.ox = (c.origin[0] + c.up[0] * sv) + c.right[0] * su;
			r.oy = (c.origin[1] + c.up[1] * sv) + c.right[1] * su;
			r.oz = (c.origin[2] + c.up[2] * sv) + c.right[2] * su;
			r.dx = -c.fwd[0]; r.dy = -c.fwd[1]; r.dz = -c.fwd[2];
			r.t_min = c.t_min; r.t_max = c.t_max;
			return;
		}
	}
	const float l2 = dx * dx + dy * dy + dz * dz;
	if (l2 == 0.0f) { dx = dy = dz = 0.0f; }
	else { const float l = __builtin_sqrtf(l2); dx /= l; dy /= l; dz /= l; }
	r.dx = dx; r.dy = dy; r.dz = dz;
	r.t_min = c.t_min; r.t_max = c.t_max;
}

// streaming forms of a 16-byte load and store: data touched once per launch (rays, records) that should not displace the scene's rows
typedef float mrt_v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 stream_load4(const float4 *q)
{
	const mrt_v4f v = __builtin_nontemporal_load(reinterpret_cast<const mrt_v4f *>(q));
	return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void stream_store4(float4 *q, const float4 &a)
{
	const mrt_v4f v = {a.x, a.y, a.z, a.w};
	__builtin_nontemporal_store(v, reinterpret_cast<mrt_v4f *>(q));
}

template <bool STREAM = false>
__device__ __forceinline__ void load_ray(const TraceParams &p, uint64_t idx, uint32_t px, uint32_t py, RayRegs &r)
{
	if (p.in_fmt == IN_GRID) { grid_ray(p, px, py, r); return; }
	float ox, oy, oz, dx, dy, dz, t0, t1;
	if (p.in_fmt == IN_HOST60) { // Ray -> GPURayPacked, gpu_ray_caster.cpp:643-650
		const float *h = reinterpret_cast<const float *>(p.rays) + idx * 15u;
		ox = h[0]; oy = h[1]; oz = h[2]; dx = h[3]; dy = h[4]; dz = h[5];
		t0 = h[12]; t1 = h[13];
	} else {
		const float4 *q = reinterpret_cast<const float4 *>(p.rays) + idx * 2u;
		const float4 a = STREAM ? stream_load4(q) : q[0], b = STREAM ? stream_load4(q + 1) : q[1];
		ox = a.x; oy = a.y; oz = a.z; t1 = a.w;
		dx = b.x; dy = b.y; dz = b.z; t0 = b.w;
	}
	r.ox = ox; r.oy = oy; r.oz = oz; r.dx = dx; r.dy = dy; r.dz = dz; r.t_min = t0; r.t_max = t1;
}

// Result store: bvh_traverse.comp.glsl:322-327, plus the readback conversion of
// gpu_ray_caster.cpp:442-456 (OUT_HOST44) / :482-487 (OUT_BOOL8) fused in.
template <bool STREAM = false>
__device__ __forceinline__ void store_hit(const TraceParams &p, uint64_t idx, const RayRegs &r,
		float t, int32_t prim, float u, float v, float nx, float ny, float nz, uint32_t layers, uint32_t slot)
{
	if (p.out_fmt == OUT_BOOL8) { reinterpret_cast<uint8_t *>(p.hits)[idx] = prim >= 0 ? 1 : 0; return; }
	if (p.out_fmt == OUT_TOKEN4) { reinterpret_cast<uint32_t *>(p.hits)[idx] = prim >= 0 ? slot : 0xFFFFFFFFu; return; }
	if (p.out_fmt == OUT_HOST44) {
		float *h = reinterpret_cast<float *>(p.hits) + idx * 11u;
		uint32_t *hu = reinterpret_cast<uint32_t *>(h);
		if (prim >= 0) {
			h[0] = t;
			h[1] = r.ox + r.dx * t; h[2] = r.oy + r.dy * t; h[3] = r.oz + r.dz * t;
			h[4] = nx; h[5] = ny; h[6] = nz; h[7] = u; h[8] = v;
			hu[9] = (uint32_t)prim; hu[10] = layers;
		} else { // Intersection::set_miss on a default-constructed record
			h[0] = FLT_MAX; h[1] = h[2] = h[3] = 0.0f; h[4] = h[5] = h[6] = 0.0f; h[7] = h[8] = 0.0f;
			hu[9] = 0xFFFFFFFFu; hu[10] = 0u;
		}
		return;
	}
	float4 *q = reinterpret_cast<float4 *>(p.hits) + idx * 2u;
	float4 a, b;
	a.x = t; a.y = __int_as_float(prim); a.z = u; a.w = v;
	b.x = nx; b.y = ny; b.z = nz; b.w = __uint_as_float(layers);
	if (STREAM) { stream_store4(q, a); stream_store4(q + 1, b); }
	else { q[0] = a; q[1] = b; }
}

// End of a ray in every kernel but the row kernels (finish_row_ray, packet_rows_kernel.h): look up what the record
// needs about the winning triangle (id, layers, the cold normal row) and store it.  Bool and token outputs need none of that.
__device__ __forceinline__ void finish_ray(const TraceParams &p, uint64_t ray_idx, const RayRegs &r,
		float best_t, float best_u, float best_v, uint32_t best_slot)
{
	int32_t prim = -1; float nx = 0.0f, ny = 0.0f, nz = 0.0f; uint32_t layers = 0u;
	if (best_slot != 0xFFFFFFFFu) {
		if (p.out_fmt == OUT_BOOL8 || p.out_fmt == OUT_TOKEN4) prim = 0; // only "hit or not" (and the slot) is stored
		else {
			prim = (int32_t)p.tri_hot[best_slot].id;
			layers = p.tri_hot[best_slot].layers;
			const float4 nn = reinterpret_cast<const float4 *>(p.tri_cold)[best_slot];
			nx = nn.x; ny = nn.y; nz = nn.z;
		}
	}
	store_hit(p, ray_idx, r, best_t, prim, best_u, best_v, nx, ny, nz, layers, best_slot);
}

// The same for a two-level scene (SceneTLAS::cast_ray, src/accel/scene_tlas.h:217-244): prim_id = the flat
// id (instance id base + mesh-local index, already in best_id), hit_layers = the instance's mask, normal =
// normalize(basis * mesh-space normal); DevInstance row = 8 float4: basis at words 12..20, mask at word 23.
__device__ __forceinline__ void finish_two_level_ray(const TraceParams &p, uint64_t ray_idx, const RayRegs &r,
		float best_t, float best_u, float best_v, uint32_t best_slot, uint32_t best_id, uint32_t best_inst)
{
	int32_t prim = -1; float nx = 0.0f, ny = 0.0f, nz = 0.0f; uint32_t layers = 0u;
	if (p.out_fmt == OUT_TOKEN8) { // {triangle slot, instance row}: expand_two_level_tokens_kernel rebuilds the record
		reinterpret_cast<uint2 *>(p.hits)[ray_idx] = make_uint2(best_slot, best_slot != 0xFFFFFFFFu ? best_inst : 0u);
		return;
	}
	if (best_slot != 0xFFFFFFFFu) {
		prim = (int32_t)best_id;
		if (p.out_fmt != OUT_BOOL8) {
			const float4 *row = reinterpret_cast<const float4 *>(p.instances) + (size_t)best_inst * 8u;
			const float4 b0 = row[3], b1 = row[4], b2 = row[5];
			const float4 no = reinterpret_cast<const float4 *>(p.tri_cold)[best_slot];
			nx = fma_(b0.x, no.x, fma_(b0.y, no.y, b0.z * no.z));
			ny = fma_(b0.w, no.x, fma_(b1.x, no.y, b1.y * no.z));
			nz = fma_(b1.z, no.x, fma_(b1.w, no.y, b2.x * no.z));
			const float l2 = fma_(nx, nx, fma_(ny, ny, nz * nz));
			if (l2 == 0.0f) { nx = ny = nz = 0.0f; }
			else { const float l = __builtin_sqrtf(l2); nx /= l; ny /= l; nz /= l; }
			layers = __float_as_uint(b2.w);
		}
	}
	store_hit(p, ray_idx, r, best_t, prim, best_u, best_v, nx, ny, nz, layers, best_slot);
}
