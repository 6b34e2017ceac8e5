// emitter_light_kernel.h — the diffuse term of the emitter point every record sampled (mrt_light_emitter_surfaces /
// mrt_light_grid_emitter_surfaces).  Included by shade_kernels.hip (inside namespace mrt, after emitter_sample_kernel.h and
// light_kernel.h; emitters.h holds EmitterLightParams).
//
// One thread per record, nothing walked: the record and its ray as record_surface reads them, the cast's word, the emitter's row as four
// 16-byte loads, {albedo, metallic} of the record's row as one, the mask byte, then (accumulate) one 16-byte load and one 16-byte
// store.  The point is emitter_sample_kernel.h's, the text the cast made its ray from; the term is in the order include/mrt_hip.h
// states (nothing is contracted).  No LDS, no scratch.
#pragma once

template <int SRC>
__global__ __launch_bounds__(MRT_WG) void light_emitter_surfaces_kernel(const TraceParams p, const EmitterLightParams s)
{
	constexpr bool HOST = SRC == SURF_HOST, GRID = SRC == SURF_GRID;
	const uint64_t i = (uint64_t)blockIdx.x * MRT_WG + threadIdx.x;
	if (i >= p.count) return;
	Surface sf = {};
	float4 *out = reinterpret_cast<float4 *>(s.out) + i;
	if (!record_surface<HOST, GRID>(p, s.records, i, sf)) {
		if (s.accumulate == 0u) *out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		return;
	}
	float tr = 0.0f, tg = 0.0f, tb = 0.0f;
	const uint32_t k = s.emitter[i];
	if (k < s.table.n && !(s.mask != nullptr && s.mask[i] == 0)) {
		face_normal(sf);
		EmitterPoint e;
		float ox, oy, oz;
		if (emitter_point(s.table, k, emitter_stream(i, s.seed_add, s.jump), sf, ox, oy, oz, e)) {
			const float4 am = (reinterpret_cast<const float4 *>(s.rows) + i * 4u)[1]; // {albedo, metallic}
			const float one_m = 1.0f - am.w;
			const float geom = (e.ndl * e.cy) / e.dist2;
			const float wgt = e.area * (2147483648.0f / (float)e.q);
			const float gw = geom * wgt;
			tr = (((am.x * one_m) * 0.31830988618f) * e.ler) * gw;
			tg = (((am.y * one_m) * 0.31830988618f) * e.leg) * gw;
			tb = (((am.z * one_m) * 0.31830988618f) * e.leb) * gw;
		}
	}
	float4 o = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
	if (s.accumulate != 0u) o = *out;
	o.x = o.x + tr; o.y = o.y + tg; o.z = o.z + tb;
	*out = o;
}
