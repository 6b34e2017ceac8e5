// emitter_shadow_kernel.h — one shadow ray per record, to a point of the emissive triangle the record samples
// (mrt_cast_emitter_shadows / mrt_cast_grid_emitter_shadows).  Included by kernels.hip (inside namespace mrt, after
// emitter_sample_kernel.h, before the kernels that use it).
//
// A source family of source_common.h (SRC_EMITSHADOW_*, any-hit only); entry i is record i and its results are the emitter word and one
// byte of the lit mask.
//   not selected (a miss, select[i] == 0, an empty table, or a word past the table's total): word MRT_EMITTER_NONE, lit, nothing walks
//   the stream, the choice and the point: emitter_sample_kernel.h, the one text of them (the light call derives the same point)
//   refused (the point on the origin, below the surface, or the emitter seen edge-on): the word k, lit, nothing walks
//   otherwise the ray {org, dir, 0, dist * 0.999f}: the emitter does not shadow itself
#pragma once

// The ray of entry i, or (false) the lit byte of an entry without one, stored; the emitter word either way.
template <int SRC, bool ANY_HIT>
__device__ __forceinline__ bool source_entry(const TraceParams &p, const EmitterShadowParams &s, uint64_t i, RayRegs &r)
{
	static_assert(emitter_shadow_source(SRC) && ANY_HIT, "emitter-shadow sources are any-hit");
	constexpr bool HOST = SRC == SRC_EMITSHADOW_HOST44, GRID = SRC == SRC_EMITSHADOW_GRID;
	bool selected = s.table.n != 0u && (s.select == nullptr || s.select[i] != 0);
	Surface sf = {};
	if (selected) selected = record_surface<HOST, GRID>(p, s.records, i, sf); // (a miss samples no emitter)
	uint32_t k = MRT_EMITTER_NONE, state = 0u;
	if (selected) {
		state = emitter_stream(i, s.seed_add, s.jump);
		k = emitter_select(s.table, pcg_word(state));
	}
	s.out_emitter[i] = k;
	if (k != MRT_EMITTER_NONE) {
		face_normal(sf);
		EmitterPoint e;
		if (emitter_point(s.table, k, state, sf, r.ox, r.oy, r.oz, e)) {
			r.dx = e.dx; r.dy = e.dy; r.dz = e.dz;
			r.t_min = 0.0f; r.t_max = e.dist * 0.999f;
			return true;
		}
	}
	store_lit(p, i, true);
	return false;
}
