// selected_shadow_kernel.h — one shadow ray per record, to the light the record draws (mrt_cast_selected_shadows /
// mrt_cast_grid_selected_shadows).  Included by kernels.hip (inside namespace mrt, after shadow_kernel.h, before the kernels that use it).
//
// The light sampling of the reference's GPU path tracer (src/gpu/shaders/pt_shade.comp.glsl step 6: pcg32_next(rng) % light_count, one
// shadow ray, the weight float(light_count)).  A source family of source_common.h (SRC_SELSHADOW_*, any-hit only); entry i is record i
// and its results are the light byte and one byte of the lit mask.
//   not selected (a primary miss, or select[i] == 0): light byte MRT_LIGHT_NONE, lit, nothing walks
//   state0 as hemisphere_kernel.h; state = A * state0 + C, (A, C) of draw select_draw: SelectShadowParams::jump
//   k = pcg_word(state) % n_lights in uint32; light byte k
//   the ray of shadow_kernel.h for the pair (i, light k): shadow_ray_to, the one text of it.  No ray (cast_shadows == 0, a point light
//   on the origin): lit, nothing walks.
// The light is indexed per lane, as ShadowParams::light is by a pair's light: the table stays in the kernel argument and a lane reads its
// four words from there (no copy, no scratch).
#pragma once

// The ray of entry i, or (false) the lit byte of an entry without one, stored; the light byte either way.
template <int SRC, bool ANY_HIT>
__device__ __forceinline__ bool source_entry(const TraceParams &p, const SelectShadowParams &s, uint64_t i, RayRegs &r)
{
	static_assert(selected_shadow_source(SRC) && ANY_HIT, "selected-shadow sources are any-hit");
	constexpr bool HOST = SRC == SRC_SELSHADOW_HOST44, GRID = SRC == SRC_SELSHADOW_GRID;
	bool selected = s.select == nullptr || s.select[i] != 0;
	if (selected) selected = record_is_hit<HOST>(s.records, i); // (a miss selects no light)
	if (!selected) {
		s.out_light[i] = (uint8_t)MRT_LIGHT_NONE;
		store_lit(p, i, true);
		return false;
	}
	uint32_t state = (kPcgInc + ((uint32_t)i * 1009u + s.seed_add)) * kPcgMul + kPcgInc;
	state = s.jump.a * state + s.jump.c;
	const uint32_t k = pcg_word(state) % s.n_lights;
	s.out_light[i] = (uint8_t)k;
	const ShadowLight L = s.light[k];
	if (shadow_ray_to<HOST, GRID>(p, s.records, i, L, r)) return true;
	store_lit(p, i, true);
	return false;
}
