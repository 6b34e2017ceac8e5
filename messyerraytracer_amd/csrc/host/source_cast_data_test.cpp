// source_cast_data_test.cpp -- host/source_cast_data.cpp and source_cast.h without a device.  Per family (shadow, selected shadow,
// reflection, hemisphere, bounce), array and grid form: every refusal and their order (a call with everything wrong is mended one
// argument at a time, and the reason must move down the header's table), the edges of every range, and the kernels' argument: the
// jumps against stepping the generator, the seed of a row band against the whole frame's, the kinds of the lights, the batch.
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../source_cast.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

namespace {

using namespace mrt;
using namespace mrt::sc;

int n_checks = 0, n_fail = 0;

void expect(bool ok, const std::string &what)
{
	n_checks++;
	if (!ok) { n_fail++; if (n_fail <= 40) std::printf("FAIL %s\n", what.c_str()); }
}

bool has(const char *s, const char *word) { return s && std::string(s).find(word) != std::string::npos; }

void *const R = reinterpret_cast<void *>(16); // never dereferenced
void *const H = reinterpret_cast<void *>(4096);
uint8_t *const M = reinterpret_cast<uint8_t *>(8192);
uint8_t *const OL = reinterpret_cast<uint8_t *>(12288);
uint8_t *const SEL = reinterpret_cast<uint8_t *>(16384);

mrt_light light(uint32_t type, uint32_t cast, float px, float py, float pz, float dx, float dy, float dz)
{
	mrt_light L;
	std::memset(&L, 0, sizeof(L));
	L.type = type; L.cast_shadows = cast;
	L.position[0] = px; L.position[1] = py; L.position[2] = pz;
	L.direction[0] = dx; L.direction[1] = dy; L.direction[2] = dz;
	return L;
}

void selected_shadow_refusals()
{
	expect(sizeof(mrt_light_select) == 24, "mrt_light_select is 24 bytes");
	mrt_light lights[MRT_MAX_LIGHTS + 1];
	for (uint32_t l = 0; l <= MRT_MAX_LIGHTS; l++) lights[l] = light(l % 3u, 1u, 1.0f, 2.0f, 3.0f, 0.0f, 1.0f, 0.0f);
	for (int grid = 0; grid < 2; grid++) {
		const std::string c = grid ? "grid: " : "array: ";
		// everything wrong at once, mended in the header's order
		mrt_light_select d;
		std::memset(&d, 0, sizeof(d));
		d.frame = MRT_PATH_MAX_FRAME + 1u;
		const void *rays = nullptr, *hits = nullptr;
		const mrt_light_select *desc = nullptr;
		const uint8_t *mask = nullptr;
		const mrt_light *ls = nullptr;
		uint32_t n = MRT_MAX_LIGHTS + 1u, flags = MRT_FLAG_COHERENT;
		lights[2].type = 3u;
		auto why = [&] { return selected_shadow_invalid(!grid, rays, hits, desc, ls, n, mask, flags); };
		expect(has(why(), "null rays"), c + "rays first");
		rays = R;
		expect(has(why(), "null hits"), c + "hits");
		hits = H;
		expect(has(why(), "null descriptor"), c + "descriptor");
		desc = &d;
		expect(has(why(), "null mask"), c + "mask");
		mask = M;
		expect(has(why(), "null d_out_light"), c + "d_out_light");
		d.d_out_light = OL;
		expect(has(why(), "null lights"), c + "lights");
		ls = lights;
		expect(has(why(), "unknown flag"), c + "flags");
		flags = MRT_FLAG_ASYNC | MRT_FLAG_HOST_LAYOUT;
		expect(grid ? has(why(), "unknown flag") : has(why(), "MRT_MAX_LIGHTS"), c + "HOST_LAYOUT is the array form's flag alone");
		flags = MRT_FLAG_ASYNC;
		expect(has(why(), "MRT_MAX_LIGHTS"), c + "n_lights");
		n = MRT_MAX_LIGHTS;
		expect(has(why(), "unknown light type"), c + "light type");
		lights[2].type = MRT_LIGHT_SPOT;
		expect(has(why(), "MRT_PATH_MAX_FRAME"), c + "frame");
		d.frame = MRT_PATH_MAX_FRAME;
		expect(why() == nullptr, c + "a valid call");
		d.d_select = SEL;
		expect(why() == nullptr, c + "d_select is optional");
		// no lights: valid, and the list may be null
		n = 0u; ls = nullptr;
		expect(why() == nullptr, c + "n_lights == 0 with null lights");
		// a light past n_lights is not looked at
		lights[5].type = 9u; n = 5u; ls = lights;
		expect(why() == nullptr, c + "a light past n_lights is not read");
		n = 6u;
		expect(has(why(), "unknown light type"), c + "the sixth light's type");
		lights[5].type = MRT_LIGHT_SPOT;
	}
}

// PCG32 stepped draw by draw
uint32_t stepped_state(uint32_t seed, uint32_t draw)
{
	uint32_t s = (kPcgInc + seed) * kPcgMul + kPcgInc;
	for (uint32_t k = 0; k < draw; k++) s = s * kPcgMul + kPcgInc;
	return s;
}

void selected_shadow_params()
{
	expect(MRT_PATH_SELECT_DRAW(0u) == 256u && MRT_PATH_SELECT_DRAW(32u) == 288u, "MRT_PATH_SELECT_DRAW");
	expect(3u * MRT_PATH_MAX_BOUNCES + (MRT_PATH_MAX_BOUNCES - 2u) + 3u < MRT_PATH_SELECT_DRAW(0u), "the loop's own draws end below the first selecting draw");
	const mrt_light lights[5] = {
		light(MRT_LIGHT_DIRECTIONAL, 1u, 9.0f, 9.0f, 9.0f, 0.25f, 0.5f, -0.75f),
		light(MRT_LIGHT_POINT, 1u, 1.0f, 2.0f, 3.0f, 8.0f, 8.0f, 8.0f),
		light(MRT_LIGHT_SPOT, 1u, -1.0f, -2.0f, -3.0f, 0.0f, -1.0f, 0.0f),
		light(MRT_LIGHT_POINT, 0u, 4.0f, 5.0f, 6.0f, 0.0f, 0.0f, 0.0f),
		light(MRT_LIGHT_DIRECTIONAL, 0u, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f),
	};
	for (uint32_t draw : {0u, 1u, 2u, 129u, 256u, 257u, 288u, 1000u}) {
		for (uint32_t frame : {0u, 7u, (uint32_t)MRT_PATH_MAX_FRAME}) {
			// a row band [y0, ..) of a grid 100 wide, and the array form (pixel0 = 0)
			for (uint32_t pixel0 : {0u, 5u * 100u, 4000000u * 1080u}) {
				mrt_light_select d;
				std::memset(&d, 0, sizeof(d));
				d.frame = frame; d.select_draw = draw; d.d_select = SEL; d.d_out_light = OL;
				SelectShadowParams s;
				std::memset(&s, 0xAB, sizeof(s));
				fill_selected_shadow(H, &d, lights, 5u, pixel0, s);
				const std::string c = "draw " + std::to_string(draw) + " frame " + std::to_string(frame) + " pixel0 " + std::to_string(pixel0) + ": ";
				expect(s.records == H && s.select == SEL && s.out_light == OL && s.n_lights == 5u, c + "pointers and count");
				for (uint32_t i : {0u, 1u, 63u, 99u, 2399u}) {
					// the kernel's seed of record i of the band is the whole frame's seed of pixel pixel0 + i
					const uint32_t seed = (pixel0 + i) * 1009u + frame * 6529u + 7u;
					expect(i * 1009u + s.seed_add == seed, c + "seed of record " + std::to_string(i));
					const uint32_t state0 = (kPcgInc + seed) * kPcgMul + kPcgInc;
					expect(s.jump.a * state0 + s.jump.c == stepped_state(seed, draw), c + "the jump reaches the stepped state, record " + std::to_string(i));
				}
				expect(s.light[0].kind == SHADOW_DIRECTIONAL && s.light[0].v[0] == 0.25f && s.light[0].v[1] == 0.5f && s.light[0].v[2] == -0.75f, c + "directional: its direction");
				expect(s.light[1].kind == SHADOW_POINT && s.light[1].v[0] == 1.0f && s.light[1].v[1] == 2.0f && s.light[1].v[2] == 3.0f, c + "point: its position");
				expect(s.light[2].kind == SHADOW_POINT && s.light[2].v[0] == -1.0f && s.light[2].v[1] == -2.0f && s.light[2].v[2] == -3.0f, c + "spot: its position");
				expect(s.light[3].kind == SHADOW_OFF && s.light[4].kind == SHADOW_OFF, c + "cast_shadows == 0 is OFF for every type");
				expect(s.light[5].kind == 0u && s.light[15].v[2] == 0.0f, c + "the lights past n_lights are zero");
			}
		}
	}
	// pcg_jump composes: the jump to a + b is the jump to a followed by b steps
	const HemiJump j = pcg_jump(256u), j1 = pcg_jump(257u);
	expect(j1.a == kPcgMul * j.a && j1.c == kPcgMul * j.c + kPcgInc, "pcg_jump(257) is pcg_jump(256) and one step");
	expect(pcg_jump(0u).a == 1u && pcg_jump(0u).c == 0u, "pcg_jump(0) is the identity");
}

void *const OUT = reinterpret_cast<void *>(20480);
void *const ORAYS = reinterpret_cast<void *>(24576);
float *const SURF = reinterpret_cast<float *>(28672);
const float kNaN = std::nanf(""), kInf = INFINITY;

// The first two rows of every family's table but selected shadow's: the array form's rays, then the flags (HOST_LAYOUT is the array
// form's alone).  why() is the call with rays and flags by reference; on return both are valid.
template <class Why>
void rays_then_flags(const std::string &c, bool grid, const void *&rays, uint32_t &flags, const char *next, Why why)
{
	rays = nullptr; flags = MRT_FLAG_COHERENT;
	if (!grid) expect(has(why(), "null rays"), c + "rays first");
	else expect(has(why(), "unknown flag"), c + "the grid form takes no rays");
	rays = grid ? nullptr : R;
	expect(has(why(), "unknown flag"), c + "flags");
	flags = MRT_FLAG_ASYNC | MRT_FLAG_HOST_LAYOUT;
	expect(grid ? has(why(), "unknown flag") : has(why(), next), c + "HOST_LAYOUT is the array form's flag alone");
	flags = MRT_FLAG_ASYNC;
	expect(has(why(), next), c + "after the flags: " + next);
}

void shadow()
{
	mrt_light lights[MRT_MAX_LIGHTS + 1];
	for (uint32_t l = 0; l <= MRT_MAX_LIGHTS; l++) lights[l] = light(l % 3u, 1u, 1.0f, 2.0f, 3.0f, 0.0f, 1.0f, 0.0f);
	for (int grid = 0; grid < 2; grid++) {
		const std::string c = grid ? "shadow, grid: " : "shadow, array: ";
		const void *rays = nullptr, *hits = nullptr;
		const uint8_t *mask = nullptr;
		const mrt_light *ls = nullptr;
		uint64_t count = (1ull << 63) + 1ull;
		uint32_t n = MRT_MAX_LIGHTS + 1u, flags = 0u;
		lights[1].type = 3u;
		auto why = [&] { return shadow_invalid(!grid, rays, hits, count, ls, n, mask, flags); };
		rays_then_flags(c, grid != 0, rays, flags, "MRT_MAX_LIGHTS", why);
		n = 2u;
		expect(has(why(), "null hits / lights / mask"), c + "hits");
		hits = H;
		expect(has(why(), "null hits / lights / mask"), c + "mask");
		mask = M;
		expect(has(why(), "null hits / lights / mask"), c + "lights");
		ls = lights;
		expect(has(why(), "count * n_lights overflows"), c + "2^63 + 1 records of 2 lights");
		count = (1ull << 63) - 1ull;
		expect(has(why(), "unknown light type"), c + "2^63 - 1 records of 2 lights fit; light type");
		lights[1].type = MRT_LIGHT_POINT;
		expect(why() == nullptr, c + "a valid call");
		count = 1ull << 63;
		expect(has(why(), "overflows"), c + "2^63 records of 2 lights");
		// the light counts
		count = 1000u; n = 0u; ls = nullptr;
		expect(why() == nullptr, c + "n_lights == 0 with null lights");
		count = ~0ull;
		expect(why() == nullptr, c + "n_lights == 0: no product to overflow");
		ls = lights; n = MRT_MAX_LIGHTS;
		expect(has(why(), "overflows"), c + "2^64 - 1 records of 16 lights");
		count = ~0ull / MRT_MAX_LIGHTS;
		expect(why() == nullptr, c + "MRT_MAX_LIGHTS lights at the overflow edge");
		count++;
		expect(has(why(), "overflows"), c + "one record past the edge");
		n = MRT_MAX_LIGHTS + 1u; count = 1u;
		expect(has(why(), "MRT_MAX_LIGHTS"), c + "MRT_MAX_LIGHTS + 1 lights");
		// a light past n_lights is not looked at
		lights[5].type = 9u; n = 5u;
		expect(why() == nullptr, c + "a light past n_lights is not read");
		n = 6u;
		expect(has(why(), "unknown light type"), c + "the sixth light's type");
		lights[5].type = MRT_LIGHT_SPOT;
	}
	const mrt_light two[2] = {light(MRT_LIGHT_DIRECTIONAL, 1u, 9.0f, 9.0f, 9.0f, 0.25f, 0.5f, -0.75f), light(MRT_LIGHT_SPOT, 0u, 1.0f, 2.0f, 3.0f, 0.0f, 0.0f, 0.0f)};
	ShadowParams s;
	std::memset(&s, 0xAB, sizeof(s));
	fill_shadow(H, 77u, two, 2u, s);
	expect(s.records == H && s.pixels == 77u, "shadow: records and pixels");
	expect(s.light[0].kind == SHADOW_DIRECTIONAL && s.light[0].v[0] == 0.25f && s.light[0].v[2] == -0.75f && s.light[1].kind == SHADOW_OFF, "shadow: the lights' kinds");
	expect(s.light[2].kind == 0u && s.light[MRT_MAX_LIGHTS - 1].v[2] == 0.0f, "shadow: the lights past n_lights are zero");
}

// t_max / max_distance: `low` itself is refused, the next float is the first one accepted
template <class Set, class Why>
void range_edges(const std::string &c, float low, const char *reason, Set set, Why why)
{
	for (float bad : {kNaN, kInf, -kInf, 0.0f, -0.0f, -1.0f, low}) {
		set(bad);
		expect(has(why(), reason), c + reason + " at " + std::to_string(bad));
	}
	for (float good : {std::nextafterf(low, 1.0f), 1e-4f * 2.0f, 1.0f, 1e30f, FLT_MAX}) {
		set(good);
		expect(!has(why(), reason), c + "in range: " + std::to_string(good));
	}
}

void reflection()
{
	for (int grid = 0; grid < 2; grid++) {
		const std::string c = grid ? "reflection, grid: " : "reflection, array: ";
		const void *rays = nullptr, *hits = nullptr, *out = nullptr;
		float max_distance = kNaN;
		uint32_t flags = 0u;
		auto why = [&] { return reflection_invalid(!grid, rays, hits, max_distance, out, flags); };
		rays_then_flags(c, grid != 0, rays, flags, "null hits / output hits", why);
		hits = H;
		expect(has(why(), "null hits / output hits"), c + "output hits");
		out = OUT;
		expect(has(why(), "max_distance must be finite and > 0"), c + "max_distance");
		range_edges(c, 0.0f, "max_distance", [&](float v) { max_distance = v; }, why);
		max_distance = 1e-4f;
		expect(why() == nullptr, c + "1e-4 is a distance (> 0)");
		max_distance = 1e30f;
		expect(why() == nullptr, c + "a valid call");
	}
	ReflectParams s;
	std::memset(&s, 0xAB, sizeof(s));
	fill_reflection(H, SEL, 12.5f, ORAYS, s);
	expect(s.records == H && s.select == SEL && s.out_rays == ORAYS && s.max_distance == 12.5f, "reflection: the argument");
}

void hemisphere()
{
	for (int grid = 0; grid < 2; grid++) {
		const std::string c = grid ? "hemisphere, grid: " : "hemisphere, array: ";
		mrt_hemisphere d;
		std::memset(&d, 0, sizeof(d));
		d.n_samples = 0u; d.t_max = kNaN;
		const void *rays = nullptr, *hits = nullptr, *out = nullptr, *out_rays = ORAYS;
		const mrt_hemisphere *desc = nullptr;
		uint64_t count = ~0ull;
		int mode = 7;
		uint32_t flags = 0u;
		auto why = [&] { return hemisphere_invalid(!grid, rays, hits, count, desc, out, out_rays, mode, flags); };
		rays_then_flags(c, grid != 0, rays, flags, "null descriptor", why);
		desc = &d;
		expect(has(why(), "n_samples outside"), c + "n_samples == 0");
		d.n_samples = MRT_MAX_HEMISPHERE_SAMPLES + 1u;
		expect(MRT_MAX_HEMISPHERE_SAMPLES == 16u && has(why(), "n_samples outside"), c + "n_samples == 17");
		d.n_samples = MRT_MAX_HEMISPHERE_SAMPLES;
		expect(has(why(), "t_max must be finite and > 1e-4"), c + "t_max");
		range_edges(c, 1e-4f, "t_max", [&](float v) { d.t_max = v; }, why);
		expect(has(why(), "unknown mode"), c + "mode");
		mode = MRT_MODE_ANY_HIT;
		expect(has(why(), "any-hit writes no rays"), c + "out-rays with any-hit");
		mode = MRT_MODE_NEAREST;
		expect(has(why(), "null hits / output"), c + "closest-hit may write rays; hits");
		mode = MRT_MODE_ANY_HIT; out_rays = nullptr; hits = H;
		expect(has(why(), "null hits / output"), c + "output");
		out = OUT;
		expect(has(why(), "count * n_samples overflows"), c + "2^64 - 1 records of 16 samples");
		count = ~0ull / 16u;
		expect(why() == nullptr, c + "16 samples at the overflow edge");
		count++;
		expect(has(why(), "overflows"), c + "one record past the edge");
		d.n_samples = 1u; count = ~0ull;
		expect(why() == nullptr, c + "one sample: any count");
		mode = MRT_MODE_NEAREST; out_rays = ORAYS; d.d_select = SEL;
		expect(why() == nullptr, c + "closest-hit with out-rays and a selection");
	}
	mrt_hemisphere d;
	std::memset(&d, 0, sizeof(d));
	d.n_samples = 4u; d.frame = 9u; d.first_draw = 1u; d.t_max = 2.5f; d.d_select = SEL;
	HemiParams s;
	std::memset(&s, 0xAB, sizeof(s));
	fill_hemisphere(H, 300u, 500u, &d, ORAYS, s);
	expect(s.records == H && s.select == SEL && s.out_rays == ORAYS && s.pixels == 300u && s.t_max == 2.5f, "hemisphere: the argument");
	expect(s.seed_add == seed_add(500u, 9u), "hemisphere: seed_add");
	HemiJump want[MRT_MAX_HEMISPHERE_SAMPLES];
	hemisphere_jumps(1u, 4u, want);
	expect(std::memcmp(s.jump, want, 4u * sizeof(HemiJump)) == 0 && s.jump[4].a == 0u && s.jump[15].c == 0u, "hemisphere: the jumps of its samples, zero past them");
}

void bounce()
{
	for (int grid = 0; grid < 2; grid++) {
		const std::string c = grid ? "bounce, grid: " : "bounce, array: ";
		mrt_bounce d;
		std::memset(&d, 0, sizeof(d));
		d.t_max = kNaN; d.metallic = kNaN; d.roughness = kNaN;
		const void *rays = nullptr, *hits = nullptr, *out = nullptr;
		const mrt_bounce *desc = nullptr;
		uint32_t flags = 0u;
		auto why = [&] { return bounce_invalid(!grid, rays, hits, desc, out, flags); };
		rays_then_flags(c, grid != 0, rays, flags, "null descriptor", why);
		desc = &d;
		expect(has(why(), "t_max must be finite and > 1e-4"), c + "t_max");
		range_edges(c, 1e-4f, "t_max", [&](float v) { d.t_max = v; }, why);
		expect(has(why(), "metallic must be in [0, 1]"), c + "metallic before roughness");
		for (int with_surface = 0; with_surface < 2; with_surface++) {
			d.d_surface = with_surface ? SURF : nullptr;
			const std::string cs = c + (with_surface ? "with d_surface, " : "without d_surface, ");
			for (int which = 0; which < 2; which++) {
				float &v = which ? d.roughness : d.metallic;
				const char *reason = which ? "roughness must be in [0, 1]" : "metallic must be in [0, 1]";
				d.metallic = d.roughness = 0.5f;
				for (float bad : {kNaN, -1e-30f, std::nextafterf(1.0f, 2.0f), kInf, -kInf}) {
					v = bad;
					expect(with_surface ? !has(why(), "must be in [0, 1]") : has(why(), reason), cs + reason + " at " + std::to_string(bad));
				}
				for (float good : {-0.0f, 0.0f, 0.5f, 1.0f}) {
					v = good;
					expect(!has(why(), "must be in [0, 1]"), cs + (which ? "roughness " : "metallic ") + std::to_string(good));
				}
			}
		}
		d.d_surface = nullptr; d.metallic = 1.0f; d.roughness = -0.0f;
		expect(has(why(), "null hits / output"), c + "hits");
		hits = H;
		expect(has(why(), "null hits / output"), c + "output");
		out = OUT;
		expect(why() == nullptr, c + "a valid call");
	}
	mrt_bounce d;
	std::memset(&d, 0, sizeof(d));
	d.frame = 3u; d.first_draw = 5u; d.t_max = 1e30f; d.metallic = 0.25f; d.roughness = 0.75f; d.d_select = SEL; d.d_surface = SURF; d.d_out_lobe = OL;
	BounceParams s;
	std::memset(&s, 0xAB, sizeof(s));
	fill_bounce(H, 640u, &d, ORAYS, s);
	expect(s.records == H && s.select == SEL && s.surface == SURF && s.out_rays == ORAYS && s.out_lobe == OL, "bounce: the pointers");
	expect(s.t_max == 1e30f && s.metallic == 0.25f && s.roughness == 0.75f && s.seed_add == seed_add(640u, 3u), "bounce: the numbers");
	expect(s.jump.a == pcg_jump(5u).a && s.jump.c == pcg_jump(5u).c, "bounce: the jump to first_draw");
}

// The state after k draws, a draw at a time: in blocks of 2^16 draws, the block's map (state -> A state + C) itself made by composing
// 2^16 single steps (2^32 single steps per case would take seconds).  k up to 2^32 + 30: the generator's period is 2^32.
uint32_t stepped_far(uint32_t state, uint64_t k)
{
	static uint32_t A = 0u, C = 0u;
	if (A == 0u) {
		A = 1u;
		for (uint32_t i = 0; i < 65536u; i++) { A = kPcgMul * A; C = kPcgMul * C + kPcgInc; }
	}
	for (uint64_t b = k >> 16; b != 0u; b--) state = A * state + C;
	for (uint32_t i = 0; i < (uint32_t)(k & 0xFFFFu); i++) state = state * kPcgMul + kPcgInc;
	return state;
}

void jumps()
{
	// the block walk against plain stepping where that is cheap
	expect(stepped_far(12345u, 200000u) == [] { uint32_t s = 12345u; for (uint32_t i = 0; i < 200000u; i++) s = s * kPcgMul + kPcgInc; return s; }(), "stepped_far is stepping");
	for (uint32_t first_draw : {0u, 1u, 0x80000000u, 0xFFFFFFFFu}) for (uint32_t n : {1u, (uint32_t)MRT_MAX_HEMISPHERE_SAMPLES}) {
		HemiJump j[MRT_MAX_HEMISPHERE_SAMPLES];
		std::memset(j, 0xAB, sizeof(j));
		hemisphere_jumps(first_draw, n, j);
		for (uint32_t s = 0; s < n; s++) {
			const std::string c = "first_draw " + std::to_string(first_draw) + ", " + std::to_string(n) + " samples, sample " + std::to_string(s) + ": ";
			for (uint32_t state0 : {0u, 0x9E3779B9u, 0xFFFFFFFFu})
				expect(j[s].a * state0 + j[s].c == stepped_far(state0, (uint64_t)first_draw + 2u * s), c + "the jump reaches the stepped state from " + std::to_string(state0));
			const HemiJump p = pcg_jump(first_draw + 2u * s); // (modulo 2^32, the period)
			expect(p.a == j[s].a && p.c == j[s].c, c + "pcg_jump agrees");
		}
		if (n < MRT_MAX_HEMISPHERE_SAMPLES) expect(j[n].a == 0xABABABABu, "first_draw " + std::to_string(first_draw) + ": nothing written past n_samples");
	}
}

void seeds()
{
	// a row band [y0, ..) of a grid grid_w wide draws what the whole frame draws for the same pixel; 5 000 000 * 1009 wraps 2^32
	for (uint32_t frame : {0u, 7u, (uint32_t)MRT_PATH_MAX_FRAME, 0xFFFFFFFFu}) for (uint32_t grid_w : {1u, 100u, 1920u, 5000000u}) for (uint32_t y0 : {0u, 1u, 5u, 1079u}) {
		const uint32_t pixel0 = y0 * grid_w;
		const std::string c = "frame " + std::to_string(frame) + " grid_w " + std::to_string(grid_w) + " y0 " + std::to_string(y0) + ": ";
		for (uint32_t i : {0u, 1u, 63u, 2399u}) {
			const uint32_t whole = (pixel0 + i) * 1009u + frame * 6529u + 7u; // the kernels' rule for pixel pixel0 + i of the whole frame
			expect(i * 1009u + seed_add(pixel0, frame) == whole, c + "seed of record " + std::to_string(i));
		}
	}
	expect((uint64_t)5000000u * 1009u > 0xFFFFFFFFull && seed_add(5000000u, 0u) == (uint32_t)(5000000ull * 1009ull + 7ull), "the product wraps 2^32");
	expect(seed_add(0u, 0u) == 7u, "the array form's seed_add of frame 0");
}

void batches()
{
	struct F { const char *name; int ray32, host, grid; bool any, nearest; };
	const F fam[] = {
		{"shadow", SRC_SHADOW_RAY32, SRC_SHADOW_HOST44, SRC_SHADOW_GRID, true, false},
		{"selected shadow", SRC_SELSHADOW_RAY32, SRC_SELSHADOW_HOST44, SRC_SELSHADOW_GRID, true, false},
		{"reflection", SRC_REFLECT_RAY32, SRC_REFLECT_HOST, SRC_REFLECT_GRID, false, true},
		{"hemisphere", SRC_HEMI_RAY32, SRC_HEMI_HOST, SRC_HEMI_GRID, true, true},
		{"bounce", SRC_BOUNCE_RAY32, SRC_BOUNCE_HOST, SRC_BOUNCE_GRID, false, true},
		{"gbuffer", SRC_GBUFFER, SRC_GBUFFER, SRC_GBUFFER, false, true},
	};
	for (const F &f : fam) {
		const std::string c = std::string(f.name) + ": ";
		// any-hit: one byte per entry for the families that answer lit / shadowed; closest-hit: a record in the input's layout
		if (f.any) for (int src : {f.ray32, f.host, f.grid}) expect(out_fmt(src, MRT_MODE_ANY_HIT) == OUT_BOOL8, c + "any-hit writes bytes, source " + std::to_string(src));
		if (f.nearest) {
			expect(out_fmt(f.ray32, MRT_MODE_NEAREST) == OUT_HIT32 && out_fmt(f.grid, MRT_MODE_NEAREST) == OUT_HIT32, c + "packed records");
			expect(out_fmt(f.host, MRT_MODE_NEAREST) == (f.host == f.ray32 ? OUT_HIT32 : OUT_HOST44), c + "host-layout records for the host source");
		} else for (int src : {f.ray32, f.host, f.grid}) expect(out_fmt(src, MRT_MODE_NEAREST) == OUT_BOOL8, c + "a shadow family has no other output, source " + std::to_string(src));
	}
	for (int src : {SRC_SHADOW_RAY32, SRC_SHADOW_HOST44, SRC_SHADOW_GRID}) {
		const Batch b = shadow_batch(src, 1000u, 3u);
		expect(b.count == 3000u && b.out_fmt == OUT_BOOL8 && b.mode == MRT_MODE_ANY_HIT, "shadow batch: records * lights, source " + std::to_string(src));
		expect(shadow_batch(src, 1000u, 0u).count == 0u && shadow_batch(src, 0u, 16u).count == 0u, "shadow batch: empty without lights or records");
	}
	for (int src : {SRC_SELSHADOW_RAY32, SRC_SELSHADOW_HOST44, SRC_SELSHADOW_GRID}) {
		const Batch b = selected_shadow_batch(src, 1000u);
		expect(b.count == 1000u && b.out_fmt == OUT_BOOL8 && b.mode == MRT_MODE_ANY_HIT, "selected-shadow batch: one entry per record, source " + std::to_string(src));
	}
	for (int src : {SRC_HEMI_RAY32, SRC_HEMI_HOST, SRC_HEMI_GRID}) for (int mode : {MRT_MODE_ANY_HIT, MRT_MODE_NEAREST}) {
		const Batch b = hemisphere_batch(src, 1000u, 16u, mode);
		expect(b.count == 16000u && b.mode == mode && b.out_fmt == out_fmt(src, mode), "hemisphere batch: records * samples, source " + std::to_string(src));
		expect(hemisphere_batch(src, ~0ull / 16u, 16u, mode).count == (~0ull / 16u) * 16u, "hemisphere batch: the overflow edge");
	}
	for (int src : {SRC_REFLECT_RAY32, SRC_REFLECT_HOST, SRC_REFLECT_GRID}) {
		const Batch b = reflection_batch(src, 77u);
		expect(b.count == 77u && b.mode == MRT_MODE_NEAREST && b.out_fmt == out_fmt(src, MRT_MODE_NEAREST), "reflection batch, source " + std::to_string(src));
	}
	for (int src : {SRC_BOUNCE_RAY32, SRC_BOUNCE_HOST, SRC_BOUNCE_GRID}) {
		const Batch b = bounce_batch(src, 77u);
		expect(b.count == 77u && b.mode == MRT_MODE_NEAREST && b.out_fmt == out_fmt(src, MRT_MODE_NEAREST), "bounce batch, source " + std::to_string(src));
	}
	expect(unknown_flag(false, MRT_FLAG_HOST_LAYOUT) && !unknown_flag(true, MRT_FLAG_HOST_LAYOUT | MRT_FLAG_ASYNC) && !unknown_flag(false, MRT_FLAG_ASYNC) && !unknown_flag(false, 0u)
			&& unknown_flag(true, MRT_FLAG_COHERENT), "unknown_flag");
}

} // namespace

int main()
{
	selected_shadow_refusals();
	selected_shadow_params();
	shadow();
	reflection();
	hemisphere();
	bounce();
	jumps();
	seeds();
	batches();
	std::printf("%d checks hold out of %d\n", n_checks - n_fail, n_checks);
	return n_fail ? 1 : 0;
}
