// selected_shadow_data_test.cpp -- host/selected_shadow_data.cpp and selected_shadow.h without a device: every refusal of
// mrt_cast_selected_shadows / mrt_cast_grid_selected_shadows and their order (a call with everything wrong is mended one argument at a
// time, and the reason must move down the header's list), and the kernel's argument: the jump to the selecting draw against stepping
// the generator, the seed of a row band against the whole frame's, the kinds of the lights.
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../selected_shadow.h"

#include <cstdio>
#include <cstring>
#include <string>

namespace {

using namespace mrt;
using namespace mrt::sel;

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

void refusals()
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
		auto why = [&] { return cast_invalid(!grid, rays, hits, desc, ls, n, mask, flags); };
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

void params()
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
				fill_params(H, &d, lights, 5u, pixel0, s);
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

} // namespace

int main()
{
	refusals();
	params();
	std::printf("%d checks hold out of %d\n", n_checks - n_fail, n_checks);
	return n_fail ? 1 : 0;
}
