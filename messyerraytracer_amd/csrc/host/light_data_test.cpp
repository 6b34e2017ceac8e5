// light_data_test.cpp -- host/light_data.cpp and lighting.h's pow01 without a device: the refusals of a light list and an environment
// (every one include/mrt_hip.h lists, every float not finite in turn) and what passes; the kernel's copy of a list (cos_outer is cosf of
// the angle, 1 - cos_outer beside it); mrt_shadow_lights' copy with nothing written past it; pow01's selects, pow01(b, 1) == b over every
// b = j * 2^-16 and the smallest floats, and pow01 against the C library's pow in double, rounded once, within one float ulp.
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../lighting.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace {

int n_checks = 0, n_fail = 0;

void expect(bool ok, const std::string &what)
{
	n_checks++;
	if (!ok) { n_fail++; std::printf("FAIL %s\n", what.c_str()); }
}

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

mrt_shade_light light(uint32_t type)
{
	mrt_shade_light L;
	std::memset(&L, 0, sizeof(L));
	L.type = type; L.cast_shadows = 1u;
	L.position[0] = 1.0f; L.position[1] = 2.0f; L.position[2] = 3.0f;
	L.direction[0] = 0.0f; L.direction[1] = -1.0f; L.direction[2] = 0.0f;
	L.color[0] = 1.0f; L.color[1] = 0.5f; L.color[2] = 0.25f;
	L.range = 10.0f; L.attenuation = 1.0f; L.spot_angle = 0.785398f; L.spot_angle_attenuation = 1.0f;
	return L;
}

mrt_environment environment()
{
	mrt_environment e;
	std::memset(&e, 0, sizeof(e));
	const float v[13] = { 0.15f, 0.25f, 0.55f, 0.6f, 0.7f, 0.85f, 0.15f, 0.12f, 0.1f, 1.0f, 1.0f, 1.0f, 0.15f };
	std::memcpy(&e, v, sizeof(v));
	return e;
}

void refusals()
{
	std::vector<mrt_shade_light> ls = { light(MRT_LIGHT_DIRECTIONAL), light(MRT_LIGHT_POINT), light(MRT_LIGHT_SPOT) };
	const mrt_environment env = environment();
	expect(mrt::light_list_invalid(ls.data(), 3, &env, 100) == nullptr, "a good list refused");
	expect(mrt::light_list_invalid(ls.data(), 3, nullptr, 100) == nullptr, "a good list without an environment refused");
	expect(mrt::light_list_invalid(nullptr, 0, nullptr, 100) == nullptr, "no lights refused");
	expect(mrt::light_list_invalid(nullptr, 0, &env, 100) == nullptr, "no lights with an environment refused");
	expect(mrt::light_list_invalid(nullptr, 1, nullptr, 100) != nullptr, "null lights with n_lights 1 accepted");
	std::vector<mrt_shade_light> many(MRT_MAX_LIGHTS + 1, light(MRT_LIGHT_DIRECTIONAL));
	expect(mrt::light_list_invalid(many.data(), MRT_MAX_LIGHTS, nullptr, 100) == nullptr, "MRT_MAX_LIGHTS lights refused");
	expect(mrt::light_list_invalid(many.data(), MRT_MAX_LIGHTS + 1, nullptr, 100) != nullptr, "MRT_MAX_LIGHTS + 1 lights accepted");
	std::vector<mrt_shade_light> b = ls;
	b[2].type = 3u;
	expect(mrt::light_list_invalid(b.data(), 3, nullptr, 100) != nullptr, "unknown light type accepted");
	b = ls; b[1].reserved = 1u;
	expect(mrt::light_list_invalid(b.data(), 3, nullptr, 100) != nullptr, "non-zero reserved word accepted");
	const float bad[3] = { std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity() };
	for (int w = 2; w < 15; w++) // words 2 .. 14 of a light are its floats
		for (float x : bad) {
			b = ls; reinterpret_cast<float *>(&b[2])[w] = x;
			expect(mrt::light_list_invalid(b.data(), 3, nullptr, 100) != nullptr, "light word " + std::to_string(w) + " not finite, accepted");
		}
	for (int w = 0; w < 13; w++)
		for (float x : bad) {
			mrt_environment e = env; reinterpret_cast<float *>(&e)[w] = x;
			expect(mrt::light_list_invalid(ls.data(), 3, &e, 100) != nullptr, "environment word " + std::to_string(w) + " not finite, accepted");
			expect(mrt::light_list_invalid(nullptr, 0, &e, 100) != nullptr, "environment word " + std::to_string(w) + " not finite without lights, accepted");
		}
	mrt_environment e = env; e.reserved[0] = 0x7FC00000u; e.reserved[2] = 0x7F800000u;
	expect(mrt::light_list_invalid(ls.data(), 3, &e, 100) == nullptr, "the environment's reserved words looked at");
	for (float r : { 0.0f, -0.0f, -1.0f }) {
		b = ls; b[1].range = r;
		expect(mrt::light_list_invalid(b.data(), 3, nullptr, 100) != nullptr, "point light range " + std::to_string(r) + " accepted");
		b = ls; b[2].range = r;
		expect(mrt::light_list_invalid(b.data(), 3, nullptr, 100) != nullptr, "spot light range " + std::to_string(r) + " accepted");
		b = ls; b[0].range = r;
		expect(mrt::light_list_invalid(b.data(), 3, nullptr, 100) == nullptr, "directional light range " + std::to_string(r) + " refused");
	}
	b = ls; b[1].range = std::numeric_limits<float>::denorm_min();
	expect(mrt::light_list_invalid(b.data(), 3, nullptr, 100) == nullptr, "smallest positive range refused");
	b = ls; b[1].attenuation = -0.5f;
	expect(mrt::light_list_invalid(b.data(), 3, nullptr, 100) != nullptr, "negative attenuation accepted");
	b = ls; b[2].spot_angle_attenuation = -1e-30f;
	expect(mrt::light_list_invalid(b.data(), 3, nullptr, 100) != nullptr, "negative spot_angle_attenuation accepted");
	b = ls; b[1].attenuation = 0.0f; b[2].spot_angle_attenuation = -0.0f; b[2].spot_angle = -4.0f; b[0].color[0] = -2.0f;
	expect(mrt::light_list_invalid(b.data(), 3, nullptr, 100) == nullptr, "finite but odd values refused");
	expect(mrt::light_list_invalid(ls.data(), 3, nullptr, UINT64_MAX / 3u) == nullptr, "largest count refused");
	expect(mrt::light_list_invalid(ls.data(), 3, nullptr, UINT64_MAX / 3u + 1u) != nullptr, "count * n_lights overflowing accepted");
	expect(mrt::light_list_invalid(nullptr, 0, nullptr, UINT64_MAX) == nullptr, "any count without lights refused");
	// order: too many lights before an unknown type, an unknown type before the environment
	many[0].type = 9u;
	expect(std::string(mrt::light_list_invalid(many.data(), MRT_MAX_LIGHTS + 1, nullptr, 1)).find("MRT_MAX_LIGHTS") != std::string::npos, "order: count of lights first");
	e = env; e.ambient_energy = bad[0];
	expect(std::string(mrt::light_list_invalid(many.data(), 1, &e, 1)).find("type") != std::string::npos, "order: lights before the environment");
}

void copies()
{
	std::vector<mrt_shade_light> ls = { light(MRT_LIGHT_DIRECTIONAL), light(MRT_LIGHT_POINT), light(MRT_LIGHT_SPOT) };
	ls[1].cast_shadows = 0u; ls[2].spot_angle = 0.3f; ls[2].position[1] = -7.0f;
	std::vector<mrt_light> out(4);
	std::memset(out.data(), 0xAB, out.size() * sizeof(mrt_light));
	mrt::shadow_lights(ls.data(), 3, out.data());
	for (int l = 0; l < 3; l++)
		expect(std::memcmp(&out[l], &ls[l], 32) == 0, "shadow light " + std::to_string(l));
	bool guard = true;
	for (size_t k = 0; k < sizeof(mrt_light); k++) guard = guard && reinterpret_cast<const unsigned char *>(&out[3])[k] == 0xAB;
	expect(guard, "mrt_shadow_lights wrote past its output");
	mrt::LightParams lp;
	std::memset(&lp, 0, sizeof(lp));
	const mrt_environment env = environment();
	mrt::fill_light_params(ls.data(), 3, &env, lp);
	expect(lp.n_lights == 3u && lp.has_env == 1u, "counts of the kernel's copy");
	expect(lp.zenith[2] == 0.55f && lp.horizon[0] == 0.6f && lp.ground[1] == 0.12f && lp.ambient[2] == 1.0f && lp.ambient_energy == 0.15f, "the kernel's environment");
	for (int l = 0; l < 3; l++) {
		const mrt::KernelLight &K = lp.light[l];
		bool ok = K.type == ls[l].type && K.range == ls[l].range && K.attenuation == ls[l].attenuation && K.spot_attenuation == ls[l].spot_angle_attenuation;
		for (int k = 0; k < 3; k++) ok = ok && K.position[k] == ls[l].position[k] && K.direction[k] == ls[l].direction[k] && K.color[k] == ls[l].color[k];
		ok = ok && bits(K.cos_outer) == bits(cosf(ls[l].spot_angle)) && bits(K.one_minus_cos_outer) == bits(1.0f - cosf(ls[l].spot_angle));
		expect(ok, "the kernel's light " + std::to_string(l));
	}
	mrt::fill_light_params(nullptr, 0, nullptr, lp);
	expect(lp.n_lights == 0u && lp.has_env == 0u, "an empty list");
}

int ulps(float a, float b) { return std::abs((int)(bits(a) - bits(b))); }

void powers()
{
	expect(mrt::pow01(0.0f, 0.0f) == 1.0f && mrt::pow01(0.3f, 0.0f) == 1.0f && mrt::pow01(0.3f, -0.0f) == 1.0f, "e == 0 -> 1");
	expect(mrt::pow01(0.0f, 2.0f) == 0.0f && mrt::pow01(1.0f, 3.7f) == 1.0f, "b == 0 -> 0, b == 1 -> 1");
	expect(mrt::pow01(0.25f, 0.5f) == 0.5f && mrt::pow01(0.5f, 2.0f) == 0.25f && mrt::pow01(0.5f, 149.0f) == std::numeric_limits<float>::denorm_min(), "exact powers of two");
	expect(mrt::pow01(0.5f, 151.0f) == 0.0f && mrt::pow01(1e-30f, 16.0f) == 0.0f, "underflow to 0");
	bool same = true;
	for (uint32_t j = 0; j <= 65536u; j++) { const float b = (float)j * (1.0f / 65536.0f); same = same && bits(mrt::pow01(b, 1.0f)) == bits(b); }
	for (uint32_t u = 1; u < 0x01000000u; u += 4099u) { float b; std::memcpy(&b, &u, 4); same = same && bits(mrt::pow01(b, 1.0f)) == bits(b); } // denormals and up
	for (uint32_t u = 0x3F800000u - 70000u; u < 0x3F800000u; u++) { float b; std::memcpy(&b, &u, 4); same = same && bits(mrt::pow01(b, 1.0f)) == bits(b); }
	expect(same, "pow01(b, 1) == b");
	int worst = 0; uint64_t differ = 0, total = 0;
	for (float e : { 0.25f, 0.5f, 1.0f, 2.0f, 3.7f, 8.0f, 16.0f })
		for (uint32_t j = 1; j < 65536u; j++) {
			const float b = (float)j * (1.0f / 65536.0f);
			const int d = ulps(mrt::pow01(b, e), (float)std::pow((double)b, (double)e));
			worst = d > worst ? d : worst; differ += d != 0; total++;
		}
	std::printf("pow01 against pow in double: %llu of %llu differ, worst %d ulp\n", (unsigned long long)differ, (unsigned long long)total, worst);
	expect(worst <= 1, "pow01 within one ulp of the rounded double power");
}

} // namespace

int main()
{
	refusals();
	copies();
	powers();
	std::printf("%d checks hold of %d\n", n_checks - n_fail, n_checks);
	return n_fail ? 1 : 0;
}
