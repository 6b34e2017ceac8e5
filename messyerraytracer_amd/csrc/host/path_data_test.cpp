// path_data_test.cpp -- host/path_data.cpp and path.h without a device: every refusal of the path state calls and their order (every
// required pointer null in turn, every environment float not finite in turn), what passes; the generator's jump against stepping and
// first_draw for bounces 0 .. 32; the kernel's copy of a descriptor; the tone mappers on values worked out by hand and their clamps;
// the gamma against the C library's pow in double, rounded once, within one float ulp below and above 1.
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../path.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

namespace {

int n_checks = 0, n_fail = 0;

void expect(bool ok, const std::string &what)
{
	n_checks++;
	if (!ok) { n_fail++; std::printf("FAIL %s\n", what.c_str()); }
}

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
bool has(const char *s, const char *word) { return s && std::string(s).find(word) != std::string::npos; }

mrt_environment environment()
{
	mrt_environment e;
	std::memset(&e, 0, sizeof(e));
	const float v[13] = { 0.15f, 0.25f, 0.55f, 0.6f, 0.7f, 0.85f, 0.15f, 0.12f, 0.1f, 1.0f, 0.9f, 0.8f, 0.15f };
	std::memcpy(&e, v, sizeof(v));
	return e;
}

void *const P = reinterpret_cast<void *>(16); // never dereferenced

mrt_path_step_desc descriptor(const mrt_environment *env)
{
	mrt_path_step_desc d;
	std::memset(&d, 0, sizeof(d));
	d.frame = 7u; d.bounce = 2u; d.max_bounces = 4u;
	d.d_direct = reinterpret_cast<const float *>(P); d.d_state = reinterpret_cast<mrt_path_state *>(P); d.env = env;
	d.d_out_select = reinterpret_cast<uint8_t *>(P);
	return d;
}

void refusals()
{
	const uint32_t known = MRT_FLAG_HOST_LAYOUT | MRT_FLAG_ASYNC;
	const mrt_environment env = environment();
	const mrt_path_step_desc good = descriptor(&env);
	expect(mrt::path_step_invalid(P, P, P, &good, 0u, known) == nullptr, "a good step refused");
	expect(mrt::path_step_invalid(P, P, P, &good, known, known) == nullptr, "both flags refused");
	mrt_path_step_desc d = good; d.d_out_lobe = nullptr; d.d_active_count = nullptr; d.reserved = 0xFFFFFFFFu;
	expect(mrt::path_step_invalid(P, P, P, &d, 0u, known) == nullptr, "optional pointers null refused, or the reserved word looked at");
	// 1. null required pointers
	expect(has(mrt::path_step_invalid(nullptr, P, P, &good, 0u, known), "null"), "null rays accepted");
	expect(has(mrt::path_step_invalid(P, nullptr, P, &good, 0u, known), "null"), "null hits accepted");
	expect(has(mrt::path_step_invalid(P, P, nullptr, &good, 0u, known), "null"), "null rows accepted");
	expect(has(mrt::path_step_invalid(P, P, P, nullptr, 0u, known), "null"), "null descriptor accepted");
	d = good; d.d_direct = nullptr; expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "null"), "null d_direct accepted");
	d = good; d.d_state = nullptr; expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "null"), "null d_state accepted");
	d = good; d.env = nullptr; expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "null"), "null env accepted");
	d = good; d.d_out_select = nullptr; expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "null"), "null d_out_select accepted");
	// 2. flags
	for (uint32_t bit = 0; bit < 32u; bit++) {
		const uint32_t f = 1u << bit;
		expect((mrt::path_step_invalid(P, P, P, &good, f, known) != nullptr) == ((f & known) == 0u), "flag bit " + std::to_string(bit));
	}
	expect(has(mrt::path_step_invalid(P, P, P, &good, MRT_FLAG_HOST_LAYOUT, MRT_FLAG_ASYNC), "flag"), "the host layout accepted by the grid form");
	// 3. bounce > max_bounces
	d = good; d.bounce = 5u; expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "bounce >"), "bounce > max_bounces accepted");
	d = good; d.bounce = 4u; expect(mrt::path_step_invalid(P, P, P, &d, 0u, known) == nullptr, "bounce == max_bounces refused");
	d = good; d.bounce = 0u; d.max_bounces = 0u; expect(mrt::path_step_invalid(P, P, P, &d, 0u, known) == nullptr, "max_bounces 0 refused");
	// 4. the reference's own limits
	d = good; d.frame = MRT_PATH_MAX_FRAME; expect(mrt::path_step_invalid(P, P, P, &d, 0u, known) == nullptr, "the largest frame refused");
	d = good; d.frame = MRT_PATH_MAX_FRAME + 1u; expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "frame"), "frame 1000000 accepted");
	d = good; d.frame = 0xFFFFFFFFu; expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "frame"), "frame 2^32 - 1 accepted");
	d = good; d.bounce = d.max_bounces = MRT_PATH_MAX_BOUNCES; expect(mrt::path_step_invalid(P, P, P, &d, 0u, known) == nullptr, "the largest bounce refused");
	d = good; d.max_bounces = MRT_PATH_MAX_BOUNCES + 1u; expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "max_bounces >"), "max_bounces 33 accepted");
	d = good; d.bounce = d.max_bounces = 0xFFFFFFFFu; expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "max_bounces >"), "bounce 2^32 - 1 accepted");
	// 5. the environment
	const float bad[3] = { std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity() };
	for (int w = 0; w < 13; w++)
		for (float x : bad) {
			mrt_environment e = env; reinterpret_cast<float *>(&e)[w] = x;
			d = descriptor(&e);
			expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "finite"), "environment word " + std::to_string(w) + " not finite, accepted");
		}
	mrt_environment e = env; e.reserved[0] = 0x7FC00000u; e.reserved[2] = 0x7F800000u;
	d = descriptor(&e);
	expect(mrt::path_step_invalid(P, P, P, &d, 0u, known) == nullptr, "the environment's reserved words looked at");
	// the order: pointer, flag, bounce, limits, environment
	e = env; e.ambient_energy = bad[0];
	d = descriptor(&e); d.bounce = 40u; d.max_bounces = 33u; d.frame = 2000000u; d.d_state = nullptr;
	expect(has(mrt::path_step_invalid(P, P, P, &d, 1u << 20, known), "null"), "order: pointers first");
	d.d_state = reinterpret_cast<mrt_path_state *>(P);
	expect(has(mrt::path_step_invalid(P, P, P, &d, 1u << 20, known), "flag"), "order: flags second");
	expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "bounce >"), "order: bounce > max_bounces third");
	d.bounce = 33u;
	expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "frame"), "order: the limits fourth");
	d.frame = 0u;
	expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "max_bounces >"), "order: the limits fourth (bounces)");
	d.bounce = d.max_bounces = 3u;
	expect(has(mrt::path_step_invalid(P, P, P, &d, 0u, known), "finite"), "order: the environment last");
	// init and finish
	expect(mrt::path_frame_invalid(P, nullptr, false, 0u, 0u) == nullptr && mrt::path_frame_invalid(P, nullptr, false, MRT_FLAG_ASYNC, 0u) == nullptr, "a good init refused");
	expect(has(mrt::path_frame_invalid(nullptr, nullptr, false, 0u, 0u), "null"), "init: null state accepted");
	expect(has(mrt::path_frame_invalid(P, nullptr, false, MRT_FLAG_HOST_LAYOUT, 0u), "flag"), "init: the host layout accepted");
	for (uint32_t m = 0; m <= 4u; m++) expect(mrt::path_frame_invalid(P, P, true, MRT_FLAG_ASYNC, m) == nullptr, "finish mode " + std::to_string(m) + " refused");
	expect(has(mrt::path_frame_invalid(P, P, true, 0u, 5u), "tonemap"), "finish: mode 5 accepted");
	expect(has(mrt::path_frame_invalid(P, P, true, 0u, 0xFFFFFFFFu), "tonemap"), "finish: mode 2^32 - 1 accepted");
	expect(has(mrt::path_frame_invalid(nullptr, P, true, 1u << 9, 9u), "null") && has(mrt::path_frame_invalid(P, nullptr, true, 1u << 9, 9u), "null"), "finish order: pointers first");
	expect(has(mrt::path_frame_invalid(P, P, true, 1u << 9, 9u), "flag"), "finish order: flags before the mode");
}

void draws()
{
	const uint32_t want[8] = { 0u, 3u, 6u, 10u, 14u, 18u, 22u, 26u }; // 3 per bounce, a roulette draw after bounces 2, 3, ...
	for (uint32_t b = 0; b < 8u; b++) expect(mrt::path_first_draw(b) == want[b], "first_draw of bounce " + std::to_string(b));
	expect(mrt::path_first_draw(MRT_PATH_MAX_BOUNCES) == 126u, "first_draw of the last bounce");
	// the jump against stepping
	uint32_t a = 1u, c = 0u;
	bool same = true;
	for (uint32_t k = 0; k <= 200u; k++) {
		uint32_t ja, jc;
		mrt::path_jump(k, ja, jc);
		same = same && ja == a && jc == c;
		a = a * 747796405u; c = c * 747796405u + 2891336453u;
	}
	expect(same, "path_jump(k) is k steps");
	const mrt_environment env = environment();
	mrt_path_step_desc d = descriptor(&env);
	d.frame = 11u; d.bounce = 3u; d.max_bounces = 5u;
	uint32_t count = 0; uint8_t lobe = 0;
	d.d_out_lobe = &lobe; d.d_active_count = &count;
	mrt::PathParams s;
	std::memset(&s, 0, sizeof(s));
	mrt::fill_path_params(&d, 640u * 20u, s);
	uint32_t ja, jc;
	mrt::path_jump(10u, ja, jc);
	expect(s.bounce == 3u && s.max_bounces == 5u && s.jump_a == ja && s.jump_c == jc, "the kernel's bounce and jump");
	expect(s.seed_add == 640u * 20u * 1009u + 11u * 6529u + 7u, "the kernel's seed");
	expect(s.direct == d.d_direct && s.state == d.d_state && s.out_select == d.d_out_select && s.out_lobe == &lobe && s.active_count == &count, "the kernel's pointers");
	expect(s.zenith[2] == 0.55f && s.horizon[0] == 0.6f && s.ground[1] == 0.12f && s.ambient[1] == 0.9f && s.ambient_energy == 0.15f, "the kernel's environment");
}

int ulps(float a, float b) { return std::abs((int)(bits(a) - bits(b))); }

void tones()
{
	const float white = mrt::hable_partial(11.2f);
	expect(mrt::tonemap(0.75f, 0u, white) == 0.75f && mrt::tonemap(-3.0f, 0u, white) == -3.0f && mrt::tonemap(1e4f, 0u, white) == 1e4f, "linear is the identity");
	expect(mrt::tonemap(1.0f, 1u, white) == 0.5f && mrt::tonemap(3.0f, 1u, white) == 0.75f && mrt::tonemap(0.0f, 1u, white) == 0.0f, "Reinhard");
	expect(mrt::tonemap(11.2f, 2u, white) == 1.0f, "Hable maps its white point to 1");
	const float e_f = 0.02f / 0.30f;
	expect(bits(mrt::hable_partial(0.0f)) == bits(((0.20f * 0.02f) / (0.20f * 0.30f)) - e_f), "Hable at 0");
	expect(bits(mrt::hable_partial(1.0f)) == bits((((0.15f + 0.10f * 0.50f) + 0.20f * 0.02f) / ((0.15f + 0.50f) + 0.20f * 0.30f)) - e_f), "Hable at 1");
	expect(mrt::tonemap(0.0f, 3u, white) == 0.0f && mrt::tonemap(1e4f, 3u, white) == 1.0f && mrt::tonemap(-0.005f, 3u, white) == 0.0f, "ACES and its clamp");
	expect(bits(mrt::tonemap(1.0f, 3u, white)) == bits((2.51f + 0.03f) / ((2.43f + 0.59f) + 0.14f)), "ACES at 1");
	expect(mrt::tonemap(0.0f, 4u, white) == 0.0f && mrt::tonemap(-2.0f, 4u, white) == 0.0f && mrt::tonemap(1e4f, 4u, white) <= 1.0f, "AgX at 0, below it and at 1e4");
	expect(bits(mrt::tonemap(1.0f, 4u, white)) == bits(1.0f / ((1.0f + 0.09f) + 0.0009f)), "AgX at 1");
	expect(mrt::path_gamma(-1.0f) == 0.0f && mrt::path_gamma(0.0f) == 0.0f && mrt::path_gamma(-0.0f) == 0.0f && mrt::path_gamma(1.0f) == 1.0f, "gamma at and below 0, at 1");
	expect(mrt::path_gamma(std::numeric_limits<float>::infinity()) == std::numeric_limits<float>::infinity(), "gamma of infinity");
	const float g = 1.0f / 2.2f;
	int worst = 0; uint64_t differ = 0, total = 0;
	for (uint32_t j = 1; j <= 65536u; j++)
		for (float scale : { 1.0f / 65536.0f, 1.0f, 37.0f }) { // (0, 1], (1, 2^16], beyond
			const float b = (float)j * scale;
			const int d = ulps(mrt::path_gamma(b), (float)std::pow((double)b, (double)g));
			worst = d > worst ? d : worst; differ += d != 0; total++;
		}
	for (float b : { std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::min(), 11.2f, 1e4f, 65536.0f, std::numeric_limits<float>::max() }) {
		const int d = ulps(mrt::path_gamma(b), (float)std::pow((double)b, (double)g));
		worst = d > worst ? d : worst; differ += d != 0; total++;
	}
	std::printf("gamma against pow in double: %llu of %llu differ, worst %d ulp\n", (unsigned long long)differ, (unsigned long long)total, worst);
	expect(worst <= 1, "gamma within one ulp of the rounded double power");
}

} // namespace

int main()
{
	refusals();
	draws();
	tones();
	std::printf("%d checks hold of %d\n", n_checks - n_fail, n_checks);
	return n_fail ? 1 : 0;
}
