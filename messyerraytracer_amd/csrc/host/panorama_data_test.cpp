// panorama_data_test.cpp -- host/panorama_data.cpp and panorama.h without a device: every refusal of mrt_upload_panorama's descriptor
// and their order, the scan of a host image; the wrap and clamp index rules of the four taps on 1x1, 2x1, 1x2 and 3x2 images with fx
// at -0.5, at an integer and at width - 0.5; the C99 sign cases of atan2_def, acos_def(+-1), and the non-finite rule (zeros, no texel
// read: the image pointer is then one that must not be dereferenced).
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../panorama.h"

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

bool has(const char *s, const char *word) { return s && std::string(s).find(word) != std::string::npos; }

uint32_t bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }

const float *const P = reinterpret_cast<const float *>(16); // never dereferenced

mrt_panorama desc(uint32_t w, uint32_t h, float energy, uint32_t flags)
{
	mrt_panorama p;
	std::memset(&p, 0, sizeof(p));
	p.pixels = P; p.width = w; p.height = h; p.energy = energy; p.flags = flags;
	return p;
}

void refusals()
{
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	expect(has(mrt::panorama_invalid(nullptr), "null panorama descriptor"), "null descriptor");
	mrt_panorama p = desc(4, 2, 1.0f, 0u);
	expect(mrt::panorama_invalid(&p) == nullptr, "a plain descriptor passes");
	p = desc(MRT_PANORAMA_MAX_DIM, MRT_PANORAMA_MAX_DIM, -2.5f, MRT_PANORAMA_ON_DEVICE);
	expect(mrt::panorama_invalid(&p) == nullptr, "the largest image, a negative energy and ON_DEVICE pass");
	p = desc(1, 1, 0.0f, 0u);
	expect(mrt::panorama_invalid(&p) == nullptr, "1x1 with energy 0 passes");
	p = desc(4, 2, 1.0f, 0u); p.pixels = nullptr;
	expect(has(mrt::panorama_invalid(&p), "pixels are null"), "null pixels");
	const uint32_t bad_dims[][2] = {{0, 2}, {4, 0}, {MRT_PANORAMA_MAX_DIM + 1u, 2}, {4, MRT_PANORAMA_MAX_DIM + 1u}, {0xFFFFFFFFu, 1}};
	for (const auto &d : bad_dims) {
		p = desc(d[0], d[1], 1.0f, 0u);
		expect(has(mrt::panorama_invalid(&p), "width or height"), "dimension " + std::to_string(d[0]) + "x" + std::to_string(d[1]));
	}
	for (float e : {inf, -inf, nan}) {
		p = desc(4, 2, e, 0u);
		expect(has(mrt::panorama_invalid(&p), "energy is not finite"), "energy not finite");
	}
	for (uint32_t b = 1; b < 32; b++) {
		p = desc(4, 2, 1.0f, 1u << b);
		expect(has(mrt::panorama_invalid(&p), "unknown flag"), "flag bit " + std::to_string(b));
		p.flags |= MRT_PANORAMA_ON_DEVICE;
		expect(has(mrt::panorama_invalid(&p), "unknown flag"), "flag bit " + std::to_string(b) + " with ON_DEVICE");
	}
	// the order: pixels, dimensions, energy, flag
	p = desc(0, 2, nan, 2u); p.pixels = nullptr;
	expect(has(mrt::panorama_invalid(&p), "pixels are null"), "order: pixels first");
	p.pixels = P;
	expect(has(mrt::panorama_invalid(&p), "width or height"), "order: dimensions second");
	p.width = 4;
	expect(has(mrt::panorama_invalid(&p), "energy"), "order: energy third");
	p.energy = 1.0f;
	expect(has(mrt::panorama_invalid(&p), "unknown flag"), "order: flag last");
	// the scan: r, g, b of every texel, never alpha
	std::vector<float> img(3 * 2 * 4, 0.5f);
	expect(mrt::panorama_texels_finite(img.data(), 6), "a finite image passes the scan");
	img[3] = nan; img[23] = inf;
	expect(mrt::panorama_texels_finite(img.data(), 6), "alpha is not read by the scan");
	for (int k : {0, 1, 2, 20, 21, 22}) {
		for (float bad : {inf, -inf, nan}) {
			const float keep = img[k];
			img[k] = bad;
			expect(!mrt::panorama_texels_finite(img.data(), 6), "the scan refuses float " + std::to_string(k));
			img[k] = keep;
		}
	}
	expect(mrt::panorama_texels_finite(img.data(), 0), "no texels: nothing to refuse");
}

// (u, v) whose fx = u * width - 0.5 and fy = v * height - 0.5 are the values given (exact for the sizes used)
void taps_at(float fx, float fy, uint32_t w, uint32_t h, mrt::PanoTaps &t)
{
	mrt::panorama_taps((fx + 0.5f) / (float)w, (fy + 0.5f) / (float)h, w, h, t);
}

void expect_taps(const char *what, float fx, float fy, uint32_t w, uint32_t h, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1, float sx, float sy)
{
	mrt::PanoTaps t;
	taps_at(fx, fy, w, h, t);
	const bool idx = t.i00 == y0 * w + x0 && t.i10 == y0 * w + x1 && t.i01 == y1 * w + x0 && t.i11 == y1 * w + x1;
	const bool wts = t.w00 == (1.0f - sx) * (1.0f - sy) && t.w10 == sx * (1.0f - sy) && t.w01 == (1.0f - sx) * sy && t.w11 == sx * sy;
	const bool inside = t.i00 < w * h && t.i10 < w * h && t.i01 < w * h && t.i11 < w * h;
	expect(idx && wts && inside, std::string(what) + " " + std::to_string(w) + "x" + std::to_string(h));
}

void index_rules()
{
	// 1x1: every tap is texel 0 whatever the weights
	expect_taps("1x1 fx -0.5", -0.5f, -0.5f, 1, 1, 0, 0, 0, 0, 0.5f, 0.5f);
	expect_taps("1x1 fx 0", 0.0f, 0.0f, 1, 1, 0, 0, 0, 0, 0.0f, 0.0f);
	expect_taps("1x1 fx 0.5", 0.5f, 0.5f, 1, 1, 0, 0, 0, 0, 0.5f, 0.5f);
	// 2x1: x wraps, y clamps to the one row
	expect_taps("2x1 fx -0.5", -0.5f, -0.5f, 2, 1, 1, 0, 0, 0, 0.5f, 0.5f);
	expect_taps("2x1 fx 0", 0.0f, 0.0f, 2, 1, 0, 1, 0, 0, 0.0f, 0.0f);
	expect_taps("2x1 fx 1", 1.0f, 0.0f, 2, 1, 1, 0, 0, 0, 0.0f, 0.0f);
	expect_taps("2x1 fx 1.5", 1.5f, 0.5f, 2, 1, 1, 0, 0, 0, 0.5f, 0.5f);
	// 1x2: the one column, y clamps at both ends
	expect_taps("1x2 fy -0.5", -0.5f, -0.5f, 1, 2, 0, 0, 0, 0, 0.5f, 0.5f);
	expect_taps("1x2 fy 0", 0.0f, 0.0f, 1, 2, 0, 0, 0, 1, 0.0f, 0.0f);
	expect_taps("1x2 fy 1", 0.0f, 1.0f, 1, 2, 0, 0, 1, 1, 0.0f, 0.0f);
	expect_taps("1x2 fy 1.5", 0.5f, 1.5f, 1, 2, 0, 0, 1, 1, 0.5f, 0.5f);
	// 3x2
	expect_taps("3x2 fx -0.5", -0.5f, -0.5f, 3, 2, 2, 0, 0, 0, 0.5f, 0.5f);
	expect_taps("3x2 fx 0", 0.0f, 0.0f, 3, 2, 0, 1, 0, 1, 0.0f, 0.0f);
	expect_taps("3x2 fx 1", 1.0f, 1.0f, 3, 2, 1, 2, 1, 1, 0.0f, 0.0f);
	expect_taps("3x2 fx 2", 2.0f, 0.25f, 3, 2, 2, 0, 0, 1, 0.0f, 0.25f);
	expect_taps("3x2 fx 2.5", 2.5f, 1.5f, 3, 2, 2, 0, 1, 1, 0.5f, 0.5f);
	// u outside [0, 1) wraps to the same taps; v outside [0, 1] clamps
	mrt::PanoTaps a, b;
	mrt::panorama_taps(0.25f, 0.25f, 4, 4, a);
	mrt::panorama_taps(-0.75f, 0.25f, 4, 4, b);
	expect(std::memcmp(&a, &b, sizeof(a)) == 0, "u = -0.75 samples as u = 0.25");
	mrt::panorama_taps(3.25f, 0.25f, 4, 4, b);
	expect(std::memcmp(&a, &b, sizeof(a)) == 0, "u = 3.25 samples as u = 0.25");
	mrt::panorama_taps(0.25f, 1.0f, 4, 4, a);
	mrt::panorama_taps(0.25f, 7.0f, 4, 4, b);
	expect(std::memcmp(&a, &b, sizeof(a)) == 0, "v = 7 samples as v = 1");
	mrt::panorama_taps(0.25f, 0.0f, 4, 4, a);
	mrt::panorama_taps(0.25f, -3.0f, 4, 4, b);
	expect(std::memcmp(&a, &b, sizeof(a)) == 0, "v = -3 samples as v = 0");
	// u - floorf(u) == 1 for a tiny negative u: fx = width - 0.5, the last column and the first
	mrt::panorama_taps(-1e-10f, 0.5f, 3, 2, a);
	expect(a.i00 % 3u == 2u && a.i10 % 3u == 0u && a.w00 + a.w01 == 0.5f, "u = -1e-10 lands on the seam");
	// the largest image: the last texel is addressed without a wrap of the index
	mrt::panorama_taps(1.0f, 1.0f, MRT_PANORAMA_MAX_DIM, MRT_PANORAMA_MAX_DIM, a);
	expect(a.i01 == MRT_PANORAMA_MAX_DIM * MRT_PANORAMA_MAX_DIM - 1u && a.i11 == (MRT_PANORAMA_MAX_DIM - 1u) * MRT_PANORAMA_MAX_DIM, "16384 x 16384 corner");
	expect(mrt::pano_wrap_x(-1, 5) == 4 && mrt::pano_wrap_x(5, 5) == 0 && mrt::pano_wrap_x(3, 5) == 3 && mrt::pano_wrap_x(0, 1) == 0 &&
			mrt::pano_wrap_x(1, 1) == 0 && mrt::pano_wrap_x(-1, 1) == 0, "pano_wrap_x");
	expect(mrt::pano_clamp_y(-1, 5) == 0 && mrt::pano_clamp_y(5, 5) == 4 && mrt::pano_clamp_y(2, 5) == 2 && mrt::pano_clamp_y(1, 1) == 0, "pano_clamp_y");
}

void definitions()
{
	const float pi = 3.14159274f, half_pi = 1.57079637f, quarter_pi = 0.785398185f, den = std::numeric_limits<float>::denorm_min();
	struct Case { float y, x, want; };
	const Case cases[] = {
		{0.0f, 1.0f, 0.0f}, {-0.0f, 1.0f, -0.0f}, {0.0f, -1.0f, pi}, {-0.0f, -1.0f, -pi},
		{0.0f, 0.0f, 0.0f}, {-0.0f, 0.0f, -0.0f}, {0.0f, -0.0f, pi}, {-0.0f, -0.0f, -pi},
		{1.0f, 0.0f, half_pi}, {1.0f, -0.0f, half_pi}, {-1.0f, 0.0f, -half_pi}, {-1.0f, -0.0f, -half_pi},
		{1.0f, 1.0f, quarter_pi}, {-1.0f, 1.0f, -quarter_pi}, {1.0f, -1.0f, (float)2.356194490192345}, {-1.0f, -1.0f, -(float)2.356194490192345},
		{den, -1.0f, pi}, {-den, -1.0f, -pi}, {den, 1.0f, den}, {-den, 1.0f, -den},
		{3.0e38f, 3.0e38f, quarter_pi}, {den, den, quarter_pi}, {1.0f, 3.0e38f, (float)(1.0 / (double)3.0e38f)},
	};
	for (const Case &c : cases)
		expect(bits(mrt::atan2_def(c.y, c.x)) == bits(c.want), "atan2_def(" + std::to_string(c.y) + ", " + std::to_string(c.x) + ")");
	// against the C library over a coarse lattice: within one ulp (the sweep of the Python tests is the fine one)
	int worst = 0;
	for (int a = -40; a <= 40; a++) {
		for (int b = -40; b <= 40; b++) {
			const float y = (float)a * 0.173f, x = (float)b * 0.291f;
			if (a == 0 && b == 0) continue;
			const float got = mrt::atan2_def(y, x), want = (float)std::atan2((double)y, (double)x);
			const int d = std::abs((int)(bits(got) & 0x7FFFFFFFu) - (int)(bits(want) & 0x7FFFFFFFu));
			if ((bits(got) ^ bits(want)) >> 31) worst = 1000;
			if (d > worst) worst = d;
		}
	}
	expect(worst <= 1, "atan2_def within 1 ulp of the C library's on the lattice (worst " + std::to_string(worst) + ")");
	expect(bits(mrt::acos_def(1.0f)) == bits(0.0f), "acos_def(1) = +0");
	expect(bits(mrt::acos_def(-1.0f)) == bits(pi), "acos_def(-1) = pi");
	expect(bits(mrt::acos_def(0.0f)) == bits(half_pi) && bits(mrt::acos_def(-0.0f)) == bits(half_pi), "acos_def(+-0) = pi / 2");
	expect(bits(mrt::acos_def(0.5f)) == bits((float)std::acos(0.5)), "acos_def(0.5)");
	float u, v;
	mrt::equirect_uv(0.0f, 1.0f, 0.0f, u, v);
	expect(u == 0.5f && v == 0.0f, "+y: (0.5, 0)");
	mrt::equirect_uv(0.0f, -1.0f, 0.0f, u, v);
	const float k_u = 0.5f / pi, k_v = 1.0f / pi; // (pi here is the float PI of the definition)
	expect(u == 0.5f && v == pi * k_v, "-y: (0.5, pi * (1 / PI))");
	mrt::equirect_uv(0.0f, 1.5f, 1.0f, u, v);
	expect(u == 0.5f && v == 0.0f, "dir.y above 1 is clamped");
	mrt::equirect_uv(0.0f, -1.5f, 1.0f, u, v);
	expect(u == 0.5f && v == pi * k_v, "dir.y below -1 is clamped");
	mrt::equirect_uv(0.0f, 0.0f, -1.0f, u, v);
	expect(u == pi * k_u + 0.5f && v == half_pi * k_v, "(+0, 0, -1): the seam from the right");
	mrt::equirect_uv(-0.0f, 0.0f, -1.0f, u, v);
	expect(u == -pi * k_u + 0.5f && v == half_pi * k_v, "(-0, 0, -1): the seam from the left");
	mrt::PanoTaps a, b; // ... where the wrap makes them the same texels
	mrt::panorama_taps(pi * k_u + 0.5f, 0.5f, 64, 32, a);
	mrt::panorama_taps(-pi * k_u + 0.5f, 0.5f, 64, 32, b);
	expect(a.i00 == b.i00 && a.i10 == b.i10 && a.i01 == b.i01 && a.i11 == b.i11 && a.i00 % 64u == 63u && a.i10 % 64u == 0u, "both sides of the seam read the same texels");
}

void non_finite_rule()
{
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	for (int k = 0; k < 3; k++) {
		for (float bad : {inf, -inf, nan}) {
			float d[3] = {0.0f, 0.6f, 0.8f};
			d[k] = bad;
			float r = 1.0f, g = 1.0f, b = 1.0f;
			mrt::sky_panorama(P, 4, 2, 3.0f, d[0], d[1], d[2], r, g, b); // P must not be read
			expect(bits(r) == 0u && bits(g) == 0u && bits(b) == 0u, "a non-finite component " + std::to_string(k) + " gives zeros");
			expect(!mrt::finite3(d[0], d[1], d[2]), "finite3 refuses it");
		}
	}
	expect(mrt::finite3(0.0f, -3.0e38f, std::numeric_limits<float>::denorm_min()), "finite3 passes finite values");
	// and a finite direction samples: a 2x1 image, straight up -> v = 0, u = 0.5: fx = 0.5, half of each texel, times the energy
	const float img[8] = {1.0f, 2.0f, 4.0f, 9.0f, 3.0f, 6.0f, 8.0f, 9.0f};
	float r, g, b;
	mrt::sky_panorama(img, 2, 1, 2.0f, 0.0f, 1.0f, 0.0f, r, g, b);
	expect(r == 4.0f && g == 8.0f && b == 12.0f, "a 2x1 image sampled straight up");
}

} // namespace

int main()
{
	refusals();
	index_rules();
	definitions();
	non_finite_rule();
	if (n_fail) { std::printf("%d of %d checks FAILED\n", n_fail, n_checks); return 1; }
	std::printf("%d checks hold\n", n_checks);
	return 0;
}
