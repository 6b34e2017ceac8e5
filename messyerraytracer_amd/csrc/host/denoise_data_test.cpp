// denoise_data_test.cpp -- host/denoise_data.cpp and denoise.h without a device: every refusal of the five calls and their order (a call
// with everything wrong is mended one argument at a time, and the reason must move down the header's list), the radius clamp, and the
// kernel's arguments.  Given a file (tests/test_denoise_cpu.py writes it from messyerraytracer_amd/denoise.py: little-endian, in the
// order read below), the host definitions are held bit for bit to the numpy restatement: expn_def on every argument of the file, the
// w_spatial tables of r = 1 .. 4, the four passes on small images of both normal kinds, and the guides.
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../denoise.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace {

using namespace mrt::dn;

int n_checks = 0, n_fail = 0;

void expect(bool ok, const std::string &what)
{
	n_checks++;
	if (!ok) { n_fail++; if (n_fail <= 40) std::printf("FAIL %s\n", what.c_str()); }
}

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
bool has(const char *s, const char *word) { return s && std::string(s).find(word) != std::string::npos; }
bool same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || bits(a) == bits(b); }

void *const A = reinterpret_cast<void *>(16); // never dereferenced
void *const B = reinterpret_cast<void *>(4096);
void *const G = reinterpret_cast<void *>(8192);
void *const O = reinterpret_cast<void *>(12288);
void *const O2 = reinterpret_cast<void *>(16384);
void *const O3 = reinterpret_cast<void *>(20480);

mrt_denoise_params defaults()
{
	mrt_denoise_params p;
	std::memset(&p, 0, sizeof(p));
	p.struct_size = (uint32_t)sizeof(p); p.kernel_radius = 2;
	p.depth_sigma = 1.0f; p.normal_sigma = 128.0f; p.color_sigma = 4.0f; p.blend_factor = 0.1f;
	p.depth_threshold = 0.1f; p.roughness_threshold = 0.3f; p.intensity = 1.0f; p.f0 = 0.04f;
	p.inv_view[0] = p.inv_view[5] = p.inv_view[10] = p.inv_view[15] = 1.0f;
	return p;
}

void refusals()
{
	expect(sizeof(mrt_denoise_params) == 112, "mrt_denoise_params is 112 bytes");
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	const mrt_denoise_params ok = defaults();
	// everything wrong at once, then mended in the header's order; W * H * 32 overflows with W = H = 0xffffffff
	const uint32_t BIG = 0xffffffffu;
	for (int call = DN_SPATIAL; call <= DN_RESOLVE; call++) {
		const std::string c = "call " + std::to_string(call) + ": ";
		const bool guides = call != DN_TEMPORAL, hist = call == DN_TEMPORAL || call == DN_RESOLVE, color = call == DN_COMPOSITE || call == DN_RESOLVE;
		const bool out = call == DN_SPATIAL || call == DN_TEMPORAL;
		mrt_denoise_params bad = ok;
		bad.struct_size = 111u; bad.normal_kind = 2u; bad.depth_sigma = nan; bad.inv_view[15] = inf;
		const void *refl = nullptr, *depth = nullptr, *guide = nullptr, *h = nullptr, *col = nullptr, *o = nullptr;
		auto why = [&](const mrt_denoise_params *p, uint32_t flags) { return denoise_invalid(call, p, BIG, BIG, refl, depth, guide, h, col, o, flags); };
		expect(has(why(nullptr, 2u), "null params"), c + "null params first");
		expect(has(why(&bad, 2u), call == DN_TEMPORAL ? "null d_current" : "null d_reflection"), c + "the first image");
		refl = A;
		if (guides) {
			expect(has(why(&bad, 2u), "null d_depth"), c + "d_depth");
			depth = B;
			expect(has(why(&bad, 2u), "null d_normal_roughness"), c + "d_normal_roughness");
			guide = G;
		}
		if (hist) { expect(has(why(&bad, 2u), "null d_history"), c + "d_history"); h = call == DN_RESOLVE ? A : O; }
		if (color) { expect(has(why(&bad, 2u), "null d_color"), c + "d_color"); col = call == DN_RESOLVE ? B : O2; }
		if (out) { expect(has(why(&bad, 2u), "null d_out"), c + "d_out"); o = call == DN_SPATIAL ? A : O3; }
		if (call == DN_RESOLVE) o = G; // d_denoised is optional, and aliases a guide here
		expect(has(why(&bad, 2u), "struct_size"), c + "struct_size");
		bad.struct_size = 112u;
		expect(has(why(&bad, 2u), "unknown flag"), c + "flags");
		expect(has(why(&bad, MRT_FLAG_ASYNC | MRT_FLAG_COHERENT), "unknown flag"), c + "ASYNC with another flag");
		expect(has(why(&bad, MRT_FLAG_ASYNC), "normal_kind"), c + "normal_kind");
		bad.normal_kind = MRT_NORMAL_WORLD;
		expect(has(why(&bad, 0u), "non-finite parameter"), c + "a NaN sigma");
		bad.depth_sigma = 1.0f;
		expect(has(why(&bad, 0u), "non-finite inv_view"), c + "an infinite inv_view");
		bad.inv_view[15] = 1.0f;
		expect(has(why(&bad, 0u), "overflows"), c + "W * H * 32");
		auto small = [&]() { return denoise_invalid(call, &bad, 7u, 5u, refl, depth, guide, h, col, o, 0u); };
		if (call == DN_SPATIAL) {
			expect(has(small(), "d_out is d_reflection"), c + "d_out == d_reflection");
			o = O;
		}
		if (call == DN_RESOLVE) {
			expect(has(small(), "read across pixels"), c + "d_history == d_reflection");
			h = O;
			expect(has(small(), "read across pixels"), c + "d_color == d_depth");
			col = O2;
			expect(has(small(), "read across pixels"), c + "d_denoised == d_normal_roughness");
			o = nullptr;
			expect(small() == nullptr, c + "no d_denoised refused");
			o = O3;
		}
		expect(small() == nullptr, c + "a good call refused");
		expect(denoise_invalid(call, &bad, 0u, BIG, refl, depth, guide, h, col, o, 0u) == nullptr, c + "W == 0 refused");
		expect(denoise_invalid(call, &bad, 0x08000000u, 0x10u, refl, depth, guide, h, col, o, 0u) == nullptr, c + "2^31 pixels refused");
		expect(has(denoise_invalid(call, &bad, 0x80000000u, 0x10000000u, refl, depth, guide, h, col, o, 0u), "overflows"), c + "2^59 pixels accepted");
		// each scalar and each matrix entry on its own
		float *scalars[8] = {&bad.depth_sigma, &bad.normal_sigma, &bad.color_sigma, &bad.blend_factor, &bad.depth_threshold, &bad.roughness_threshold,
				&bad.intensity, &bad.f0};
		for (float *s : scalars) {
			const float keep = *s;
			*s = -inf; expect(has(small(), "non-finite parameter"), c + "an infinite scalar");
			*s = -1e30f; expect(small() == nullptr, c + "a large negative scalar refused");
			*s = keep;
		}
		for (float &m : bad.inv_view) {
			const float keep = m;
			m = nan; expect(has(small(), "non-finite inv_view"), c + "a NaN matrix entry");
			m = keep;
		}
		if (call == DN_TEMPORAL) { // in place is allowed
			expect(denoise_invalid(call, &bad, 7u, 5u, refl, nullptr, nullptr, O, nullptr, O, 0u) == nullptr, c + "d_out == d_history refused");
		}
	}
	// the guides
	expect(has(guides_invalid(nullptr, nullptr, UINT64_MAX, NAN, nullptr, nullptr, 2u), "null d_hits"), "guides: d_hits");
	expect(has(guides_invalid(A, nullptr, UINT64_MAX, NAN, nullptr, nullptr, 2u), "null d_rows"), "guides: d_rows");
	expect(has(guides_invalid(A, B, UINT64_MAX, NAN, nullptr, nullptr, 2u), "null d_depth"), "guides: d_depth");
	expect(has(guides_invalid(A, B, UINT64_MAX, NAN, O, nullptr, 2u), "null d_normal_roughness"), "guides: d_normal_roughness");
	expect(has(guides_invalid(A, B, UINT64_MAX, NAN, O, O2, 2u), "unknown flag"), "guides: flags");
	expect(has(guides_invalid(A, B, UINT64_MAX, NAN, O, O2, MRT_FLAG_ASYNC), "non-finite"), "guides: inv_depth_range");
	expect(has(guides_invalid(A, B, UINT64_MAX, 0.5f, O, O2, 0u), "overflows"), "guides: count");
	expect(guides_invalid(A, B, UINT64_MAX / 64u, 0.5f, O, O2, 0u) == nullptr && guides_invalid(A, B, 0u, 0.0f, O, O2, MRT_FLAG_ASYNC) == nullptr, "guides: a good call refused");
}

void arguments()
{
	mrt_denoise_params p = defaults();
	for (int k = 0; k < 16; k++) p.inv_view[k] = (float)(k + 1);
	const int radii[][2] = {{0, 1}, {-7, 1}, {1, 1}, {2, 2}, {3, 3}, {4, 4}, {5, 4}, {9, 4}, {0x7fffffff, 4}, {(int)0x80000000, 1}};
	for (auto &rr : radii) {
		p.kernel_radius = rr[0];
		DenoiseArgs a;
		fill_denoise_args(&p, 33u, 17u, a);
		expect(a.radius == rr[1] && a.w == 33u && a.h == 17u, "radius " + std::to_string(rr[0]));
		const int n = 2 * a.radius + 1;
		expect(a.w_spatial[(n * n) / 2] == 1.0f && a.w_spatial[0] == a.w_spatial[n * n - 1] && a.w_spatial[0] < a.w_spatial[1], "the table's shape");
		for (int k = n * n; k < 81; k++) expect(a.w_spatial[k] == 0.0f, "the table's tail is zero");
		expect(a.m[0] == 1.0f && a.m[1] == 2.0f && a.m[2] == 3.0f && a.m[3] == 5.0f && a.m[6] == 9.0f && a.m[8] == 11.0f, "the 3x3 of inv_view");
	}
	p.has_history = 7u;
	DenoiseArgs a;
	fill_denoise_args(&p, 1u, 1u, a);
	expect(a.has_history == 1u, "has_history is a flag");
	// expn_def by hand
	expect(bits(expn_def(0.0f)) == bits(1.0f) && bits(expn_def(-0.0f)) == bits(1.0f), "expn_def(+-0) is 1");
	expect(expn_def(-104.5f) == 0.0f && expn_def(-1e30f) == 0.0f && expn_def(-std::numeric_limits<float>::infinity()) == 0.0f, "the flush to 0");
	expect(expn_def(-103.9f) > 0.0f, "a denormal result");
	expect(std::isnan(expn_def(NAN)) && std::isinf(expn_def(90.0f)) && expn_def(1.0f) == 2.7182817f, "NaN, a large and a small positive argument");
	// pow01 a few ulps above 1 has no select: b^e like any other
	expect(mrt::pow01(1.0f + 0x1p-22f, 128.0f) == 1.0000305f && mrt::pow01(1.0f + 0x1p-23f, 128.0f) > 1.0f, "pow01 just above 1");
	expect(std::isnan(mrt::pow01(NAN, 128.0f)), "pow01 of a NaN base");
}

struct Reader {
	std::FILE *f;
	bool ok = true;
	uint32_t u32() { uint32_t v = 0; ok = ok && std::fread(&v, 4, 1, f) == 1; return v; }
	template <class T> std::vector<T> array(size_t n)
	{
		std::vector<T> v(n);
		if (n) ok = ok && std::fread(v.data(), sizeof(T), n, f) == n;
		return v;
	}
};

size_t compare(const std::vector<Px4> &got, const std::vector<float> &want)
{
	size_t bad = 0;
	for (size_t i = 0; i < got.size(); i++) {
		const float g[4] = {got[i].x, got[i].y, got[i].z, got[i].w};
		for (int k = 0; k < 4; k++) bad += !same(g[k], want[4 * i + k]);
	}
	return bad;
}

int recorded(const char *path)
{
	Reader r{std::fopen(path, "rb")};
	if (!r.f) { std::printf("FAIL cannot open %s\n", path); return 1; }
	// expn_def
	const uint32_t n_exp = r.u32();
	const auto ey = r.array<float>(n_exp), ev = r.array<float>(n_exp);
	size_t bad = 0;
	for (uint32_t i = 0; i < n_exp; i++) bad += !same(expn_def(ey[i]), ev[i]);
	expect(r.ok && bad == 0, "expn_def: " + std::to_string(bad) + " arguments differ from the restatement");
	// tables
	for (int radius = 1; radius <= 4; radius++) {
		const int n = (2 * radius + 1) * (2 * radius + 1);
		const auto want = r.array<float>(n);
		float got[81];
		spatial_table(radius, got);
		bad = 0;
		for (int k = 0; k < n; k++) bad += bits(got[k]) != bits(want[k]);
		expect(r.ok && bad == 0, "w_spatial of radius " + std::to_string(radius));
	}
	// the passes
	const uint32_t n_cases = r.u32();
	for (uint32_t c = 0; c < n_cases && r.ok; c++) {
		const auto pb = r.array<unsigned char>(sizeof(mrt_denoise_params));
		mrt_denoise_params p;
		std::memcpy(&p, pb.data(), sizeof(p));
		const uint32_t w = r.u32(), h = r.u32();
		const size_t n = (size_t)w * h;
		const auto refl = r.array<Px4>(n); const auto depth = r.array<float>(n); const auto guide = r.array<Px4>(n);
		auto hist = r.array<Px4>(n); auto color = r.array<Px4>(n);
		const auto want_den = r.array<float>(4 * n), want_hist = r.array<float>(4 * n), want_color = r.array<float>(4 * n);
		if (!r.ok) break;
		DenoiseArgs a;
		fill_denoise_args(&p, w, h, a);
		std::vector<Px4> den(n);
		for (uint32_t y = 0; y < h; y++)
			for (uint32_t x = 0; x < w; x++) {
				const size_t i = (size_t)y * w + x;
				den[i] = spatial_pixel(a, a.w_spatial, GlobalFetch{refl.data(), depth.data(), guide.data(), w, h, a.normal_kind, (int64_t)x, (int64_t)y});
				hist[i] = temporal_pixel(a, den[i], hist[i]); // in place
				(void)composite_pixel(a, x, y, hist[i], depth[i], guide[i], color[i]);
			}
		const std::string what = "case " + std::to_string(c) + " (" + std::to_string(w) + " x " + std::to_string(h) + "): ";
		expect((bad = compare(den, want_den)) == 0, what + std::to_string(bad) + " spatial words differ");
		expect((bad = compare(hist, want_hist)) == 0, what + std::to_string(bad) + " temporal words differ");
		expect((bad = compare(color, want_color)) == 0, what + std::to_string(bad) + " composite words differ");
	}
	// the guides
	const uint32_t n_g = r.u32();
	const auto hits = r.array<mrt_hit32>(n_g); const auto rows = r.array<mrt_surface64>(n_g);
	const auto inv = r.array<float>(1);
	const auto want_d = r.array<float>(n_g), want_g = r.array<float>(4 * (size_t)n_g);
	bad = 0;
	for (uint32_t i = 0; i < n_g && r.ok; i++) {
		float d; Px4 g;
		guide_texels(hits[i], rows[i], inv[0], d, g);
		bad += !same(d, want_d[i]) + !same(g.x, want_g[4 * i]) + !same(g.y, want_g[4 * i + 1]) + !same(g.z, want_g[4 * i + 2]) + !same(g.w, want_g[4 * i + 3]);
	}
	expect(r.ok && bad == 0, "guides: " + std::to_string(bad) + " words differ");
	expect(r.ok && std::fgetc(r.f) == EOF, "the file is read to its end");
	std::fclose(r.f);
	std::printf("recorded: %u exp arguments, %u cases, %u guide records\n", n_exp, n_cases, n_g);
	return 0;
}

} // namespace

int main(int argc, char **argv)
{
	refusals();
	arguments();
	if (argc > 1 && recorded(argv[1])) return 1;
	std::printf("%d checks hold %s\n", n_checks - n_fail, n_fail ? "(some FAILED)" : "(all)");
	return n_fail ? 1 : 0;
}
