// svgf_data_test.cpp -- host/svgf_data.cpp and svgf.h without a device: every refusal of the six calls and their order (a call with
// everything wrong is mended one argument at a time, and the reason must move down the header's list) and the kernels' arguments.
// Given a file (tests/test_svgf_cpu.py writes it from messyerraytracer_amd/svgf.py: little-endian, in the order read below), the host
// definitions are held bit for bit to the numpy restatement: the five per-pixel passes chained on small images, and the guides.
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../svgf.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace {

using namespace mrt::sv;

int n_checks = 0, n_fail = 0;

void expect(bool ok, const std::string &what)
{
	n_checks++;
	if (!ok) { n_fail++; if (n_fail <= 40) std::printf("FAIL %s\n", what.c_str()); }
}

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
bool has(const char *s, const char *word) { return s && std::string(s).find(word) != std::string::npos; }
bool same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || bits(a) == bits(b); }

const void *ptr(int k) { return reinterpret_cast<const void *>((uintptr_t)4096 * (uintptr_t)(k + 1)); } // never dereferenced

mrt_svgf_params defaults()
{
	mrt_svgf_params p;
	std::memset(&p, 0, sizeof(p));
	p.struct_size = (uint32_t)sizeof(p); p.iterations = 5u;
	p.color_alpha = 0.2f; p.moments_alpha = 0.2f; p.max_history = 32.0f; p.normal_threshold = 0.95f; p.position_threshold = 0.05f;
	p.sigma_l = 4.0f; p.sigma_n = 128.0f; p.sigma_plane = 0.01f;
	return p;
}

// the images a call takes, in its argument order: {field, the word of its refusal}
struct Slot { const void *SvgfImages::*field; const char *word; bool history; };

std::vector<Slot> slots(int call)
{
	const bool t = call == SV_TEMPORAL, f = call == SV_FRAME;
	std::vector<Slot> s;
	s.push_back({&SvgfImages::illum, "null d_illum", false});
	if (call == SV_MODULATE || f) s.push_back({&SvgfImages::albedo, "null d_albedo", false});
	if (call == SV_VARIANCE) s.push_back({&SvgfImages::moments, "null d_moments", false});
	if (call != SV_MODULATE) {
		s.push_back({&SvgfImages::normal_depth, "null d_normal_depth", false});
		s.push_back({&SvgfImages::position, "null d_position", false});
	}
	if (t || f) {
		s.push_back({&SvgfImages::prev_illum, "null d_prev_illum", true});
		s.push_back({&SvgfImages::prev_moments, "null d_prev_moments", true});
		s.push_back({&SvgfImages::prev_normal_depth, "null d_prev_normal_depth", true});
		s.push_back({&SvgfImages::prev_position, "null d_prev_position", true});
	}
	if (call != SV_MODULATE) s.push_back({&SvgfImages::out_illum, t ? "null d_out_illum" : (f ? "null d_next_illum" : "null d_out"), false});
	if (t || f) s.push_back({&SvgfImages::out_moments, t ? "null d_out_moments" : "null d_next_moments", false});
	if (f) {
		s.push_back({&SvgfImages::scratch_a, "null d_scratch_a", false});
		s.push_back({&SvgfImages::scratch_b, "null d_scratch_b", false});
	}
	if (call == SV_MODULATE || f) s.push_back({&SvgfImages::rgba, "null d_rgba", false});
	return s;
}

void refusals()
{
	expect(sizeof(mrt_svgf_params) == 48, "mrt_svgf_params is 48 bytes");
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	const mrt_svgf_params ok = defaults();
	const uint32_t BIG = 0xffffffffu;
	mrt_camera ortho;
	std::memset(&ortho, 0, sizeof(ortho));
	ortho.kind = MRT_CAMERA_ORTHOGRAPHIC;
	mrt_camera persp = ortho;
	persp.kind = MRT_CAMERA_PERSPECTIVE;
	for (int call = SV_TEMPORAL; call <= SV_FRAME; call++) {
		const std::string c = "call " + std::to_string(call) + ": ";
		const bool temporal = call == SV_TEMPORAL || call == SV_FRAME, tone = call == SV_MODULATE || call == SV_FRAME;
		// everything wrong at once, then mended in the header's order
		mrt_svgf_params bad = ok;
		bad.struct_size = 47u; bad.has_history = 1u; bad.iterations = 6u; bad.tonemap_mode = 5u;
		bad.color_alpha = nan; bad.max_history = 0.5f; bad.sigma_plane = 0.0f;
		SvgfImages im = {};
		const mrt_camera *cam = nullptr;
		uint32_t step = 3u;
		auto why = [&](const mrt_svgf_params *p, uint32_t flags) { return svgf_invalid(call, p, BIG, BIG, step, cam, im, flags); };
		expect(has(why(nullptr, 2u), "null params"), c + "null params first");
		// every image equal to the first, so that the last check fails too
		for (const Slot &s : slots(call)) {
			expect(has(why(&bad, 2u), s.word), c + s.word);
			im.*(s.field) = ptr(0);
		}
		expect(has(why(&bad, 2u), "struct_size"), c + "struct_size");
		bad.struct_size = 48u;
		expect(has(why(&bad, 2u), "unknown flag"), c + "flags");
		expect(has(why(&bad, MRT_FLAG_ASYNC | MRT_FLAG_COHERENT), "unknown flag"), c + "ASYNC with another flag");
		if (temporal) {
			expect(has(why(&bad, MRT_FLAG_ASYNC), "null prev_cam"), c + "prev_cam");
			cam = &ortho;
			expect(has(why(&bad, 0u), "not MRT_CAMERA_PERSPECTIVE"), c + "an orthographic camera");
			cam = &persp;
		}
		if (call == SV_ATROUS) {
			for (uint32_t s : {0u, 3u, 5u, 32u, 17u}) { step = s; expect(has(why(&bad, 0u), "step is not"), c + "step " + std::to_string(s)); }
			step = 16u;
		}
		if (call == SV_FRAME) {
			expect(has(why(&bad, 0u), "iterations"), c + "iterations 6");
			bad.iterations = 0u;
			expect(has(why(&bad, 0u), "iterations"), c + "iterations 0");
			bad.iterations = 1u;
		}
		if (tone) { expect(has(why(&bad, 0u), "tonemap_mode"), c + "tonemap_mode"); bad.tonemap_mode = 4u; }
		expect(has(why(&bad, 0u), "non-finite"), c + "a NaN alpha");
		bad.color_alpha = 0.2f;
		expect(has(why(&bad, 0u), "max_history"), c + "max_history");
		bad.max_history = 1.0f;
		expect(has(why(&bad, 0u), "not > 0"), c + "sigma_plane 0");
		bad.sigma_plane = 0.01f;
		expect(has(why(&bad, 0u), "overflows"), c + "W * H * 32");
		auto small = [&]() { return svgf_invalid(call, &bad, 7u, 5u, step, cam, im, 0u); };
		if (call != SV_MODULATE) {
			// the images apart, one alias at a time
			int k = 0;
			const std::vector<Slot> sl = slots(call);
			for (const Slot &s : sl) im.*(s.field) = ptr(k++);
			expect(small() == nullptr, c + "a good call refused");
			const void *SvgfImages::*outs[5] = {&SvgfImages::out_illum, &SvgfImages::out_moments, &SvgfImages::scratch_a, &SvgfImages::scratch_b,
					&SvgfImages::rgba};
			for (auto o : outs) {
				if (!(im.*o)) continue;
				const void *keep = im.*o;
				for (const Slot &s : sl) {
					if (s.field == o) continue;
					const bool allowed = call == SV_TEMPORAL && !s.history && s.field != &SvgfImages::out_illum && s.field != &SvgfImages::out_moments;
					im.*o = im.*(s.field);
					expect(allowed ? small() == nullptr : has(small(), "read across pixels"), c + "an output equal to " + (s.word + 5));
					im.*o = keep;
				}
			}
			if (temporal) { // without history the previous images are not looked at
				bad.has_history = 0u;
				im.prev_illum = im.prev_moments = im.prev_normal_depth = im.prev_position = nullptr;
				cam = nullptr;
				expect(small() == nullptr, c + "null previous images refused without history");
				im.prev_illum = im.out_illum;
				expect(small() == nullptr, c + "an unread previous image counted as an alias");
			}
		} else {
			expect(small() == nullptr, c + "d_rgba == d_illum refused");
		}
		expect(svgf_invalid(call, &bad, 0u, BIG, step, cam, im, 0u) == nullptr, c + "W == 0 refused");
		expect(svgf_invalid(call, &bad, 0x08000000u, 0x10u, step, cam, im, 0u) == nullptr, c + "2^31 pixels refused");
		expect(has(svgf_invalid(call, &bad, 0x80000000u, 0x10000000u, step, cam, im, 0u), "overflows"), c + "2^59 pixels accepted");
		// each float on its own
		float *scalars[8] = {&bad.color_alpha, &bad.moments_alpha, &bad.max_history, &bad.normal_threshold, &bad.position_threshold, &bad.sigma_l,
				&bad.sigma_n, &bad.sigma_plane};
		for (int k = 0; k < 8; k++) {
			const float keep = *scalars[k];
			*scalars[k] = inf; expect(has(small(), "non-finite"), c + "an infinite float");
			*scalars[k] = -1.0f;
			expect(k < 2 ? small() == nullptr : has(small(), k == 2 ? "max_history" : "not > 0"), c + "a negative float " + std::to_string(k));
			*scalars[k] = keep;
		}
	}
	// the guides
	const void *g[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	const char *words[8] = {"null d_rays", "null d_hits", "null d_rows", "null d_source", "null d_illum", "null d_albedo", "null d_normal_depth", "null d_position"};
	auto gw = [&](uint32_t kind, uint64_t count, uint32_t flags) { return svgf_guides_invalid(g[0], g[1], g[2], kind, g[3], count, g[4], g[5], g[6], g[7], flags); };
	for (int k = 0; k < 8; k++) {
		expect(has(gw(1u, UINT64_MAX, 2u), words[k]), std::string("guides: ") + words[k]);
		g[k] = ptr(k < 5 ? k : 4);
	}
	expect(has(gw(1u, UINT64_MAX, 2u), "unknown flag"), "guides: flags");
	expect(has(gw(1u, UINT64_MAX, MRT_FLAG_ASYNC), "source_kind"), "guides: the tone-mapped kind");
	expect(has(gw(3u, UINT64_MAX, 0u), "source_kind"), "guides: an unknown kind");
	expect(has(gw(MRT_ACCUM_SRC_RGBA, UINT64_MAX, 0u), "overflows"), "guides: count");
	expect(has(gw(MRT_ACCUM_SRC_PATH_STATE, 4u, 0u), "two outputs"), "guides: equal outputs");
	for (int k = 5; k < 8; k++) g[k] = ptr(k);
	expect(gw(MRT_ACCUM_SRC_PATH_STATE, UINT64_MAX / 64u, 0u) == nullptr && gw(MRT_ACCUM_SRC_RGBA, 0u, MRT_FLAG_ASYNC) == nullptr, "guides: a good call refused");
}

void arguments()
{
	mrt_svgf_params p = defaults();
	p.has_history = 7u; p.tonemap_mode = 3u;
	mrt_camera cam;
	std::memset(&cam, 0, sizeof(cam));
	for (int k = 0; k < 3; k++) { cam.origin[k] = 1.0f + k; cam.fwd[k] = 4.0f + k; cam.right[k] = 7.0f + k; cam.up[k] = 10.0f + k; }
	cam.half_w = 0.5f; cam.half_h = 0.25f; cam.jitter_x = 0.125f; cam.jitter_y = 0.75f;
	SvgfArgs a;
	fill_svgf_args(&p, 33u, 17u, 8u, &cam, 2.5f, a);
	expect(a.w == 33u && a.h == 17u && a.step == 8 && a.has_history == 1u && a.mode == 3u && a.white == 2.5f, "the frame, the step and the flags");
	expect(a.origin[2] == 3.0f && a.fwd[0] == 4.0f && a.right[1] == 8.0f && a.up[2] == 12.0f && a.half_w == 0.5f && a.half_h == 0.25f &&
			a.jitter_x == 0.125f && a.jitter_y == 0.75f, "the camera");
	expect(a.color_alpha == 0.2f && a.max_history == 32.0f && a.sigma_plane == 0.01f && a.sigma_n == 128.0f, "the floats");
	p.has_history = 0u;
	fill_svgf_args(&p, 1u, 1u, 1u, nullptr, 1.0f, a);
	expect(a.has_history == 0u && a.half_w == 0.0f, "no camera without history");
	expect(b3(0) == 0.375f && b3(-1) == 0.25f && b3(1) == 0.25f && b3(2) == 0.0625f && b3(-2) == 0.0625f, "the B3 kernel");
	expect(lum(Px4{1.0f, 1.0f, 1.0f, 0.0f}) == (0.2126f + 0.7152f) + 0.0722f, "lum's order");
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

size_t compare(const std::vector<Px4> &got, const std::vector<Px4> &want)
{
	size_t bad = 0;
	for (size_t i = 0; i < got.size(); i++)
		bad += !same(got[i].x, want[i].x) + !same(got[i].y, want[i].y) + !same(got[i].z, want[i].z) + !same(got[i].w, want[i].w);
	return bad;
}

int recorded(const char *path)
{
	Reader r{std::fopen(path, "rb")};
	if (!r.f) { std::printf("FAIL cannot open %s\n", path); return 1; }
	const float white = mrt::hable_partial(11.2f);
	const uint32_t n_cases = r.u32();
	for (uint32_t c = 0; c < n_cases && r.ok; c++) {
		const auto pb = r.array<unsigned char>(sizeof(mrt_svgf_params));
		const auto cb = r.array<unsigned char>(sizeof(mrt_camera));
		mrt_svgf_params p;
		mrt_camera cam;
		std::memcpy(&p, pb.data(), sizeof(p));
		std::memcpy(&cam, cb.data(), sizeof(cam));
		const uint32_t w = r.u32(), h = r.u32();
		const size_t n = (size_t)w * h;
		const auto illum = r.array<Px4>(n), albedo = r.array<Px4>(n), nd = r.array<Px4>(n), pos = r.array<Px4>(n);
		const auto p_illum = r.array<Px4>(n), p_mom = r.array<Px4>(n), p_nd = r.array<Px4>(n), p_pos = r.array<Px4>(n);
		const auto want_t = r.array<Px4>(n), want_m = r.array<Px4>(n), want_v = r.array<Px4>(n);
		std::vector<std::vector<Px4>> want_a;
		for (int k = 0; k < 5; k++) want_a.push_back(r.array<Px4>(n));
		const auto want_rgba = r.array<Px4>(n);
		const auto want_rgba8 = r.array<uint32_t>(n);
		if (!r.ok) break;
		const std::string what = "case " + std::to_string(c) + " (" + std::to_string(w) + " x " + std::to_string(h) + "): ";
		SvgfArgs a;
		fill_svgf_args(&p, w, h, 1u, &cam, white, a);
		std::vector<Px4> t(n), m(n), v(n), cur(n), next(n), rgba(n);
		const Images prev = {p_illum.data(), p_mom.data(), p_nd.data(), p_pos.data(), w, h};
		for (size_t i = 0; i < n; i++) temporal_pixel(a, prev, illum[i], nd[i], pos[i], t[i], m[i]);
		size_t bad;
		expect((bad = compare(t, want_t)) == 0, what + std::to_string(bad) + " temporal illum words differ");
		expect((bad = compare(m, want_m)) == 0, what + std::to_string(bad) + " moments words differ");
		const Images vin = {t.data(), m.data(), nd.data(), pos.data(), w, h};
		for (uint32_t y = 0; y < h; y++)
			for (uint32_t x = 0; x < w; x++) v[(size_t)y * w + x] = variance_pixel(a, vin, x, y);
		expect((bad = compare(v, want_v)) == 0, what + std::to_string(bad) + " variance words differ");
		cur = v;
		for (int k = 0; k < 5; k++) {
			a.step = 1 << k;
			const Images ain = {cur.data(), nullptr, nd.data(), pos.data(), w, h};
			for (uint32_t y = 0; y < h; y++)
				for (uint32_t x = 0; x < w; x++) next[(size_t)y * w + x] = atrous_pixel(a, ain, x, y);
			expect((bad = compare(next, want_a[k])) == 0, what + std::to_string(bad) + " a-trous words differ at step " + std::to_string(a.step));
			cur.swap(next);
		}
		bad = 0;
		for (size_t i = 0; i < n; i++) {
			rgba[i] = modulate_pixel(a, cur[i], albedo[i]);
			const uint32_t b = mrt::to_rgba8(rgba[i].x) | (mrt::to_rgba8(rgba[i].y) << 8) | (mrt::to_rgba8(rgba[i].z) << 16) | (mrt::to_rgba8(rgba[i].w) << 24);
			bad += b != want_rgba8[i];
		}
		expect(bad == 0, what + std::to_string(bad) + " pixels' bytes differ");
		expect((bad = compare(rgba, want_rgba)) == 0, what + std::to_string(bad) + " modulate words differ");
	}
	// the guides
	const uint32_t n_g = r.u32();
	const auto rays = r.array<mrt_ray32>(n_g); const auto hits = r.array<mrt_hit32>(n_g); const auto rows = r.array<mrt_surface64>(n_g);
	const auto rad = r.array<Px4>(n_g);
	const auto wi = r.array<Px4>(n_g), wa = r.array<Px4>(n_g), wn = r.array<Px4>(n_g), wp = r.array<Px4>(n_g);
	std::vector<Px4> gi(n_g), ga(n_g), gn(n_g), gp(n_g);
	for (uint32_t i = 0; i < n_g && r.ok; i++) guides_pixel(rays[i], hits[i], rows[i], rad[i], gi[i], ga[i], gn[i], gp[i]);
	const size_t bad = r.ok ? compare(gi, wi) + compare(ga, wa) + compare(gn, wn) + compare(gp, wp) : 1;
	expect(r.ok && bad == 0, "guides: " + std::to_string(bad) + " words differ");
	expect(r.ok && std::fgetc(r.f) == EOF, "the file is read to its end");
	std::fclose(r.f);
	std::printf("recorded: %u cases, %u guide records\n", n_cases, n_g);
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
