// gbuffer_data_test.cpp -- host/gbuffer_data.cpp and gbuffer.h without a device: every refusal of mrt_cast_gbuffer_reflections and
// mrt_reflection_image and their order (a call with everything wrong is mended one argument at a time, and the reason must move down
// the header's list), and the kernels' argument.  Given a file (tests/test_gbuffer_cpu.py writes it from
// messyerraytracer_amd/gbuffer.py: little-endian, in the order read below), the host definitions are held bit for bit to the numpy
// restatement: the ray of every texel of the file (traced or not, origin, direction) and its image pixel without and with a lit colour.
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../gbuffer.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace {

using namespace mrt::gb;

int n_checks = 0, n_fail = 0;

void expect(bool ok, const std::string &what)
{
	n_checks++;
	if (!ok) { n_fail++; if (n_fail <= 40) std::printf("FAIL %s\n", what.c_str()); }
}

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
bool has(const char *s, const char *word) { return s && std::string(s).find(word) != std::string::npos; }
bool same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || bits(a) == bits(b); }

float *const A = reinterpret_cast<float *>(16); // never dereferenced
float *const B = reinterpret_cast<float *>(4096);
void *const O = reinterpret_cast<void *>(12288);
void *const O2 = reinterpret_cast<void *>(16384);

mrt_gbuffer defaults()
{
	mrt_gbuffer g;
	std::memset(&g, 0, sizeof(g));
	g.struct_size = (uint32_t)sizeof(g); g.normal_kind = MRT_NORMAL_OCTAHEDRAL;
	for (int k = 0; k < 4; k++) g.inv_projection[5 * k] = g.inv_view[5 * k] = 1.0f;
	g.roughness_threshold = 0.3f; g.max_distance = 25.0f;
	g.d_depth = A; g.d_normal_roughness = B;
	return g;
}

void refusals()
{
	expect(sizeof(mrt_gbuffer) == 160, "mrt_gbuffer is 160 bytes");
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	const uint32_t BIG = 0xffffffffu;
	for (int call = 0; call < 2; call++) { // 0: the cast (its flags are checked in cast.hip), 1: the image
		const std::string c = call ? "image: " : "cast: ";
		mrt_gbuffer bad = defaults();
		bad.d_depth = nullptr; bad.d_normal_roughness = nullptr; bad.struct_size = 159u; bad.normal_kind = 2u;
		bad.inv_projection[7] = nan; bad.inv_view[15] = inf; bad.roughness_threshold = 0.0f; bad.max_distance = -1.0f;
		const void *hits = nullptr, *out = nullptr;
		uint32_t flags = call ? 2u : 0u;
		auto why = [&](const mrt_gbuffer *g, uint32_t w = BIG, uint32_t h = BIG) {
			return call ? image_invalid(g, w, h, hits, out, flags) : cast_invalid(g, w, h, out);
		};
		expect(has(why(nullptr), "null descriptor"), c + "null descriptor first");
		if (call) {
			expect(has(why(&bad), "null d_hits"), c + "d_hits");
			hits = O;
			expect(has(why(&bad), "null d_reflection"), c + "d_reflection");
			out = O2;
			expect(has(why(&bad), "unknown flag"), c + "flags");
			flags = MRT_FLAG_ASYNC | MRT_FLAG_COHERENT;
			expect(has(why(&bad), "unknown flag"), c + "ASYNC with another flag");
			flags = MRT_FLAG_ASYNC;
		}
		expect(has(why(&bad), "null d_depth"), c + "d_depth");
		bad.d_depth = A;
		expect(has(why(&bad), "null d_normal_roughness"), c + "d_normal_roughness");
		bad.d_normal_roughness = B;
		if (!call) { expect(has(why(&bad), "null d_out_hits"), c + "d_out_hits"); out = O; }
		expect(has(why(&bad), "struct_size"), c + "struct_size");
		bad.struct_size = 160u;
		expect(has(why(&bad), "normal_kind"), c + "normal_kind");
		bad.normal_kind = MRT_NORMAL_WORLD;
		expect(has(why(&bad), "non-finite inv_projection"), c + "a NaN inv_projection");
		bad.inv_projection[7] = 0.0f;
		expect(has(why(&bad), "non-finite inv_view"), c + "an infinite inv_view");
		bad.inv_view[15] = 1.0f;
		expect(has(why(&bad), "roughness_threshold"), c + "a zero roughness_threshold");
		for (float t : {nan, inf, -0.3f}) { bad.roughness_threshold = t; expect(has(why(&bad), "roughness_threshold"), c + "roughness_threshold"); }
		bad.roughness_threshold = 0.3f;
		expect(has(why(&bad), "max_distance"), c + "a negative max_distance");
		for (float t : {nan, inf, 0.0f}) { bad.max_distance = t; expect(has(why(&bad), "max_distance"), c + "max_distance"); }
		bad.max_distance = 1e30f;
		expect(has(why(&bad), "overflows"), c + "W * H * 32");
		expect(why(&bad, 7u, 5u) == nullptr, c + "a good call refused");
		expect(why(&bad, 0u, BIG) == nullptr && why(&bad, BIG, 0u) == nullptr, c + "an empty frame refused");
		expect(why(&bad, 0x08000000u, 0x10u) == nullptr, c + "2^31 pixels refused");
		expect(has(why(&bad, 0x80000000u, 0x10000000u), "overflows"), c + "2^59 pixels accepted");
		for (float &m : bad.inv_projection) { const float keep = m; m = -inf; expect(has(why(&bad, 7u, 5u), "inv_projection"), c + "an infinite matrix entry"); m = keep; }
		for (float &m : bad.inv_view) { const float keep = m; m = nan; expect(has(why(&bad, 7u, 5u), "inv_view"), c + "a NaN matrix entry"); m = keep; }
	}
}

void arguments()
{
	mrt_gbuffer g = defaults();
	for (int k = 0; k < 16; k++) { g.inv_projection[k] = (float)(k + 1); g.inv_view[k] = (float)(101 + k); }
	mrt::GBufferParams s;
	fill_params(&g, 67u, 35u, O, s);
	bool ok = s.depth == A && s.guide == B && s.out_rays == O && s.w == 67u && s.h == 35u && s.normal_kind == g.normal_kind &&
			s.roughness_threshold == 0.3f && s.max_distance == 25.0f;
	for (int k = 0; k < 16; k++) ok = ok && s.inv_projection[k] == (float)(k + 1) && s.inv_view[k] == (float)(101 + k);
	expect(ok, "the kernels' argument");
	expect(sky(1.0f) && sky(2.0f) && sky(NAN) && !sky(0.99999994f) && !sky(0.0f) && !sky(-1.0f), "the sky test");
	expect(finite(0.0f) && finite(-3.4e38f) && !finite(NAN) && !finite(std::numeric_limits<float>::infinity()), "finite");
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

// One texel of the file: a whole call's worth of inputs, so that every texel can have its own matrices and frame.
struct Texel {
	uint32_t kind, w, h, x, y;
	float threshold, depth;
	float g[4], P[16], V[16];
	int32_t prim_id;
	float hn[3], lit[4];
};
struct Want { uint32_t traced; float org[3], dir[3], grey[4], lit[4]; };

int recorded(const char *path)
{
	Reader r{std::fopen(path, "rb")};
	if (!r.f) { std::printf("FAIL cannot open %s\n", path); return 1; }
	const uint32_t n = r.u32();
	const auto in = r.array<Texel>(n);
	const auto want = r.array<Want>(n);
	expect(r.ok && std::fgetc(r.f) == EOF, "the file is read to its end");
	std::fclose(r.f);
	if (!r.ok) return 1;
	size_t bad_traced = 0, bad_ray = 0, bad_grey = 0, bad_lit = 0, n_traced = 0;
	for (uint32_t i = 0; i < n; i++) {
		const Texel &t = in[i];
		const Want &w = want[i];
		const Px4 g{t.g[0], t.g[1], t.g[2], t.g[3]};
		float org[3] = {0.0f, 0.0f, 0.0f}, dir[3] = {0.0f, 0.0f, 0.0f};
		const bool traced = reflection_ray(t.kind, t.P, t.V, t.threshold, t.x, t.y, t.w, t.h, t.depth, g, org, dir);
		bad_traced += traced != (w.traced != 0u);
		if (traced && w.traced) {
			n_traced++;
			for (int k = 0; k < 3; k++) bad_ray += !same(org[k], w.org[k]) + !same(dir[k], w.dir[k]);
		}
		const Px4 lit{t.lit[0], t.lit[1], t.lit[2], t.lit[3]};
		const Px4 a = image_pixel(t.kind, t.P, t.V, t.threshold, t.x, t.y, t.w, t.h, t.depth, g, t.prim_id, t.hn[0], t.hn[1], t.hn[2], false, lit);
		const Px4 b = image_pixel(t.kind, t.P, t.V, t.threshold, t.x, t.y, t.w, t.h, t.depth, g, t.prim_id, t.hn[0], t.hn[1], t.hn[2], true, lit);
		bad_grey += !same(a.x, w.grey[0]) + !same(a.y, w.grey[1]) + !same(a.z, w.grey[2]) + !same(a.w, w.grey[3]);
		bad_lit += !same(b.x, w.lit[0]) + !same(b.y, w.lit[1]) + !same(b.z, w.lit[2]) + !same(b.w, w.lit[3]);
	}
	expect(bad_traced == 0, std::to_string(bad_traced) + " texels differ from the restatement in whether they have a ray");
	expect(bad_ray == 0, std::to_string(bad_ray) + " ray words differ from the restatement");
	expect(bad_grey == 0, std::to_string(bad_grey) + " image words differ from the restatement");
	expect(bad_lit == 0, std::to_string(bad_lit) + " lit image words differ from the restatement");
	std::printf("recorded: %u texels, %zu with a ray\n", n, n_traced);
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
