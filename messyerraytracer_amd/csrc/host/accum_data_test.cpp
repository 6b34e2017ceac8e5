// accum_data_test.cpp -- host/accum_data.cpp and accum.h without a device: every refusal of the four calls and their order, the Halton
// pair on values worked out by hand, the frame policy (mrt_accum_begin_frame, mrt_accum_end_frame) over scripted frame sequences with
// the expectations written out -- AA off then on, a move mid-sequence, a rotation alone, a resolution change at end of frame,
// max_samples 0, 1 and 3 reached and passed, a NaN pose -- and the running mean's step on exact cases.
// Given a file (tests/test_accumulate_cpu.py writes it from tests/golden/accumulate_reference.npz: counts and arrays, little-endian, in
// the order read below), the same calls are held bit for bit to what the reference's own text recorded: every Halton pair, every motion
// decision, every scripted frame and every running mean with its bytes.
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../accum.h"

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
	if (!ok) { n_fail++; if (n_fail <= 40) std::printf("FAIL %s\n", what.c_str()); }
}

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
bool has(const char *s, const char *word) { return s && std::string(s).find(word) != std::string::npos; }
bool same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || bits(a) == bits(b); }

void *const P = reinterpret_cast<void *>(16); // never dereferenced
void *const Q = reinterpret_cast<void *>(4096);
const float I3[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };

mrt_accum_state fresh(uint32_t aa, int32_t max_samples)
{
	mrt_accum_state st;
	std::memset(&st, 0, sizeof(st));
	st.struct_size = (uint32_t)sizeof(st); st.aa_enabled = aa; st.max_samples = max_samples;
	return st;
}

const char *check(uint32_t kind, const void *src, uint64_t count, uint32_t mode, uint32_t n_prior, const void *acc, uint32_t flags)
{
	return mrt::accumulate_invalid(kind, src, count, mode, n_prior, acc, flags);
}

void refusals()
{
	expect(sizeof(mrt_accum_state) == 96, "mrt_accum_state is 96 bytes");
	// mrt_halton_jitter
	float j[2] = { -1.0f, -1.0f };
	expect(mrt_halton_jitter(0u, nullptr) == MRT_ERR_INVALID, "halton: a null pointer accepted");
	expect(mrt_halton_jitter(0x7fffffffu, j) == MRT_ERR_INVALID && mrt_halton_jitter(0xffffffffu, j) == MRT_ERR_INVALID && j[0] == -1.0f && j[1] == -1.0f,
			"halton: an index above 0x7ffffffe accepted or written");
	expect(mrt_halton_jitter(0x7fffffffu, nullptr) == MRT_ERR_INVALID, "halton: null and a bad index");
	expect(mrt_halton_jitter(0x7ffffffeu, j) == MRT_OK, "halton: 0x7ffffffe refused");
	// the two frame calls
	mrt_accum_state st = fresh(1u, 4);
	const float o[3] = { 0, 0, 0 };
	expect(mrt_accum_begin_frame(nullptr, o, I3) == MRT_ERR_INVALID && mrt_accum_begin_frame(&st, nullptr, I3) == MRT_ERR_INVALID
			&& mrt_accum_begin_frame(&st, o, nullptr) == MRT_ERR_INVALID, "begin_frame: a null pointer accepted");
	expect(mrt_accum_end_frame(nullptr, 4u) == MRT_ERR_INVALID, "end_frame: a null state accepted");
	for (uint32_t sz : { 0u, 92u, 95u, 97u, 104u, 0xFFFFFFFFu }) {
		mrt_accum_state bad = fresh(1u, 4); bad.struct_size = sz; bad.count = 2u;
		mrt_accum_state keep = bad;
		expect(mrt_accum_begin_frame(&bad, o, I3) == MRT_ERR_INVALID && mrt_accum_end_frame(&bad, 4u) == MRT_ERR_INVALID && !std::memcmp(&bad, &keep, sizeof(bad)),
				"struct_size " + std::to_string(sz) + " accepted, or the state written");
	}
	st.reserved = 0xFFFFFFFFu;
	expect(mrt_accum_begin_frame(&st, o, I3) == MRT_OK && mrt_accum_end_frame(&st, 4u) == MRT_OK && st.reserved == 0xFFFFFFFFu, "the reserved word looked at or written");
	// mrt_accumulate: pointer, flag, kind, mode, n_prior, aliasing, count
	expect(check(0u, P, 1u, 0u, 0u, Q, 0u) == nullptr && check(2u, P, 1u, 4u, 0x7ffffffeu, Q, MRT_FLAG_ASYNC) == nullptr, "a good call refused");
	expect(has(check(0u, nullptr, 1u, 0u, 0u, Q, 0u), "null") && has(check(0u, P, 1u, 0u, 0u, nullptr, 0u), "null"), "a null source or accumulator accepted");
	for (uint32_t bit = 0; bit < 32u; bit++) {
		const uint32_t f = 1u << bit;
		expect((check(0u, P, 1u, 0u, 0u, Q, f) != nullptr) == (f != MRT_FLAG_ASYNC), "flag bit " + std::to_string(bit));
	}
	for (uint32_t k = 0; k < 3u; k++) expect(check(k, P, 1u, 0u, 0u, Q, 0u) == nullptr, "source_kind " + std::to_string(k) + " refused");
	for (uint32_t k : { 3u, 4u, 255u, 0x80000000u, 0xFFFFFFFFu }) expect(has(check(k, P, 1u, 0u, 0u, Q, 0u), "source_kind"), "source_kind " + std::to_string(k) + " accepted");
	for (uint32_t k = 1; k < 3u; k++) {
		for (uint32_t m = 0; m <= 4u; m++) expect(check(k, P, 1u, m, 0u, Q, 0u) == nullptr, "tone map mode " + std::to_string(m) + " refused");
		expect(has(check(k, P, 1u, 5u, 0u, Q, 0u), "tonemap") && has(check(k, P, 1u, 0xFFFFFFFFu, 0u, Q, 0u), "tonemap"), "tone map mode > 4 accepted");
	}
	expect(check(0u, P, 1u, 5u, 0u, Q, 0u) == nullptr && check(0u, P, 1u, 0xFFFFFFFFu, 0u, Q, 0u) == nullptr, "RGBA: the tone map mode looked at");
	expect(has(check(0u, P, 1u, 0u, 0x7fffffffu, Q, 0u), "n_prior") && has(check(0u, P, 1u, 0u, 0xFFFFFFFFu, Q, 0u), "n_prior"), "n_prior above 0x7ffffffe accepted");
	expect(has(check(0u, P, 1u, 0u, 0u, P, 0u), "d_source"), "d_accum == d_source accepted");
	expect(check(0u, P, 0x07FFFFFFFFFFFFFFull, 0u, 0u, Q, 0u) == nullptr, "the largest count refused");
	expect(has(check(0u, P, 0x0800000000000000ull, 0u, 0u, Q, 0u), "overflow") && has(check(0u, P, ~0ull, 0u, 0u, Q, 0u), "overflow"), "count * 32 overflowing accepted");
	expect(check(0u, P, 0u, 0u, 0u, Q, 0u) == nullptr, "count 0 refused");
	// the order
	expect(has(check(9u, nullptr, ~0ull, 9u, 0xFFFFFFFFu, nullptr, 1u << 20), "null"), "order: pointers first");
	expect(has(check(9u, P, ~0ull, 9u, 0xFFFFFFFFu, P, 1u << 20), "flag"), "order: flags second");
	expect(has(check(9u, P, ~0ull, 9u, 0xFFFFFFFFu, P, 0u), "source_kind"), "order: the kind third");
	expect(has(check(1u, P, ~0ull, 9u, 0xFFFFFFFFu, P, 0u), "tonemap"), "order: the mode fourth");
	expect(has(check(1u, P, ~0ull, 4u, 0xFFFFFFFFu, P, 0u), "n_prior"), "order: n_prior fifth");
	expect(has(check(1u, P, ~0ull, 4u, 7u, P, 0u), "d_source"), "order: aliasing sixth");
	expect(has(check(1u, P, ~0ull, 4u, 7u, Q, 0u), "overflow"), "order: the count last");
	expect(check(1u, P, 77u, 4u, 7u, Q, 0u) == nullptr, "the mended call refused");
}

void halton_by_hand()
{
	// index + 1 = 1, 2, 3, 4, 5, 6: base 2 is 1/2, 1/4, 3/4, 1/8, 5/8, 3/8 exactly; base 3 is 1/3, 2/3, 1/9, 4/9, 7/9, 2/9 as the loop rounds them
	const float want2[6] = { 0.5f, 0.25f, 0.75f, 0.125f, 0.625f, 0.375f };
	const float t = 1.0f / 3.0f, n = t * t;
	const float want3[6] = { 0.0f + t * 1.0f, 0.0f + t * 2.0f, (0.0f + t * 0.0f) + n * 1.0f, (0.0f + t * 1.0f) + n * 1.0f, (0.0f + t * 2.0f) + n * 1.0f, (0.0f + t * 0.0f) + n * 2.0f };
	for (uint32_t k = 0; k < 6u; k++) {
		float j[2];
		expect(mrt_halton_jitter(k, j) == MRT_OK && bits(j[0]) == bits(want2[k]) && bits(j[1]) == bits(want3[k]), "halton pair of index " + std::to_string(k));
	}
	float j[2];
	mrt_halton_jitter(0x7ffffffeu, j); // index + 1 = 2^31 - 1: 31 one bits
	expect(j[0] == 1.0f, "halton2 of 2^31 - 1 rounds to 1"); // 1 - 2^-31 is not a float
	for (uint32_t k = 0; k < 5000u; k++) {
		mrt_halton_jitter(k, j);
		expect(j[0] > 0.0f && j[0] < 1.0f && j[1] > 0.0f && j[1] < 1.0f, "halton pair " + std::to_string(k) + " outside (0, 1)");
	}
}

struct Frame { uint32_t aa; int32_t max_samples; uint64_t pixels; float origin[3]; const float *basis;
	uint32_t sample_index, accumulate, n_prior, count_after; bool jittered; };

void run(const char *name, const std::vector<Frame> &frames)
{
	mrt_accum_state st = fresh(0u, 0);
	int k = 0;
	for (const Frame &f : frames) {
		st.aa_enabled = f.aa; st.max_samples = f.max_samples;
		const std::string at = std::string(name) + ", frame " + std::to_string(k++);
		expect(mrt_accum_begin_frame(&st, f.origin, f.basis) == MRT_OK, at + ": begin_frame");
		float j[2] = { 0.5f, 0.5f };
		if (f.jittered) mrt_halton_jitter(f.sample_index, j);
		expect(st.sample_index == f.sample_index && bits(st.jitter_x) == bits(j[0]) && bits(st.jitter_y) == bits(j[1]), at + ": sample_index / jitter");
		expect(!std::memcmp(st.prev_origin, f.origin, 12) && !std::memcmp(st.prev_basis, f.basis, 36), at + ": the previous pose");
		expect(mrt_accum_end_frame(&st, f.pixels) == MRT_OK, at + ": end_frame");
		expect(st.accumulate == f.accumulate && st.n_prior == f.n_prior && st.count == f.count_after && (!f.accumulate || st.pixels == f.pixels), at + ": accumulate / n_prior / count");
	}
}

void policy()
{
	static const float R[9] = { 0.995004177f, 0, 0.0998334140f, 0, 1, 0, -0.0998334140f, 0, 0.995004177f }; // 0.1 rad about y
	const float nan = std::numeric_limits<float>::quiet_NaN();
	// { aa, max, pixels, origin, basis,   sample_index, accumulate, n_prior, count after, jittered }
	run("AA off, then on", {
		{ 0, 8, 12, { 0, 0, 0 }, I3, 0, 0, 0, 0, false }, { 0, 8, 12, { 0, 0, 0 }, I3, 0, 0, 0, 0, false },
		{ 1, 8, 12, { 0, 0, 0 }, I3, 0, 1, 0, 1, true }, { 1, 8, 12, { 0, 0, 0 }, I3, 1, 1, 1, 2, true }, { 1, 8, 12, { 0, 0, 0 }, I3, 2, 1, 2, 3, true },
		{ 0, 8, 12, { 0, 0, 0 }, I3, 0, 0, 0, 0, false }, { 1, 8, 12, { 0, 0, 0 }, I3, 0, 1, 0, 1, true } });
	run("a move mid-sequence", {
		{ 1, 64, 12, { 1, 1, 1 }, I3, 0, 1, 0, 1, true }, { 1, 64, 12, { 1, 1, 1 }, I3, 1, 1, 1, 2, true }, { 1, 64, 12, { 1, 1, 1 }, I3, 2, 1, 2, 3, true },
		{ 1, 64, 12, { 1, 1.5f, 1 }, I3, 0, 1, 0, 1, true }, { 1, 64, 12, { 1, 1.5f, 1 }, I3, 1, 1, 1, 2, true },
		{ 1, 64, 12, { 1, 1.5f + 4e-5f, 1 }, I3, 2, 1, 2, 3, true } }); // under the threshold
	run("a rotation alone", {
		{ 1, 64, 12, { 0, 2, 0 }, I3, 0, 1, 0, 1, true }, { 1, 64, 12, { 0, 2, 0 }, I3, 1, 1, 1, 2, true },
		{ 1, 64, 12, { 0, 2, 0 }, R, 0, 1, 0, 1, true }, { 1, 64, 12, { 0, 2, 0 }, R, 1, 1, 1, 2, true } });
	run("a resolution change at end of frame", {
		{ 1, 64, 12, { 0, 0, 0 }, I3, 0, 1, 0, 1, true }, { 1, 64, 12, { 0, 0, 0 }, I3, 1, 1, 1, 2, true },
		{ 1, 64, 20, { 0, 0, 0 }, I3, 2, 1, 0, 1, true },   // the frame was jittered as sample 2 and starts the new mean
		{ 1, 64, 20, { 0, 0, 0 }, I3, 1, 1, 1, 2, true } });
	for (int32_t mx : { 0, 1, -5 })
		run("max_samples below 2", {
			{ 1, mx, 12, { 0, 0, 0 }, I3, 0, 1, 0, 1, true }, { 1, mx, 12, { 0, 0, 0 }, I3, 1, 0, 0, 1, false }, { 1, mx, 12, { 0, 0, 0 }, I3, 1, 0, 0, 1, false } });
	run("max_samples 3, reached and passed", {
		{ 1, 3, 12, { 0, 0, 0 }, I3, 0, 1, 0, 1, true }, { 1, 3, 12, { 0, 0, 0 }, I3, 1, 1, 1, 2, true }, { 1, 3, 12, { 0, 0, 0 }, I3, 2, 1, 2, 3, true },
		{ 1, 3, 12, { 0, 0, 0 }, I3, 3, 0, 0, 3, false }, { 1, 3, 12, { 0, 0, 0 }, I3, 3, 0, 0, 3, false },   // the raw, un-jittered frame
		{ 1, 3, 12, { 0, 0, 1 }, I3, 0, 1, 0, 1, true } });                                                   // a move starts again
	run("a NaN pose resets nothing", {
		{ 1, 64, 12, { 1, 2, 3 }, I3, 0, 1, 0, 1, true }, { 1, 64, 12, { 1, 2, 3 }, I3, 1, 1, 1, 2, true },
		{ 1, 64, 12, { 1, nan, 3 }, I3, 2, 1, 2, 3, true }, { 1, 64, 12, { 9, 9, 9 }, I3, 3, 1, 3, 4, true },  // after a NaN pose even a move is not seen
		{ 1, 64, 12, { 1, 2, 3 }, I3, 0, 1, 0, 1, true } });
}

void mean_by_hand()
{
	expect(bits(mrt::accum_inv(1u)) == bits(0.5f) && bits(mrt::accum_inv(2u)) == bits(1.0f / 3.0f) && bits(mrt::accum_inv(4095u)) == bits(1.0f / 4096.0f), "1 / (n + 1)");
	expect(bits(mrt::accum_inv(0x7ffffffeu)) == bits(1.0f / 2147483648.0f), "1 / (n + 1) of the largest n_prior");
	expect(mrt::accum_step(0.0f, 1.0f, 0.5f) == 0.5f && mrt::accum_step(1.0f, 0.0f, 0.25f) == 0.75f && mrt::accum_step(2.0f, 2.0f, 0.5f) == 2.0f, "exact steps");
	const float big = std::numeric_limits<float>::max(), inf = std::numeric_limits<float>::infinity();
	expect(mrt::accum_step(big, -big, 0.5f) == -inf, "the difference of FLT_MAX and -FLT_MAX overflows");
	expect(std::isnan(mrt::accum_step(-inf, big, 0.5f)) && std::isnan(mrt::accum_step(0.0f, std::numeric_limits<float>::quiet_NaN(), 0.5f)), "inf - inf and a NaN sample");
	expect(bits(mrt::accum_step(-0.0f, -0.0f, 0.5f)) == bits(0.0f) && bits(mrt::accum_step(0.0f, -0.0f, 0.5f)) == bits(0.0f), "signed zeros");
	// a step of less than half an ulp leaves the mean where it is; (after n_prior == 0 -0 survives only as the copied first sample)
	expect(bits(mrt::accum_step(1.0f, from_bits(0x3f800001u), 1.0f / 3.0f)) == bits(1.0f), "a step below half an ulp");
}

// ---- the recorded values
template <class T>
bool rd(FILE *f, std::vector<T> &v, size_t n)
{
	v.resize(n);
	return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int recorded(const char *path)
{
	FILE *f = std::fopen(path, "rb");
	if (!f) { std::printf("FAIL cannot open %s\n", path); return 2; }
	std::vector<uint32_t> n, h_idx, m_out, q_in, q_out;
	std::vector<float> h_out, m_in, a_src, a_acc;
	std::vector<uint8_t> a_bytes;
	bool ok = rd(f, n, 1) && rd(f, h_idx, n[0]) && rd(f, h_out, 2 * (size_t)n[0]);
	ok = ok && rd(f, n, 1) && rd(f, m_in, 24 * (size_t)n[0]) && rd(f, m_out, n[0]);
	ok = ok && rd(f, n, 1) && rd(f, q_in, 16 * (size_t)n[0]) && rd(f, q_out, 6 * (size_t)n[0]);
	ok = ok && rd(f, n, 2);
	const size_t n_s = ok ? n[0] : 0, n_v = ok ? n[1] : 0;
	ok = ok && rd(f, a_src, n_s * n_v) && rd(f, a_acc, n_s * n_v) && rd(f, a_bytes, n_s * n_v);
	std::fclose(f);
	if (!ok) { std::printf("FAIL short read of %s\n", path); return 2; }
	// Halton pairs
	for (size_t k = 0; k < h_idx.size(); k++) {
		float j[2];
		expect(mrt_halton_jitter(h_idx[k], j) == MRT_OK && bits(j[0]) == bits(h_out[2 * k]) && bits(j[1]) == bits(h_out[2 * k + 1]), "recorded halton pair " + std::to_string(h_idx[k]));
	}
	// motion decisions: the count was 7 before
	for (size_t k = 0; k < m_out.size(); k++) {
		mrt_accum_state st = fresh(1u, 256);
		const float *p = &m_in[24 * k];
		std::memcpy(st.prev_origin, p, 12); std::memcpy(st.prev_basis, p + 3, 36);
		st.count = 7u;
		expect(mrt_accum_begin_frame(&st, p + 12, p + 15) == MRT_OK && st.count == m_out[k] && st.sample_index == m_out[k], "recorded motion decision " + std::to_string(k));
	}
	// scripted frames
	mrt_accum_state st = fresh(0u, 0);
	uint32_t seq = 0xFFFFFFFFu;
	for (size_t k = 0; k < q_out.size() / 6; k++) {
		const uint32_t *w = &q_in[16 * k], *o = &q_out[6 * k];
		if (w[0] != seq) { st = fresh(0u, 0); seq = w[0]; }
		st.aa_enabled = w[1]; st.max_samples = (int32_t)w[2];
		float pose[12];
		std::memcpy(pose, w + 4, 48);
		const bool began = mrt_accum_begin_frame(&st, pose, pose + 3) == MRT_OK;
		const bool first = st.sample_index == o[0] && bits(st.jitter_x) == o[1] && bits(st.jitter_y) == o[2];
		const bool ended = mrt_accum_end_frame(&st, w[3]) == MRT_OK;
		expect(began && first && ended && st.accumulate == o[3] && st.n_prior == o[4] && st.count == o[5], "recorded frame " + std::to_string(k) + " of sequence " + std::to_string(w[0]));
	}
	// running means and their bytes
	std::vector<float> acc(n_v);
	for (size_t s = 0; s < n_s; s++) {
		const float inv = mrt::accum_inv((uint32_t)s);
		bool means = true, bytes = true;
		for (size_t v = 0; v < n_v; v++) {
			acc[v] = s == 0 ? a_src[v] : mrt::accum_step(acc[v], a_src[s * n_v + v], inv);
			means = means && same(acc[v], a_acc[s * n_v + v]);
			bytes = bytes && mrt::to_rgba8(a_acc[s * n_v + v]) == a_bytes[s * n_v + v] && mrt::to_rgba8(acc[v]) == a_bytes[s * n_v + v];
		}
		expect(means, "recorded means after sample " + std::to_string(s));
		expect(bytes, "recorded bytes after sample " + std::to_string(s));
	}
	std::printf("recorded: %zu halton pairs, %zu motion decisions, %zu frames, %zu x %zu means\n", h_idx.size(), m_out.size(), q_out.size() / 6, n_s, n_v);
	return 0;
}

} // namespace

int main(int argc, char **argv)
{
	refusals();
	halton_by_hand();
	policy();
	mean_by_hand();
	if (argc > 1 && recorded(argv[1])) return 2;
	std::printf("%d checks hold of %d\n", n_checks - n_fail, n_checks);
	return n_fail ? 1 : 0;
}
