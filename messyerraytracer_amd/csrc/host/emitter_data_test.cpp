// emitter_data_test.cpp -- host/emitter_data.cpp and emitters.h without a device.  Per call (build, emitter shadow, emitter light,
// emitter step), array and grid form: every refusal and their order (a call with everything wrong is mended one argument at a time, and
// the reason must move down the header's table), and the kernels' arguments: the jump against stepping the generator, the seed of a row
// band against the whole frame's, the table passed through.  The integer weights: ceil_log2 and the scale at every bound, q0 and q at
// their edges, and for tables of many sizes and weight spreads that every q is at least 1 and the total lies in (2^31 - n, 2^31].
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../emitters.h"
#include "../path.h"
#include "../source_cast.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

using namespace mrt;
using namespace mrt::em;

int n_checks = 0, n_fail = 0;

void expect(bool ok, const std::string &what)
{
	n_checks++;
	if (!ok) { n_fail++; if (n_fail <= 40) std::printf("FAIL %s\n", what.c_str()); }
}

bool has(const char *s, const char *word) { return s && std::string(s).find(word) != std::string::npos; }

void *const R = reinterpret_cast<void *>(16); // never dereferenced
void *const H = reinterpret_cast<void *>(4096);
void *const ROWS = reinterpret_cast<void *>(6144);
uint8_t *const M = reinterpret_cast<uint8_t *>(8192);
uint32_t *const OE = reinterpret_cast<uint32_t *>(12288);
uint8_t *const SEL = reinterpret_cast<uint8_t *>(16384);
float *const OUT = reinterpret_cast<float *>(20480);

void build_refusals()
{
	expect(has(build_invalid(nullptr, 1u, 0u), "null tris"), "build: null tris with triangles");
	expect(build_invalid(nullptr, 0u, 0u) == nullptr, "build: no triangles, no array");
	expect(has(build_invalid(nullptr, 1u, 2u), "null tris"), "build: the pointer before the flag");
	expect(has(build_invalid(R, 1u, 2u), "unknown flag"), "build: an unknown flag");
	expect(has(build_invalid(R, 1u, MRT_BUILD_TRIS_ON_DEVICE | MRT_BUILD_SAFE_HANDOFF), "unknown flag"), "build: a flag of the scene builds");
	expect(build_invalid(R, 1u, MRT_BUILD_TRIS_ON_DEVICE) == nullptr && build_invalid(R, 0xFFFFFFFFu, 0u) == nullptr, "build: valid calls");
}

void shadow_refusals()
{
	expect(sizeof(mrt_emitter_select) == 24 && sizeof(mrt_emitter64) == 64, "the structs' sizes");
	for (int grid = 0; grid < 2; grid++) {
		const std::string c = grid ? "shadow, grid: " : "shadow, array: ";
		mrt_emitter_select d;
		std::memset(&d, 0, sizeof(d));
		d.frame = MRT_PATH_MAX_FRAME + 1u;
		const void *rays = nullptr, *hits = nullptr;
		const mrt_emitter_select *desc = nullptr;
		const uint8_t *mask = nullptr;
		uint32_t flags = MRT_FLAG_COHERENT;
		auto why = [&] { return shadow_invalid(!grid, rays, hits, desc, mask, flags); };
		expect(has(why(), "null rays"), c + "rays first");
		rays = R;
		expect(has(why(), "null hits"), c + "hits");
		hits = H;
		expect(has(why(), "null descriptor"), c + "descriptor");
		desc = &d;
		expect(has(why(), "null mask"), c + "mask");
		mask = M;
		expect(has(why(), "null d_out_emitter"), c + "d_out_emitter");
		d.d_out_emitter = OE;
		expect(has(why(), "unknown flag"), c + "flags");
		flags = MRT_FLAG_ASYNC | MRT_FLAG_HOST_LAYOUT;
		expect(grid ? has(why(), "unknown flag") : has(why(), "MRT_PATH_MAX_FRAME"), c + "HOST_LAYOUT is the array form's flag alone");
		flags = MRT_FLAG_ASYNC;
		expect(has(why(), "MRT_PATH_MAX_FRAME"), c + "frame");
		d.frame = MRT_PATH_MAX_FRAME;
		expect(why() == nullptr, c + "a valid call");
		d.d_select = SEL;
		expect(why() == nullptr, c + "d_select is optional");
		d.draw = 0xFFFFFFFFu;
		expect(why() == nullptr, c + "any draw");
	}
}

void light_refusals()
{
	for (int grid = 0; grid < 2; grid++) {
		const std::string c = grid ? "light, grid: " : "light, array: ";
		mrt_emitter_select d;
		std::memset(&d, 0, sizeof(d));
		d.frame = MRT_PATH_MAX_FRAME + 1u;
		mrt_light_out o;
		o.d_rgba = nullptr;
		const void *rays = nullptr, *hits = nullptr, *rows = nullptr;
		const mrt_emitter_select *desc = nullptr;
		const mrt_light_out *out = nullptr;
		uint32_t flags = MRT_FLAG_BOOL_OUT, acc = 2u;
		auto why = [&] { return light_invalid(!grid, rays, hits, rows, desc, acc, out, flags); };
		expect(has(why(), "null rays"), c + "rays first");
		rays = R;
		expect(has(why(), "null hits"), c + "hits");
		hits = H;
		expect(has(why(), "null rows"), c + "rows");
		rows = ROWS;
		expect(has(why(), "null descriptor"), c + "descriptor");
		desc = &d;
		expect(has(why(), "null d_out_emitter"), c + "d_out_emitter");
		d.d_out_emitter = OE;
		expect(has(why(), "null output"), c + "output");
		out = &o;
		expect(has(why(), "null output"), c + "the output's plane");
		o.d_rgba = OUT;
		expect(has(why(), "unknown flag"), c + "flags");
		flags = MRT_FLAG_ASYNC | MRT_FLAG_HOST_LAYOUT;
		expect(grid ? has(why(), "unknown flag") : has(why(), "accumulate"), c + "HOST_LAYOUT is the array form's flag alone");
		flags = 0u;
		expect(has(why(), "accumulate"), c + "accumulate");
		acc = MRT_EMITTER_ACCUMULATE;
		expect(has(why(), "MRT_PATH_MAX_FRAME"), c + "frame");
		d.frame = 0u;
		expect(why() == nullptr, c + "a valid call");
		acc = 0u;
		expect(why() == nullptr, c + "written, not accumulated");
	}
}

void step_refusals()
{
	mrt_path_step_desc d;
	std::memset(&d, 0, sizeof(d));
	d.max_bounces = 4u;
	expect(step_invalid(&d, nullptr) == nullptr, "step: bounce 0 takes no lobe bytes");
	expect(step_invalid(&d, SEL) == nullptr, "step: bounce 0 may be given them");
	for (uint32_t b = 1u; b <= 4u; b++) {
		d.bounce = b;
		expect(has(step_invalid(&d, nullptr), "d_prev_lobe"), "step: bounce " + std::to_string(b) + " needs the lobe bytes");
		expect(step_invalid(&d, SEL) == nullptr, "step: bounce " + std::to_string(b) + " with them");
	}
	// after mrt_path_step's own refusals: a descriptor that path_step_invalid refuses is refused by it, whatever the lobe bytes
	mrt_environment env;
	std::memset(&env, 0, sizeof(env));
	d.d_direct = OUT; d.d_state = reinterpret_cast<mrt_path_state *>(H); d.env = &env; d.d_out_select = M;
	d.bounce = 5u;
	expect(path_step_invalid(R, H, ROWS, &d, 0u, MRT_FLAG_ASYNC) != nullptr, "step: bounce > max_bounces is mrt_path_step's refusal");
	d.bounce = 4u;
	expect(path_step_invalid(R, H, ROWS, &d, 0u, MRT_FLAG_ASYNC) == nullptr, "step: a descriptor mrt_path_step takes");
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
	expect(MRT_PATH_EMITTER_DRAW(0u) == 512u && MRT_PATH_EMITTER_DRAW(32u) == 640u, "MRT_PATH_EMITTER_DRAW");
	expect(MRT_PATH_SELECT_DRAW(MRT_PATH_MAX_BOUNCES) < MRT_PATH_EMITTER_DRAW(0u), "clear of the light-selecting draws");
	expect(MRT_PATH_EMITTER_DRAW(1u) - MRT_PATH_EMITTER_DRAW(0u) >= 3u, "three draws per bounce");
	const EmitterTable table = {ROWS, reinterpret_cast<const uint32_t *>(H), 77u, 2147483000u};
	for (uint32_t draw : {0u, 1u, 512u, 516u, 640u, 100000u}) {
		for (uint32_t frame : {0u, 7u, (uint32_t)MRT_PATH_MAX_FRAME}) {
			for (uint32_t pixel0 : {0u, 5u * 100u, 4000000u * 1080u}) {
				mrt_emitter_select d;
				std::memset(&d, 0, sizeof(d));
				d.frame = frame; d.draw = draw; d.d_select = SEL; d.d_out_emitter = OE;
				EmitterShadowParams s;
				std::memset(&s, 0xAB, sizeof(s));
				fill_shadow(H, &d, table, pixel0, s);
				mrt_light_out o;
				o.d_rgba = OUT;
				EmitterLightParams l;
				std::memset(&l, 0xAB, sizeof(l));
				fill_light(H, ROWS, &d, M, MRT_EMITTER_ACCUMULATE, &o, table, pixel0, l);
				const std::string c = "draw " + std::to_string(draw) + " frame " + std::to_string(frame) + " pixel0 " + std::to_string(pixel0) + ": ";
				expect(s.records == H && s.select == SEL && s.out_emitter == OE, c + "the cast's pointers");
				expect(s.table.rows == ROWS && s.table.cdf == table.cdf && s.table.n == 77u && s.table.total == 2147483000u, c + "the cast's table");
				expect(l.records == H && l.rows == ROWS && l.emitter == OE && l.mask == M && l.out == OUT && l.accumulate == 1u, c + "the light call's pointers");
				expect(l.table.rows == ROWS && l.table.n == 77u && l.table.total == 2147483000u, c + "the light call's table");
				expect(l.seed_add == s.seed_add && l.jump.a == s.jump.a && l.jump.c == s.jump.c, c + "the light call draws what the cast drew");
				for (uint32_t i : {0u, 1u, 63u, 99u, 2399u}) {
					// the kernel's seed of record i of the band is the whole frame's seed of pixel pixel0 + i
					const uint32_t seed = (pixel0 + i) * 1009u + frame * 6529u + 7u;
					expect(i * 1009u + s.seed_add == seed, c + "seed of record " + std::to_string(i));
					const uint32_t state0 = (kPcgInc + seed) * kPcgMul + kPcgInc;
					expect(s.jump.a * state0 + s.jump.c == stepped_state(seed, draw), c + "the jump reaches the stepped state, record " + std::to_string(i));
				}
			}
		}
	}
}

void weights()
{
	expect(ceil_log2(1u) == 0u && ceil_log2(2u) == 1u && ceil_log2(3u) == 2u && ceil_log2(4u) == 2u && ceil_log2(5u) == 3u, "ceil_log2 of small counts");
	expect(ceil_log2(MRT_MAX_EMITTERS) == 20u && ceil_log2(MRT_MAX_EMITTERS - 1u) == 20u && ceil_log2((MRT_MAX_EMITTERS >> 1) + 1u) == 20u &&
			ceil_log2(MRT_MAX_EMITTERS >> 1) == 19u, "ceil_log2 at the largest table");
	expect(weight_scale(1u) == 2147483648.0f && weight_scale(2u) == 1073741824.0f && weight_scale(3u) == 536870912.0f &&
			weight_scale(MRT_MAX_EMITTERS) == 2048.0f, "Q = 2^(31 - ceil_log2(n))");
	expect(first_weight(1.0f, 1.0f, weight_scale(1u)) == 2147483648u, "q0 of the only emitter is 2^31");
	expect(first_weight(1e-30f, 1.0f, 2048.0f) == 1u && first_weight(1.0f, 1.0f, 2048.0f) == 2048u && first_weight(0.5f, 1.0f, 2048.0f) == 1024u,
			"q0: at least 1, the largest is Q");
	expect(final_weight(2147483648u, 2147483648ull) == 2147483648u && final_weight(1u, 2147483648ull) == 1u && final_weight(1u, 3ull) == 715827882u,
			"q = (q0 << 31) / T0");
	// tables of many sizes and spreads: q >= 1, total in (2^31 - n, 2^31], the CDF strictly increasing
	uint32_t rng = 12345u;
	auto next = [&] { rng = rng * kPcgMul + kPcgInc; return (float)(rng >> 8) * (1.0f / 16777216.0f); };
	for (uint32_t n : {1u, 2u, 3u, 5u, 64u, 257u, 1000u, 4097u, 1u << 17, (uint32_t)MRT_MAX_EMITTERS}) {
		for (float spread : {0.0f, 1.0f, 20.0f, 60.0f}) {
			std::vector<float> w(n);
			float w_max = 0.0f;
			for (uint32_t k = 0; k < n; k++) { w[k] = std::ldexp(0.5f + 0.5f * next(), -(int)(spread * next())); w_max = w[k] > w_max ? w[k] : w_max; }
			const float Q = weight_scale(n);
			std::vector<uint32_t> q0(n);
			uint64_t t0 = 0u;
			for (uint32_t k = 0; k < n; k++) { q0[k] = first_weight(w[k], w_max, Q); t0 += q0[k]; }
			uint64_t total = 0u;
			bool ok = t0 <= (1ull << 31);
			for (uint32_t k = 0; k < n; k++) { const uint32_t q = final_weight(q0[k], t0); ok = ok && q >= 1u; total += q; }
			expect(ok && total > (1ull << 31) - n && total <= (1ull << 31), "n = " + std::to_string(n) + ", spread 2^" + std::to_string((int)spread) +
					": total " + std::to_string(total));
		}
	}
}

} // namespace

int main()
{
	build_refusals();
	shadow_refusals();
	light_refusals();
	step_refusals();
	params();
	weights();
	std::printf("%d of %d checks hold \n", n_checks - n_fail, n_checks);
	return n_fail ? 1 : 0;
}
