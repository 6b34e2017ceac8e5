// channel_data_test.cpp -- host/channel_data.cpp and channels.h without a device: every refusal of the channel and image calls and
// their order (each required pointer null in turn, all 32 flag bits, each range NaN and +-inf, each of the 2 x 11 output entries
// alone, COLOR refused), the selection mask word of a dozen descriptors, the kernel's copy of a descriptor, to_rgba8 on values worked
// out by hand, and Hable's white value against what mrt_path_finish passes.
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../channels.h"

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

void *const P = reinterpret_cast<void *>(16); // never dereferenced
float *const PF = reinterpret_cast<float *>(P);
uint8_t *const PB = reinterpret_cast<uint8_t *>(P);

mrt_channel_out descriptor()
{
	mrt_channel_out d;
	std::memset(&d, 0, sizeof(d));
	d.struct_size = (uint32_t)sizeof(d);
	d.inv_depth_range = 0.25f; d.inv_pos_range = 2.0f;
	return d;
}

const uint32_t KNOWN = MRT_FLAG_HOST_LAYOUT | MRT_FLAG_ASYNC;
const char *check(const mrt_channel_out &d, uint32_t flags = 0u) { return mrt::channel_out_invalid(P, P, &d, flags, KNOWN); }

void refusals()
{
	mrt_channel_out good = descriptor();
	good.d_rgba[MRT_CHANNEL_NORMAL] = PF;
	expect(sizeof(mrt_channel_out) == 192, "mrt_channel_out is 192 bytes");
	expect(check(good) == nullptr && check(good, KNOWN) == nullptr, "a good descriptor refused");
	mrt_channel_out d = good; d.reserved = 0xFFFFFFFFu;
	expect(check(d) == nullptr, "the reserved word looked at");
	// 1. null pointers, each in turn
	expect(has(mrt::channel_out_invalid(nullptr, P, &good, 0u, KNOWN), "null"), "null rays accepted");
	expect(has(mrt::channel_out_invalid(P, nullptr, &good, 0u, KNOWN), "null"), "null hits accepted");
	expect(has(mrt::channel_out_invalid(P, P, nullptr, 0u, KNOWN), "null"), "null descriptor accepted");
	// 2. struct_size
	for (uint32_t sz : { 0u, 184u, 191u, 193u, 200u, 0xFFFFFFFFu }) {
		d = good; d.struct_size = sz;
		expect(has(check(d), "struct_size"), "struct_size " + std::to_string(sz) + " accepted");
	}
	// 3. flags
	for (uint32_t bit = 0; bit < 32u; bit++) {
		const uint32_t f = 1u << bit;
		expect((check(good, f) != nullptr) == ((f & KNOWN) == 0u), "flag bit " + std::to_string(bit));
		expect((mrt::channel_out_invalid(P, P, &good, f, MRT_FLAG_ASYNC) != nullptr) == (f != MRT_FLAG_ASYNC), "grid form, flag bit " + std::to_string(bit));
		expect((mrt::image_call_invalid(P, P, P, true, f, 0u) != nullptr) == (f != MRT_FLAG_ASYNC), "finish, flag bit " + std::to_string(bit));
		expect((mrt::image_call_invalid(P, nullptr, P, false, f, 0u) != nullptr) == (f != MRT_FLAG_ASYNC), "to_rgba8, flag bit " + std::to_string(bit));
	}
	expect(has(mrt::channel_out_invalid(P, P, &good, MRT_FLAG_HOST_LAYOUT, MRT_FLAG_ASYNC), "flag"), "the host layout accepted by the grid form");
	// 4. COLOR, 5. nothing selected, and each of the 2 x 11 entries alone
	for (uint32_t c = 0; c < MRT_CHANNEL_COUNT; c++)
		for (int plane = 0; plane < 2; plane++) {
			d = descriptor();
			if (plane) d.d_rgba8[c] = PB; else d.d_rgba[c] = PF;
			const std::string name = std::string(plane ? "d_rgba8[" : "d_rgba[") + std::to_string(c) + "]";
			if (c == MRT_CHANNEL_COLOR) expect(has(check(d), "COLOR"), name + " accepted");
			else {
				expect(check(d) == nullptr, name + " alone refused");
				expect(mrt::channel_mask(&d) == 1u << c, name + ": the mask");
			}
		}
	d = descriptor();
	expect(has(check(d), "no channel"), "an empty selection accepted");
	// 6. the ranges
	const float bad[3] = { std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity() };
	for (float x : bad) {
		d = good; d.inv_depth_range = x; expect(has(check(d), "finite"), "inv_depth_range not finite, accepted");
		d = good; d.inv_pos_range = x; expect(has(check(d), "finite"), "inv_pos_range not finite, accepted");
	}
	for (float x : { 0.0f, -0.0f, -3.0f, std::numeric_limits<float>::max(), std::numeric_limits<float>::denorm_min() }) {
		d = good; d.inv_depth_range = x; d.inv_pos_range = x;
		expect(check(d) == nullptr, "a finite range refused");
	}
	// the order: pointer, struct_size, flag, COLOR, selection, ranges
	d = descriptor(); d.struct_size = 8u; d.d_rgba8[MRT_CHANNEL_COLOR] = PB; d.inv_pos_range = bad[0];
	expect(has(mrt::channel_out_invalid(P, nullptr, &d, 1u << 20, KNOWN), "null"), "order: pointers first");
	expect(has(check(d, 1u << 20), "struct_size"), "order: struct_size second");
	d.struct_size = (uint32_t)sizeof(d);
	expect(has(check(d, 1u << 20), "flag"), "order: flags third");
	expect(has(check(d), "COLOR"), "order: COLOR fourth");
	d.d_rgba8[MRT_CHANNEL_COLOR] = nullptr;
	expect(has(check(d), "no channel"), "order: the selection fifth");
	d.d_rgba8[MRT_CHANNEL_UV] = PB;
	expect(has(check(d), "finite"), "order: the ranges last");
	d.inv_pos_range = 1.0f;
	expect(check(d) == nullptr, "the mended descriptor refused");
	// the image calls: pointer, flag, mode, outputs
	expect(mrt::image_call_invalid(P, P, P, true, 0u, 0u) == nullptr && mrt::image_call_invalid(P, P, nullptr, true, MRT_FLAG_ASYNC, 4u) == nullptr
			&& mrt::image_call_invalid(P, nullptr, P, true, 0u, 2u) == nullptr, "a good finish refused");
	for (uint32_t m = 0; m <= 4u; m++) expect(mrt::image_call_invalid(P, P, P, true, 0u, m) == nullptr, "finish mode " + std::to_string(m) + " refused");
	expect(has(mrt::image_call_invalid(P, P, P, true, 0u, 5u), "tonemap") && has(mrt::image_call_invalid(P, P, P, true, 0u, 0xFFFFFFFFu), "tonemap"), "finish: mode > 4 accepted");
	expect(has(mrt::image_call_invalid(nullptr, P, P, true, 0u, 0u), "null"), "finish: null input accepted");
	expect(has(mrt::image_call_invalid(P, nullptr, nullptr, true, 0u, 0u), "no output"), "finish: both outputs null accepted");
	expect(has(mrt::image_call_invalid(nullptr, nullptr, nullptr, true, 1u << 9, 9u), "null"), "finish order: the pointer first");
	expect(has(mrt::image_call_invalid(P, nullptr, nullptr, true, 1u << 9, 9u), "flag"), "finish order: flags second");
	expect(has(mrt::image_call_invalid(P, nullptr, nullptr, true, 0u, 9u), "tonemap"), "finish order: the mode third");
	expect(mrt::image_call_invalid(P, nullptr, P, false, 0u, 0u) == nullptr && mrt::image_call_invalid(P, nullptr, P, false, MRT_FLAG_ASYNC, 77u) == nullptr, "a good to_rgba8 refused, or its mode looked at");
	expect(has(mrt::image_call_invalid(nullptr, nullptr, P, false, 0u, 0u), "null") && has(mrt::image_call_invalid(P, nullptr, nullptr, false, 0u, 0u), "null"), "to_rgba8: a null pointer accepted");
	expect(has(mrt::image_call_invalid(P, nullptr, nullptr, false, 1u << 9, 0u), "null"), "to_rgba8 order: pointers first");
}

void masks()
{
	// a dozen descriptors: the channels given as floats, as bytes, and the mask word
	const struct { uint32_t floats, bytes; } sel[12] = {
		{ 0x002u, 0u }, { 0u, 0x400u }, { 0x7FEu, 0u }, { 0u, 0x7FEu }, { 0x7FEu, 0x7FEu }, { 0x2AAu, 0x554u },
		{ 0x004u, 0x004u }, { 0x0F0u, 0x00Eu }, { 0x700u, 0x0FEu }, { 0x082u, 0x200u }, { 0x400u, 0x002u }, { 0x156u, 0x156u } };
	for (int k = 0; k < 12; k++) {
		mrt_channel_out d = descriptor();
		d.inv_depth_range = 0.5f + (float)k; d.inv_pos_range = -1.5f - (float)k;
		for (uint32_t c = 0; c < MRT_CHANNEL_COUNT; c++) {
			if (sel[k].floats >> c & 1u) d.d_rgba[c] = PF + 4 * c;
			if (sel[k].bytes >> c & 1u) d.d_rgba8[c] = PB + 4 * c;
		}
		const uint32_t want = sel[k].floats | sel[k].bytes;
		expect(mrt::channel_mask(&d) == want, "mask of descriptor " + std::to_string(k));
		expect(check(d) == nullptr, "descriptor " + std::to_string(k) + " refused");
		mrt::ChannelParams c;
		std::memset(&c, 0xA5, sizeof(c));
		const void *keep = c.records;
		mrt::fill_channel_params(&d, c);
		bool same = c.mask == want && bits(c.inv_depth_range) == bits(d.inv_depth_range) && bits(c.inv_pos_range) == bits(d.inv_pos_range);
		for (uint32_t ch = 0; ch < MRT_CHANNEL_COUNT; ch++) same = same && c.rgba[ch] == d.d_rgba[ch] && c.rgba8[ch] == d.d_rgba8[ch];
		expect(same && c.records == keep, "the kernel's copy of descriptor " + std::to_string(k));
	}
	expect((mrt::CHANNELS_ROW & mrt::CHANNELS_MATERIAL) == mrt::CHANNELS_MATERIAL && mrt::CHANNELS_ROW == 0x682u && mrt::CHANNELS_MATERIAL == 0x082u, "the row and material channel sets");
}

void bytes()
{
	for (uint32_t k = 0; k <= 255u; k++) expect(mrt::to_rgba8((float)k / 255.0f) == k, "to_rgba8 of " + std::to_string(k) + " / 255");
	expect(mrt::to_rgba8(0.0f) == 0u && mrt::to_rgba8(-0.0f) == 0u && mrt::to_rgba8(-1.0f) == 0u && mrt::to_rgba8(-1e30f) == 0u, "to_rgba8 at and below 0");
	expect(mrt::to_rgba8(1.0f) == 255u && mrt::to_rgba8(1.5f) == 255u && mrt::to_rgba8(1e30f) == 255u, "to_rgba8 at and above 1");
	expect(mrt::to_rgba8(std::numeric_limits<float>::infinity()) == 255u && mrt::to_rgba8(-std::numeric_limits<float>::infinity()) == 0u, "to_rgba8 of the infinities");
	expect(mrt::to_rgba8(std::numeric_limits<float>::quiet_NaN()) == 0u, "to_rgba8 of a NaN");
	expect(mrt::to_rgba8(0.5f) == 128u && mrt::to_rgba8(0.25f) == 64u && mrt::to_rgba8(0.002f) == 1u && mrt::to_rgba8(0.0019f) == 0u, "to_rgba8 rounds half up");
	expect(bits(mrt::finish_white()) == bits(mrt::hable_partial(11.2f)), "Hable's white value is mrt_path_finish's");
	expect(mrt::tonemap(11.2f, 2u, mrt::finish_white()) == 1.0f, "Hable maps its white point to 1");
}

} // namespace

int main()
{
	refusals();
	masks();
	bytes();
	std::printf("%d checks hold of %d\n", n_checks - n_fail, n_checks);
	return n_fail ? 1 : 0;
}
