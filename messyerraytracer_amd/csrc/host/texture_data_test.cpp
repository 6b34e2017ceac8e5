// texture_data_test.cpp -- host/texture_data.cpp and texture.h without a device: every refusal of mrt_upload_textures and their order
// (each required pointer null in turn, each dimension bound, every flag bit, every format word, binding indices, normal_scale not
// finite, the pool's overflow), what passes; the pool offsets and the descriptor table word by word for a few texture lists, with a
// guard behind the table.  No pixel and no tangent is ever read: their pointers are never dereferenced.
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../texture.h"

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

void *const P = reinterpret_cast<void *>(16); // never dereferenced

mrt_texture texture(uint32_t w, uint32_t h, uint32_t format)
{
	mrt_texture t;
	std::memset(&t, 0, sizeof(t));
	t.width = w; t.height = h; t.format = format; t.pixels = P;
	return t;
}

mrt_material_textures binding(uint32_t albedo, uint32_t normal, float scale)
{
	mrt_material_textures b;
	std::memset(&b, 0, sizeof(b));
	b.albedo_texture = albedo; b.normal_texture = normal; b.normal_scale = scale;
	return b;
}

struct Set {
	std::vector<mrt_texture> tex;
	std::vector<mrt_material_textures> bind;
	mrt_texture_set s;
	Set()
	{
		tex = { texture(8, 8, MRT_TEXEL_RGBA8), texture(3, 5, MRT_TEXEL_RGBA32F) };
		bind = { binding(0, 1, 1.0f), binding(MRT_NO_TEXTURE, MRT_NO_TEXTURE, 0.0f), binding(1, MRT_NO_TEXTURE, -4.0f) };
		sync();
	}
	void sync()
	{
		std::memset(&s, 0, sizeof(s));
		s.struct_size = (uint32_t)sizeof(mrt_texture_set);
		s.n_textures = (uint32_t)tex.size(); s.n_bindings = (uint32_t)bind.size(); s.n_tangent_tris = 7u;
		s.textures = tex.data(); s.bindings = bind.data(); s.tangents12 = reinterpret_cast<const float *>(P);
	}
};

void refusals()
{
	Set g;
	expect(mrt::texture_set_invalid(&g.s) == nullptr, "a good set refused");
	{ Set d; d.s.flags = MRT_TEXTURES_ON_DEVICE; expect(mrt::texture_set_invalid(&d.s) == nullptr, "the device flag refused"); }
	{ Set d; d.s.reserved = 0xFFFFFFFFu; d.tex[0].reserved = 0xFFFFFFFFu; d.bind[0].reserved = 0x7FC00000u;
	  expect(mrt::texture_set_invalid(&d.s) == nullptr, "a reserved word looked at"); }
	{ Set d; d.s.n_textures = d.s.n_bindings = d.s.n_tangent_tris = 0u; d.s.textures = nullptr; d.s.bindings = nullptr; d.s.tangents12 = nullptr;
	  expect(mrt::texture_set_invalid(&d.s) == nullptr, "an empty set refused"); }
	{ Set d; d.s.n_tangent_tris = 0u; d.s.tangents12 = nullptr; expect(mrt::texture_set_invalid(&d.s) == nullptr, "absent tangents refused"); }
	{ Set d; d.s.n_bindings = 0u; d.s.bindings = nullptr; expect(mrt::texture_set_invalid(&d.s) == nullptr, "no bindings refused"); }
	// 1. the descriptor
	expect(has(mrt::texture_set_invalid(nullptr), "null"), "a null descriptor accepted");
	// 2. struct_size
	for (uint32_t size : { 0u, (uint32_t)sizeof(mrt_texture_set) - 8u, (uint32_t)sizeof(mrt_texture_set) + 8u, 0xFFFFFFFFu }) {
		Set d; d.s.struct_size = size;
		expect(has(mrt::texture_set_invalid(&d.s), "struct_size"), "struct_size " + std::to_string(size) + " accepted");
	}
	// 3. every flag bit
	for (uint32_t bit = 0; bit < 32u; bit++) {
		Set d; d.s.flags = 1u << bit;
		expect((mrt::texture_set_invalid(&d.s) != nullptr) == (bit != 0u), "flag bit " + std::to_string(bit));
		if (bit) expect(has(mrt::texture_set_invalid(&d.s), "flag"), "flag bit " + std::to_string(bit) + ": another refusal");
	}
	// 4. a count with a null array, each in turn
	{ Set d; d.s.textures = nullptr; expect(has(mrt::texture_set_invalid(&d.s), "null textures"), "null textures accepted"); }
	{ Set d; d.s.bindings = nullptr; expect(has(mrt::texture_set_invalid(&d.s), "null bindings"), "null bindings accepted"); }
	{ Set d; d.s.tangents12 = nullptr; expect(has(mrt::texture_set_invalid(&d.s), "null tangents12"), "null tangents12 accepted"); }
	// 5. each dimension bound, on either texture
	for (int which = 0; which < 2; which++)
		for (int axis = 0; axis < 2; axis++) {
			for (uint32_t bad : { 0u, MRT_TEXTURE_MAX_DIM + 1u, 0x80000000u, 0xFFFFFFFFu }) {
				Set d; (axis ? d.tex[which].height : d.tex[which].width) = bad;
				expect(has(mrt::texture_set_invalid(&d.s), "width or height"), "dimension " + std::to_string(bad) + " accepted");
			}
			for (uint32_t ok : { 1u, MRT_TEXTURE_MAX_DIM }) {
				Set d; (axis ? d.tex[which].height : d.tex[which].width) = ok;
				expect(mrt::texture_set_invalid(&d.s) == nullptr, "dimension " + std::to_string(ok) + " refused");
			}
		}
	// 6. the format
	for (uint32_t f : { 2u, 3u, 0x80000000u, 0xFFFFFFFFu }) {
		Set d; d.tex[1].format = f;
		expect(has(mrt::texture_set_invalid(&d.s), "format"), "format " + std::to_string(f) + " accepted");
	}
	// 7. pixels
	for (int which = 0; which < 2; which++) {
		Set d; d.tex[which].pixels = nullptr;
		expect(has(mrt::texture_set_invalid(&d.s), "pixels"), "null pixels accepted");
	}
	// 8. binding indices
	for (int field = 0; field < 2; field++) {
		for (uint32_t bad : { 2u, 3u, 0x7FFFFFFFu, 0xFFFFFFFEu }) {
			Set d; (field ? d.bind[2].normal_texture : d.bind[2].albedo_texture) = bad;
			expect(has(mrt::texture_set_invalid(&d.s), "index"), "binding index " + std::to_string(bad) + " accepted");
		}
		for (uint32_t ok : { 0u, 1u, MRT_NO_TEXTURE }) {
			Set d; (field ? d.bind[2].normal_texture : d.bind[2].albedo_texture) = ok;
			expect(mrt::texture_set_invalid(&d.s) == nullptr, "binding index " + std::to_string(ok) + " refused");
		}
	}
	{ Set d; d.s.n_textures = 0u; d.s.textures = nullptr; expect(has(mrt::texture_set_invalid(&d.s), "index"), "an index with no textures accepted"); }
	// 9. normal_scale
	const float bad[3] = { std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity() };
	for (float x : bad)
		for (int b = 0; b < 3; b++) {
			Set d; d.bind[b].normal_scale = x;
			expect(has(mrt::texture_set_invalid(&d.s), "finite"), "normal_scale not finite accepted");
		}
	{ Set d; d.bind[0].normal_scale = std::numeric_limits<float>::max(); d.bind[1].normal_scale = -0.0f;
	  expect(mrt::texture_set_invalid(&d.s) == nullptr, "a finite normal_scale refused"); }
	// 10. the pool: 16 images of 16384 x 16384 RGBA32F are 2^32 units; 15 and one RGBA8 image of the same size (2^26 units) are not
	{
		Set d; d.tex.assign(16, texture(MRT_TEXTURE_MAX_DIM, MRT_TEXTURE_MAX_DIM, MRT_TEXEL_RGBA32F)); d.sync();
		expect(has(mrt::texture_set_invalid(&d.s), "pooled"), "a pool of 2^32 units accepted");
		d.tex[15] = texture(MRT_TEXTURE_MAX_DIM, MRT_TEXTURE_MAX_DIM, MRT_TEXEL_RGBA8); d.sync();
		expect(mrt::texture_set_invalid(&d.s) == nullptr, "a pool of 15 * 2^28 + 2^26 units refused");
		d.tex.assign(40, texture(MRT_TEXTURE_MAX_DIM, MRT_TEXTURE_MAX_DIM, MRT_TEXEL_RGBA32F)); d.sync();
		expect(has(mrt::texture_set_invalid(&d.s), "pooled"), "a pool of 40 * 2^28 units accepted");
	}
	// the order: descriptor, struct_size, flag, null arrays, per texture {dimension, format, pixels}, per binding {index, scale}, pool
	{
		Set d; d.tex.assign(17, texture(MRT_TEXTURE_MAX_DIM, MRT_TEXTURE_MAX_DIM, MRT_TEXEL_RGBA32F)); d.sync();
		d.bind[1].normal_scale = bad[0]; d.bind[0].albedo_texture = 99u;
		d.tex[3].pixels = nullptr; d.tex[3].format = 9u; d.tex[3].width = 0u;
		d.s.tangents12 = nullptr; d.s.bindings = nullptr; d.s.textures = nullptr; d.s.flags = 1u << 7; d.s.struct_size = 4u;
		expect(has(mrt::texture_set_invalid(&d.s), "struct_size"), "order: struct_size first");
		d.s.struct_size = (uint32_t)sizeof(mrt_texture_set);
		expect(has(mrt::texture_set_invalid(&d.s), "flag"), "order: the flag second");
		d.s.flags = 0u;
		expect(has(mrt::texture_set_invalid(&d.s), "null textures"), "order: null textures");
		d.s.textures = d.tex.data();
		expect(has(mrt::texture_set_invalid(&d.s), "null bindings"), "order: null bindings");
		d.s.bindings = d.bind.data();
		expect(has(mrt::texture_set_invalid(&d.s), "null tangents12"), "order: null tangents12");
		d.s.tangents12 = reinterpret_cast<const float *>(P);
		expect(has(mrt::texture_set_invalid(&d.s), "width or height"), "order: the dimension");
		d.tex[3].width = 4u;
		expect(has(mrt::texture_set_invalid(&d.s), "format"), "order: the format");
		d.tex[3].format = MRT_TEXEL_RGBA32F;
		expect(has(mrt::texture_set_invalid(&d.s), "pixels"), "order: the pixels");
		d.tex[3].pixels = P;
		expect(has(mrt::texture_set_invalid(&d.s), "index"), "order: the binding index");
		d.bind[0].albedo_texture = 16u;
		expect(has(mrt::texture_set_invalid(&d.s), "finite"), "order: normal_scale");
		d.bind[1].normal_scale = 2.0f;
		expect(has(mrt::texture_set_invalid(&d.s), "pooled"), "order: the pool last");
	}
}

void layouts()
{
	expect(mrt::texel_bytes(MRT_TEXEL_RGBA8) == 4u && mrt::texel_bytes(MRT_TEXEL_RGBA32F) == 16u && mrt::texel_bytes(2u) == 0u, "texel_bytes");
	struct Case { std::vector<mrt_texture> tex; std::vector<uint32_t> offsets; uint64_t units; };
	const uint32_t A = MRT_TEXEL_RGBA8, B = MRT_TEXEL_RGBA32F, M = MRT_TEXTURE_MAX_DIM;
	const std::vector<Case> cases = {
		{ {}, {}, 0u },
		{ { texture(1, 1, A) }, { 0u }, 1u },                                           // 4 bytes: one unit
		{ { texture(1, 1, A), texture(1, 1, B), texture(2, 2, A), texture(2, 2, B) }, { 0u, 1u, 2u, 3u }, 7u },
		{ { texture(3, 5, A), texture(3, 5, B), texture(8, 8, A), texture(8, 8, B), texture(64, 16, A) }, { 0u, 4u, 19u, 35u, 99u }, 355u }, // 60 bytes: 4 units
		{ { texture(5, 1, A), texture(1, 5, A), texture(1, 1, B) }, { 0u, 2u, 4u }, 5u },   // 20 bytes: 2 units, 12 bytes of padding
		{ { texture(M, M, B), texture(M, M, A), texture(1, 1, A) }, { 0u, 1u << 28, (1u << 28) + (1u << 26) }, (1ull << 28) + (1ull << 26) + 1u },
	};
	for (size_t c = 0; c < cases.size(); c++) {
		const Case &k = cases[c];
		mrt_texture_set s;
		std::memset(&s, 0, sizeof(s));
		s.struct_size = (uint32_t)sizeof(s); s.n_textures = (uint32_t)k.tex.size(); s.textures = k.tex.empty() ? nullptr : k.tex.data();
		expect(mrt::texture_set_invalid(&s) == nullptr, "layout case " + std::to_string(c) + " refused");
		std::vector<uint32_t> words(k.tex.size() * 4u + 8u, 0xA5A5A5A5u); // the table, then a guard
		const uint64_t units = mrt::texture_pool_layout(&s, reinterpret_cast<mrt::TextureDesc *>(words.data()));
		expect(units == k.units, "layout case " + std::to_string(c) + ": pool units " + std::to_string(units));
		for (size_t t = 0; t < k.tex.size(); t++) {
			const uint32_t want[4] = { k.offsets[t], k.tex[t].width, k.tex[t].height, k.tex[t].format };
			for (int w = 0; w < 4; w++)
				expect(words[t * 4u + w] == want[w], "layout case " + std::to_string(c) + ", texture " + std::to_string(t) + ", word " + std::to_string(w));
			// an image ends where the next begins, or before it by less than one unit
			const uint64_t bytes = (uint64_t)k.tex[t].width * k.tex[t].height * mrt::texel_bytes(k.tex[t].format);
			const uint64_t next = t + 1 < k.tex.size() ? k.offsets[t + 1] : units;
			expect((uint64_t)k.offsets[t] * 16u + bytes <= next * 16u && next * 16u - ((uint64_t)k.offsets[t] * 16u + bytes) < 16u, "layout case " + std::to_string(c) + ": image " + std::to_string(t) + " against the next");
		}
		bool guard = true;
		for (size_t w = k.tex.size() * 4u; w < words.size(); w++) guard = guard && words[w] == 0xA5A5A5A5u;
		expect(guard, "layout case " + std::to_string(c) + ": the guard behind the table");
	}
}

} // namespace

int main()
{
	refusals();
	layouts();
	std::printf("%d checks hold of %d\n", n_checks - n_fail, n_checks);
	return n_fail ? 1 : 0;
}
