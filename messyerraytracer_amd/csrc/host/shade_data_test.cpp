// shade_data_test.cpp -- host/shade_data.cpp (the checks of an mrt_shade_data descriptor and the 64-byte rows packed from host arrays)
// without a device: every optional per-triangle array absent or present (all eight combinations) for n_tris 0, 1 and 5, each row word
// against the layout {n0 xyz, material id | n1 xyz, uv0.x | n2 xyz, uv0.y | uv1 xy, uv2 xy}, nothing written past the rows; and the
// descriptor's refusals: null, a wrong struct_size, an unknown flag, materials missing, every float of a material not finite in turn.
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../shade_data.h"

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

mrt_shade_data descriptor(uint32_t n_tris, const std::vector<mrt_material> &mats, const uint32_t *ids, const float *n9, const float *uv6)
{
	mrt_shade_data d;
	std::memset(&d, 0, sizeof(d));
	d.struct_size = sizeof(d); d.n_tris = n_tris; d.n_materials = (uint32_t)mats.size();
	d.materials = mats.empty() ? nullptr : mats.data();
	d.material_ids = ids; d.normals9 = n9; d.uvs6 = uv6;
	return d;
}

mrt_material material(float x)
{
	mrt_material m;
	std::memset(&m, 0, sizeof(m));
	m.albedo[0] = x; m.albedo[1] = x + 0.125f; m.albedo[2] = x + 0.25f; m.metallic = 0.5f; m.roughness = 0.02f; m.specular = 0.5f;
	m.emission[0] = 1.0f; m.emission[1] = 2.0f; m.emission[2] = 3.0f; m.emission_energy = 4.0f; m.flags = 3u;
	return m;
}

void packing()
{
	const uint32_t kGuard = 0xDEADBEEFu;
	for (uint32_t n : {0u, 1u, 5u}) {
		// exactly n elements each, so that a read past an array's end is a read past its allocation
		std::vector<uint32_t> ids(n);
		std::vector<float> n9((size_t)n * 9u), uv6((size_t)n * 6u);
		for (uint32_t t = 0; t < n; t++) {
			ids[t] = 1000u + t * 7u;
			for (int k = 0; k < 9; k++) n9[t * 9u + k] = 1.0f + (float)t * 16.0f + (float)k * 0.25f;
			for (int k = 0; k < 6; k++) uv6[t * 6u + k] = -2.0f - (float)t * 8.0f - (float)k * 0.5f;
		}
		for (int mask = 0; mask < 8; mask++) {
			const bool has_n = mask & 1, has_i = mask & 2, has_u = mask & 4;
			const std::string name = "n_tris " + std::to_string(n) + " mask " + std::to_string(mask);
			const std::vector<mrt_material> mats = { material(0.25f) };
			const mrt_shade_data d = descriptor(n, mats, has_i ? ids.data() : nullptr, has_n ? n9.data() : nullptr, has_u ? uv6.data() : nullptr);
			expect(mrt::shade_data_invalid(&d) == nullptr, name + ": refused");
			const uint32_t want_present = n == 0u ? 0u : (has_n ? mrt::SHADE_HAS_NORMALS : 0u) | (has_i ? mrt::SHADE_HAS_IDS : 0u) | (has_u ? mrt::SHADE_HAS_UVS : 0u);
			expect(mrt::shade_data_present(&d) == want_present, name + ": present bits");
			std::vector<uint32_t> rows((size_t)n * 16u + 4u, kGuard);
			mrt::pack_shade_rows_host(&d, rows.data());
			for (uint32_t t = 0; t < n; t++) {
				const uint32_t *r = rows.data() + (size_t)t * 16u;
				bool ok = true;
				for (int v = 0; v < 3; v++)
					for (int k = 0; k < 3; k++) ok = ok && r[4 * v + k] == (has_n ? bits(n9[t * 9u + 3 * v + k]) : 0u);
				ok = ok && r[3] == (has_i ? ids[t] : 0u);
				ok = ok && r[7] == (has_u ? bits(uv6[t * 6u]) : 0u) && r[11] == (has_u ? bits(uv6[t * 6u + 1]) : 0u);
				for (int k = 0; k < 4; k++) ok = ok && r[12 + k] == (has_u ? bits(uv6[t * 6u + 2 + k]) : 0u);
				expect(ok, name + ": row " + std::to_string(t));
			}
			bool guard = true;
			for (int k = 0; k < 4; k++) guard = guard && rows[(size_t)n * 16u + k] == kGuard;
			expect(guard, name + ": wrote past the rows");
		}
	}
}

void refusals()
{
	const std::vector<mrt_material> mats = { material(0.25f), material(0.5f) };
	const uint32_t ids[1] = { 0u };
	mrt_shade_data d = descriptor(1, mats, ids, nullptr, nullptr);
	expect(mrt::shade_data_invalid(&d) == nullptr, "a good descriptor refused");
	expect(mrt::shade_data_invalid(nullptr) != nullptr, "null descriptor accepted");
	d.struct_size = sizeof(d) - 4u;
	expect(mrt::shade_data_invalid(&d) != nullptr, "wrong struct_size accepted");
	d = descriptor(1, mats, ids, nullptr, nullptr);
	d.flags = 2u;
	expect(mrt::shade_data_invalid(&d) != nullptr, "unknown flag accepted");
	d.flags = MRT_SHADE_ARRAYS_ON_DEVICE;
	expect(mrt::shade_data_invalid(&d) == nullptr, "MRT_SHADE_ARRAYS_ON_DEVICE refused");
	d = descriptor(1, mats, ids, nullptr, nullptr);
	d.materials = nullptr;
	expect(mrt::shade_data_invalid(&d) != nullptr, "n_materials > 0 with null materials accepted");
	d.n_materials = 0u;
	expect(mrt::shade_data_invalid(&d) == nullptr, "no materials refused");
	d = descriptor(0, {}, nullptr, nullptr, nullptr);
	expect(mrt::shade_data_invalid(&d) == nullptr, "an empty descriptor refused");
	// every float of a material, in the last material, not finite in turn; flags and reserved are not floats: any bits pass
	const float bad[3] = { std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity() };
	for (int w = 0; w < 10; w++)
		for (float b : bad) {
			std::vector<mrt_material> m = mats;
			reinterpret_cast<float *>(&m[1])[w] = b;
			d = descriptor(1, m, ids, nullptr, nullptr);
			expect(mrt::shade_data_invalid(&d) != nullptr, "material word " + std::to_string(w) + " not finite, accepted");
		}
	std::vector<mrt_material> m = mats;
	m[0].flags = 0x7FC00000u; m[0].reserved = 0x7F800000u;
	d = descriptor(1, m, ids, nullptr, nullptr);
	expect(mrt::shade_data_invalid(&d) == nullptr, "flags / reserved looked at as floats");
	m[0].albedo[0] = std::numeric_limits<float>::denorm_min(); m[0].roughness = -0.0f; m[0].emission_energy = -3.0f;
	d = descriptor(1, m, ids, nullptr, nullptr);
	expect(mrt::shade_data_invalid(&d) == nullptr, "finite but odd values refused");
}

} // namespace

int main()
{
	packing();
	refusals();
	std::printf("%d checks hold of %d\n", n_checks - n_fail, n_checks);
	return n_fail ? 1 : 0;
}
