// shade_data.h -- the resident shade data of a context (mrt_upload_shade_data): the descriptor's checks and the 64-byte row of a
// triangle, shared by the host path (host/shade_data.cpp: host arrays, packed before one copy) and the device path (surface_kernel.h:
// device arrays, packed by pack_shade_rows_kernel), so that both write the same rows.  Host-only code may include this without HIP.
#pragma once
#include <cstdint>
#include "../../include/mrt_hip.h"

#ifndef MRT_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define MRT_HD __host__ __device__
#else
#define MRT_HD
#endif
#endif

static_assert(sizeof(mrt_material) == 48, "mrt_material must be 48 bytes: three 16-byte loads");
static_assert(sizeof(mrt_surface64) == 64, "mrt_surface64 must be 64 bytes: four 16-byte stores");

namespace mrt {

// which per-triangle arrays are resident (SurfaceParams::present)
enum : uint32_t { SHADE_HAS_NORMALS = 1u << 0, SHADE_HAS_IDS = 1u << 1, SHADE_HAS_UVS = 1u << 2 };

// Row t: {n0 xyz, material id | n1 xyz, uv0.x | n2 xyz, uv0.y | uv1 xy, uv2 xy} as 16 words; an absent array leaves zeros.
MRT_HD inline void pack_shade_row(const uint32_t *ids, const float *normals9, const float *uvs6, uint64_t t, uint32_t out[16])
{
	union { float f; uint32_t u; } c;
	for (int k = 0; k < 16; k++) out[k] = 0u;
	if (normals9) {
		const float *n = normals9 + t * 9u;
		for (int v = 0; v < 3; v++)
			for (int k = 0; k < 3; k++) { c.f = n[3 * v + k]; out[4 * v + k] = c.u; }
	}
	if (ids) out[3] = ids[t];
	if (uvs6) {
		const float *q = uvs6 + t * 6u;
		c.f = q[0]; out[7] = c.u; c.f = q[1]; out[11] = c.u;
		for (int k = 0; k < 4; k++) { c.f = q[2 + k]; out[12 + k] = c.u; }
	}
}

// host/shade_data.cpp (no device, no library)
// What mrt_upload_shade_data refuses about its descriptor, or null.
const char *shade_data_invalid(const mrt_shade_data *data);
// SHADE_HAS_* of the descriptor's non-null per-triangle arrays (0 when n_tris == 0)
uint32_t shade_data_present(const mrt_shade_data *data);
// The rows of host arrays: rows = n_tris x 16 words.
void pack_shade_rows_host(const mrt_shade_data *data, uint32_t *rows);

} // namespace mrt
