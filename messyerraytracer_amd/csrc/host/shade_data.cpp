// shade_data.cpp -- host side of mrt_upload_shade_data: the descriptor's checks and the row packing of host arrays (shade_data.h).
// No device and no HIP call, so that csrc/host/shade_data_test.cpp drives it alone.
#include "../shade_data.h"

#include <cmath>

namespace mrt {

const char *shade_data_invalid(const mrt_shade_data *data)
{
	if (!data) return "null shade data descriptor";
	if (data->struct_size != sizeof(mrt_shade_data)) return "mrt_shade_data.struct_size does not match";
	if (data->flags & ~(uint32_t)MRT_SHADE_ARRAYS_ON_DEVICE) return "unknown flag for shade data";
	if (data->n_materials && !data->materials) return "n_materials > 0 with null materials";
	for (uint32_t m = 0; m < data->n_materials; m++) {
		const mrt_material &M = data->materials[m];
		const float f[10] = { M.albedo[0], M.albedo[1], M.albedo[2], M.metallic, M.roughness, M.specular,
			M.emission[0], M.emission[1], M.emission[2], M.emission_energy };
		for (float x : f)
			if (!std::isfinite(x)) return "a material holds a value that is not finite";
	}
	return nullptr;
}

uint32_t shade_data_present(const mrt_shade_data *data)
{
	if (data->n_tris == 0u) return 0u;
	return (data->normals9 ? SHADE_HAS_NORMALS : 0u) | (data->material_ids ? SHADE_HAS_IDS : 0u) | (data->uvs6 ? SHADE_HAS_UVS : 0u);
}

void pack_shade_rows_host(const mrt_shade_data *data, uint32_t *rows)
{
	for (uint64_t t = 0; t < data->n_tris; t++)
		pack_shade_row(data->material_ids, data->normals9, data->uvs6, t, rows + t * 16u);
}

} // namespace mrt
