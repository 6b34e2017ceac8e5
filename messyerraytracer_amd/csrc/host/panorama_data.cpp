// panorama_data.cpp -- host side of mrt_upload_panorama: the refusals in the order include/mrt_hip.h lists and the scan of a
// host-resident image (panorama.h).  No device and no HIP call, so that csrc/host/panorama_data_test.cpp drives it alone.
#include "../panorama.h"

#include <cmath>

namespace mrt {

const char *panorama_invalid(const mrt_panorama *pano)
{
	if (!pano) return "null panorama descriptor";
	if (!pano->pixels) return "a panorama's pixels are null";
	if (pano->width == 0u || pano->height == 0u || pano->width > MRT_PANORAMA_MAX_DIM || pano->height > MRT_PANORAMA_MAX_DIM)
		return "a panorama's width or height is 0 or above MRT_PANORAMA_MAX_DIM";
	if (!std::isfinite(pano->energy)) return "a panorama's energy is not finite";
	if (pano->flags & ~(uint32_t)MRT_PANORAMA_ON_DEVICE) return "unknown flag for a panorama";
	return nullptr;
}

bool panorama_texels_finite(const float *pixels, uint64_t n_texels)
{
	for (uint64_t i = 0; i < n_texels; i++)
		if (!finite3(pixels[i * 4u], pixels[i * 4u + 1u], pixels[i * 4u + 2u])) return false;
	return true;
}

} // namespace mrt
