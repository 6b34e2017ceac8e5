// channels.h -- the renderer's channels and its 8-bit image (mrt_shade_channels, mrt_shade_grid_channels, mrt_finish_color,
// mrt_image_to_rgba8): to_rgba8 as include/mrt_hip.h states it (one definition for the kernels, channel_kernel.h, and the host), and
// the checks of the calls (host/channel_data.cpp).  Host-only code may include this without HIP.
#pragma once
#include "mrt_internal.h"
#include "path.h"

static_assert(sizeof(mrt_channel_out) == 192, "mrt_channel_out must be 192 bytes");
static_assert(MRT_CHANNEL_COUNT == 11, "RayImage::Channel has eleven values");

namespace mrt {

// RayImage::to_image per component: a NaN becomes 0
MRT_HD inline uint32_t to_rgba8(float c)
{
	float x = c * 255.0f + 0.5f;
	x = 0.0f < x ? x : 0.0f;
	x = x < 255.0f ? x : 255.0f;
	return (uint32_t)x;
}

// host/channel_data.cpp (no device, no library)
// What the two channel calls refuse before the band is looked at, or null, in the order include/mrt_hip.h lists; known = the flags
// of the form.
const char *channel_out_invalid(const void *d_rays_or_cam, const void *d_hits, const mrt_channel_out *out, uint32_t flags, uint32_t known);
// Bit c set: channel c of a descriptor is selected.
uint32_t channel_mask(const mrt_channel_out *out);
// The kernel's copy of a checked descriptor: the mask, the two ranges and the planes (the records and the shade data are the caller's).
void fill_channel_params(const mrt_channel_out *out, ChannelParams &c);
// What mrt_finish_color (need_mode) and mrt_image_to_rgba8 refuse, or null, in the header's order.
const char *image_call_invalid(const void *d_in, const void *d_rgba, const void *d_rgba8, bool need_mode, uint32_t flags, uint32_t tonemap_mode);
// Hable's white value, hp(11.2f): what mrt_path_finish passes to its kernel.
float finish_white();

} // namespace mrt
