// channel_data.cpp -- host side of mrt_shade_channels / mrt_shade_grid_channels / mrt_finish_color / mrt_image_to_rgba8: the
// refusals in the order include/mrt_hip.h lists, the selection mask, the kernel's copy of a descriptor and Hable's white value
// (channels.h).  No device and no HIP call, so that csrc/host/channel_data_test.cpp drives it alone.
#include "../channels.h"

#include <cmath>

namespace mrt {

uint32_t channel_mask(const mrt_channel_out *out)
{
	uint32_t mask = 0u;
	for (uint32_t c = 0; c < MRT_CHANNEL_COUNT; c++)
		if (out->d_rgba[c] || out->d_rgba8[c]) mask |= 1u << c;
	return mask;
}

const char *channel_out_invalid(const void *d_rays_or_cam, const void *d_hits, const mrt_channel_out *out, uint32_t flags, uint32_t known)
{
	if (!d_rays_or_cam || !d_hits || !out) return "null rays / hits / outputs";
	if (out->struct_size != sizeof(mrt_channel_out)) return "struct_size is not sizeof(mrt_channel_out)";
	if (flags & ~known) return "unknown flag for a channel pass";
	if (out->d_rgba[MRT_CHANNEL_COLOR] || out->d_rgba8[MRT_CHANNEL_COLOR]) return "COLOR is mrt_light_* followed by mrt_finish_color";
	if (channel_mask(out) == 0u) return "no channel selected";
	if (!std::isfinite(out->inv_depth_range) || !std::isfinite(out->inv_pos_range)) return "inv_depth_range / inv_pos_range is not finite";
	return nullptr;
}

void fill_channel_params(const mrt_channel_out *out, ChannelParams &c)
{
	c.mask = channel_mask(out);
	c.inv_depth_range = out->inv_depth_range; c.inv_pos_range = out->inv_pos_range;
	for (uint32_t k = 0; k < MRT_CHANNEL_COUNT; k++) { c.rgba[k] = out->d_rgba[k]; c.rgba8[k] = out->d_rgba8[k]; }
}

const char *image_call_invalid(const void *d_in, const void *d_rgba, const void *d_rgba8, bool need_mode, uint32_t flags, uint32_t tonemap_mode)
{
	if (!d_in || (!need_mode && !d_rgba8)) return "null input / output";
	if (flags & ~(uint32_t)MRT_FLAG_ASYNC) return "unknown flag for an image call";
	if (need_mode && tonemap_mode > 4u) return "tonemap_mode > 4";
	if (need_mode && !d_rgba && !d_rgba8) return "no output asked for";
	return nullptr;
}

float finish_white() { return hable_partial(11.2f); }

} // namespace mrt
