// mrt_context.h — the context behind the C-ABI (mrt_ctx) and what api.hip, cast.hip and schedule.hip share: the kernel
// launchers of kernels.hip / prep_kernels.hip / shade_kernels.hip / device_build.hip, the error and buffer helpers.
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>
#include "mrt_internal.h"
#include "launch_policy.h"
#include "texture.h"
#include "panorama.h"

namespace mrt {
// ---- kernels.hip: the walks
hipError_t launch_trace(const TraceParams &p, bool any_hit, bool count, hipStream_t stream);
const char *last_trace_variant();
bool quad_kernel_built();
hipError_t launch_trace_persistent(const TraceParams &p, unsigned long long *next_ray, uint32_t *overflow,
		uint32_t lds_depth, uint32_t refill, uint32_t leaf_wait, uint32_t blocks, bool any_hit, bool count, hipStream_t stream);
// record-driven casts (source_common.h): S = the family's parameter struct (instantiated in kernels.hip for ShadowParams, SelectShadowParams, ReflectParams,
// HemiParams, BounceParams, GBufferParams and EmitterShadowParams), params = an S, src = one of SourceFamily<S>'s sources, any_hit = a mode the family has; blocks != 0: the
// persistent kernel (next_ray .. leaf_wait as launch_trace_persistent)
template <class S>
hipError_t launch_source(const TraceParams &p, const void *params, int src, bool any_hit, unsigned long long *next_ray, uint32_t *overflow,
		uint32_t lds_depth, uint32_t refill, uint32_t leaf_wait, uint32_t blocks, hipStream_t stream);
// ---- prep_kernels.hip: what prepares a scene or a cast
hipError_t launch_build_rows4(const Dev4Node *nodes4, const TriHot *hot, const TriCold *cold, uint32_t n_nodes4, uint32_t n_tris,
		void *rows, hipStream_t stream);
hipError_t launch_build_rows(const DevNode *nodes, const TriHot *hot, const TriCold *cold, uint32_t n_nodes, uint32_t n_tris,
		void *rows, hipStream_t stream);
hipError_t launch_grid_rays(const TraceParams &p, mrt_ray32 *out, hipStream_t stream);
hipError_t launch_expand_tokens(const TraceParams &p, const uint32_t *tokens, hipStream_t stream);
hipError_t launch_detect_grid(const void *rays, uint32_t in_fmt, uint64_t count, uint32_t tile_w_log2,
		unsigned long long *scratch, uint32_t *out, uint32_t *host_out, hipStream_t stream);
hipError_t launch_morton_keys(const void *rays, uint32_t in_fmt, uint64_t count, uint32_t *keys, uint32_t *index, hipStream_t stream);
hipError_t launch_origin_dir_keys(const void *rays, uint32_t in_fmt, uint64_t count, const float lo[3], const float hi[3],
		uint32_t *keys, uint32_t *index, hipStream_t stream);
// ---- shade_kernels.hip: the passes over hit records
// src = a SurfaceSrc; t (texture.h) / pano (panorama.h) null: no texture set / no panorama resident
// shading surfaces (surface_kernel.h); the rows of shade data given as device arrays (any of the three may be null)
hipError_t launch_resolve_surfaces(const TraceParams &p, const SurfaceParams &s, const TextureParams *t, int src, hipStream_t stream);
// direct light on resolved surfaces (light_kernel.h): over all lights, or with s.selected given the one light of each record
struct LightParams;
hipError_t launch_light_surfaces(const TraceParams &p, const LightParams &s, const PanoramaParams *pano, int src, hipStream_t stream);
// the path tracer's per-pixel state (path_kernel.h); white = Hable's white value for tone-map mode 2
struct PathParams;
hipError_t launch_path_init(mrt_path_state *state, uint64_t count, hipStream_t stream);
hipError_t launch_path_step(const TraceParams &p, const PathParams &s, const PanoramaParams *pano, int src, hipStream_t stream);
hipError_t launch_path_finish(const mrt_path_state *state, uint64_t count, uint32_t mode, float white, float *rgba, hipStream_t stream);
// emissive triangles as light sources: the step that leaves out emission a diffuse-lobe ray found (path_kernel.h) and the sampled
// point's diffuse term (emitter_light_kernel.h)
struct EmitterLightParams;
hipError_t launch_path_step_emitters(const TraceParams &p, const PathParams &s, const PanoramaParams *pano, const uint8_t *prev_lobe, int src, hipStream_t stream);
hipError_t launch_light_emitter_surfaces(const TraceParams &p, const EmitterLightParams &s, int src, hipStream_t stream);
hipError_t launch_pack_shade_rows(const uint32_t *ids, const float *normals9, const float *uvs6, uint32_t n_tris, void *rows, hipStream_t stream);
// the renderer's channels (channel_kernel.h): src = a SurfaceSrc, t all zero with no texture set resident; the lit frame's last pass
// and the 8-bit image (path_frame_kernel.h)
hipError_t launch_shade_channels(const TraceParams &p, const ChannelParams &c, const TextureParams &t, int src, hipStream_t stream);
hipError_t launch_finish_color(const float *lit, uint64_t count, uint32_t mode, float white, float *rgba, uint8_t *rgba8, hipStream_t stream);
hipError_t launch_image_to_rgba8(const float *rgba, uint64_t count, uint8_t *rgba8, hipStream_t stream);
// the running mean of progressive frames (accum_kernel.h): kind = an MRT_ACCUM_SRC_*, first: n_prior == 0, inv = 1 / (n_prior + 1)
hipError_t launch_accumulate(int kind, bool first, const void *source, uint64_t count, uint32_t mode, float white, float inv, float *accum,
		uint8_t *rgba8, hipStream_t stream);
// the reflection effect's image passes (denoise_kernel.h): fused = spatial, temporal and composite in one launch (out optional)
namespace dn { struct DenoiseArgs; }
hipError_t launch_denoise(bool fused, const dn::DenoiseArgs &a, const float *reflection, const float *depth, const float *guide, float *history,
		float *color, float *out, hipStream_t stream);
hipError_t launch_denoise_temporal(const dn::DenoiseArgs &a, const float *current, const float *history, float *out, hipStream_t stream);
hipError_t launch_composite(const dn::DenoiseArgs &a, const float *reflection, const float *depth, const float *guide, float *color, hipStream_t stream);
hipError_t launch_reflection_guides(const mrt_hit32 *hits, const mrt_surface64 *rows, uint64_t count, float inv_depth_range, float *depth,
		float *guide, hipStream_t stream);
// the reflection image of a G-buffer cast (gbuffer_image_kernel.h): s = the frame and its G-buffer (out_rays and max_distance unused)
hipError_t launch_reflection_image(const GBufferParams &s, const mrt_hit32 *hits, const float *lit, float *out, hipStream_t stream);
// the SVGF pass chain (svgf_kernel.h); kind = MRT_ACCUM_SRC_RGBA or _PATH_STATE; spatial: atrous ? pass 4 at a.step : pass 3
namespace sv { struct SvgfArgs; }
hipError_t launch_svgf_guides(int kind, const mrt_ray32 *rays, const mrt_hit32 *hits, const mrt_surface64 *rows, const void *source, uint64_t count,
		float *illum, float *albedo, float *normal_depth, float *position, hipStream_t stream);
hipError_t launch_svgf_temporal(const sv::SvgfArgs &a, const float *illum, const float *normal_depth, const float *position, const float *prev_illum,
		const float *prev_moments, const float *prev_normal_depth, const float *prev_position, float *out_illum, float *out_moments, hipStream_t stream);
hipError_t launch_svgf_spatial(bool atrous, const sv::SvgfArgs &a, const float *illum, const float *moments, const float *normal_depth,
		const float *position, float *out, hipStream_t stream);
hipError_t launch_svgf_modulate(const sv::SvgfArgs &a, const float *illum, const float *albedo, float *rgba, uint8_t *rgba8, hipStream_t stream);
// ---- device_build.hip
hipError_t grow_arena(BuildArena *arena, size_t need, hipStream_t stream); // hipErrorOutOfMemory: no allocation, the arena is empty
hipError_t launch_collapse4(const DevNode *nodes, uint32_t n_nodes, Dev4Node *nodes4, hipStream_t stream);
hipError_t launch_collapse8(const DevNode *nodes, uint32_t n_nodes, Dev8Node *nodes8, float *leaf_box, uint32_t *bad, hipStream_t stream);
hipError_t launch_offset_refs(DevNode *dst, const DevNode *src, uint32_t n, uint32_t node_base, uint32_t tri_base, void *stream);
hipError_t launch_offset_refs8(Dev8Node *dst, const Dev8Node *src, uint32_t n, uint32_t node_base, uint32_t tri_base, void *stream);
hipError_t launch_flatten_instances(const float *d_verts9, const mrt_instance *d_instances, const uint32_t *d_first_out,
		uint32_t n_instances, uint32_t max_tris_per_instance, mrt_tri64 *d_out, void *stream);
}

struct DevBuf {
	void *ptr = nullptr;
	size_t cap = 0;
};

struct mrt_ctx {
	int device = 0;
	mrt_options opts{};
	mrt::Knobs knobs;            // read from the environment by mrt_create
	hipStream_t own_stream = nullptr;
	hipStream_t stream = nullptr;
	hipEvent_t ev[6] = {};
	char err[512] = {0};
	// scene
	mrt::DevNode *d_nodes = nullptr; mrt::TriHot *d_hot = nullptr; mrt::TriCold *d_cold = nullptr;
	mrt::Dev4Node *d_nodes4 = nullptr; uint32_t n_nodes4 = 0;
	mrt::Dev8Node *d_nodes8 = nullptr; uint32_t n_nodes8 = 0, stack8 = 0;
	float *d_leaf_box = nullptr; // exact leaf boxes that go with d_nodes8
	mrt::BuildArena build_arena; // temporaries of the device builder, kept between builds (and of the refit)
	// flat scenes, for mrt_refit_scene (refit.hip): slot k of d_hot / d_cold holds input triangle d_slot_src[k] (every flat-scene path
	// writes it); d_parent, made by the first refit and kept: every node's parent, | 1 << 31 for a right child, 0xFFFFFFFF for the root
	uint32_t *d_slot_src = nullptr, *d_parent = nullptr;
	void *d_rows4 = nullptr;     // flat scenes with the 4-wide layout: 128-byte node rows + triangle rows (packet_quad_kernel.h)
	void *d_rows = nullptr;      // flat scenes: nodes + triangles as one array of 64-byte rows (packet_rows_kernel.h)
	// two-level scene: d_nodes = TLAS + every BLAS, d_hot / d_cold = mesh-space triangles, d_instances in TLAS leaf order
	mrt::DevInstance *d_instances = nullptr;
	mrt::TwoLevelHost *two_level = nullptr; // host copy kept for mrt_update_instances
	float bounds_lo[3] = {0, 0, 0}, bounds_hi[3] = {0, 0, 0};
	uint32_t n_nodes = 0, n_tris = 0, depth = 0, stack_depth = 0, stack4 = 0;
	bool scene = false;
	// per-dispatch buffers (grow only, x1.5: gpu_ray_caster.cpp:776-817)
	DevBuf rays, hits, keys_in, keys_out, idx_in, idx_out, sort_tmp, overflow;
	DevBuf refit_in;               // a refit's triangles, staged from the host or flattened from instances
	// top levels built on the device (tlas_device.hip): the scratch of one update (staged instances, registration rows, world boxes,
	// status block; grow only) and the scene's tables, made from two_level on first use: per instance {its mesh, flat id base}, per mesh
	// {range, roots, box}.  The mesh table goes stale when a refit moves the meshes (tlas_blas_ok = false); free_scene drops both.
	DevBuf tlas_work, tlas_inst_tab, tlas_blas_tab;
	bool tlas_inst_ok = false, tlas_blas_ok = false;
	int cu_count = 256;
	unsigned long long *d_counters = nullptr;
	// what detect_grid_kernel decided, also written to this host-mapped word block {row width, rows, tiles_x, verdict}
	// so that the host knows after the stream sync which of the two queued kernels did the work (no extra copy)
	uint32_t *h_auto = nullptr, *d_auto_host = nullptr;
	// small host-array casts (RayDispatcher::cast_ray / any_hit: one ray; tiles of a few hundred rays): rays and hits go
	// through two pinned, device-mapped buffers instead of two DMA copies (mrt_cast)
	void *h_small_in = nullptr, *d_small_in = nullptr, *h_small_out = nullptr, *d_small_out = nullptr;
	// Frame-coherent tile schedule of grid casts: what every schedule unit (one 8x8 tile, or the two of a 128-ray wave)
	// cost in the last cast of this grid, and the launch order made of it (longest first); see schedule_grid().
	struct TileSchedule {
		uint32_t grid_w = 0, grid_h = 0, y0 = 0, rows = 0, unit = 0, n_units = 0, tile_w_log2 = 0; bool pieces = false;
		// two generations: frame f notes its costs in cost[f & 1] and the side stream sorts them into order[f & 1] while frame
		// f + 1 (launched in the order of frame f - 1) already runs: back-to-back frames never wait for a sort
		uint32_t frame = 0, gen = 0;       // frames of this grid, sorts issued for it
		bool measuring = false;            // this frame notes its costs (and is sorted afterwards)
		bool have_order[2] = {false, false};
		DevBuf cost[2], order[2], cost_sorted, iota, tmp;
		DevBuf slots[2], hdr[2];           // what is launched: the order with its most expensive units in pieces (schedule_split)
		uint32_t n_slots_max = 0;
		hipStream_t side = nullptr;
		hipEvent_t traced = nullptr, ready[2] = {nullptr, nullptr};
		void forget() { have_order[0] = have_order[1] = false; }
	};
	mrt::DetectMemo detect;           // what the last detect found, for how many rays, as of the last wait (launch_policy.h)
	// per grid and cast mode, for the last few of them (mrt::GridStates): how it is cast, and its tile schedule in sched[same index]
	mrt::GridStates grids;
	TileSchedule sched[mrt::GridStates::kCount];
	uint64_t sched_counts[3] = {0, 0, 0}; // mrt_schedule_counts: casts under the schedule, those launched in a measured order, sorts queued
	char queued_variant[96] = "", queued_alt_variant[96] = "", last_variant[96] = ""; // instantiation names (mrt_last_kernel_variant)
	uint32_t queued_kernel = 0, queued_alt_kernel = 0; bool queued_detect = false; // what the last cast put on the stream
	// host-array pipeline (cast_host_pipelined): copy streams and per-chunk events, created on first use
	hipStream_t up_stream = nullptr, dn_stream = nullptr;
	std::vector<hipEvent_t> pipe_ev;
	// async state
	bool pending = false;
	uint64_t pending_count = 0; uint32_t pending_flags = 0; int pending_mode = 0;
	const void *pending_dev_hits = nullptr;
	mrt_stats stats{};
	// shade data (surface.hip): the context's, not the scene's -- free_scene leaves it alone
	DevBuf shade_rows, shade_materials;
	uint32_t shade_n_tris = 0, shade_n_materials = 0, shade_present = 0; // present: mrt::SHADE_HAS_* (shade_data.h)
	// texture set (texture.hip): the context's, like the shade data; tex_resident: the resolves launch the textured kernel
	DevBuf tex_texels, tex_table, tex_bindings, tex_tangents;
	uint32_t tex_n_bindings = 0, tex_n_tangent_tris = 0; // (no tangents resident: 0)
	bool tex_resident = false;
	// panorama (panorama.hip): the context's, like the texture set; pano_resident: the lighting calls with an environment and the path
	// steps launch the panorama kernels
	DevBuf pano_texels;
	uint32_t pano_width = 0, pano_height = 0;
	float pano_energy = 0.0f;
	bool pano_resident = false;
	// emitter table (emitters.hip): the context's, like the shade data; emit_n rows and CDF words, emit_total = the last CDF word
	DevBuf emit_rows, emit_cdf, emit_in, emit_work;
	uint32_t emit_n = 0, emit_total = 0;
};

#define HIP_TRY(ctx, call)                                                                          \
	do {                                                                                            \
		hipError_t e_ = (call);                                                                     \
		if (e_ != hipSuccess) {                                                                     \
			std::snprintf((ctx)->err, sizeof((ctx)->err), "%s failed: %s (%s:%d)", #call,           \
					hipGetErrorString(e_), __FILE__, __LINE__);                                      \
			return MRT_ERR_HIP;                                                                     \
		}                                                                                           \
	} while (0)

inline int fail(mrt_ctx *ctx, int code, const char *msg)
{
	if (ctx) std::snprintf(ctx->err, sizeof(ctx->err), "%s", msg);
	return code;
}

inline int ensure(mrt_ctx *ctx, DevBuf &b, size_t bytes)
{
	if (b.cap >= bytes) return MRT_OK;
	size_t want = bytes + bytes / 2; // grow x1.5
	if (b.ptr) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); HIP_TRY(ctx, hipFree(b.ptr)); b.ptr = nullptr; b.cap = 0; }
	hipError_t e = hipMalloc(&b.ptr, want);
	if (e != hipSuccess) { want = bytes; e = hipMalloc(&b.ptr, want); }
	if (e != hipSuccess) { b.ptr = nullptr; return fail(ctx, MRT_ERR_OOM, "device allocation failed"); }
	b.cap = want;
	return MRT_OK;
}

inline void release(DevBuf &b) { if (b.ptr) (void)hipFree(b.ptr); b.ptr = nullptr; b.cap = 0; }

// tlas_device.hip: the top level of the resident two-level scene built on the device from n instances (a device array, or a host array
// staged with one copy; form: 0 radix tree, 1 PLOC, 2 binned SAH) and committed, or refused with the scene unchanged; check_only: the
// per-instance checks alone (mesh ranges, transforms), nothing built.  On the context's stream, blocks until done; *ms = its device
// time.  Does not drain a pending dispatch.
namespace mrt {
int device_update_tlas(mrt_ctx *ctx, const mrt_instance *instances, uint32_t n, bool on_device, int form, bool check_only, float *ms);
}

// api.hip
void free_scene(mrt_ctx *ctx);
size_t ray_stride(uint32_t flags);
size_t hit_stride(const mrt_ctx *ctx, uint32_t flags, int mode);
uint32_t out_format(const mrt_ctx *ctx, uint32_t flags, int mode);
void base_params(mrt_ctx *ctx, mrt::TraceParams &p);
int grid_params(mrt_ctx *ctx, const mrt_camera *cam, uint32_t grid_w, uint32_t grid_h, uint32_t y0, uint32_t y1, mrt::TraceParams &p);
// The rays of a call over hit records (surface.hip, lighting.hip, path.hip) that are an array, not a grid: p for count rays at d_rays in
// the layout flags names (no scene: nothing is walked); returns the SurfaceSrc.
inline int record_params(const void *d_rays, uint64_t count, uint32_t flags, mrt::TraceParams &p)
{
	std::memset(&p, 0, sizeof(p));
	p.rays = d_rays; p.count = count;
	const bool host = (flags & MRT_FLAG_HOST_LAYOUT) != 0;
	p.in_fmt = host ? mrt::IN_HOST60 : mrt::IN_RAY32;
	return host ? mrt::SURF_HOST : mrt::SURF_RAY32;
}
// The opening of such a call after its own checks (returns from the call like HIP_TRY): a pending dispatch is refused, no records is
// MRT_OK, else the device is selected.
#define BEGIN_PASS(ctx, count)                                                                             \
	do {                                                                                                   \
		if ((ctx)->pending) return fail((ctx), MRT_ERR_PENDING, "collect the pending dispatch first");     \
		if ((count) == 0) return MRT_OK;                                                                   \
		HIP_TRY((ctx), hipSetDevice((ctx)->device));                                                       \
	} while (0)
// ... and the end of such a call, its pass queued: back at once for MRT_FLAG_ASYNC, else when the stream is done
inline int finish_call(mrt_ctx *ctx, uint32_t flags)
{
	if (flags & MRT_FLAG_ASYNC) return MRT_OK;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return MRT_OK;
}
// What the context holds resident, as the kernels' parameter blocks take it: the shade data into the fields SurfaceParams and
// ChannelParams share, the texture set (all zero with none resident: no binding applies) and the panorama.
template <class S>
inline void shade_data_params(const mrt_ctx *ctx, S &s)
{
	s.shade_rows = ctx->shade_rows.ptr; s.materials = ctx->shade_materials.ptr;
	s.n_tris = ctx->shade_n_tris; s.n_materials = ctx->shade_n_materials; s.present = ctx->shade_present;
}
inline mrt::TextureParams texture_params(const mrt_ctx *ctx)
{
	mrt::TextureParams t;
	std::memset(&t, 0, sizeof(t));
	if (ctx->tex_resident) {
		t.texels = ctx->tex_texels.ptr; t.table = ctx->tex_table.ptr; t.bindings = ctx->tex_bindings.ptr;
		t.tangents = ctx->tex_n_tangent_tris ? ctx->tex_tangents.ptr : nullptr;
		t.n_bindings = ctx->tex_n_bindings; t.n_tangent_tris = ctx->tex_n_tangent_tris;
	}
	return t;
}
inline mrt::EmitterTable emitter_table(const mrt_ctx *ctx)
{
	return {ctx->emit_n ? ctx->emit_rows.ptr : nullptr, ctx->emit_n ? (const uint32_t *)ctx->emit_cdf.ptr : nullptr, ctx->emit_n, ctx->emit_total};
}
inline mrt::PanoramaParams panorama_params(const mrt_ctx *ctx)
{
	return {ctx->pano_texels.ptr, ctx->pano_width, ctx->pano_height, ctx->pano_energy, 0u};
}
// schedule.hip: before the launch of a scheduled cast (fills p's schedule fields), after it (ev[4] recorded)
int schedule_grid(mrt_ctx *ctx, const mrt::CastPlan &c, mrt::TraceParams &p);
int schedule_sort(mrt_ctx *ctx);
