// dispatch.h — host helpers of the kernel units (kernels.hip, shade_kernels.hip, prep_kernels.hip): runtime values as template
// arguments, and the launch of a pass with one thread per entry.  Included inside namespace mrt, after <type_traits> and the HIP
// runtime; MRT_WG is device_common.h's.
#pragma once

// Runtime values as template arguments.  dispatch(f, Among<Vs...>{v}, ...) calls f(std::integral_constant...) with, for every
// Among, the one of its Vs that equals its v (none: f is not called).  The first Among varies slowest, and the instantiations f
// makes are emitted in that order: the launchers of kernels.hip list theirs so that the code object keeps its kernels where they were.
template <auto... Vs> struct Among { std::common_type_t<decltype(Vs)...> v; };
using Bool = Among<true, false>;
template <class F> static void dispatch(F &&f) { f(); }
template <class F, auto... Vs, class... Rest>
static void dispatch(F &&f, Among<Vs...> first, Rest... rest)
{
	(void)(... || (first.v == Vs && (dispatch([&](auto... cs) { f(std::integral_constant<decltype(Vs), Vs>{}, cs...); }, rest...), true)));
}

// One thread per entry, MRT_WG threads per block; no entries: nothing is launched.  LIMIT: more than 2^31 - 1 blocks is
// hipErrorInvalidValue (without it the count is the caller's to bound, as it always was for the launchers that say so).
template <bool LIMIT, class Kernel, class... Args>
static hipError_t launch_per_entry(Kernel kernel, uint64_t count, hipStream_t stream, const Args &...args)
{
	if (count == 0) return hipSuccess;
	const uint64_t blocks = (count + MRT_WG - 1) / MRT_WG;
	if (LIMIT && blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
	hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(MRT_WG), 0, stream, args...);
	return hipGetLastError();
}

// A per-record pass that reads its rays from one of the three SurfaceSrc: pick(SRC) names the kernel.  Any other src is
// hipErrorInvalidValue (but no records: nothing to refuse).
template <class Pick, class... Args>
static hipError_t launch_surface_pass(Pick pick, int src, const TraceParams &p, hipStream_t stream, const Args &...args)
{
	hipError_t e = p.count ? hipErrorInvalidValue : hipSuccess;
	dispatch([&](auto SRC) { e = launch_per_entry<true>(pick(SRC), p.count, stream, p, args...); },
			Among<SURF_RAY32, SURF_HOST, SURF_GRID>{(SurfaceSrc)src});
	return e;
}
