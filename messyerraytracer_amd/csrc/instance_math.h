// instance_math.h -- the per-instance arithmetic of a two-level scene (BLASInstance, src/accel/blas_instance.h:47-107), shared by the
// host path (two_level_prep.cpp: mrt_update_instances, uploads, refits) and the device top-level build (tlas_device.hip), so that
// both write the same DevInstance rows and world boxes bit for bit.  Every operation is spelled out in the order it is evaluated and
// nothing is contracted into an fma; double division and the double -> float conversion round to nearest on the host and on the
// device alike.  csrc/host/instance_math_test.cpp holds both functions to the host path's earlier text on random and edge cases.
#pragma once
#include <cmath>
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define MRT_HD __host__ __device__
#else
#define MRT_HD
#endif

namespace mrt {

// Inverse of the affine map x -> B x + o in double (cofactors), rounded once to float: inv = rows {m00 m01 m02 tx}.
// false if B is singular or a value is not finite (inv is then partly written).
MRT_HD inline bool invert_affine(const float basis[9], const float origin[3], float inv[12])
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
	const double a = basis[0], b = basis[1], c = basis[2], d = basis[3], e = basis[4], f = basis[5], g = basis[6], h = basis[7], i = basis[8];
	const double c00 = e * i - f * h, c01 = c * h - b * i, c02 = b * f - c * e;
	const double c10 = f * g - d * i, c11 = a * i - c * g, c12 = c * d - a * f;
	const double c20 = d * h - e * g, c21 = b * g - a * h, c22 = a * e - b * d;
	const double det = a * c00 + b * c10 + c * c20;
	if (!(fabs(det) > 0.0) || !__builtin_isfinite(det)) return false;
	const double m[9] = { c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det };
	for (int r = 0; r < 3; r++) {
		const double t = -(m[3 * r] * (double)origin[0] + m[3 * r + 1] * (double)origin[1] + m[3 * r + 2] * (double)origin[2]);
		inv[4 * r] = (float)m[3 * r]; inv[4 * r + 1] = (float)m[3 * r + 1]; inv[4 * r + 2] = (float)m[3 * r + 2]; inv[4 * r + 3] = (float)t;
		if (!__builtin_isfinite(inv[4 * r]) || !__builtin_isfinite(inv[4 * r + 1]) || !__builtin_isfinite(inv[4 * r + 2]) || !__builtin_isfinite(inv[4 * r + 3])) return false;
	}
	return true;
}

// World box of a mesh box under x -> B x + o: the eight corners (BLASInstance::compute_world_bounds, blas_instance.h:76-107),
// evaluated in double and rounded outwards to float so that the box still contains the exact image.
MRT_HD inline void world_box(const float lo[3], const float hi[3], const float basis[9], const float origin[3], float wlo[3], float whi[3])
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
	double mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
	for (int k = 0; k < 8; k++) {
		const double x = (k & 1) ? hi[0] : lo[0], y = (k & 2) ? hi[1] : lo[1], z = (k & 4) ? hi[2] : lo[2];
		for (int r = 0; r < 3; r++) {
			const double w = ((double)basis[3 * r] * x + (double)basis[3 * r + 1] * y) + (double)basis[3 * r + 2] * z + (double)origin[r];
			if (w < mn[r]) mn[r] = w;
			if (w > mx[r]) mx[r] = w;
		}
	}
	for (int r = 0; r < 3; r++) {
		float l = (float)mn[r], u = (float)mx[r];
		if ((double)l > mn[r]) l = nextafterf(l, -INFINITY);
		if ((double)u < mx[r]) u = nextafterf(u, INFINITY);
		wlo[r] = l; whi[r] = u;
	}
}

} // namespace mrt
