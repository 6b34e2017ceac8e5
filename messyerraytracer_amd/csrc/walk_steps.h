// walk_steps.h -- the steps of a one-ray walk, one text each: the reciprocal set of a ray, the slab test of a box, the
// triangle test, the acceptance rule with its tie break and a ray's way into an instance's mesh space.  Shared by the token expansion
// (prep_kernels.hip) and the host walkers (host/cpu_backend.hpp); fma_, dot3 and safe_inv by every kernel unit.  The lane walks and the C++ packet walks state the same arithmetic in their own text, as the
// inline-assembly walks do: DESIGN.md 4.2a has the timings and register counts that keep them there.  This is the canonical form of
// DESIGN.md ("Arithmetic"): compiled with -ffp-contract=off, every fused operation an explicit __builtin_fmaf, every expression tree in
// the order of oracle/mrt_oracle.c, so that host and device give the same bits.  host/walk_steps_test.cpp holds every step to the oracle.
// A point, a vector, a box corner or a row is anything with float members x, y, z (and w): a float4 of a kernel, a V3 or V4 here,
// a Vector3 of the host types.
#pragma once
#include <cstdint>

#ifndef MRT_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define MRT_HD __host__ __device__
#else
#define MRT_HD
#endif
#endif
#define MRT_STEP MRT_HD inline __attribute__((always_inline))

namespace mrt {

struct V3 { float x, y, z; };
struct V4 { float x, y, z, w; };

MRT_STEP float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
MRT_STEP float dot3(float ax, float ay, float az, float bx, float by, float bz)
{
	return fma_(ax, bx, fma_(ay, by, az * bz));
}
// safe_inv_direction, bvh_traverse.comp.glsl:137-145 == Ray::_precompute, src/core/ray.h:78-89
MRT_STEP float safe_inv(float d)
{
	const float eps = 1e-9f;
	const float big = 1.0f / eps;
	return __builtin_fabsf(d) > eps ? 1.0f / d : (d >= 0.0f ? big : -big);
}

// What a slab test needs of a ray: (box - o) * inv is evaluated as fma(box, inv, -(o * inv)).
struct RayInv { float ix, iy, iz, nrx, nry, nrz; };
template <class O, class D>
MRT_STEP RayInv ray_inverse(const O &o, const D &d)
{
	RayInv k;
	k.ix = safe_inv(d.x); k.iy = safe_inv(d.y); k.iz = safe_inv(d.z);
	k.nrx = -(o.x * k.ix); k.nry = -(o.y * k.iy); k.nrz = -(o.z * k.iz);
	return k;
}

// ray_aabb, glsl:84-99, clamped to [t_min, lim]: whether the ray passes the box, and where it enters.
template <class L, class H>
MRT_STEP bool slab_box(const L &lo, const H &hi, const RayInv &k, float t_min, float lim, float &tnear)
{
	const float x0 = fma_(lo.x, k.ix, k.nrx), x1 = fma_(hi.x, k.ix, k.nrx);
	const float y0 = fma_(lo.y, k.iy, k.nry), y1 = fma_(hi.y, k.iy, k.nry);
	const float z0 = fma_(lo.z, k.iz, k.nrz), z1 = fma_(hi.z, k.iz, k.nrz);
	tnear = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(x0, x1), __builtin_fminf(y0, y1)), __builtin_fmaxf(__builtin_fminf(z0, z1), t_min));
	const float tfar = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(x0, x1), __builtin_fmaxf(y0, y1)), __builtin_fminf(__builtin_fmaxf(z0, z1), lim));
	return tnear <= tfar;
}
// Both children of a 64-byte node {lmin, lref | lmax, rref | rmin, . | rmax, .}.
template <class R>
MRT_STEP void slab_pair(const R &a, const R &b, const R &c, const R &d, const RayInv &k, float t_min, float lim, bool &hl, float &tl, bool &hr, float &tr)
{
	hl = slab_box(a, b, k, t_min, lim, tl);
	hr = slab_box(c, d, k, t_min, lim, tr);
}

// ray_triangle, glsl:105-131 == Triangle::intersect, src/core/triangle.h:56-105 (Moller-Trumbore; q0 = v0, q1 = edge1, q2 = edge2).
// REJECT: the walk's form, false as soon as the ray is parallel to the triangle or (u, v) lies outside it.  Without it every value is
// worked out whatever comes of it: what rebuilds the record of a hit that a walk has accepted (prep_kernels.hip).
template <bool REJECT, class O, class D, class Q0, class Q1, class Q2>
MRT_STEP bool tri_solve(const O &o, const D &d, const Q0 &q0, const Q1 &q1, const Q2 &q2, float &t, float &u, float &v)
{
	const float pvx = fma_(d.y, q2.z, -(d.z * q2.y));
	const float pvy = fma_(d.z, q2.x, -(d.x * q2.z));
	const float pvz = fma_(d.x, q2.y, -(d.y * q2.x));
	const float det = dot3(q1.x, q1.y, q1.z, pvx, pvy, pvz);
	if (REJECT && __builtin_fabsf(det) < 1e-8f) return false;
	const float inv_det = 1.0f / det;
	const float tvx = o.x - q0.x, tvy = o.y - q0.y, tvz = o.z - q0.z;
	u = dot3(tvx, tvy, tvz, pvx, pvy, pvz) * inv_det;
	if (REJECT && (u < 0.0f || u > 1.0f)) return false;
	const float qvx = fma_(tvy, q1.z, -(tvz * q1.y));
	const float qvy = fma_(tvz, q1.x, -(tvx * q1.z));
	const float qvz = fma_(tvx, q1.y, -(tvy * q1.x));
	v = dot3(d.x, d.y, d.z, qvx, qvy, qvz) * inv_det;
	if (REJECT && (v < 0.0f || u + v > 1.0f)) return false;
	t = dot3(q2.x, q2.y, q2.z, qvx, qvy, qvz) * inv_det;
	return true;
}
template <class O, class D, class Q0, class Q1, class Q2>
MRT_STEP bool tri_hit(const O &o, const D &d, const Q0 &q0, const Q1 &q1, const Q2 &q2, float &t, float &u, float &v)
{
	return tri_solve<true>(o, d, q0, q1, q2, t, u, v);
}
template <class O, class D, class Q0, class Q1, class Q2>
MRT_STEP void tri_tuv(const O &o, const D &d, const Q0 &q0, const Q1 &q1, const Q2 &q2, float &t, float &u, float &v)
{
	tri_solve<false>(o, d, q0, q1, q2, t, u, v);
}

// glsl:124 accepts t_min <= t < lim (lim = the best hit so far, or the ray's t_max); an exact tie goes to the lower triangle id, so
// that the answer does not depend on the order triangles are visited in.  best_slot = 0xFFFFFFFF: no hit yet (lim is then t_max,
// which no hit may equal).
MRT_STEP bool closer_hit(float t, uint32_t id, float t_min, float lim, uint32_t best_slot, uint32_t best_id)
{
	return !(t < t_min) && (t < lim || (t == lim && best_slot != 0xFFFFFFFFu && id < best_id));
}

// World ray -> the mesh space of an instance whose inverse transform has the rows m0, m1, m2 = {M row, t}: o' = M o + t, d' = M d,
// not renormalised, so t stays world-parameterised (blas_instance.h:56-66, tiny_bvh.h:3327-3331).
template <class M, class O, class D>
MRT_STEP void to_instance_space(const M &m0, const M &m1, const M &m2, const O &o, const D &d, V3 &oi, V3 &di)
{
	oi.x = fma_(m0.x, o.x, fma_(m0.y, o.y, fma_(m0.z, o.z, m0.w)));
	oi.y = fma_(m1.x, o.x, fma_(m1.y, o.y, fma_(m1.z, o.z, m1.w)));
	oi.z = fma_(m2.x, o.x, fma_(m2.y, o.y, fma_(m2.z, o.z, m2.w)));
	di.x = fma_(m0.x, d.x, fma_(m0.y, d.y, m0.z * d.z));
	di.y = fma_(m1.x, d.x, fma_(m1.y, d.y, m1.z * d.z));
	di.z = fma_(m2.x, d.x, fma_(m2.y, d.y, m2.z * d.z));
}

} // namespace mrt
