// walk_steps_test.cpp -- walk_steps.h (compiled for the host here; for the device in prep_kernels.hip) against the
// project's oracle, bit for bit: oracle/mrt_oracle.c is compiled into this driver, so safe_inv, slab and tri_hit below are the
// oracle's own functions; what the oracle writes inline (the reciprocal set, a ray's way into an instance)
// is quoted from it with its line.  Random inputs and the edges a walk can meet: det at +-1e-8 and one ulp to each side, (u, v) on
// the triangle's three edges and one ulp outside, t == t_min, t == best_t with a lower, an equal and a higher id with and without a
// hit before, boxes touched exactly at t_min and at the limit, zero direction components, the +inf point box of an unused 4-wide
// slot against FLT_MAX, mirrored and sheared instance rows.  Floats are compared with memcmp; the one exception is the sign of a zero
// entry distance (same_t below).
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../walk_steps.h"

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../../oracle/mrt_oracle.c" // (written to compile as C++ too; its static functions are the reference here)

namespace {

using mrt::RayInv;
using mrt::V3;
using mrt::V4;

long g_checks = 0, g_fails = 0;

bool same(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }
void check(bool ok, const char *what, long i)
{
	g_checks++;
	if (!ok) { g_fails++; std::printf("FAIL %s (case %ld)\n", what, i); }
}
// an entry distance: fminf and fmaxf leave the sign of min(-0, +0) open (the oracle's calls as much as these), and no walk reads it
bool same_t(float a, float b) { return same(a, b) || (a == 0.0f && b == 0.0f); }
float up(float x) { return std::nextafterf(x, INFINITY); }
float down(float x) { return std::nextafterf(x, -INFINITY); }

// the oracle's reciprocal set: trace_one, mrt_oracle.c:382-383
void orc_inverse(const float o[3], const float d[3], float inv[3], float nro[3])
{
	for (int k = 0; k < 3; k++) { inv[k] = safe_inv(d[k]); nro[k] = -(o[k] * inv[k]); }
}

void check_inverse(const float o[3], const float d[3], long i)
{
	float inv[3], nro[3];
	orc_inverse(o, d, inv, nro);
	const RayInv k = mrt::ray_inverse(V3{ o[0], o[1], o[2] }, V3{ d[0], d[1], d[2] });
	check(same(k.ix, inv[0]) && same(k.iy, inv[1]) && same(k.iz, inv[2]) && same(k.nrx, nro[0]) && same(k.nry, nro[1]) && same(k.nrz, nro[2]),
			"ray_inverse", i);
	for (int a = 0; a < 3; a++) check(same(mrt::safe_inv(d[a]), safe_inv(d[a])), "safe_inv", i);
}

// slab_box and slab_pair against slab();
// expect: 1 = must pass, 0 = must miss, -1 = whatever the oracle says
void check_box(const float o[3], const float d[3], const float lo[3], const float hi[3], float t_min, float lim, int expect, long i)
{
	float inv[3], nro[3], want_t = 0.0f, got_t = 0.0f;
	orc_inverse(o, d, inv, nro);
	const bool want = slab(lo, hi, inv, nro, t_min, lim, &want_t) != 0;
	const RayInv k = mrt::ray_inverse(V3{ o[0], o[1], o[2] }, V3{ d[0], d[1], d[2] });
	const V3 l = { lo[0], lo[1], lo[2] }, h = { hi[0], hi[1], hi[2] };
	const bool got = mrt::slab_box(l, h, k, t_min, lim, got_t);
	check(got == want && same_t(got_t, want_t), "slab_box", i);
	if (expect >= 0) check(want == (expect != 0), "slab_box: the case is the edge it was built to be", i);
	bool hl, hr; float tl = 0.0f, tr = 0.0f;
	mrt::slab_pair(l, h, h, l, k, t_min, lim, hl, tl, hr, tr); // (the right child: the same box with its corners swapped)
	float swapped_t = 0.0f;
	const bool swapped = slab(hi, lo, inv, nro, t_min, lim, &swapped_t) != 0;
	check(hl == want && same_t(tl, want_t) && hr == swapped && same_t(tr, swapped_t), "slab_pair", i);
}

// tri_hit && closer_hit against tri_hit() of the oracle; tri_tuv against both.  expect as in check_box.
void check_tri(const float o[3], const float d[3], const orc_tri64 &tri, float t_min, float best_t, bool have_hit, uint32_t best_id, int expect, long i)
{
	float wt = 0.0f, wu = 0.0f, wv = 0.0f, t = 0.0f, u = 0.0f, v = 0.0f;
	const bool want = tri_hit(&tri, o, d, t_min, best_t, have_hit ? 1 : 0, best_id, &wt, &wu, &wv) != 0;
	const V3 O = { o[0], o[1], o[2] }, D = { d[0], d[1], d[2] };
	const V3 q0 = { tri.v0[0], tri.v0[1], tri.v0[2] }, q1 = { tri.edge1[0], tri.edge1[1], tri.edge1[2] }, q2 = { tri.edge2[0], tri.edge2[1], tri.edge2[2] };
	const uint32_t best_slot = have_hit ? 7u : 0xFFFFFFFFu;
	const bool inside = mrt::tri_hit(O, D, q0, q1, q2, t, u, v);
	const bool got = inside && mrt::closer_hit(t, tri.id, t_min, best_t, best_slot, best_id);
	check(got == want && (!want || (same(t, wt) && same(u, wu) && same(v, wv))), "tri_hit && closer_hit", i);
	if (expect >= 0) check(want == (expect != 0), "tri_hit: the case is the edge it was built to be", i);
	// tri_tuv on every triangle, rejected or not: tri_hit() of the oracle (mrt_oracle.c:345-356) with its returns taken out
	float pvec[3], tvec[3], qvec[3], t2 = 0.0f, u2 = 0.0f, v2 = 0.0f;
	v_cross(d, tri.edge2, pvec);
	const float inv_det = 1.0f / v_dot(tri.edge1, pvec);
	tvec[0] = o[0] - tri.v0[0]; tvec[1] = o[1] - tri.v0[1]; tvec[2] = o[2] - tri.v0[2];
	const float eu = v_dot(tvec, pvec) * inv_det;
	v_cross(tvec, tri.edge1, qvec);
	const float ev = v_dot(d, qvec) * inv_det, et = v_dot(tri.edge2, qvec) * inv_det;
	mrt::tri_tuv(O, D, q0, q1, q2, t2, u2, v2);
	check(same(t2, et) && same(u2, eu) && same(v2, ev), "tri_tuv", i);
	if (inside) check(same(t2, t) && same(u2, u) && same(v2, v), "tri_tuv against tri_hit", i);
}

orc_tri64 make_tri(float v0x, float v0y, float v0z, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, uint32_t id)
{
	orc_tri64 t;
	std::memset(&t, 0, sizeof(t));
	t.v0[0] = v0x; t.v0[1] = v0y; t.v0[2] = v0z; t.edge1[0] = e1x; t.edge1[1] = e1y; t.edge1[2] = e1z;
	t.edge2[0] = e2x; t.edge2[1] = e2y; t.edge2[2] = e2z; t.id = id; t.layers = 0xFFFFFFFFu;
	return t;
}

// a ray's way into an instance: two_level_one, mrt_oracle.c:879-884
void check_instance(const float m[12], const float o[3], const float d[3], long i)
{
	const float oo[3] = { fmaf(m[0], o[0], fmaf(m[1], o[1], fmaf(m[2], o[2], m[3]))),
			fmaf(m[4], o[0], fmaf(m[5], o[1], fmaf(m[6], o[2], m[7]))),
			fmaf(m[8], o[0], fmaf(m[9], o[1], fmaf(m[10], o[2], m[11]))) };
	const float od[3] = { fmaf(m[0], d[0], fmaf(m[1], d[1], m[2] * d[2])),
			fmaf(m[4], d[0], fmaf(m[5], d[1], m[6] * d[2])),
			fmaf(m[8], d[0], fmaf(m[9], d[1], m[10] * d[2])) };
	V3 oi, di;
	mrt::to_instance_space(V4{ m[0], m[1], m[2], m[3] }, V4{ m[4], m[5], m[6], m[7] }, V4{ m[8], m[9], m[10], m[11] }, V3{ o[0], o[1], o[2] }, V3{ d[0], d[1], d[2] }, oi, di);
	check(same(oi.x, oo[0]) && same(oi.y, oo[1]) && same(oi.z, oo[2]) && same(di.x, od[0]) && same(di.y, od[1]) && same(di.z, od[2]), "to_instance_space", i);
	check_inverse(oo, od, i); // (the reciprocal set of the mesh-space ray, as a walk takes it next)
}

} // namespace

int main()
{
	std::mt19937 rng(20240917u);
	std::uniform_real_distribution<float> pos(-10.0f, 10.0f), unit(-1.0f, 1.0f), frac(0.0f, 1.0f);
	long c = 0;

	// ---- random rays, boxes, triangles, instance rows ----
	for (int i = 0; i < 20000; i++, c++) {
		const float o[3] = { pos(rng), pos(rng), pos(rng) };
		float d[3] = { unit(rng), unit(rng), unit(rng) };
		if (i % 7 == 0) d[i % 3] = 0.0f;
		if (i % 11 == 0) d[(i + 1) % 3] = -0.0f;
		const float a[3] = { pos(rng), pos(rng), pos(rng) }, e[3] = { 4.0f * frac(rng), 4.0f * frac(rng), 4.0f * frac(rng) };
		const float hi[3] = { a[0] + e[0], a[1] + e[1], a[2] + e[2] };
		const float t_min = i % 3 == 0 ? 0.0f : frac(rng), lim = i % 5 == 0 ? FLT_MAX : 30.0f * frac(rng);
		check_inverse(o, d, c);
		check_box(o, d, a, hi, t_min, lim, -1, c);
		// a triangle in front of the ray more often than not: around the point o + s d
		const float s = 20.0f * frac(rng);
		const orc_tri64 tri = make_tri(o[0] + s * d[0] + unit(rng), o[1] + s * d[1] + unit(rng), o[2] + s * d[2] + unit(rng),
				2.0f * unit(rng), 2.0f * unit(rng), 2.0f * unit(rng), 2.0f * unit(rng), 2.0f * unit(rng), 2.0f * unit(rng), (uint32_t)(i % 17));
		check_tri(o, d, tri, t_min, lim, i % 2 == 0, (uint32_t)(i % 13), -1, c);
		float m[12];
		for (int k = 0; k < 12; k++) m[k] = 2.0f * unit(rng);
		if (i % 4 == 1) { m[0] = -m[0]; m[4] = -m[4]; m[8] = -m[8]; }               // mirrored: the first column negated
		if (i % 4 == 2) { m[1] = m[0] * 0.75f + m[1]; m[5] = m[4] * 0.75f + m[5]; } // sheared
		if (i % 4 == 3) { m[0] = 1.0f; m[1] = 0.5f; m[2] = 0.0f; m[4] = 0.0f; m[5] = -1.0f; m[6] = 0.25f; m[8] = 0.0f; m[9] = 0.0f; m[10] = 1.0f; } // both
		check_instance(m, o, d, c);
	}

	// ---- safe_inv: zero, the threshold and its neighbours, the ends of the range ----
	const float eps = 1e-9f;
	const float ds[] = { 0.0f, -0.0f, eps, -eps, up(eps), down(eps), -up(eps), -down(eps), FLT_MIN, -FLT_MIN, FLT_TRUE_MIN, FLT_MAX, -FLT_MAX, INFINITY, -INFINITY, 1.0f, -1.0f };
	for (float dx : ds) for (float dy : { 0.0f, 1.0f, -0.0f }) {
		const float o[3] = { 1.5f, -2.0f, 0.0f }, d[3] = { dx, dy, -dx };
		check_inverse(o, d, c++);
		const float lo[3] = { -1.0f, -3.0f, -1.0f }, hi[3] = { 2.0f, 1.0f, 1.0f };
		check_box(o, d, lo, hi, 0.0f, FLT_MAX, -1, c++);
	}

	// ---- boxes touched exactly at t_min and at the limit: the ray runs along +x from the origin, the box spans x in [1, 2] ----
	{
		const float o[3] = { 0.0f, 0.0f, 0.0f }, d[3] = { 1.0f, 0.0f, 0.0f }, lo[3] = { 1.0f, -1.0f, -1.0f }, hi[3] = { 2.0f, 1.0f, 1.0f };
		check_box(o, d, lo, hi, 2.0f, 10.0f, 1, c++);        // leaves the box exactly at t_min
		check_box(o, d, lo, hi, up(2.0f), 10.0f, 0, c++);
		check_box(o, d, lo, hi, 0.0f, 1.0f, 1, c++);         // enters the box exactly at the limit
		check_box(o, d, lo, hi, 0.0f, down(1.0f), 0, c++);
		check_box(o, d, lo, hi, 1.0f, 1.0f, 1, c++);         // t_min == limit == the entry
		const float dn[3] = { -1.0f, 0.0f, -0.0f }, on[3] = { 3.0f, 0.0f, 0.0f };
		check_box(on, dn, lo, hi, 2.0f, 10.0f, 1, c++);      // the same from the other side: enters at 1, leaves at 2
		check_box(on, dn, lo, hi, 0.0f, 1.0f, 1, c++);
		check_box(on, dn, lo, hi, 0.0f, down(1.0f), 0, c++);
	}

	// ---- the point box at +inf of an unused 4-wide child slot against a finite limit: never entered ----
	{
		const float inf3[3] = { INFINITY, INFINITY, INFINITY };
		for (float dx : { 1.0f, -1.0f, 0.0f, -0.0f }) for (float dy : { 0.5f, -0.5f, 0.0f }) for (float t_min : { 0.0f, 1.0f }) {
			const float o[3] = { 1.0f, -2.0f, 3.0f }, d[3] = { dx, dy, -dx };
			check_box(o, d, inf3, inf3, t_min, FLT_MAX, 0, c++);
			check_box(o, d, inf3, inf3, t_min, fminf(5.0f, FLT_MAX), 0, c++);
		}
	}

	// ---- det exactly at +-1e-8 and one ulp to each side: d = (0, 0, 1), e2 = (0, 1, 0) give pvec = (-1, 0, 0), so det = -e1.x; the
	// origin is v0, so u = v = t = 0 and the triangle is hit exactly when det is not rejected ----
	{
		const float k = 1e-8f;
		const float dets[] = { k, up(k), down(k), -k, -up(k), -down(k), 0.0f, -0.0f };
		const int hit[] = { 1, 1, 0, 1, 1, 0, 0, 0 };
		for (int i = 0; i < 8; i++) {
			const float o[3] = { 0.25f, 0.5f, -1.0f }, d[3] = { 0.0f, 0.0f, 1.0f };
			const orc_tri64 tri = make_tri(o[0], o[1], o[2], -dets[i], 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 3u);
			check_tri(o, d, tri, 0.0f, 100.0f, false, 0xFFFFFFFFu, hit[i], c++);
		}
	}

	// ---- (u, v) on the edges of the unit triangle and one ulp outside: the ray comes down -z at (x, y), so u = x and v = y exactly ----
	{
		const orc_tri64 tri = make_tri(0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 5u);
		const float two_ulps = 1.1920929e-07f; // 2^-23: 0.5 + 0.5 + 2^-23 is a float above 1 (one ulp of 0.5 more would round back to 1)
		const float xs[] = { 0.0f, 1.0f, 0.5f, 0.25f, 0.0f, -FLT_TRUE_MIN, up(1.0f), 0.5f + two_ulps, 0.25f, 0.0f, 0.25f, 0.0f };
		const float ys[] = { 0.25f, 0.0f, 0.5f, 0.75f, 0.0f, 0.25f, 0.0f, 0.5f, 0.75f + two_ulps, 1.0f, -FLT_TRUE_MIN, up(1.0f) };
		const int hit[] = { 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 0, 0 };
		for (int i = 0; i < 12; i++) {
			const float o[3] = { xs[i], ys[i], 1.0f }, d[3] = { 0.0f, 0.0f, -1.0f };
			check_tri(o, d, tri, 0.0f, 100.0f, false, 0xFFFFFFFFu, hit[i], c++);
		}
		// ---- t == t_min (t = 1 here) and its neighbours ----
		const float o[3] = { 0.25f, 0.25f, 1.0f }, d[3] = { 0.0f, 0.0f, -1.0f };
		check_tri(o, d, tri, 1.0f, 100.0f, false, 0xFFFFFFFFu, 1, c++);
		check_tri(o, d, tri, up(1.0f), 100.0f, false, 0xFFFFFFFFu, 0, c++);
		check_tri(o, d, tri, down(1.0f), 100.0f, false, 0xFFFFFFFFu, 1, c++);
		// ---- t == best_t: a lower, an equal and a higher id than the triangle's 5, with and without a hit before ----
		check_tri(o, d, tri, 0.0f, 1.0f, true, 9u, 1, c++);          // the hit before has the higher id: this one wins the tie
		check_tri(o, d, tri, 0.0f, 1.0f, true, 5u, 0, c++);
		check_tri(o, d, tri, 0.0f, 1.0f, true, 2u, 0, c++);
		check_tri(o, d, tri, 0.0f, 1.0f, false, 0xFFFFFFFFu, 0, c++); // no hit before: best_t is the ray's t_max, which excludes t
		check_tri(o, d, tri, 0.0f, 1.0f, false, 9u, 0, c++);
		check_tri(o, d, tri, 0.0f, up(1.0f), true, 2u, 1, c++);       // closer than the best: the ids do not count
		check_tri(o, d, tri, 0.0f, down(1.0f), true, 9u, 0, c++);
		check_tri(o, d, tri, 1.0f, 1.0f, true, 9u, 1, c++);           // t_min == t == best_t
	}

	// ---- the tie rule by itself, every combination ----
	for (float t : { 0.0f, 1.0f, up(1.0f), down(1.0f) }) for (float lim : { 1.0f, FLT_MAX }) for (float t_min : { 0.0f, 1.0f, up(1.0f) })
		for (uint32_t slot : { 0u, 0xFFFFFFFFu }) for (uint32_t id : { 0u, 4u, 0xFFFFFFFEu }) for (uint32_t best_id : { 0u, 4u, 0xFFFFFFFFu }) {
			// tri_hit() of mrt_oracle.c:357-358, after its u, v rejections
			const bool want = !(t < t_min) && (t < lim || (t == lim && slot != 0xFFFFFFFFu && id < best_id));
			check(mrt::closer_hit(t, id, t_min, lim, slot, best_id) == want, "closer_hit", c++);
		}

	if (g_fails) { std::printf("%ld of %ld checks FAILED\n", g_fails, g_checks); return 1; }
	std::printf("%ld checks hold\n", g_checks);
	return 0;
}
