// instance_math_test.cpp -- instance_math.h (invert_affine, world_box: compiled for the host here, for the device in tlas_device.hip)
// against the host path's own text as it stood before the two functions were shared, bit for bit: on random transforms and mesh boxes
// and on edge cases (near-singular and singular bases, negative determinants, large translations, mesh boxes of zero extent, non-finite
// values).  A device top level whose rows differ from the host path's by one ulp would show in the cast records.
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../instance_math.h"

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

namespace {

// the host path's invert_affine and world_box as they were written in two_level_prep.cpp
bool ref_invert_affine(const float basis[9], const float origin[3], float inv[12])
{
	const double a = basis[0], b = basis[1], c = basis[2], d = basis[3], e = basis[4], f = basis[5], g = basis[6], h = basis[7], i = basis[8];
	const double c00 = e * i - f * h, c01 = c * h - b * i, c02 = b * f - c * e;
	const double c10 = f * g - d * i, c11 = a * i - c * g, c12 = c * d - a * f;
	const double c20 = d * h - e * g, c21 = b * g - a * h, c22 = a * e - b * d;
	const double det = a * c00 + b * c10 + c * c20;
	if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
	const double m[9] = { c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det };
	for (int r = 0; r < 3; r++) {
		const double t = -(m[3 * r] * (double)origin[0] + m[3 * r + 1] * (double)origin[1] + m[3 * r + 2] * (double)origin[2]);
		inv[4 * r] = (float)m[3 * r]; inv[4 * r + 1] = (float)m[3 * r + 1]; inv[4 * r + 2] = (float)m[3 * r + 2]; inv[4 * r + 3] = (float)t;
		if (!std::isfinite(inv[4 * r]) || !std::isfinite(inv[4 * r + 1]) || !std::isfinite(inv[4 * r + 2]) || !std::isfinite(inv[4 * r + 3])) return false;
	}
	return true;
}

void ref_world_box(const float lo[3], const float hi[3], const float basis[9], const float origin[3], float wlo[3], float whi[3])
{
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
		if ((double)l > mn[r]) l = std::nextafterf(l, -INFINITY);
		if ((double)u < mx[r]) u = std::nextafterf(u, INFINITY);
		wlo[r] = l; whi[r] = u;
	}
}

int n_checks = 0, n_fail = 0, n_singular = 0;

bool same_bits(const float *a, const float *b, int n) { return std::memcmp(a, b, sizeof(float) * (size_t)n) == 0; }

void check(const char *what, const float basis[9], const float origin[3], const float lo[3], const float hi[3])
{
	float inv_a[12], inv_b[12];
	std::memset(inv_a, 0, sizeof(inv_a)); std::memset(inv_b, 0, sizeof(inv_b));
	const bool ok_a = mrt::invert_affine(basis, origin, inv_a), ok_b = ref_invert_affine(basis, origin, inv_b);
	n_checks++;
	if (ok_a != ok_b || (ok_a && !same_bits(inv_a, inv_b, 12))) {
		n_fail++;
		std::printf("FAIL %s: invert_affine differs (shared %d, host %d)\n", what, ok_a, ok_b);
	}
	if (!ok_b) n_singular++;
	float wa[6], wb[6];
	mrt::world_box(lo, hi, basis, origin, wa, wa + 3);
	ref_world_box(lo, hi, basis, origin, wb, wb + 3);
	n_checks++;
	// (NaN boxes compare by bits too: the same NaN from the same operations)
	if (!same_bits(wa, wb, 6)) {
		n_fail++;
		std::printf("FAIL %s: world_box differs: shared [%a %a %a | %a %a %a] host [%a %a %a | %a %a %a]\n", what,
				wa[0], wa[1], wa[2], wa[3], wa[4], wa[5], wb[0], wb[1], wb[2], wb[3], wb[4], wb[5]);
	}
	for (int r = 0; r < 3; r++) {
		// the box contains the exact image of the mesh box's corners: rounded outwards where a conversion rounded
		if (std::isfinite(wb[r]) && std::isfinite(wb[3 + r]) && wb[r] > wb[3 + r]) {
			n_fail++;
			std::printf("FAIL %s: world_box axis %d is empty\n", what, r);
		}
	}
}

void rotation(std::mt19937 &g, float s, float basis[9])
{
	std::uniform_real_distribution<float> u(-1.0f, 1.0f);
	float q[4], n2 = 0.0f;
	do { n2 = 0.0f; for (float &v : q) { v = u(g); n2 += v * v; } } while (n2 < 1e-3f || n2 > 1.0f);
	const float l = std::sqrt(n2);
	for (float &v : q) v /= l;
	const float w = q[0], x = q[1], y = q[2], z = q[3];
	const float m[9] = { 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
		2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
		2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y) };
	for (int k = 0; k < 9; k++) basis[k] = m[k] * s;
}

} // namespace

int main()
{
	std::mt19937 g(20261016u);
	std::uniform_real_distribution<float> u(-1.0f, 1.0f), sc(0.05f, 4.0f), tr(-50.0f, 50.0f);
	float basis[9], origin[3], lo[3], hi[3];
	auto random_box = [&] { for (int c = 0; c < 3; c++) { const float a = u(g) * 3.0f, b = u(g) * 3.0f; lo[c] = a < b ? a : b; hi[c] = a < b ? b : a; } };
	char name[64];
	// random similarity transforms, general (sheared, non-uniform) bases, mirrored ones
	for (int t = 0; t < 20000; t++) {
		random_box();
		for (int c = 0; c < 3; c++) origin[c] = tr(g);
		if (t % 3 == 0) rotation(g, sc(g), basis);
		else for (int k = 0; k < 9; k++) basis[k] = u(g) * sc(g);
		if (t % 5 == 0) for (int k = 0; k < 3; k++) basis[k] = -basis[k]; // negative determinant
		std::snprintf(name, sizeof(name), "random %d", t);
		check(name, basis, origin, lo, hi);
	}
	// near-singular: two rows almost parallel, down to exactly parallel
	for (int t = 0; t < 2000; t++) {
		random_box();
		for (int c = 0; c < 3; c++) origin[c] = tr(g);
		for (int k = 0; k < 9; k++) basis[k] = u(g);
		const float eps = std::ldexp(1.0f, -(t % 40));
		for (int k = 0; k < 3; k++) basis[3 + k] = basis[k] * (1.0f + eps * (k == t % 3 ? 1.0f : 0.0f));
		if (t % 7 == 0) for (int k = 0; k < 3; k++) basis[3 + k] = basis[k];
		std::snprintf(name, sizeof(name), "near-singular %d", t);
		check(name, basis, origin, lo, hi);
	}
	// tiny and huge scales (the inverse overflows or underflows float)
	for (int t = 0; t < 2000; t++) {
		random_box();
		for (int c = 0; c < 3; c++) origin[c] = u(g);
		rotation(g, std::ldexp(1.0f, (t % 250) - 125), basis);
		std::snprintf(name, sizeof(name), "scale 2^%d", (t % 250) - 125);
		check(name, basis, origin, lo, hi);
	}
	// large translations
	for (int t = 0; t < 2000; t++) {
		random_box();
		rotation(g, sc(g), basis);
		for (int c = 0; c < 3; c++) origin[c] = u(g) * std::ldexp(1.0f, 10 + t % 110);
		std::snprintf(name, sizeof(name), "translation %d", t);
		check(name, basis, origin, lo, hi);
	}
	// mesh boxes of zero extent (a flat mesh, a point), identity and axis permutations
	for (int t = 0; t < 2000; t++) {
		random_box();
		const int axis = t % 4;
		if (axis < 3) hi[axis] = lo[axis]; else for (int c = 0; c < 3; c++) hi[c] = lo[c];
		if (t % 2) rotation(g, sc(g), basis);
		else { std::memset(basis, 0, sizeof(basis)); basis[0 + (t / 2) % 3] = 1.0f; basis[3 + ((t / 2) + 1) % 3] = -1.0f; basis[6 + ((t / 2) + 2) % 3] = 1.0f; }
		for (int c = 0; c < 3; c++) origin[c] = tr(g);
		std::snprintf(name, sizeof(name), "zero extent %d", t);
		check(name, basis, origin, lo, hi);
	}
	// non-finite values: a NaN or an infinity in a basis, in an origin
	const float bad[3] = { NAN, INFINITY, -INFINITY };
	for (int t = 0; t < 36; t++) {
		random_box();
		rotation(g, 1.0f, basis);
		for (int c = 0; c < 3; c++) origin[c] = tr(g);
		if (t < 27) basis[t % 9] = bad[t / 9]; else origin[t % 3] = bad[(t - 27) / 3];
		std::snprintf(name, sizeof(name), "non-finite %d", t);
		check(name, basis, origin, lo, hi);
	}
	// an all-zero basis
	std::memset(basis, 0, sizeof(basis));
	check("zero basis", basis, origin, lo, hi);
	if (n_singular < 100) { n_fail++; std::printf("FAIL only %d singular cases exercised\n", n_singular); }
	std::printf("%d singular or non-finite transforms refused alike\n", n_singular);
	if (n_fail) { std::printf("%d of %d checks FAIL\n", n_fail, n_checks); return 1; }
	std::printf("%d checks hold (invert_affine and world_box of instance_math.h against the host path)\n", n_checks);
	return 0;
}
