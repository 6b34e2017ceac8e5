// build_rules_test.cpp -- build_rules.h (compiled for the host here, for the device in device_build.hip, refit.hip and tlas_device.hip)
// against the host path's own text as it stood before the rules were shared, bit for bit: the mrt_make_triangles loop, the two
// widening loops and the quantise lambda of scene_prep.cpp, the fix lambdas of two_level_prep.cpp, and a restatement of the device's
// box rule (the host never had one), on random and edge inputs.  A builder whose rows differ from the other path's by one ulp would
// show in the cast records.
// Prints "FAIL ..." per mismatch and "<n> checks hold" at the end; exit status 1 on any failure.
#include "../build_rules.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace {

using namespace mrt;

// ---- the host path's text, as it was written in scene_prep.cpp and two_level_prep.cpp ----

inline void normalize3(float v[3])
{
	float l2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
	if (l2 == 0.0f) { v[0] = v[1] = v[2] = 0.0f; return; }
	float l = std::sqrt(l2);
	v[0] /= l; v[1] /= l; v[2] /= l;
}
inline void cross3(const float a[3], const float b[3], float r[3])
{
	r[0] = a[1] * b[2] - a[2] * b[1];
	r[1] = a[2] * b[0] - a[0] * b[2];
	r[2] = a[0] * b[1] - a[1] * b[0];
}
void ref_make_triangles(const float *verts9, const uint32_t *ids, const uint32_t *layers, uint32_t n_tris, mrt_tri64 *out)
{
	for (uint32_t i = 0; i < n_tris; i++) {
		const float *a = verts9 + 9 * (size_t)i, *b = a + 3, *c = a + 6;
		mrt_tri64 &t = out[i];
		for (int k = 0; k < 3; k++) { t.v0[k] = a[k]; t.edge1[k] = b[k] - a[k]; t.edge2[k] = c[k] - a[k]; }
		cross3(t.edge1, t.edge2, t.normal);
		normalize3(t.normal);
		t.id = ids ? ids[i] : i;
		t.layers = layers ? layers[i] : 0xFFFFFFFFu;
		t.pad2 = 0.0f; t.pad3 = 0.0f;
	}
}

struct Child { float mn[3], mx[3]; uint32_t ref; };
struct Kids { Child ch[8]; uint32_t n; };

// the widening loops of prepare_scene over the binary tree dev, for the node w2: 4-wide, then 8-wide
uint32_t ref_widen4(const std::vector<DevNode> &dev, uint32_t w2, Child ch[4])
{
	auto area = [](const Child &c) {
		const float e0 = c.mx[0] - c.mn[0], e1 = c.mx[1] - c.mn[1], e2 = c.mx[2] - c.mn[2];
		return e0 * e1 + e1 * e2 + e2 * e0;
	};
	auto children_of = [&](uint32_t w, Child &l, Child &r) {
		const DevNode &g = dev[w];
		for (int c = 0; c < 3; c++) { l.mn[c] = g.lmin[c]; l.mx[c] = g.lmax[c]; r.mn[c] = g.rmin[c]; r.mx[c] = g.rmax[c]; }
		l.ref = g.left_ref; r.ref = g.right_ref;
	};
	uint32_t n = 2;
	children_of(w2, ch[0], ch[1]);
	while (n < 4) {
		int best = -1; float best_a = -1.0f;
		for (uint32_t i = 0; i < n; i++) if (ch[i].ref < kSentinel) { const float a = area(ch[i]); if (a > best_a) { best_a = a; best = (int)i; } }
		if (best < 0) break;
		Child l, r; children_of(ch[best].ref, l, r);
		ch[best] = l; ch[n++] = r;
	}
	return n;
}
void ref_widen8(const std::vector<DevNode> &dev, uint32_t w2, Kids &k)
{
	auto area = [](const Child &c) {
		const float e0 = c.mx[0] - c.mn[0], e1 = c.mx[1] - c.mn[1], e2 = c.mx[2] - c.mn[2];
		return e0 * e1 + e1 * e2 + e2 * e0;
	};
	auto children_of = [&](uint32_t w, Child &l, Child &r) {
		const DevNode &g = dev[w];
		for (int c = 0; c < 3; c++) { l.mn[c] = g.lmin[c]; l.mx[c] = g.lmax[c]; r.mn[c] = g.rmin[c]; r.mx[c] = g.rmax[c]; }
		l.ref = g.left_ref; r.ref = g.right_ref;
	};
	k.n = 2;
	children_of(w2, k.ch[0], k.ch[1]);
	while (k.n < 8) {
		int best = -1; float best_a = -1.0f;
		for (uint32_t i = 0; i < k.n; i++) if (k.ch[i].ref < kSentinel) { const float a = area(k.ch[i]); if (a > best_a) { best_a = a; best = (int)i; } }
		if (best < 0) break;
		Child l, r; children_of(k.ch[best].ref, l, r);
		k.ch[best] = l; k.ch[k.n++] = r;
	}
}

// the quantise lambda of prepare_scene for one node (its leaf_box writes left out: they stay with the callers); returns !bad
bool ref_quantise(const Kids &k, Dev8Node &node)
{
	bool bad = false;
	std::memset(&node, 0, sizeof(node));
	node.n_children = (uint8_t)k.n;
	float scale[3] = { 1.0f, 1.0f, 1.0f };
	for (int a = 0; a < 3; a++) {
		float lo = k.ch[0].mn[a], hi = k.ch[0].mx[a];
		for (uint32_t i = 1; i < k.n; i++) { lo = std::min(lo, k.ch[i].mn[a]); hi = std::max(hi, k.ch[i].mx[a]); }
		node.org[a] = lo;
		// smallest power-of-two step with (hi - lo) / step <= 254 (one step of headroom for the outward rounding)
		int e = 1;
		const double ext = (double)hi - (double)lo;
		if (!(ext >= 0.0) || !std::isfinite(ext)) { bad = true; continue; } // NaN / infinite box
		if (ext > 0.0) { e = (int)std::ceil(std::log2(ext / 254.0)) + 127; if (e < 1) e = 1; if (e > 254) e = 254; }
		for (;;) { // guard against log2 rounding: make sure the extent fits
			uint32_t bits = (uint32_t)e << 23; float s; std::memcpy(&s, &bits, 4);
			if ((double)s * 254.0 >= ext || e >= 254) { scale[a] = s; break; }
			e++;
		}
		node.exp[a] = (uint8_t)e;
	}
	for (uint32_t i = 0; i < 8; i++) {
		if (i >= k.n) { node.ref[i] = kSentinel; continue; }
		node.ref[i] = k.ch[i].ref;
		for (int a = 0; a < 3 && !bad; a++) {
			// outward rounding, verified on the value the kernel will decode: fmaf(q, scale, org)
			int ql = (int)std::floor(((double)k.ch[i].mn[a] - (double)node.org[a]) / (double)scale[a]);
			if (ql < 0) ql = 0;
			if (ql > 255) ql = 255;
			while (ql > 0 && std::fmaf((float)ql, scale[a], node.org[a]) > k.ch[i].mn[a]) ql--;
			int qh = (int)std::ceil(((double)k.ch[i].mx[a] - (double)node.org[a]) / (double)scale[a]);
			if (qh < 0) qh = 0;
			if (qh > 255) qh = 255;
			while (qh < 255 && std::fmaf((float)qh, scale[a], node.org[a]) < k.ch[i].mx[a]) qh++;
			if (std::fmaf((float)ql, scale[a], node.org[a]) > k.ch[i].mn[a] || std::fmaf((float)qh, scale[a], node.org[a]) < k.ch[i].mx[a])
				bad = true; // cannot happen for finite boxes (one step of headroom); never ship a box that does not contain its child
			node.qlo[a][i] = (uint8_t)ql; node.qhi[a][i] = (uint8_t)qh;
		}
	}
	return !bad;
}

// the box rule, restated: the bounds of v0, v0 + e1, v0 + e2, each one float step outwards, a zero to -+FLT_MIN
float ref_step(float f, bool up)
{
	if (f == 0.0f) return up ? FLT_MIN : -FLT_MIN;
	uint32_t u; std::memcpy(&u, &f, 4);
	u = ((f > 0.0f) == up) ? u + 1u : u - 1u; // away from zero: one more in magnitude
	std::memcpy(&f, &u, 4);
	return f;
}
void ref_tri_box(const float v0[3], const float e1[3], const float e2[3], float mn[3], float mx[3])
{
	for (int k = 0; k < 3; k++) {
		const float p1 = v0[k] + e1[k], p2 = v0[k] + e2[k];
		mn[k] = ref_step(std::fmin(v0[k], std::fmin(p1, p2)), false);
		mx[k] = ref_step(std::fmax(v0[k], std::fmax(p1, p2)), true);
	}
}

// ---- the checks ----

int n_checks = 0, n_fail = 0, n_bad = 0;

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
bool same(const void *a, const void *b, size_t n) { return std::memcmp(a, b, n) == 0; }
void expect(bool ok, const char *what, int k)
{
	n_checks++;
	if (!ok) { n_fail++; std::printf("FAIL %s %d\n", what, k); }
}

void check_triangle(const float v9[9], uint32_t id, uint32_t layers, const char *what, int k)
{
	mrt_tri64 want, have;
	std::memset(&want, 0xAB, sizeof(want)); std::memset(&have, 0xCD, sizeof(have));
	ref_make_triangles(v9, &id, &layers, 1, &want);
	have = make_tri64(v9, v9 + 3, v9 + 6, id, layers);
	expect(same(&want, &have, sizeof(want)), what, k);
	// the box rule on the triangle as the device sees it
	float mn[3], mx[3];
	ref_tri_box(want.v0, want.edge1, want.edge2, mn, mx);
	const Box b = tri_box(have.v0, have.edge1, have.edge2);
	expect(same(mn, b.mn, 12) && same(mx, b.mx, 12), "tri_box of", k);
}

void check_steps(float f, int k)
{
	expect(bits(ulp_down(f)) == bits(ref_step(f, false)) && bits(ulp_up(f)) == bits(ref_step(f, true)), "ulp_down / ulp_up", k);
	if (std::isfinite(f) && f != 0.0f && std::fabs(f) < FLT_MAX) // one step of the float line, as nextafterf takes it
		expect(ulp_down(f) == std::nextafterf(f, -INFINITY) && ulp_up(f) == std::nextafterf(f, INFINITY), "ulp step against nextafterf", k);
	expect(ord2f(f2ord(f)) == f || f != f, "ord2f(f2ord)", k);
}

// a random binary tree over n_leaves leaves in dev (node 0 the root), boxes drawn by draw(); chain: every right child a leaf
template <class Draw> void random_tree(std::mt19937 &g, uint32_t n_leaves, bool chain, Draw draw, std::vector<DevNode> &dev)
{
	dev.assign(n_leaves - 1, DevNode{});
	uint32_t next_node = 1, next_leaf = 0;
	struct Item { uint32_t node, leaves; };
	std::vector<Item> stack{ { 0u, n_leaves } };
	while (!stack.empty()) {
		const Item it = stack.back(); stack.pop_back();
		const uint32_t ll = chain ? it.leaves - 1 : 1 + g() % (it.leaves - 1), rl = it.leaves - ll;
		DevNode &d = dev[it.node];
		draw(d.lmin, d.lmax); draw(d.rmin, d.rmax);
		if (ll == 1) { d.left_ref = kLeafBit | next_leaf++; d.left_count = 1; } else { d.left_ref = next_node; stack.push_back({ next_node++, ll }); }
		if (rl == 1) { d.right_ref = kLeafBit | next_leaf++; d.right_count = 1; } else { d.right_ref = next_node; stack.push_back({ next_node++, rl }); }
	}
}

// every node of dev through both widenings and the grid, shared against host
void check_tree(const std::vector<DevNode> &dev, const char *what, int k, uint32_t want_n4 = 0, uint32_t want_n8 = 0)
{
	auto node_of = [&](uint32_t w) -> const DevNode & { return dev[w]; };
	auto same_kids = [](const Child *r, const float (*box)[6], const uint32_t *ref, uint32_t n) {
		for (uint32_t i = 0; i < n; i++)
			if (!same(r[i].mn, box[i], 12) || !same(r[i].mx, box[i] + 3, 12) || r[i].ref != ref[i]) return false;
		return true;
	};
	for (uint32_t w = 0; w < dev.size(); w++) {
		Child r4[4]; struct { float box[4][6]; uint32_t ref[4]; } h4;
		std::memset(r4, 0, sizeof(r4)); std::memset(&h4, 0, sizeof(h4));
		const uint32_t n4 = ref_widen4(dev, w, r4);
		take_children(dev[w], h4.box, h4.ref, 0, 1);
		const uint32_t m4 = open_widest(h4.box, h4.ref, node_of);
		expect(n4 == m4 && same_kids(r4, h4.box, h4.ref, n4) && (!want_n4 || w != 0 || n4 == want_n4), what, k);
		Kids r8; struct { float box[8][6]; uint32_t ref[8]; } h8;
		std::memset(&r8, 0, sizeof(r8)); std::memset(&h8, 0, sizeof(h8));
		ref_widen8(dev, w, r8);
		take_children(dev[w], h8.box, h8.ref, 0, 1);
		const uint32_t m8 = open_widest(h8.box, h8.ref, node_of);
		expect(r8.n == m8 && same_kids(r8.ch, h8.box, h8.ref, m8) && (!want_n8 || w != 0 || m8 == want_n8), what, k);
		Dev8Node want, have;
		const bool ok_want = ref_quantise(r8, want), ok_have = quantise8(h8.box, h8.ref, m8, have);
		if (!ok_want) n_bad++;
		expect(ok_want == ok_have && same(&want, &have, sizeof(want)), "quantise8 of", k);
	}
}

} // namespace

int main()
{
	std::mt19937 g(20261019u);
	std::uniform_real_distribution<float> u(-1.0f, 1.0f);
	float v9[9];
	// ---- triangles and their boxes: random at several magnitudes, then the edge cases
	for (int t = 0; t < 20000; t++) {
		const float s = std::ldexp(1.0f, (t % 60) - 30);
		for (float &x : v9) x = u(g) * s;
		check_triangle(v9, (uint32_t)g(), (uint32_t)g(), "make_tri64 random", t);
	}
	for (int t = 0; t < 200; t++) { // zero area: two equal vertices, three equal vertices, collinear ones (normal 0 where the cross product is 0)
		for (float &x : v9) x = u(g);
		if (t % 3 == 0) std::memcpy(v9 + 3, v9, 12);
		else if (t % 3 == 1) { std::memcpy(v9 + 3, v9, 12); std::memcpy(v9 + 6, v9, 12); }
		else for (int c = 0; c < 3; c++) { v9[c] = (float)(t % 7); v9[3 + c] = (float)(t % 7) + 1.0f; v9[6 + c] = (float)(t % 7) + 3.0f; }
		check_triangle(v9, 7u, 1u, "make_tri64 zero area", t);
		mrt_tri64 z = make_tri64(v9, v9 + 3, v9 + 6, 0, 0);
		expect(z.normal[0] == 0.0f && z.normal[1] == 0.0f && z.normal[2] == 0.0f, "zero-area normal is 0", t);
	}
	const float edge[] = { 0.0f, -0.0f, FLT_MIN, -FLT_MIN, 1.4e-45f, -1.4e-45f, 3e-39f, -3e-39f, FLT_MAX, -FLT_MAX, 1.0f, -1.0f, INFINITY, -INFINITY, NAN };
	const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
	for (int t = 0; t < n_edge; t++) check_steps(edge[t], t);
	for (int t = 0; t < 20000; t++) check_steps(std::ldexp(u(g), (int)(g() % 270) - 140), 100 + t);
	for (int t = 0; t < n_edge * n_edge; t++) { // a coordinate at +-0, a denormal, +-FLT_MAX, a non-finite value
		for (float &x : v9) x = u(g);
		v9[t % 9] = edge[t % n_edge]; v9[(t / 9) % 9] = edge[t / n_edge];
		check_triangle(v9, 1u, 2u, "make_tri64 edge coordinate", t);
	}
	// ---- refs
	const uint32_t refs[] = { 0u, 1u, 12345u, kSentinel - 1u, kSentinel, kLeafBit, kLeafBit | 1u, kLeafBit | 0x7FFFFFFFu, 0xFFFFFFFFu };
	for (uint32_t ref : refs)
		for (uint32_t node_base : { 0u, 7u, 0x40000000u, 0u - 5u })
			for (uint32_t tri_base : { 0u, 9u, 0x7FFFFFF0u, 0u - 3u }) {
				auto fix = [&](uint32_t ref) { return ref < kSentinel ? ref + node_base : (ref >= kLeafBit ? (kLeafBit | ((ref & 0x7FFFFFFFu) + tri_base)) : ref); };
				expect(fix(ref) == rebase_ref(ref, node_base, tri_base), "rebase_ref", (int)(ref >> 28));
			}
	expect(rebase_ref(kSentinel, 5u, 5u) == kSentinel && rebase_ref(kSentinel - 1u, 0u, 9u) == kSentinel - 1u && rebase_ref(kLeafBit, 3u, 4u) == (kLeafBit | 4u), "rebase_ref at the sentinel", 0);
	expect(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512, "align256", 0);
	// ---- widening and grids over random trees
	std::vector<DevNode> dev;
	auto box_at = [&](float scale, float centre) {
		return [&g, &u, scale, centre](float mn[3], float mx[3]) {
			for (int c = 0; c < 3; c++) { const float a = centre + u(g) * scale, b = centre + u(g) * scale; mn[c] = a < b ? a : b; mx[c] = a < b ? b : a; }
		};
	};
	for (int t = 0; t < 400; t++) {
		random_tree(g, 2 + g() % 40, false, box_at(std::ldexp(1.0f, (t % 80) - 40), t % 5 ? 0.0f : 1000.0f), dev);
		check_tree(dev, "open_widest random", t);
	}
	// only leaf children: widening stops at 2
	random_tree(g, 2, false, box_at(1.0f, 0.0f), dev);
	check_tree(dev, "open_widest two leaves", 0, 2, 2);
	// a chain fills all 4 and all 8 slots
	random_tree(g, 12, true, box_at(1.0f, 0.0f), dev);
	check_tree(dev, "open_widest chain", 0, 4, 8);
	// equal areas (the first of equals is opened), boxes of zero extent
	for (int t = 0; t < 50; t++) {
		random_tree(g, 2 + g() % 20, false, [&](float mn[3], float mx[3]) { for (int c = 0; c < 3; c++) { mn[c] = (float)(t % 3); mx[c] = mn[c] + (t % 2 ? 1.0f : 0.0f); } }, dev);
		check_tree(dev, "open_widest equal areas / zero extent", t);
	}
	// extents whose exponent clamps at 1 and at 254, extents of exactly 254 * 2^k, coordinates at +-FLT_MAX, denormal boxes
	for (int t = 0; t < 600; t++) {
		const int kind = t % 6;
		random_tree(g, 2 + g() % 12, false, [&](float mn[3], float mx[3]) {
			for (int c = 0; c < 3; c++) {
				if (kind == 0) { mn[c] = u(g) * 1e-40f; mx[c] = mn[c] + std::fabs(u(g)) * 1e-40f; }          // the exponent clamps at 1
				else if (kind == 1) { mn[c] = -FLT_MAX * std::fabs(u(g)); mx[c] = FLT_MAX * std::fabs(u(g)); }  // ... at 254 (the extent overflows float)
				else if (kind == 2) { mn[c] = 0.0f; mx[c] = (g() % 2) ? std::ldexp(254.0f, (t % 200) - 100) : std::ldexp(1.0f, (t % 200) - 100); } // exactly 254 * 2^k
				else if (kind == 3) { mn[c] = (g() % 2) ? -FLT_MAX : -1.0f; mx[c] = (g() % 2) ? FLT_MAX : 1.0f; }
				else if (kind == 4) { mn[c] = std::ldexp(3.0f, (t % 200) - 100); mx[c] = mn[c] + std::ldexp(254.0f, (t % 200) - 100 - (int)(g() % 3)); }
				else { mn[c] = (g() % 2) ? 0.0f : -0.0f; mx[c] = (g() % 2) ? 0.0f : 1.4e-45f; }
			}
		}, dev);
		check_tree(dev, "quantise8 edge extents", t);
	}
	// NaN and infinite boxes: the bad flag on both sides (a whole node without a finite extent; one child open to infinity)
	const int bad_before = n_bad;
	for (int t = 0; t < 60; t++) {
		random_tree(g, 2, false, [&](float mn[3], float mx[3]) {
			for (int c = 0; c < 3; c++) { mn[c] = t % 3 == 0 ? NAN : (t % 3 == 1 ? -INFINITY : u(g)); mx[c] = t % 3 == 0 ? NAN : INFINITY; }
		}, dev);
		check_tree(dev, "quantise8 non-finite", t);
	}
	expect(n_bad - bad_before == 60, "every non-finite box is refused", n_bad - bad_before);
	for (int t = 0; t < 200; t++) { // a stray non-finite value among finite boxes: a face open to infinity in any child, a NaN in the first
		bool first = true;
		random_tree(g, 2 + g() % 12, false, [&](float mn[3], float mx[3]) {
			for (int c = 0; c < 3; c++) { const float a = u(g), b = u(g); mn[c] = a < b ? a : b; mx[c] = a < b ? b : a; }
			if (first && t % 3 == 0) mn[g() % 3] = NAN;
			else if (g() % 4 == 0) { if (g() % 2) mn[g() % 3] = -INFINITY; else mx[g() % 3] = INFINITY; }
			first = false;
		}, dev);
		check_tree(dev, "quantise8 stray non-finite", t);
	}
	if (n_fail) { std::printf("%d of %d checks FAIL\n", n_fail, n_checks); return 1; }
	std::printf("%d checks hold (build_rules.h against the host path; %d boxes refused alike)\n", n_checks, n_bad);
	return 0;
}
