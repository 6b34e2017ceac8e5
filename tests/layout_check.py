"""Structural validator of the acceleration layouts a context keeps resident (Context.debug_snapshot, capi.prepare_scene_host,
capi.two_level_prepare_host).  Pure numpy: nothing here calls the library or the oracle; float32 formulas are restated with
float32 operations in the order the code documents, so "bitwise equal" means that.  Every function visits every node, child,
slot and instance of a snapshot and returns a list of Finding(rule, array, element, message); an empty list is a clean layout.

Rules (numbers as in DESIGN.md, "Structural gates"):
  1 topology       every node reached once from the root(s); refs valid, no sentinel in a live child; leaves partition the slots
                   into runs ending at the one flagged triangle; left_count / right_count = run length (leaf) or 0 (inner child)
  2 nesting        a child box stored in a node == min / max of the two boxes stored in the node it points to, bit for bit
  3 leaf boxes     == the restated formula (device builds, refits), or == the caller's boxes (host upload)
  4 containment    how far, in ulps of the box coordinate, a float64 vertex v0, v0 + e1, v0 + e2 lies outside its leaf box (a figure:
                   containment_slack; the tests hold device trees to the host tree's worst value)
  5 triangles      slot_src a permutation; slot k holds input triangle slot_src[k] byte for byte
  6 parents        parent[root] == 0xFFFFFFFF, every other entry names the node that points to it, bit 31 for right children
  7 4-wide         every child is a subtree or leaf of the 2-wide tree with its exact box; children partition their node's leaves;
                   unused slots are sentinels at +inf; stack4 covers a depth-first walk
  8 8-wide         decoded boxes contain the exact ones and are at most one grid step + one ulp outside (see check_wide);
                   leaf_box at every leaf's first slot == the exact leaf box; stack8 covers the walk
  9 rows           d_rows / d_rows4 == the arrays rebuilt from the snapshot's own nodes and triangles, byte for byte
 10 scalars        depth covers the tree; bounds == the root's box; scene_abs_max == the largest |bound|
 11 instances      TLAS leaves partition the instance rows into runs ending at flag bit 0; index a permutation; root, id_base,
                   layers, basis as the input says
 12 transforms     inv == invert_affine restated (float64 cofactors, one rounding); TLAS leaf box == union of the run's world boxes
                   (instance_math.h world_box restated)

The two zeros compare equal wherever a box is a min / max of others (fminf / fmaxf do not order -0 and +0); everything else is
compared by bit pattern.
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

SENT = np.uint32(0x7FFFFFFF)
LEAF = np.uint32(0x80000000)
ROOT_PARENT = np.uint32(0xFFFFFFFF)
FLT_MIN = np.float32(1.17549435e-38)

Finding = namedtuple("Finding", "rule array element message")


class _Out(list):
    """findings; at most `cap` per (rule, array) are kept in full, the rest only counted in the last one's message"""
    cap = 8

    def __init__(self):
        super().__init__()
        self.counts = {}

    def add(self, rule, array, elements, message):
        elements = np.atleast_1d(np.asarray(elements)).ravel()
        if elements.size == 0:
            return
        key = (rule, array, message)
        seen = self.counts.get(key, 0)
        self.counts[key] = seen + elements.size
        for e in elements[:max(0, self.cap - seen)]:
            self.append(Finding(rule, array, int(e), message if elements.size <= self.cap else f"{message} ({elements.size} elements)"))

    def flag(self, rule, array, mask, message, index=None):
        mask = np.asarray(mask)
        if mask.any():
            where = np.flatnonzero(mask.reshape(mask.shape[0], -1).any(axis=1)) if mask.ndim > 1 else np.flatnonzero(mask)
            self.add(rule, array, where if index is None else np.asarray(index)[where], message)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _differ(a, b, zeros_equal=True):
    """elementwise: not the same float32 (bit pattern; the two zeros equal if zeros_equal)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    d = _bits(a) != _bits(b)
    if zeros_equal:
        d &= ~((a == 0) & (b == 0))
    return d


def ulp_down(f):
    """csrc/build_rules.h ulp_down: one float32 step towards -inf (0 -> -FLT_MIN)"""
    f = np.ascontiguousarray(f, dtype=np.float32)
    u = f.view(np.uint32)
    step = np.where(f > 0, np.uint32(0xFFFFFFFF), np.uint32(1)).astype(np.uint32)  # + (-1) or + 1, modulo 2^32
    return np.where(f == 0, -FLT_MIN, (u + step).view(np.float32)).astype(np.float32)


def ulp_up(f):
    f = np.ascontiguousarray(f, dtype=np.float32)
    u = f.view(np.uint32)
    step = np.where(f > 0, np.uint32(1), np.uint32(0xFFFFFFFF)).astype(np.uint32)
    return np.where(f == 0, FLT_MIN, (u + step).view(np.float32)).astype(np.float32)


def slot_boxes_device(hot):
    """csrc/build_rules.h tri_box (device builds and refits): bounds of v0, v0 + e1, v0 + e2 in float32, one ulp outwards."""
    v0, e1, e2 = hot["v0"], hot["e1"], hot["e2"]
    p1, p2 = v0 + e1, v0 + e2  # float32 sums
    mn = ulp_down(np.minimum(v0, np.minimum(p1, p2)))
    mx = ulp_up(np.maximum(v0, np.maximum(p1, p2)))
    return mn, mx


# ---- the 2-wide tree ---------------------------------------------------------------------------------------------------------

def walk2(nodes, roots, lo, hi, n_slots, out, array="nodes", cover=False, wrapped_ok=True):
    """Breadth-first from `roots` through the rows [lo, hi) of `nodes` (rule 1: reachability, refs, counts).  Edge e = child
    e & 1 (0 left, 1 right) of reached node t.order[e >> 1]."""
    n = nodes.shape[0]
    t = SimpleNamespace()  # what the walk found: the reached nodes, their levels, one row per child ("edge")
    roots = np.unique(np.asarray(roots, dtype=np.int64))
    bad = (roots < lo) | (roots >= hi)
    out.flag(1, array, bad, "root outside the node range", roots)
    frontier = roots[~bad]
    seen = np.zeros(n, dtype=np.int64)
    level = np.zeros(n, dtype=np.int32)
    seen[frontier] = 1
    levels = []
    lvl = 1
    while frontier.size:
        level[frontier] = lvl
        levels.append(frontier)
        refs = np.concatenate([nodes["left_idx"][frontier], nodes["right_idx"][frontier]]).astype(np.int64)
        src = np.concatenate([frontier, frontier])
        out.flag(1, array, refs == int(SENT), "sentinel in a live child", src)
        inner = refs < int(SENT)
        oob = inner & ((refs < lo) | (refs >= hi))
        out.flag(1, array, oob, "child ref outside the node range", src)
        cand = refs[inner & ~oob]
        before = seen.copy()
        np.add.at(seen, cand, 1)
        first = np.unique(cand)
        frontier = first[before[first] == 0]
        lvl += 1
        if lvl > 4096:
            out.add(1, array, [0], "walk deeper than 4096 levels")
            break
    out.flag(1, array, seen > 1, "node reached more than once")
    if cover:
        idx = np.arange(lo, hi)
        out.flag(1, array, seen[lo:hi] == 0, "node never reached from the root", idx)
    t.levels = levels
    t.level = level
    t.order = np.concatenate(levels) if levels else np.zeros(0, dtype=np.int64)
    t.depth_levels = len(levels)
    o = t.order
    m = o.size
    t.e_node = np.repeat(o, 2)
    t.e_side = np.tile(np.array([0, 1]), m)
    ref = np.empty(2 * m, dtype=np.uint32)
    cnt = np.empty(2 * m, dtype=np.uint32)
    mn = np.empty((2 * m, 3), dtype=np.float32)
    mx = np.empty((2 * m, 3), dtype=np.float32)
    ref[0::2], ref[1::2] = nodes["left_idx"][o], nodes["right_idx"][o]
    cnt[0::2], cnt[1::2] = nodes["left_count"][o], nodes["right_count"][o]
    mn[0::2], mn[1::2] = nodes["left_min"][o], nodes["right_min"][o]
    mx[0::2], mx[1::2] = nodes["left_max"][o], nodes["right_max"][o]
    t.e_ref, t.e_cnt, t.e_mn, t.e_mx = ref, cnt, mn, mx
    t.e_leaf = ref >= LEAF
    t.e_inner = ref < SENT
    t.e_first = (ref & SENT).astype(np.int64)
    # counts: the run length of a leaf child, 0 for an inner child
    out.flag(1, array, t.e_inner & (cnt != 0), "count of an inner child is not 0", t.e_node)
    out.flag(1, array, t.e_leaf & (cnt == 0), "count of a leaf child is 0", t.e_node)
    out.flag(1, array, t.e_leaf & (t.e_first + cnt > n_slots), "leaf run outside the slot range", t.e_node)
    # leaves partition [0, n_slots): sorted by first slot, each run starts where the one before ends.  A tree that is one wrapped
    # root leaf of a single slot names that slot on both sides (scene_prep.cpp, tlas_commit_kernel): counted once.
    leaf = np.flatnonzero(t.e_leaf & (cnt != 0) & (t.e_first + cnt <= n_slots))
    if wrapped_ok and m == 1 and leaf.size == 2 and ref[0] == ref[1] and cnt[0] == cnt[1] == 1 and n_slots == 1:
        leaf = leaf[:1]
    leaf = leaf[np.argsort(t.e_first[leaf], kind="stable")]
    t.leaf_edges = leaf
    t.leaf_first = t.e_first[leaf]
    t.leaf_count = cnt[leaf].astype(np.int64)
    ends = t.leaf_first + t.leaf_count
    if leaf.size == 0:
        out.add(1, array, [0], "the tree has no leaves")
    else:
        out.flag(1, array, np.concatenate([[t.leaf_first[0] != 0], t.leaf_first[1:] != ends[:-1]]),
                 "leaf runs do not tile the slots (gap or overlap before this leaf)", t.e_node[leaf])
        if ends[-1] != n_slots:
            out.add(1, array, [t.e_node[leaf[-1]]], "leaf runs end before the last slot")
    return t


def check_leaf_flags(t, flags, out, array="tri_hot"):
    """rule 1: the last-in-leaf flag is set at the last slot of every leaf run and nowhere else (no other flag bit exists)"""
    want = np.zeros(flags.shape[0], dtype=np.uint32)
    ends = t.leaf_first + t.leaf_count - 1
    want[ends[(ends >= 0) & (ends < want.shape[0])]] = 1
    out.flag(1, array, (flags == 0) & (want == 1), "leaf's last triangle lacks the last-in-leaf flag")
    out.flag(1, array, (flags != 0) & (want == 0), "flag set inside a leaf run")
    out.flag(1, array, flags > 1, "unknown flag bits")


def check_nesting(nodes, t, out, array="nodes"):
    """rule 2"""
    e = np.flatnonzero(t.e_inner & (t.e_ref < nodes.shape[0]))
    c = t.e_ref[e].astype(np.int64)
    mn = np.minimum(nodes["left_min"][c], nodes["right_min"][c])
    mx = np.maximum(nodes["left_max"][c], nodes["right_max"][c])
    bad_in = (t.e_mn[e] > mn) | (t.e_mx[e] < mx)
    out.flag(2, array, bad_in, "child box smaller than the union of the child's own two boxes", t.e_node[e])
    out.flag(2, array, (_differ(t.e_mn[e], mn) | _differ(t.e_mx[e], mx)).any(axis=1) & ~bad_in.any(axis=1),
             "child box larger than the union of the child's own two boxes", t.e_node[e])


def _run_reduce(values, firsts, counts, op):
    """op-reduction of values[first : first + count] per run; runs sorted, disjoint"""
    if firsts.size == 0:
        return np.zeros((0,) + values.shape[1:], dtype=values.dtype)
    idx = np.empty(2 * firsts.size, dtype=np.int64)
    idx[0::2], idx[1::2] = firsts, firsts + counts
    pad = np.concatenate([values, values[-1:]])  # reduceat needs every index < len
    return op.reduceat(pad, idx, axis=0)[0::2]


def check_leaf_boxes(t, slot_mn, slot_mx, out, what, array="nodes"):
    """rule 3: a leaf child's box == the union of its run's slot boxes"""
    if t.leaf_edges.size == 0:
        return
    ok = (t.leaf_first >= 0) & (t.leaf_first + t.leaf_count <= slot_mn.shape[0])
    le, f, c = t.leaf_edges[ok], t.leaf_first[ok], t.leaf_count[ok]
    mn = _run_reduce(slot_mn, f, c, np.minimum)
    mx = _run_reduce(slot_mx, f, c, np.maximum)
    if t.order.size == 1 and le.size == 2 and not (_differ(t.e_mn[0], t.e_mn[1]).any() or _differ(t.e_mx[0], t.e_mx[1]).any()):
        # a wrapped root leaf (scene_prep.cpp, sah_wrap_kernel): both sides carry the box of the whole run until a refit boxes the halves
        mn[:], mx[:] = mn.min(axis=0), mx.max(axis=0)
    small = (t.e_mn[le] > mn) | (t.e_mx[le] < mx)
    out.flag(3, array, small, f"leaf box smaller than {what}", t.e_node[le])
    out.flag(3, array, (_differ(t.e_mn[le], mn) | _differ(t.e_mx[le], mx)).any(axis=1) & ~small.any(axis=1),
             f"leaf box differs from {what}", t.e_node[le])


def host_leaf_boxes(nodes32, n_slots):
    """per slot, the box of the caller's leaf that holds it (mrt_bvh_node32 leaves; prim_idx is already resolved by the slot order).
    A root leaf owns every slot (node 1 is the unused hole); the device wraps it as two runs that both carry its box."""
    leaf = np.flatnonzero(nodes32["tri_count"] > 0)
    if nodes32["tri_count"][0] > 0:
        leaf = leaf[:1]
    f, c = nodes32["left_first"][leaf].astype(np.int64), nodes32["tri_count"][leaf].astype(np.int64)
    order = np.argsort(f)
    owner = np.repeat(leaf[order], c[order])[:n_slots]
    mn = np.full((n_slots, 3), np.inf, dtype=np.float32)
    mx = np.full((n_slots, 3), -np.inf, dtype=np.float32)
    mn[:owner.size], mx[:owner.size] = nodes32["aabb_min"][owner], nodes32["aabb_max"][owner]
    return mn, mx


def vertex_boxes(verts9, slot_src):
    """per slot, the exact bounds of the input triangle's three vertices: the leaf boxes of the host builder"""
    v = np.ascontiguousarray(verts9, dtype=np.float32).reshape(-1, 3, 3)[slot_src]
    return v.min(axis=1), v.max(axis=1)


def containment_slack(snap, t=None):
    """rule 4: the largest distance by which a vertex (v0, v0 + e1, v0 + e2 in float64) lies outside the box of its leaf, in units in
    the last place of that box coordinate; 0.0 when every vertex is inside."""
    out = _Out()
    if t is None:
        t = _blas_tree(snap, out)
    hot = snap["tri_hot"]
    v0 = hot["v0"].astype(np.float64)
    verts = np.stack([v0, v0 + hot["e1"].astype(np.float64), v0 + hot["e2"].astype(np.float64)], axis=1)
    owner = np.repeat(t.leaf_edges, t.leaf_count)[:hot.shape[0]]
    mn, mx = t.e_mn[owner], t.e_mx[owner]
    below = (mn.astype(np.float64)[:, None, :] - verts) / np.spacing(np.abs(mn))[:, None, :]
    above = (verts - mx.astype(np.float64)[:, None, :]) / np.spacing(np.abs(mx))[:, None, :]
    return float(max(0.0, below.max(), above.max()))


def check_triangles(snap, input_tris, out, slot_src=None):
    """rule 5"""
    hot, cold = snap["tri_hot"], snap["tri_cold"]
    n = hot.shape[0]
    src = snap.get("slot_src") if slot_src is None else slot_src
    if src is None:
        out.add(5, "slot_src", [0], "the scene has no slot map")
        return
    src = src.astype(np.int64)
    counts = np.bincount(src[src < n], minlength=n)
    out.flag(5, "slot_src", src >= n, "entry outside the triangle range")
    out.flag(5, "slot_src", (src < n) & (counts[np.minimum(src, n - 1)] > 1), "input triangle named by more than one slot")
    want = input_tris[np.minimum(src, n - 1)]
    for name, have, exp in (("v0", hot["v0"], want["v0"]), ("e1", hot["e1"], want["edge1"]), ("e2", hot["e2"], want["edge2"])):
        out.flag(5, "tri_hot", _differ(have, exp, zeros_equal=False), f"{name} is not the input triangle's")
    out.flag(5, "tri_hot", hot["id"] != want["id"], "id is not the input triangle's")
    out.flag(5, "tri_hot", hot["layers"] != want["layers"], "layers are not the input triangle's")
    out.flag(5, "tri_cold", _differ(cold["normal"], want["normal"], zeros_equal=False), "normal is not the input triangle's")
    out.flag(5, "tri_cold", cold["pad"] != 0, "padding word is not zero")


def expected_parents(t, lo, n):
    """rule 6: the table refit_parents_kernel documents, for the rows [lo, lo + n)"""
    p = np.full(n, ROOT_PARENT, dtype=np.uint32)
    e = np.flatnonzero(t.e_inner)
    c = t.e_ref[e].astype(np.int64) - lo
    ok = (c >= 0) & (c < n)
    p[c[ok]] = (t.e_node[e][ok] - lo).astype(np.uint32) | (t.e_side[e][ok].astype(np.uint32) << np.uint32(31))
    return p


def check_parents(snap, t, lo, out):
    parent = snap["parent"]
    want = expected_parents(t, lo, parent.shape[0])
    reached = t.order[(t.order >= lo) & (t.order < lo + parent.shape[0])] - lo
    have, exp = parent[reached], want[reached]
    side = ((have ^ exp) == LEAF) & (exp != ROOT_PARENT) & (have != ROOT_PARENT)
    out.flag(6, "parent", side, "wrong side bit", reached + lo)
    out.flag(6, "parent", (have != exp) & ~side, "entry does not name the node that points to this one", reached + lo)


# ---- the wide layouts ----------------------------------------------------------------------------------------------------------

def _slot_hash(n_slots):
    h = np.random.default_rng(0x5EED).integers(0, 2 ** 63, size=n_slots, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    return np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(h, dtype=np.uint64)])  # csum[k] = sum of the hashes of slots < k


def _tree_signatures(t, n_slots):
    """per edge and per node of the 2-wide tree: the sum (mod 2^64) of its slots' random 64-bit hashes -- equal sums are equal slot
    sets for every purpose here"""
    csum = _slot_hash(n_slots)
    t.csum = csum
    e_sig = np.zeros(t.e_ref.shape[0], dtype=np.uint64)
    f = np.clip(t.e_first, 0, n_slots)
    l = np.clip(t.e_first + t.e_cnt.astype(np.int64), 0, n_slots)
    e_sig[t.e_leaf] = (csum[l] - csum[f])[t.e_leaf]
    pos = np.full(int(t.order.max()) + 1 if t.order.size else 1, -1, dtype=np.int64)
    pos[t.order] = np.arange(t.order.size)
    n_sig = np.zeros(t.order.size, dtype=np.uint64)
    start = np.cumsum([0] + [lv.size for lv in t.levels])
    for k in range(len(t.levels) - 1, -1, -1):
        a, b = start[k], start[k + 1]
        es = np.arange(2 * a, 2 * b)
        inner = es[t.e_inner[es] & (t.e_ref[es] < pos.shape[0])]
        child = pos[t.e_ref[inner].astype(np.int64)]
        e_sig[inner[child >= 0]] = n_sig[child[child >= 0]]
        n_sig[a:b] = e_sig[2 * a:2 * b:2] + e_sig[2 * a + 1:2 * b:2]
    t.e_sig, t.n_sig, t.pos = e_sig, n_sig, pos
    return t


def decode8(nodes8):
    """Dev8Node child boxes as the walk decodes them: fma(q, 2^(exp - 127), org) in float32.  q has 8 bits and the scale is a power of
    two, so q * scale is exact and the float32 sum below rounds once, as the fma does."""
    scale = (nodes8["exp"].astype(np.uint32) << np.uint32(23)).view(np.float32)            # (n, 3)
    lo = nodes8["qlo"].astype(np.float32) * scale[:, :, None] + nodes8["org"][:, :, None]   # (n, 3, 8)
    hi = nodes8["qhi"].astype(np.float32) * scale[:, :, None] + nodes8["org"][:, :, None]
    return lo.astype(np.float32).transpose(0, 2, 1), hi.astype(np.float32).transpose(0, 2, 1), scale  # (n, 8, 3)


def check_wide(width, wnodes, wroots, t, t_roots, node_base, n_slots, stack_have, stack_extra, out, leaf_box=None):
    """rules 7 (width 4) and 8 (width 8) against the walked 2-wide tree t (with signatures).  wroots[k] is the wide root that goes with
    the 2-wide root t_roots[k]; node_base: a layout at binary-node indices holds binary node b at wide index b - node_base.

    The 8-wide looseness bound, from quantise8 (csrc/build_rules.h, the one text of the host and the device collapse): the grid step s is
    the smallest power of two with 254 s >= the node's extent.  qlo starts as floor((lo - org) / s) computed in double (a start
    value only: the difference of two floats is exact in double while their exponents are within 29 bits of each other, and nothing
    below relies on it), and the loop lowers qlo while the DECODED value fma(qlo, s, org) is still above lo; the kernel then
    re-checks the decoded value and drops the layout if it is not <= lo.  So the stored q has decoded(q) <= lo, and either the loop
    stopped there, i.e. decoded(q + 1) > lo, or q is the start value floor(t), t = (lo - org) / s up to double rounding, for which
    org + (q + 1) s > lo up to that rounding (2^-53 relative on a quotient below 255: far inside the ulp allowed next).  Two
    neighbouring decoded values differ by at most s plus one float32 rounding each.  Hence 0 <= lo - decoded_lo < s + ulp, and the
    same for hi with ceil and the upward loop (qhi <= 254 before the loop, 255 is the headroom).  In grid steps: strictly less than one step plus one float32 ulp of the coordinate (below two steps whenever the step
    is not finer than the floats themselves).  The walk's correctness needs only the containment; the bound keeps the boxes tight."""
    rule, array = (7, "nodes4") if width == 4 else (8, "nodes8")
    n = wnodes.shape[0]
    ref = wnodes["ref"].astype(np.uint32)
    nch = wnodes["n_children"].astype(np.int64)
    wroots = np.asarray(wroots, dtype=np.int64)
    okr = (wroots >= 0) & (wroots < n)
    out.flag(rule, array, ~okr, "root outside the layout", np.arange(wroots.size))
    # breadth-first over the wide nodes; pend[w] = entries pending on the stack when w is entered
    seen = np.zeros(n, dtype=np.int64)
    pend = np.zeros(n, dtype=np.int64)
    frontier = np.unique(wroots[okr])
    seen[frontier] = 1
    levels = []
    while frontier.size and len(levels) < 4096:
        levels.append(frontier)
        r = ref[frontier]                                            # (m, W)
        live = np.arange(width)[None, :] < nch[frontier][:, None]
        out.flag(rule, array, (nch[frontier] < 2) | (nch[frontier] > width), "n_children outside 2 .. width", frontier)
        out.flag(rule, array, (r == SENT) & live, "sentinel in a used child slot", frontier)
        out.flag(rule, array, (r != SENT) & ~live, "ref in an unused child slot", frontier)
        inner = live & (r < SENT)
        oob = inner & (r >= n)
        out.flag(rule, array, oob, "child ref outside the layout", frontier)
        rows, cols = np.nonzero(inner & ~oob)
        cand = r[rows, cols].astype(np.int64)
        before = seen.copy()
        np.add.at(seen, cand, 1)
        pend[cand] = pend[frontier[rows]] + nch[frontier[rows]] - 1
        first = np.unique(cand)
        frontier = first[before[first] == 0]
    out.flag(rule, array, seen > 1, "node reached more than once")
    order = np.concatenate(levels) if levels else np.zeros(0, dtype=np.int64)
    if order.size == 0:
        return
    need = int((pend[order] + np.clip(nch[order], 0, width) - 1).max()) + 1 + stack_extra
    if stack_have < need:
        out.add(rule, array, [0], f"stack bound {stack_have} below the layout's need {need}")
    # boxes of the child slots
    if width == 4:
        cmn, cmx = wnodes["box"][:, :, 0:3], wnodes["box"][:, :, 3:6]
        unused = np.arange(4)[None, :] >= nch[order][:, None]
        out.flag(rule, array, unused[:, :, None] & ~np.isposinf(wnodes["box"][order]), "unused slot's box is not at +inf", order)
    else:
        cmn, cmx, scale = decode8(wnodes)
    # signatures bottom-up over the wide tree: a leaf child is its 2-wide leaf's run, an inner child the sum of its node
    run_of_first = np.zeros(n_slots + 1, dtype=np.int64)
    run_of_first[t.leaf_first] = t.leaf_count
    wsig = np.zeros(n, dtype=np.uint64)
    csig = np.zeros((n, width), dtype=np.uint64)
    for lv in reversed(levels):
        r = ref[lv]
        live = np.arange(width)[None, :] < nch[lv][:, None]
        isleaf = live & (r >= LEAF)
        first = np.where(isleaf, (r & SENT).astype(np.int64), 0)
        first_ok = isleaf & (first < n_slots)
        first = np.where(first_ok, first, 0)
        run = np.where(first_ok, run_of_first[first], 0)
        out.flag(rule, array, isleaf & (run == 0), "leaf ref is not the first slot of a leaf of the 2-wide tree", lv)
        s = np.where(isleaf, t.csum[first + run] - t.csum[first], np.uint64(0))
        inner = live & (r < SENT) & (r < n)
        s = np.where(inner, wsig[np.where(inner, r, 0).astype(np.int64)], s)
        csig[lv] = s
        wsig[lv] = s.sum(axis=1, dtype=np.uint64)
    # every wide root holds its 2-wide root's slots; every child is one edge of the 2-wide tree
    troot_pos = t.pos[np.asarray(t_roots, dtype=np.int64)[okr]]
    out.flag(rule, array, wsig[wroots[okr]] != t.n_sig[troot_pos], "root does not cover the slots of the 2-wide root", wroots[okr])
    sort = np.argsort(t.e_sig, kind="stable")
    keys = t.e_sig[sort]
    live = np.arange(width)[None, :] < nch[order][:, None]
    rows, cols = np.nonzero(live)
    w = order[rows]
    sig = csig[w, cols]
    at = np.clip(np.searchsorted(keys, sig), 0, keys.size - 1)
    found = keys[at] == sig
    out.flag(rule, array, ~found, "child's triangles are not a subtree or leaf of the 2-wide tree", w)
    e = sort[at]
    r = ref[w, cols]
    out.flag(rule, array, found & (r >= LEAF) & (t.e_ref[e] != r), "leaf child's ref differs from the 2-wide leaf's", w)
    out.flag(rule, array, found & (r < SENT) & ~t.e_inner[e], "inner child stands for a leaf of the 2-wide tree", w)
    if node_base is not None:
        out.flag(rule, array, found & (r < SENT) & t.e_inner[e] & (r.astype(np.int64) != t.e_ref[e].astype(np.int64) - node_base),
                 "inner child is not at its binary node's index", w)
    # a node's children partition the slots of the 2-wide node it stands for: the sum of the children's slot sets is the node's by
    # construction of wsig; that node is the edge's child for every inner child (checked above through the signature)
    have_mn, have_mx = cmn[w, cols], cmx[w, cols]
    exact_mn, exact_mx = t.e_mn[e], t.e_mx[e]
    if width == 4:
        small = found[:, None] & ((have_mn > exact_mn) | (have_mx < exact_mx))
        out.flag(rule, array, small, "child box smaller than the 2-wide box of the same subtree", w)
        out.flag(rule, array, found & (_differ(have_mn, exact_mn, False) | _differ(have_mx, exact_mx, False)).any(axis=1) & ~small.any(axis=1),
                 "child box differs from the 2-wide box of the same subtree", w)
    else:
        out.flag(rule, array, found[:, None] & ((have_mn > exact_mn) | (have_mx < exact_mx)), "decoded child box does not contain the exact box", w)
        step = scale[w].astype(np.float64)
        gap_lo = exact_mn.astype(np.float64) - have_mn.astype(np.float64)
        gap_hi = have_mx.astype(np.float64) - exact_mx.astype(np.float64)
        tol_lo = step + np.spacing(np.maximum(np.abs(exact_mn), np.abs(have_mn))).astype(np.float64)
        tol_hi = step + np.spacing(np.maximum(np.abs(exact_mx), np.abs(have_mx))).astype(np.float64)
        out.flag(rule, array, found[:, None] & ((gap_lo >= tol_lo) | (gap_hi >= tol_hi)), "decoded child box more than a grid step + an ulp outside the exact box", w)
        if leaf_box is None:
            out.add(8, "leaf_box", [0], "the 8-wide layout has no leaf_box table")
        else:
            le = t.leaf_edges
            f = t.leaf_first
            ok = f < leaf_box.shape[0]
            lb = leaf_box[f[ok]]
            bad = _differ(lb[:, 0:3], t.e_mn[le[ok]], False) | _differ(lb[:, 4:7], t.e_mx[le[ok]], False)
            out.flag(8, "leaf_box", bad, "row at the leaf's first slot is not the exact leaf box", f[ok])


# ---- row arrays ----------------------------------------------------------------------------------------------------------------

def tri_rows(hot, cold):
    n = hot.shape[0]
    rows = np.empty((n, 16), dtype=np.uint32)
    rows[:, 0:12] = np.ascontiguousarray(hot).view(np.uint32).reshape(n, 12)
    rows[:, 12:16] = np.ascontiguousarray(cold).view(np.uint32).reshape(n, 4)
    return rows


def expected_rows(nodes, hot, cold):
    """rule 9: build_rows_kernel restated"""
    n = nodes.shape[0]
    rows = np.ascontiguousarray(nodes).view(np.uint32).reshape(n, 16).copy()
    for col in (3, 7):
        r = rows[:, col]
        rows[:, col] = np.where(r >= LEAF, LEAF | (np.uint32(n) + (r & SENT)), r)
    return np.concatenate([rows, tri_rows(hot, cold)])


def expected_rows4(nodes4, hot, cold):
    """build_rows4_kernel restated: 128-byte node rows {min, max per axis and child | refs | n_children}, then the triangle rows"""
    n = nodes4.shape[0]
    rows = np.zeros((n, 32), dtype=np.uint32)
    box = nodes4["box"].view(np.uint32).reshape(n, 4, 6)
    for k in range(4):
        for c in range(3):
            rows[:, 6 * k + 2 * c] = box[:, k, c]
            rows[:, 6 * k + 2 * c + 1] = box[:, k, 3 + c]
    r = nodes4["ref"]
    rows[:, 24:28] = np.where(r == SENT, r, np.where(r >= LEAF, LEAF | (np.uint32(2 * n) + (r & SENT)), np.uint32(2) * r))
    rows[:, 28] = nodes4["n_children"]
    return np.concatenate([rows.reshape(2 * n, 16), tri_rows(hot, cold)])


def check_rows(snap, out):
    if snap.get("rows") is not None:
        want = expected_rows(snap["nodes"], snap["tri_hot"], snap["tri_cold"])
        if want.shape != snap["rows"].shape:
            out.add(9, "rows", [0], f"{snap['rows'].shape[0]} rows, expected {want.shape[0]}")
        else:
            out.flag(9, "rows", want != snap["rows"], "row is not the node / triangle it was built from")
    if snap.get("rows4") is not None and snap.get("nodes4") is not None:
        want = expected_rows4(snap["nodes4"], snap["tri_hot"], snap["tri_cold"])
        if want.shape != snap["rows4"].shape:
            out.add(9, "rows4", [0], f"{snap['rows4'].shape[0]} units, expected {want.shape[0]}")
        else:
            out.flag(9, "rows4", want != snap["rows4"], "unit is not the 4-wide node / triangle it was built from")


# ---- whole snapshots -------------------------------------------------------------------------------------------------------------

def _blas_tree(snap, out):
    """the walk of the triangle-holding part of a snapshot: the whole tree of a flat scene, every BLAS of a two-level one"""
    n_tris = snap["tri_hot"].shape[0]
    if snap.get("two_level"):
        roots = np.unique(snap["instances"]["root"])
        return walk2(snap["nodes"], roots, int(snap["tlas_cap"]), snap["nodes"].shape[0], n_tris, out, wrapped_ok=False)
    return walk2(snap["nodes"], [0], 0, snap["nodes"].shape[0], n_tris, out, cover=True)


def _root_box(nodes, root):
    g = nodes[root]
    return np.minimum(g["left_min"], g["right_min"]), np.maximum(g["left_max"], g["right_max"])


def check_flat(snap, input_tris=None, leaf_boxes="device", nodes32=None, skip=()):
    """Every rule that applies to a flat scene's snapshot.  input_tris: the mrt_tri64 array the scene was made from (rule 5).
    leaf_boxes: "device" (the library computed them: every device build, every refit), "host" (the caller's: nodes32 = the uploaded
    mrt_bvh_node32 array).  skip: rule numbers to leave out (the tests delete rules to prove each one is needed)."""
    out = _Out()
    nodes, hot = snap["nodes"], snap["tri_hot"]
    n_tris = hot.shape[0]
    t = walk2(nodes, [0], 0, nodes.shape[0], n_tris, out, cover=True)
    check_leaf_flags(t, hot["flags"], out)
    if 2 not in skip:
        check_nesting(nodes, t, out)
    if 3 not in skip:
        if leaf_boxes == "device":
            mn, mx = slot_boxes_device(hot)
            check_leaf_boxes(t, mn, mx, out, "the bounds of v0, v0 + e1, v0 + e2 one ulp outwards")
        else:
            mn, mx = host_leaf_boxes(nodes32, n_tris)
            check_leaf_boxes(t, mn, mx, out, "the uploaded leaf box")
    if input_tris is not None and 5 not in skip:
        check_triangles(snap, input_tris, out)
    if snap.get("parent") is not None and 6 not in skip:
        check_parents(snap, t, 0, out)
    _tree_signatures(t, n_tris)
    binary = lambda n_wide: 0 if n_wide == nodes.shape[0] and n_wide > 1 else None
    if snap.get("nodes4") is not None and 7 not in skip:
        check_wide(4, snap["nodes4"], [0], t, [0], binary(snap["nodes4"].shape[0]), n_tris, int(snap["stack4"]), 0, out)
    if snap.get("nodes8") is not None and 8 not in skip:
        check_wide(8, snap["nodes8"], [0], t, [0], binary(snap["nodes8"].shape[0]), n_tris, int(snap["stack8"]), 0, out, snap.get("leaf_box"))
    if 9 not in skip:
        check_rows(snap, out)
    if 10 not in skip:
        if int(snap["depth"]) < t.depth_levels + 1:
            out.add(10, "depth", [0], f"stack need {snap['depth']} below the tree's {t.depth_levels + 1}")
        check_bounds(snap, nodes, out)
    return [f for f in out if f.rule not in skip]


def check_bounds(snap, nodes, out):
    if snap.get("bounds_lo") is None:
        return
    mn, mx = _root_box(nodes, 0)
    if _differ(snap["bounds_lo"], mn).any() or _differ(snap["bounds_hi"], mx).any():
        out.add(10, "bounds", [0], "scene bounds are not the root's box")
    if snap.get("scene_abs_max") is not None:
        want = np.float32(max(np.abs(snap["bounds_lo"]).max(), np.abs(snap["bounds_hi"]).max()))
        if _bits(want) != _bits(snap["scene_abs_max"]):
            out.add(10, "scene_abs_max", [0], "not the largest absolute bound")


def invert_affine(basis, origin):
    """instance_math.h invert_affine restated: cofactors in float64, each element rounded once to float32; (n, 12)"""
    B = basis.astype(np.float64).reshape(-1, 9)
    o = origin.astype(np.float64).reshape(-1, 3)
    a, b, c, d, e, f, g, h, i = (B[:, k] for k in range(9))
    c00, c01, c02 = e * i - f * h, c * h - b * i, b * f - c * e
    c10, c11, c12 = f * g - d * i, a * i - c * g, c * d - a * f
    c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
    det = a * c00 + b * c10 + c * c20
    m = np.stack([c00, c01, c02, c10, c11, c12, c20, c21, c22], axis=1) / det[:, None]
    inv = np.empty((B.shape[0], 12), dtype=np.float64)
    for r in range(3):
        t = -(m[:, 3 * r] * o[:, 0] + m[:, 3 * r + 1] * o[:, 1] + m[:, 3 * r + 2] * o[:, 2])
        inv[:, 4 * r:4 * r + 3] = m[:, 3 * r:3 * r + 3]
        inv[:, 4 * r + 3] = t
    return inv.astype(np.float32)


def world_box(lo, hi, basis, origin):
    """instance_math.h world_box restated: the eight corners in float64, rounded outwards to float32; (n, 3) each"""
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    B = basis.astype(np.float64).reshape(-1, 3, 3)
    o = origin.astype(np.float64).reshape(-1, 3)
    mn = np.full(o.shape, np.inf)
    mx = np.full(o.shape, -np.inf)
    for k in range(8):
        x = np.where(k & 1, hi[:, 0], lo[:, 0])
        y = np.where(k & 2, hi[:, 1], lo[:, 1])
        z = np.where(k & 4, hi[:, 2], lo[:, 2])
        for r in range(3):
            w = ((B[:, r, 0] * x + B[:, r, 1] * y) + B[:, r, 2] * z) + o[:, r]
            mn[:, r] = np.where(w < mn[:, r], w, mn[:, r])
            mx[:, r] = np.where(w > mx[:, r], w, mx[:, r])
    l, u = mn.astype(np.float32), mx.astype(np.float32)
    l = np.where(l.astype(np.float64) > mn, np.nextafter(l, np.float32(-np.inf)), l)
    u = np.where(u.astype(np.float64) < mx, np.nextafter(u, np.float32(np.inf)), u)
    return l.astype(np.float32), u.astype(np.float32)


def mesh_triangles(verts9, first_tri, n_tris):
    """make_tri64 (csrc/build_rules.h) restated for one mesh of a two-level scene: mesh-local ids, all layers (float32, nothing contracted)"""
    from messyerraytracer_amd import types as T
    v = np.ascontiguousarray(verts9, dtype=np.float32).reshape(-1, 3, 3)[first_tri:first_tri + n_tris]
    out = np.zeros(n_tris, dtype=T.TRI64)
    a, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    nn = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    l2 = (nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1]) + nn[:, 2] * nn[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.sqrt(l2)
        nn = np.where((l2 == 0)[:, None], np.float32(0), nn / l[:, None]).astype(np.float32)
    out["v0"], out["edge1"], out["edge2"], out["normal"] = a, e1, e2, nn
    out["id"] = np.arange(n_tris, dtype=np.uint32)
    out["layers"] = 0xFFFFFFFF
    return out


def check_two_level(snap, verts9, input_instances, leaf_boxes="device", skip=()):
    """Every rule that applies to a two-level scene's snapshot.  verts9 / input_instances: what the scene was uploaded, refit or
    updated with last.  leaf_boxes: "device" (device-built BLASes, or any refit), "host" (host-built BLASes: the exact bounds of the
    triangles' vertices, which is what the host builder boxes a leaf by)."""
    out = _Out()
    nodes, hot, inst = snap["nodes"], snap["tri_hot"], snap["instances"]
    n_tris, n_inst, cap = hot.shape[0], inst.shape[0], int(snap["tlas_cap"])
    n_tlas = int(snap["n_tlas_nodes"])
    # ---- rule 11: the top level over the instance rows
    tl = walk2(nodes, [0], 0, n_tlas, n_inst, out, cover=True)
    check_leaf_flags(tl, inst["flags"], out, array="instances")
    if n_inst != input_instances.shape[0]:
        out.add(11, "instances", [0], f"{n_inst} rows for {input_instances.shape[0]} instances")
        return list(out)
    idx = inst["index"].astype(np.int64)
    out.flag(11, "instances", idx >= n_inst, "registration index out of range")
    idx = np.minimum(idx, n_inst - 1)
    out.flag(11, "instances", np.bincount(idx, minlength=n_inst)[idx] > 1, "registration index appears more than once")
    src = input_instances[idx]
    id_base = np.concatenate([[0], np.cumsum(input_instances["n_tris"].astype(np.int64))[:-1]])
    out.flag(11, "instances", inst["id_base"] != id_base[idx], "id_base is not the running triangle count of the instances before it")
    out.flag(11, "instances", inst["layers"] != src["layers"], "layers are not the input instance's")
    out.flag(11, "instances", _differ(inst["basis"], src["basis"], False), "basis is not the input instance's")
    out.flag(11, "instances", (inst["root"] < cap) | (inst["root"] >= nodes.shape[0]), "BLAS root outside the BLAS rows")
    # one root per distinct mesh, the same for every instance of a mesh
    mesh_key = src["first_tri"].astype(np.int64) << 32 | src["n_tris"].astype(np.int64)
    def spread(group, value):  # per row: does its group hold more than one value?
        o = np.argsort(group, kind="stable")
        starts = np.flatnonzero(np.concatenate([[True], group[o][1:] != group[o][:-1]]))
        lo_v, hi_v = np.minimum.reduceat(value[o], starts), np.maximum.reduceat(value[o], starts)
        which = np.cumsum(np.concatenate([[0], (group[o][1:] != group[o][:-1]).astype(np.int64)]))
        res = np.zeros(group.shape[0], dtype=bool)
        res[o] = (lo_v != hi_v)[which]
        return res
    root64 = inst["root"].astype(np.int64)
    out.flag(11, "instances", spread(mesh_key, root64), "instances of one mesh disagree on its BLAS root")
    out.flag(11, "instances", spread(root64, mesh_key), "two meshes share one BLAS root")
    if any(f.rule == 11 and "root" in f.message for f in out):
        return list(out)  # which rows are whose BLAS is not known: the per-BLAS rules have nothing to stand on
    # ---- per BLAS: the flat rules over the BLAS rows
    roots, first_of = np.unique(inst["root"], return_index=True)
    roots = roots.astype(np.int64)
    t = walk2(nodes, roots, cap, nodes.shape[0], n_tris, out, wrapped_ok=False)
    both = np.zeros(nodes.shape[0], dtype=np.int64)
    both[tl.order] += 1
    both[t.order] += 1
    out.flag(1, "nodes", both > 1, "node belongs to the TLAS and to a BLAS")
    check_leaf_flags(t, hot["flags"], out)
    if 2 not in skip:
        check_nesting(nodes, tl, out)
        check_nesting(nodes, t, out)
    # the slot range and the mesh of every BLAS: a BLAS's slots follow each other in the order of first use of the meshes
    _tree_signatures(t, n_tris)
    mesh_first, mesh_n = src["first_tri"][first_of].astype(np.int64), src["n_tris"][first_of].astype(np.int64)
    # the registration index at which a mesh is first used orders the BLASes' slot ranges
    by_root = np.argsort(inst["root"], kind="stable")
    first_use = np.minimum.reduceat(idx[by_root], np.searchsorted(inst["root"][by_root], roots))
    blas_order = np.argsort(first_use, kind="stable")
    slot_base = np.zeros(roots.size, dtype=np.int64)
    slot_base[blas_order] = np.concatenate([[0], np.cumsum(mesh_n[blas_order])[:-1]])
    want_sig = t.csum[np.minimum(slot_base + mesh_n, n_tris)] - t.csum[np.minimum(slot_base, n_tris)]
    out.flag(1, "nodes", t.n_sig[t.pos[roots]] != want_sig, "BLAS does not hold exactly its mesh's slot range", roots)
    tris = np.concatenate([mesh_triangles(verts9, int(mesh_first[b]), int(mesh_n[b])) for b in blas_order])
    if 5 not in skip:
        # slot -> staged triangle: the slot map if a refit made one, else the mesh-local id within the BLAS's range
        base_of_slot = np.repeat(slot_base[blas_order], mesh_n[blas_order])[:n_tris]
        by_id = base_of_slot + np.minimum(hot["id"].astype(np.int64), np.repeat(mesh_n[blas_order], mesh_n[blas_order])[:n_tris] - 1)
        if snap.get("slot_src") is not None:
            out.flag(5, "slot_src", snap["slot_src"].astype(np.int64) != by_id, "entry is not the BLAS's slot base + the slot's mesh-local id")
        check_triangles(snap, tris, out, slot_src=by_id.astype(np.uint32))
    if 3 not in skip:
        if leaf_boxes == "device":
            mn, mx = slot_boxes_device(hot)
            check_leaf_boxes(t, mn, mx, out, "the bounds of v0, v0 + e1, v0 + e2 one ulp outwards")
        else:
            v = np.concatenate([np.ascontiguousarray(verts9, dtype=np.float32).reshape(-1, 3, 3)[int(mesh_first[b]):int(mesh_first[b] + mesh_n[b])] for b in blas_order])
            mn, mx = vertex_boxes(v, by_id if 5 not in skip else np.arange(n_tris))
            check_leaf_boxes(t, mn, mx, out, "the bounds of the mesh triangles' vertices")
    if snap.get("parent") is not None and 6 not in skip:
        check_parents(snap, t, cap, out)
    blas_levels = np.array([t.level[t.order].max() if t.order.size else 0])  # levels are counted from every BLAS root at 1
    if snap.get("nodes8") is not None and 8 not in skip:
        n8 = snap["nodes8"].shape[0]
        root8 = inst["root8"][first_of].astype(np.int64)
        binary = cap if n8 == nodes.shape[0] - cap and bool((root8 == roots - cap).all()) else None
        # stack8 = the TLAS path + the rest of a TLAS leaf + the return marker + the deepest 8-wide BLAS walk
        check_wide(8, snap["nodes8"], root8, t, roots, binary, n_tris, int(snap["stack8"]), tl.depth_levels + 1 + 2, out, snap.get("leaf_box"))
    # ---- rule 12: inverse transforms and the TLAS leaf boxes
    if 12 not in skip:
        out.flag(12, "instances", _differ(inst["inv"], invert_affine(src["basis"], src["origin"]), False), "inv is not invert_affine of the input transform")
        rmn = np.minimum(nodes["left_min"][inst["root"]], nodes["right_min"][inst["root"]])
        rmx = np.maximum(nodes["left_max"][inst["root"]], nodes["right_max"][inst["root"]])
        wmn, wmx = world_box(rmn, rmx, src["basis"], src["origin"])
        tops = _Out()
        check_leaf_boxes(tl, wmn, wmx, tops, "the union of its instances' world boxes", array="nodes")
        out.extend(f._replace(rule=12) for f in tops)
    if 10 not in skip:
        need = tl.depth_levels + 1 + 2 + int(blas_levels.max()) + 1
        if int(snap["depth"]) < need:
            out.add(10, "depth", [0], f"stack need {snap['depth']} below the trees' {need}")
        check_bounds(snap, nodes, out)
    return [f for f in out if f.rule not in skip]


def summary(findings, limit=12):
    lines = [f"rule {f.rule} {f.array}[{f.element}]: {f.message}" for f in findings[:limit]]
    if len(findings) > limit:
        lines.append(f"... {len(findings) - limit} more")
    return "\n".join(lines) or "no findings"
