"""The library on a caller's HIP stream (mrt_set_stream), every call held to stream order: what bench.py, the tools and mrt_group do,
and what no other test does.  The caller is messyerraytracer_amd/test_support/stream_gate.cpp (libmrt_stream_gate.so: a
non-blocking stream, device-to-device copies on it, and a gate -- a host function queued on the stream that sleeps a fixed time, so that everything queued behind it is held
back while the calls under test are made).

One pattern throughout, the gated sequence.  Every device input exists twice: a staged buffer with the data, and the live buffer the
library is given, which starts as a well-formed decoy (rays that miss everything, miss records, MRT_TOKEN_MISS tokens, the old triangles
or instances, zero images).  On the caller's stream S: the gate, the copies staged -> live, the library calls (MRT_FLAG_ASYNC where they
take it), the copies of every output to a result buffer.  The test waits for S alone and then reads.  A call that read its input before
the caller's copy, ran any part of itself on another stream, or left its output incomplete for the caller's copy gives decoy-derived or
stale bytes -- a wrong answer, never a fault.  For an ASYNC call the gate must still be closed when the call returns (it returned without
waiting, and nothing of it can have run yet); a blocking call returns after the gate.  Expected values are the oracle's and the numpy
restatements'; the same sequence run ungated and blocking on the context's own stream (the warm-up, which also lets first calls
allocate and plan) must give the same bytes.  Guard bytes behind every output.

Gate length: the longest host time from launching a gate to the return of the last ASYNC call behind it, over all sequences of this
file on an MI355X host, was 0.31 ms (GATE_OBSERVED_MS: the path-traced loop's 36 calls; a single cast takes 0.02 - 0.07 ms); the
gate is GATE_MS = 50 ms, the value it started from, 160 x that.  hipLaunchHostFunc holds the stream back (the first test); no
device-side filler is needed.  No case is marked as waiting: the only calls that return after the gate are the blocking ones the
header names (scene changes, uploads, mrt_set_stream), and the tests require exactly that of them.

What records cannot show: work whose only effect is a launch order.  The sorted path's permutation and the tile schedule's order
are permutations whatever they were computed from, so a sort moved to another stream changes no record.  The sorted path's order is
therefore read back and held to its own cast (mrt_debug_sort_order), the tile schedule's use is counted (mrt_schedule_counts: which
frames launched a measured order, how many sorts were queued) -- its order itself comes from measured cycles and has no expected
value --, and casts are queued twice behind one gate, where per-context scratch that does decide records (the persistent walk's
ray counters) is shared."""
import ctypes as C
import time

import numpy as np
import pytest

from messyerraytracer_amd import build, capi, synth, types as T
from oracle import pyoracle as po
import parity
from test_hemisphere_gpu import Dev, scene

pytestmark = pytest.mark.gpu

F = np.float32
GATE_OBSERVED_MS = 0.31   # (measured: see the module docstring)
GATE_MS = 50
GUARD = 256               # bytes behind every output
PATTERN = 0xA5
ASYNC = capi.FLAG_ASYNC
DEV = capi.FLAG_RAYS_ON_DEVICE | capi.FLAG_HITS_ON_DEVICE
FAR = F(1e30)
ENQUEUE_MS = {}           # sequence -> host ms from the gate's launch to the return of the last ASYNC call behind it


# ---- the caller ---------------------------------------------------------------------------------------------------------------------

_GATE_LIB = None


def gate_lib():
    global _GATE_LIB
    if _GATE_LIB is None:
        capi.load()                                       # (first: both link the same HIP runtime)
        L = C.CDLL(build.STREAM_GATE)
        L.sg_stream_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.sg_stream_destroy.argtypes = [C.c_void_p]
        L.sg_stream_synchronize.argtypes = [C.c_void_p]
        L.sg_gate.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.sg_gate_started.argtypes = L.sg_gate_done.argtypes = L.sg_gate_free.argtypes = [C.c_void_p]
        L.sg_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        _GATE_LIB = L
    return _GATE_LIB


def hip_ok(rc, what):
    assert rc == 0, f"{what}: hipError_t {rc}"


class Gate:
    def __init__(self, L, h):
        self.L, self.h = L, h

    def started(self):
        return self.L.sg_gate_started(self.h)

    def done(self):
        return self.L.sg_gate_done(self.h)

    def free(self):
        assert self.L.sg_gate_free(self.h) == 0, "the gate is still closed"


class Caller:
    """a renderer's own stream: a gate, copies and a wait"""

    def __init__(self):
        self.L = gate_lib()
        s = C.c_void_p()
        hip_ok(self.L.sg_stream_create(0, C.byref(s)), "hipStreamCreateWithFlags")
        self.s = s.value

    def gate(self, ms=GATE_MS):
        h = C.c_void_p()
        hip_ok(self.L.sg_gate(self.s, ms, C.byref(h)), "hipLaunchHostFunc")
        return Gate(self.L, h.value)

    def copy(self, dst, src, nbytes):
        hip_ok(self.L.sg_copy(self.s, dst, src, nbytes), "hipMemcpyAsync")

    def sync(self):
        hip_ok(self.L.sg_stream_synchronize(self.s), "hipStreamSynchronize")

    def destroy(self):
        if self.s:
            hip_ok(self.L.sg_stream_destroy(self.s), "hipStreamDestroy")
            self.s = None


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class In:
    """a device input: `staged` holds the data, `live` -- what the library is given -- starts as the decoy"""

    def __init__(self, dev, data, decoy):
        self.dev, self.data, self.decoy = dev, raw(data).copy(), raw(decoy).copy()
        assert self.data.shape == self.decoy.shape and not np.array_equal(self.data, self.decoy)
        self.n = self.data.shape[0]
        self.staged, self.live = dev.put(self.data), dev.put(self.decoy)

    def reset(self):
        self.dev.ctx.h2d(self.live, self.decoy)

    def fill(self):
        self.dev.ctx.h2d(self.live, self.data)

    def check(self, what=""):
        np.testing.assert_array_equal(self.dev.get(self.live, self.n, np.uint8), self.data, err_msg=what + ": the live input is not the staged data")


class Out:
    """a device output of the library (or a buffer it updates in place, starting as `init`) with guard bytes behind it, and the result
    buffer the caller copies it to"""

    def __init__(self, dev, nbytes, init=None):
        self.dev, self.n = dev, int(nbytes)
        first = np.full(self.n, PATTERN, np.uint8) if init is None else raw(init).copy()
        assert first.shape[0] == self.n
        self.start = np.concatenate([first, np.full(GUARD, PATTERN, np.uint8)])
        self.out, self.res = dev.put(self.start), dev.put(np.full(self.n + GUARD, PATTERN, np.uint8))

    def reset(self):
        self.dev.ctx.h2d(self.out, self.start)
        self.dev.ctx.h2d(self.res, np.full(self.n + GUARD, PATTERN, np.uint8))

    def read_out(self, what=""):
        got = self.dev.get(self.out, self.n + GUARD, np.uint8)
        assert (got[self.n:] == PATTERN).all(), what + ": guard bytes behind the output overwritten"
        return got[:self.n]

    def read(self, what=""):
        """the result buffer; the output itself holds the same"""
        got = self.dev.get(self.res, self.n + GUARD, np.uint8)
        assert (got[self.n:] == PATTERN).all(), what + ": guard bytes behind the result overwritten"
        np.testing.assert_array_equal(self.read_out(what), got[:self.n], err_msg=what + ": the result is not the output")
        return got[:self.n]


def note(what, ms, done):
    ENQUEUE_MS[what] = max(ms, ENQUEUE_MS.get(what, 0.0))
    print(f"[caller-stream] {what}: {ms:.3f} ms from the gate to the return of the last ASYNC call (gate done then: {done}); "
          f"longest so far {max(ENQUEUE_MS.values()):.3f} ms, gate {GATE_MS} ms")


def warm(ctx, ins, outs, calls, what):
    """The sequence ungated and blocking on the context's own stream: first calls allocate, load and plan here.  Returns the outputs'
    bytes."""
    ctx.set_stream(0)
    for b in list(ins) + list(outs):
        b.reset()
    for i in ins:
        i.fill()
    calls(0)
    return [o.read_out(what + " (own stream)") for o in outs]


def gated(ctx, cs, ins, outs, calls, what, waits=False):
    """The gated sequence on the caller's stream; `calls(ASYNC)` makes the library calls.  waits: the calls are known to wait for the
    stream (the header says so): the gate is open when they return.  Returns the result buffers' bytes."""
    ctx.set_stream(cs.s)
    for b in list(ins) + list(outs):
        b.reset()                                     # (mrt_memcpy_h2d: waits for S, on which nothing is gated yet)
    t0 = time.perf_counter()
    g = cs.gate()
    for i in ins:
        cs.copy(i.live, i.staged, i.n)
    calls(ASYNC)
    ms = (time.perf_counter() - t0) * 1e3
    done = g.done()
    for o in outs:
        cs.copy(o.res, o.out, o.n)
    cs.sync()                                         # the only wait: no mrt_synchronize, no mrt_memcpy_* before it
    assert g.done() == 1
    g.free()
    if waits:
        assert done == 1, f"{what}: a call that waits for the stream returned while the gate was closed"
    else:
        note(what, ms, done)
        assert done == 0, (f"{what}: the gate had opened when the last ASYNC call returned ({ms:.1f} ms after its launch, gate {GATE_MS} ms): "
                           "a call waited for the stream, or the gate is too short for this host")
    got = [o.read(what) for o in outs]
    for i in ins:
        i.check(what)
    return got


def sequence(ctx, cs, ins, outs, calls, what, waits=False):
    """warm-up, then the gated run; the two must agree byte for byte.  Returns (result bytes, the variant the warm-up's last cast ran)."""
    own = warm(ctx, ins, outs, calls, what)
    variant, stats = ctx.last_kernel_variant(), ctx.stats()
    got = gated(ctx, cs, ins, outs, calls, what, waits)
    for k, (a, b) in enumerate(zip(got, own)):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: output {k} on the caller's stream differs from the own-stream run")
    print(f"[caller-stream] {what}: {variant} ({stats['last_kernel_launches']} launches)")
    return got, variant, stats


# ---- inputs and expectations, made once -----------------------------------------------------------------------------------------------

WANT = {}


def decoy_rays(n):
    """valid rays that start far outside every scene and point away from it"""
    r = np.zeros(n, T.RAY32)
    r["origin"], r["direction"], r["t_min"], r["t_max"] = (1000.0, 1000.0, 1000.0), (1.0, 0.0, 0.0), F(1e-3), FAR
    return r


def miss_records(n):
    h = np.zeros(n, T.HIT32)
    h["prim_id"] = -1
    return h


def incoherent(kind, n):
    if (kind, n) not in WANT:
        rays = synth.incoherent_rays(n, 17)
        WANT[(kind, n)] = (rays, scene(kind).oracle(rays))
    return WANT[(kind, n)]


def grid(kind, w, h, query_mask=0xFFFFFFFF):
    if (kind, w, h, query_mask) not in WANT:
        o, f, fov = scene(kind).cam
        rays = po.grid_rays(o, f, w, h, fov)
        WANT[(kind, w, h, query_mask)] = (rays, scene(kind).oracle(rays, query_mask))
    return WANT[(kind, w, h, query_mask)]


def camera(kind, w, h):
    o, f, fov = scene(kind).cam
    return capi.camera_look(o, f, w, h, fov)


def hits_of(b):
    return b.view(T.HIT32)


def check_records(got, want, what):
    got = hits_of(got)
    assert not (raw(got).reshape(-1, 32) == PATTERN).all(axis=1).any(), what + ": records never written"
    parity.assert_exact(got, want, what)
    assert (want["prim_id"] >= 0).any() and (want["prim_id"] < 0).any()


class Rig:
    """a context with a scene resident, its device buffers and a caller's stream"""

    def __init__(self, kind, **opts):
        self.kind, self.ctx = kind, capi.Context(0, **opts)
        self.dev, self.cs = Dev(self.ctx), Caller()
        scene(kind).upload(self.ctx)

    def close(self):
        self.ctx.set_stream(0)
        self.dev.free()
        self.ctx.close()
        self.cs.destroy()


@pytest.fixture
def soup(built):
    r = Rig("soup")
    yield r
    r.close()


# ---- 0. the gate itself ----------------------------------------------------------------------------------------------------------------

def test_the_gate_holds_a_stream_back(built):
    """hipLaunchHostFunc as the gate: a copy queued behind it has not run while it is closed (read through another context, whose
    copies are on another stream), and has once the stream is waited for; the wait lasts about as long as the gate."""
    reader = capi.Context(0)
    dev, cs = Dev(reader), Caller()
    try:
        data = np.arange(1 << 16, dtype=np.uint32)
        src, dst = dev.put(data), dev.put(np.full(1 << 16, 0xA5A5A5A5, np.uint32))
        t0 = time.perf_counter()
        g = cs.gate(200)
        cs.copy(dst, src, data.nbytes)
        seen = dev.get(dst, 1 << 16, np.uint32)                  # while the gate is closed
        closed = g.done() == 0
        cs.sync()
        ms = (time.perf_counter() - t0) * 1e3
        assert g.started() == 1 and g.done() == 1
        assert closed, "the read-back took longer than the gate: nothing was observed"
        assert (seen == 0xA5A5A5A5).all(), "a copy queued behind the gate ran while it was closed"
        np.testing.assert_array_equal(dev.get(dst, 1 << 16, np.uint32), data)
        assert ms >= 190.0, f"the stream was waited for in {ms:.1f} ms, the gate sleeps 200 ms"
        g.free()
    finally:
        dev.free()
        reader.close()
        cs.destroy()


# ---- 1. array casts ----------------------------------------------------------------------------------------------------------------------

ARRAY_CASES = {
    # name: (rays, FLAG_COHERENT, what the warm-up's variant starts with, its launches)
    "lane-4096": (4096, 0, "trace_lane_kernel<false", 1),
    "keys-8193": (8193, 0, "trace_lane_kernel<false", 3),
    "persistent-65536": (65536, 0, "trace_lane_persistent_kernel<false, 8,", 3),
    "coherent-64x64": ((64, 64), capi.FLAG_COHERENT, "trace_packet_asm_kernel<false", 2),
}


@pytest.mark.parametrize("case", list(ARRAY_CASES))
def test_array_cast(soup, case):
    """mrt_cast, rays and hits on the device, ASYNC: the lane kernel, the sorted path (keys, rocPRIM sort, permuted trace), the
    persistent 8-wide walk (its ray counters and overflow buffer), and detect + packet walk for a coherent batch."""
    size, coh, prefix, launches = ARRAY_CASES[case]
    rays, want = grid("soup", *size) if coh else incoherent("soup", size)
    n = rays.shape[0]
    d_rays, outs = In(soup.dev, rays, decoy_rays(n)), [Out(soup.dev, n * 32) for _ in range(2)]

    def calls(a):                                                 # twice behind one gate: the casts share the context's work buffers
        for o in outs:
            soup.ctx.cast(d_rays.live, o.out, count=n, flags=DEV | coh | a)

    got, variant, stats = sequence(soup.ctx, soup.cs, [d_rays], outs, calls, "array cast " + case)
    assert variant.startswith(prefix) and stats["last_kernel_launches"] == launches, (variant, stats["last_kernel_launches"])
    if coh:
        assert stats["detected_grid_w"] == size[0]
    for k in range(2):
        check_records(got[k], want, f"{case}, cast {k}")


def test_sorted_cast_walks_its_own_order(soup):
    """The sort of the sorted path decides no record (any order of the rays gives the same ones), so the records cannot show a sort
    that ran on another stream, before the keys of its cast were made.  The order itself can: between the warm-up and the gated cast
    another batch of as many rays is cast, so that what the key and index buffers hold is not this cast's; after the gated cast
    mrt_debug_sort_order must give the warm-up's order of these rays, a permutation, and not the other batch's."""
    n = 8193
    rays, want = incoherent("soup", n)
    other = synth.incoherent_rays(n, 99)
    d_rays, d_hits = In(soup.dev, rays, decoy_rays(n)), Out(soup.dev, n * 32)
    ctx = soup.ctx

    def cast(a):
        ctx.cast(d_rays.live, d_hits.out, count=n, flags=DEV | a)

    own = warm(ctx, [d_rays], [d_hits], cast, "sorted cast order")
    assert ctx.stats()["last_kernel_launches"] == 3
    order = ctx.debug_sort_order(n)
    np.testing.assert_array_equal(np.sort(order), np.arange(n, dtype=np.uint32))
    ctx.cast(other)                                               # blocking, from the host: the same buffers, another batch's keys
    assert ctx.stats()["last_kernel_launches"] == 3
    assert (ctx.debug_sort_order(n) != order).any()
    (got,) = gated(ctx, soup.cs, [d_rays], [d_hits], cast, "sorted cast order")
    np.testing.assert_array_equal(got, own[0])
    check_records(got, want, "sorted cast")
    np.testing.assert_array_equal(ctx.debug_sort_order(n), order, err_msg="the cast walked an order that is not of its own rays")


def test_any_hit_bool_out(soup):
    rays, want = incoherent("soup", 4096)
    n = rays.shape[0]
    d_rays, d_out = In(soup.dev, rays, decoy_rays(n)), Out(soup.dev, n)
    (got,), variant, _ = sequence(soup.ctx, soup.cs, [d_rays], [d_out],
                                  lambda a: soup.ctx.cast(d_rays.live, d_out.out, count=n, mode=capi.MODE_ANY_HIT, flags=DEV | capi.FLAG_BOOL_OUT | a),
                                  "any-hit BOOL_OUT")
    assert variant.startswith("trace_lane_kernel<true")
    assert (got <= 1).all(), "bytes never written"
    np.testing.assert_array_equal(got.astype(bool), want["prim_id"] >= 0)
    assert got.any() and not got.all()


def token_sequence(rig, rays, want, explicit, what):
    """TOKEN_OUT, then mrt_expand_tokens on the context's stream (hip_stream = 0) or on S passed explicitly"""
    ctx, n, tb = rig.ctx, rays.shape[0], rig.ctx.token_bytes()
    d_rays = In(rig.dev, rays, decoy_rays(n))
    d_tok, d_hits = Out(rig.dev, n * tb, np.full(n * tb, 0xFF, np.uint8)), Out(rig.dev, n * 32)      # (tokens start as MRT_TOKEN_MISS)

    def calls(a):
        ctx.cast(d_rays.live, d_tok.out, count=n, flags=DEV | capi.FLAG_TOKEN_OUT | a)
        ctx.expand_tokens(d_rays.live, d_tok.out, d_hits.out, n, stream=rig.cs.s if explicit and a else None)
        if not a:
            ctx.synchronize()                                     # (mrt_expand_tokens never waits)

    (tok, got), _, _ = sequence(ctx, rig.cs, [d_rays], [d_tok, d_hits], calls, what)
    first = tok.view(np.uint32).reshape(n, tb // 4)[:, 0]
    np.testing.assert_array_equal(first != capi.TOKEN_MISS, want["prim_id"] >= 0, err_msg=what + ": tokens")
    check_records(got, want, what)


@pytest.mark.parametrize("explicit", [False, True], ids=["stream0", "streamS"])
def test_tokens_then_expand(soup, explicit):
    rays, want = incoherent("soup", 4096)
    assert soup.ctx.token_bytes() == 4
    token_sequence(soup, rays, want, explicit, "TOKEN_OUT + expand, " + ("S passed" if explicit else "hip_stream 0"))


def test_two_level_cast_and_tokens(built):
    """the same closest-hit cast on the two-level room, and its 8-byte tokens expanded"""
    rig = Rig("room_tl")
    try:
        rays, want = grid("room_tl", 64, 64)
        n = rays.shape[0]
        d_rays, d_hits = In(rig.dev, rays, decoy_rays(n)), Out(rig.dev, n * 32)
        (got,), variant, _ = sequence(rig.ctx, rig.cs, [d_rays], [d_hits], lambda a: rig.ctx.cast(d_rays.live, d_hits.out, count=n, flags=DEV | a),
                                      "two-level array cast")
        assert variant.startswith("trace_two_level_kernel<false"), variant
        got = hits_of(got)
        parity.assert_exact(got, want, "two-level array cast")
        assert (want["prim_id"] >= 0).any()
        assert rig.ctx.token_bytes() == 8
        d_rays2 = In(rig.dev, rays, decoy_rays(n))
        d_tok, d_exp = Out(rig.dev, n * 8, np.full(n * 8, 0xFF, np.uint8)), Out(rig.dev, n * 32)

        def calls(a):
            rig.ctx.cast(d_rays2.live, d_tok.out, count=n, flags=DEV | capi.FLAG_TOKEN_OUT | a)
            rig.ctx.expand_tokens(d_rays2.live, d_tok.out, d_exp.out, n)
            if not a:
                rig.ctx.synchronize()

        (_, exp), _, _ = sequence(rig.ctx, rig.cs, [d_rays2], [d_tok, d_exp], calls, "two-level TOKEN_OUT + expand")
        parity.assert_exact(hits_of(exp), want, "two-level tokens expanded")
    finally:
        rig.close()


# ---- 2. grid casts -----------------------------------------------------------------------------------------------------------------------

def test_grid_cast_into_device_records(soup):
    rays, want = grid("soup", 64, 64)
    cam, n = camera("soup", 64, 64), 64 * 64
    d_hits = Out(soup.dev, n * 32)
    (got,), variant, _ = sequence(soup.ctx, soup.cs, [], [d_hits],
                                  lambda a: soup.ctx.cast_grid(cam, 64, 64, hits=d_hits.out, flags=capi.FLAG_HITS_ON_DEVICE | a), "grid cast 64x64")
    assert variant.startswith("trace_packet_asm_kernel<false"), variant
    check_records(got, want, "grid cast 64x64")


def test_scheduled_frames_behind_one_gate(built, monkeypatch):
    """MRT_SCHEDULE_MIN_LOG2=15, a 256 x 128 grid of the forced 64-ray packet kernel, the output poison on: eight blocking frames (the
    warm-up and four more, so that the next frame is one that renews the order), the scene uploaded again (its orders are forgotten,
    its arrays kept), then four ASYNC frames into four buffers behind one gate -- the first notes its costs and queues their sort on
    the schedule's side stream, none of the four can see that sort finished -- and four more ungated, launched in measured orders.
    mrt_schedule_counts says which of these each frame took.  All eight against the oracle; an untraced tile would keep the poison."""
    monkeypatch.setenv("MRT_POISON_OUTPUT", "1")
    monkeypatch.setenv("MRT_SCHEDULE_MIN_LOG2", "15")
    rig = Rig("soup", kernel=capi.KERNEL_PACKET_ASM)
    try:
        ctx, w, h = rig.ctx, 256, 128
        rays, want = grid("soup", w, h)
        cam, n = camera("soup", w, h), w * h
        outs = [Out(rig.dev, n * 32) for _ in range(4)]

        def calls(a):
            for o in outs:
                ctx.cast_grid(cam, w, h, hits=o.out, flags=capi.FLAG_HITS_ON_DEVICE | a)

        own = warm(ctx, [], outs, calls, "scheduled frames")
        variant = ctx.last_kernel_variant()
        assert variant.startswith("trace_packet_asm_kernel<false"), variant
        c0 = ctx.schedule_counts()
        assert c0["scheduled"] == 4 and c0["sorts"] >= 1 and c0["ordered"] >= 1, c0      # the grid is under the tile schedule
        calls(0)
        scene("soup").upload(ctx)
        c1 = ctx.schedule_counts()
        got = gated(ctx, rig.cs, [], outs, calls, "four scheduled frames behind one gate")
        c2 = ctx.schedule_counts()
        print(f"[caller-stream] schedule counts: warm-up {c0}, before the gate {c1}, after it {c2}")
        assert c2["scheduled"] == c1["scheduled"] + 4 and c2["sorts"] == c1["sorts"] + 1, (c1, c2)   # one frame's costs were sorted
        assert c2["ordered"] == c1["ordered"], (c1, c2)           # no frame behind the gate saw a finished sort
        for k in range(4):
            check_records(got[k], want, f"gated frame {k}")
            np.testing.assert_array_equal(got[k], own[k])
        for o in outs:
            o.reset()
        calls(ASYNC)                                              # ungated: the sort has finished, its order is launched
        c3 = ctx.schedule_counts()
        assert c3["scheduled"] == c2["scheduled"] + 4 and c3["ordered"] > c2["ordered"], (c2, c3)
        for o in outs:
            rig.cs.copy(o.res, o.out, o.n)
        rig.cs.sync()
        for k, o in enumerate(outs):
            check_records(o.read(), want, f"ungated frame {k}")
    finally:
        rig.close()


def test_detected_width_when_the_library_never_sees_the_wait(built, monkeypatch):
    """Coherent casts of one size (their width found on the device), waited for by the caller's own stream synchronize alone, then a
    larger coherent ASYNC cast behind a gate: planned from nothing the library has not seen complete, every ray of it traced."""
    monkeypatch.setenv("MRT_POISON_OUTPUT", "1")
    monkeypatch.setenv("MRT_SCHEDULE_MIN_LOG2", "15")
    rig = Rig("soup")
    try:
        ctx, cs = rig.ctx, rig.cs
        ra, wa = grid("soup", 256, 128)
        rb, wb = grid("soup", 320, 208)
        na, nb = ra.shape[0], rb.shape[0]
        d_ra, d_rb = In(rig.dev, ra, decoy_rays(na)), In(rig.dev, rb, decoy_rays(nb))
        out_a, out_b = [Out(rig.dev, na * 32) for _ in range(3)], Out(rig.dev, nb * 32)

        def calls(a):
            for o in out_a:
                ctx.cast(d_ra.live, o.out, count=na, flags=DEV | capi.FLAG_COHERENT | a)
                if a:
                    cs.sync()                                     # the caller's wait: the library is not told
            ctx.cast(d_rb.live, out_b.out, count=nb, flags=DEV | capi.FLAG_COHERENT | a)

        own = warm(ctx, [d_ra, d_rb], out_a + [out_b], calls, "detected widths")
        st = ctx.stats()                                          # of the blocking 320 x 208 cast: detect, then the packet walk
        assert st["detected_grid_w"] == 320 and st["last_kernel_launches"] == 2 and st["reserved"] == 0, st
        assert ctx.last_kernel_variant().startswith("trace_packet_"), ctx.last_kernel_variant()
        # the gated run by hand: the first casts are waited for one by one, the gate goes in front of the larger cast
        ctx.set_stream(cs.s)
        for b in [d_ra, d_rb] + out_a + [out_b]:
            b.reset()
        cs.copy(d_ra.live, d_ra.staged, d_ra.n)
        c0 = ctx.schedule_counts()
        for o in out_a:
            ctx.cast(d_ra.live, o.out, count=na, flags=DEV | capi.FLAG_COHERENT | ASYNC)
            cs.sync()
        # (the library saw none of these waits: it may not take the width of one of them for the next, so none is scheduled)
        assert ctx.schedule_counts() == c0, (c0, ctx.schedule_counts())
        t0 = time.perf_counter()
        g = cs.gate()
        cs.copy(d_rb.live, d_rb.staged, d_rb.n)
        ctx.cast(d_rb.live, out_b.out, count=nb, flags=DEV | capi.FLAG_COHERENT | ASYNC)
        ms, done = (time.perf_counter() - t0) * 1e3, g.done()
        for o in out_a + [out_b]:
            cs.copy(o.res, o.out, o.n)
        cs.sync()
        assert g.done() == 1
        g.free()
        note("a larger coherent cast after caller-side waits", ms, done)
        assert done == 0
        for k, o in enumerate(out_a):
            got = o.read()
            check_records(got, wa, f"256x128 coherent cast {k}")
            np.testing.assert_array_equal(got, own[k])
        got = out_b.read()
        check_records(got, wb, "320x208 coherent cast behind the gate")
        np.testing.assert_array_equal(got, own[3])
        d_ra.check()
        d_rb.check()
    finally:
        rig.close()


# ---- 3. whole frames in one queue ------------------------------------------------------------------------------------------------------

def snap(cs, dst, src, nbytes, a):
    """the caller's own copy between two library calls: in stream order behind the gate; after a blocking call, waited for"""
    cs.copy(dst, src, nbytes)
    if not a:
        cs.sync()


def test_a_reflected_frame_in_one_queue(built):
    """synth.room() at 64 x 48, two frames behind one gate, every call ASYNC and no host wait inside: primary grid -> resolve -> shadows
    -> light -> reflection cast -> resolve -> light -> mrt_reflection_guides -> mrt_resolve_reflections (the history carried from frame
    to frame by the caller's copy) -> a channel plane, mrt_image_to_rgba8 -> mrt_accumulate.  Every buffer against the numpy chain of
    test_denoise_gpu.py on the oracle's records."""
    from messyerraytracer_amd import accumulate as A, channels as Ch, denoise as Dn
    from test_denoise_gpu import H, W, reflected_frame, same_floats
    from test_hemisphere_gpu import shadow_mask
    from test_lighting_gpu import environment, light_list
    from test_surface_gpu import shade_data, upload
    rig = Rig("room")
    try:
        ctx, dev, cs, sc = rig.ctx, rig.dev, rig.cs, scene("room")
        shade = shade_data("room")
        upload(ctx, shade)
        lights, env = light_list("room")[:4], environment()
        slights = capi.shadow_lights(lights)
        n, cam, inv_range = W * H, camera("room", W, H), F(1.0 / 12.0)
        rays, hits = grid("room", W, H, 1)                        # layer 1: the sphere and the boxes; the walls are misses
        sizes = dict(hits=32, rows=64, mask=len(lights), lit=16, rhits=32, rrays=32, rrows=64, rlit=16, depth=4, guide=16, color=16,
                     normal=16, rgba8=4, acc8=4, acc=16)
        fr = [{k: Out(dev, n * s) for k, s in sizes.items()} for _ in range(2)]
        fr[0]["hist"], fr[1]["hist"] = Out(dev, n * 16), Out(dev, n * 16)
        accum = Out(dev, n * 16)
        ps = [Dn.params(normal_kind=Dn.NORMAL_WORLD, has_history=f > 0, roughness_threshold=0.9, intensity=2.0) for f in range(2)]
        outs = [b for f in fr for b in f.values()] + [accum]

        def calls(a):
            for f, (b, p) in enumerate(zip(fr, ps)):
                ctx.cast_grid(cam, W, H, hits=b["hits"].out, query_mask=1, flags=capi.FLAG_HITS_ON_DEVICE | a)
                ctx.resolve_grid_surfaces(cam, W, H, b["hits"].out, b["rows"].out, flags=a)
                ctx.cast_grid_shadows(cam, W, H, b["hits"].out, slights, b["mask"].out, flags=a)
                ctx.light_grid_surfaces(cam, W, H, b["hits"].out, b["rows"].out, lights, b["lit"].out, b["mask"].out, env, flags=a)
                ctx.cast_grid_reflections(cam, W, H, b["hits"].out, b["rhits"].out, FAR, d_out_rays=b["rrays"].out, flags=a)
                ctx.resolve_surfaces(b["rrays"].out, b["rhits"].out, n, b["rrows"].out, flags=a)
                ctx.light_surfaces(b["rrays"].out, b["rhits"].out, b["rrows"].out, n, lights, b["rlit"].out, None, env, flags=a)
                Dn.reflection_guides(ctx, b["hits"].out, b["rows"].out, n, inv_range, b["depth"].out, b["guide"].out, flags=a)
                snap(cs, b["color"].out, b["lit"].out, n * 16, a)
                if f:
                    snap(cs, b["hist"].out, fr[f - 1]["hist"].out, n * 16, a)
                Dn.resolve_reflections(ctx, p, W, H, b["rlit"].out, b["depth"].out, b["guide"].out, b["hist"].out, b["color"].out, flags=a)
                ctx.shade_grid_channels(cam, W, H, b["hits"].out, inv_range, 1.0, {Ch.NORMAL: b["normal"].out}, flags=a)
                ctx.image_to_rgba8(b["color"].out, n, b["rgba8"].out, flags=a)
                ctx.accumulate(capi.ACCUM_SRC_RGBA, b["color"].out, n, accum.out, f, b["acc8"].out, flags=a)
                snap(cs, b["acc"].out, accum.out, n * 16, a)

        got, _, _ = sequence(ctx, cs, [], outs, calls, "a reflected frame, two frames in one queue")
        got = dict(zip([(f, k) for f in range(2) for k in fr[f]] + ["accum"], got))
        hist = acc = None
        for f in range(2):
            g = {k: got[(f, k)] for k in fr[f]}
            mask = shadow_mask(sc, rays, hits, slights)
            w = reflected_frame(rays, hits, sc.oracle, shade, lights, env, inv_range, ps[f], hist, mask.reshape(len(lights), n))
            hist = w["hist"]
            what = f"frame {f}: "
            parity.assert_exact(hits_of(g["hits"]), hits, what + "primary records")
            assert w["hit"].any() and (~w["hit"]).any() and (mask == 0).any()
            np.testing.assert_array_equal(g["rows"], raw(w["rows"]), err_msg=what + "rows")
            np.testing.assert_array_equal(g["mask"], mask, err_msg=what + "shadow mask")
            np.testing.assert_array_equal(g["lit"], raw(w["lit"]), err_msg=what + "lit")
            np.testing.assert_array_equal(g["rrays"], raw(w["rrays"]), err_msg=what + "reflection rays")
            parity.assert_exact(hits_of(g["rhits"]), w["rhits"], what + "reflection records")
            np.testing.assert_array_equal(g["rrows"], raw(w["rrows"]), err_msg=what + "reflection rows")
            np.testing.assert_array_equal(g["rlit"], raw(w["rlit"]), err_msg=what + "reflection lit")
            np.testing.assert_array_equal(g["depth"], raw(w["depth"]), err_msg=what + "depth guide")
            np.testing.assert_array_equal(g["guide"], raw(w["guide"]), err_msg=what + "normal-roughness guide")
            same_floats(g["hist"].view(F).reshape(H, W, 4), w["hist"], what + "history")
            same_floats(g["color"].view(F).reshape(H, W, 4), w["color"], what + "colour")
            assert (raw(w["color"]) != raw(w["lit"])).any()           # reflections were blended in
            color = g["color"].view(F).reshape(-1, 4)                 # (a NaN's payload: the bytes follow the device's own floats)
            np.testing.assert_array_equal(g["rgba8"].reshape(-1, 4), Ch.to_rgba8(color), err_msg=what + "bytes")
            ch = Ch.shade_channels(rays["direction"], Ch.hit_position(rays["origin"], rays["direction"], hits["t"]), hits["normal"], w["hit"],
                                   hits["t"], hits["prim_id"].view(np.uint32), hits["bary_u"], hits["bary_v"], inv_range, F(1.0), shade, None,
                                   (Ch.NORMAL,))
            np.testing.assert_array_equal(g["normal"], raw(ch[Ch.NORMAL]), err_msg=what + "normal channel")
            acc, acc8 = A.accumulate_frame(acc, A.SRC_RGBA, color, f)
            np.testing.assert_array_equal(g["acc"], raw(acc), err_msg=what + "accumulator")
            np.testing.assert_array_equal(g["acc8"].reshape(-1, 4), acc8, err_msg=what + "accumulated bytes")
        np.testing.assert_array_equal(got["accum"], raw(acc))
    finally:
        rig.close()


def test_a_path_traced_loop_in_one_queue(built):
    """The loop of test_path_gpu.py (soup, 96 x 72, four lights, max_bounces 4) behind one gate: init, primary grid, then per bounce
    resolve -> shadows -> light without environment -> step -> bounce cast, every call ASYNC, no read-back between bounces (a bounce with
    nothing active steps nothing), then the finished frame; against path.trace_frame fed the records of each bounce, as there."""
    from messyerraytracer_amd import path as P
    from test_lighting_gpu import environment, light_list
    from test_path_gpu import FRAME, LOOP_BOUNCES, LOOP_GRID, LOOP_KIND, LOOP_LIGHTS
    from test_surface_gpu import shade_data, upload
    rig = Rig(LOOP_KIND)
    try:
        ctx, dev, cs = rig.ctx, rig.dev, rig.cs
        upload(ctx, shade_data(LOOP_KIND))
        lights, env = light_list(LOOP_KIND)[:LOOP_LIGHTS], environment()
        slights = capi.shadow_lights(lights)
        (w, h), nb = LOOP_GRID, LOOP_BOUNCES + 1
        n, cam = w * h, camera(LOOP_KIND, w, h)
        rays0, hits0 = grid(LOOP_KIND, w, h)
        sizes = dict(hits=32, rays=32, rows=64, pairs=8, shits=32, mask=LOOP_LIGHTS, direct=16, select=1, lobe=1, cast_lobe=1, state=32)
        bs = [{k: Out(dev, n * s) for k, s in sizes.items()} for _ in range(nb)]
        state, counts, rgba = Out(dev, n * 32), Out(dev, 4 * nb, np.zeros(nb, np.uint32)), Out(dev, n * 16)
        outs = [b for d in bs for b in d.values()] + [state, counts, rgba]

        def calls(a):
            ctx.path_init(state.out, n, flags=a)
            ctx.cast_grid(cam, w, h, hits=bs[0]["hits"].out, flags=capi.FLAG_HITS_ON_DEVICE | a)
            for b, d in enumerate(bs):
                kw = dict(frame=FRAME, bounce=b, max_bounces=LOOP_BOUNCES, d_out_lobe=d["lobe"].out, d_active_count=counts.out + 4 * b, flags=a)
                if b == 0:
                    ctx.resolve_grid_surfaces(cam, w, h, d["hits"].out, d["rows"].out, d["pairs"].out, d["shits"].out, flags=a)
                    ctx.cast_grid_shadows(cam, w, h, d["hits"].out, slights, d["mask"].out, flags=a)
                    ctx.light_grid_surfaces(cam, w, h, d["hits"].out, d["rows"].out, lights, d["direct"].out, d["mask"].out, None, flags=a)
                    ctx.path_grid_step(cam, w, h, d["shits"].out, d["rows"].out, d["direct"].out, state.out, env, d["select"].out, **kw)
                else:
                    ctx.resolve_surfaces(d["rays"].out, d["hits"].out, n, d["rows"].out, d["pairs"].out, d["shits"].out, flags=a)
                    ctx.cast_shadows(d["rays"].out, d["hits"].out, n, slights, d["mask"].out, flags=a)
                    ctx.light_surfaces(d["rays"].out, d["hits"].out, d["rows"].out, n, lights, d["direct"].out, d["mask"].out, None, flags=a)
                    ctx.path_step(d["rays"].out, d["shits"].out, d["rows"].out, n, d["direct"].out, state.out, env, d["select"].out, **kw)
                snap(cs, d["state"].out, state.out, n * 32, a)
                if b < LOOP_BOUNCES:
                    bk = dict(frame=FRAME, first_draw=P.first_draw(b), t_max=FAR, d_select=d["select"].out, d_surface=d["pairs"].out,
                              d_out_lobe=d["cast_lobe"].out, d_out_rays=bs[b + 1]["rays"].out, flags=a)
                    if b == 0:
                        ctx.cast_grid_bounce(cam, w, h, d["shits"].out, bs[b + 1]["hits"].out, **bk)
                    else:
                        ctx.cast_bounce(d["rays"].out, d["shits"].out, n, bs[b + 1]["hits"].out, **bk)
            ctx.path_finish(state.out, n, rgba.out, 0, flags=a)

        # (never written: the rays of bounce 0, made in the kernels, and what follows the last bounce)
        got, _, _ = sequence(ctx, cs, [], outs, calls, "a path-traced loop in one queue")
        got = dict(zip([(b, k) for b in range(nb) for k in bs[b]] + ["state", "counts", "rgba"], got))
        parity.assert_exact(hits_of(got[(0, "hits")]), hits0, "primary records")
        records = []
        for b in range(nb):
            shits = hits_of(got[(b, "shits")])
            direction = rays0["direction"] if b == 0 else got[(b, "rays")].view(T.RAY32)["direction"]
            records.append(dict(rows=got[(b, "rows")].view(T.SURFACE64), hit=shits["prim_id"] != -1, normal=shits["normal"], direction=direction,
                                direct=got[(b, "direct")].view(F).reshape(-1, 4)))
        want = P.trace_frame(iter(records), env, np.arange(n, dtype=np.uint64), FRAME, LOOP_BOUNCES)
        counted = got["counts"].view(np.uint32)
        assert len(want) >= 3
        for b, (st, select, lobe, active) in enumerate(want):
            np.testing.assert_array_equal(got[(b, "state")], raw(st), err_msg=f"state after bounce {b}")
            np.testing.assert_array_equal(got[(b, "select")], select, err_msg=f"select of bounce {b}")
            np.testing.assert_array_equal(got[(b, "lobe")], lobe, err_msg=f"lobe of bounce {b}")
            assert counted[b] == active == int(select.sum()), b
            if b < LOOP_BOUNCES:
                np.testing.assert_array_equal(got[(b, "cast_lobe")], lobe, err_msg=f"the bounce cast's lobe {b}")
        for b in range(len(want), nb):                             # nothing was active any more: nothing is stepped
            np.testing.assert_array_equal(got[(b, "state")], raw(want[-1][0]))
            assert counted[b] == 0 and not got[(b, "select")].any()
        np.testing.assert_array_equal(got["state"], raw(want[-1][0]))
        np.testing.assert_array_equal(got["rgba"], raw(P.path_finish(want[-1][0], 0)))
        assert (want[-1][0]["active"] == 0).all() and (P.path_finish(want[-1][0], 0)[:, :3] > 0).any()
    finally:
        rig.close()


# ---- 4. scene changes and uploads are ordered on the stream ----------------------------------------------------------------------------

def change_sequence(rig, ins, late, use, change, nbytes, what):
    """gate; the caller's copies of `ins`; use(A, ASYNC); the caller's copies of `late` (what the change reads on the device); change(),
    which blocks and so returns after the gate; use(B, ASYNC).  A is what the state before the change gives, B what the state after it
    gives.  The warm-up runs the same on the own stream and then undoes the change (change() on the decoys, which are the old state).
    Returns (A, B) from the caller's stream, equal to the own-stream run's."""
    ctx, cs = rig.ctx, rig.cs
    a_out, b_out = Out(rig.dev, nbytes), Out(rig.dev, nbytes)
    bufs = list(ins) + list(late) + [a_out, b_out]
    ctx.set_stream(0)
    for b in bufs:
        b.reset()
    for i in ins:
        i.fill()
    use(a_out.out, 0)
    for i in late:
        i.fill()
    change(True)
    use(b_out.out, 0)
    own = [a_out.read_out(what), b_out.read_out(what)]
    for i in late:
        i.reset()
    change(False)                                              # the old state again
    ctx.set_stream(cs.s)
    for b in bufs:
        b.reset()
    t0 = time.perf_counter()
    g = cs.gate()
    for i in ins:
        cs.copy(i.live, i.staged, i.n)
    use(a_out.out, ASYNC)
    ms, done_a = (time.perf_counter() - t0) * 1e3, g.done()
    for i in late:
        cs.copy(i.live, i.staged, i.n)
    change(True)
    done_change = g.done()
    use(b_out.out, ASYNC)
    for o in (a_out, b_out):
        cs.copy(o.res, o.out, o.n)
    cs.sync()
    assert g.done() == 1
    g.free()
    note(what, ms, done_a)
    assert done_a == 0, what + ": the ASYNC call in front of the change waited for the stream"
    assert done_change == 1, what + ": the change returned while the work queued before it was still held back"
    got = [a_out.read(what), b_out.read(what)]
    for i in list(ins) + list(late):
        i.check(what)
    for k in range(2):
        np.testing.assert_array_equal(got[k], own[k], err_msg=f"{what}: {'AB'[k]} differs from the own-stream run")
    return got


def moved_soup():
    if "moved soup" not in WANT:
        sc = scene("soup")
        v1 = synth.deform(sc.verts, 0.3, 1.3, 3)
        rays = grid("soup", 64, 64)[0]
        WANT["moved soup"] = (v1, capi.make_triangles(v1, layers=sc.layers), po.OracleScene(v1, layers=sc.layers).trace(rays))
    return WANT["moved soup"]


def test_flat_refit_is_ordered_on_the_stream(soup):
    """mrt_refit_scene, MRT_BUILD_TRIS_ON_DEVICE: the cast queued before it sees the old triangles although the caller's copy of the
    new ones into the live buffer is queued in between; the cast after it sees the new ones."""
    sc, ctx = scene("soup"), soup.ctx
    _, tris1, want1 = moved_soup()
    want0 = grid("soup", 64, 64)[1]
    assert (want0["prim_id"] != want1["prim_id"]).any()
    cam, n = camera("soup", 64, 64), 64 * 64
    tris = In(soup.dev, tris1, capi.make_triangles(sc.verts, layers=sc.layers))
    a, b = change_sequence(soup, [], [tris], lambda out, fl: ctx.cast_grid(cam, 64, 64, hits=out, flags=capi.FLAG_HITS_ON_DEVICE | fl),
                           lambda new: ctx.refit_scene(tris.live, tris1.shape[0], on_device=True), n * 32, "flat refit")
    check_records(a, want0, "the cast queued before the refit: the old triangles")
    check_records(b, want1, "the cast after the refit: the new triangles")


@pytest.mark.parametrize("how", ["instances", "refit"])
def test_two_level_changes_are_ordered_on_the_stream(built, how):
    """mrt_update_instances_device with the instances on the device, and mrt_refit_two_level_scene with the mesh vertices on the device."""
    sc = scene("room_tl")
    rig = Rig("room_tl")
    try:
        ctx = rig.ctx
        rays, want0 = grid("room_tl", 64, 64)
        cam, n = camera("room_tl", 64, 64), 64 * 64
        if how == "instances":
            inst1 = sc.inst.copy()
            inst1["origin"][6:] += F([0.4, 0.25, -0.3])              # the sphere and the boxes move
            live = In(rig.dev, inst1, sc.inst)
            want1 = po.OracleTwoLevelScene(sc.local, inst1).trace(rays)

            def change(new):
                ctx.update_instances_device(live.live, on_device=True, n_instances=inst1.shape[0])
        else:
            v1 = synth.deform(sc.local, 0.15, 0.9, 4)
            live = In(rig.dev, v1, sc.local)
            want1 = po.OracleTwoLevelScene(v1, sc.inst).trace(rays)

            def change(new):
                ctx.refit_two_level_scene(live.live, sc.inst, n_mesh_tris=v1.shape[0], on_device=True)
        assert (raw(want0) != raw(want1)).any()
        a, b = change_sequence(rig, [], [live], lambda out, fl: ctx.cast_grid(cam, 64, 64, hits=out, flags=capi.FLAG_HITS_ON_DEVICE | fl),
                               change, n * 32, "two-level " + how)
        parity.assert_exact(hits_of(a), want0, how + ": the cast queued before the change")
        parity.assert_exact(hits_of(b), want1, how + ": the cast after the change")
    finally:
        rig.close()


@pytest.mark.parametrize("n_tris", [2000, 1])
def test_device_build_reads_triangles_in_stream_order(built, n_tris):
    """mrt_build_scene_device, MRT_BUILD_TRIS_ON_DEVICE (the radix tree; one triangle: the host wraps it): the triangles are written by
    a copy behind the gate; the call blocks, and the scene is theirs, not the decoy's."""
    sc = scene("soup")
    if n_tris == 1:
        new = F([[[-8, -8, 0], [8, -8, 0], [0, 8, 0]]])               # across the view
        old = new + F([0, 0, -40])                                     # behind the camera
        want = po.OracleScene(new).trace(grid("soup", 64, 64)[0])
        tris_new, tris_old = capi.make_triangles(new), capi.make_triangles(old)
    else:
        _, tris_new, want = moved_soup()
        tris_old = capi.make_triangles(sc.verts, layers=sc.layers)
    ctx, dev, cs = capi.Context(0), None, Caller()
    try:
        dev = Dev(ctx)
        cam, n = camera("soup", 64, 64), 64 * 64
        tris, out = In(dev, tris_new, tris_old), Out(dev, n * 32)

        def calls(a):
            ctx.build_scene_device(tris.live, n_tris, on_device=True)
            ctx.cast_grid(cam, 64, 64, hits=out.out, flags=capi.FLAG_HITS_ON_DEVICE | a)

        own = warm(ctx, [tris], [out], calls, "device build")
        tris.reset()
        ctx.build_scene_device(tris.live, n_tris, on_device=True)     # the decoy's scene again
        (got,) = gated(ctx, cs, [tris], [out], calls, f"device build of {n_tris} triangles", waits=True)
        np.testing.assert_array_equal(got, own[0])
        check_records(got, want, f"device build of {n_tris} triangles")
    finally:
        ctx.set_stream(0)
        if dev:
            dev.free()
        ctx.close()
        cs.destroy()


@pytest.mark.parametrize("what", ["shade data", "textures", "panorama"])
def test_uploads_wait_for_the_stream(soup, what):
    """mrt_upload_shade_data / mrt_upload_textures / mrt_upload_panorama while an ASYNC call that reads the old data is still queued
    behind the gate: the upload waits for the stream, the queued call gives the old result and the next one the new."""
    from messyerraytracer_amd import lighting as Lg, texture as X
    from test_hemisphere_gpu import hit_point
    from test_lighting_gpu import environment, light_list
    from test_panorama_gpu import ENERGY, image
    from test_surface_gpu import expected, shade_data, upload, without
    from test_texture_gpu import images, texture_set, textured_shade, upload_shade, upload_textures
    ctx = soup.ctx
    rays, hits = grid("soup", 64, 64)
    cam, n = camera("soup", 64, 64), 64 * 64
    recs = In(soup.dev, hits, miss_records(n))
    ins = [recs]
    hit, dirs = hits["prim_id"] != -1, rays["direction"]

    def resolve(out, fl):
        ctx.resolve_grid_surfaces(cam, 64, 64, recs.live, out, flags=fl)

    def textured(shade, tex):
        return X.resolve_textured(dirs, hits["normal"], hit, hits["prim_id"].view(np.uint32), hits["bary_u"], hits["bary_v"], shade, tex)[0]

    if what == "shade data":
        old = shade_data("soup")
        new = without(old, "normals")
        new.materials = old.materials[::-1].copy()
        use, size = resolve, 64
        want = [expected(rays, hits, s)[0] for s in (old, new)]

        def change(is_new):
            upload(ctx, new if is_new else old)
    elif what == "textures":
        shade, old = textured_shade("soup"), texture_set("soup")
        new = X.TextureSet(images()[4:5], X.bindings([0] * 5, [None] * 5, [1.0] * 5), None)      # one 2 x 2 texture, every albedo
        upload_shade(ctx, shade)
        use, size = resolve, 64
        want = [textured(shade, t) for t in (old, new)]

        def change(is_new):
            upload_textures(ctx, new if is_new else old)
    else:
        shade = shade_data("soup")
        upload(ctx, shade)
        rows_host = expected(rays, hits, shade)[0]
        rows = In(soup.dev, rows_host, np.zeros(n, T.SURFACE64))
        ins.append(rows)
        lights, env = light_list("soup")[:4], environment()
        panos = [(image("3x2"), ENERGY), (image("1x1"), ENERGY)]
        use, size = (lambda out, fl: ctx.light_grid_surfaces(cam, 64, 64, recs.live, rows.live, lights, out, None, env, flags=fl)), 16
        want = [Lg.shade_linear(rows_host, hit, hit_point(rays, hits), dirs, lights, None, env, panorama=p)[0] for p in panos]

        def change(is_new):
            ctx.upload_panorama(*panos[1 if is_new else 0])
    change(False)
    assert (raw(want[0]) != raw(want[1])).any()
    a, b = change_sequence(soup, ins, [], use, change, n * size, "upload of " + what)
    np.testing.assert_array_equal(a, raw(want[0]), err_msg=what + ": the call queued before the upload reads the old data")
    np.testing.assert_array_equal(b, raw(want[1]), err_msg=what + ": the call after the upload reads the new data")


# ---- 5. switching streams ----------------------------------------------------------------------------------------------------------------

class CastSet:
    """Casts of one context queued as one sequence, each with the check of its output: what the hops of test_switching_streams repeat"""

    def __init__(self, rig):
        self.rig, self.ins, self.outs, self.steps, self.checks = rig, [], [], [], []

    def rays(self, rays):
        self.ins.append(In(self.rig.dev, rays, decoy_rays(rays.shape[0])))
        return self.ins[-1]

    def out(self, nbytes, check, init=None):
        self.outs.append(Out(self.rig.dev, nbytes, init))
        self.checks.append(check)
        return self.outs[-1]

    def records(self, want, what):
        return self.out(want.shape[0] * 32, lambda got, name: check_records(got, want, f"{name}: {what}"))

    def cast(self, d_rays, want, what, flags=0):
        ctx, o, n = self.rig.ctx, self.records(want, what), want.shape[0]
        self.steps.append(lambda a: ctx.cast(d_rays.live, o.out, count=n, flags=DEV | flags | a))

    def grid(self, kind, w, h, want, what):
        ctx, o, cam = self.rig.ctx, self.records(want, what), camera(kind, w, h)
        self.steps.append(lambda a: ctx.cast_grid(cam, w, h, hits=o.out, flags=capi.FLAG_HITS_ON_DEVICE | a))

    def any_hit(self, d_rays, want, what):
        def check(got, name):
            assert (got <= 1).all(), f"{name}: {what}: bytes never written"
            np.testing.assert_array_equal(got.astype(bool), want["prim_id"] >= 0, err_msg=f"{name}: {what}")
        ctx, n = self.rig.ctx, want.shape[0]
        o = self.out(n, check)
        self.steps.append(lambda a: ctx.cast(d_rays.live, o.out, count=n, mode=capi.MODE_ANY_HIT, flags=DEV | capi.FLAG_BOOL_OUT | a))

    def tokens(self, d_rays, want, what):
        ctx, n, tb = self.rig.ctx, want.shape[0], self.rig.ctx.token_bytes()

        def check(got, name):
            first = got.view(np.uint32).reshape(n, tb // 4)[:, 0]
            np.testing.assert_array_equal(first != capi.TOKEN_MISS, want["prim_id"] >= 0, err_msg=f"{name}: {what}: tokens")
        tok = self.out(n * tb, check, np.full(n * tb, 0xFF, np.uint8))
        exp = self.out(n * 32, lambda got, name: parity.assert_exact(hits_of(got), want, f"{name}: {what}: expanded"))
        self.steps.append(lambda a: ctx.cast(d_rays.live, tok.out, count=n, flags=DEV | capi.FLAG_TOKEN_OUT | a))
        self.steps.append(lambda a: ctx.expand_tokens(d_rays.live, tok.out, exp.out, n))

    def calls(self, a):
        for step in self.steps:
            step(a)
        if not a:
            self.rig.ctx.synchronize()                            # (mrt_expand_tokens never waits)

    def warm(self, name):
        self.own = warm(self.rig.ctx, self.ins, self.outs, self.calls, name)

    def hop(self, cs, name):
        """the sequence on the caller's stream cs behind a gate, or (None) ASYNC on the context's own stream and mrt_synchronize"""
        ctx = self.rig.ctx
        if cs is None:
            ctx.set_stream(0)
            for b in self.ins + self.outs:
                b.reset()
            for i in self.ins:
                i.fill()
            self.calls(ASYNC)
            ctx.synchronize()
            got = [o.read_out(name) for o in self.outs]
        else:
            got = gated(ctx, cs, self.ins, self.outs, self.calls, name)
        for k, (g, check) in enumerate(zip(got, self.checks)):
            check(g, name)
            np.testing.assert_array_equal(g, self.own[k], err_msg=f"{name}: output {k} differs from the own-stream run")


def test_switching_streams(built, monkeypatch):
    """S1 -> S2 -> the own stream -> S1, and after every switch every cast of the cases above, held to the oracle: on a flat scene the
    lane kernel, the sorted path, the persistent walk, detect + packet walk, any-hit bytes, tokens and their expansion, a grid, and
    coherent casts of two sizes (the detected-width memo); on a second context the 256 x 128 frames under the tile schedule, whose side
    stream, events and measured orders outlive each switch; on a third the two-level scene.  Then: mrt_set_stream with gated work
    queued returns once that work is complete; MRT_ERR_PENDING leaves the stream as it was; the streams are destroyed after the
    contexts have left them."""
    monkeypatch.setenv("MRT_POISON_OUTPUT", "1")
    monkeypatch.setenv("MRT_SCHEDULE_MIN_LOG2", "15")
    rig, sched_rig, tl_rig = Rig("soup"), Rig("soup", kernel=capi.KERNEL_PACKET_ASM), Rig("room_tl")
    cs2 = Caller()
    try:
        ctx, cs1 = rig.ctx, rig.cs
        rays, want = incoherent("soup", 4096)
        n = 4096
        flat = CastSet(rig)
        d_rays = flat.rays(rays)
        flat.cast(d_rays, want, "lane kernel, 4096 rays")
        d_hits = flat.outs[-1]
        for count in (8193, 65536):
            r, w_ = incoherent("soup", count)
            flat.cast(flat.rays(r), w_, f"{count} incoherent rays")
        for w, h in ((64, 64), (256, 128), (256, 128), (320, 208)):
            r, w_ = grid("soup", w, h)
            flat.cast(flat.rays(r), w_, f"coherent {w}x{h}", capi.FLAG_COHERENT)
        flat.any_hit(d_rays, want, "any-hit bytes")
        flat.tokens(d_rays, want, "tokens")
        flat.grid("soup", 64, 64, grid("soup", 64, 64)[1], "grid 64x64")
        sched = CastSet(sched_rig)
        for k in range(4):
            sched.grid("soup", 256, 128, grid("soup", 256, 128)[1], f"scheduled frame {k}")
        tl = CastSet(tl_rig)
        tl_rays, tl_want = grid("room_tl", 64, 64)
        d_tl = tl.rays(tl_rays)
        tl.out(tl_want.shape[0] * 32, lambda got, name: parity.assert_exact(hits_of(got), tl_want, name + ": two-level cast"))
        tl.steps.append(lambda a: tl_rig.ctx.cast(d_tl.live, tl.outs[0].out, count=tl_want.shape[0], flags=DEV | a))
        tl.tokens(d_tl, tl_want, "two-level tokens")
        sets = (flat, sched, tl)
        for s, name in zip(sets, ("flat", "scheduled", "two-level")):
            s.warm("switching streams, " + name)
        c0 = sched_rig.ctx.schedule_counts()
        assert c0["scheduled"] == 4 and c0["sorts"] >= 1, c0
        own = flat.own
        for hop, cs in enumerate((cs1, cs2, None, cs1)):
            where = f"hop {hop} to " + ("the own stream" if cs is None else "S1" if cs is cs1 else "S2")
            for s, name in zip(sets, ("flat", "scheduled", "two-level")):
                s.hop(cs, f"{where}, {name}")
        c1 = sched_rig.ctx.schedule_counts()
        print(f"[caller-stream] schedule counts across the hops: {c0} -> {c1}")
        assert c1["scheduled"] == c0["scheduled"] + 16 and c1["ordered"] > c0["ordered"], (c0, c1)   # orders measured on one stream, launched on the next
        for r in (sched_rig, tl_rig):
            r.ctx.set_stream(0)
        # the context is on S1: a switch with gated work queued returns when that work is complete
        for b in (d_rays, d_hits):
            b.reset()
        g = cs1.gate()
        cs1.copy(d_rays.live, d_rays.staged, d_rays.n)
        ctx.cast(d_rays.live, d_hits.out, count=n, flags=DEV | ASYNC)
        assert g.done() == 0
        ctx.set_stream(cs2.s)
        assert g.done() == 1, "mrt_set_stream returned while work was queued on the old stream"
        check_records(d_hits.read_out(), want, "the output straight after mrt_set_stream")         # (read on S2, no wait for S1)
        cs1.sync()
        g.free()
        # a pending dispatch: refused, and the stream is still S2
        ctx.submit(rays)
        with pytest.raises(capi.MrtError) as e:
            ctx.set_stream(cs1.s)
        assert e.value.status == capi.ERR_PENDING
        parity.assert_exact(ctx.collect(), want, "the collected dispatch")
        flat.hop(cs2, "still on S2 after the refused switch")
        # back to the own stream, the caller's streams destroyed, another cast, a clean close
        ctx.set_stream(0)
        cs1.destroy()
        cs2.destroy()
        parity.assert_exact(ctx.cast(rays), want, "a cast after the caller's streams are gone")
        d_rays.fill()
        ctx.cast(d_rays.live, d_hits.out, count=n, flags=DEV)
        np.testing.assert_array_equal(d_hits.read_out(), own[0])
        for s, name in ((sched, "scheduled"), (tl, "two-level")):  # the other contexts, on their own streams since the hops
            s.hop(None, "after the caller's streams are gone, " + name)
    finally:
        for r in (rig, sched_rig, tl_rig):
            r.close()
        cs2.destroy()


# ---- 6. two contexts on one stream ------------------------------------------------------------------------------------------------------

def test_two_contexts_on_one_stream(soup):
    """Context A casts a grid into device records, context B (the same scene, the same stream) casts shadows and resolves surfaces over
    them, every call ASYNC; one wait for the stream."""
    from test_hemisphere_gpu import shadow_mask
    from test_lighting_gpu import light_list
    from test_surface_gpu import expected, shade_data, upload
    a_ctx, cs, dev = soup.ctx, soup.cs, soup.dev
    b_ctx = capi.Context(0)
    try:
        sc = scene("soup")
        sc.upload(b_ctx)
        shade = shade_data("soup")
        upload(b_ctx, shade)
        slights = capi.shadow_lights(light_list("soup")[:3])
        rays, hits = grid("soup", 64, 64)
        cam, n = camera("soup", 64, 64), 64 * 64
        recs, mask, rows = Out(dev, n * 32), Out(dev, n * 3), Out(dev, n * 64)

        def calls(a):
            a_ctx.cast_grid(cam, 64, 64, hits=recs.out, flags=capi.FLAG_HITS_ON_DEVICE | a)
            b_ctx.cast_grid_shadows(cam, 64, 64, recs.out, slights, mask.out, flags=a)
            b_ctx.resolve_grid_surfaces(cam, 64, 64, recs.out, rows.out, flags=a)

        b_ctx.set_stream(0)
        own = warm(a_ctx, [], [recs, mask, rows], calls, "two contexts")
        b_ctx.set_stream(cs.s)
        got = gated(a_ctx, cs, [], [recs, mask, rows], calls, "two contexts on one stream")
        for k in range(3):
            np.testing.assert_array_equal(got[k], own[k])
        check_records(got[0], hits, "context A's records")
        np.testing.assert_array_equal(got[1], shadow_mask(sc, rays, hits, slights), err_msg="context B's shadow mask")
        np.testing.assert_array_equal(got[2], raw(expected(rays, hits, shade)[0]), err_msg="context B's rows")
    finally:
        b_ctx.set_stream(0)
        b_ctx.close()


# ---- 7. blocking casts on a caller's stream ---------------------------------------------------------------------------------------------

def test_blocking_host_casts_on_a_callers_stream(soup):
    """2^20 + 4097 host rays (two chunks of the upload / trace / download pipeline, its copy streams beside S): the bytes of the same cast
    on the own stream.  A blocking cast on S is timed; an ASYNC cast leaves no kernel named, as the header says."""
    ctx, cs = soup.ctx, soup.cs
    n = (1 << 20) + 4097
    rays = synth.incoherent_rays(n, 23)
    ctx.set_stream(0)
    own = ctx.cast(rays)
    ctx.set_stream(cs.s)
    got = ctx.cast(rays)
    np.testing.assert_array_equal(raw(got), raw(own))
    for part in (slice(0, 4096), slice(n - 4097, n)):
        parity.assert_exact(got[part], scene("soup").oracle(rays[part]), "pipelined cast on S")
    st = ctx.stats()
    assert np.isfinite(st["last_trace_ms"]) and st["last_trace_ms"] > 0 and st["last_kernel"] != 0 and ctx.last_kernel_variant() != ""
    small, want = incoherent("soup", 4096)
    d_rays, d_hits = In(soup.dev, small, decoy_rays(4096)), Out(soup.dev, 4096 * 32)
    ctx.cast(d_rays.staged, d_hits.out, count=4096, flags=DEV)                                     # blocking, device arrays, on S
    st = ctx.stats()
    assert np.isfinite(st["last_trace_ms"]) and st["last_trace_ms"] > 0 and ctx.last_kernel_variant().startswith("trace_lane_kernel<false")
    check_records(d_hits.read_out(), want, "a blocking device cast on S")
    def cast(a):
        ctx.cast(d_rays.live, d_hits.out, count=4096, flags=DEV | a)
        if not a:                                                  # the warm-up's blocking cast: timed
            assert ctx.stats()["last_trace_ms"] > 0 and ctx.stats()["last_kernel"] != 0

    ((got,), _, _) = sequence(ctx, cs, [d_rays], [d_hits], cast, "an ASYNC cast after blocking ones")
    check_records(got, want, "an ASYNC cast after blocking ones")
    st = ctx.stats()                                               # no timing and no kernel named after an ASYNC cast: not the blocking one's
    assert st["last_trace_ms"] == 0 and st["last_sort_ms"] == 0 and st["last_h2d_ms"] == 0 and st["last_d2h_ms"] == 0, st
    assert st["last_kernel"] == 0 and ctx.last_kernel_variant() == ""
