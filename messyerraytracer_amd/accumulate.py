"""Progressive frames as include/mrt_hip.h states them (mrt_halton_jitter, mrt_accum_begin_frame, mrt_accum_end_frame, mrt_accumulate)
restated in numpy on channels.py and path.py: RayRenderer's Halton(2,3) jitter, its camera-motion reset, the bookkeeping of its running
mean and the mean itself -- float32, one operation at a time, in the order the header states.  Test and tool plumbing
(tests/test_accumulate_*.py, tools/bench_accumulate.py): the device's accumulator and bytes must equal these byte for byte."""
import numpy as np

from . import channels as Ch
from . import path as P

F = np.float32
SRC_RGBA, SRC_LIT, SRC_PATH_STATE = 0, 1, 2
INV3 = F(1.0) / F(3.0)
POS_EPS, ROT_EPS = F(1e-4), F(1e-3)
POS_EPS2 = POS_EPS * POS_EPS
ROT_EPS2 = ROT_EPS * ROT_EPS
MAX_INDEX = 0x7FFFFFFE
_QUIET = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


def halton2(idx):
    """the reference's lambda on an int idx"""
    f, r, i = F(1), F(0), int(idx)
    while i > 0:
        f = f * F(0.5)
        r = r + f * F(i & 1)
        i >>= 1
    return r


def halton3(idx):
    f, r, i = F(1), F(0), int(idx)
    while i > 0:
        f = f * INV3
        r = r + f * F(i % 3)
        i //= 3
    return r


def halton_jitter(sample_index):
    """mrt_halton_jitter: (jx, jy)"""
    if not 0 <= int(sample_index) <= MAX_INDEX:
        raise ValueError("sample_index 0 .. 0x7ffffffe")
    return halton2(int(sample_index) + 1), halton3(int(sample_index) + 1)


def length_squared(v):
    with np.errstate(**_QUIET):
        v = np.asarray(v, dtype=F)
        return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def camera_changed(origin, basis, prev_origin, prev_basis):
    """(moved, rotated) of ray_renderer.cpp:452-459; the bases [3, 3] row-major; rotated is not looked for after a move"""
    with np.errstate(**_QUIET):
        o, b = np.asarray(origin, dtype=F).reshape(3), np.asarray(basis, dtype=F).reshape(3, 3)
        po, pb = np.asarray(prev_origin, dtype=F).reshape(3), np.asarray(prev_basis, dtype=F).reshape(3, 3)
        moved = bool(length_squared(o - po) > POS_EPS2)
        rotated = False
        if not moved:
            for c in range(3):
                if rotated:
                    break
                rotated = bool(length_squared(b[:, c] - pb[:, c]) > ROT_EPS2)
        return moved, rotated


def new_state(aa_enabled=True, max_samples=256):
    """mrt_accum_state as a dict: the settings and the persistent words"""
    return dict(aa_enabled=bool(aa_enabled), max_samples=int(max_samples), count=0, pixels=0, prev_origin=np.zeros(3, F),
                prev_basis=np.zeros((3, 3), F), jitter=(F(0.5), F(0.5)), sample_index=0, accumulate=0, n_prior=0)


def _open(st):
    return st["aa_enabled"] and st["count"] < (st["max_samples"] if st["max_samples"] > 1 else 1)


def begin_frame(st, origin, basis):
    """mrt_accum_begin_frame on a new_state() dict, in place"""
    if not st["aa_enabled"] or any(camera_changed(origin, basis, st["prev_origin"], st["prev_basis"])):
        st["count"] = 0
    st["prev_origin"] = np.asarray(origin, dtype=F).reshape(3).copy()
    st["prev_basis"] = np.asarray(basis, dtype=F).reshape(3, 3).copy()
    st["sample_index"] = st["count"]
    st["jitter"] = halton_jitter(st["count"]) if _open(st) else (F(0.5), F(0.5))
    return st


def end_frame(st, pixels):
    """mrt_accum_end_frame on a new_state() dict, in place"""
    st["accumulate"], st["n_prior"] = 0, 0
    if not _open(st):
        return st
    if int(pixels) != st["pixels"]:
        st["pixels"], st["count"] = int(pixels), 0
    st["n_prior"], st["accumulate"] = st["count"], 1
    st["count"] += 1
    return st


def accumulate(acc, s, n_prior):
    """The running mean's step on arrays of any shape: s itself (every bit) for n_prior == 0, else acc + (s - acc) * (1 / (n_prior + 1))
    in three separately rounded float32 operations"""
    s = np.ascontiguousarray(s, dtype=F)
    if int(n_prior) == 0:
        return s.copy()
    with np.errstate(**_QUIET):
        acc = np.asarray(acc, dtype=F)
        inv = F(1.0) / F(int(n_prior) + 1)
        d = (s - acc).astype(F)
        p = (d * inv).astype(F)
        return (acc + p).astype(F)


def sample(source_kind, source, tonemap_mode=0):
    """The four floats mrt_accumulate takes from a pixel of `source`: [N, 4] float32 (SRC_RGBA: as they are; SRC_LIT: finish_color's) or
    [N] T.PATH_STATE (SRC_PATH_STATE: path_finish's)"""
    if source_kind == SRC_RGBA:
        return np.ascontiguousarray(source, dtype=F)
    if source_kind == SRC_LIT:
        return Ch.finish_color(source, tonemap_mode)
    if source_kind == SRC_PATH_STATE:
        return P.path_finish(source, tonemap_mode)
    raise ValueError("source_kind 0 .. 2")


def accumulate_frame(acc, source_kind, source, n_prior, tonemap_mode=0):
    """mrt_accumulate: (the accumulator [N, 4] float32, its bytes [N, 4] uint8)"""
    out = accumulate(acc, sample(source_kind, source, tonemap_mode), n_prior)
    return out, Ch.to_rgba8(out)
