"""The cast launch policy without a device: which kernel a cast gets and how it is launched (launch_policy.cpp), for a table of
casts on both sides of every threshold -- counts, flags, scene layouts, options, entry points, the previous cast's detected
width --, each with the instantiation its plan resolves to and the launch geometry (resolve_trace / resolve_persistent), a table of
hand-made launches on both sides of every branch of the resolvers, plus the grid kernel tuner over fifteen frames with fake timings, the per-grid state LRU and the detected width across
sequences of blocking, ASYNC, pipelined and submitted casts (csrc/host/launch_policy_test.cpp, which links launch_policy.cpp alone)."""
import subprocess

from messyerraytracer_amd import build as mbuild


def test_launch_policy_table_tuner_and_lru():
    exe = mbuild.build_policy_test()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and " checks hold " in r.stdout, r.stdout
