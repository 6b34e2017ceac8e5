#!/usr/bin/env python3
"""Records tests/golden/build_digests.json: the digests tests/test_build_digests_gpu.py holds the scene builders to.

    python tests/golden/make_build_digests.py [OUT]     (needs the GPU and a built library)

Every group of the test is run twice, each time in a fresh context; an array whose two digests disagree is left out of
"digests" and named under "unstable".  Run it on the commit whose bytes are to be pinned, in two processes, and compare the two
files before committing one."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_build_digests_gpu as bd  # noqa: E402


def main():
    out = {"digests": {}, "unstable": {}}
    for group, (fn, name, path) in bd.GROUPS.items():
        a, b = fn(name, path), fn(name, path)
        for case in a:
            bad = sorted(k for k in a[case] if a[case][k] != b[case].get(k))
            out["digests"][case] = {k: v for k, v in a[case].items() if k not in bad}
            if bad:
                out["unstable"][case] = bad
        print(group, "ok" if not any(c in out["unstable"] for c in a) else "UNSTABLE", flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else bd.FIXTURE, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
