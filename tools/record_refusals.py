#!/usr/bin/env python3
"""Records what a library refuses, and with which words, over the domain of tests/refusal_domain.py into
tests/golden/refusal_table.npz, which tests/test_refusals_host.py replays on the tree under test.  The library recorded is one
built from an EARLIER commit (a checkout of it, built with make -C nerf-workspaces-explorer_amd/csrc), never the tree under test:

    python tools/record_refusals.py --lib <checkout of COMMIT>/nerf-workspaces-explorer_amd/libnwe_hip.so --commit COMMIT

The table holds every distinct (code, text) once and one index per call, in the order of the walk, with a digest of the calls
themselves: a replay over another enumeration fails on the digest, not on a thousand shifted rows.  No GPU is needed."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digest(cases):
    h = hashlib.sha256()
    for case in cases:
        h.update(repr(case).encode())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", required=True, help="the library to record: libnwe_hip.so of a built checkout of --commit")
    ap.add_argument("--commit", required=True, help="the commit that library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "refusal_table.npz"))
    args = ap.parse_args()
    os.environ["NWE_LIB"] = os.path.abspath(args.lib)   # read by nwe_amd._lib when it is imported
    sys.path.insert(0, ROOT)
    from tests import refusal_domain

    cases, rows, refusals = [], [], {}
    for case, code, text in refusal_domain.walk():
        cases.append(case)
        rows.append(refusals.setdefault((code, text), len(refusals)))
    assert len(refusals) < 65536
    header = (f"refusals of commit {args.commit}: code and nwe_last_error text of every call of tests/refusal_domain.py walk() on host-only "
              f"contexts of a library built from that commit, recorded by `python tools/record_refusals.py --lib <checkout of {args.commit}>/"
              f"nerf-workspaces-explorer_amd/libnwe_hip.so --commit {args.commit}`.  rows[i] indexes codes / texts for call i of the walk; text "
              f"'' = not refused; cases = sha256 over repr() of the calls")
    np.savez_compressed(args.out, header=np.array(header), codes=np.array([k[0] for k in refusals], dtype=np.int32),
                        texts=np.array([k[1] for k in refusals]), rows=np.array(rows, dtype=np.uint16), cases=np.array(digest(cases)))
    print(f"{len(rows)} calls, {len(refusals)} distinct refusals, {os.path.getsize(args.out)} bytes -> {args.out}")


if __name__ == "__main__":
    main()
