# coding: utf-8
"""The pinned results of the single-tile attention backward (needs the GPU; run on the commit whose bytes are to be pinned).

For every case of tests/attn_bwd_cases.CASES -- six (B, nh, Lq, Lk) shapes with key masks, a causal mask, dropout and a
sentence that sees key 0 only, each with dO read and with dO = dY . W_o^T folded in at n = 128, 512 and 640 -- runs
zk_attn_bwd TWICE and records the sha256 of the dq, dk and dv bytes and their first 8 values.

Writes tests/golden/attn_bwd_parent.json (or the path given as the first argument), which
tests/test_gpu_attn_bwd_image.py must reproduce exactly: a change of the kernel that reorders a sum or rounds an
operand differently shows there.  Fails when the two runs disagree (the kernel would not be deterministic).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import attn_bwd_cases as AC  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else AC.GOLDEN
    first = {name: AC.record(name) for name in AC.CASES}
    again = {name: AC.record(name) for name in AC.CASES}
    bad = [n for n in AC.CASES if first[n] != again[n]]
    assert not bad, "two runs disagree: %s" % bad
    with open(path, "w") as f:
        json.dump(first, f, indent=1, sort_keys=True)
        f.write("\n")
    for n in AC.CASES:
        print("%-28s dq %s dk %s dv %s" % (n, *(first[n][x]["sha256"][:12] for x in ("dq", "dk", "dv"))), flush=True)
    print("wrote %s (%d bytes), two runs agree on all %d cases" % (path, os.path.getsize(path), len(AC.CASES)))


if __name__ == "__main__":
    main()
