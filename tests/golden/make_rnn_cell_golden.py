# coding: utf-8
"""The pinned results of the dense recurrent cell launches (needs the GPU; run on the commit whose bytes are to be pinned).

For every case of tests/rnn_cell_cases.CASES -- the ATR step, the two GRU launches and ff + residual, bf16 and fp32 forms,
through the C ABI entry points on guarded buffers -- runs the launch TWICE and records, per output window (out, out_copy, and
z, rh of the GRU), the sha256 of the window's bytes and its first 8 values.

Writes tests/golden/rnn_cells_parent.json (or the path given as the first argument), which
tests/test_gpu_rnn_cells_image.py must reproduce exactly: a change of a kernel that reorders a sum, fuses another multiply
into an add or rounds an operand differently shows there.  Fails when the two runs disagree.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import rnn_cell_cases as RC  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else RC.GOLDEN
    first = {name: RC.record(name) for name in RC.CASES}
    again = {name: RC.record(name) for name in RC.CASES}
    bad = [n for n in RC.CASES if first[n] != again[n]]
    assert not bad, "two runs disagree: %s" % bad
    with open(path, "w") as f:
        json.dump(first, f, indent=1, sort_keys=True)
        f.write("\n")
    for n in RC.CASES:
        print("%-40s %s" % (n, "  ".join("%s %s" % (k, v["sha256"][:12]) for k, v in sorted(first[n].items()))), flush=True)
    print("wrote %s (%d bytes), two runs agree on all %d cases" % (path, os.path.getsize(path), len(RC.CASES)))


if __name__ == "__main__":
    main()
