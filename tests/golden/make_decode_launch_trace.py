# coding: utf-8
"""The pinned launch trace of decoding (needs the GPU; run on the commit whose launches are to be pinned).

For every case of tests/decode_trace.CASES -- the seven models in bf16 and in decode_dtype=float32, the forms selected by
ZERO_HIP_DECODE_FUSE_ATT / ZERO_HIP_DECODE_FUSE_LN / ZERO_HIP_F32_FUSE / use_ffn, a head size of 32 (the launch-per-op
path), a two-member ensemble, rnnsearch with both encoder forms, rnnsearch_deepatt with each of its four cells and deepnmt in
five configurations (tests/deepnmt_ref.CONFIGS (A), (B), (C), (A) with olrn, (B) with lrn) -- records every call of the
library's entry points by encoding_fn, by two eager decoding_fn steps with a cache reorder between them, and the node count of the captured step
graph of a whole beam search; for every scoring case -- the fp32 scorer of four models and of its switches, the bf16
scorer of transformer_fixup -- every call by one score_fn (tests/decode_trace.run_case).

Writes tests/golden/decode_launch_trace.json (or the path given as the first argument), which
tests/test_gpu_decode_launch_trace.py must reproduce exactly: a host-side change of decoding or scoring that adds, drops, reorders
or re-parameterises a launch shows there.  With ``--missing`` the entries the file already has are kept as they are and only
the cases it lacks are recorded: new cases are pinned without touching the old ones.  A few seconds per case.
"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import decode_trace as DT  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if a != "--missing"]
    path = args[0] if args else DT.GOLDEN
    traces = DT.load(path) if "--missing" in sys.argv else {}
    for name in DT.CASES:
        if name in traces:
            continue
        with pytest.MonkeyPatch.context() as patch:
            traces[name] = DT.run_case(name, patch)
        assert tuple(ph for ph in traces[name] if ph != "graph_nodes") == DT.phases(name)
        print("%-40s %s" % (name, DT.summary(traces[name])), flush=True)
    DT.dump(traces, path)
    assert not any(DT.diff(traces[n], DT.load(path)[n]) for n in traces)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
