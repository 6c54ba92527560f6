#!/usr/bin/env python
"""Record tests/golden/bf16_conv_routes.json.gz: what m3d_conv_bf16_variant answers for every descriptor of the grid of
tests/bf16_conv_routes.py (124 416 descriptors, one digit each), as tests/test_bf16_conv_route_host.py compares them.

Needs no GPU: the query reads no memory behind the descriptor's pointers.  Run it with a library built from the commit whose
routes are the record, i.e. BEFORE a change that must leave them as they are, with no M3D_* knob set:

    M3D_HIP_LIB=<that build's libm3dssd_hip.so> python tools/gen_golden_bf16_conv_routes.py [OUT_FILE]

The committed record was made with a library built from commit 6941e28 ("Add a fused BatchNorm + residual + LeakyReLU training
operator (opt-in)"), where the query and the launch of m3d_conv_bf16_forward were still two separately written chains.
"""
import collections
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import bf16_conv_routes as R  # noqa: E402


def main(out):
    knobs = sorted(k for k in os.environ if k.startswith("M3D_BF16_"))
    assert not knobs, "the record is made with every knob at its default (set: %s)" % ", ".join(knobs)
    codes = R.grid_codes()
    for code, count in sorted(collections.Counter(codes).items()):
        print("code %s: %6d" % (code, count))
    text = json.dumps({"grid": [[name, values] for name, values in R.GRID], "codes": codes}, separators=(",", ":"))
    with open(out, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:     # (mtime 0: the same routes give the same bytes)
        f.write(text.encode())
    print(out, "%d descriptors, %d bytes" % (len(codes), os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else R.RECORD)
