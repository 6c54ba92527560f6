#!/usr/bin/env python
"""Record tests/golden/plan_manifest.json.gz: the launch plans and packed parameters of the cases of tests/plan_manifest.py (fp32 and
bf16, the three shipped configurations, one odd feature-map size, DLA-102) as tests/test_gpu_plan_manifest.py compares them.

Needs the GPU (an engine packs its weights on the device).  Run it on the commit whose plans are the record, i.e. BEFORE a change
that must leave them as they are:

    python tools/gen_golden_plan_manifest.py [OUT_FILE]       (default tests/golden/plan_manifest.json.gz)
"""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import plan_manifest  # noqa: E402


def main(out):
    manifest = {}
    for case in plan_manifest.CASES:
        manifest[case] = plan_manifest.dump_case(case)
        print("%-40s %3d ops, tail %s" % (case, len(manifest[case]["ops"]), manifest[case]["tail_start"]))
    # compact and gzip-compressed (mtime 0: the same plans give the same bytes): as indented text the record is 40 000 lines
    text = json.dumps(manifest, separators=(",", ":"), sort_keys=True)
    with open(out, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
        f.write(text.encode())
    print(out, "%.1f KB" % (os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "plan_manifest.json.gz"))
