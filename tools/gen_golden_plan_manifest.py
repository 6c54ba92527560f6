#!/usr/bin/env python
"""Record tests/golden/plan_manifest.json.gz: the launch plans and packed parameters of the cases of tests/plan_manifest.py (fp32 and
bf16, the three shipped configurations, one odd feature-map size, DLA-102, the benchmark's fp32 shape with the fp32 planner's knobs,
a batch of 20) as tests/test_gpu_plan_manifest.py compares them.

Needs the GPU (an engine packs its weights on the device).  Run it on the commit whose plans are the record, i.e. BEFORE a change
that must leave them as they are:

    python tools/gen_golden_plan_manifest.py [OUT_FILE]       (default tests/golden/plan_manifest.json.gz)

The committed record was made with m3dssd_amd/engine.py and engine_bf16.py of commit 92fddee ("Derive the ctypes binding of the C ABI
from the public header"), before Engine._conv was split into one route per kernel family: a checkout of that commit with only
tests/plan_manifest.py, this tool and tests/test_gpu_plan_manifest.py of the later tree copied in.  It added the fields of every
descriptor and the cases at 384x1280 and 160x192; what the earlier record held of its ten cases came out as it was (with
OLD_RECORD=<the earlier file> in the environment the tool compares them before it writes).

One rename is applied to what is recorded.  The two knob cases (plan_manifest.KNOBS) were recorded before the backbone of both plans
was put on one DLA walk.  With TREE_ENTRY = False the bf16 builder of that time named the pooling launch of level3 / level4
``base.base.level{3,4}.tree1.downsample``; the shared walk names it ``base.base.level{3,4}.downsample``, as the fp32 plan and the
reference's module tree do.  The record holds the new name (RENAMED below; a no-op on a commit that has the shared walk).
"""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import plan_manifest  # noqa: E402

RENAMED = {"base.base.level%d.tree1.downsample" % lv: "base.base.level%d.downsample" % lv for lv in (3, 4)}


def main(out):
    manifest = {}
    for case in plan_manifest.CASES:
        manifest[case] = plan_manifest.dump_case(case)
        for op in manifest[case]["ops"]:
            op[0] = RENAMED.get(op[0], op[0])
        print("%-40s %3d ops, tail %s" % (case, len(manifest[case]["ops"]), manifest[case]["tail_start"]))
    old = os.environ.get("OLD_RECORD")
    if old:
        # an earlier record (ops of four slots, no descriptor fields): what it held must come out as it was
        with gzip.open(old, "rt") as f:
            for case, want in json.load(f).items():
                got = json.loads(json.dumps(manifest[case]))
                got["ops"] = [op[:len(want["ops"][0])] for op in got["ops"]]
                assert got == want, case
                print("%-40s equals the earlier record" % case)
    # compact and gzip-compressed (mtime 0: the same plans give the same bytes): as indented text the record is 40 000 lines
    text = json.dumps(manifest, separators=(",", ":"), sort_keys=True)
    with open(out, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
        f.write(text.encode())
    print(out, "%.1f KB" % (os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "plan_manifest.json.gz"))
