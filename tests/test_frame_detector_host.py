"""CPU suite of the single-frame mode: the two C-ABI names of the multi-workgroup top-k (header, binding table, library), its
workspace rule, the FrameDetector refusal on a CPU module, and tools/latency_frame.py: the per-launch fill table from a kernel
trace (no GPU needed) and the refusal of the timing paths without a device."""
import csv
import os
import re
import subprocess
import sys

import pytest
import torch

from m3dssd_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "latency_frame.py")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(_hip.HEADER).read(), flags=re.S)


def test_header_signature_table_and_library_agree_on_the_new_names():
    L, hdr = _hip.lib(), _header()
    for name, nargs in (("m3d_topk_decode_mw_workspace_bytes", 3), ("m3d_topk_decode_planar_mw", 18)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == nargs
        assert hasattr(L, name) and name in _hip.SIGNATURES
        assert len(_hip.SIGNATURES[name][1]) == nargs
    # the arguments of m3d_topk_decode_planar, then wgs_per_image in front of the stream
    assert _hip.SIGNATURES["m3d_topk_decode_planar_mw"][1] == (_hip.SIGNATURES["m3d_topk_decode_planar"][1][:-1] + [_hip.c_int, _hip.P])
    assert L.m3d_abi_version() == 5
    assert "m3d_topk_decode_planar_mw" in open(_hip.HEADER).read().split("#define M3D_ABI_VERSION")[0]     # listed as additive


def test_mw_workspace_rule_answers_without_a_gpu():
    f = _hip.lib().m3d_topk_decode_mw_workspace_bytes
    assert f(0, 100, 10) == -1 and f(1, 0, 10) == -1 and f(1, 100, 0) == -1
    by_b = [f(b, 276480, 3000) for b in (1, 2, 3, 4, 8)]
    by_r = [f(1, r, 1) for r in (1, 5, 10007, 46080, 276480)]
    for sizes in (by_b, by_r):
        assert all(s > 0 for s in sizes) and all(b > a for a, b in zip(sizes, sizes[1:]))
    # holds the single-workgroup kernel's candidate buffers, the selected keys, one histogram and the counters per image
    assert f(1, 276480, 3000) >= _hip.lib().m3d_topk_decode_workspace_bytes(1, 276480) + 3000 * 8 + 2048 * 4 + 8
    assert f(2, 46080, 16384) > f(2, 46080, 3000)


def test_frame_detector_refuses_a_cpu_module():
    from m3dssd_amd import synth
    from m3dssd_amd.pipeline import FrameDetector, PipelinedDetector  # noqa: F401
    from model.M3d_inference_align import build
    conf = synth.synth_conf((128, 320), 0, batch_size=1, device="cpu")
    net = build(conf, "test")
    with pytest.raises(NotImplementedError, match="ROCm device"):
        FrameDetector(net, conf, 128, 320)
    with pytest.raises(NotImplementedError):
        FrameDetector(torch.nn.DataParallel(net), conf, 128, 320, batch=2, refine=True)
    with pytest.raises(TypeError):
        FrameDetector(torch.nn.Linear(2, 2), conf, 128, 320)


COLS = ["Kind", "Agent_Id", "Queue_Id", "Stream_Id", "Thread_Id", "Dispatch_Id", "Kernel_Id", "Kernel_Name", "Correlation_Id",
        "Start_Timestamp", "End_Timestamp", "LDS_Block_Size", "Scratch_Size", "VGPR_Count", "Accum_VGPR_Count", "SGPR_Count",
        "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"]


def _write_trace(path, launches):
    """launches: (name, start_ns, end_ns, workgroup xyz, grid xyz in work-items)."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_ALL)
        w.writerow(COLS)
        for i, (name, t0, t1, wg, grid) in enumerate(launches):
            w.writerow(["KERNEL_DISPATCH", 1, 1, 0, 77, i + 1, 5, name, i + 1, t0, t1, 0, 0, 32, 0, 16, *wg, *grid])


def test_merge_trace_fill_table(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import latency_frame as lf
    finally:
        sys.path.pop(0)
    p = str(tmp_path / "t_kernel_trace.csv")
    launches = [
        # an earlier replay: must not be listed
        ("stem(float*)", 100, 200, (256, 1, 1), (256 * 300, 1, 1)),
        ("select_post_kernel(float const*, int)", 300, 400, (256, 1, 1), (256, 1, 1)),
        # the last replay, written out of order (the tool sorts by start)
        ("void topk_decode_kernel<true>(TopkArgs)", 11000, 41000, (1024, 1, 1), (1024, 1, 1)),
        ("conv_kernel(float*)", 1000, 6000, (256, 1, 1), (256 * 512, 1, 1)),                 # 512 workgroups: 2 per CU
        ("topk_mw_hist_kernel(TopkArgs)", 7500, 9500, (1024, 1, 1), (1024 * 64, 3, 1)),      # grid (64, 3): 192 workgroups
        ("side_branch_kernel(int)", 5000, 7000, (64, 2, 1), (64 * 16, 2 * 16, 1)),           # 16 x 16 = 256: exactly the CUs
        ("ragged_kernel(int)", 9500, 10000, (256, 1, 1), (1000, 1, 1)),                      # ceil(1000 / 256) = 4
        ("select_post_kernel(float const*, int)", 41500, 42000, (256, 1, 1), (256, 1, 1)),
    ]
    _write_trace(p, launches)
    table = lf.fill_table(lf.last_replay(lf.read_trace(p)))
    assert [t["kernel"] for t in table] == ["conv_kernel", "side_branch_kernel", "topk_mw_hist_kernel", "ragged_kernel",
                                            "topk_decode_kernel<true>", "select_post_kernel"]
    assert [t["workgroups"] for t in table] == [512, 256, 192, 4, 1, 1]
    assert [t["wg_per_cu"] for t in table] == [2.0, 1.0, 0.75, 0.016, 0.004, 0.004]
    assert [t["under_filled"] for t in table] == [False, False, True, True, True, True]
    assert [t["dur_us"] for t in table] == [5.0, 2.0, 2.0, 0.5, 30.0, 0.5]
    # gap to the end of everything launched before: the side branch overlaps the conv (-1 us), the histogram starts 0.5 us after
    # the side branch ended (not 1.5 us after the conv), back-to-back launches have a gap of 0
    assert [t["gap_us"] for t in table] == [None, -1.0, 0.5, 0.0, 1.0, 0.5]
    # the command line prints the same table and marks the under-filled launches; it needs no GPU
    save = str(tmp_path / "replay.csv")
    r = subprocess.run([sys.executable, TOOL, "--merge-trace", p, "--save-replay-csv", save], capture_output=True, text=True,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 + 6 + 1
    marks = [ln.rstrip().endswith("<CU") for ln in lines[1:7]]
    assert marks == [False, False, True, True, True, True]
    assert '"under_filled": 4' in lines[-1] and '"launches": 6' in lines[-1]
    saved = list(csv.DictReader(open(save)))
    assert list(saved[0].keys()) == COLS and len(saved) == 6 and saved[0]["Kernel_Name"].startswith("conv_kernel")
    # a trace without the columns is refused, not guessed at
    bad = str(tmp_path / "bad.csv")
    with open(bad, "w") as f:
        f.write('"Kernel_Name","Start_Timestamp","End_Timestamp"\n"select_post_kernel",1,2\n')
    r = subprocess.run([sys.executable, TOOL, "--merge-trace", bad], capture_output=True, text=True)
    assert r.returncode != 0 and "Grid_Size" in r.stderr


def test_timing_paths_refuse_to_run_without_a_gpu():
    if torch.cuda.is_available():
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    else:
        env = dict(os.environ)
    for extra in ([], ["--trace-run"]):
        r = subprocess.run([sys.executable, TOOL, "--reps", "1", "--warmup", "0", "--out", os.devnull] + extra,
                           capture_output=True, text=True, env=env)
        assert r.returncode != 0
        assert "no ROCm device" in r.stderr and "never fall back" in r.stderr
        assert not r.stdout.strip()
