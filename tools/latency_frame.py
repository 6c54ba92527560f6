#!/usr/bin/env python
"""What a caller with ONE camera frame waits for: call latency of the synchronous detection routes at small batch sizes, the two
top-k kernels alone, and the per-launch fill of one single-frame replay.

Seeded synthetic weights and frames at 384x1280 (m3dssd_amd.synth).  One JSON line per (dtype, batch), appended to
profiles/latency_frame.jsonl together with m3d_source_hashes().  Routes:
  eager           detect_batch: ~80 launches issued from Python per call (the only synchronous route before FrameDetector)
  eager_again     the same route a second time in the same loop: the spread of the measurement against itself
  frame_wg1       FrameDetector(topk_wgs=1): one hipGraph per frame, single-workgroup top-k
  frame           FrameDetector(): the library's choice of top-k
  pipelined_step  ms per PipelinedDetector.step -- the THROUGHPUT figure (the step returns the previous batch): not a latency
Per route p50 / p99 / min of two timings of the same calls: `wall_ms`, the host clock around the call plus a device synchronise
(what a caller waits for), and `event_ms`, the HIP-event time.  `--warmup` untimed rounds, then `--reps` timed ones; the routes are
interleaved round-robin inside the timed loop; every detector is built once, before timing.

Kernel leg (`kernel` lines; --kernel-batches, default 1): m3d_topk_decode_planar against m3d_topk_decode_planar_mw for the
workgroup counts of --wgs-sweep at R = 276 480, k = 3000, on the keys and planar staging of one seeded forward, same interleaving;
`wg1_again` is the single-workgroup kernel as a second arm (the spread).

Per-launch fill (no counters, no other tracing, a run of its own):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/latency_frame.py --trace-run
    python tools/latency_frame.py --merge-trace DIR/.../t_kernel_trace.csv [--save-replay-csv profiles/latency_frame_trace_f32.csv]
--merge-trace needs no GPU: for the last replay in the trace it lists, per launch, kernel name, workgroups, workgroups / 256 CUs,
duration and the gap to the end of everything launched before it (negative: overlapped); launches with fewer workgroups than the
chip has CUs are marked with `<CU`.

Without a ROCm device the measuring paths stop with a message; nothing falls back."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CUS = 256                                   # MI355X
CROP = (384, 1280)
REPLAY_END = "select_post_kernel"           # the last launch of a FrameDetector replay without refinement
OUT = os.path.join(ROOT, "profiles", "latency_frame.jsonl")


# ---------------------------------------------------------------------------------------------------------------- trace (no GPU)
def _dims(row, base):
    """Product over x, y, z of ceil(grid / workgroup) from the trace's columns (rocprofv3 reports the grid in work-items)."""
    if base + "_X" in row:
        return [int(row[base + "_" + a]) for a in "XYZ"]
    if base in row:
        return [int(row[base]), 1, 1]
    raise SystemExit("latency_frame --merge-trace: the trace has no %s / %s_X column (columns: %s)" % (base, base, ", ".join(row)))


def read_trace(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            grid, wg = _dims(r, "Grid_Size"), _dims(r, "Workgroup_Size")
            wgs = 1
            for g, w in zip(grid, wg):
                wgs *= -(-g // max(w, 1))
            rows.append({"name": r["Kernel_Name"], "start": int(r["Start_Timestamp"]), "end": int(r["End_Timestamp"]),
                         "workgroups": wgs, "raw": r})
    rows.sort(key=lambda r: r["start"])
    return rows


def last_replay(rows, end_name=REPLAY_END):
    """The launches of the last replay: everything behind the previous launch of `end_name` up to the last one."""
    ends = [i for i, r in enumerate(rows) if end_name in r["name"]]
    if not ends:
        raise SystemExit("latency_frame --merge-trace: no %s launch in the trace" % end_name)
    lo = ends[-2] + 1 if len(ends) > 1 else 0
    return rows[lo:ends[-1] + 1]


def fill_table(rows, cus=CUS):
    """Per launch: workgroups, share of the CUs, duration, gap to the end of everything launched before it, under-filled mark."""
    out, latest_end = [], None
    for r in rows:
        out.append({"kernel": short_name(r["name"]), "workgroups": r["workgroups"], "wg_per_cu": round(r["workgroups"] / cus, 3),
                    "dur_us": round((r["end"] - r["start"]) / 1e3, 2),
                    "gap_us": None if latest_end is None else round((r["start"] - latest_end) / 1e3, 2),
                    "under_filled": r["workgroups"] < cus})
        latest_end = r["end"] if latest_end is None else max(latest_end, r["end"])
    return out


def short_name(name):
    name = name.split("(", 1)[0]
    return name.replace("void ", "").strip()


def merge_trace(path, save=None, end_name=REPLAY_END):
    rows = last_replay(read_trace(path), end_name)
    table = fill_table(rows)
    print("%-4s %-64s %10s %8s %10s %10s" % ("#", "kernel", "workgroups", "wg/CU", "dur_us", "gap_us"))
    for i, t in enumerate(table):
        print("%-4d %-64s %10d %8.3f %10.2f %10s %s" % (i, t["kernel"][:64], t["workgroups"], t["wg_per_cu"], t["dur_us"],
                                                       "-" if t["gap_us"] is None else "%.2f" % t["gap_us"],
                                                       "<CU" if t["under_filled"] else ""))
    span = (max(r["end"] for r in rows) - rows[0]["start"]) / 1e3
    busy = sum(t["dur_us"] for t in table)
    summary = {"tool": "latency_frame", "kind": "fill", "launches": len(table), "under_filled": sum(t["under_filled"] for t in table),
               "under_filled_dur_us": round(sum(t["dur_us"] for t in table if t["under_filled"]), 1),
               "span_us": round(span, 1), "sum_dur_us": round(busy, 1),
               "sum_positive_gaps_us": round(sum(t["gap_us"] for t in table if t["gap_us"] and t["gap_us"] > 0), 1)}
    print(json.dumps(summary))
    if save:
        cols = list(rows[0]["raw"].keys())
        with open(save, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=cols, quoting=csv.QUOTE_ALL)
            w.writeheader()
            for r in rows:
                w.writerow(r["raw"])
    return table


# ---------------------------------------------------------------------------------------------------------------- timing (GPU)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("latency_frame: no ROCm device -- the timing paths need the MI355X and never fall back "
                         "(only --merge-trace runs without one)")
    return torch.device("cuda:0")


def _stats(v):
    v = sorted(v)
    n = len(v)
    return {"p50": round(v[n // 2], 4), "p99": round(v[min(n - 1, int(0.99 * n))], 4), "min": round(v[0], 4)}


def interleaved(arms, warmup, reps):
    """arms: {name: callable}.  Round-robin: every round calls each arm once; per call the host wall clock to a synchronised
    result and the HIP-event time."""
    import torch
    names = list(arms)
    for _ in range(warmup):
        for n in names:
            arms[n]()
    torch.cuda.synchronize()
    wall, ev = {n: [] for n in names}, {n: [] for n in names}
    for _ in range(reps):
        for n in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            arms[n]()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            wall[n].append((t1 - t0) * 1e3)
            ev[n].append(e0.elapsed_time(e1))
    return {n: {"wall_ms": _stats(wall[n]), "event_ms": _stats(ev[n])} for n in names}


def _net(dtype, B):
    import torch
    from m3dssd_amd import synth
    from model.M3d_inference_align import build
    conf = synth.synth_conf(CROP, 0, batch_size=B, device="cuda:0")
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0))
    return net.to(torch.device("cuda:0")).set_compute_dtype(dtype), conf


def _sclk(dev, fn):
    """Shader clock (GHz) while `fn` replays: one wave samples the cycle counter against the 100 MHz wall clock over 30 ms."""
    import ctypes
    import torch
    from m3dssd_amd import _hip
    try:
        probe = torch.zeros(4, dtype=torch.int64, device=dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        _hip.check(_hip.lib().m3d_clock_probe(ctypes.c_void_p(probe.data_ptr()), 0.03, ctypes.c_void_p(side.cuda_stream)))
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.05:
            fn()
        torch.cuda.synchronize()
        pc = probe.cpu().tolist()
        return round((pc[2] - pc[0]) / (pc[3] - pc[1]) * 0.1, 3) if pc[3] > pc[1] else None
    except Exception:
        return None


def route_leg(dtype, B, a, dev):
    from lib.rpn_util import detect_batch
    from m3dssd_amd import synth
    from m3dssd_amd.pipeline import FrameDetector, PipelinedDetector
    net, conf = _net(dtype, B)
    x = synth.synth_frames(B, CROP, 1234).to(dev)
    f1 = FrameDetector(net, conf, CROP[0], CROP[1], batch=B, topk_wgs=1)
    f0 = FrameDetector(net, conf, CROP[0], CROP[1], batch=B)
    pipe = PipelinedDetector(net, conf, B, CROP[0], CROP[1])
    arms = {"eager": lambda: detect_batch(net, x, conf), "frame_wg1": lambda: f1.detect(x), "frame": lambda: f0.detect(x),
            "eager_again": lambda: detect_batch(net, x, conf), "pipelined_step": lambda: pipe.step(x)}
    arms = {k: v for k, v in arms.items() if k in a.routes}
    res = {"tool": "latency_frame", "kind": "routes", "dtype": dtype, "B": B, "crop": list(CROP), "reps": a.reps, "warmup": a.warmup,
           "frame_topk_wgs": f0.topk_wgs, "routes": interleaved(arms, a.warmup, a.reps),
           "note": "wall_ms = host clock around the call + device synchronise (call latency); event_ms = HIP events around the same "
                   "call; pipelined_step is a throughput step (returns the previous batch), not a latency",
           "sclk_under_frame_ghz": _sclk(dev, lambda: f0.detect(x))}
    return res


def kernel_leg(B, a, dev):
    """The two top-k kernels alone on the keys and planar staging of one seeded fp32 forward."""
    import ctypes
    import torch
    from lib.rpn_util import detect_batch
    from m3dssd_amd import _hip, synth
    L = _hip.lib()
    net, conf = _net("f32", B)
    x = synth.synth_frames(B, CROP, 1234).to(dev)
    detect_batch(net, x, conf)                               # leaves cls_planar / box_planar / score_bits in the plan
    eng = net.engine()
    n = eng.plan_for(B, CROP[0], CROP[1]).named
    bits, cls_pl, box_pl = n["score_bits"], n["cls_planar"], n["box_planar"]
    R = bits.shape[1]
    A, k = eng.A, min(int(conf.nms_topN_pre), R)
    P, rois = eng.P, net.rois.to(dev)
    nb1, nbm = L.m3d_topk_decode_workspace_bytes(B, R), L.m3d_topk_decode_mw_workspace_bytes(B, R, k)
    ws = torch.empty(nbm, device=dev, dtype=torch.uint8)
    ab_ref, ab = torch.empty(B, k, 14, device=dev), torch.empty(B, k, 14, device=dev)
    ptrs = [bits.data_ptr(), cls_pl.data_ptr(), box_pl.data_ptr(), rois.data_ptr(), P["anchors"].data_ptr(), P["means"].data_ptr(),
            P["stds"].data_ptr(), None]

    def st():
        return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def wg1(out=ab):
        _hip.check(L.m3d_topk_decode_planar(*ptrs, out.data_ptr(), None, ws.data_ptr(), nb1, B, A, R // A, k, st()))

    def mw(w):
        return lambda: _hip.check(L.m3d_topk_decode_planar_mw(*ptrs, ab.data_ptr(), None, ws.data_ptr(), nbm, B, A, R // A, k, w, st()))

    wg1(ab_ref)
    arms = {"wg1": wg1}
    for w in a.wgs_sweep:
        mw(w)()
        torch.cuda.synchronize()
        if not torch.equal(ab, ab_ref):
            raise SystemExit("latency_frame: m3d_topk_decode_planar_mw(wgs = %d) differs from m3d_topk_decode_planar" % w)
        arms["mw_%d" % w] = mw(w)
    arms["wg1_again"] = wg1
    return {"tool": "latency_frame", "kind": "kernel", "B": B, "R": R, "k": k, "reps": a.reps, "warmup": a.warmup,
            "arms": interleaved(arms, a.warmup, a.reps),
            "note": "kernel time of the top-k + decode alone (event_ms); wg1_again = the single-workgroup kernel as a second arm"}


def trace_run(a, dev):
    """What the kernel trace is taken of: five synchronised replays of one fp32 frame at B = 1."""
    import torch
    from m3dssd_amd import synth
    from m3dssd_amd.pipeline import FrameDetector
    net, conf = _net(a.dtype[0], 1)
    det = FrameDetector(net, conf, CROP[0], CROP[1], topk_wgs=a.trace_topk_wgs)
    x = synth.synth_frames(1, CROP, 1234).to(dev)
    for _ in range(5):
        det.detect(x)
        torch.cuda.synchronize()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", nargs="+", default=["f32", "bf16"], choices=["f32", "bf16"])
    ap.add_argument("--batch", type=int, nargs="*", default=[1, 2, 4])
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--routes", nargs="+", default=["eager", "frame_wg1", "frame", "eager_again", "pipelined_step"])
    ap.add_argument("--kernel-batches", type=int, nargs="*", default=[1])
    ap.add_argument("--wgs-sweep", type=int, nargs="+", default=[4, 8, 16, 32, 64, 128, 256])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--trace-topk-wgs", type=int, default=None)
    ap.add_argument("--merge-trace")
    ap.add_argument("--save-replay-csv")
    ap.add_argument("--replay-end", default=REPLAY_END)
    a = ap.parse_args(argv)
    if a.merge_trace:
        merge_trace(a.merge_trace, a.save_replay_csv, a.replay_end)
        return 0
    dev = _need_gpu()
    if a.trace_run:
        trace_run(a, dev)
        return 0
    from m3dssd_amd import _hip
    hashes = _hip.lib_source_hashes()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(res):
        print(json.dumps(res), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(dict(res, source_hashes=hashes)) + "\n")

    for B in a.kernel_batches:
        emit(kernel_leg(B, a, dev))
    for dtype in a.dtype:
        for B in a.batch:
            emit(route_leg(dtype, B, a, dev))
    return 0


if __name__ == "__main__":
    sys.exit(main())
