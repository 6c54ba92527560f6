"""GPU tests (-m gpu; every check goes through the C ABI of libm3dssd_hip.so) of the drop-in boundary (SURVEY 8 row b) and multi-GPU path (row e) on the device: library loading / error reporting,
checkpoint loading through wrappers, DataParallel replicas, non-current devices, bench.py launch paths, two-rank gather, RCCL.
Re-filed by component in round 5 (before: per-round files); tolerances are stated at the checks."""
import collections
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from m3dssd_amd import _hip, synth
from gpu_common import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------ library
def test_library_loads_and_reports_errors():
    from m3dssd_amd import _hip
    L = _hip.lib()
    assert L.m3d_abi_version() == 5
    d = _hip.ConvDesc()
    assert L.m3d_conv2d_forward(d, None) != 0          # null pointers -> M3D_E_ARG, no crash
    assert b"null" in L.m3d_last_error()
    with pytest.raises(NotImplementedError):
        from m3dssd_amd.host import ops
        ops.dcn_v2_forward(torch.zeros(1, 2, 4, 4), torch.zeros(1, 18, 4, 4), torch.zeros(1, 9, 4, 4),
                           torch.zeros(2, 2, 3, 3), torch.zeros(2), 1, 1)


# ------------------------------------------------------------------------------------ the benched configuration vs the oracle
def test_bench_config_batch8_wave_plan_matches_oracle_directly():
    """BASELINE.json configs[1] as benched: bs = 8, 1280x384 -> the plan with the wave-granular kernels (Winograd wave, conv /
    deformable wave, batched heads) against the CPU oracle on the same 8 frames (no HIP-vs-HIP hop): cls upstream of the
    decisions, everything downstream with the engine's decisions injected; 3-D box parameters within 1e-3 abs."""
    from model.M3d_inference_align import build
    from oracle import model_cpu
    dev = _dev()
    B, crop = 8, (384, 1280)
    conf = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0")
    sd = synth.synth_state_dict(0)
    x = synth.synth_frames(B, crop, 1234)
    x[4:, :, :, (2 * crop[1]) // 3:] = 0.0                      # half of the frames with the test-time zero border
    net = build(conf, "test")
    net.load_state_dict(sd, strict=True)
    net = net.to(dev)
    with torch.no_grad():
        cls, prob, b2, b3 = (t.cpu() for t in net(x.to(dev))[:4])
    plan = net.engine().plan_for(B, *crop)
    kinds = {op[1] for op in plan.ops}
    # (round 3: the 3x3 stride-1 layers of level2..5 and cls.0 run on the F(4x4,3x3) kernel, level5 in its split-K form; round 4:
    # all of them on the 64-channel form at two workgroups per CU, level4 -- 240 workgroups for 512 slots -- as K-pair workgroups)
    assert any(k.startswith("wino44<16,16,splitk") for k in kinds) and "wino44<16,16>" in kinds and "wino44<16,16,kpair>" in kinds, kinds
    assert any(k.startswith("conv_wave<deform") for k in kinds), kinds
    fh, fw = crop[0] // 8, crop[1] // 8
    ind = plan.named["sel_idx"].view(B, 1, fh, fw).long().cpu()
    prob_sel = plan.named["sel_prob"].view(B, 1, fh, fw).cpu()
    cconf = synth.synth_conf(crop, 0, batch_size=B, device="cpu")
    taps = {}
    with torch.no_grad():
        free = model_cpu.rpn_forward(sd, cconf, x, taps)
        inj = model_cpu.rpn_forward(sd, cconf, x, inject={"sel": {"ind": ind, "hard": (prob_sel > 0.5).float()}})
    e_cls = (cls - free[0]).abs().max().item() / (1.0 + free[0].abs().max().item())
    fg = taps["fg_prob"]
    o_mask, o_ind = fg.max(dim=1, keepdim=True)
    diff, flip = (o_ind != ind), ((o_mask > 0.5) != (prob_sel > 0.5))
    if diff.any():
        assert ((o_mask - torch.gather(fg, 1, ind))[diff].abs() < 1e-4).all()
    if flip.any():
        assert ((o_mask - 0.5)[flip].abs() < 1e-4).all()
    e_prob = (prob - inj[1]).abs().max().item()
    e_b2 = (b2 - inj[2]).abs().max().item()
    e_b3 = (b3 - inj[3]).abs().max().item()
    _log("bench_config_batch8", dict(cls_rel=e_cls, prob=e_prob, bbox_2d=e_b2, bbox_3d=e_b3, n_idx=int(diff.sum()),
                                     n_flip=int(flip.sum()), pixels=int(diff.numel())))
    assert e_cls < 1e-3 and e_prob < 1e-4 and e_b2 < 1e-3
    assert e_b3 < 1e-3                                           # BASELINE.json: 3-D box params within 1e-3 abs (fp32)
    assert int(diff.sum()) + int(flip.sum()) <= 16               # near-ties only, and only a handful of them


# ------------------------------------------------------------------------------------ device handling
def test_module_on_a_device_that_is_not_current():
    """Engine launches go to the stream of the ENGINE's device whatever the caller's current device is (a second device
    when the box has one; with one device the same path runs under an explicit non-default current stream)."""
    from lib.rpn_util import detect_batch
    from model.M3d_inference_align import build
    n_dev = torch.cuda.device_count()
    tgt = torch.device("cuda", n_dev - 1)
    conf = synth.synth_conf((128, 320), 0, batch_size=2, device=str(tgt))
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0))
    net = net.to(tgt)
    x = synth.synth_frames(2, (128, 320), 5).to(tgt)
    with torch.cuda.device(tgt):
        ref = [t.clone() for t in net(x)[:4]]
        rd, rc = (t.clone() for t in detect_batch(net, x, conf))
    torch.cuda.synchronize(tgt)
    side = torch.cuda.Stream(tgt)
    with torch.cuda.device(0), torch.cuda.stream(side):
        got = [t.clone() for t in net(x)[:4]]
        gd, gc = (t.clone() for t in detect_batch(net, x, conf))
    side.synchronize()
    for u, v in zip(ref, got):
        assert torch.equal(u, v)
    assert torch.equal(rd, gd) and torch.equal(rc, gc)
    with pytest.raises(RuntimeError):
        net.engine().forward(x.cpu().to("cuda:0") if n_dev > 1 else x[:, :, :100])   # wrong device / bad size


_FIRST_LAUNCH_SCRIPT = r"""
import ctypes, json, sys
import numpy as np
import torch
import torch.nn.functional as F
sys.path[:0] = [%(root)r, %(tests)r]
import gpu_common as G
from m3dssd_amd import _hip
from m3dssd_amd.host import standalone as S

L = _hip.lib()
BF16 = torch.bfloat16


def bf16_close(got, ref):                   # tests/test_gpu_bf16.py:_check, bf16 output: one rounding of the result + fp32 summation noise
    scale = ref.abs().max().item() + 1e-6
    bad = (got.double() - ref).abs() > 2.0 ** -8 * ref.abs() + 1e-3 * scale
    assert not bad.any(), ((got.double() - ref).abs().max().item(), scale, int(bad.sum()))


def families(dev):
    out = {}
    # F(2x2,3x3) Winograd, 135 168 B of LDS, on the shape of WINO_CASES[0] (tests/test_gpu_conv.py: _relerr < 2e-4)
    n, ci, h, w, co = G.WINO_CASES[0][:5]
    g = torch.Generator().manual_seed(1)
    x, wt = torch.randn(n, ci, h, w, generator=g), torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5
    v, _ = S._to_nhwc(x.to(dev))
    o, keep = S.conv_nhwc(v, wt.to(dev), None, None, 1, 1, act=1, wino=True)
    out["wino"] = S._to_nchw(o, co).cpu()
    assert G._relerr(out["wino"], F.leaky_relu(F.conv2d(x.double(), wt.double(), padding=1), 0.01)) < 2e-4
    # fused head MLP: the smallest case of test_fused_head_mlp_matches_torch (_relerr < 2e-4)
    d, o, ref, keep = G._head_case(133, 128, 5, 64, dev, ref_dtype=torch.float64)
    _hip.check(L.m3d_head_mlp_forward(ctypes.byref(d), S._stream()))
    out["head_mlp"] = o.view(ref.shape).cpu()
    assert G._relerr(out["head_mlp"], ref) < 2e-4
    # implicit GEMM on its 128 x 128 x 32 tile, the only one above 64 KB of LDS (test_conv_igemm_matches_torch: _relerr < 2e-4)
    n, ci, h, w, co = 1, 32, 128, 200, 256
    x, wt = torch.randn(n, ci, h, w, generator=g), torch.randn(co, ci, 1, 1, generator=g) / ci ** 0.5
    v, _ = S._to_nhwc(x.to(dev))
    wp, _, cop, _, _ = S._pack(wt.to(dev), v.c, 32)
    sc, sh = S._affine(co, None, None, dev)
    o = torch.empty(n * h * w * co, device=dev)
    d = _hip.ConvDesc()
    d.inp, d.in_cs, d.N, d.H, d.W, d.Cin = v.ptr, v.cs, n, h, w, v.c
    d.wgt, d.Cout, d.Cout_pad = wp.data_ptr(), co, cop
    d.kh, d.kw, d.stride, d.pad, d.dil, d.Ho, d.Wo = 1, 1, 1, 0, 1, h, w
    d.out, d.out_cs, d.scale, d.shift, d.sigmoid_from = o.data_ptr(), co, sc.data_ptr(), sh.data_ptr(), -1
    t = [ctypes.c_int() for _ in range(4)]
    _hip.check(L.m3d_conv2d_tile(ctypes.byref(d), *[ctypes.byref(c) for c in t]))
    assert [c.value for c in t[:3]] == [128, 128, 32], [c.value for c in t]
    _hip.check(L.m3d_conv2d_forward(ctypes.byref(d), S._stream()))
    out["igemm"] = o.view(n, h, w, co).permute(0, 3, 1, 2).cpu()
    assert G._relerr(out["igemm"], F.conv2d(x.double(), wt.double())) < 2e-4
    # bf16: the wide wave-tile kernel (variant 5, WIDE_CASES[0]) and the persistent-grid 64 -> 64 kernel (variant 8, sized by the CU count)
    for name, (n, ci, h, w, co), variant in (("wide", (1, 64, 8, 16, 128), 5), ("c64", (1, 64, 8, 32, 64), 8)):
        x = torch.randn(n, ci, h, w, generator=g).to(BF16).float()
        wt = (torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5).to(BF16).float()
        b = torch.randn(co, generator=g) * 0.1
        out[name] = G._run_conv(x, wt, b, None, 1, 1, 0, None, 0, -1, 0, in_cs=ci + 8, variant=variant, wide=variant == 5)
        bf16_close(out[name], F.conv2d(x.double(), wt.double(), b.double(), padding=1))
    # top-k select + decode with k = 8192 (4096 is the largest k that needs no raise): test_topk_decode_matches_stable_sort
    R, k, A = 16384, 8192, 36
    scores = torch.rand(R, generator=g) ** 6
    ins = [u.to(dev).contiguous() for u in G._topk_inputs(R, A, 3, scores)]
    bits = G._sortable_bits(scores)
    bits_dev = torch.from_numpy(bits.numpy().astype(np.uint32).view(np.int32)).to(dev)
    ab, rows = torch.empty(1, k, 14, device=dev), torch.empty(1, k, device=dev, dtype=torch.int32)
    nb = L.m3d_topk_decode_workspace_bytes(1, R)
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    _hip.check(L.m3d_topk_decode(bits_dev.data_ptr(), *[u.data_ptr() for u in ins], ab.data_ptr(), rows.data_ptr(), ws.data_ptr(),
                                 nb, 1, R, k, G._stream()))
    order = np.lexsort((np.arange(R), -bits.numpy().astype(np.int64)))[:k]
    want = torch.empty(1, k, 14, device=dev)
    rows64 = torch.from_numpy(order[None].astype(np.int64)).to(dev)
    _hip.check(L.m3d_decode_rows(rows64.data_ptr(), *[u.data_ptr() for u in ins], want.data_ptr(), 1, R, k, G._stream()))
    torch.cuda.synchronize()
    assert np.array_equal(rows[0].cpu().numpy().astype(np.int64), order) and torch.equal(ab, want)
    out["topk"] = ab.cpu()
    return out


n_dev = torch.cuda.device_count()
res = {}
for i in reversed(range(n_dev)):            # highest ordinal first, device 0 last: no launcher has run on a device before its turn
    dev = torch.device("cuda", i)
    torch.cuda.set_device(dev)
    G._dev = lambda dev=dev: dev
    res[i] = families(dev)
for i in range(1, n_dev):
    for name, t in res[0].items():
        assert torch.equal(t, res[i][name]), (i, name)
print(json.dumps({"FIRST_LAUNCH_OK": n_dev, "families": sorted(res[0])}))
"""


def test_first_launch_on_every_device(tmp_path):
    """The launchers' once-per-device state (csrc/common.h: raised LDS limits, CU count, zero page) in a FRESH process: on every
    visible device, highest ordinal first and device 0 last, the first call of each family that raises its dynamic-LDS limit (F(2x2)
    Winograd, fused head MLP, the 128 x 128 x 32 implicit-GEMM tile, the bf16 wide tile, top-k with k = 8192) and of one
    persistent-grid launcher (bf16 64 -> 64) meets that family's own tolerance against torch fp64, and every device gives the bits
    of device 0.  With one visible device this is one iteration; the multi-device half needs torch.cuda.device_count() >= 2."""
    script = tmp_path / "first_launch.py"
    script.write_text(_FIRST_LAUNCH_SCRIPT % dict(root=ROOT, tests=os.path.join(ROOT, "tests")))
    res = subprocess.run([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300,
                         cwd=ROOT)
    assert res.returncode == 0, res.stdout[-3000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    assert got["FIRST_LAUNCH_OK"] == torch.cuda.device_count() >= 1
    assert got["families"] == ["c64", "head_mlp", "igemm", "topk", "wide", "wino"]
    _log("first_launch_on_every_device", {"devices": got["FIRST_LAUNCH_OK"]})


def test_rccl_single_rank_collective_runs():
    """RCCL itself on the leased GPU: a 1-rank nccl process group runs the same all_gather_into_tensor the N > 1 path issues."""
    import subprocess
    import sys
    code = ("import os, torch, torch.distributed as dist\n"
            "os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT='%d', RANK='0', WORLD_SIZE='1')\n"
            "torch.cuda.set_device(0)\n"
            "dist.init_process_group('nccl', rank=0, world_size=1)\n"
            "b = torch.arange(2 * 41 * 14, device='cuda', dtype=torch.float32).view(2, 41, 14)\n"
            "o = torch.empty_like(b)\n"
            "dist.all_gather_into_tensor(o, b)\n"
            "torch.cuda.synchronize()\n"
            "assert torch.equal(o, b)\n"
            "dist.destroy_process_group()\n"
            "print('RCCL_OK')\n" % _free_port())
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0 and "RCCL_OK" in res.stdout, res.stdout[-2000:]


# ------------------------------------------------------------------------------------ host boundary
def test_module_prefixed_checkpoint_then_forward_equals_plain_load():
    dev = _dev()
    x = synth.synth_frames(2, CROP, 5).to(dev)
    net, conf, sd = _net_sd()
    net.load_state_dict(sd)
    ref = [t.clone() for t in net.to(dev)(x)[:4]]
    net2, _, _ = _net_sd()
    net2.load_state_dict(collections.OrderedDict(("module." + k, v) for k, v in sd.items()), strict=True)
    got = net2.to(dev)(x)[:4]
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


def test_load_through_wrapper_repacks_the_engine():
    """forward -> wrapper.load_state_dict(other checkpoint) -> forward must run the NEW weights (nn.Module.load_state_dict on a
    parent recurses through child._load_from_state_dict and never calls RPN.load_state_dict)."""
    dev = _dev()
    x = synth.synth_frames(2, CROP, 6).to(dev)
    net, conf, sd0 = _net_sd(0)
    sd1 = synth.synth_state_dict(1)
    net.load_state_dict(sd0)
    net = net.to(dev)
    out0 = [t.clone() for t in net(x)[:4]]
    wrapper = nn.DataParallel(net, device_ids=[0])
    wrapper.load_state_dict(collections.OrderedDict(("module." + k, v) for k, v in sd1.items()))
    out1 = [t.clone() for t in net(x)[:4]]
    assert not torch.equal(out0[3], out1[3]), "the packed engine still holds the previous checkpoint"
    fresh, _, _ = _net_sd(1)
    fresh.load_state_dict(sd1)
    ref1 = fresh.to(dev)(x)[:4]
    for a, b in zip(out1, ref1):
        assert torch.equal(a, b)
    holder = nn.ModuleDict({"det": net})
    holder.load_state_dict(collections.OrderedDict(("det." + k, v) for k, v in sd0.items()))
    for a, b in zip(net(x)[:4], out0):
        assert torch.equal(a, b)


def test_data_parallel_wrapper_on_the_leased_device_equals_the_module():
    """The reference script wraps the net in nn.DataParallel (scripts/test_rpn_3d.py:50-51).  With one visible device the
    wrapper calls the module itself; a replica made for a second device would pack its own engine (the replica hook is
    exercised directly: it must not share the source's plans)."""
    dev = _dev()
    x = synth.synth_frames(2, CROP, 7).to(dev)
    net, conf, sd = _net_sd()
    net.load_state_dict(sd)
    net = net.to(dev)
    ref = [t.clone() for t in net(x)]
    got = nn.DataParallel(net, device_ids=[0])(x)
    assert len(got) == 6
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    # a REAL replica (torch.nn.parallel.replicate: `_parameters` is empty, the broadcast copies hang on it as plain attributes
    # and every child is a replica too) must run: it asks the source module for the engine of its device
    from torch.nn.parallel import replicate
    rep = replicate(net, [0])[0]
    assert rep is not net and len(list(rep.parameters())) == 0 and getattr(rep, "_is_replica", False)
    assert rep._engine is None and net._engine is not None
    for a, b in zip(rep(x)[:4], ref[:4]):
        assert torch.equal(a, b)
    assert rep.engine(x.device) is net._engine          # same device: the source's own packed engine, not a second copy
    # a replica "on another device" packs a per-device engine once, from the source's state_dict, and keeps it across replicas
    e1 = net._engine_for("cuda:0")
    assert e1 is net._engine
    net.refresh_engine()
    assert "_device_engines" not in net.__dict__ and net._engine is None


def _bench_line_and_detail(out, detail_path):
    """ONE JSON line on stdout, < 4 KB (the driver keeps only the tail of stdout: BENCH_r05.json had parsed = null for a 24 KB line);
    the full record sits in the detail file the line names."""
    import bench
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    assert len(lines[0]) < bench.LINE_LIMIT == 4096, len(lines[0])
    r = json.loads(lines[0])
    assert r["detail"] == str(detail_path)
    return r, json.load(open(detail_path))


def test_bench_two_ranks_gloo_emits_one_parseable_line(tmp_path):
    """`python bench.py --gpus 2` self-launches under torch.distributed.run; both ranks share the leased device (gloo), run the
    pipelined graph, the per-step gather_block, the barriers and the all_reduce(MAX) of the elapsed time; rank 0 prints ONE
    compact JSON line for the whole job and writes the full record to the detail file."""
    det = tmp_path / "detail.json"
    rc, out, err = _run_bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--detail", str(det)],
                              {"M3D_DIST_BACKEND": "gloo"})
    assert rc == 0, err[-3000:]
    r, full = _bench_line_and_detail(out, det)
    assert r["n_gpus"] == 2 and r["config"]["global_batch"] == 16 and r["config"]["per_gpu_batch"] == 8
    assert r["steps"] == 3 and r["scaling"] == "weak" and r["dist_backend"] == "gloo"
    assert r["value"] > 0 and abs(r["value"] - 16 * 3 / (r["ms_per_step"] * 3e-3)) / r["value"] < 0.01
    assert "configs2_bf16" not in r and "cpu_baseline" not in r and "dropin" not in r          # N = 1 only
    assert r["roofline"]["frac"] > 0 and "traffic" in r["roofline"]
    assert r["value"] == full["value"] and r["roofline"]["frac"] == full["roofline"]["frac"]
    # the N > 1 record proves what the collective saw and isolates its cost (VERDICT r3 #4d)
    c = full["rccl"]
    assert c["world_size"] == 2 and c["backend"] == "gloo" and len(c["ranks_seen"]) == 2
    assert sorted(d["rank"] for d in c["ranks_seen"]) == [0, 1] and len({d["pid"] for d in c["ranks_seen"]}) == 2
    assert c["distinct_devices"] == 1                   # both test ranks share the leased GPU (RCCL would need 2: see below)
    assert c["gathered_rows"][0] == 16 and c["gathered_rows"][2] == 14 and c["allgather_us"] > 0
    assert c["shards_recomputed_on_rank0"] == 2 and c["shards_match"] is True
    assert r["rccl"]["shards_match"] is True and r["rccl"]["world_size"] == 2
    assert r["step_roofline"]["mfma_frac"] > 0 and 0 < r["mfma_time_weighted_frac"] < 1
    assert full["helper_kernels"]["bundle"]["algorithmic_gbs"] > 0


def test_forward_returns_fresh_tensors_unless_reuse_outputs():
    """VERDICT r5 #6 / M3d_inference_align.py:303-313: the reference returns fresh tensors, so a caller may keep the outputs of one
    forward across the next.  RPN.forward clones the four big outputs by default; conf.reuse_outputs / net.reuse_outputs = True
    returns views of the plan-owned buffers (what the device detection stage uses internally) that the next forward overwrites."""
    from model.M3d_inference_align import build
    dev = _dev()
    crop, B = (128, 320), 2
    conf = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0")
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0), strict=True)
    net = net.to(dev)
    x0, x1 = synth.synth_frames(B, crop, 1).to(dev), synth.synth_frames(B, crop, 2).to(dev)
    with torch.no_grad():
        kept = net(x0)                                   # kept across the next forward, as a reference-style caller would
        snap = [t.clone() for t in kept[:4]]
        other = net(x1)
        torch.cuda.synchronize()
    plan = net.engine().plan_for(B, *crop)
    owned = {plan.named[k].data_ptr() for k in ("cls", "prob", "bbox_2d", "bbox_3d")}
    for a, b, c in zip(kept[:4], snap, other[:4]):
        assert torch.equal(a, b) and not torch.equal(a, c)          # untouched by the second forward, which computed something else
        assert a.data_ptr() not in owned and c.data_ptr() not in owned and a.data_ptr() != c.data_ptr()
    assert tuple(kept[4].tolist()) == (16.0, 40.0) and kept[5].shape == (36 * 16 * 40, 5)
    # opt-in: views of the plan's buffers, overwritten by the next call
    net.reuse_outputs = True
    with torch.no_grad():
        v0 = net(x0)
        s0 = [t.clone() for t in v0[:4]]
        net(x1)
        torch.cuda.synchronize()
    assert {t.data_ptr() for t in v0[:4]} == owned
    for a, b, c in zip(v0[:4], s0, snap):
        assert torch.equal(b, c) and not torch.equal(a, b)          # same values as the fresh form; the view now holds batch x1
    conf2 = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0")
    conf2.reuse_outputs = True
    assert build(conf2, "test").reuse_outputs is True


def test_pipelined_detector_joins_before_the_first_write_of_what_detect_reads():
    """with SELECT_KEYS anchor_select of forward(k) writes plan.named['score_bits'] in the middle of the
    forward; in the bundled form (planar=False) detect(k-1) on the side branch reads it, so the join has to sit in front of that op
    -- not at bundle_outputs.  Results equal detect_batch for a sequence of different batches in both forms."""
    from model.M3d_inference_align import build
    from lib.rpn_util import detect_batch
    from m3dssd_amd.pipeline import PipelinedDetector
    dev = _dev()
    crop, B = (128, 320), 2
    conf = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0")
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0), strict=True)
    net = net.to(dev)
    frames = [synth.synth_frames(B, crop, 10 + i).to(dev) for i in range(4)]
    want = []
    for f in frames:
        d, c = detect_batch(net, f, conf)
        want.append((d.clone(), c.clone()))
    for planar in (False, True):
        pipe = PipelinedDetector(net, conf, B, crop[0], crop[1], planar=planar)
        n = pipe.plan.named
        assert n.get("keys_by_select") and "score_bits_first_write_op" in n
        if planar:
            assert pipe.n_join == n["planar_first_op"] <= n["score_bits_first_write_op"]
        else:
            assert pipe.n_join == n["score_bits_first_write_op"] < pipe.n_fwd
            assert pipe.plan.ops[pipe.n_join][0] == "anchor_select"
        got = []
        for f in frames:
            r = pipe.step(f)
            if r is not None:
                got.append((r[0].clone(), r[1].clone()))
        r = pipe.flush()
        got.append((r[0].clone(), r[1].clone()))
        torch.cuda.synchronize()
        for (d, c), (wd, wc) in zip(got, want):
            assert torch.equal(c, wc) and torch.equal(d, wd), planar
    # the guard itself: a join behind the first writer is refused
    pipe.n_join = pipe.n_fwd
    with pytest.raises(AssertionError):
        pipe._check_no_write_beside_detect()


def test_detection_stage_takes_the_data_parallel_wrapper_like_the_reference_script(tmp_path):
    """scripts/test_rpn_3d.py:50-59 wraps the network in nn.DataParallel and hands THE WRAPPER to test_kitti_3d -> im_detect_3d
    (lib/rpn_util.py:1439: `net(im)`).  The device detection stage needs the module behind it (engine, plan buffers):
    im_detect_3d / detect_batch / test_kitti_3d / PipelinedDetector unwrap `.module` and return what the bare module returns."""
    from model.M3d_inference_align import build
    from lib.rpn_util import detect_batch, im_detect_3d, test_kitti_3d
    from m3dssd_amd.config import Conf
    from m3dssd_amd.pipeline import PipelinedDetector
    dev = _dev()
    crop, B = (128, 320), 2
    conf = synth.synth_conf(crop, 0, batch_size=B, device="cuda:0")
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0), strict=True)
    net = net.to(dev)
    wrapped = nn.DataParallel(net, device_ids=[0])
    x = synth.synth_frames(B, crop, 5).to(dev)
    d0, c0 = (t.clone() for t in detect_batch(net, x, conf))
    d1, c1 = detect_batch(wrapped, x, conf)
    assert torch.equal(d0, d1) and torch.equal(c0, c1)
    a = im_detect_3d(x[:1], net, conf)
    b = im_detect_3d(x[:1], wrapped, conf)
    assert a.shape[1] == 14 and np.array_equal(a, b)
    pipe = PipelinedDetector(wrapped, conf, B, crop[0], crop[1])
    assert pipe.step(x) is None
    r = pipe.flush()
    assert torch.equal(r[0], d0) and torch.equal(r[1], c0)
    p2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884],
                   [0.0, 0.0, 0.0, 1.0]])
    data = [(x[i:i + 1].cpu(), Conf(id="%06d" % i, p2=p2, scale_factor=1.0)) for i in range(B)]
    for tag, n in (("bare", net), ("wrapped", wrapped)):
        test_kitti_3d(data, n, conf, str(tmp_path / tag), str(tmp_path), use_log=False, require_labels=False)
    for i in range(B):
        assert open(tmp_path / "bare" / ("%06d.txt" % i)).read() == open(tmp_path / "wrapped" / ("%06d.txt" % i)).read()
    with pytest.raises(TypeError):
        detect_batch(nn.Linear(2, 2), x, conf)


def test_bench_nccl_refuses_more_ranks_than_devices():
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a single-device lease")
    rc, out, err = _run_bench(["--gpus", "2", "--steps", "1", "--warmup", "1", "--no-cpu-baseline"], {"M3D_DIST_BACKEND": "nccl"},
                              timeout=300)
    assert rc != 0 and "visible devices" in (out + err)


def test_bench_default_line_is_compact_and_carries_configs2_dropin_and_roofline(tmp_path):
    """`python bench.py --full`, N = 1: ONE line < 4 KB holding the f32 headline, the dominant kernel's roofline,
    the bs = 64 bf16 measurement, the configs[3] shard and the drop-in leg (the reference's own call sequence, eager and as one
    graph); the kernel-family tables are in the detail file, not on stdout."""
    det = tmp_path / "detail.json"
    rc, out, err = _run_bench(["--steps", "5", "--warmup", "2", "--full", "--configs2-steps", "3", "--configs3-steps", "2", "--dropin-steps", "3",
                               "--no-cpu-baseline", "--detail", str(det)], {})
    assert rc == 0, err[-3000:]
    r, full = _bench_line_and_detail(out, det)
    assert r["dtype"] == "f32" and r["config"]["per_gpu_batch"] == 8 and "workload" in r["config"]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "data"):
        assert k in r, k
    rf = r["roofline"]
    assert rf["bound"] == "mfma" and rf["peak"] == 157.3 and 0 < rf["frac"] < 1 and rf["avg_launch_ms"] > 0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and "traffic" in rf and "kernel" in rf
    assert "bundle_outputs NOT run" in r["work_in_timed_region"]
    c2 = r["configs2_bf16"]
    assert c2["dtype"] == "bf16" and c2["per_gpu_batch"] == 64 and c2["steps"] == 3
    assert c2["value"] > r["value"] and c2["roofline"]["peak"] == 2500.0 and c2["step"]["mfma_frac"] > 0
    for d in (r["dropin"], c2["dropin"]):               # net(x) -> six fresh tensors -> decode + NMS, eager and as one graph
        assert d["eager"]["value"] > 0 and d["graph"]["value"] >= 0.8 * d["eager"]["value"]
        assert d["graph"]["ms_per_step"] > 0 and 0 < d["vs_headline_graph"] < 1.2
    assert r["configs3_shard32"]["f32"]["value"] > 0 and r["configs3_shard32"]["bf16"]["value"] > 0
    assert r["feed_u8"]["value"] > 0
    # the full record keeps what the line dropped
    assert "mfma_kernel_families" not in r and "helper_kernels" not in r and "gpu_ms_by_kernel_one_step" not in r
    assert len(full["mfma_kernel_families"]) > 5 and "step_roofline" in full["configs2_bf16"]
    assert full["configs2_bf16"]["config"]["per_gpu_batch"] == 64 and len(full["configs2_bf16"]["mfma_kernel_families"]) > 5


def test_bench_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """`python bench.py --steps K --warmup W --dump-outputs DIR`: the headline keys and nothing that takes passes of its own; DIR holds
    the detections of the last timed step, equal to one detection pass of the same seeded frames in this process."""
    from m3dssd_amd.host.detect import detect_device, select_block
    from model.M3d_inference_align import build
    import bench
    det, dump = tmp_path / "detail.json", tmp_path / "out"
    rc, out, err = _run_bench(["--steps", "4", "--warmup", "2", "--dump-outputs", str(dump), "--detail", str(det)], {})
    assert rc == 0, err[-3000:]
    r, full = _bench_line_and_detail(out, det)
    assert r["steps"] == 4 and r["warmup"] == 2 and r["dtype"] == "f32" and r["config"]["per_gpu_batch"] == 8
    assert r["value"] > 0 and abs(r["value"] - 8 * 4 / (r["ms_per_step"] * 4e-3)) / r["value"] < 0.01
    for k in ("dropin", "configs2_bf16", "configs3_shard32", "feed_u8", "cpu_baseline", "step_roofline", "sclk_under_step_ghz"):
        assert k not in r and k not in full, k
    assert r["roofline"] is None and "mfma_kernel_families" not in full
    dets, counts = np.load(dump / "detections.npy"), np.load(dump / "counts.npy")
    assert dets.dtype == np.float32 and counts.dtype == np.float32
    conf = synth.synth_conf(bench.CROP, 0, batch_size=8, device="cuda:0")
    net = build(conf, "test")
    net.load_state_dict(synth.synth_state_dict(0), strict=True)
    net = net.to(_dev())
    x = synth.synth_frames(8, bench.CROP, 1234).to(_dev())
    with torch.no_grad():
        block, cnt = select_block(*detect_device(net, x, conf), conf)
    assert dets.shape == (8, int(conf.nms_topN_post), 14) and counts.shape == (8,)
    assert np.array_equal(counts, cnt.float().cpu().numpy()) and counts.sum() > 0
    assert np.array_equal(dets, block[:, :-1].cpu().numpy())


def test_fp32_forward_is_bit_identical_over_100_runs_at_the_bench_size():
    """the compare-built padding predicates of the non-deformable MFMA kernels (Winograd wave, plain wave conv,
    fused heads) sit next to matrix instructions at 2-3 waves per SIMD like the deformable kernels did when they dropped a
    corner once per 10^5..10^6 states; a wrong select there would show as run-to-run differences at these grid sizes."""
    bad, nbuf, kinds = _soak("f32", 8, (384, 1280), 100)
    assert {"wino44", "conv_wave", "head_mlp", "igemm"} <= kinds, kinds
    assert not bad, bad[:3]
    assert nbuf > 20


@pytest.mark.parametrize("nbytes", [16, 4096 + 7, 223200, 1 << 20])
def test_upload_indirect_copies_what_the_slot_names(nbytes):
    """m3d_upload_indirect: the kernel reads the source ADDRESS from an 8-byte word in pinned host memory when it runs; sizes
    that are not multiples of 16 bytes, a NULL slot (no copy) and a device-resident source."""
    L = _hip.lib()
    dev = _dev()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.RandomState(nbytes % 97)
    a = torch.from_numpy(rng.randint(0, 256, size=nbytes).astype(np.uint8)).pin_memory()
    b = torch.from_numpy(rng.randint(0, 256, size=nbytes).astype(np.uint8)).pin_memory()
    slot = torch.zeros(1, dtype=torch.int64).pin_memory()
    dst = torch.zeros(-(-nbytes // 16) * 16 + 16, dtype=torch.uint8, device=dev)
    for src in (a, b):
        slot[0] = src.data_ptr()
        _hip.check(L.m3d_upload_indirect(ctypes.c_void_p(slot.data_ptr()), ctypes.c_void_p(dst.data_ptr()), nbytes, st))
        torch.cuda.synchronize()
        assert torch.equal(dst[:nbytes].cpu(), src) and int(dst[nbytes:].sum()) == 0       # nothing past the end is touched
    slot[0] = 0
    dst.fill_(7)
    _hip.check(L.m3d_upload_indirect(ctypes.c_void_p(slot.data_ptr()), ctypes.c_void_p(dst.data_ptr()), nbytes, st))
    torch.cuda.synchronize()
    assert int((dst != 7).sum()) == 0                                                      # NULL slot: no copy
    d_src = a.to(dev)
    slot[0] = d_src.data_ptr()
    _hip.check(L.m3d_upload_indirect(ctypes.c_void_p(slot.data_ptr()), ctypes.c_void_p(dst.data_ptr()), nbytes, st))
    torch.cuda.synchronize()
    assert torch.equal(dst[:nbytes].cpu(), a)

