"""GPU tests (-m gpu; every call goes through the C ABI of libm3dssd_hip.so) of the HBM-bound helpers of the bf16 path
(csrc/bf16_kernels.hip): m3d_maxpool2x2_bf16, m3d_upsample2x_add_bf16 (segment form, row form and grid-stride form),
m3d_softmax_rows_bf16, m3d_f32_to_bf16 and m3d_stem_conv7x7_bf16 -- the twins of the fp32 kernels of tests/test_gpu_rpn_glue.py.
The whole-network tests run them at network tolerance only.

References, case tables, bounds and input builders live in tests/bf16_glue_ref.py (checked without a GPU by
tests/test_bf16_glue_host.py).  bf16 values are compared as uint16 bit patterns.  Every buffer a kernel reads or writes sits
between two guard regions pre-filled with a sentinel word, and so do the pad channels of a pixel stride wider than C; every test
asserts that they still hold it.

Exact comparisons (bits): max-pool (max rounds nothing), fp32 -> bf16 against torch's CPU conversion, and the up-sampling on the
exact-arithmetic operands (small integers times multiples of 1/8: every partial sum in any order, fused or not, is exact in fp32
and the result is a bf16 number, so all three forms must return the float64 result bit for bit).
Derived bounds (u = 2^-8, e = 2^-24):
  * up-sampling, random operands: |got - ref| <= u |ref| + 6 e S, S = sum of |product| over the up-to-four taps + |skip|: at most five
    fp32 roundings of partial sums bounded by S, then one rounding to bf16.
  * row softmax: |got - ref| <= u ref + 1e-6: the derived fp32 row-softmax bound of tests/test_gpu_rpn_glue.py, then one rounding.
  * stem: |got - ref| <= u |ref| + 151 e T, T = |scale| sum |x w| + |shift|: 147 fused multiply-adds, one multiply, one add,
    LeakyReLU is 1-Lipschitz (max(v, 0.01f v): the fp32 slope and its product stay inside the two spare units), one rounding to bf16.
    For uint8 frames the convolution input is computed in numpy float32 in the kernel's order (/ 255, - mean, / std: each step
    correctly rounded on both sides), so it is identical.
The knob M3D_UPSAMPLE_ROWS is read once per process: one child process per value runs the whole up-sampling table, the parent
compares.  Left out: the `long long` instantiation of the grid-stride up-sampling kernel (more than 2^31 work items, 34 GB of output).

The large grid-stride case C = 16 at 2 x 512 x 512 has exactly 16384 x 256 work items: the largest grid, but one pass.  C = 24 at the
same size (1.5 x the cap) runs next to it for the stride step.

Measured on the MI355X (worst error / bound, logged through gpu_common._log): up-sampling, random operands 0.996 in each of the three
forms (the bf16 rounding of a value just above a power of two; the exact operands agree bit for bit in all 1088 runs per form);
row softmax 0.994 (384 / 337 / 384), 0.94 .. 0.97 elsewhere, 0 at valid = 1; stem 0.98 on fp32 images (0.69 on the one-pixel image),
0.99 on uint8 frames, 0.91 / 0.92 on the all-0 / all-255 frames.  All of them are the final rounding: the fp32 terms stay far inside
theirs.  fp32 subnormals come out as bf16 subnormals, as torch rounds them.  Times: the three-child up-sampling test 9.5 s (2.9 s per
child), the large up-sampling cases 0.5 s, the max-pool and conversion cases beyond the grid cap 0.1 s each.
"""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_glue_ref as R
from m3dssd_amd import _hip
from gpu_common import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu

SENT = -559038737          # 0xDEADBEEF as int32; as two bf16: 0xBEEF (-0.467), 0xDEAD (-6.2e18) -- bit patterns no test produces as a result
GUARD = 64                 # 4-byte words on each side: 256 bytes, so the payload keeps the allocation's alignment
WGT_GUARD = 512            # below the [4][4][C] up-sampling weights: a tap index that is off by one row stays inside the guard


class Guarded:
    """nbytes (a multiple of 4) on the device between two sentinel-filled guard regions; the payload starts out as sentinel too."""

    def __init__(self, nbytes, guard=GUARD):
        nbytes = int(nbytes)
        assert nbytes > 0 and nbytes % 4 == 0 and guard % 4 == 0
        self.n, self.lo = nbytes // 4, guard
        self.raw = torch.full((guard + self.n + guard,), SENT, dtype=torch.int32, device=_dev())
        self.words = self.raw[guard:guard + self.n]
        self.ptr = self.words.data_ptr()
        assert self.ptr % 16 == 0

    def put(self, arr):
        a = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        assert a.size == 4 * self.n, (a.size, 4 * self.n)
        self.words.view(torch.uint8).copy_(torch.from_numpy(a.copy()))
        return self

    def put_t(self, t):
        self.words.view(t.dtype).copy_(t.reshape(-1))
        return self

    def guards_ok(self):
        return bool((self.raw[:self.lo] == SENT).all()) and bool((self.raw[self.lo + self.n:] == SENT).all())

    def get(self, dtype=np.uint16):
        """Payload as a numpy array (synchronises), after asserting that both guards still hold the sentinel."""
        raw = self.raw.cpu().numpy()
        assert (raw[:self.lo] == SENT).all(), "write below the buffer"
        assert (raw[self.lo + self.n:] == SENT).all(), "write beyond the buffer"
        return raw[self.lo:self.lo + self.n].view(dtype).copy()

    def untouched(self):
        return bool((self.get(np.int32) == SENT).all())


def _sent16(shape):
    """What a bf16 buffer of this shape holds where nothing was written."""
    return np.full(int(np.prod(shape)) // 2, SENT, np.int32).view(np.uint16).reshape(shape)


def _with_pads(bits, cs):
    """bits [..., C] (uint16) -> [..., cs] with sentinel pad channels."""
    out = _sent16(bits.shape[:-1] + (cs,)).copy()
    out[..., :bits.shape[-1]] = bits
    return out


def _ratio(err, bound):
    return float((err / bound).max())


# ======================================================================================== 1. max-pool
def _maxpool(bits, C, c_in0, out_cs, c_out0):
    """bits: uint16 [N][H][W][in_cs]; pools channels [c_in0, c_in0 + C) into channels [c_out0, c_out0 + C) of an [N][H/2][W/2][out_cs]
    buffer.  -> (status, the whole output buffer as uint16 or None if it has no element, output Guarded)."""
    L = _hip.lib()
    N, H, W, in_cs = bits.shape
    d = Guarded(2 * bits.size).put(bits)
    shape = (N, H // 2, W // 2, out_cs)
    nout = int(np.prod(shape))
    out = Guarded(2 * nout if nout else 64)
    rc = L.m3d_maxpool2x2_bf16(d.ptr + 2 * c_in0, in_cs, out.ptr + 2 * c_out0, out_cs, N, H, W, C, _stream())
    got = out.get().reshape(shape) if nout else None
    assert np.array_equal(d.get().reshape(bits.shape), bits), "input modified"
    return rc, got, out


@pytest.mark.parametrize("C,in_cs,c_in0,out_cs,c_out0", R.MAXPOOL_PARAMS)
def test_maxpool_bf16_exact(C, in_cs, c_in0, out_cs, c_out0):
    """Bits against F.max_pool2d of the widened values: even and odd H / W (floor), one output pixel, several blocks, channel
    slices of wider buffers (neighbouring channels keep the sentinel); random values, and all-negative ones (a maximum that starts
    from 0 instead of the first element returns 0 there)."""
    for si, (N, H, W) in enumerate(R.MAXPOOL_MAPS):
        for negative in (False, True):
            bits = R.maxpool_input(C * 100 + in_cs + 10 * si + negative, N, H, W, in_cs, negative)
            rc, got, _ = _maxpool(bits, C, c_in0, out_cs, c_out0)
            _hip.check(rc)
            x = torch.from_numpy(R.widen(bits[..., c_in0:c_in0 + C])).double()
            ref = F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous().numpy()
            tag = (N, H, W, negative)
            assert np.array_equal(got[..., c_out0:c_out0 + C], R.bf16_bits(ref)), tag
            assert np.array_equal(R.widen(got[..., c_out0:c_out0 + C]).astype(np.float64), ref), tag
            sent = _sent16(got.shape)
            assert np.array_equal(got[..., :c_out0], sent[..., :c_out0]) and np.array_equal(got[..., c_out0 + C:], sent[..., c_out0 + C:]), tag


def test_maxpool_bf16_degenerate_maps_write_nothing():
    """H or W of 1: zero output elements.  The call returns M3D_OK, writes nothing and leaves no error behind: a call on a valid
    shape right after it succeeds.  (A launch with a grid of 0 blocks is an error of the runtime: the entry point returns first.)"""
    L = _hip.lib()
    for N, H, W in R.MAXPOOL_DEGENERATE:
        rc, got, out = _maxpool(R.maxpool_input(N + H + W, N, H, W, 8, False), 8, 0, 8, 0)
        assert rc == 0, ((N, H, W), rc, L.m3d_last_error())
        assert got is None and out.untouched()
        bits = R.maxpool_input(5, 1, 2, 2, 8, False)
        rc, got, _ = _maxpool(bits, 8, 0, 8, 0)
        assert rc == 0, ((N, H, W), "the valid call after it", rc, L.m3d_last_error())
        assert np.array_equal(got.reshape(8), R.bf16_bits(R.widen(bits).reshape(4, 8).max(axis=0)))
    torch.cuda.synchronize()


def test_maxpool2x2_fp32_degenerate_maps_write_nothing():
    """The fp32 twin (csrc/backbone_kernels.hip) issued the same launch with a grid of 0 blocks."""
    L = _hip.lib()
    for N, H, W in R.MAXPOOL_DEGENERATE:
        x = np.random.default_rng(N + H + W).standard_normal((N, H, W, 4)).astype(np.float32)
        d, out = Guarded(4 * x.size).put(x), Guarded(64)
        rc = L.m3d_maxpool2x2(d.ptr, 4, out.ptr, 4, N, H, W, 4, _stream())
        assert rc == 0, ((N, H, W), rc, L.m3d_last_error())
        assert out.untouched() and d.guards_ok()
        y = np.random.default_rng(9).standard_normal((1, 2, 2, 4)).astype(np.float32)
        dy, oy = Guarded(4 * y.size).put(y), Guarded(4 * 4)
        rc = L.m3d_maxpool2x2(dy.ptr, 4, oy.ptr, 4, 1, 2, 2, 4, _stream())
        assert rc == 0, ((N, H, W), "the valid call after it", rc, L.m3d_last_error())
        assert np.array_equal(oy.get(np.float32), y.reshape(4, 4).max(axis=0))
    torch.cuda.synchronize()


def test_maxpool_bf16_beyond_grid_cap():
    """N * (H / 2) * (W / 2) * (C / 8) work items above the cap of 16384 workgroups x 256 threads: the grid-stride loop takes a
    second pass.  Input (integers: bf16 numbers) and reference (amax over a reshaped fp32 view: max is exact) stay on the device."""
    L = _hip.lib()
    N, H, W, C = R.MAXPOOL_BIG
    assert R.maxpool_items(N, H, W, C) > R.MAXPOOL_BF16_CAP[0] * R.MAXPOOL_BF16_CAP[1]
    g = torch.Generator(device=_dev()).manual_seed(3)
    x = torch.randint(-120, 121, (N, H, W, C), device=_dev(), dtype=torch.int32, generator=g).to(torch.bfloat16)
    d = Guarded(2 * x.numel()).put_t(x)
    out = Guarded(2 * x.numel() // 4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _hip.check(L.m3d_maxpool2x2_bf16(d.ptr, C, out.ptr, C, N, H, W, C, _stream()))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    ref = x.view(N, H // 2, 2, W // 2, 2, C).float().amax(dim=(2, 4)).to(torch.bfloat16)
    got = out.words.view(torch.bfloat16).view(N, H // 2, W // 2, C)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    assert out.guards_ok() and d.guards_ok() and torch.equal(d.words.view(torch.bfloat16), x.reshape(-1))
    _log("bf16_glue.maxpool_big", {"items": R.maxpool_items(N, H, W, C), "call_ms": ms})


def test_maxpool_bf16_argument_checks():
    L = _hip.lib()
    d, out = Guarded(2 * 2 * 4 * 4 * 16), Guarded(2 * 2 * 2 * 2 * 16)
    for C, in_cs, out_cs in ((12, 16, 16), (8, 12, 16), (8, 16, 12), (4, 16, 16)):
        assert L.m3d_maxpool2x2_bf16(d.ptr, in_cs, out.ptr, out_cs, 2, 4, 4, C, _stream()) != 0 and b"maxpool_bf16" in L.m3d_last_error()
    assert out.untouched()


# ======================================================================================== 2. up-sampling + skip
def _upsample(x, w, skip, padded):
    """x [N][H][W][C], w [4][4][C], skip [N][2H][2W][C] or None (torch float32 on the host; x and skip bf16 numbers).
    -> (status, uint16 [N][2H][2W][C], flags): flags bit 0 = every guard intact, bit 1 = pad channels of the output still sentinel."""
    L = _hip.lib()
    N, H, W, C = x.shape
    in_cs, skip_cs, out_cs = R.ups_strides(C, padded)
    din = Guarded(2 * N * H * W * in_cs).put(_with_pads(R.bf16_bits(x.numpy()), in_cs))
    dw = Guarded(4 * 16 * C, guard=WGT_GUARD).put(w.numpy().astype(np.float32))
    ds = None if skip is None else Guarded(2 * N * 4 * H * W * skip_cs).put(_with_pads(R.bf16_bits(skip.numpy()), skip_cs))
    out = Guarded(2 * N * 4 * H * W * out_cs)
    rc = L.m3d_upsample2x_add_bf16(din.ptr, in_cs, dw.ptr, None if ds is None else ds.ptr, skip_cs, out.ptr, out_cs, N, H, W, C, _stream())
    got = out.words.cpu().numpy().view(np.uint16).reshape(N, 2 * H, 2 * W, out_cs)
    guards = out.guards_ok() and din.guards_ok() and dw.guards_ok() and (ds is None or ds.guards_ok())
    pads = np.array_equal(got[..., C:], _sent16(got.shape)[..., C:])
    return rc, got[..., :C].copy(), int(guards) | (int(pads) << 1)


def _upsample_child(path):
    """Body of one child process: the whole case table under the value of M3D_UPSAMPLE_ROWS this process was started with.  Writes
    the output bits of every (case, kind, skip / NULL) run, dense strides, concatenated in table order, and one status byte per
    run and stride variant: bit 0 guards, bit 1 pad channels, bit 2 (padded variant) same bits as the dense-stride run."""
    bits, status = [], []
    for index, (C, N, H, W) in enumerate(R.UPS_SHAPES):
        for kind in R.UPS_KINDS:
            x, w, skip = R.ups_operands(kind, index, C, N, H, W)
            dense = None
            for has_skip, padded in R.UPS_VARIANTS:
                rc, got, flags = _upsample(x, w, skip if has_skip else None, padded)
                _hip.check(rc)
                if padded:
                    status.append(flags | (int(np.array_equal(got, dense)) << 2))
                else:
                    dense = got
                    bits.append(got.reshape(-1))
                    status.append(flags | 4)
    torch.cuda.synchronize()
    np.savez(path, bits=np.concatenate(bits), status=np.array(status, np.uint8))


_CHILD = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import test_gpu_bf16_glue as t
t._upsample_child(sys.argv[1])
''' % (ROOT, os.path.join(ROOT, "tests"))


def test_upsample_bf16_three_forms_match_float64(tmp_path):
    """One child process per value of M3D_UPSAMPLE_ROWS (0: grid-stride form, 1: segment form, 2: row form at C = 64 / 128 / 256;
    the other channel counts take the grid-stride form under every value), one after the other; none is started after one that
    failed.  Exact-arithmetic operands: the three forms equal the float64 result, and so each other, bit for bit.  Random
    operands: inside the derived bound.  Segment lengths 1, 2, >= 3, ragged last segments, W = 1, H = 1, skip and NULL, dense and
    padded strides (the child compares the two and checks the sentinel pad channels and every guard)."""
    runs, secs = {}, {}
    for knob in R.UPS_KNOBS:
        path = str(tmp_path / ("ups%s.npz" % knob))
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, "-c", _CHILD, path], env=dict(os.environ, M3D_UPSAMPLE_ROWS=knob), capture_output=True,
                           text=True, timeout=600, cwd=ROOT)
        secs[knob] = time.perf_counter() - t0
        assert r.returncode == 0, (knob, r.stderr[-3000:])
        z = np.load(path)
        runs[knob] = (z["bits"], z["status"])
        os.remove(path)
    nruns = len(R.UPS_SHAPES) * len(R.UPS_KINDS) * len(R.UPS_VARIANTS)
    for knob, (bits, status) in runs.items():
        assert status.shape == (nruns,)
    worst = {k: 0.0 for k in R.UPS_KNOBS}
    off = si = 0
    for index, (C, N, H, W) in enumerate(R.UPS_SHAPES):
        for kind in R.UPS_KINDS:
            x, w, skip = R.ups_operands(kind, index, C, N, H, W)
            for has_skip in (True, False):
                ref, S = R.upsample_ref(x, w, skip if has_skip else None)
                ref, S = ref.numpy(), S.numpy()
                want = R.bf16_bits(ref) if kind == "exact" else None
                for knob, (bits, status) in runs.items():
                    tag = (knob, kind, C, N, H, W, "skip" if has_skip else "NULL")
                    assert status[si] == 7 and status[si + 1] == 7, tag + (int(status[si]), int(status[si + 1]))
                    got = bits[off:off + ref.size].reshape(ref.shape)
                    if kind == "exact":
                        bad = got != want
                        assert not bad.any(), tag + (int(bad.sum()), tuple(int(v[0]) for v in np.nonzero(bad)))
                    else:
                        err, bound = np.abs(R.widen(got).astype(np.float64) - ref), R.upsample_bound(torch.from_numpy(ref), torch.from_numpy(S)).numpy()
                        worst[knob] = max(worst[knob], _ratio(err, bound))
                        assert (err <= bound).all(), tag + (_ratio(err, bound),)
                off += ref.size
                si += 2
    assert all(off == len(b) for b, _ in runs.values())
    print("upsample2x_add_bf16: worst err / bound per knob %s, child seconds %s" % (worst, secs))
    _log("bf16_glue.upsample_forms", {"worst_over_bound": worst, "child_seconds": secs})


@pytest.mark.parametrize("C,N,H,W", R.UPSAMPLE_BIG)
def test_upsample_bf16_grid_stride_at_and_beyond_the_grid_cap(C, N, H, W):
    """Grid-stride form (C = 16 / 24 take it under every knob value) at 2 x 512 x 512.  C = 16: 2 * 4 * 512 * 512 * 2 work items, exactly
    the cap of 16384 x 256 -- the largest grid, still one pass; C = 24: 1.5 x the cap, the loop takes its stride step.  Exact-
    arithmetic operands drawn on the device; the fp32 sum of the exact terms there IS the float64 result; bits."""
    L = _hip.lib()
    assert R.upsample_items(C, N, H, W) >= R.UPSAMPLE_CAP[0] * R.UPSAMPLE_CAP[1]
    x, w, skip = R.ups_exact_operands(7, C, N, H, W, device=_dev())
    din, dw = Guarded(2 * x.numel()).put_t(x.to(torch.bfloat16)), Guarded(4 * w.numel(), guard=WGT_GUARD).put_t(w)
    ds, out = Guarded(2 * skip.numel()).put_t(skip.to(torch.bfloat16)), Guarded(2 * skip.numel())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _hip.check(L.m3d_upsample2x_add_bf16(din.ptr, C, dw.ptr, ds.ptr, C, out.ptr, C, N, H, W, C, _stream()))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    ref = R.upsample_terms(x, w, skip).sum(0)
    assert float(ref.abs().max()) <= 27.0 and torch.equal(ref.to(torch.bfloat16).float(), ref)
    got = out.words.view(torch.bfloat16).view(N, 2 * H, 2 * W, C)
    assert torch.equal(got.view(torch.int16), ref.to(torch.bfloat16).view(torch.int16))
    assert out.guards_ok() and din.guards_ok() and dw.guards_ok() and ds.guards_ok()
    _log("bf16_glue.upsample_big", {"C": C, "items": R.upsample_items(C, N, H, W), "call_ms": ms})


def test_upsample_bf16_argument_checks():
    L = _hip.lib()
    N, H, W = 1, 2, 3
    din, dw, ds, out = Guarded(2 * N * H * W * 32), Guarded(4 * 16 * 32, guard=WGT_GUARD), Guarded(2 * N * 4 * H * W * 32), Guarded(2 * N * 4 * H * W * 32)
    for C, in_cs, skip_cs, out_cs, with_skip in ((12, 16, 16, 16, True), (16, 20, 16, 16, True), (16, 16, 20, 16, True), (16, 16, 16, 20, True),
                                                 (16, 16, 16, 12, False), (4, 16, 16, 16, False)):
        rc = L.m3d_upsample2x_add_bf16(din.ptr, in_cs, dw.ptr, ds.ptr if with_skip else None, skip_cs, out.ptr, out_cs, N, H, W, C, _stream())
        assert rc != 0 and b"upsample2x_add_bf16" in L.m3d_last_error(), (C, in_cs, skip_cs, out_cs)
    assert out.untouched()


# ======================================================================================== 3. row softmax
def _softmax(x, valid, out_cs):
    """x: float32 [rows][cs] -> uint16 [rows][out_cs]."""
    L = _hip.lib()
    rows, cs = x.shape
    d, out = Guarded(4 * x.size).put(x.astype(np.float32)), Guarded(2 * rows * out_cs)
    _hip.check(L.m3d_softmax_rows_bf16(d.ptr, rows, valid, cs, out.ptr, out_cs, _stream()))
    got = out.get().reshape(rows, out_cs)
    assert np.array_equal(d.get(np.float32).view(np.int32), x.astype(np.float32).reshape(-1).view(np.int32)), "input modified"
    return got


def _softmax_check(x, valid, out_cs, tag):
    got = _softmax(x, valid, out_cs)
    ref = R.softmax_ref(x, valid)
    err, bound = np.abs(R.widen(got[:, :valid]).astype(np.float64) - ref), R.softmax_bound(ref)
    assert (err <= bound).all(), tag + (_ratio(err, bound),)
    assert (got[:, valid:] == 0).all(), tag + ("pad columns are not zero bits",)      # K = keys_pad of the P.V GEMM reads them
    return _ratio(err, bound), got


@pytest.mark.parametrize("cs,valid,out_cs", R.SOFTMAX_CASES)
def test_softmax_rows_bf16_matches_float64(cs, valid, out_cs):
    """Row counts around the 4 rows of a workgroup, `valid` around the 64 lanes and at the 512-column limit, cs != out_cs, logit
    scales 1, 3 and 10; columns [valid, out_cs) are zero bits."""
    worst = 0.0
    rows_list = R.SOFTMAX_ROWS + ((R.SOFTMAX_BIG[1],) if (cs, valid, out_cs) == R.SOFTMAX_BIG[0] else ())
    for ri, rows in enumerate(rows_list):
        for si, scale in enumerate(R.SOFTMAX_SCALES):
            x = R.softmax_logits(cs * 7 + valid + 10 * ri + si, rows, cs, scale)
            ratio, _ = _softmax_check(x, valid, out_cs, (rows, cs, valid, out_cs, scale))
            worst = max(worst, ratio)
    print("softmax_rows_bf16 cs %d valid %d out_cs %d: worst err / bound = %.3f" % (cs, valid, out_cs, worst))
    _log("bf16_glue.softmax_rows", {"cs": cs, "valid": valid, "out_cs": out_cs, "worst_over_bound": worst})


@pytest.mark.parametrize("cs,valid,out_cs", [(384, 337, 384), (64, 63, 64), (128, 65, 72), (512, 512, 512), (600, 500, 512)])
def test_softmax_rows_bf16_known_values(cs, valid, out_cs):
    rows = 5
    rng = np.random.default_rng(cs + valid)
    one = int(R.bf16_bits(np.array([1.0]))[0])
    # valid = 1 -> exactly 1.0 (whatever the logit), zero bits behind it
    x = (rng.standard_normal((rows, cs)) * 50).astype(np.float32)
    got = _softmax(x, 1, out_cs)
    assert (got[:, 0] == one).all() and (got[:, 1:] == 0).all()
    # a constant row -> bf16(1 / valid) everywhere
    x = np.repeat((rng.standard_normal((rows, 1)) * 50).astype(np.float32), cs, axis=1)
    got = _softmax(x, valid, out_cs)
    assert (got[:, :valid] == R.bf16_bits(np.array([1.0 / valid]))[0]).all() and (got[:, valid:] == 0).all()
    # one -inf logit -> zero bits at that column, the rest still inside the bound
    x = (rng.standard_normal((rows, cs)) * 3).astype(np.float32)
    hole = rng.integers(0, valid, size=rows)
    x[np.arange(rows), hole] = -np.inf
    _, got = _softmax_check(x, valid, out_cs, (cs, valid, out_cs, "-inf"))
    assert (got[np.arange(rows), hole] == 0).all()
    # logits of spread 1e4: finite, non-negative probabilities (and still inside the bound)
    x = (rng.standard_normal((rows, cs)) * 1e4).astype(np.float32)
    _, got = _softmax_check(x, valid, out_cs, (cs, valid, out_cs, "1e4"))
    p = R.widen(got[:, :valid])
    assert np.isfinite(p).all() and (p >= 0).all() and (got[:, :valid] >> 15 == 0).all()


def test_softmax_rows_bf16_argument_checks():
    L = _hip.lib()
    d, out = Guarded(4 * 4 * 600), Guarded(2 * 4 * 520)
    for rows, valid, cs, out_cs in ((4, 65, 64, 72), (4, 65, 128, 64), (4, 500, 600, 520), (0, 8, 8, 8), (4, 0, 8, 8)):
        rc = L.m3d_softmax_rows_bf16(d.ptr, rows, valid, cs, out.ptr, out_cs, _stream())
        assert rc != 0 and b"softmax_rows_bf16" in L.m3d_last_error(), (rows, valid, cs, out_cs)
    assert out.untouched()


# ======================================================================================== 4. fp32 -> bf16
def _convert(pats):
    """uint32 fp32 bit patterns -> uint16 bf16 bit patterns."""
    L = _hip.lib()
    pats = np.ascontiguousarray(pats, dtype=np.uint32)
    src, dst = Guarded(4 * pats.size).put(pats), Guarded(2 * pats.size)
    _hip.check(L.m3d_f32_to_bf16(src.ptr, dst.ptr, pats.size, _stream()))
    got = dst.get()
    assert np.array_equal(src.get(np.uint32), pats), "input modified"
    return got


def _mismatch(pats, got, want):
    bad = np.nonzero(got != want)[0]
    return ["%08x -> %04x, want %04x" % (pats[i], got[i], want[i]) for i in bad[:8]], len(bad)


def test_f32_to_bf16_round_to_nearest_even_bits():
    """Bits against torch's CPU conversion: ties with an even and an odd upper half across the exponent range and both signs, the
    two neighbours of each tie, exact values, carries into the next binade and into inf; +-0, +-inf, +-FLT_MAX, the largest value that
    stays finite; 4096 random values."""
    g = torch.Generator().manual_seed(8)
    rnd = (torch.randn(4096, generator=g) * 100).numpy().view(np.uint32)
    for name, pats in (("ties", R.convert_patterns()), ("specials", R.CONVERT_SPECIALS), ("random", rnd)):
        got, want = _convert(pats), R.bf16_bits(pats.view(np.float32))
        assert np.array_equal(got, want), (name,) + _mismatch(pats, got, want)


def test_f32_to_bf16_subnormal_inputs_round_like_torch():
    """fp32 subnormals become bf16 subnormals (same exponent range), rounded to nearest even: no flush to zero."""
    pats = R.CONVERT_SUBNORMALS
    got, want = _convert(pats), R.bf16_bits(pats.view(np.float32))
    assert np.array_equal(got, want), _mismatch(pats, got, want)


def test_f32_to_bf16_nan_stays_nan():
    """Quiet and signalling NaN of several payloads, among them payloads in the low half only (rounding by adding 0x7FFF + lsb turns
    0x7F800001 into inf): NaN out.  Payload bits are not compared."""
    got = _convert(R.CONVERT_NANS)
    assert np.isnan(R.widen(got)).all(), ["%08x -> %04x" % (p, b) for p, b in zip(R.CONVERT_NANS, got)]


def test_f32_to_bf16_beyond_grid_cap():
    """n = 8192 * 256 * 8 + 8: the last 8 elements (ties, so that a copy without rounding shows) are converted in the second pass of
    the grid-stride loop."""
    L = _hip.lib()
    n = R.F32_TO_BF16_BIG
    assert n // 8 > R.F32_TO_BF16_CAP[0] * R.F32_TO_BF16_CAP[1]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, generator=g) * 100
    x[-8:] = torch.from_numpy(np.array([b for b, _ in R.convert_tie_table()[16:24]], np.uint32).view(np.float32).copy())
    src, dst = Guarded(4 * n).put_t(x.to(_dev())), Guarded(2 * n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _hip.check(L.m3d_f32_to_bf16(src.ptr, dst.ptr, n, _stream()))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    got, want = dst.get(), x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want), _mismatch(x.numpy().view(np.uint32), got, want)
    assert src.guards_ok()
    _log("bf16_glue.f32_to_bf16_big", {"n": n, "call_ms": ms})


def test_f32_to_bf16_argument_checks():
    L = _hip.lib()
    src, dst = Guarded(4 * 16), Guarded(2 * 16)
    for n in (0, 12, -8):
        assert L.m3d_f32_to_bf16(src.ptr, dst.ptr, n, _stream()) != 0 and b"f32_to_bf16" in L.m3d_last_error(), n
    assert dst.untouched()


# ======================================================================================== 5. stem
def _c3(v):
    return (ctypes.c_float * 3)(*[float(t) for t in v])


def _stem(image, is_u8, img_h, img_w, N, H, W, out_cs, seed):
    """image: float32 [N][3][H][W], or uint8 frames [N][img_h][img_w][3].  -> (uint16 [N][H][W][out_cs], w, scale, shift)."""
    L = _hip.lib()
    w, sc, sh = R.stem_params(seed)
    raw = np.ascontiguousarray(image).reshape(-1).view(np.uint8)
    raw = np.concatenate([raw, np.zeros(-raw.size % 4, np.uint8)])                    # whole words; the tail is never read
    dimg = Guarded(raw.size).put(raw)
    dw, dsc, dsh = Guarded(4 * 147 * 16).put(R.stem_pack_weight(w)), Guarded(4 * 16).put(sc), Guarded(4 * 16).put(sh)
    out = Guarded(2 * N * H * W * out_cs)
    _hip.check(L.m3d_stem_conv7x7_bf16(dimg.ptr, is_u8, img_h, img_w, _c3(R.STEM_MEAN) if is_u8 else None, _c3(R.STEM_STDS) if is_u8 else None,
                                       dw.ptr, dsc.ptr, dsh.ptr, out.ptr, out_cs, N, H, W, _stream()))
    got = out.get().reshape(N, H, W, out_cs)
    assert dimg.guards_ok() and dw.guards_ok() and dsc.guards_ok() and dsh.guards_ok()
    assert np.array_equal(got[..., 16:], _sent16(got.shape)[..., 16:]), "pad channels written"
    return got, w, sc, sh


def _stem_check(got, img32, w, sc, sh, tag):
    ref, T = R.stem_ref(img32, w, sc, sh)
    err, bound = np.abs(R.widen(got[..., :16]).astype(np.float64) - ref), R.stem_bound(ref, T)
    assert (err <= bound).all(), tag + (_ratio(err, bound), int((err > bound).sum()))
    return _ratio(err, bound)


@pytest.mark.parametrize("N,H,W,out_cs", R.STEM_F32_CASES)
def test_stem_bf16_f32_image_matches_float64(N, H, W, out_cs):
    """One pixel, ragged tiles of the 8 x 32 tiling in both directions, exact tiles, an interior tile without image border (24 x 96),
    N = 3, out_cs > 16 (pad channels keep the sentinel)."""
    img = np.random.default_rng(H * 100 + W).standard_normal((N, 3, H, W)).astype(np.float32)
    got, w, sc, sh = _stem(img, 0, 0, 0, N, H, W, out_cs, H + W)
    ratio = _stem_check(got, img, w, sc, sh, (N, H, W, out_cs))
    print("stem_bf16 fp32 image %s: worst err / bound = %.3f" % ((N, H, W, out_cs), ratio))
    _log("bf16_glue.stem_f32", {"case": [N, H, W, out_cs], "worst_over_bound": ratio})


@pytest.mark.parametrize("N,H,W,img_h,img_w,fill", [c + ("random",) for c in R.STEM_U8_CASES] +
                         [R.STEM_U8_CONSTANT_CASE + (f,) for f in R.STEM_U8_FILLS if f != "random"])
def test_stem_bf16_u8_frames_match_float64(N, H, W, img_h, img_w, fill):
    """uint8 BGR frames with Preprocess in the loads: a frame equal to the crop, smaller in both directions (the border value
    (0 - mean) / std, not 0), a one-pixel frame, the frame edge inside the patch of an interior tile, a frame one pixel short of the
    crop; frames of all 0 and all 255."""
    frames = R.stem_frames(H + W + img_h, N, img_h, img_w, fill)
    got, w, sc, sh = _stem(frames, 1, img_h, img_w, N, H, W, 16 if fill == "random" else 24, H + img_w)
    img = R.stem_normalise_u8(frames, H, W)
    ratio = _stem_check(got, img, w, sc, sh, (N, H, W, img_h, img_w, fill))
    print("stem_bf16 uint8 frames %s: worst err / bound = %.3f" % ((N, H, W, img_h, img_w, fill), ratio))
    _log("bf16_glue.stem_u8", {"case": [N, H, W, img_h, img_w, fill], "worst_over_bound": ratio})


def test_stem_bf16_argument_checks():
    L = _hip.lib()
    N, H, W = 1, 8, 32
    dimg, dw, dsc, dsh = Guarded(4 * N * 3 * H * W), Guarded(4 * 147 * 16), Guarded(4 * 16), Guarded(4 * 16)
    out = Guarded(2 * N * H * W * 24)
    mean, stds, zero = _c3(R.STEM_MEAN), _c3(R.STEM_STDS), _c3((0.225, 0.0, 0.229))
    bad = [
        (0, 0, 0, None, None, 8), (0, 0, 0, None, None, 20),                          # out_cs below 16 / not a multiple of 8
        (1, H + 1, W, mean, stds, 16), (1, H, W + 1, mean, stds, 16),                 # frame larger than the crop
        (1, 0, W, mean, stds, 16), (1, H, W, mean, zero, 16),                         # empty frame; a zero std
        (1, H, W, None, stds, 16), (1, H, W, mean, None, 16),                         # uint8 input without its normalisation
    ]
    for is_u8, ih, iw, m, s, out_cs in bad:
        rc = L.m3d_stem_conv7x7_bf16(dimg.ptr, is_u8, ih, iw, m, s, dw.ptr, dsc.ptr, dsh.ptr, out.ptr, out_cs, N, H, W, _stream())
        assert rc != 0 and b"stem_bf16" in L.m3d_last_error(), (is_u8, ih, iw, out_cs)
    assert out.untouched()
