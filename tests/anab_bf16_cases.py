"""Cases, operands and yardsticks of the bf16 ANAB attention operator (m3d_anab_attention_forward_bf16 / _backward_bf16), shared by
tests/test_anab_bf16_host.py and tests/test_gpu_anab_bf16.py.

Error measure: err = max|got - ref64| / max|ref64| per tensor, and per column (= per scale) for grad_gates; ref64 is
anab_train_ref.core_grads in float64 on the CPU on the operands after their rounding to bf16.

Exact operands (``exact_case``): a 16x16 map (windows nest, areas are powers of two) with operands on a dyadic lattice for which
none of the operator's rounding points rounds, so forward and gradients must equal the float64 reference rounded once to bf16.
  k   channels 0..127: the first-order Reed-Muller codeword of the pixel index, +-1 (256 codewords of length 128: two of them are
      orthogonal or antipodal).  A query 32 * code(p) has the logit 128 * 32 * g at the fine key of p and at most a quarter of that
      at any other key, whatever the gates.  Channels 128..131 mark regions (+1 inside, -1 outside): N = two 4x4 blocks A and B
      (sign flipped: -1 inside), block A, and two 2x2 windows T1, T2 of B; a query 4096 on one of them aims at key 0 (logit
      0.75 * 4096 against at most half), at the scale-4 bin A, at the scale-8 bins T1 / T2 (1 against 1/2).  A pooled bin is a mean
      of its sub-bins, so a coarse bin wins only through its gate: its own gate is 1 and the gates of the bins below it are 1/2.
      Block B lies in block row 1 or 2, so T1 / T2 are keys of the second key tile; the fine keys fill tiles 2..10.
      Channels from 132 on: +-1 (they meet zeros of the queries).
  g   {1/2, 1}, constant inside the window of its scale: scale 1: 1; scale 4: 1 on A; scale 8: 1 on T1, T2; scale 16: 1 on the
      pixels of B outside T1, T2; else 1/2.  khat / vhat = gate * (sum of +-1) / area: at most 8 significant bits.
  v   +-1.  grad_out +-1, on two-hot rows in 8 channels only (zeros elsewhere).
  q   one-hot rows (one target) and two-hot rows: 32 * (code(a) + code(b)) for fine keys a, b with orthogonal codes, equal gates
      and different 2x2 windows: both logits 128 * 32 * g, the rest at least 1024 below; P = 1/2, 1/2 and
      dS = +-(dP_a - dP_b) / 4 with |dP_a - dP_b| <= 16 in steps of 1/2: 6 bits.
Every gap between the top logits and the rest is >= 1024: exp(S - max) is 0 or 1 in float32 and in float64."""
import torch

import anab_train_ref as R
import exact_inputs as X

BF16 = torch.bfloat16
F64 = torch.float64
NAMES = ("out", "grad_q", "grad_k", "grad_v", "grad_gates")

# (B, H, W, Ck, Cv)
CASES = [(2, 8, 16, 168, 128),      # two bins per pixel at scale 16
         (1, 16, 16, 64, 128),      # nested windows
         (1, 12, 32, 128, 128),     # uneven windows
         (1, 8, 16, 168, 256),      # value-channel split
         (2, 16, 72, 168, 128),     # B > 1 with three pixel chunks, the last one ragged
         (2, 16, 40, 168, 256),
         (1, 32, 4, 168, 128),      # W < 8
         (1, 128, 1, 168, 128)]     # W = 1
IDS = ["%dx%dx%d_ck%d_cv%d" % c for c in CASES]
CONTRACT = [4, 5]
EXACT_SHAPES = [(2, 16, 16, 168, 128), (1, 16, 16, 168, 256)]
RATIO = 1.5                         # err_op <= RATIO * err_t16 (derivation: docs/LAB_NOTES.md)
GUARD = 7.25


def bf(t):
    """Rounded to bf16, kept as float32."""
    return t.to(BF16).float()


def layout(Ck, Cv):
    """Column offsets of q | k | v | gates in the wide bf16 matrix and its width: q at a multiple of 8 elements (16-byte loads),
    k, v, gates at even offsets that are no multiple of 8, row stride a multiple of 8."""
    oq = 8
    ok = oq + Ck + 2
    ov = ok + Ck + 2
    og = ov + Cv + 2
    return ((oq, Ck), (ok, Ck), (ov, Cv), (og, 4)), (og + 4 + 2 + 7) // 8 * 8


def embed(ts, go):
    """[q, k, v, g] and grad_out (float32 holding bf16 values) -> (wide bf16, views, gwide bf16): column slices of wider matrices
    whose other columns hold 1e30."""
    Ck, Cv = ts[0].shape[1], ts[2].shape[1]
    views, width = layout(Ck, Cv)
    wide = torch.full((ts[0].shape[0], width), 1e30)
    for (o, c), t in zip(views, ts):
        wide[:, o:o + c] = t
    gwide = torch.full((go.shape[0], Cv + 16), 1e30)
    gwide[:, 8:8 + Cv] = go
    return wide.to(BF16), views, gwide.to(BF16)


def random_case(i):
    """Case ``i``: the inputs of anab_train_ref.make_core_case rounded to bf16 -> ([q, k, v, g], grad_out) as float32."""
    B, H, W, Ck, Cv = CASES[i]
    wide, views, gwide = R.make_core_case(B, H, W, Ck, Cv, seed=400 + i)
    return [bf(wide[:, o:o + c]) for o, c in views], bf(gwide[:, 4:4 + Cv])


def err(got, ref):
    return ((got.detach().double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max()).item()


def errs_of(got, ref64):
    """{name: err} per tensor plus grad_gates_s0 .. _s3 per gate column."""
    out = {n: err(g, r) for n, g, r in zip(NAMES, got, ref64)}
    for s in range(4):
        out["grad_gates_s%d" % s] = err(got[4][:, s], ref64[4][:, s])
    return out


def check_bound(e_op, e_ref, what=""):
    for name in e_op:
        assert e_op[name] <= RATIO * e_ref[name], "%s%s: err %.3e > %.1f * %.3e" % (what, name, e_op[name], RATIO, e_ref[name])


def run(L, stream, dev, dims, wide, views, gwide, needs=(True, True, True, True), fill=None, ws_fill=None, forward=True, img=None,
        out_off=4, canary=4096):
    """The C ABI on strided views: outputs are slices (columns out_off .. out_off + C) of wider bf16 matrices pre-filled with GUARD
    (or poisoned with ``fill``); the workspace has exactly the size the library asks for, is poisoned with ``fill`` / ``ws_fill``, and
    ``canary`` bytes behind it hold a pattern that must stand.  ``img``: that image alone (B = 1, pointers moved to its rows).
    Returns [out, grad_q, grad_k, grad_v, grad_gates] as the WIDE matrices."""
    import poison
    from m3dssd_amd import _hip
    B, H, W, Ck, Cv = dims
    row0 = 0
    if img is not None:
        row0, B = img * H * W, 1
    n = B * H * W
    cs = wide.stride(0)
    ptr = [wide.data_ptr() + 2 * (row0 * cs + o) for o, _ in views]
    go_ptr = gwide.data_ptr() + 2 * (row0 * gwide.stride(0) + 8)
    pattern = (torch.arange(canary, device=dev) % 251).to(torch.uint8)

    def fresh(c):
        t = torch.full((n, c + 8), GUARD, device=dev, dtype=BF16)
        if fill is not None:
            poison.poison_(t, fill)
        return t

    def workspace(backward):
        nbytes = L.m3d_anab_attention_workspace_bytes_bf16(B, H, W, Ck, Cv, backward)
        assert nbytes > 0
        ws = torch.zeros(nbytes + 256 + canary, device=dev, dtype=torch.uint8)
        if (fill or ws_fill) is not None:
            ws.fill_({"nan": 0xFF, "huge": 0x7F}[fill or ws_fill])
        base = (ws.data_ptr() + 255) // 256 * 256
        end = base - ws.data_ptr() + nbytes
        ws[end:end + canary] = pattern
        return ws, base, nbytes, end

    res = [None] * 5
    if forward:
        res[0] = fresh(Cv)
        ws, base, nbytes, end = workspace(0)
        _hip.check(L.m3d_anab_attention_forward_bf16(*ptr, res[0].data_ptr() + 2 * out_off, B, H, W, Ck, Cv, cs, cs, cs, cs,
                                                     res[0].stride(0), base, nbytes, stream))
        assert torch.equal(ws[end:end + canary], pattern), "the forward wrote behind the workspace size it asks for"
    for j, c in enumerate((Ck, Ck, Cv, 4)):
        if needs[j]:
            res[1 + j] = fresh(c)
    ws, base, nbytes, end = workspace(1)
    gp = [t.data_ptr() + 2 * out_off if t is not None else None for t in res[1:]]
    gcs = [t.stride(0) if t is not None else 0 for t in res[1:]]
    _hip.check(L.m3d_anab_attention_backward_bf16(*ptr, go_ptr, *gp, B, H, W, Ck, Cv, cs, cs, cs, cs, gwide.stride(0), *gcs, base,
                                                  nbytes, stream))
    torch.cuda.synchronize()
    assert torch.equal(ws[end:end + canary], pattern), "the backward wrote behind the workspace size it asks for"
    return res


# ------------------------------------------------------------------------------------ exact operands
GAIN_FINE, GAIN_COARSE = 32.0, 4096.0
N_CODE = 128


def _codes():
    """[256, 128]: codeword of pixel index p = (-1)^(a0 + <a, i>), a0 = bit 7 of p, a = bits 0..6."""
    p = torch.arange(256).view(-1, 1)
    i = torch.arange(N_CODE).view(1, -1)
    par = torch.zeros(256, N_CODE, dtype=torch.long)
    for b in range(7):
        par += ((p >> b) & 1) * ((i >> b) & 1)
    par += (p >> 7) & 1
    return (1 - 2 * (par & 1)).to(F64)


def _exact_image(g, Ck, Cv):
    """One 16x16 image: q, k, v, gates, grad_out (float64) and the target keys of its rows [256, 2] (second entry -1: one-hot)."""
    H = W = 16
    pix = torch.arange(256)
    yy, xx = pix // W, pix % W
    blk = (yy // 4) * 4 + xx // 4                                   # scale-4 bin of a pixel
    win = (yy // 2) * 8 + xx // 2                                   # scale-8 bin
    bB = int(torch.randint(4, 12, (1,), generator=g))              # block row 1 or 2
    bA = int([b for b in torch.randperm(16, generator=g).tolist() if b != bB][0])
    wins_B = torch.unique(win[blk == bB])
    T1, T2 = (int(w) for w in wins_B[torch.randperm(4, generator=g)[:2]])
    inA, inB, inT1, inT2 = blk == bA, blk == bB, win == T1, win == T2
    pm = lambda m: m.to(F64) * 2 - 1                                # noqa: E731
    k = X._pick(g, [-1.0, 1.0], (256, Ck))
    k[:, :N_CODE] = _codes()
    k[:, N_CODE + 0] = -pm(inA | inB)
    k[:, N_CODE + 1] = pm(inA)
    k[:, N_CODE + 2] = pm(inT1)
    k[:, N_CODE + 3] = pm(inT2)
    gates = torch.full((256, 4), 0.5, dtype=F64)
    gates[:, 0] = 1.0
    gates[inA, 1] = 1.0
    gates[inT1 | inT2, 2] = 1.0
    gates[inB & ~inT1 & ~inT2, 3] = 1.0
    v = X._pick(g, [-1.0, 1.0], (256, Cv))
    go = X._pick(g, [-1.0, 1.0], (256, Cv))
    # targets: rows 0..3 aim at key 0, bin A, T1, T2; every fourth row after them is two-hot; the rest one-hot on a fine key; the
    # first targets of rows 4..255 are 252 different fine keys (a permutation), so every key tile from the third on is hit
    q = torch.zeros(256, Ck, dtype=F64)
    target = torch.full((256, 2), -1, dtype=torch.long)
    coarse = (0, 1 + bA, 17 + T1, 17 + T2)
    for r, key in enumerate(coarse):
        q[r, N_CODE + r] = GAIN_COARSE
        target[r, 0] = key
    code = _codes()
    perm = torch.randperm(256, generator=g)
    nxt = 0
    for r in range(4, 256):
        a = int(perm[nxt % 256])
        nxt += 1
        if r % 4 == 0:
            # partner: orthogonal code (not a, not its antipode a ^ 128), the same fine gate, another 2x2 window
            ok = (gates[:, 3] == gates[a, 3]) & (win != win[a]) & (pix != a) & (pix != (a ^ 128))
            cand = pix[ok]
            b = int(cand[int(torch.randint(0, cand.numel(), (1,), generator=g))])
            q[r, :N_CODE] = GAIN_FINE * (code[a] + code[b])
            target[r] = torch.tensor([81 + a, 81 + b])
            keep = torch.randperm(Cv, generator=g)[:8]
            row = torch.zeros(Cv, dtype=F64)
            row[keep] = go[r, keep]
            go[r] = row
        else:
            q[r, :N_CODE] = GAIN_FINE * code[a]
            target[r, 0] = 81 + a
    return q, k, v, gates, go, target


def exact_case(B, Ck, Cv, seed):
    """([q, k, v, g], grad_out, target [B*256, 2]) as float32 / long for a 16x16 map; every value is a bf16 number."""
    g = X._gen(seed)
    parts = [_exact_image(g, Ck, Cv) for _ in range(B)]
    cat = lambda j: torch.cat([p[j] for p in parts], 0)            # noqa: E731
    ts = [cat(j).float() for j in range(4)]
    for t in ts:
        assert torch.equal(bf(t), t)
    return ts, cat(4).float(), cat(5)


def _pool_matrix(H, W):
    """w [337, H*W] float64: w_b(p) = [p in win_b] / area_b, and the scale index of every bin."""
    rows, scale = [], []
    for si, s in enumerate(R.PSP):
        for i in range(s):
            for j in range(s):
                h0, h1 = (i * H) // s, ((i + 1) * H + s - 1) // s
                w0, w1 = (j * W) // s, ((j + 1) * W + s - 1) // s
                m = torch.zeros(H, W, dtype=F64)
                m[h0:h1, w0:w1] = 1.0 / ((h1 - h0) * (w1 - w0))
                rows.append(m.flatten())
                scale.append(si)
    return torch.stack(rows), torch.tensor(scale)


def emulate(ops, rnd=X.EXACT):
    """The operator from its definition in float64 with the rounding points of include/m3dssd_hip.h inserted through ``rnd``
    (exact_inputs.Rounding: ``narrow`` = a bf16 MFMA operand, ``matmul`` = an fp32 accumulation in a scrambled order):
    [out | grad_q | grad_k | grad_v | grad_gates] side by side, [B*HW, Cv + 2 Ck + Cv + 4], BEFORE the one rounding of each output
    to bf16 (assert_exact_under also asserts that these are fp32 numbers)."""
    (q, k, v, g), go, (B, H, W) = [t.to(F64) for t in ops["ts"]], ops["go"].to(F64), ops["dims"]
    hw = H * W
    wp, scale = _pool_matrix(H, W)
    outs = []
    for b in range(B):
        sl = slice(b * hw, (b + 1) * hw)
        qb, kb, vb, gb, gob = q[sl], k[sl], v[sl], g[sl], go[sl]
        gsel = gb[:, scale].t()                                     # [337, hw]: the gate of the bin's scale at every pixel
        wg = wp * gsel
        khat, vhat = rnd.narrow(rnd.matmul(wg, kb)), rnd.narrow(rnd.matmul(wg, vb))
        S = rnd.matmul(qb, khat.t().contiguous())
        e = torch.exp((S - S.max(-1, keepdim=True)[0]).to(torch.float32)).to(F64)
        l = e.sum(-1, keepdim=True)
        out = rnd.matmul(rnd.narrow(e), vhat) / l
        P = e / l
        dP = rnd.matmul(gob, vhat.t().contiguous())
        D = (e * dP).sum(-1, keepdim=True) / l
        dS = rnd.narrow(P * (dP - D))
        dq = rnd.matmul(dS, khat)
        dkhat = rnd.matmul(dS.t().contiguous(), qb)
        dvhat = rnd.matmul(rnd.narrow(P).t().contiguous(), gob)
        dk = rnd.matmul(wg.t().contiguous(), dkhat)
        dv = rnd.matmul(wg.t().contiguous(), dvhat)
        per_bin = rnd.matmul(kb, dkhat.t().contiguous()) + rnd.matmul(vb, dvhat.t().contiguous())      # [hw, 337]
        dg = torch.stack([(per_bin * wp.t() * (scale == s).to(F64)).sum(-1) for s in range(4)], -1)
        outs.append(torch.cat([out, dq, dk, dv, dg], 1))
    return torch.cat(outs, 0)


def split(flat, Ck, Cv):
    return list(torch.split(flat, [Cv, Ck, Ck, Cv, 4], dim=1))
