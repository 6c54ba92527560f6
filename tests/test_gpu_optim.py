"""GPU tests (-m gpu) of the fused optimizer step (csrc/optim.hip, m3dssd_amd/host/optim.py): bit for bit against the float32
numpy restatement tests/optim_ref.py over a table of awkward tensor sizes and alignments, the device-side step decision,
zero_grads, checkpoints to and from torch.optim, three iterations on the model, and the error paths of the C ABI.

Values are normal float32; denormals are outside the contract.  Where a NaN / inf is planted, NaN compares equal to NaN whatever
its payload (optim_ref.same_bits)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import optim_ref as R
from gpu_common import _dev
from m3dssd_amd import _hip
from m3dssd_amd.host import optim as O

pytestmark = pytest.mark.gpu

CHUNK = _hip.CONSTANTS["M3D_OPTIM_CHUNK"]
SENT = -559038737          # 0xDEADBEEF as int32
GUARD = 64                 # 4-byte elements between two tensors (a multiple of 4: alignment is decided by `odd` alone)
FUSED = {R.SGD: O.SGD, R.ADAM: O.Adam, R.ADAMAX: O.Adamax}
TORCH = {R.SGD: torch.optim.SGD, R.ADAM: torch.optim.Adam, R.ADAMAX: torch.optim.Adamax}
KINDS = [R.SGD, R.ADAM, R.ADAMAX]
IDS = ["sgd", "adam", "adamax"]


class Arena:
    """One sentinel-filled device buffer; tensors are carved out of it with GUARD sentinels between them, 16-byte aligned unless
    ``odd`` (then at an odd element offset: 4-byte aligned only)."""

    def __init__(self, n_total):
        self.raw = torch.full((n_total,), SENT, dtype=torch.int32, device=_dev())
        assert self.raw.data_ptr() % 16 == 0
        self.at = GUARD
        self.spans = []

    def carve(self, n, odd=False):
        start = (self.at + 3) // 4 * 4 + (1 if odd else 0)
        assert start + n + GUARD <= self.raw.numel()
        self.at = start + n + GUARD
        self.spans.append((start, n))
        t = self.raw[start:start + n].view(torch.float32)
        assert (t.data_ptr() % 16 != 0) == bool(odd)
        return t

    def host(self):
        return self.raw.cpu().numpy()

    def check_guards(self, host):
        mask = np.ones(host.shape, dtype=bool)
        for s, n in self.spans:
            mask[s:s + n] = False
        assert (host[mask] == SENT).all(), "a write outside the tensors"


class Table:
    """The parameter set of the bit-for-bit tests: group 0 = the sizes of optim_ref.table_sizes, a misaligned parameter, a
    parameter with a misaligned gradient, one parameter whose grad is None and one with requires_grad=False; group 1 = 300 tensors
    of 7 elements.  Host copies mirror every tensor for the restatement."""

    def __init__(self, seed, small=False):
        self.rng = np.random.default_rng(seed)
        sizes = [5, 1025, CHUNK + 1] if small else R.table_sizes(CHUNK)
        plan = [(n, False, False, True) for n in sizes] + [(1029, True, False, True), (1030, False, True, True), (37, False, False, False)]
        plan = [plan, [(7, False, False, True)] * (3 if small else 300)]
        self.arena = Arena(sum(2 * (n + GUARD + 8) for g in plan for n, _, _, _ in g) + 4 * GUARD + 64)
        self.params, self.grads, self.h_params = [], [], []
        for g in plan:
            ps, gs, hs = [], [], []
            for n, odd_p, odd_g, has_grad in g:
                p = torch.nn.Parameter(self.arena.carve(n, odd_p))
                hp = R.values(self.rng, n, 0.5)
                p.data.copy_(torch.from_numpy(hp))
                if has_grad:
                    p.grad = self.arena.carve(n, odd_g)
                ps.append(p); gs.append(p.grad); hs.append(hp)
            self.params.append(ps); self.grads.append(gs); self.h_params.append(hs)
        frozen = torch.nn.Parameter(self.arena.carve(19), requires_grad=False)
        self.h_frozen = R.values(self.rng, 19, 0.5)
        frozen.data.copy_(torch.from_numpy(self.h_frozen))
        self.params[0].append(frozen); self.grads[0].append(None); self.h_params[0].append(self.h_frozen.copy())

    def new_grads(self, scale=0.1):
        """Fresh gradient values on the device and, returned, on the host (None where the parameter has no gradient)."""
        out = []
        for gs in self.grads:
            hs = []
            for g in gs:
                if g is None:
                    hs.append(None)
                    continue
                h = R.values(self.rng, g.numel(), scale)
                g.copy_(torch.from_numpy(h))
                hs.append(h)
            out.append(hs)
        return out

    def device_values(self):
        """(params, grads) as the device holds them, per group, from ONE download; the guards are checked on the way."""
        host = self.arena.host()
        self.arena.check_guards(host)
        base = self.arena.raw.data_ptr()

        def pick(t):
            if t is None:
                return None
            s = (t.data_ptr() - base) // 4
            return host[s:s + t.numel()].view(np.float32).copy()
        return [[pick(p) for p in ps] for ps in self.params], [[pick(g) for g in gs] for gs in self.grads]

    def groups(self, kind):
        mom = 0.9 if kind == R.SGD else 0.0
        return [R.group(0.01, momentum=mom, weight_decay=5e-4), R.group(0.003, momentum=mom, weight_decay=1e-3)]

    def optimizer(self, kind, groups=None):
        groups = groups or self.groups(kind)
        return FUSED[kind]([dict(params=ps, lr=g["lr"], weight_decay=g["weight_decay"], **(dict(momentum=g["momentum"]) if kind == R.SGD else {}))
                            for ps, g in zip(self.params, groups)])


def states_of(opt, table, kind):
    """{(gi, pi): [state arrays]} from ONE download of the flat state allocation; everything outside the views must still be zero."""
    flat = opt._flat.cpu().numpy()
    used = np.zeros(flat.shape, dtype=bool)
    out = {}
    for gi, ps in enumerate(table.params):
        for pi, p in enumerate(ps):
            st = opt.state.get(p, {})
            arr = []
            for name in R.STATE_KEYS[kind]:
                if name in st and p.numel() == 0:                  # (an empty view has no address)
                    arr.append(np.zeros(0, dtype=np.float32))
                elif name in st:
                    s = (st[name].data_ptr() - opt._flat.data_ptr()) // 4
                    assert st[name].data_ptr() % 16 == 0 and 0 <= s and s + p.numel() <= flat.size
                    used[s:s + p.numel()] = True
                    arr.append(flat[s:s + p.numel()].copy())
            if arr:
                out[(gi, pi)] = arr
    assert (flat[~used] == 0).all(), "a write into the padding of the state allocation"
    return out


def assert_matches(table, opt, ref, kind, what):
    dp, _ = table.device_values()
    for gi, ps in enumerate(dp):
        for pi, p in enumerate(ps):
            assert R.same_bits(p, table.h_params[gi][pi]), "%s: parameter %d of group %d (numel %d)" % (what, pi, gi, p.size)
    got = states_of(opt, table, kind)
    assert got.keys() == {k for k in ref.state if kind != R.SGD or ref.groups[k[0]]["momentum"] != 0}, what
    for key, arr in got.items():
        for k, a in enumerate(arr):
            assert R.same_bits(a, ref.state[key][k].reshape(-1)), "%s: %s of parameter %s" % (what, R.STATE_KEYS[kind][k], key)


# ------------------------------------------------------------------------------------ 1. bit for bit against the restatement
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_five_steps_equal_the_restatement_bit_for_bit(kind):
    table = Table(100 + kind)
    opt = table.optimizer(kind)
    ref = R.Ref(kind, table.groups(kind), np.float32)
    zero_loss = torch.zeros((), device=_dev())
    for step in range(5):
        if step:                                                    # as adjust_lr does between iterations
            for g, h in zip(opt.param_groups, ref.groups):
                g["lr"] = h["lr"] = h["lr"] * (0.7 + 0.1 * step)
        h_grads = table.new_grads()
        zero = step % 2 == 1
        opt.step(loss=zero_loss)                                    # prepare alone decides "no step": the sum, and nothing else
        assert not opt.last_step_taken()
        first = opt.grad_sq_sum.cpu().numpy().tobytes()
        opt.step(zero_grads=zero)
        sq, bad, go = ref.step(table.h_params, h_grads)
        assert go and opt.last_step_taken() and int(opt.grad_nonfinite) == bad == 0
        got = float(opt.grad_sq_sum)
        assert opt.grad_sq_sum.cpu().numpy().tobytes() == first, "grad_sq_sum differs between two launches"
        assert abs(got - sq) <= 1e-12 * sq, (got, sq)
        assert_matches(table, opt, ref, kind, "step %d" % step)
        _, dg = table.device_values()
        for gs, hs in zip(dg, h_grads):
            for g, h in zip(gs, hs):
                if g is not None:
                    assert R.same_bits(g, np.zeros_like(h) if zero else h), "gradients after zero_grads=%s" % zero
    assert opt.step_count() == 5
    # the two parameters without a gradient were never in the table
    assert all(p not in opt.state for p in table.params[0][-2:])
    assert np.array_equal(table.h_params[0][-1], table.h_frozen)


def test_momentum_zero_uses_no_buffer():
    table = Table(7, small=True)
    groups = [R.group(0.01, momentum=0.0, weight_decay=5e-4), R.group(0.003, momentum=0.9)]
    opt = table.optimizer(R.SGD, groups)
    ref = R.Ref(R.SGD, groups, np.float32)
    for step in range(2):
        ref.step(table.h_params, table.new_grads())
        opt.step()
        assert_matches(table, opt, ref, R.SGD, "step %d" % step)
    assert all(p not in opt.state for p in table.params[0]) and all("momentum_buffer" in opt.state[p] for p in table.params[1])


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_the_table_follows_the_gradients(kind):
    """A gradient tensor replaced by a new allocation (zero_grad(set_to_none=True) and a backward) moves a pointer of the table
    and nothing else; a parameter that gets its first gradient later joins with zero state and keeps everybody else's."""
    table = Table(400 + kind, small=True)
    opt = table.optimizer(kind)
    ref = R.Ref(kind, table.groups(kind), np.float32)

    def one(what):
        ref.step(table.h_params, table.new_grads())
        opt.step()
        assert_matches(table, opt, ref, kind, what)

    one("first step")
    flat, block = opt._flat.data_ptr(), opt._block.data_ptr()
    for gi, pi in ((0, 0), (1, 1)):
        p = table.params[gi][pi]
        p.grad = table.grads[gi][pi] = table.arena.carve(p.numel(), odd=gi == 1)
    one("after two gradients moved")
    assert (opt._flat.data_ptr(), opt._block.data_ptr()) == (flat, block), "the state was reallocated for a moved gradient"
    late = table.params[0][-2]
    assert late.grad is None and late not in opt.state
    late.grad = table.grads[0][-2] = table.arena.carve(late.numel())
    one("after a parameter joined")
    one("one more step")
    assert opt._flat.data_ptr() != flat and late in opt.state and opt.step_count() == 4


# ------------------------------------------------------------------------------------ 2. the decision
def _snapshot(table, opt):
    return table.arena.host().tobytes(), opt._flat.cpu().numpy().tobytes(), opt._block[_hip.CONSTANTS["M3D_OPTIM_STATE_T"]:O.HEAD_BYTES].cpu().numpy().tobytes()


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_the_step_decision_is_taken_on_the_device(kind):
    table = Table(200 + kind, small=True)
    opt = table.optimizer(kind)
    ref = R.Ref(kind, table.groups(kind), np.float32)
    ref.step(table.h_params, table.new_grads())
    opt.step()
    assert_matches(table, opt, ref, kind, "first step")
    cases = [(1.0, None, False), (0.0, None, False), (-1.0, None, False), (float("nan"), None, False), (float("inf"), None, False),
             (None, None, False), (None, float("nan"), True), (None, float("inf"), True), (None, float("nan"), False),
             (None, float("inf"), False), (1.0, float("nan"), True), (0.0, float("inf"), False)]
    for loss, planted, skip in cases:
        what = "loss %s, planted %s, skip_nonfinite %s" % (loss, planted, skip)
        h_grads = table.new_grads()
        if planted is not None:
            for gi, pi, at in ((0, 1, 1024), (1, 2, 3)):           # the tail of a 1025-element tensor, and a 7-element one
                h_grads[gi][pi][at] = planted
                table.grads[gi][pi][at] = planted
        dev_loss = None if loss is None else torch.tensor(loss, device=_dev(), dtype=torch.float32)
        before = _snapshot(table, opt)
        t_before = opt.step_count()
        opt.step(loss=dev_loss, skip_nonfinite=skip, zero_grads=True)
        sq, bad, go = ref.step(table.h_params, h_grads, loss=loss, skip_nonfinite=skip, zero_grads=True)
        assert go == ((loss is None or loss > 0) and not (skip and planted is not None)), what
        assert int(opt.stepped) == int(go) and opt.last_step_taken() == go and int(opt.grad_nonfinite) == bad == (0 if planted is None else 2), what
        if planted is None:
            assert abs(float(opt.grad_sq_sum) - sq) <= 1e-12 * sq, what
        if go:
            assert opt.step_count() == t_before + 1 == ref.t, what
            assert_matches(table, opt, ref, kind, what)
            _, dg = table.device_values()
            assert all((g == 0).all() for gs in dg for g in gs if g is not None), what
        else:
            # parameters, gradients (zero_grads was asked for), guards, state, step counter, running products: the same bytes
            assert _snapshot(table, opt) == before and opt.step_count() == t_before, what
            if planted is not None:                                 # put finite gradients back for the next case
                table.new_grads()


# ------------------------------------------------------------------------------------ 3. zero_grads
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_zero_grads_changes_nothing_but_the_gradients(kind):
    a, b = Table(300, small=True), Table(300, small=True)
    oa, ob = a.optimizer(kind), b.optimizer(kind)
    for _ in range(2):
        ga, gb = a.new_grads(), b.new_grads()
        oa.step(zero_grads=False)
        ob.step(zero_grads=True)
        pa, da = a.device_values()
        pb, db = b.device_values()
        for x, y in zip([p for ps in pa for p in ps], [p for ps in pb for p in ps]):
            assert R.same_bits(x, y)
        for x, y, h in zip([g for gs in da for g in gs], [g for gs in db for g in gs], [g for gs in ga for g in gs]):
            if x is not None:
                assert R.same_bits(x, h) and (y == 0).all() and np.signbit(y).sum() == 0
        assert oa._flat.cpu().numpy().tobytes() == ob._flat.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------ 4. checkpoints
def _host_case_on_device():
    params, grads = R.host_case()
    dev = _dev()
    ps = [[torch.nn.Parameter(torch.from_numpy(p.copy()).to(dev)) for p in pp] for pp in params]
    return ps, grads


def _set_grads(ps, gs):
    for pp, gg in zip(ps, gs):
        for p, g in zip(pp, gg):
            if g is None:
                p.grad = None
            elif p.grad is None:
                p.grad = torch.from_numpy(g).to(p.device)
            else:
                p.grad.copy_(torch.from_numpy(g))


def _make(cls, kind, ps):
    return cls([dict(params=pp, lr=g["lr"], weight_decay=g["weight_decay"], **(dict(momentum=g["momentum"]) if kind == R.SGD else {}))
                for pp, g in zip(ps, R.HOST_GROUPS[kind])])


def _clone(ps):
    return [[torch.nn.Parameter(p.detach().clone()) for p in pp] for pp in ps]


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
@pytest.mark.parametrize("direction", ["fused_to_torch", "torch_to_fused"])
def test_checkpoints_go_both_ways(kind, direction):
    """3 steps with one class, its state_dict into the other class on copies, 2 more steps on each: parameters and state agree
    within optim_ref.BOUND_F32_VS_F64 (4x the float32-against-float64 error tests/test_optim_host.py measures on this case)."""
    ps, grads = _host_case_on_device()
    first, second = (FUSED[kind], TORCH[kind]) if direction == "fused_to_torch" else (TORCH[kind], FUSED[kind])
    oa = _make(first, kind, ps)
    for gs in grads[:3]:
        _set_grads(ps, gs)
        oa.step()
    qs = _clone(ps)
    ob = _make(second, kind, qs)
    # (a checkpoint is a copy: torch's load_state_dict keeps the very tensors of the dict it is handed)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    for gs in grads[3:]:
        _set_grads(ps, gs)
        _set_grads(qs, gs)
        oa.step()
        ob.step()
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    assert sa.keys() == sb.keys() and len(sa) == 3
    worst = 0.0
    for p, q in zip([p for pp in ps for p in pp], [q for qq in qs for q in qq]):
        worst = max(worst, R.rel_err(p.detach().cpu().numpy(), q.detach().cpu().numpy()))
    for i in sa:
        assert sa[i].keys() == sb[i].keys()
        for k in sa[i]:
            worst = max(worst, R.rel_err(torch.as_tensor(sa[i][k]).cpu().numpy(), torch.as_tensor(sb[i][k]).cpu().numpy()))
        if kind != R.SGD:
            assert float(sa[i]["step"]) == float(sb[i]["step"]) == 5.0
    print("%s %s: worst difference %.3e (bound %.3e)" % (IDS[kind], direction, worst, R.BOUND_F32_VS_F64))
    assert worst <= R.BOUND_F32_VS_F64
    assert torch.equal(ps[-1][-1], qs[-1][-1])                      # the parameter without a gradient


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_a_reloaded_optimizer_continues_bit_for_bit(kind):
    ps, grads = _host_case_on_device()
    oa = _make(FUSED[kind], kind, ps)
    for gs in grads[:3]:
        _set_grads(ps, gs)
        oa.step()
    qs = _clone(ps)
    ob = _make(FUSED[kind], kind, qs)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    assert ob.step_count() == (1 if kind == R.SGD else 3)
    for gs in grads[3:]:
        _set_grads(ps, gs)
        _set_grads(qs, gs)
        oa.step()
        ob.step()
    for p, q in zip([p for pp in ps for p in pp], [q for qq in qs for q in qq]):
        assert R.same_bits(p.detach().cpu().numpy(), q.detach().cpu().numpy())
        assert oa.state.get(p, {}).keys() == ob.state.get(q, {}).keys()
        for k in oa.state.get(p, {}):
            assert R.same_bits(oa.state[p][k].cpu().numpy(), ob.state[q][k].cpu().numpy()), k
    if kind != R.SGD:
        a, b = _snapshot_head(oa), _snapshot_head(ob)
        assert a == b, "step counter or running products differ after a reload"


def _snapshot_head(opt):
    return opt._block[_hip.CONSTANTS["M3D_OPTIM_STATE_T"]:O.HEAD_BYTES].cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------ 5. on the model
def test_three_iterations_on_the_model():
    """anab_fullalign, DLA-34, B = 2 at 64x128, RPN_3D_loss, torch.use_deterministic_algorithms: make_optimizer + adjust_lr +
    step(loss, skip_nonfinite, zero_grads).  Every parameter after every step equals the restatement applied to the downloaded
    parameters and gradients bit for bit; two runs from one seed end with the same bits; eval() packs the stepped weights."""
    from lib.loss.rpn_3d import RPN_3D_loss
    from lib.rpn_util import detect_batch
    from m3dssd_amd import synth
    from m3dssd_amd.host import ops
    from model.M3d_inference_align import build
    import rpn_loss_ref as RR
    crop, B, iters = (64, 128), 2, 3
    flags = synth.config_flags("anab_fullalign")
    before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
              torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)

    def make_conf():
        conf = RR.loss_conf(crop, 0, device="cuda:0")
        conf.update(flags)
        conf.batch_size = B
        conf.solver_type, conf.lr, conf.momentum, conf.weight_decay = "sgd", 0.002, 0.9, 0.0005
        conf.lr_policy, conf.lr_steps, conf.lr_target, conf.max_iter, conf.warmup = "cos", None, 0.002 * 1e-5, 8, 0.25
        return conf

    def run(check):
        conf = make_conf()
        net = build(conf, "train")
        net.load_state_dict(synth.synth_state_dict(0, back_bone="dla34", **flags), strict=True)
        net = net.to(_dev()).train()
        x = synth.synth_frames(B, crop, 1234).to(_dev())
        imobjs = RR.make_case(31, crop, B, 6)[4]
        crit = RPN_3D_loss(conf)
        opt = O.make_optimizer(conf, net)
        names = [n for n, _ in net.named_parameters()]
        plist = [p for _, p in net.named_parameters()]
        ref = R.Ref(R.SGD, [R.group(conf.lr, momentum=conf.momentum, weight_decay=conf.weight_decay)], np.float32)
        for it in range(iters):
            lr = O.adjust_lr(conf, opt, it)
            cls, prob, b2, b3, fs = net(x)
            loss, _ = crit(cls, prob, b2, b3, imobjs, fs)
            loss.backward()
            if check:
                assert lr == opt.param_groups[0]["lr"] and (it == 0) == (lr == 0.0)
                h_p = [p.detach().cpu().numpy().copy() for p in plist]
                h_g = [None if p.grad is None else p.grad.cpu().numpy().copy() for p in plist]
                assert float(loss.detach()) > 0 and sum(g is not None for g in h_g) > 100
            opt.step(loss=loss, skip_nonfinite=True, zero_grads=True)
            if check:
                ref.groups[0]["lr"] = lr
                _, bad, go = ref.step([h_p], [h_g], loss=float(loss.detach()), skip_nonfinite=True)
                assert go and bad == 0 and opt.last_step_taken() and int(opt.grad_nonfinite) == 0
                wrong = [n for n, p, h in zip(names, plist, h_p) if not R.same_bits(p.detach().cpu().numpy(), h)]
                assert not wrong, (it, len(wrong), wrong[:8])
                assert all(g is None or not p.grad.any() for p, g in zip(plist, h_g))
        return net, conf, x, {n: p.detach().clone() for n, p in zip(names, plist)}

    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
        assert ops.dcn_deterministic()
        net, conf, x, a = run(True)
        _, _, _, b = run(False)
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before[2], before[3]
    differ = [n for n in a if not R.same_bits(a[n].cpu().numpy(), b[n].cpu().numpy())]
    assert not differ, (len(differ), len(a), differ[:8])
    start = synth.synth_state_dict(0, back_bone="dla34", **flags)
    assert sum(not torch.equal(a[n].cpu(), start[n]) for n in a) > len(a) // 2, "the steps moved the weights"
    net.eval()
    with torch.no_grad():
        after = net(x)
    fresh = build(conf, "test")
    fresh.load_state_dict(net.state_dict(), strict=True)
    fresh = fresh.to(_dev()).eval()
    with torch.no_grad():
        want = fresh(x)
    assert all(torch.equal(p, q) for p, q in zip(after, want))
    dets, counts = detect_batch(net, x, conf)
    assert np.isfinite(dets.cpu().numpy()).all() and counts.numel() == B


# ------------------------------------------------------------------------------------ 6. C-ABI error paths
def test_cabi_error_paths_write_nothing():
    L = _hip.lib()
    dev = _dev()
    n = 100
    p = torch.full((n,), 1.5, device=dev)
    g = torch.full((n,), 0.5, device=dev)
    table = np.zeros(1, dtype=O._ENTRY)
    table[0] = (p.data_ptr(), g.data_ptr(), 0, 0, n, 0, 0)
    d_table = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)
    d_chunks = torch.zeros(2, dtype=torch.int32, device=dev)
    need = L.m3d_optim_state_bytes(1)
    assert need >= O.HEAD_BYTES + 12 and need % 16 == 0 and L.m3d_optim_state_bytes(-1) == -1 and L.m3d_optim_state_bytes(0) == O.HEAD_BYTES
    block = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
    hyper = np.zeros((9, 6), dtype=np.float64)
    hyper[:, 0] = 0.1
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def prepare(table=d_table.data_ptr(), kind=0, n_groups=1, state_bytes=need, hyper_ptr=hyper.ctypes.data):
        return L.m3d_optim_prepare(table, 1, d_chunks.data_ptr(), 1, kind, hyper_ptr, n_groups, None, 0, block.data_ptr(), state_bytes, s)

    def step(table=d_table.data_ptr(), kind=0, n_groups=1, state_bytes=need, hyper_ptr=hyper.ctypes.data):
        return L.m3d_optim_step(table, 1, d_chunks.data_ptr(), 1, kind, hyper_ptr, n_groups, 0, block.data_ptr(), state_bytes, s)

    E_ARG = _hip.CONSTANTS["M3D_E_ARG"]
    for fn in (prepare, step):
        for kw, word in ((dict(table=None), "null"), (dict(state_bytes=need - 1), str(need)), (dict(kind=3), "kind"),
                         (dict(n_groups=9), "groups"), (dict(kind=-1), "kind"), (dict(n_groups=0), "groups"), (dict(hyper_ptr=None), "null")):
            assert fn(**kw) == E_ARG, kw
            assert word in L.m3d_last_error().decode(), (kw, L.m3d_last_error().decode())
    bad = hyper.copy()
    bad[0, 0] = np.nan
    assert prepare(hyper_ptr=bad.ctypes.data) == E_ARG and "finite" in L.m3d_last_error().decode()
    torch.cuda.synchronize()
    assert (block.cpu() == 0x5A).all() and (p.cpu() == 1.5).all() and (g.cpu() == 0.5).all()
    # the same arguments, valid: the step is taken (SGD without momentum: p -= lr * g)
    block.zero_()
    assert prepare() == 0 and step() == 0
    torch.cuda.synchronize()
    assert np.array_equal(p.cpu().numpy(), np.full(n, np.float32(1.5) + np.float32(-0.1) * np.float32(0.5), dtype=np.float32))
    head = block[:O.HEAD_BYTES].cpu().numpy().view(O._HEAD)[0]
    assert head["grad_sq_sum"] == n * 0.25 and head["grad_nonfinite"] == 0 and head["do_step"] == 1 and head["t"] == 1
