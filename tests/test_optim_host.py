"""CPU tests of the fused optimizers' host side (m3dssd_amd/host/optim.py) and of the restatement tests/optim_ref.py that is the
contract of the kernels: the restatement against torch.optim in float64, its float32 form against its float64 form (the bound
the GPU comparison with torch.optim uses), adjust_lr against values tabulated from the reference's lib.core.adjust_lr
(tools/gen_golden_adjust_lr.py), and the behaviour that needs no device."""
import os

import numpy as np
import pytest
import torch

import optim_ref as R
from m3dssd_amd import _hip
from m3dssd_amd.config import Conf
from m3dssd_amd.host import optim as O

TORCH = {R.SGD: torch.optim.SGD, R.ADAM: torch.optim.Adam, R.ADAMAX: torch.optim.Adamax}
FUSED = {R.SGD: O.SGD, R.ADAM: O.Adam, R.ADAMAX: O.Adamax}
KINDS = [R.SGD, R.ADAM, R.ADAMAX]
IDS = ["sgd", "adam", "adamax"]


def torch_groups(kind, params):
    out = []
    for ps, g in zip(params, R.HOST_GROUPS[kind]):
        kw = dict(params=ps, lr=g["lr"], weight_decay=g["weight_decay"])
        if kind == R.SGD:
            kw["momentum"] = g["momentum"]
        out.append(kw)
    return out


def _run(kind):
    """Worst rel_err over 5 steps: (float64 restatement vs torch.optim in float64, float32 restatement vs the float64 one)."""
    params, grads = R.host_case()
    p64 = [[p.astype(np.float64) for p in ps] for ps in params]
    p32 = [[p.copy() for p in ps] for ps in params]
    tp = [[torch.nn.Parameter(torch.from_numpy(p.astype(np.float64))) for p in ps] for ps in params]
    opt = TORCH[kind](torch_groups(kind, tp))
    r64, r32 = R.Ref(kind, R.HOST_GROUPS[kind], np.float64), R.Ref(kind, R.HOST_GROUPS[kind], np.float32)
    vs_torch = vs_f64 = 0.0
    for gs in grads:
        for gi, gg in enumerate(gs):
            for pi, g in enumerate(gg):
                tp[gi][pi].grad = None if g is None else torch.from_numpy(g.astype(np.float64))
        opt.step()
        r64.step(p64, [[None if g is None else g.astype(np.float64) for g in gg] for gg in gs])
        r32.step(p32, gs)
        for gi, gg in enumerate(gs):
            for pi, g in enumerate(gg):
                vs_torch = max(vs_torch, R.rel_err(p64[gi][pi], tp[gi][pi].detach().numpy()))
                vs_f64 = max(vs_f64, R.rel_err(p32[gi][pi], p64[gi][pi]))
                if g is None:
                    assert (gi, pi) not in r64.state and tp[gi][pi] not in opt.state
                    continue
                for k, name in enumerate(R.STATE_KEYS[kind]):
                    vs_torch = max(vs_torch, R.rel_err(r64.state[(gi, pi)][k], opt.state[tp[gi][pi]][name].numpy()))
                    vs_f64 = max(vs_f64, R.rel_err(r32.state[(gi, pi)][k], r64.state[(gi, pi)][k]))
    # the parameter without a gradient is left alone by all three
    assert np.array_equal(p64[-1][-1], params[-1][-1].astype(np.float64)) and np.array_equal(p32[-1][-1], params[-1][-1])
    assert np.array_equal(tp[-1][-1].detach().numpy(), params[-1][-1].astype(np.float64))
    return vs_torch, vs_f64


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_restatement_follows_torch_in_float64(kind):
    """Two groups (lr 0.01 / 0.003, weight decay 5e-4 / 1e-3), momentum 0.9, one parameter without a gradient, 5 steps.
    Measured worst case over the three solvers: 7.35e-17 of 1 + |p| (0.33 ulp of float64); asserted at 4x."""
    vs_torch, _ = _run(kind)
    print("float64 restatement vs torch.optim: %.3e (bound %.3e)" % (vs_torch, R.BOUND_F64_VS_TORCH))
    assert vs_torch <= R.BOUND_F64_VS_TORCH


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_float32_restatement_against_float64(kind):
    """The same run in float32 against float64.  Measured worst case over the three solvers: 5.62e-08 of 1 + |p| (0.47 ulp of
    float32); asserted at 4x -- the bound tests/test_gpu_optim.py uses for the fused step against torch.optim on the device."""
    _, vs_f64 = _run(kind)
    print("float32 restatement vs float64: %.3e (bound %.3e)" % (vs_f64, R.BOUND_F32_VS_F64))
    assert vs_f64 <= R.BOUND_F32_VS_F64


def test_prepare_decision_and_bias_corrections():
    g = [np.array([1.0, -2.0], np.float32), np.array([[3.0]], np.float32)]
    assert R.decide(g) == (14.0, 0, True)
    for loss, go in ((1.0, True), (0.0, False), (-1.0, False), (float("nan"), False), (float("inf"), True)):
        assert R.decide(g, loss)[2] is go
    bad = [np.array([np.nan, 1.0, np.inf], np.float32)]
    assert R.decide(bad)[1:] == (2, True) and R.decide(bad, 1.0, True)[1:] == (2, False)
    r = R.Ref(R.ADAM, [R.group(0.01, betas=(0.9, 0.999))], np.float64)
    for t in range(1, 8):
        r.advance()
        bc1, bc2s, step = r.bias(0)
        assert abs(bc1 - (1 - 0.9 ** t)) <= 4e-16 and abs(bc2s - (1 - 0.999 ** t) ** 0.5) <= 4e-16 and abs(step - 0.01 / (1 - 0.9 ** t)) <= 4e-16


# ------------------------------------------------------------------------------------ adjust_lr
def _golden_rows(golden_dir):
    z = np.load(os.path.join(golden_dir, "adjust_lr.npz"))
    assert all(z[k].dtype.kind in "fi" for k in z.files), "the fixture holds numbers only"
    return z


def _conf(z, i):
    conf = Conf()
    conf.solver_type = ("sgd", "adam", "adamax")[int(z["solver"][i])]
    conf.lr_policy = ("step", "poly", "cos")[int(z["policy"][i])]
    conf.lr, conf.lr_target, conf.warmup, conf.max_iter = float(z["lr"][i]), float(z["lr_target"][i]), float(z["warmup"][i]), int(z["max_iter"][i])
    steps = z["lr_steps"][i]
    conf.lr_steps = None if np.isnan(steps).all() else [float(s) for s in steps[~np.isnan(steps)]]
    if z["batch_skip"][i]:
        conf.batch_skip = int(z["batch_skip"][i])
    return conf


def test_adjust_lr_equals_the_reference(golden_dir):
    z = _golden_rows(golden_dir)
    n, k = z["iters"].shape
    assert n >= 10 and k == 7 and set(z["policy"].tolist()) == {0, 1, 2} and (z["batch_skip"] > 0).any() and (z["solver"] > 0).any()
    assert np.isfinite(z["lr_steps"]).any(axis=1).any() and (z["returned"] == 0).any()
    for i in range(n):
        for j in range(k):
            ps = [torch.nn.Parameter(torch.zeros(1)), torch.nn.Parameter(torch.zeros(1))]
            cls = FUSED[int(z["solver"][i])]
            opt = cls([dict(params=[p], lr=float(lr)) for p, lr in zip(ps, z["group_lrs"][i])])
            got = O.adjust_lr(_conf(z, i), opt, int(z["iters"][i, j]))
            what = "policy row %d, iteration %d" % (i, z["iters"][i, j])
            if z["returned"][i, j]:
                assert got is not None and np.float64(got).tobytes() == z["lr_out"][i, j].tobytes(), what
            else:
                assert got is None, what
            after = np.array([g["lr"] for g in opt.param_groups], dtype=np.float64)
            assert after.tobytes() == z["group_out"][i, j].tobytes(), what


def test_adjust_lr_refuses_an_unknown_policy():
    conf = Conf(solver_type="sgd", lr=0.1, lr_target=0.01, lr_steps=None, max_iter=10, lr_policy="exp", warmup=0.1)
    with pytest.raises(ValueError, match="lr_policy"):
        O.adjust_lr(conf, O.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), 3)


# ------------------------------------------------------------------------------------ host behaviour
def _params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


@pytest.mark.parametrize("cls,kw,name", [
    (O.SGD, dict(momentum=0.9, nesterov=True), "nesterov"), (O.SGD, dict(momentum=0.9, dampening=0.1), "dampening"),
    (O.SGD, dict(maximize=True), "maximize"), (O.Adam, dict(amsgrad=True), "amsgrad"), (O.Adam, dict(maximize=True), "maximize"),
    (O.Adam, dict(decoupled_weight_decay=True), "decoupled_weight_decay"), (O.Adamax, dict(maximize=True), "maximize"),
    (O.Adam, dict(foreach=True), "foreach"), (O.Adam, dict(capturable=True), "capturable"),
])
def test_unsupported_options_raise(cls, kw, name):
    with pytest.raises(ValueError, match=name):
        cls(_params(), lr=0.1, **kw)


def test_unsupported_tensors_raise():
    with pytest.raises(ValueError, match="float32"):
        O.SGD([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))], lr=0.1)
    with pytest.raises(ValueError, match="float32"):
        O.Adam([torch.nn.Parameter(torch.zeros(3, dtype=torch.bfloat16))], lr=0.1)
    with pytest.raises(ValueError, match="ROCm"):
        p = torch.nn.Parameter(torch.zeros(3, device="meta"))
        p.grad = torch.zeros(3, device="meta")
        O.SGD([p], lr=0.1).step()
    with pytest.raises(ValueError, match="groups"):
        O.SGD([dict(params=[torch.nn.Parameter(torch.zeros(1))]) for _ in range(9)], lr=0.1)
    opt = O.SGD(_params(), lr=0.1)
    opt.param_groups[0]["nesterov"] = True          # an option switched on after construction is met at the step
    with pytest.raises(ValueError, match="nesterov"):
        opt.step()


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_a_host_parameter_has_no_fallback(kind):
    ps = _params()
    opt = FUSED[kind](ps, lr=0.1)
    opt.step()                                       # no gradient anywhere: nothing to do, as torch
    ps[0].grad = torch.ones(3)
    with pytest.raises(NotImplementedError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(ps[0].detach(), torch.zeros(3))


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_state_dict_layout_is_torchs(kind):
    """Before a step (the state a host can reach): the same dict as the torch class -- group keys in order, values, empty state --
    and each class loads the other's dict."""
    kw = dict(lr=0.01, weight_decay=5e-4, **(dict(momentum=0.9) if kind == R.SGD else {}))
    ours, theirs = FUSED[kind](_params(), **kw), TORCH[kind](_params(), **kw)
    a, b = ours.state_dict(), theirs.state_dict()
    assert a == b and [list(g) for g in a["param_groups"]] == [list(g) for g in b["param_groups"]]
    # a torch dict WITH state, as a checkpoint holds it
    ps = _params()
    full = TORCH[kind](ps, **kw)
    for p in ps:
        p.grad = torch.full_like(p, 0.5)
    full.step()
    full.step()
    sd = full.state_dict()
    ours.load_state_dict(sd)
    back = ours.state_dict()
    assert back["param_groups"] == sd["param_groups"] and back["state"].keys() == sd["state"].keys()
    for i, st in sd["state"].items():
        assert back["state"][i].keys() == st.keys()
        for k, v in st.items():
            assert torch.equal(torch.as_tensor(back["state"][i][k]).double(), torch.as_tensor(v).double()), (i, k)
    assert ours.step_count() == (1 if kind == R.SGD else 2)
    theirs.load_state_dict(back)                      # and the other way


def test_differing_step_counters_are_refused():
    ps = _params()
    full = torch.optim.Adam(ps, lr=0.1)
    ps[0].grad = torch.ones(3)
    full.step()
    ps[1].grad = torch.ones(2, 2)
    full.step()
    with pytest.raises(ValueError, match="counter"):
        O.Adam(_params(), lr=0.1).load_state_dict(full.state_dict())


def test_make_optimizer_is_the_solver_switch():
    net = torch.nn.Linear(3, 2)
    conf = Conf(solver_type="SGD", lr=0.004, momentum=0.9, weight_decay=0.0005)
    opt = O.make_optimizer(conf, net)
    assert type(opt) is O.SGD and opt.defaults["momentum"] == 0.9 and opt.defaults["weight_decay"] == 0.0005 and opt.defaults["lr"] == 0.004
    conf.solver_type = "adam"
    opt = O.make_optimizer(conf, net)
    assert type(opt) is O.Adam and opt.defaults["betas"] == (0.9, 0.999) and opt.defaults["weight_decay"] == 0.0005
    conf.solver_type = "Adamax"
    assert type(O.make_optimizer(conf, net)) is O.Adamax
    conf.solver_type = "rmsprop"
    with pytest.raises(ValueError, match="solver_type"):
        O.make_optimizer(conf, net)


def test_the_header_declares_the_entry_points():
    fns = _hip.DECLS.functions
    assert {"m3d_optim_prepare", "m3d_optim_step", "m3d_optim_state_bytes"} <= set(fns)
    assert fns["m3d_optim_state_bytes"][0] == "long long"
    assert [k for k, _ in fns["m3d_optim_step"][1]][-1] == "m3d_stream_t"
    c = _hip.CONSTANTS
    assert c["M3D_ABI_VERSION"] == 5 and c["M3D_OPTIM_CHUNK"] % 1024 == 0 and c["M3D_OPTIM_MAX_GROUPS"] == 8
    assert c["M3D_OPTIM_STATE_HEAD_BYTES"] == O._HEAD.itemsize
