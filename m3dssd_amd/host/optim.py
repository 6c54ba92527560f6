"""The optimizers ``init_training_model`` (lib/core.py:76-99) can build -- SGD(lr, momentum, weight_decay), Adam(lr, weight_decay),
Adamax(lr, weight_decay) -- as one fused device step (csrc/optim.hip), ``adjust_lr`` (lib/core.py:105-176) and the solver switch.

``SGD`` / ``Adam`` / ``Adamax`` subclass ``torch.optim.Optimizer``: same constructor arguments and defaults, same ``param_groups``
keys and ``state_dict()`` layout as the torch class of the same name (a checkpoint goes either way), and

    step(closure=None, loss=None, skip_nonfinite=False, zero_grads=False)

runs m3d_optim_prepare and m3d_optim_step over every parameter that has a gradient: two library calls (three kernels: the
gradient pass, its one-workgroup finish, the update), no synchronisation, no upload in steady state.  ``loss`` is the device
scalar the criterion returned: the step is taken iff ``loss > 0`` (the reference's ``if total_loss > 0``, decided on the device;
NaN: no step), with ``skip_nonfinite`` additionally iff no gradient element is inf / NaN.  A step that is not taken writes
nothing, not even the zeros of ``zero_grads``.  ``grad_sq_sum`` (float64), ``grad_nonfinite`` (int64) and ``stepped`` (int32) are
0-d device views of the state block, valid after a ``step``; ``last_step_taken()`` downloads the flag.

The arithmetic is the library's (tests/optim_ref.py), not torch's: the same formulas in a fixed order of single float32
operations, so that a step maps bits to bits whatever torch's default / foreach / fused forms do.  Differences to torch.optim:
one step counter for the whole optimizer (torch keeps one per parameter: they differ only for a parameter that received its
first gradient later than the others -- ``load_state_dict`` refuses a dict whose counters differ); bias corrections from running
products beta^t instead of ``pow``.  Not implemented (ValueError naming the option): nesterov, dampening, amsgrad, maximize,
decoupled weight decay, foreach / fused / capturable / differentiable, tensor learning rates, non-float32, sparse or
non-contiguous tensors, more than M3D_OPTIM_MAX_GROUPS groups.  A host parameter: NotImplementedError, no CPU fallback.
"""
import math

import numpy as np
import torch

from .. import _hip
from . import ops

_C = _hip.CONSTANTS
CHUNK, MAX_GROUPS, HYPER_COLS = _C["M3D_OPTIM_CHUNK"], _C["M3D_OPTIM_MAX_GROUPS"], _C["M3D_OPTIM_HYPER_COLS"]
HEAD_BYTES = _C["M3D_OPTIM_STATE_HEAD_BYTES"]
_ENTRY = np.dtype([("p", "<u8"), ("g", "<u8"), ("s0", "<u8"), ("s1", "<u8"), ("numel", "<i8"), ("group", "<i4"), ("pad", "<i4")])
assert _ENTRY.itemsize == _C["M3D_OPTIM_ENTRY_BYTES"]
_HEAD = np.dtype([("grad_sq_sum", "<f8"), ("grad_nonfinite", "<i8"), ("do_step", "<i4"), ("pad", "<i4"), ("t", "<i8"),
                  ("prod1", "<f8", MAX_GROUPS), ("prod2", "<f8", MAX_GROUPS), ("bc1", "<f4", MAX_GROUPS),
                  ("bc2_sqrt", "<f4", MAX_GROUPS), ("step_size", "<f4", MAX_GROUPS)])
assert _HEAD.itemsize == HEAD_BYTES and _HEAD.fields["t"][1] == _C["M3D_OPTIM_STATE_T"] and \
    _HEAD.fields["prod1"][1] == _C["M3D_OPTIM_STATE_PROD1"] and _HEAD.fields["step_size"][1] == _C["M3D_OPTIM_STATE_STEP_SIZE"]
# group options the kernels read; every other key of a group must hold the value torch gives it by default
_READ = ("params", "lr", "momentum", "weight_decay", "betas", "eps")


def _torch_defaults(cls, **kw):
    """The ``defaults`` dict the torch class builds from these arguments (its argument checks included): the group keys, and with
    them the state_dict layout, are torch's own in whatever version is installed."""
    return dict(cls([torch.zeros(1)], **kw).defaults)


class _Fused(torch.optim.Optimizer):
    KIND, TORCH, STATE_KEYS = None, None, ()

    def __init__(self, params, **kw):
        if torch.is_tensor(kw.get("lr")):
            raise ValueError("%s: a tensor lr is not supported (the settings travel as kernel arguments)" % type(self).__name__)
        defaults = _torch_defaults(self.TORCH, **kw)
        self._plain = _torch_defaults(self.TORCH)
        self._key = None                 # [(param ptr, grad ptr, numel, group, has momentum buffer)] of the table on the device
        self._pkey = None                # the same without the gradient pointers: what the state allocation depends on
        self._table = self._chunks = self._block = self._flat = None
        self._n_entries = self._n_chunks = 0
        self._device = None
        self._t_host = 0                 # the step counter to start the next state block from (load_state_dict); else it lives on the device
        super().__init__(params, defaults)
        self._hyper()

    # ---- settings -------------------------------------------------------------------------------------------------------------
    def _hyper(self):
        """float64 [n_groups, M3D_OPTIM_HYPER_COLS] (lr, momentum, weight_decay, beta1, beta2, eps) of the groups as they are NOW."""
        who = type(self).__name__
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError("%s: %d parameter groups; the kernels take up to %d" % (who, len(self.param_groups), MAX_GROUPS))
        h = np.zeros((len(self.param_groups), HYPER_COLS), dtype=np.float64)
        for gi, g in enumerate(self.param_groups):
            for k, v in g.items():
                if k in _READ:
                    continue
                dflt = self._plain.get(k)
                if torch.is_tensor(v) or not (v == dflt or (not v and not dflt)):
                    raise ValueError("%s: option %s=%r is not implemented by the fused step" % (who, k, v))
            if torch.is_tensor(g["lr"]):
                raise ValueError("%s: option lr as a tensor is not implemented by the fused step" % who)
            betas = g.get("betas", (0.0, 0.0))
            h[gi] = (g["lr"], g.get("momentum", 0.0), g["weight_decay"], betas[0], betas[1], g.get("eps", 0.0))
        return h

    def add_param_group(self, group):
        super().add_param_group(group)
        for p in self.param_groups[-1]["params"]:
            if p.dtype != torch.float32:
                raise ValueError("%s: a %s parameter; the fused step is float32 only" % (type(self).__name__, p.dtype))

    # ---- the table ------------------------------------------------------------------------------------------------------------
    def _has_buf(self, group):
        return self.KIND != 0 or group["momentum"] != 0

    def _current_key(self):
        key = []
        for gi, group in enumerate(self.param_groups):
            buf = self._has_buf(group)
            for p in group["params"]:
                if p.grad is not None:
                    key.append((p.data_ptr(), p.grad.data_ptr(), p.numel(), gi, buf))
        return key

    def _check_tensor(self, p):
        who = type(self).__name__
        for what, t in (("parameter", p), ("gradient", p.grad)):
            if t.device.type == "cpu":
                raise NotImplementedError("%s: a host %s; the fused step runs on the ROCm device, there is no CPU fallback" % (who, what))
            if not t.is_cuda or t.is_sparse or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("%s: a %s that is not a dense, contiguous float32 ROCm tensor (%s, %s)" % (who, what, t.dtype, t.device))
        if self._device is None:
            self._device = p.device
        if p.device != self._device or p.grad.device != self._device:
            raise ValueError("%s: parameters on %s and %s; one optimizer drives one device" % (who, self._device, p.device))

    def _head_host(self, t):
        head = np.zeros(1, dtype=_HEAD)
        head["t"] = t
        head["prod1"], head["prod2"] = 1.0, 1.0
        if self.KIND != 0:
            for gi, g in enumerate(self.param_groups):
                p1 = p2 = 1.0
                for _ in range(t):                      # t multiplications, as the device made them
                    p1 *= g["betas"][0]
                    p2 *= g["betas"][1]
                head["prod1"][0, gi], head["prod2"][0, gi] = p1, p2
        return head

    def _build(self, key):
        """Table, chunk list, flat state allocation and state block for the current set of (parameter, gradient) pointers.  When
        only gradient pointers moved (``zero_grad(set_to_none=True)`` between steps) the state allocation and the state block stay
        and the table alone is uploaded again."""
        entries = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is not None:
                    self._check_tensor(p)
                    entries.append((p, gi, self._has_buf(group)))
        dev = self._device
        if dev is None:
            return False                                # no gradient anywhere yet, nothing to launch on
        pkey = [(k[0], k[2], k[3], k[4]) for k in key]
        keep = self._block is not None and pkey == self._pkey
        n_state = len(self.STATE_KEYS)
        total, offs = 0, []
        for p, gi, buf in entries:
            o = []
            for _ in range(n_state if buf else 0):
                o.append(total)
                total += (p.numel() + 3) // 4 * 4       # every state tensor starts 16-byte aligned
            offs.append(o)
        flat = self._flat if keep else torch.zeros(max(total, 4), device=dev, dtype=torch.float32)
        table = np.zeros(max(len(entries), 1), dtype=_ENTRY)
        for i, ((p, gi, buf), o) in enumerate(zip(entries, offs)):
            ptrs = [0, 0]
            for k, (name, off) in enumerate(zip(self.STATE_KEYS, o)):
                st = self.state[p]
                if not keep:
                    view = flat[off:off + p.numel()].view(p.shape)
                    if st.get(name) is not None:        # an earlier table's view, or what load_state_dict put there
                        view.copy_(st[name])
                    st[name] = view
                ptrs[k] = st[name].data_ptr()
            table[i] = (p.data_ptr(), p.grad.data_ptr(), ptrs[0], ptrs[1], p.numel(), gi, 0)
        self._table = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)
        self._n_entries, self._key = len(entries), key
        if keep:
            return True
        counts = np.array([(p.numel() + CHUNK - 1) // CHUNK for p, _, _ in entries], dtype=np.int64)
        n_chunks = int(counts.sum())
        if n_chunks >= 2 ** 31:
            raise ValueError("%s: %d chunks" % (type(self).__name__, n_chunks))
        chunks = np.zeros((max(n_chunks, 1), 2), dtype=np.int32)
        if n_chunks:
            chunks[:n_chunks, 0] = np.repeat(np.arange(len(entries)), counts)
            chunks[:n_chunks, 1] = np.arange(n_chunks) - np.repeat(np.cumsum(counts) - counts, counts)
        nbytes = int(_hip.lib().m3d_optim_state_bytes(n_chunks))
        block = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
        if self._block is not None:
            block[:HEAD_BYTES].copy_(self._block[:HEAD_BYTES])          # t, the products: stream-ordered, no download
        else:
            block[:HEAD_BYTES].copy_(torch.from_numpy(self._head_host(self._t_host).view(np.uint8).reshape(-1)))
        self._chunks = torch.from_numpy(chunks.reshape(-1)).to(dev)
        self._flat, self._block, self._n_chunks, self._pkey = flat, block, n_chunks, pkey
        return True

    # ---- the step -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None, loss=None, skip_nonfinite=False, zero_grads=False):
        out = None
        if closure is not None:
            with torch.enable_grad():
                out = closure()
        hyper = self._hyper()
        key = self._current_key()                       # host pointers only: no device call
        if key != self._key and not self._build(key):
            return out
        loss_ptr = None
        if loss is not None:
            if not torch.is_tensor(loss) or not loss.is_cuda or loss.dtype != torch.float32 or loss.numel() != 1 or loss.device != self._device:
                raise ValueError("%s.step: loss must be the float32 device scalar the criterion returned" % type(self).__name__)
            loss_ptr = loss.detach().data_ptr()
        L = _hip.lib()
        args = (self._table.data_ptr(), self._n_entries, self._chunks.data_ptr(), self._n_chunks, self.KIND, hyper.ctypes.data,
                hyper.shape[0])
        with torch.cuda.device(self._device):
            s = ops._stream()
            _hip.check(L.m3d_optim_prepare(*args, loss_ptr, int(bool(skip_nonfinite)), self._block.data_ptr(), self._block.numel(), s))
            _hip.check(L.m3d_optim_step(*args, int(bool(zero_grads)), self._block.data_ptr(), self._block.numel(), s))
        return out

    def _field(self, name, dtype):
        if self._block is None:
            raise RuntimeError("%s: no step has run yet" % type(self).__name__)
        off = _C["M3D_OPTIM_STATE_" + name]
        return self._block[off:off + torch.empty((), dtype=dtype).element_size()].view(dtype)[0]

    @property
    def grad_sq_sum(self):
        """Sum of squares of every gradient element of the last ``step``: 0-d float64 device view."""
        return self._field("GRAD_SQ_SUM", torch.float64)

    @property
    def grad_nonfinite(self):
        """Number of inf / NaN gradient elements of the last ``step``: 0-d int64 device view."""
        return self._field("NONFINITE", torch.int64)

    @property
    def stepped(self):
        """1 where the last ``step`` was taken, else 0: 0-d int32 device view."""
        return self._field("DO_STEP", torch.int32)

    def last_step_taken(self):
        return bool(self.stepped.item())                # the download

    def step_count(self):
        """Taken steps so far (a download once a step has run)."""
        return self._t_host if self._block is None else int(self._field("T", torch.int64).item())

    # ---- checkpoints: torch.optim's dict for the same class -------------------------------------------------------------------
    def state_dict(self):
        t = self.step_count()
        with_state = [p for g in self.param_groups for p in g["params"] if any(k in self.state.get(p, ()) for k in self.STATE_KEYS)]
        if self.KIND != 0:
            for p in with_state:
                self.state[p]["step"] = torch.tensor(float(t), dtype=torch.float32)
        sd = super().state_dict()
        sd["state"] = {i: dict(st) for i, st in sd["state"].items()}          # (torch hands out self.state's own dicts)
        for p in with_state:
            self.state[p].pop("step", None)
        if t == 0:
            sd["state"] = {}                            # torch creates a parameter's state at its first step
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._hyper()
        steps = set()
        for st in self.state.values():
            if "step" in st:
                steps.add(int(float(st.pop("step"))))
        if len(steps) > 1:
            raise ValueError("%s.load_state_dict: per-parameter step counters %s differ; the fused step keeps one counter"
                             % (type(self).__name__, sorted(steps)))
        if self.KIND == 0:              # torch's SGD stores no counter: a stored buffer means its first step is behind it
            t = int(any(st.get("momentum_buffer") is not None for st in self.state.values()))
        else:
            t = steps.pop() if steps else 0
        self._t_host, self._key, self._pkey, self._block = t, None, None, None          # the next step builds table and state block from these


class SGD(_Fused):
    """torch.optim.SGD(params, lr, momentum, weight_decay) on the fused device step."""
    KIND, TORCH, STATE_KEYS = 0, torch.optim.SGD, ("momentum_buffer",)

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, **options):
        if nesterov:
            raise ValueError("SGD: option nesterov is not implemented by the fused step")
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, **options)


class Adam(_Fused):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) on the fused device step."""
    KIND, TORCH, STATE_KEYS = 1, torch.optim.Adam, ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **options):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **options)


class Adamax(_Fused):
    """torch.optim.Adamax(params, lr, betas, eps, weight_decay) on the fused device step."""
    KIND, TORCH, STATE_KEYS = 2, torch.optim.Adamax, ("exp_avg", "exp_inf")

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, **options):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **options)


def make_optimizer(conf, network):
    """The solver switch of ``init_training_model`` (lib/core.py:76-99) over the fused classes."""
    kind = conf.solver_type.lower()
    if kind == 'sgd':
        return SGD(network.parameters(), lr=conf.lr, momentum=conf.momentum, weight_decay=conf.weight_decay)
    if kind == 'adam':
        return Adam(network.parameters(), lr=conf.lr, weight_decay=conf.weight_decay)
    if kind == 'adamax':
        return Adamax(network.parameters(), lr=conf.lr, weight_decay=conf.weight_decay)
    raise ValueError('{} solver_type not understood'.format(conf.solver_type))         # (the reference leaves `optimizer` unbound)


def adjust_lr(conf, optimizer, iter):
    """``adjust_lr`` of lib/core.py:105-176, expression for expression (the returned learning rates are equal as float64): the
    'step', 'poly' and 'cos' policies of the SGD solver with warm-up and ``lr_steps``, the ``batch_skip`` early return (None), and
    for the other solvers the mean learning rate of the groups, which are left as they are."""
    if 'batch_skip' in conf and ((iter + 1) % conf.batch_skip) > 0:
        return

    if conf.solver_type.lower() == 'sgd':
        lr = conf.lr
        lr_steps = conf.lr_steps
        max_iter = conf.max_iter
        lr_policy = conf.lr_policy
        lr_target = conf.lr_target

        if lr_steps:
            steps = np.array(lr_steps) * max_iter
            total_steps = steps.shape[0]
            step_count = np.sum((steps - iter) <= 0)
        else:
            total_steps = max_iter
            step_count = iter

        if lr_policy.lower() == 'step':
            # the exact number of steps needed to get to lr_target
            scale = (lr_target / lr) ** (1 / total_steps)
            lr *= scale ** step_count
        elif lr_policy.lower() == 'poly':
            if step_count < int(total_steps * conf.warmup):
                scale = step_count / (total_steps * conf.warmup)
                lr = scale * conf.lr
            else:
                power = 0.9
                scale = total_steps / (1 - (lr_target / lr) ** (1 / power))
                lr *= (1 - step_count / scale) ** power
        elif lr_policy.lower() == 'cos':
            if step_count < int(max_iter * conf.warmup):
                scale = step_count / (max_iter * conf.warmup)
                lr = scale * conf.lr
            else:
                step_count -= int(max_iter * conf.warmup)
                max_iter -= int(max_iter * conf.warmup)
                scale = step_count / max_iter
                lr = conf.lr_target + 0.5 * (conf.lr - conf.lr_target) * (1 + math.cos(scale * math.pi))
        else:
            raise ValueError('{} lr_policy not understood'.format(lr_policy))

        for g in optimizer.param_groups:
            g['lr'] = lr
    else:
        lr = np.mean(np.array([g['lr'] for g in optimizer.param_groups]))
    return lr
