"""The optimizer step restated in numpy: the CONTRACT of csrc/optim.hip (m3d_optim_prepare / m3d_optim_step).

numpy never fuses a multiplication with an addition, and its float32 `+ - * /` and `sqrt` are correctly rounded, so with
``dtype=np.float32`` every line below is one IEEE operation and the kernel has to give the same bits.  With ``dtype=np.float64``
the same lines follow ``torch.optim.SGD / Adam / Adamax`` (single-tensor forms) to a few float64 ulps: the differences are
torch's `beta ** step` where this uses a running product, `(value * g) * g` in addcmul where this has `value * (g * g)`, and
the fused multiply-adds of torch's CPU kernels.

    all     g += wd*p                                   (skipped for wd == 0, as torch does)
    SGD     buf = g on the first taken step, else buf = momentum*buf + g;   p += (-lr)*buf       (momentum 0: p += (-lr)*g)
    Adam    m += (1-beta1)*(g-m);  v = beta2*v + (1-beta2)*(g*g);  denom = sqrt(v)/sqrt(bc2) + eps;  p += (-(lr/bc1))*(m/denom)
    Adamax  m += (1-beta1)*(g-m);  u = max(beta2*u, |g|+eps);  p += (-(lr/bc1))*(m/u)

Every scalar is the float64 (Python) expression rounded ONCE to ``dtype``: -lr, momentum, wd, 1-beta1, beta2, 1-beta2, eps;
bc1 = 1 - beta1^t, sqrt(bc2) = sqrt(1 - beta2^t) and lr / bc1 are float64 arithmetic on the running products, rounded once.
"""
import math

import numpy as np

SGD, ADAM, ADAMAX = 0, 1, 2
STATE_KEYS = {SGD: ("momentum_buffer",), ADAM: ("exp_avg", "exp_avg_sq"), ADAMAX: ("exp_avg", "exp_inf")}


def group(lr, momentum=0.0, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8):
    return dict(lr=float(lr), momentum=float(momentum), weight_decay=float(weight_decay), betas=(float(betas[0]), float(betas[1])),
                eps=float(eps))


def decide(grads, loss=None, skip_nonfinite=False):
    """m3d_optim_prepare's decision: (sum of g*g in float64, count of non-finite elements, do_step).  ``loss``: None or a number."""
    sq, bad = 0.0, 0
    for g in grads:
        g64 = np.asarray(g, dtype=np.float64).reshape(-1)
        sq += float(np.sum(g64 * g64))
        bad += int(np.count_nonzero(~np.isfinite(g64)))
    go = True
    if loss is not None:
        go = bool(np.float32(loss) > np.float32(0))          # False for NaN
    if skip_nonfinite:
        go = go and bad == 0
    return sq, bad, go


class Ref:
    """One optimizer over ``groups`` (dicts of ``group()``); ``params[gi]`` is the list of numpy arrays of group gi, updated in
    place.  State arrays are created on the first step a parameter takes part in (zeros), like the flat allocation of the device."""

    def __init__(self, kind, groups, dtype=np.float32):
        self.kind, self.groups, self.dt = kind, [dict(g) for g in groups], np.dtype(dtype).type
        self.t = 0
        self.prod1 = [1.0] * len(groups)
        self.prod2 = [1.0] * len(groups)
        self.state = {}              # (gi, pi) -> [s0, s1]

    def bias(self, gi):
        """(bc1, sqrt(bc2), lr / bc1) of group gi for the current t, float64 arithmetic rounded once."""
        bc1 = 1.0 - self.prod1[gi]
        bc2 = 1.0 - self.prod2[gi]
        return self.dt(bc1), self.dt(math.sqrt(bc2)), self.dt(self.groups[gi]["lr"] / bc1)

    def advance(self):
        self.t += 1
        if self.kind != SGD:
            for gi, h in enumerate(self.groups):
                self.prod1[gi] *= h["betas"][0]
                self.prod2[gi] *= h["betas"][1]

    def step(self, params, grads, loss=None, skip_nonfinite=False, zero_grads=False):
        """params / grads: per group, lists of arrays; a grad of None leaves its parameter out.  Returns (sq, bad, do_step)."""
        flat = [g for gs in grads for g in gs if g is not None]
        sq, bad, go = decide(flat, loss, skip_nonfinite)
        if not go:
            return sq, bad, go
        self.advance()
        first = self.t == 1
        dt = self.dt
        for gi, h in enumerate(self.groups):
            neg_lr, mom, wd = dt(-h["lr"]), dt(h["momentum"]), dt(h["weight_decay"])
            omb1, b2, omb2, eps = dt(1.0 - h["betas"][0]), dt(h["betas"][1]), dt(1.0 - h["betas"][1]), dt(h["eps"])
            if self.kind != SGD:
                _, bc2s, step_size = self.bias(gi)
                neg_step = -step_size
            for pi, (p, g_in) in enumerate(zip(params[gi], grads[gi])):
                if g_in is None:
                    continue
                g = g_in.astype(dt)
                st = self.state.setdefault((gi, pi), [np.zeros_like(p), np.zeros_like(p)])
                with np.errstate(all="ignore"):
                    if h["weight_decay"] != 0:
                        g = g + wd * p
                    if self.kind == SGD:
                        if h["momentum"] != 0:
                            st[0][...] = g if first else mom * st[0] + g
                            g = st[0]
                        p[...] = p + neg_lr * g
                    else:
                        m = st[0]
                        m[...] = m + omb1 * (g - m)
                        if self.kind == ADAM:
                            v = st[1]
                            v[...] = b2 * v + omb2 * (g * g)
                            denom = np.sqrt(v) / bc2s + eps
                            p[...] = p + neg_step * (m / denom)
                        else:
                            u = st[1]
                            u[...] = np.maximum(b2 * u, np.abs(g) + eps)
                            p[...] = p + neg_step * (m / u)
                if zero_grads:
                    g_in[...] = 0
        return sq, bad, go


# ---- the seeded cases of the GPU test ---------------------------------------------------------------------------------------------
def table_sizes(chunk):
    """numel of the plain tensors of the GPU table: the sizes at which a chunked multi-tensor kernel goes wrong."""
    return [0, 1, 3, 4, 5, 1023, 1024, 1025, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]


def values(rng, n, scale):
    """n float32 values of magnitude ~scale, none closer to zero than scale / 64 (squares and products stay normal float32)."""
    x = rng.standard_normal(n).astype(np.float32) * np.float32(scale)
    return (x + np.copysign(np.float32(scale / 64), x)).astype(np.float32)


def same_bits(a, b):
    """Bit equality of two float arrays; NaN equals NaN whatever its payload (payloads are outside the contract)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


# ---- the small case the host test measures its bounds on (the GPU checkpoint tests run the same one) ------------------------------
HOST_GROUPS = {
    SGD: [group(0.01, momentum=0.9, weight_decay=5e-4), group(0.003, momentum=0.9, weight_decay=1e-3)],
    ADAM: [group(0.01, weight_decay=5e-4), group(0.003, weight_decay=1e-3)],
    ADAMAX: [group(0.01, weight_decay=5e-4), group(0.003, weight_decay=1e-3)],
}
HOST_SHAPES = [[(33,), (8, 5)], [(17,), (4,)]]          # per group; the last parameter never gets a gradient
HOST_STEPS = 5


def host_case(seed=11):
    """(params, grads per step) as float32 arrays: params[gi][pi], grads[step][gi][pi] (None for the last parameter)."""
    rng = np.random.default_rng(seed)
    params = [[values(rng, int(np.prod(s)), 0.5).reshape(s) for s in shapes] for shapes in HOST_SHAPES]
    grads = []
    for _ in range(HOST_STEPS):
        gs = [[values(rng, int(np.prod(s)), 0.1).reshape(s) for s in shapes] for shapes in HOST_SHAPES]
        gs[-1][-1] = None
        grads.append(gs)
    return params, grads


def rel_err(a, b):
    """max |a - b| / (1 + |b|), in float64."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b)))) if a.size else 0.0


# Worst cases measured by tests/test_optim_host.py on the case above (CPU, 5 steps, parameters and every state tensor, all three
# solvers), as rel_err; the tests assert at 4x the measurement:
#   float64 restatement against torch.optim (CPU, float64)   7.35e-17 (0.33 ulp of float64) -- torch's pow and fused multiply-adds
#   float32 restatement against the float64 restatement      5.62e-08 (0.47 ulp of float32) -- the rounding of the float32 operations
MEASURED_F64_VS_TORCH = 7.35e-17
MEASURED_F32_VS_F64 = 5.62e-8
BOUND_F64_VS_TORCH = 4 * MEASURED_F64_VS_TORCH
BOUND_F32_VS_F64 = 4 * MEASURED_F32_VS_F64          # also the bound of the fused step against torch.optim on the device (float32 both)
