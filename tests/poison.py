"""Poisoned allocations: a helper for the tests that ask whether a result depends on memory nobody wrote.

`poisoned_allocations(fill)` replaces torch.empty, torch.empty_like, torch.empty_strided and Tensor.new_empty for the length of a
`with` block.  Every tensor they return on a listed device type (default: "cuda") is filled, on the current stream, before it is
handed back:

    fill     float dtypes (f16 / bf16 / f32 / f64, complex)      integer, bool and byte dtypes
    "zero"   all bytes 0x00                                      all bytes 0x00
    "nan"    all bytes 0xFF (NaN in every float type)            every 32-bit word = 1
    "huge"   all bytes 0x7F (3.39e38 in f32 and bf16)            every 32-bit word = 2

Integer and byte buffers get small values on purpose: a counter or index read before it is written then lands inside any real
buffer, so a forgotten initialisation shows as a wrong result and not as a GPU fault.  (A float partial that lives in a byte
workspace is therefore only weakly poisoned: tests/test_gpu_poison.py fills those workspaces itself.)

Nothing is filled while the current stream is capturing a graph: a fill would become a node of the graph.  Such tensors are
counted in `stats.skipped_capturing`.  CPU (and pinned) tensors are left alone unless `devices=` lists "cpu".

The `with` block yields the counters: tensors and bytes filled, in total, per dtype and per calling file, so that a test can
assert that it was not vacuous.  This module is no conftest and changes no pytest setting."""
import collections
import contextlib
import sys

import torch

FILLS = ("zero", "nan", "huge")
_FLOAT_BYTE = {"zero": 0x00, "nan": 0xFF, "huge": 0x7F}
_INT_WORD = {"zero": 0, "nan": 1, "huge": 2}

_REAL_EMPTY = torch.empty


class PoisonStats:
    def __init__(self, fill):
        self.fill = fill
        self.tensors = 0
        self.bytes = 0
        self.skipped_capturing = 0
        self.by_dtype = collections.Counter()          # dtype -> tensors filled
        self.bytes_by_dtype = collections.Counter()
        self.by_file = collections.Counter()           # file name of the caller of torch.empty & co. -> tensors filled
        self.bytes_by_file = collections.Counter()

    def from_file(self, suffix):
        """Tensors filled whose allocating call sits in a file whose path ends with `suffix` (e.g. "m3dssd_amd/engine.py")."""
        return sum(n for f, n in self.by_file.items() if f.replace("\\", "/").endswith(suffix))

    def from_dir(self, part):
        """Tensors filled whose allocating call sits in a file whose path contains `part` (e.g. "/m3dssd_amd/")."""
        return sum(n for f, n in self.by_file.items() if part in f.replace("\\", "/"))


def _is_float(dtype):
    return dtype.is_floating_point or dtype.is_complex


def _storage_bytes(t):
    """uint8 tensor over the whole storage of t (a fresh allocation owns its storage from byte 0)."""
    return _REAL_EMPTY(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())


def poison_(t, fill):
    """Fill the storage of t in place with the pattern of `fill` for its dtype (on the current stream of its device)."""
    if fill not in FILLS:
        raise ValueError("fill must be one of %s, got %r" % (FILLS, fill))
    u8 = _storage_bytes(t)
    n = u8.numel()
    if n == 0:
        return t
    if _is_float(t.dtype):
        u8.fill_(_FLOAT_BYTE[fill])
        return t
    word, whole = _INT_WORD[fill], n // 4 * 4
    if whole:
        u8[:whole].view(torch.int32).fill_(word)
    if n > whole:                                      # odd byte counts: the little-endian word goes on, cut short
        u8[whole:].zero_()
        u8[whole:whole + 1].fill_(word)
    return t


@contextlib.contextmanager
def poisoned_allocations(fill, devices=("cuda",), monkeypatch=None):
    """Context manager, see the module docstring.  monkeypatch: pytest's fixture (optional); the patch is undone when the block
    is left either way, also by an exception."""
    if fill not in FILLS:
        raise ValueError("fill must be one of %s, got %r" % (FILLS, fill))
    devices = tuple(devices)
    stats = PoisonStats(fill)

    def after(t, depth):
        if not isinstance(t, torch.Tensor) or t.device.type not in devices:
            return t
        if t.is_cuda:
            with torch.cuda.device(t.device):
                if torch.cuda.is_current_stream_capturing():
                    stats.skipped_capturing += 1
                    return t
                poison_(t, fill)
        else:
            poison_(t, fill)
        nbytes = t.untyped_storage().nbytes()
        fname = sys._getframe(depth).f_code.co_filename
        stats.tensors += 1
        stats.bytes += nbytes
        stats.by_dtype[t.dtype] += 1
        stats.bytes_by_dtype[t.dtype] += nbytes
        stats.by_file[fname] += 1
        stats.bytes_by_file[fname] += nbytes
        return t

    def wrap(orig):
        def patched(*args, **kwargs):
            return after(orig(*args, **kwargs), 2)
        patched.__name__ = getattr(orig, "__name__", "patched")
        patched.__wrapped__ = orig
        return patched

    targets = [(torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty")]
    with contextlib.ExitStack() as stack:
        if monkeypatch is not None:
            m = stack.enter_context(monkeypatch.context())
            for obj, name in targets:
                m.setattr(obj, name, wrap(getattr(obj, name)))
        else:
            for obj, name in targets:
                own = obj.__dict__.get(name, None) if isinstance(obj, type) else getattr(obj, name)
                setattr(obj, name, wrap(getattr(obj, name)))
                # (Tensor.new_empty is inherited from the C base class: undoing the patch means deleting the override)
                stack.callback((lambda o, n, v: delattr(o, n) if v is None else setattr(o, n, v)), obj, name, own)
        yield stats
