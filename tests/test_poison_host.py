"""Host tests of tests/poison.py on CPU tensors (devices=("cpu",)): the byte patterns per dtype, odd byte counts, the counters,
the undoing of the patch, and that a device that is not listed is left alone."""
import pytest
import torch

import poison
from poison import poisoned_allocations

FLOATS = (torch.float16, torch.bfloat16, torch.float32, torch.float64)
PATCHED = ((torch, "empty"), (torch, "empty_like"), (torch, "empty_strided"), (torch.Tensor, "new_empty"))


def _current():
    return [getattr(o, n) for o, n in PATCHED]


def _bytes(t):
    return t.contiguous().view(torch.uint8).flatten()


@pytest.mark.parametrize("dtype", FLOATS, ids=str)
def test_float_patterns(dtype):
    with poisoned_allocations("nan", devices=("cpu",)):
        t = torch.empty(3, 5, dtype=dtype)
    assert torch.isnan(t).all() and (_bytes(t) == 0xFF).all()
    with poisoned_allocations("huge", devices=("cpu",)):
        t = torch.empty(3, 5, dtype=dtype)
    assert (_bytes(t) == 0x7F).all()
    if dtype in (torch.float32, torch.bfloat16):
        assert torch.isfinite(t).all() and (t.float() > 3.38e38).all() and (t.float() < 3.40e38).all()
    with poisoned_allocations("zero", devices=("cpu",)):
        t = torch.empty(3, 5, dtype=dtype)
    assert (_bytes(t) == 0).all() and (t == 0).all()


@pytest.mark.parametrize("fill,word", [("zero", 0), ("nan", 1), ("huge", 2)])
def test_integer_patterns_are_small_words(fill, word):
    with poisoned_allocations(fill, devices=("cpu",)):
        i32 = torch.empty(7, dtype=torch.int32)
        i16 = torch.empty(8, dtype=torch.int16)
        u8 = torch.empty(12, dtype=torch.uint8)
        b = torch.empty(4, dtype=torch.bool)
        i64 = torch.empty(3, dtype=torch.int64)
    assert (i32 == word).all()
    assert i16.tolist() == [word, 0] * 4                      # little-endian halves of the 32-bit word
    assert u8.tolist() == [word, 0, 0, 0] * 3
    assert _bytes(b.view(torch.uint8)).tolist() == [word, 0, 0, 0]
    assert (i64 == word * (2 ** 32 + 1)).all()                # both 32-bit halves hold the word (the package has no int64 site)


@pytest.mark.parametrize("fill,word", [("nan", 1), ("huge", 2)])
def test_odd_byte_counts(fill, word):
    with poisoned_allocations(fill, devices=("cpu",)):
        u8 = [torch.empty(n, dtype=torch.uint8) for n in (1, 2, 3, 5, 7, 9)]
        i16 = torch.empty(3, dtype=torch.int16)               # 6 bytes
        f16 = torch.empty(3, dtype=torch.float16)             # 6 bytes
    for t in u8:
        assert t.tolist() == [word if i % 4 == 0 else 0 for i in range(t.numel())]
    assert i16.tolist() == [word, 0, word]
    assert torch.isnan(f16).all() and (_bytes(f16) == (0xFF if fill == "nan" else 0x7F)).all()


def test_every_patched_entry_and_the_counters():
    base = torch.zeros(2, 3)
    with poisoned_allocations("nan", devices=("cpu",)) as st:
        a = torch.empty(4, dtype=torch.float32)                       # 16 bytes
        b = torch.empty_like(base)                                    # 24 bytes
        c = torch.empty_strided((2, 3), (3, 1), dtype=torch.float64)  # 48 bytes
        d = base.new_empty(5, dtype=torch.int32)                      # 20 bytes
        e = torch.empty(0)
    for t in (a, b, c):
        assert torch.isnan(t).all()
    assert (d == 1).all() and e.numel() == 0
    assert st.fill == "nan" and st.tensors == 5 and st.bytes == 16 + 24 + 48 + 20 and st.skipped_capturing == 0
    assert st.by_dtype == {torch.float32: 3, torch.float64: 1, torch.int32: 1}
    assert st.bytes_by_dtype[torch.float32] == 40 and st.bytes_by_dtype[torch.int32] == 20
    assert list(st.by_file) == [__file__] and st.by_file[__file__] == 5 and st.bytes_by_file[__file__] == 108
    assert st.from_file("tests/test_poison_host.py") == 5 and st.from_file("m3dssd_amd/engine.py") == 0
    assert st.from_dir("/tests/") == 5


def test_non_dense_strides_fill_the_whole_storage():
    with poisoned_allocations("nan", devices=("cpu",)) as st:
        t = torch.empty_strided((2, 2), (4, 1), dtype=torch.float32)  # 6 elements of storage, 4 visible
    assert torch.isnan(t).all() and st.bytes == t.untyped_storage().nbytes()
    whole = torch.empty(0, dtype=torch.float32).set_(t.untyped_storage())
    assert torch.isnan(whole).all()


def test_patch_is_undone_on_exit_and_on_exception():
    before = _current()
    had_override = "new_empty" in torch.Tensor.__dict__
    with poisoned_allocations("huge", devices=("cpu",)):
        assert all(a is not b for a, b in zip(_current(), before))
    assert all(a is b for a, b in zip(_current(), before))
    assert ("new_empty" in torch.Tensor.__dict__) == had_override
    with pytest.raises(KeyError):
        with poisoned_allocations("huge", devices=("cpu",)):
            raise KeyError("x")
    assert all(a is b for a, b in zip(_current(), before))
    assert ("new_empty" in torch.Tensor.__dict__) == had_override


def test_with_the_monkeypatch_fixture(monkeypatch):
    before = _current()
    with poisoned_allocations("nan", devices=("cpu",), monkeypatch=monkeypatch) as st:
        t = torch.empty(3)
        assert torch.isnan(t).all()
    assert st.tensors == 1 and all(a is b for a, b in zip(_current(), before))


def test_unlisted_devices_are_left_untouched(monkeypatch):
    """The default lists "cuda" only: CPU tensors come back as torch made them (the fill routine is never entered), and nothing
    is counted."""
    def refuse(t, fill):
        raise AssertionError("poison_ called for a tensor on %s" % t.device)
    monkeypatch.setattr(poison, "poison_", refuse)
    marker = torch.full((64,), 5.0)
    with poisoned_allocations("nan") as st:
        a = torch.empty(64)
        b = torch.empty_like(marker)
        c = marker.new_empty(8)
        m = torch.empty(4, device="meta")
    assert st.tensors == 0 and st.bytes == 0 and not st.by_file
    assert a.shape == (64,) and b.shape == (64,) and c.shape == (8,) and m.device.type == "meta"
    with poisoned_allocations("nan", devices=("cpu",)) as st:
        m = torch.empty(4, device="meta")
    assert st.tensors == 0


def test_unknown_fill_is_an_error():
    with pytest.raises(ValueError):
        with poisoned_allocations("ones"):
            pass
    with pytest.raises(ValueError):
        poison.poison_(torch.zeros(2), "ones")
