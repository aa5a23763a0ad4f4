"""Host tests of tests/wsguard.py on CPU tensors and fake owners: the helper must DETECT what the GPU contract tests rely on it
to detect — a one-byte write into either guard, a swapped cache entry, an untouched interior — for every kind of owner and
every pattern, and must pass a call that behaves."""
import pytest
import torch

import wsguard


class FakeCorpus:
    """The two accessors of ``DeviceCorpus`` that wsguard uses, over CPU tensors."""

    def __init__(self, sizes):
        self._ws = {key: (torch.zeros(n, dtype=torch.uint8), 7) for key, n in sizes.items()}

    def cached_workspaces(self):
        return {key: hit[0] for key, hit in self._ws.items()}

    def replace_cached_workspace(self, key, ws):
        self._ws[key] = (ws, self._ws[key][1])

    def call(self, at=0, value=0x11):
        """A well-behaved library call: writes inside every workspace it was given, nowhere else."""
        for ws, _ in self._ws.values():
            if ws.numel():
                ws[at] = value
                ws[-1] = value ^ 0x5A


class FakePipeline:
    def __init__(self, depth, need):
        self._ws = [torch.zeros(need, dtype=torch.uint8) for _ in range(depth)]


class FakeIvf:
    def __init__(self):
        self._probe_buf = torch.zeros(1000, dtype=torch.uint8)
        self._ivf_ws = torch.zeros(333, dtype=torch.uint8)


def _owners():
    return {"corpus": FakeCorpus({(5, 20): 1001, ("range", 3, 9): 64}), "pipeline": FakePipeline(3, 515), "ivf": FakeIvf(),
            "merge": {("cpu", 0): torch.zeros(4097, dtype=torch.uint8)}}


def _tensors(owner):
    return [get() for _, _, get, _ in wsguard._raw_slots(owner)]


def _touch_all(owner):
    for t in _tensors(owner):
        t[0] ^= 0x3C
        t[-1] ^= 0xC3


@pytest.mark.parametrize("pattern", wsguard.PATTERNS)
@pytest.mark.parametrize("kind", ["corpus", "pipeline", "ivf", "merge"])
def test_a_call_that_stays_inside_passes_and_each_violation_is_caught(kind, pattern):
    owner = _owners()[kind]
    before = [(t.numel(), t.data_ptr()) for t in _tensors(owner)]
    n = wsguard.guard(owner)
    assert n == len(before) >= 1
    wsguard.poison(owner, pattern)
    views = _tensors(owner)
    for v, (numel, ptr) in zip(views, before):
        assert v.numel() == numel and v.data_ptr() != ptr          # exactly `need` bytes, of another buffer
    # the guards are at least 4096 bytes, a multiple of 256, on both sides
    assert wsguard.G >= 4096 and wsguard.G % 256 == 0
    for slot in wsguard._registry[id(owner)][1]:
        assert slot.full.numel() == 2 * wsguard.G + slot.need and slot.view.data_ptr() == slot.full.data_ptr() + wsguard.G
    # untouched interior: vacuous, must fail
    with pytest.raises(AssertionError, match="did not use it"):
        wsguard.check(owner)
    _touch_all(owner)
    assert wsguard.check(owner) == n
    # one byte into the front guard, then into the back guard, of the last workspace
    slot = wsguard._registry[id(owner)][1][-1]
    for at, word in ((wsguard.G - 1, "front"), (wsguard.G + slot.need, "back"), (0, "front"), (slot.full.numel() - 1, "back")):
        keep = int(slot.full[at])
        slot.full[at] = keep ^ 0x01
        with pytest.raises(AssertionError, match=f"the {word} guard"):
            wsguard.check(owner)
        slot.full[at] = keep
        wsguard.check(owner)
    wsguard.release(owner)


def test_a_swapped_cache_entry_is_caught():
    for kind, owner in _owners().items():
        wsguard.guard(owner)
        wsguard.poison(owner, "0xff")
        _touch_all(owner)
        wsguard.check(owner)
        label, ws, get, put = wsguard._raw_slots(owner)[0]
        put(torch.zeros(ws.numel() + 1, dtype=torch.uint8))       # what a call that re-asked the size and grew the tensor does
        with pytest.raises(AssertionError, match="no longer holds the guarded view"):
            wsguard.check(owner)
        put(ws.clone())                                           # same size, other memory
        with pytest.raises(AssertionError, match="no longer holds the guarded view"):
            wsguard.check(owner)
        wsguard.check(owner, in_place=False)                      # the guards themselves are intact
        wsguard.release(owner)


def test_the_tuning_epoch_survives_the_swap():
    owner = FakeCorpus({(1, 2): 10})
    wsguard.guard(owner)
    assert owner._ws[(1, 2)][1] == 7 and owner._ws[(1, 2)][0].numel() == 10


def test_patterns_are_what_the_contract_names():
    buf = torch.empty(4096, dtype=torch.uint8)
    assert wsguard.PATTERNS == ("zeros", "random", "0x7f", "0xff")
    assert int(wsguard.fill_bytes(buf, "zeros").max()) == 0
    assert bool((wsguard.fill_bytes(buf, "0x7f") == 0x7F).all()) and bool((wsguard.fill_bytes(buf, "0xff") == 0xFF).all())
    a = wsguard.fill_bytes(buf, "random", seed=3).clone()
    assert torch.equal(a, wsguard.fill_bytes(buf, "random", seed=3)) and len(torch.unique(a)) > 200
    assert not torch.equal(a, wsguard.fill_bytes(buf, "random", seed=4))
    with pytest.raises(ValueError):
        wsguard.fill_bytes(buf, "0x80")


def test_guarded_outputs_and_buffers():
    out = wsguard.GuardedOutput((5, 3), torch.int64, "cpu")
    assert out.mid.shape == (5, 3) and out.mid.is_contiguous()
    with pytest.raises(AssertionError, match="never written"):
        out.check()
    out.mid.copy_(torch.arange(15).view(5, 3))
    out.check()
    out.mid[2, 1] = -1                                            # the documented -1 of an empty list is a written value
    out.check()
    out.full[out.pad - 1, 2] = 0
    with pytest.raises(AssertionError, match="in front of"):
        out.check()
    out = wsguard.GuardedOutput((7,), torch.float32, "cpu")
    out.mid.fill_(float("nan"))
    out.check()
    out.full[out.pad + 7] = 1.0
    with pytest.raises(AssertionError, match="behind"):
        out.check()
    buf = wsguard.GuardedBuffer(100, "cpu", "0x7f")
    with pytest.raises(AssertionError, match="did not use it"):
        buf.check()
    buf.view[5] = 0
    buf.check()
    buf._slot.full[wsguard.G + 100] = 0
    with pytest.raises(AssertionError, match="back guard"):
        buf.check()
    wsguard.check_ids(torch.tensor([0, 4, -1]), 5, allow_empty=True)
    with pytest.raises(AssertionError):
        wsguard.check_ids(torch.tensor([0, 5]), 5)
    with pytest.raises(AssertionError):
        wsguard.check_ids(torch.tensor([-1]), 5)


def test_bit_equality_sees_nan_payloads_and_signed_zero():
    a = torch.tensor([0.0, float("nan")])
    wsguard.assert_bit_equal((a,), (a.clone(),))
    with pytest.raises(AssertionError, match="differs"):
        wsguard.assert_bit_equal((a,), (torch.tensor([-0.0, float("nan")]),))
    b = a.clone()
    b.view(torch.int32)[1] += 1                                   # another NaN
    with pytest.raises(AssertionError, match="differs"):
        wsguard.assert_bit_equal((a,), (b,))
