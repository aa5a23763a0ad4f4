"""Guarded, poisoned workspaces and outputs for the workspace-contract tests (a plain helper module, like parity.py).

The C ABI works in caller-owned workspaces whose contents on entry are undefined (include/dewi_hip.h), and the Python layer
keeps them in caches that outlive a call.  This module swaps every cached workspace of an owner for the middle of a larger
buffer, fills the whole buffer with a hostile pattern, and afterwards checks that

* the bytes in front of and behind the workspace are what the fill wrote (no write outside ``workspace_bytes``),
* the cache still holds the guarded view (a call that swapped the tensor ran on memory nobody poisoned: vacuous, fails),
* a workspace of non-zero size was written to at all.

Owners (duck-typed, so that the host test can pass a fake):

* ``cached_workspaces()`` / ``replace_cached_workspace(key, ws)``: a ``DeviceCorpus``;
* a ``_ws`` LIST of tensors: a ``PipelinedSearcher`` (every slot);
* ``_probe_buf`` and ``_ivf_ws`` attributes: an ``IVFIndex`` (its cell lists hold built data, not scratch: the test builds
  them into a guarded buffer of its own, ``GuardedBuffer``);
* a plain dict key -> tensor: ``_engine._merge_ws``.

Outputs are the middle rows of a larger tensor prefilled with a sentinel: ``GuardedOutput``.
"""
import numpy as np
import torch

G = 4096                                   # guard bytes on either side of a workspace: a multiple of 256, at least 4096
PATTERNS = ("zeros", "random", "0x7f", "0xff")    # from mild to hostile: a logic error shows before a count of 2^32 - 1 is read
SENTINEL = 0xA5                            # every byte of an output before the call: id < -1, score -2.87e-16 (bits 0xA5A5A5A5)

_registry = {}                             # id(owner) -> (owner, [slot])


def fill_bytes(buf, pattern, seed=0):
    """Fill a uint8 tensor with one of ``PATTERNS``: 0x00; seeded random bytes; 0x7F (0x7F7F7F7F: a finite fp32 near FLT_MAX, a
    large positive count); 0xFF (NaN as fp32, -1 as an id, the largest count, the empty-key pattern)."""
    assert buf.dtype == torch.uint8
    if pattern == "zeros":
        buf.zero_()
    elif pattern == "random":
        gen = torch.Generator(device="cpu").manual_seed(1234 + seed)
        buf.copy_(torch.randint(0, 256, (buf.numel(),), dtype=torch.uint8, generator=gen))
    elif pattern == "0x7f":
        buf.fill_(0x7F)
    elif pattern == "0xff":
        buf.fill_(0xFF)
    else:
        raise ValueError(f"unknown pattern {pattern!r}: one of {PATTERNS}")
    return buf


class _Slot:
    """One guarded workspace: ``full`` = guard | the ``need`` bytes the library gets | guard; ``fill``: what poison wrote."""

    def __init__(self, label, need, device, get, put):
        self.label, self.need, self.get, self.put = label, int(need), get, put
        self.full = torch.empty(G + self.need + G, dtype=torch.uint8, device=device)
        self.fill = None
        self.view = self.full[G: G + self.need]

    def poison(self, pattern, seed):
        fill_bytes(self.full, pattern, seed)
        self.fill = self.full.clone()

    def check(self, interior=True, in_place=True):
        assert self.fill is not None, f"{self.label}: check() before poison()"
        for name, lo, hi in (("front", 0, G), ("back", G + self.need, G + self.need + G)):
            got, want = self.full[lo:hi], self.fill[lo:hi]
            if not torch.equal(got, want):
                at = int(torch.nonzero(got != want)[0].item())
                where = at - G if name == "front" else at
                raise AssertionError(f"{self.label}: the {name} guard was written to, first at byte {where} "
                                     f"{'before the start' if name == 'front' else 'past the end'} of the {self.need}-byte workspace")
        if in_place:
            cur = self.get()
            assert cur is not None and cur.data_ptr() == self.view.data_ptr() and cur.numel() == self.need, \
                f"{self.label}: the cache no longer holds the guarded view (the call ran on another tensor: vacuous)"
        if interior and self.need > 0:
            assert not torch.equal(self.view, self.fill[G: G + self.need]), \
                f"{self.label}: no byte of the workspace differs from the fill (the call did not use it: vacuous)"


def _raw_slots(owner):
    """[(label, tensor, get, put)] of every cached workspace of ``owner``."""
    out = []
    if hasattr(owner, "cached_workspaces"):
        for key, ws in owner.cached_workspaces().items():
            out.append((f"workspace {key}", ws, lambda key=key: owner.cached_workspaces().get(key),
                        lambda v, key=key: owner.replace_cached_workspace(key, v)))
    elif isinstance(owner, dict):
        for key, ws in list(owner.items()):
            out.append((f"merge workspace {key}", ws, lambda key=key: owner.get(key),
                        lambda v, key=key: owner.__setitem__(key, v)))
    elif isinstance(getattr(owner, "_ws", None), list):
        for i, ws in enumerate(owner._ws):
            out.append((f"pipeline slot {i}", ws, lambda i=i: owner._ws[i], lambda v, i=i: owner._ws.__setitem__(i, v)))
    elif hasattr(owner, "_probe_buf") and hasattr(owner, "_ivf_ws"):
        for attr in ("_probe_buf", "_ivf_ws"):
            ws = getattr(owner, attr)
            if ws is not None:
                out.append((attr, ws, lambda attr=attr: getattr(owner, attr), lambda v, attr=attr: setattr(owner, attr, v)))
    else:
        raise TypeError(f"wsguard does not know the workspaces of a {type(owner).__name__}")
    return out


def guard(owner):
    """Swap every cached workspace tensor of ``need`` bytes for the view ``[G : G + need]`` of a fresh ``G + need + G``-byte
    buffer, under the same key (and tuning epoch): the library then receives exactly ``need`` bytes with guards on both
    sides.  Returns the number of workspaces guarded.  Call ``poison`` before the call under test."""
    slots = []
    for label, ws, get, put in _raw_slots(owner):
        assert ws.dtype == torch.uint8 and ws.dim() == 1 and ws.is_contiguous(), label
        slot = _Slot(label, ws.numel(), ws.device, get, put)
        put(slot.view)
        slots.append(slot)
    _registry[id(owner)] = (owner, slots)
    return len(slots)


def poison(owner, pattern, seed=0):
    """Refill the interior and the guards of every guarded workspace of ``owner`` with ``pattern`` (``PATTERNS``)."""
    for i, slot in enumerate(_registry[id(owner)][1]):
        slot.poison(pattern, seed + i)


def check(owner, interior=True, in_place=True):
    """Both guards of every workspace are byte for byte what ``poison`` wrote; the cache still holds the guarded view, same
    ``data_ptr`` and ``numel`` (``in_place``); a workspace of non-zero size has at least one byte that differs from the fill
    (``interior``).  ``AssertionError`` names the workspace and the first disturbed byte."""
    owner_, slots = _registry[id(owner)]
    assert owner_ is owner
    for slot in slots:
        slot.check(interior=interior, in_place=in_place)
    return len(slots)


def release(owner):
    """Forget the guards of ``owner`` (the views stay where they are; a later ``guard`` wraps them afresh)."""
    _registry.pop(id(owner), None)


class GuardedBuffer:
    """A caller-owned buffer of ``need`` bytes for a direct C-ABI call, guarded and poisoned like a cached workspace."""

    def __init__(self, need, device, pattern, label="buffer", seed=0):
        self._slot = _Slot(label, need, device, lambda: self._slot.view, lambda v: None)
        self._slot.poison(pattern, seed)
        self.view = self._slot.view

    def check(self, interior=True):
        self._slot.check(interior=interior, in_place=False)


class GuardedOutput:
    """An output tensor of ``shape`` as the middle rows of a larger one, every byte prefilled with ``SENTINEL``: ``pad`` guard
    rows (elements, for a 1-D output) in front and behind.  ``mid`` is contiguous and is what the call gets."""

    def __init__(self, shape, dtype, device, pad=None, label="output"):
        shape = tuple(int(s) for s in shape)
        self.label = label
        self.pad = (8 if len(shape) > 1 else 64) if pad is None else int(pad)
        self.rows = shape[0]
        self.full = torch.empty((self.rows + 2 * self.pad,) + shape[1:], dtype=dtype, device=device)
        self.full.view(torch.uint8).fill_(SENTINEL)
        self.mid = self.full[self.pad: self.pad + self.rows]

    def _bytes(self, t):
        return t.contiguous().view(torch.uint8)

    def check_guards(self):
        for name, part in (("in front of", self.full[: self.pad]), ("behind", self.full[self.pad + self.rows:])):
            assert bool((self._bytes(part) == SENTINEL).all()), f"{self.label}: the guard rows {name} the output were written to"

    def check_written(self):
        """Every element was written: none still holds the sentinel bytes (no id and no score a call returns has them)."""
        if self.mid.numel() == 0:
            return
        b = self._bytes(self.mid).view(-1, self.mid.element_size())
        still = (b == SENTINEL).all(dim=1)
        assert not bool(still.any()), \
            f"{self.label}: {int(still.sum())} of {still.numel()} elements were never written (first {int(torch.nonzero(still)[0])})"

    def check(self):
        self.check_guards()
        self.check_written()


def check_ids(ids, n, allow_empty=False, lo=0):
    """ids lie in ``[lo, lo + n)``; ``allow_empty``: or are the -1 of an empty per-query list."""
    a = ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
    ok = (a >= lo) & (a < lo + n)
    if allow_empty:
        ok |= a == -1
    assert ok.all(), f"ids outside [{lo}, {lo + n}): {a[~ok][:8].tolist()}"


def bits(t):
    """A tensor (or array) as host bytes: two results are bit-equal iff these are equal (NaN payloads and -0 included)."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy(), a.shape


def assert_bit_equal(got, want, what=""):
    """Two tuples of tensors / arrays are equal bit for bit, element by element of the tuple."""
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        (gb, gs), (wb, ws) = bits(g), bits(w)
        assert gs == ws, f"{what}: item {i} has shape {gs}, base {ws}"
        if not np.array_equal(gb, wb):
            at = int(np.flatnonzero(gb != wb)[0])
            raise AssertionError(f"{what}: item {i} differs from the base result, first at byte {at} of {gb.size} "
                                 f"({int(np.count_nonzero(gb != wb))} bytes differ)")
