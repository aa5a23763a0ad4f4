"""Predicates over the attribute columns of an index (additive; the reference has no counterpart) — host logic only.

    from dewi.where import col
    w = (col("year") >= 2020) & col("site").isin(["a.org", "b.org"]) & (col("noise") < 0.2)
    index.search(q, k=10, filter=w)

``col(name)`` names an attribute column (``ExactIndex.set_attributes``); comparisons on it make a ``Where`` and ``&``, ``|``,
``~`` combine them.  Python gives ``&`` and ``|`` a HIGHER precedence than comparisons, so every comparison wants its
parentheses.  ``Where.compile(index)`` resolves names, kinds and vocabularies into the postfix program that
``dewi_predicate_masks`` (include/dewi_hip.h) evaluates on the device; nothing here touches a device.

What a column takes:

* int columns (integers, bools): ``<  <=  ==  !=  >=  >``, ``between(lo, hi)`` (inclusive), ``isin(ints)``, ``any_bits(m)``,
  ``all_bits(m)``, with integer constants inside int32;
* float columns (fp32): ``<  <=  ==  !=  >=  >``, ``between(lo, hi)``, ``isnan()``.  A constant is rounded with ``np.float32``
  first and the comparison is ``fp32(x) op fp32(c)``, with IEEE rules: every comparison with a NaN is false except ``!=``,
  -0 equals +0 (so ``~(x < c)`` holds for a NaN row where ``x >= c`` does not);
* categorical columns (strings): ``==``, ``!=``, ``isin(strings)``; ``None`` is the missing value.  A string that is not in
  the column's vocabulary matches nothing: it compiles to a comparison against a code no row holds.

``ValueError`` (before any device work): an unknown column, a string against a column that is not categorical, a float
operator or constant on an int column, a bit or set operator on a float column, a constant outside int32, ``isin`` codes that
are negative or 2^24 and above, a program of more than 64 instructions or deeper than 32.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._native import PRED_MAX_COLUMNS, PRED_MAX_DEPTH, PRED_MAX_INSTR, PRED_MAX_PROGRAMS, PRED_OP_CODES

#: the largest value an ``isin`` set may hold, exclusive: its bitset has one bit per value from 0 on
ISIN_MAX_VALUE = 1 << 24
_CMP = ("lt", "le", "eq", "ne", "ge", "gt")
Instr = Tuple[int, int, int, int]          # (op, column, a, b) — dewi_pred_instr


@dataclasses.dataclass
class Program:
    """Compiled predicates: ``columns`` the attribute names the instructions index, ``programs`` one list of
    ``(op, column, a, b)`` per predicate, ``sets`` the uint32 words of every ``isin`` bitset, concatenated."""

    columns: List[str]
    programs: List[List[Instr]]
    sets: np.ndarray


class Where:
    """A predicate over attribute columns: made by comparisons on ``col(name)``, combined with ``&``, ``|`` and ``~``."""

    def __and__(self, other: "Where") -> "Where":
        return _Node("AND", (self, _where(other)))

    def __or__(self, other: "Where") -> "Where":
        return _Node("OR", (self, _where(other)))

    def __invert__(self) -> "Where":
        return _Node("NOT", (self,))

    def __bool__(self) -> bool:
        raise TypeError("a Where has no truth value: combine predicates with & | ~ (and parenthesise the comparisons)")

    def compile(self, index) -> Program:
        """The postfix program of this predicate for ``index`` — an index with attributes, or its schema
        ``{name: (kind, vocabulary)}`` with kind ``"int"`` / ``"float"`` / ``"cat"`` and the vocabulary a sequence of strings
        (code = position) or ``None``."""
        return compile_programs([self], index)


def _where(x) -> Where:
    if not isinstance(x, Where):
        raise TypeError(f"expected a Where, got {type(x).__name__} (parenthesise comparisons: (col('a') > 1) & (col('b') < 2))")
    return x


class _Node(Where):
    def __init__(self, op: str, args: Tuple[Where, ...]):
        self.op, self.args = op, args

    def __repr__(self) -> str:
        if self.op == "NOT":
            return f"~{self.args[0]!r}"
        return f"({self.args[0]!r} {'&' if self.op == 'AND' else '|'} {self.args[1]!r})"


class _Leaf(Where):
    def __init__(self, name: str, op: str, args: tuple):
        self.name, self.op, self.args = name, op, args

    def __repr__(self) -> str:
        return f"col({self.name!r}).{self.op}{self.args!r}"


class Col:
    """An attribute column by name (``col(name)``): its comparisons make ``Where`` leaves."""

    __hash__ = None

    def __init__(self, name: str):
        if not isinstance(name, str):
            raise TypeError(f"a column is named by a string, got {type(name).__name__}")
        self.name = name

    def __lt__(self, c): return _Leaf(self.name, "lt", (c,))
    def __le__(self, c): return _Leaf(self.name, "le", (c,))
    def __eq__(self, c): return _Leaf(self.name, "eq", (c,))
    def __ne__(self, c): return _Leaf(self.name, "ne", (c,))
    def __ge__(self, c): return _Leaf(self.name, "ge", (c,))
    def __gt__(self, c): return _Leaf(self.name, "gt", (c,))

    def between(self, lo, hi) -> Where:
        """``lo <= x <= hi``, both ends included."""
        return _Leaf(self.name, "between", (lo, hi))

    def isin(self, values) -> Where:
        """x is one of ``values``: integers in [0, 2^24) for an int column, strings (or ``None``) for a categorical one."""
        return _Leaf(self.name, "isin", (list(values),))

    def any_bits(self, mask: int) -> Where:
        """``(x & mask) != 0``."""
        return _Leaf(self.name, "any_bits", (mask,))

    def all_bits(self, mask: int) -> Where:
        """``(x & mask) == mask``."""
        return _Leaf(self.name, "all_bits", (mask,))

    def isnan(self) -> Where:
        return _Leaf(self.name, "isnan", ())


def col(name: str) -> Col:
    return Col(name)


def always() -> Where:
    """The predicate every row passes."""
    return _Leaf("", "true", ())


# ---------------------------------------------------------------------------------------------------------------- compile
def schema_of(index) -> Dict[str, Tuple[str, Optional[Dict[str, int]]]]:
    """``{name: (kind, {string: code} or None)}`` of an index (``attribute_schema()``) or of a plain schema mapping."""
    raw = index.attribute_schema() if hasattr(index, "attribute_schema") else index
    out = {}
    for name, (kind, vocab) in raw.items():
        if kind not in ("int", "float", "cat"):
            raise ValueError(f"column {name!r}: unknown kind {kind!r}")
        if kind == "cat" and not isinstance(vocab, dict):
            vocab = {s: i for i, s in enumerate(vocab or ())}
        out[name] = (kind, vocab if kind == "cat" else None)
    return out


def _is_int(c) -> bool:
    return isinstance(c, (int, np.integer, bool, np.bool_)) and not isinstance(c, (float, np.floating))


def _i32(c, what: str) -> int:
    if not _is_int(c):
        raise ValueError(f"{what}: an int column takes integer constants, got {c!r}")
    v = int(c)
    if not -(1 << 31) <= v < (1 << 31):
        raise ValueError(f"{what}: constant {v} outside int32")
    return v & 0xFFFFFFFF


def _bits_mask(c, what: str) -> int:
    if not _is_int(c):
        raise ValueError(f"{what}: a bit mask is an integer, got {c!r}")
    v = int(c)
    if not -(1 << 31) <= v < (1 << 32):
        raise ValueError(f"{what}: mask {v} outside 32 bits")
    return v & 0xFFFFFFFF


def _f32(c, what: str) -> int:
    if isinstance(c, (str, bytes)) or c is None:
        raise ValueError(f"{what}: a float column takes numbers, got {c!r}")
    with np.errstate(over="ignore"):
        return int(np.asarray(np.float32(c)).view(np.uint32))


class _Emitter:
    def __init__(self, schema):
        self.schema = schema
        self.columns: List[str] = []
        self.sets: List[np.ndarray] = []
        self.set_words = 0

    def column(self, name: str) -> Tuple[int, str, Optional[Dict[str, int]]]:
        if name not in self.schema:
            raise ValueError(f"unknown attribute column {name!r} (the index has {sorted(self.schema)})")
        if name not in self.columns:
            if len(self.columns) >= PRED_MAX_COLUMNS:
                raise ValueError(f"predicates of one call name more than {PRED_MAX_COLUMNS} columns")
            self.columns.append(name)
        kind, vocab = self.schema[name]
        return self.columns.index(name), kind, vocab

    def bitset(self, values: Sequence[int], what: str) -> Tuple[int, int]:
        """(first word, bits) of a new set holding ``values``."""
        vals = sorted(set(values))
        if vals and (vals[0] < 0 or vals[-1] >= ISIN_MAX_VALUE):
            raise ValueError(f"{what}: isin values must lie in [0, {ISIN_MAX_VALUE}), got {vals[0]} .. {vals[-1]}")
        bits = vals[-1] + 1 if vals else 0
        words = np.zeros((bits + 31) // 32, dtype=np.uint32)
        v = np.asarray(vals, dtype=np.int64)
        np.bitwise_or.at(words, v >> 5, (np.uint32(1) << (v & 31).astype(np.uint32)))
        first = self.set_words
        self.sets.append(words)
        self.set_words += int(words.size)
        return first, bits

    def leaf(self, w: _Leaf, out: List[Instr]) -> None:
        ops = PRED_OP_CODES
        if w.op == "true":
            out.append((ops["TRUE"], 0, 0, 0))
            return
        c, kind, vocab = self.column(w.name)
        what = f"col({w.name!r}).{w.op}"
        strings = [a for a in (w.args[0] if w.op == "isin" else w.args) if isinstance(a, str)]
        if strings and kind != "cat":
            raise ValueError(f"{what}: column {w.name!r} is not categorical, it cannot be compared with the string {strings[0]!r}")
        if kind == "cat":
            missing = len(vocab)                                   # a code no row holds: codes are -1 .. len - 1

            def code(s):
                if s is None:
                    return -1
                if not isinstance(s, str):
                    raise ValueError(f"{what}: a categorical column is compared with strings or None, got {s!r}")
                return vocab.get(s, missing)
            if w.op in ("eq", "ne"):
                out.append((ops["I_EQ" if w.op == "eq" else "I_NE"], c, code(w.args[0]) & 0xFFFFFFFF, 0))
            elif w.op == "isin":
                codes = [code(s) for s in w.args[0]]
                first, bits = self.bitset([v for v in codes if 0 <= v < missing], what)
                out.append((ops["I_IN_SET"], c, first, bits))
                if -1 in codes:
                    out.append((ops["I_EQ"], c, 0xFFFFFFFF, 0))
                    out.append((ops["OR"], 0, 0, 0))
            else:
                raise ValueError(f"{what}: a categorical column takes ==, != and isin")
            return
        if kind == "int":
            if w.op in _CMP:
                out.append((ops["I_" + w.op.upper()], c, _i32(w.args[0], what), 0))
            elif w.op == "between":
                out.append((ops["I_BETWEEN"], c, _i32(w.args[0], what), _i32(w.args[1], what)))
            elif w.op in ("any_bits", "all_bits"):
                out.append((ops["I_" + w.op.upper()], c, _bits_mask(w.args[0], what), 0))
            elif w.op == "isin":
                if not all(_is_int(v) for v in w.args[0]):
                    raise ValueError(f"{what}: an int column takes integer values")
                first, bits = self.bitset([int(v) for v in w.args[0]], what)
                out.append((ops["I_IN_SET"], c, first, bits))
            else:
                raise ValueError(f"{what}: column {w.name!r} holds integers ({w.op} is a float operator)")
            return
        if w.op in _CMP:
            out.append((ops["F_" + w.op.upper()], c, _f32(w.args[0], what), 0))
        elif w.op == "between":
            out.append((ops["F_BETWEEN"], c, _f32(w.args[0], what), _f32(w.args[1], what)))
        elif w.op == "isnan":
            out.append((ops["F_IS_NAN"], c, 0, 0))
        else:
            raise ValueError(f"{what}: column {w.name!r} holds floats ({w.op} is an integer operator)")

    def emit(self, w: Where, out: List[Instr]) -> None:
        if isinstance(w, _Leaf):
            self.leaf(w, out)
        elif isinstance(w, _Node):
            for a in w.args:
                self.emit(a, out)
            out.append((PRED_OP_CODES[w.op], 0, 0, 0))
        else:
            raise TypeError(f"expected a Where, got {type(w).__name__}")


def program_depth(program: Sequence[Instr]) -> int:
    """The deepest stack a postfix program reaches; ``ValueError`` when it pops an empty stack or does not end with one value."""
    depth = deepest = 0
    for op, _, _, _ in program:
        if op in (PRED_OP_CODES["AND"], PRED_OP_CODES["OR"]):
            if depth < 2:
                raise ValueError("program pops an empty stack")
            depth -= 1
        elif op == PRED_OP_CODES["NOT"]:
            if depth < 1:
                raise ValueError("program pops an empty stack")
        else:
            depth += 1
            deepest = max(deepest, depth)
    if depth != 1:
        raise ValueError(f"program ends with {depth} values on the stack, not 1")
    return deepest


def compile_programs(wheres: Sequence[Where], index) -> Program:
    """Compile predicates that one ``dewi_predicate_masks`` call evaluates together: they share the column table and the set
    words.  ``ValueError`` for everything the module docstring lists."""
    wheres = list(wheres)
    if not 1 <= len(wheres) <= PRED_MAX_PROGRAMS:
        raise ValueError(f"one call takes 1 .. {PRED_MAX_PROGRAMS} predicates, got {len(wheres)}")
    em = _Emitter(schema_of(index))
    programs = []
    for j, w in enumerate(wheres):
        out: List[Instr] = []
        em.emit(_where(w), out)
        if len(out) > PRED_MAX_INSTR:
            raise ValueError(f"predicate {j} compiles to {len(out)} instructions (at most {PRED_MAX_INSTR})")
        if program_depth(out) > PRED_MAX_DEPTH:
            raise ValueError(f"predicate {j} needs a stack deeper than {PRED_MAX_DEPTH}")
        programs.append(out)
    sets = np.concatenate(em.sets) if em.sets else np.zeros(0, np.uint32)
    return Program(em.columns, programs, sets.astype(np.uint32))


def is_where_list(x) -> bool:
    """A non-empty list / tuple of ``Where``s: per-query predicates."""
    return isinstance(x, (list, tuple)) and len(x) > 0 and all(isinstance(w, Where) for w in x)


__all__ = ["Where", "Col", "col", "always", "Program", "compile_programs", "program_depth", "schema_of", "is_where_list",
           "ISIN_MAX_VALUE"]
