"""NumPy model of ``dewi_predicate_masks`` (include/dewi_hip.h) and a generator of valid postfix programs — a plain helper
module like ``parity.py``, not a test module.

``evaluate`` is vectorised over the rows (one bool array per stack slot); ``evaluate_naive`` in ``test_where_host.py`` runs the
same contract one row at a time and the two are held against each other there.
"""
import numpy as np

OPS = ("I_LT", "I_LE", "I_EQ", "I_NE", "I_GE", "I_GT", "I_BETWEEN", "I_ANY_BITS", "I_ALL_BITS", "I_IN_SET",
       "F_LT", "F_LE", "F_EQ", "F_NE", "F_GE", "F_GT", "F_BETWEEN", "F_IS_NAN", "TRUE", "AND", "OR", "NOT")
OP = {name: i for i, name in enumerate(OPS)}
INT_LEAVES = tuple(range(OP["I_LT"], OP["I_IN_SET"] + 1))
FLOAT_LEAVES = tuple(range(OP["F_LT"], OP["F_IS_NAN"] + 1))
MAX_INSTR, MAX_DEPTH = 64, 32

# values every test column holds somewhere: the edges of both formats
INT_EDGES = np.array([-(1 << 31), (1 << 31) - 1, -1, 0, 1, 2, 31, 32, 33, 63, 64, 100], dtype=np.int32)
FLOAT_EDGES = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, 1.0, -1.0, 0.5, 3.4028235e38],
                       dtype=np.float32)


def _i32(u):
    return np.int64(u) - (1 << 32) if int(u) >= (1 << 31) else np.int64(u)


def _f32(u):
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def leaf(op, x, a, b, sets):
    """One leaf op over a column: ``x`` the raw uint32 words [n] -> bool [n]."""
    xi = x.view(np.int32).astype(np.int64)
    xf = x.view(np.float32)
    ia, ib = _i32(a), _i32(b)
    name = OPS[op]
    with np.errstate(invalid="ignore"):
        if name == "I_LT": return xi < ia
        if name == "I_LE": return xi <= ia
        if name == "I_EQ": return xi == ia
        if name == "I_NE": return xi != ia
        if name == "I_GE": return xi >= ia
        if name == "I_GT": return xi > ia
        if name == "I_BETWEEN": return (xi >= ia) & (xi <= ib)
        if name == "I_ANY_BITS": return (x & np.uint32(a)) != 0
        if name == "I_ALL_BITS": return (x & np.uint32(a)) == np.uint32(a)
        if name == "I_IN_SET":
            ok = (xi >= 0) & (xi < int(b))
            out = np.zeros(x.shape, dtype=bool)
            v = xi[ok]
            out[ok] = ((sets[int(a) + (v >> 5)] >> (v & 31).astype(np.uint32)) & 1) != 0      # no word read for another x
            return out
        fa, fb = _f32(a), _f32(b)
        if name == "F_LT": return xf < fa
        if name == "F_LE": return xf <= fa
        if name == "F_EQ": return xf == fa
        if name == "F_NE": return xf != fa
        if name == "F_GE": return xf >= fa
        if name == "F_GT": return xf > fa
        if name == "F_BETWEEN": return (xf >= fa) & (xf <= fb)
        if name == "F_IS_NAN": return xf != xf
    raise ValueError(f"not a leaf op: {op}")


def words(column):
    """A column (int32 or float32 array) as its raw uint32 words."""
    c = np.ascontiguousarray(column)
    assert c.dtype in (np.int32, np.float32), c.dtype
    return c.view(np.uint32)


def evaluate(columns, types, program, sets, base=None):
    """``program``: a sequence of ``(op, column, a, b)``; ``columns``: int32 / float32 arrays [n]; ``types``: 0 int32, 1 fp32
    per column; ``sets``: uint32 words; ``base``: ``None`` or bytes [n] (non-zero = allowed).  Returns uint8 [n] of 0 / 1."""
    n = len(columns[0]) if columns else (len(base) if base is not None else 0)
    sets = np.asarray(sets, dtype=np.uint32)
    stack = []
    assert 1 <= len(program) <= MAX_INSTR
    for op, c, a, b in program:
        if op == OP["AND"]:
            y = stack.pop()
            stack[-1] = stack[-1] & y
        elif op == OP["OR"]:
            y = stack.pop()
            stack[-1] = stack[-1] | y
        elif op == OP["NOT"]:
            stack[-1] = ~stack[-1]
        elif op == OP["TRUE"]:
            stack.append(np.ones(n, dtype=bool))
        else:
            assert types[c] == (1 if op in FLOAT_LEAVES else 0), (OPS[op], c, types[c])
            stack.append(leaf(op, words(columns[c]), a, b, sets))
        assert len(stack) <= MAX_DEPTH
    assert len(stack) == 1
    out = stack[0]
    if base is not None:
        out = out & (np.asarray(base) != 0)
    return out.astype(np.uint8)


def random_sets(rs, n_sets=3, poison=True):
    """(words, [(first word, bits)]): ``n_sets`` random bitsets whose sizes are no multiples of 32, with all-ones poison words in
    front, between and behind them that belong to no set."""
    parts, where, at = [], [], 0
    for _ in range(n_sets):
        if poison:
            parts.append(np.full(1, 0xFFFFFFFF, dtype=np.uint32))
            at += 1
        bits = int(rs.choice([1, 5, 31, 33, 70, 100, 127]))
        w = rs.randint(0, 1 << 32, size=(bits + 31) // 32, dtype=np.uint64).astype(np.uint32)
        parts.append(w)
        where.append((at, bits))
        at += int(w.size)
    if poison:
        parts.append(np.full(1, 0xFFFFFFFF, dtype=np.uint32))
    return np.concatenate(parts), where


def random_leaf(rs, types, set_table):
    c = int(rs.randint(len(types)))
    if types[c] == 1:
        op = int(rs.choice(FLOAT_LEAVES))
        a, b = (int(v) for v in rs.choice(FLOAT_EDGES, 2).view(np.uint32))
        if rs.rand() < 0.5:
            a, b = (int(v) for v in np.sort(rs.randn(2).astype(np.float32)).view(np.uint32))
        return (op, c, a, b)
    ops = [o for o in INT_LEAVES if o != OP["I_IN_SET"] or set_table]
    op = int(rs.choice(ops))
    if op == OP["I_IN_SET"]:
        a, b = set_table[int(rs.randint(len(set_table)))]
        return (op, c, int(a), int(b))
    a, b = (int(v) for v in rs.choice(INT_EDGES, 2).view(np.uint32))
    if rs.rand() < 0.5:
        a, b = (int(v) for v in np.sort(rs.randint(-50, 150, 2).astype(np.int32)).view(np.uint32))
    return (op, c, a, b)


def random_program(rs, types, set_table=(), length=None, max_depth=MAX_DEPTH):
    """A valid postfix program of exactly ``length`` instructions (default: random in 1 .. 64) over columns of ``types``,
    whose stack never exceeds ``max_depth`` and ends at 1.  Leaves, NOTs and binary ops are drawn so that deep stacks — up
    to ``max_depth`` — do occur."""
    length = int(rs.randint(1, MAX_INSTR + 1)) if length is None else int(length)
    assert 1 <= length <= MAX_INSTR and 1 <= max_depth <= MAX_DEPTH
    out, depth = [], 0
    greedy = rs.rand() < 0.5                   # half of the programs climb as high as they can before folding
    for i in range(length):
        left = length - i                      # instructions still to write, this one included
        # after this instruction the depth d must come down to 1 with the left - 1 others: d - 1 <= left - 1
        can_push = depth < max_depth and depth + 1 <= left
        can_binary = depth >= 2
        can_not = depth >= 1 and depth <= left             # a NOT keeps the depth: depth - 1 <= left - 1
        must_fold = depth - 1 >= left - 1 and depth > 1     # only binary ops can still bring it down in time
        choices = []
        if must_fold:
            choices = ["bin"]
        else:
            if can_push:
                choices += ["leaf"] * (30 if greedy else 3)
            if can_binary:
                choices += ["bin"] * (1 if greedy else 3)
            if can_not and depth - 1 <= left - 2:
                choices += ["not"]
        if not choices:
            choices = ["leaf"] if depth == 0 else (["bin"] if can_binary else ["not"])
        pick = choices[int(rs.randint(len(choices)))]
        if pick == "leaf":
            if not types or rs.rand() < 0.05:
                out.append((OP["TRUE"], 0, 0, 0))
            else:
                out.append(random_leaf(rs, types, list(set_table)))
            depth += 1
        elif pick == "bin":
            out.append((OP["AND"] if rs.rand() < 0.5 else OP["OR"], 0, 0, 0))
            depth -= 1
        else:
            out.append((OP["NOT"], 0, 0, 0))
    assert depth == 1 and len(out) == length, (depth, len(out), length)
    return out


def edge_column(rs, n, kind, pad=0):
    """A column of ``pad + n`` values with the format's edge values mixed in: int32 (``kind`` 0) or float32 (1)."""
    m = pad + n
    if kind == 1:
        c = rs.randn(m).astype(np.float32)
        at = rs.rand(m) < 0.3
        c[at] = rs.choice(FLOAT_EDGES, int(at.sum()))
        return c
    c = rs.randint(-50, 150, m).astype(np.int32)
    at = rs.rand(m) < 0.3
    c[at] = rs.choice(INT_EDGES, int(at.sum()))
    return c
