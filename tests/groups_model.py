"""NumPy model of the near-duplicate groups (``dewi_groups_*``): connected components of an edge set over rows 0 .. n - 1.

Contract, as the header states it: a group's label is its smallest row; ``sizes[i]`` is the number of rows of row i's group;
the representative is the group's smallest row (``keep="first"``) or its row with the largest key (``keep="dewi"``: -0 == +0,
ties go to the lower row, a NaN key loses to every number, so it wins only in an all-NaN group).  Not a test module.
"""
import numpy as np


def labels_of(n, a, b):
    """Labels int64 [n] of the components of the edges (a[i], b[i]); self-loops and repeats are harmless."""
    parent = list(range(n))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(i) for i in range(n)], dtype=np.int64)


def representatives_of(labels, keep="first", key=None):
    labels = np.asarray(labels, dtype=np.int64)
    if keep == "first":
        return labels.copy()
    assert keep == "dewi" and key is not None
    key = np.asarray(key, dtype=np.float32)
    nan = np.isnan(key)
    clean = np.where(nan, np.float32(0), key) + np.float32(0)          # -0 -> +0
    rows = np.arange(labels.size)
    order = np.lexsort((rows, -clean.astype(np.float64), nan, labels))  # per label: numbers first, largest key, lowest row
    first = np.ones(labels.size, dtype=bool)
    first[1:] = labels[order][1:] != labels[order][:-1]
    best = np.zeros(labels.size, dtype=np.int64)
    best[labels[order][first]] = order[first]                            # indexed by label
    return best[labels]


def groups(n, a, b, keep="first", key=None):
    """``(labels, sizes, representatives, n_groups)`` of the edges over n rows."""
    labels = labels_of(n, a, b)
    sizes = np.bincount(labels, minlength=n).astype(np.int64)[labels] if n else np.zeros(0, np.int64)
    return labels, sizes, representatives_of(labels, keep, key), int(np.unique(labels).size)
