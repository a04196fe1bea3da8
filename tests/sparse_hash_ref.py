"""The canonical hash reduce-by-key (K5c) once more, in plain Python: splitmix64 on ints, a list for
the table, a dict for the runs.  No torch, no numpy, nothing shared with the code under test.

Definition: for ``n`` rows the table has ``t`` = the smallest power of two >= max(1024, 2n) slots;
``home(k) = splitmix64(k mod 2**64) & (t - 1)``; the canonical table is what plain linear probing
builds when the distinct keys other than -1 are inserted in ascending unsigned 64-bit order.  The
output lists the occupied slots in ascending slot order, then the run of rows keyed -1 (the table's
EMPTY marker) if there is one; a run's rows combine in ascending input index."""

M64 = (1 << 64) - 1
EMPTY = M64


def splitmix64(k: int) -> int:
    k &= M64
    k ^= k >> 30
    k = (k * 0xBF58476D1CE4E5B9) & M64
    k ^= k >> 27
    k = (k * 0x94D049BB133111EB) & M64
    k ^= k >> 31
    return k


def table_slots(n: int) -> int:
    t = 1024
    while t < 2 * n:
        t *= 2
    return t


def home(key: int, t: int) -> int:
    return splitmix64(key) & (t - 1)


def canonical_table(keys, n=None):
    """The table (a list of t entries: the key as a signed int, or None) for the rows' keys."""
    n = len(keys) if n is None else n
    t = table_slots(n)
    table = [None] * t
    for u in sorted({k & M64 for k in keys} - {EMPTY}):
        h = home(u, t)
        while table[h] is not None:
            h = (h + 1) % t
        table[h] = u - (1 << 64) if u >> 63 else u
    return table


def canonical_order(keys):
    """The distinct keys in output order."""
    out = [k for k in canonical_table(keys) if k is not None]
    if any(k == -1 for k in keys):
        out.append(-1)
    return out


def canonical_rbk(keys, rows, combine):
    """(keys, rows, counts) in output order; ``rows[i]`` is a list, ``combine(a, b)`` folds two
    elements, applied along every run in ascending input index."""
    runs = {}
    for i, k in enumerate(keys):
        runs.setdefault(k, []).append(i)
    order = canonical_order(keys)
    out_rows = []
    for k in order:
        idx = runs[k]
        acc = list(rows[idx[0]])
        for i in idx[1:]:
            acc = [combine(a, b) for a, b in zip(acc, rows[i])]
        out_rows.append(acc)
    return order, out_rows, [len(runs[k]) for k in order]


def keys_with_homes(t: int, lo: int, hi: int, count: int, start: int = 1, step: int = 0x10001):
    """``count`` distinct positive keys whose homes in a table of ``t`` slots lie in [lo, hi]."""
    out, k = [], start
    while len(out) < count:
        if lo <= home(k, t) <= hi:
            out.append(k)
        k += step
    return out
