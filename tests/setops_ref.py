"""Reference for the set operations between two sorted runs (kc.h kc_combine_*)
over structured numpy records (key: W little-endian u64 words, word 0 most
significant; cnt: u32). combine() is written with dicts keyed by the key tuple
and a sort at the end: it merges nothing and cuts no tiles, so it shares no
idea with the kernel. combine_vec() is the same function for sizes where the
dicts are slow (membership through a sorted concatenation); test_setops_host
pins it to combine()."""
import numpy as np

U32 = 0xFFFFFFFF
UNION, INTERSECT, SUBTRACT, COUNT_SUBTRACT = 0, 1, 2, 3
SUM, MIN, MAX, LEFT, RIGHT = 0, 1, 2, 3, 4
OPS = {"union": UNION, "intersect": INTERSECT, "subtract": SUBTRACT, "count_subtract": COUNT_SUBTRACT}
MODES = {"sum": SUM, "min": MIN, "max": MAX, "left": LEFT, "right": RIGHT}
OP_NAMES = {v: k for k, v in OPS.items()}
MODE_NAMES = {v: k for k, v in MODES.items()}
# every (op, mode) the interface accepts: the subtractions take SUM only
CASES = [(op, m) for op in (UNION, INTERSECT) for m in (SUM, MIN, MAX, LEFT, RIGHT)] + [(SUBTRACT, SUM),
                                                                                      (COUNT_SUBTRACT, SUM)]


def rec_dtype(W):
    return np.dtype([("key", "<u8", (W,)), ("cnt", "<u4")])


def _both(mode, a, b):
    return {SUM: (a + b) & U32, MIN: min(a, b), MAX: max(a, b), LEFT: a, RIGHT: b}[mode]


def combine(a, b, op, mode):
    """The records of `a` op `b` (the module's semantics), sorted by key."""
    W = a["key"].shape[1]
    da = {tuple(int(x) for x in k): int(c) for k, c in zip(a["key"], a["cnt"])}
    db = {tuple(int(x) for x in k): int(c) for k, c in zip(b["key"], b["cnt"])}
    assert len(da) == len(a) and len(db) == len(b), "one record per key"
    out = {}
    if op == UNION:
        for k in set(da) | set(db):
            out[k] = _both(mode, da[k], db[k]) if k in da and k in db else da.get(k, db.get(k))
    elif op == INTERSECT:
        for k in set(da) & set(db):
            out[k] = _both(mode, da[k], db[k])
    elif op == SUBTRACT:
        for k in set(da) - set(db):
            out[k] = da[k]
    elif op == COUNT_SUBTRACT:
        for k, c in da.items():
            if k not in db:
                out[k] = c
            elif c > db[k]:
                out[k] = c - db[k]
    else:
        raise ValueError(op)
    r = np.zeros(len(out), dtype=rec_dtype(W))
    for i, k in enumerate(sorted(out)):  # tuples of ints: word 0 first, unsigned
        r["key"][i] = k
        r["cnt"][i] = out[k]
    return r


def lexorder(key):
    """Stable argsort of (n, W) u64 keys, word 0 most significant."""
    return np.lexsort([key[:, j] for j in range(key.shape[1] - 1, -1, -1)])


def combine_vec(a, b, op, mode):
    """combine() without Python loops over the records."""
    W = a["key"].shape[1]
    na, nb = len(a), len(b)
    key = np.concatenate([a["key"], b["key"]])
    order = lexorder(key)  # stable: of two equal keys a's record comes first
    sk = key[order]
    same = np.zeros(na + nb, dtype=bool)  # equal to the record before it
    if na + nb > 1:
        same[1:] = (sk[1:] == sk[:-1]).all(axis=1)
    first = ~same
    has_next = np.zeros(na + nb, dtype=bool)
    has_next[:-1] = same[1:]
    from_a = order < na
    cnt = np.concatenate([a["cnt"], b["cnt"]]).astype(np.uint64)[order]
    nxt = np.zeros(na + nb, dtype=np.uint64)
    nxt[:-1] = cnt[1:]
    pair = first & has_next  # a's record of a shared key; nxt is b's count
    ca, cb = cnt, nxt
    both = {SUM: (ca + cb) & np.uint64(U32), MIN: np.minimum(ca, cb), MAX: np.maximum(ca, cb), LEFT: ca,
            RIGHT: cb}[mode]
    only = first & ~has_next
    if op == UNION:
        keep, val = first, np.where(pair, both, cnt)
    elif op == INTERSECT:
        keep, val = pair, both
    elif op == SUBTRACT:
        keep, val = only & from_a, cnt
    elif op == COUNT_SUBTRACT:
        keep = (only & from_a) | (pair & (ca > cb))
        val = np.where(pair, ca - np.minimum(ca, cb), cnt)
    else:
        raise ValueError(op)
    r = np.zeros(int(keep.sum()), dtype=rec_dtype(W))
    r["key"] = sk[keep]
    r["cnt"] = val[keep].astype(np.uint32)
    return r


def merged_positions(a, b):
    """from_a[p] and the source index idx[p] of position p of the merge of a
    and b with a's record first at equal keys."""
    na = len(a)
    order = lexorder(np.concatenate([a["key"], b["key"]]))
    from_a = order < na
    return from_a, np.where(from_a, order, order - na)


# ---- crafted runs (shared by the host and the GPU tests) ---------------------

COUNT_POOL = np.array([0, 1, 2, U32 - 1, U32], dtype=np.uint32)


def key_pool(W, m, seed):
    """m distinct sorted keys. Leading words come from {0, 1, 2}, so many keys
    share words 0..W-2 and differ only in the last word (a comparison that
    stops early is caught at W >= 2); last words are even and >= 2, so the
    0^W key is not among them."""
    rng = np.random.default_rng(seed)
    key = np.zeros((m, W), dtype=np.uint64)
    for j in range(W - 1):
        key[:, j] = rng.integers(0, 3, m, dtype=np.uint64)
    key[:, W - 1] = 2 * rng.choice(1 << 20, m, replace=False).astype(np.uint64) + 2
    return key[lexorder(key)]


def run_of(keys, seed, hole=False, counts=COUNT_POOL):
    """A run over the given sorted keys with counts drawn from `counts`; with
    `hole`, the 0^W hole record (count 0) comes first."""
    rng = np.random.default_rng(seed)
    h = 1 if hole else 0
    r = np.zeros(len(keys) + h, dtype=rec_dtype(keys.shape[1]))
    r["key"][h:] = keys
    r["cnt"][h:] = counts[rng.integers(0, len(counts), len(keys))]
    return r


def split_runs(W, n_total, seed, shared=1 / 3, hole=(False, False)):
    """Two runs with n_total records together (the hole records included),
    about `shared` of the keys in both, the rest dealt at random."""
    rng = np.random.default_rng(seed)
    n = n_total - int(hole[0]) - int(hole[1])
    assert n >= 0
    ns = int(n * shared / (1 + shared))  # shared keys: each is a record of both runs
    pool = key_pool(W, n - ns, seed + 1)
    tag = rng.permutation(np.concatenate([np.full(ns, 2), rng.integers(0, 2, n - 2 * ns)]))
    a = run_of(pool[tag != 1], seed + 2, hole[0])
    b = run_of(pool[tag != 0], seed + 3, hole[1])
    assert len(a) + len(b) == n_total
    return a, b
