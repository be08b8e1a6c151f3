"""Kernel-level tests of the key-prefix (partition) engine: P1 / P2
(count_front<W, SINK_HIST> and <W, SINK_SCATTER> behind launch_part_hist and
launch_part_scatter), the group histograms (hist_group_sum_k,
hist_group_totals_k), P5 (count_buckets<W>) and P5s (sort_runs_k<W>, with
packed_seg_copy_k closing the gaps of its direct mode), driven through
libkc_kernel_shim.so (tools/kc_kernel_shim.cpp). The references are plain
numpy (tests/kernel_ref.py: p5_runs_ref, check_segments, part_front_ref,
checked on the CPU by tests/test_kernel_ref.py); everything is integers, so
every comparison is exact.

The engine gives the same bytes whatever these kernels decide: a P5 pass that
aborts or falls back without need, a descriptor whose digit shift is too
coarse, a P5s that flags a run it could sort all cost time and keep the counts
right, so the end-to-end byte comparisons cannot see them. These tests pin
them at the kernel, at a few thousand keys.

Edge sizes come from the library (kcs_bucket_lds_slots, kcs_sort_runs_keys,
kcs_part_geometry, kcs_n_cu). One constant is copied: MAX_SORT_BIN = 48, the
largest bin sort_runs_k sorts (kMaxSortBin in kc_kernels.hip, which
kc_device.h does not declare). What depends on race timing (the m chosen
after an abort, which keys a full table pushes to the fallback, the order of
records inside an unsorted segment) is asserted by its invariants only.
"""
import ctypes
import os

import numpy as np
import pytest

import kernel_ref as kr
import skm_reads

pytestmark = pytest.mark.gpu

U64 = np.uint64
FILL = 0xEE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_PATH = os.path.join(ROOT, "kmer-counter_amd", "libkc_kernel_shim.so")
MAX_SORT_BIN = 48  # kMaxSortBin (kc_kernels.hip): the one constant copied here
WS = (1, 2, 3, 4)

ST_NAMES = ("ST_VALID", "ST_KEY0", "ST_KEY0_PRESENT", "ST_CLAIMED", "ST_ERR", "ST_SPILL2_FILL", "ST_P5_PASSES",
            "ST_P5_ABORTS", "ST_P5_KEYS", "ST_DEDUP", "ST_P5_MAXM", "ST_DESC_FILL")
ST_VALID = ST_KEY0 = ST_KEY0_PRESENT = ST_CLAIMED = ST_ERR = ST_SPILL2_FILL = None
ST_P5_PASSES = ST_P5_ABORTS = ST_P5_KEYS = ST_DEDUP = ST_P5_MAXM = ST_DESC_FILL = None


class Shim:
    def __init__(self, kca):
        kca.lib()  # libkc_hip.so first: the shim links it
        if not os.path.exists(SHIM_PATH):
            raise ImportError(f"{SHIM_PATH} is missing: run `make -C kmer-counter_amd`")
        L = ctypes.CDLL(SHIM_PATH)
        vp, u64, u32, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        L.kcs_bucket_lds_slots.argtypes = [i]
        L.kcs_sort_runs_keys.argtypes = [i]
        L.kcs_seg_sort_cap.argtypes = [i]
        L.kcs_err_spill_overflow.restype = u64
        L.kcs_err_rec_overflow.restype = u64
        L.kcs_stat_indices.argtypes = [vp]
        L.kcs_count_buckets.argtypes = [i, vp, u64, vp, u32, vp, vp, vp, u32, i, u32, i, u64, u64, u64, u32, u64, i,
                                        vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.kcs_sort_runs.argtypes = [i, vp, u64, vp, u32, i, u64, u64, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i,
                                    u64, vp]
        L.kcs_packed_seg_copy.argtypes = [i, u64, vp, u64, vp, u64, vp, vp, vp, vp, u64, i, i]
        L.kcs_seg_sort.argtypes = [i, u64, vp, vp, u64, u64, vp, vp, vp, vp, vp, u64, i, i, vp, vp, i, vp, vp, vp]
        L.kcs_part_geometry.argtypes = [i, i, u64, vp]
        L.kcs_part_front.argtypes = [vp, u64, i, i, i, i, u32, u32, i, i, vp, i, vp, u64, i, i, u32, vp, u64, i, vp,
                                     vp, vp, vp, vp]
        L.kcs_hist_group.argtypes = [vp, u64, u32, u32, i, vp, vp]
        self.L = L
        self.n_cu = L.kcs_n_cu()
        assert self.n_cu > 0
        self.st_n = L.kcs_st_n()
        L.kcs_stat_indices_p5.argtypes = [vp]
        idx = np.full(len(ST_NAMES) + 1, -7, dtype=np.int32)  # ten from kcs_stat_indices, two from its P5 companion
        assert L.kcs_stat_indices(idx.ctypes.data) == 0
        assert idx[10] == -7, "kcs_stat_indices wrote past its ten entries"
        assert L.kcs_stat_indices_p5(idx[10:].ctypes.data) == 0
        assert idx[12] == -7
        idx = idx[:12]
        assert len(set(idx.tolist())) == idx.size and 0 <= idx.min() and idx.max() < self.st_n
        globals().update(zip(ST_NAMES, (int(x) for x in idx)))
        self.invalid = L.kcs_invalid_value()
        assert self.invalid != 0
        self.err_spill = L.kcs_err_spill_overflow()
        self.err_rec = L.kcs_err_rec_overflow()

    def lds_slots(self, W):
        s = self.L.kcs_bucket_lds_slots(W)
        assert s >= 1024 and s % 64 == 0
        return s

    def sr_keys(self, W):
        s = self.L.kcs_sort_runs_keys(W)
        assert 1024 <= s <= self.L.kcs_seg_sort_cap(W)  # a sorted run is copied by seg_sort_k as one segment
        return s

    def limit(self, W, lcap=None):
        """The fill at which a P5 pass aborts, and the keys a planned pass or a multi run may hold."""
        lcap = self.lds_slots(W) if lcap is None else lcap
        limit = lcap * 13 >> 4
        return limit, limit * 7 // 8


@pytest.fixture(scope="module")
def shim(kca):
    return Shim(kca)


def _p(a):
    return None if a is None else a.ctypes.data


def _fillbuf(shape, dtype):
    return np.frombuffer(bytes([FILL]) * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype=dtype).reshape(
        shape).copy()


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def rand_low(rng, n, bits):
    """n distinct values in [1, 2^bits)."""
    out = np.unique(rng.integers(1, 1 << bits, size=n + n // 8 + 8, dtype=np.uint64))
    assert out.size >= n
    return rng.permutation(out)[:n]


def with_words(rng, W, w0):
    """(W, n) keys over word 0 values w0: the other words random."""
    w0 = np.asarray(w0, dtype=U64)
    rest = rng.integers(0, 1 << 63, size=(W - 1, w0.size), dtype=np.uint64) * U64(2) + U64(1)
    return np.concatenate([w0[None, :], rest], axis=0)


def bucket_keys(rng, W, b, n, sub=None):
    """n distinct keys of bucket b (of its sub-bucket `sub`)."""
    if sub is None:
        w0 = (U64(b) << U64(48)) | rand_low(rng, n, 48)
    else:
        w0 = (U64(b) << U64(48)) | (U64(sub) << U64(40)) | rand_low(rng, n, 40)
    return with_words(rng, W, w0)


def layout(per_bucket, rng=None):
    """per_bucket: nb arrays (W, n_b) -> (keys (W, n + 1), starts): the
    buckets' keys one after the other (shuffled inside a bucket with rng)."""
    cols = []
    for k in per_bucket:
        cols.append(k[:, rng.permutation(k.shape[1])] if rng is not None else k)
    keys = np.concatenate(cols + [np.zeros((cols[0].shape[0], 1), dtype=U64)], axis=1)
    starts = np.concatenate([[0], np.cumsum([k.shape[1] for k in per_bucket])]).astype(U64)
    return np.ascontiguousarray(keys), starts


def presplit(keys, nb, rng=None):
    """Keys (W, n) of buckets < nb -> (keys (W, n + 1) grouped by bucket and
    sub-bucket, in random order inside one; starts; sub_starts)."""
    keys = np.asarray(keys, dtype=U64)
    top = (keys[0] >> U64(40)).astype(np.int64)
    assert top.max(initial=0) < nb * 256
    if rng is not None:
        keys = keys[:, rng.permutation(keys.shape[1])]
        top = (keys[0] >> U64(40)).astype(np.int64)
    o = np.argsort(top, kind="stable")
    sub = np.searchsorted(top[o], np.arange(nb * 256 + 1), side="left").astype(U64)
    out = np.concatenate([keys[:, o], np.zeros((keys.shape[0], 1), dtype=U64)], axis=1)
    return np.ascontiguousarray(out), np.ascontiguousarray(sub[::256]), sub


def sized_subs(rng, W, b, sizes):
    """Distinct keys of bucket b: sizes[s] keys in sub-bucket s."""
    return np.concatenate([bucket_keys(rng, W, b, n, s) for s, n in sorted(sizes.items()) if n], axis=1)


def run_range(b, s0, e):
    return ((b << 48) | (s0 << 40), (b << 48) + (e << 40))


def runs_of(sub, nb, per):
    """[(b, s0, e, multi, lo, hi)] of every non-empty run."""
    out = []
    for b in range(nb):
        ss = sub[b * 256:b * 256 + 257]
        for s0, e, multi in kr.p5_runs_ref(ss, per):
            out.append((b, s0, e, multi, int(ss[s0]), int(ss[e])))
    return out


def ceil_log2(x):
    return max(0, int(x - 1).bit_length())


# ---------------------------------------------------------------------------
# P5: count_buckets
# ---------------------------------------------------------------------------

def run_p5(shim, W, keys, starts, *, sub=None, run_flags=None, bucket_flags=None, run_per=0, distinct=0, lcap=0,
           grid=None, rec_cap=None, desc_cap=4096, table_cap=64, probe_limit=8, spill_cap=64, expect=0):
    n = int(starts[-1])
    nb = len(starts) - 1
    stride = keys.shape[1]
    assert keys.shape[0] == W and keys.flags.c_contiguous and stride >= n
    rec_cap = n + 8 if rec_cap is None else rec_cap
    grid = shim.n_cu if grid is None else grid
    sw = kr.slot_words(W)
    out = dict(rec_keys=_fillbuf((W, rec_cap), U64), rec_cnts=_fillbuf(rec_cap, np.uint32),
               desc_key=_fillbuf(desc_cap, U64), desc_start=_fillbuf(desc_cap, U64),
               desc_len=_fillbuf(desc_cap, np.uint32), table=np.zeros(table_cap * sw, dtype=U64),
               spill=_fillbuf((W, spill_cap), U64), stats=np.zeros(shim.st_n, dtype=U64))
    cursor = ctypes.c_uint64(0)
    starts = np.ascontiguousarray(starts, dtype=U64)
    rc = shim.L.kcs_count_buckets(W, _p(keys), stride, _p(starts), nb, _p(sub), _p(run_flags), _p(bucket_flags),
                                  run_per, distinct, lcap, grid, rec_cap, desc_cap, table_cap, probe_limit, spill_cap,
                                  FILL, _p(out["rec_keys"]), _p(out["rec_cnts"]), ctypes.addressof(cursor),
                                  _p(out["desc_key"]), _p(out["desc_start"]), _p(out["desc_len"]), _p(out["table"]),
                                  _p(out["spill"]), _p(out["stats"]))
    assert rc == expect, f"kcs_count_buckets: {rc} (guard clobbered: {shim.L.kcs_guard_clobbered()})"
    out["cursor"] = int(cursor.value)
    out["st"] = {name: int(out["stats"][globals()[name]]) for name in ST_NAMES}
    return out


def fallback_of(W, res, spill_cap):
    """(keys, counts) of what a launch left in the fallback table and the spill."""
    tk, tc = kr.table_entries(W, res["table"])
    ns = min(res["st"]["ST_SPILL2_FILL"], spill_cap)
    sk = res["spill"][:, :ns]
    kr.check_fill(res["spill"][:, ns:], FILL)
    return np.concatenate([tk, sk], axis=1), np.concatenate([tc, np.ones(ns, dtype=np.int64)]), tk.shape[1], ns


def no_fallback(W, res):
    st = res["st"]
    assert st["ST_CLAIMED"] == 0 and st["ST_SPILL2_FILL"] == 0 and st["ST_ERR"] == 0, st
    assert not res["table"].any(), "a key in the fallback table"
    kr.check_fill(res["spill"], FILL)


def check_p5(what, W, keys, ranges, res, extra=None):
    segs = kr.check_segments(what, keys, ranges, res["rec_keys"], res["rec_cnts"], res["cursor"],
                             (res["desc_key"], res["desc_start"], res["desc_len"]), res["st"]["ST_DESC_FILL"], FILL,
                             extra=extra)
    kr.check_fill(res["rec_keys"][:, res["cursor"]:], FILL)
    kr.check_fill(res["rec_cnts"][res["cursor"]:], FILL)
    assert not any(s[5] for s in segs), f"{what}: count_buckets flagged a segment sorted"
    return segs


def plain_ranges(starts):
    return [(int(starts[b]), int(starts[b + 1]), b << 48, (b + 1) << 48) for b in range(len(starts) - 1)
            if starts[b + 1] > starts[b]]


def split_shifts_ok(what, segs, top_shift, maxm):
    """Segments of a range split into m = 2^j passes: shift top_shift - j,
    the segment's range aligned to its size, j at most log2(maxm)."""
    for r, key, a, n, s, srt in segs:
        j = top_shift - s
        assert 0 <= j <= ceil_log2(max(maxm, 1)), f"{what}: shift {s} with the largest split {maxm}"
        assert (key & kr.M48) % (1 << (s + 12)) == 0, f"{what}: desc_key {key:#x} not aligned to its range 2^{s + 12}"


@pytest.mark.parametrize("W", WS)
def test_p5_repeats_take_one_pass_per_bucket(shim, W):
    """Few distinct keys, many repeats, empty and one-key buckets between
    them: one pass per bucket, no abort, nothing in the fallback, shift 36.
    W >= 2: keys of bucket 0 whose word 0 is 0, and keys that differ only in
    their last word."""
    rng = np.random.default_rng(100 + W)
    empty = np.zeros((W, 0), dtype=U64)
    few = bucket_keys(rng, W, 2, 50)
    b0 = bucket_keys(rng, W, 0, 30)
    if W >= 2:
        b0 = np.concatenate([b0, with_words(rng, W, np.zeros(40, dtype=U64))], axis=1)
    same = np.repeat(bucket_keys(rng, W, 5, 1), 64, axis=1)
    same[W - 1] = rand_low(rng, 64, 40)  # W = 1: 64 keys of bucket 0's range moved below
    if W == 1:
        same[0] |= U64(5) << U64(48)
    mid = bucket_keys(rng, W, 5, 300)
    per_bucket = [np.tile(b0, 3), bucket_keys(rng, W, 1, 1), np.tile(few, 100), empty, empty,
                  np.concatenate([np.tile(mid, 3), np.tile(same, 2)], axis=1), empty, bucket_keys(rng, W, 7, 1)]
    keys, starts = layout(per_bucket, rng)
    res = run_p5(shim, W, keys, starts)
    st = res["st"]
    segs = check_p5("repeats", W, keys, plain_ranges(starts), res)
    no_fallback(W, res)
    assert st["ST_P5_ABORTS"] == 0 and st["ST_P5_MAXM"] == 0
    assert st["ST_P5_PASSES"] == st["ST_DESC_FILL"] == len(segs) == 5
    assert [s[4] for s in segs] == [36] * 5
    assert [s[1] for s in segs] == [b << 48 for b in (0, 1, 2, 5, 7)]
    assert [s[3] for s in segs] == [b0.shape[1], 1, 50, 364, 1]


@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("frac", ("limit", "per"))
def test_p5_under_the_abort_limit(shim, W, frac):
    """limit - 1 distinct keys (and per = 7/8 limit, what a planned pass may
    hold) fill the table without an abort. While an insert gave up after 64
    probes this failed for every W: limit - 1 keys aborted in 16 of 16 trials
    (4 seeds per W), per keys in 5 of 16, 65% of the slots in none."""
    rng = np.random.default_rng(200 + W)
    limit, per = shim.limit(W)
    nd = limit - 1 if frac == "limit" else per
    under = bucket_keys(rng, W, 1, nd)
    keys, starts = layout([np.zeros((W, 0), dtype=U64), np.concatenate([under, under[:, :100]], axis=1)], rng)
    res = run_p5(shim, W, keys, starts)
    print(f"W={W} limit={limit} distinct={nd}: {res['st']}")
    segs = check_p5("under the limit", W, keys, plain_ranges(starts), res)
    no_fallback(W, res)
    assert res["st"]["ST_P5_ABORTS"] == 0 and res["st"]["ST_P5_PASSES"] == 1, res["st"]
    assert [(s[3], s[4]) for s in segs] == [(nd, 36)]


@pytest.mark.parametrize("W", WS)
def test_p5_over_the_abort_limit(shim, W):
    """1.5 * limit distinct keys abort and split by a power of two, every
    segment with shift 36 - log2 m over an aligned range, and nothing reaches
    the fallback."""
    rng = np.random.default_rng(250 + W)
    limit, per = shim.limit(W)
    over = bucket_keys(rng, W, 3, limit + limit // 2)
    keys, starts = layout([bucket_keys(rng, W, 0, 1), np.zeros((W, 0), dtype=U64), np.zeros((W, 0), dtype=U64),
                           np.concatenate([over, over[:, :77]], axis=1)], rng)
    res = run_p5(shim, W, keys, starts)
    st = res["st"]
    print(f"W={W} limit={limit} over: {st}")
    segs = check_p5("over the limit", W, keys, plain_ranges(starts), res)
    no_fallback(W, res)
    m = st["ST_P5_MAXM"]
    assert st["ST_P5_ABORTS"] >= 1 and m >= 2 and m & (m - 1) == 0, st
    split_shifts_ok("over the limit", segs[1:], 36, m)
    assert segs[0][4] == 36 and min(s[4] for s in segs[1:]) == 36 - ceil_log2(m)
    assert st["ST_DESC_FILL"] == len(segs) <= st["ST_P5_PASSES"] <= 1 + m


@pytest.mark.parametrize("W", WS)
def test_p5_distinct_hint_plans_the_split(shim, W):
    """distinct = 1 and 3 * per distinct keys: m = 4 from the key count, no
    aborted first pass."""
    rng = np.random.default_rng(300 + W)
    limit, per = shim.limit(W)
    keys, starts = layout([bucket_keys(rng, W, 0, 1), bucket_keys(rng, W, 1, 3 * per)], rng)
    res = run_p5(shim, W, keys, starts, distinct=1)
    st = res["st"]
    segs = check_p5("distinct", W, keys, plain_ranges(starts), res)
    no_fallback(W, res)
    assert st["ST_P5_ABORTS"] == 0 and st["ST_P5_MAXM"] == 0, st
    assert st["ST_P5_PASSES"] == 1 + 4 and len(segs) == 5, st
    assert [s[4] for s in segs] == [36, 34, 34, 34, 34]
    assert [s[1] for s in segs[1:]] == [(1 << 48) | (j << 46) for j in range(4)]
    # the same keys without the hint: an abort, the same counts
    res0 = run_p5(shim, W, keys, starts)
    check_p5("no hint", W, keys, plain_ranges(starts), res0)
    assert res0["st"]["ST_P5_ABORTS"] >= 1


def lcap64_case():
    rng = np.random.default_rng(64)
    k = bucket_keys(rng, 1, 2, 60000)
    return layout([np.zeros((1, 0), dtype=U64), bucket_keys(rng, 1, 1, 3), np.tile(k, 2)], rng)


def test_p5_last_resort_fills_the_global_table(shim):
    """lcap = 64 and 60,000 distinct keys in one bucket: the split reaches
    m = 1024, where the surplus of a pass goes to the global table."""
    keys, starts = lcap64_case()
    res = run_p5(shim, 1, keys, starts, lcap=64, table_cap=1 << 15, probe_limit=256, desc_cap=2048)
    st = res["st"]
    ek, ec, nt, ns = fallback_of(1, res, 64)
    segs = check_p5("table", 1, keys, plain_ranges(starts), res, extra=(ek, ec))
    assert st["ST_P5_MAXM"] == 1024 and st["ST_P5_ABORTS"] >= 1, st
    assert st["ST_CLAIMED"] == nt > 0 and ns == 0 and st["ST_ERR"] == 0, st
    assert np.all(ec == 2), "a key split between the LDS table and the fallback"
    assert min(s[4] for s in segs) == 26
    split_shifts_ok("table", segs[1:], 36, 1024)


def test_p5_last_resort_spills_past_a_tiny_table(shim):
    keys, starts = lcap64_case()
    res = run_p5(shim, 1, keys, starts, lcap=64, table_cap=4, probe_limit=2, spill_cap=1 << 15, desc_cap=2048)
    st = res["st"]
    ek, ec, nt, ns = fallback_of(1, res, 1 << 15)
    check_p5("spill", 1, keys, plain_ranges(starts), res, extra=(ek, ec))
    assert 0 < st["ST_CLAIMED"] == nt <= 4 and ns == st["ST_SPILL2_FILL"] > 0 and st["ST_ERR"] == 0, st


def test_p5_spill_overflow_is_reported(shim):
    keys, starts = lcap64_case()
    res = run_p5(shim, 1, keys, starts, lcap=64, table_cap=4, probe_limit=2, spill_cap=16, desc_cap=2048)
    st = res["st"]
    assert st["ST_ERR"] == shim.err_spill and st["ST_SPILL2_FILL"] > 16, st
    assert not np.any(res["spill"] == U64(int.from_bytes(bytes([FILL]) * 8, "little"))), "spill entries below the cap"
    # what was kept is still right: every record is a key of the input with at most its count
    wk, wc = kr.count_keys_ref(keys[:, :int(starts[-1])])
    gk, gc = kr.count_keys_ref(res["rec_keys"][:, :res["cursor"]], res["rec_cnts"][:res["cursor"]])
    pos = np.searchsorted(wk[0], gk[0])
    assert np.array_equal(wk[0][pos], gk[0]) and np.all(gc <= wc[pos])


def test_p5_ungrouped_probing(shim):
    """lcap = 66 is no multiple of 4: W = 1 probes slot by slot."""
    rng = np.random.default_rng(66)
    keys, starts = layout([np.tile(bucket_keys(rng, 1, 0, 30), 5), bucket_keys(rng, 1, 1, 1),
                           np.tile(bucket_keys(rng, 1, 2, 200), 2)], rng)
    res = run_p5(shim, 1, keys, starts, lcap=66)
    st = res["st"]
    segs = check_p5("lcap 66", 1, keys, plain_ranges(starts), res)
    no_fallback(1, res)
    assert st["ST_P5_ABORTS"] >= 1 and st["ST_P5_MAXM"] >= 4, st
    assert [s[4] for s in segs[:2]] == [36, 36] and segs[0][3] == 30
    split_shifts_ok("lcap 66", segs[2:], 36, st["ST_P5_MAXM"])


@pytest.mark.parametrize("W", (1, 2))
@pytest.mark.parametrize("lcap", (1, 63))
def test_p5_tiny_tables_use_the_fallback_only(shim, W, lcap):
    """lcap < 64: no split (mmax = 1); what the LDS table cannot hold goes to the global table."""
    rng = np.random.default_rng(lcap + W)
    keys, starts = layout([np.tile(bucket_keys(rng, W, 0, 90), 3), np.zeros((W, 0), dtype=U64),
                           np.tile(bucket_keys(rng, W, 2, 5), 4)], rng)
    res = run_p5(shim, W, keys, starts, lcap=lcap, table_cap=1024, probe_limit=64)
    st = res["st"]
    ek, ec, nt, ns = fallback_of(W, res, 64)
    segs = check_p5("tiny", W, keys, plain_ranges(starts), res, extra=(ek, ec))
    assert st["ST_P5_ABORTS"] == 0 and st["ST_P5_MAXM"] == 0 and st["ST_P5_PASSES"] == 2 == len(segs), st
    assert [s[4] for s in segs] == [36, 36]
    assert segs[0][3] == lcap and segs[1][3] == min(lcap, 5)
    assert nt == st["ST_CLAIMED"] == 95 - res["cursor"] and ns == 0 and st["ST_ERR"] == 0


def test_p5_lcap_above_the_maximum_is_the_maximum(shim):
    rng = np.random.default_rng(9)
    slots = shim.lds_slots(1)
    keys, starts = layout([bucket_keys(rng, 1, 0, slots // 2)], rng)
    a = run_p5(shim, 1, keys, starts, lcap=0, grid=0)
    b = run_p5(shim, 1, keys, starts, lcap=slots + 1)
    for res in (a, b):
        check_p5("lcap", 1, keys, plain_ranges(starts), res)
        no_fallback(1, res)
        assert res["st"]["ST_P5_ABORTS"] == 0 and res["st"]["ST_P5_PASSES"] == 1


def test_p5_record_overflow_stops_the_launch(shim):
    """rec_cap one short of bucket 1's records: ERR_REC_OVERFLOW, nothing
    written past the buffer, bucket 2 never started."""
    rng = np.random.default_rng(11)
    keys, starts = layout([bucket_keys(rng, 2, 0, 10), np.tile(bucket_keys(rng, 2, 1, 20), 2),
                           bucket_keys(rng, 2, 2, 15)], rng)
    res = run_p5(shim, 2, keys, starts, grid=1, rec_cap=29)
    st = res["st"]
    assert st["ST_ERR"] == shim.err_rec and res["cursor"] == 30 and st["ST_P5_PASSES"] == 2 == st["ST_DESC_FILL"], st
    wk, wc = kr.bucket_counts_ref(keys, 0, starts[1])
    gk, gc = kr.count_keys_ref(res["rec_keys"][:, :10], res["rec_cnts"][:10])
    kr.check_equal("bucket 0", gk, wk)
    kr.check_equal("bucket 0 counts", gc, wc)
    assert np.all(res["rec_keys"][0, 10:29] >> U64(48) == 1) and np.all(res["rec_cnts"][10:29] == 2)
    assert np.unique(res["rec_keys"][0, 10:29]).size == 19


def test_p5_descriptor_capacity(shim):
    """More emitting passes than descriptors fit: all are counted, desc_cap written."""
    rng = np.random.default_rng(12)
    keys, starts = layout([bucket_keys(rng, 1, b, 5 + b) for b in range(5)], rng)
    res = run_p5(shim, 1, keys, starts, desc_cap=3)
    assert res["st"]["ST_DESC_FILL"] == 5 == res["st"]["ST_P5_PASSES"] and res["st"]["ST_ERR"] == 0
    ln, sh, srt = kr.desc_fields(res["desc_len"])
    assert np.all(sh == 36) and np.all(srt == 0) and sorted(ln.tolist()) == sorted(
        int(starts[int(k >> U64(48)) + 1] - starts[int(k >> U64(48))]) for k in res["desc_key"])
    gk, gc = kr.count_keys_ref(res["rec_keys"][:, :res["cursor"]], res["rec_cnts"][:res["cursor"]])
    wk, wc = kr.count_keys_ref(keys[:, :int(starts[-1])])
    kr.check_equal("records", gk, wk)


@pytest.mark.parametrize("W", (1, 3))
def test_p5_grid_of_one_gives_the_same_records(shim, W):
    rng = np.random.default_rng(13 + W)
    limit, per = shim.limit(W)
    per_bucket = [np.tile(bucket_keys(rng, W, b, 40 * (b % 4)), 2) for b in range(15)]
    per_bucket.append(bucket_keys(rng, W, 15, limit + 100))
    keys, starts = layout(per_bucket, rng)
    one = run_p5(shim, W, keys, starts, grid=1)
    many = run_p5(shim, W, keys, starts, grid=shim.n_cu)
    for res in (one, many):
        check_p5("grid", W, keys, plain_ranges(starts), res)
        no_fallback(W, res)
    rec = [np.concatenate([r["rec_keys"][:, :r["cursor"]], r["rec_cnts"][None, :r["cursor"]].astype(U64)])
           for r in (one, many)]
    kr.check_record_multiset("grid 1 against one workgroup per CU", rec[0], rec[1])
    # one workgroup walks the buckets in order: the descriptors are in key order
    nd = one["st"]["ST_DESC_FILL"]
    assert np.all(np.diff(one["desc_key"][:nd].astype(np.int64)) > 0)


def presplit_case(shim, W, rng, per, b=2):
    """One bucket: an empty leading run, a sub-bucket above per, multi runs of
    3, 193 and 56 sub-buckets, the last one ending at sub-bucket 256."""
    sizes = {3: per + per // 2, 4: per // 3, 5: per // 3, 6: per // 3, 7: per // 2, 100: per // 2, 200: 10, 255: 20}
    return sized_subs(rng, W, b, sizes)


@pytest.mark.parametrize("W", WS)
def test_p5_presplit_runs_and_shifts(shim, W):
    """Pre-split buckets: the run boundaries are p5_runs_ref's; a multi run's
    shift is 28 + ceil(log2(sub-buckets)), a single sub-bucket above per is
    split at fshift = 40 with shift 28 - log2 m."""
    rng = np.random.default_rng(400 + W)
    limit, per = shim.limit(W)
    k2 = presplit_case(shim, W, rng, per)
    k0 = sized_subs(rng, W, 0, {0: 5, 1: 5, 254: 1})
    keys, starts, sub = presplit(np.concatenate([k0, k2], axis=1), 4, rng)
    res = run_p5(shim, W, keys, starts, sub=sub)
    st = res["st"]
    runs = runs_of(sub, 4, per)
    assert [(r[0], r[1], r[2], r[3]) for r in runs] == [(0, 0, 256, True), (2, 3, 4, False), (2, 4, 7, True),
                                                         (2, 7, 200, True), (2, 200, 256, True)]
    ranges = [(lo, hi) + run_range(b, s0, e) for b, s0, e, multi, lo, hi in runs]
    segs = check_p5("pre-split", W, keys, ranges, res)
    no_fallback(W, res)
    by_run = {i: [s for s in segs if s[0] == i] for i in range(len(runs))}
    for i, (b, s0, e, multi, lo, hi) in enumerate(runs):
        if multi:
            assert len(by_run[i]) == 1, f"run {runs[i]}: {len(by_run[i])} segments"
            r, key, a, n, s, srt = by_run[i][0]
            assert key == run_range(b, s0, e)[0] and s == 28 + ceil_log2(e - s0), (runs[i], hex(key), s)
    m = st["ST_P5_MAXM"]
    assert st["ST_P5_ABORTS"] >= 1 and m >= 2 and m & (m - 1) == 0, st
    split_shifts_ok("sub-bucket above per", by_run[1], 28, m)
    assert min(s[4] for s in by_run[1]) == 28 - ceil_log2(m)
    assert st["ST_DESC_FILL"] == len(segs)


@pytest.mark.parametrize("W", WS)
def test_p5_presplit_counts_only_flagged_runs(shim, W):
    """With run_flags / bucket_flags and run_per = sort_runs_keys(W): the runs
    are walked with that size, only flagged ones are counted, a bucket without
    a flag is skipped whole."""
    rng = np.random.default_rng(500 + W)
    SP = shim.sr_keys(W)
    k = np.concatenate([sized_subs(rng, W, 0, {1: SP // 2, 2: SP // 2, 3: SP // 2, 9: 40}),
                        sized_subs(rng, W, 1, {0: 100, 77: SP + 1}),
                        sized_subs(rng, W, 2, {0: SP + SP // 4, 1: 30, 128: SP // 2, 255: SP // 2 + 1})], axis=1)
    keys, starts, sub = presplit(k, 3, rng)
    runs = runs_of(sub, 3, SP)
    assert [(r[0], r[1], r[2], r[3]) for r in runs] == [
        (0, 0, 3, True), (0, 3, 256, True), (1, 0, 77, True), (1, 77, 78, False), (2, 0, 1, False),
        (2, 1, 255, True), (2, 255, 256, True)]
    flagged = [1, 4, 6]  # a multi run, a sub-bucket above SP, the last run of the last bucket
    rf = np.zeros(3 * 256, dtype=np.uint8)
    bf = np.zeros(3, dtype=np.uint8)
    for i in flagged:
        rf[runs[i][0] * 256 + runs[i][1]] = 1
        bf[runs[i][0]] = 1
    res = run_p5(shim, W, keys, starts, sub=sub, run_flags=rf, bucket_flags=bf, run_per=SP, distinct=1)
    ranges = [(runs[i][4], runs[i][5]) + run_range(*runs[i][:3]) for i in flagged]
    segs = check_p5("flagged", W, keys, ranges, res)
    no_fallback(W, res)
    assert res["st"]["ST_P5_ABORTS"] == 0, res["st"]
    multi = [s for s in segs if s[0] in (0, 2)]
    assert [(s[1], s[4]) for s in multi] == [(run_range(0, 3, 256)[0], 28 + 8), (run_range(2, 255, 256)[0], 28)]
    assert len([s for s in segs if s[0] == 1]) == 2  # SP + SP / 4 distinct keys at distinct = 1: m = 2
    assert all(s[4] == 27 for s in segs if s[0] == 1)


# ---------------------------------------------------------------------------
# P5s: sort_runs_k
# ---------------------------------------------------------------------------

def run_p5s(shim, W, keys, sub, *, grid=None, rec_cap=None, desc_cap=1024, packed=False, pk_base=0):
    nb = (len(sub) - 1) // 256
    n = int(sub[-1])
    stride = keys.shape[1]
    assert keys.shape[0] == W and keys.flags.c_contiguous and stride >= n
    rec_cap = n + 8 if rec_cap is None else rec_cap
    grid = 2 * shim.n_cu if grid is None else grid
    out = dict(rec_keys=_fillbuf((W, rec_cap), U64), rec_cnts=_fillbuf(rec_cap, np.uint32),
               desc_key=_fillbuf(desc_cap, U64), desc_start=_fillbuf(desc_cap, U64),
               desc_len=_fillbuf(desc_cap, np.uint32), run_flags=np.zeros(nb * 256, dtype=np.uint8),
               bucket_flags=np.zeros(nb, dtype=np.uint8), stats=np.zeros(shim.st_n, dtype=U64),
               packed=_fillbuf((pk_base + n, 8 * W + 4), np.uint8) if packed else None)
    cursor = ctypes.c_uint64(0)
    nflag = ctypes.c_uint32(0)
    sub = np.ascontiguousarray(sub, dtype=U64)
    rc = shim.L.kcs_sort_runs(W, _p(keys), stride, _p(sub), nb, grid, rec_cap, desc_cap, FILL, _p(out["rec_keys"]),
                              _p(out["rec_cnts"]), ctypes.addressof(cursor), _p(out["desc_key"]),
                              _p(out["desc_start"]), _p(out["desc_len"]), _p(out["run_flags"]),
                              _p(out["bucket_flags"]), ctypes.addressof(nflag), _p(out["stats"]), int(packed), pk_base,
                              _p(out["packed"]))
    assert rc == 0, f"kcs_sort_runs: {rc} (guard clobbered: {shim.L.kcs_guard_clobbered()})"
    out["cursor"] = int(cursor.value)
    out["nflag"] = int(nflag.value)
    out["st"] = {name: int(out["stats"][globals()[name]]) for name in ST_NAMES}
    return out


def check_p5s(what, shim, W, keys, sub, res, flagged=()):
    """Every run of p5_runs_ref(ss, SP) is either sorted into one segment
    (its distinct keys ascending with their counts, the descriptor at the
    run's first key, flagged sorted) or, when its index is in `flagged`,
    flagged and left without records. Returns the runs."""
    SP = shim.sr_keys(W)
    nb = (len(sub) - 1) // 256
    runs = runs_of(sub, nb, SP)
    for i, r in enumerate(runs):
        assert r[3] or i in flagged, f"{what}: run {r} holds more than SP keys and is not expected flagged"
    want_rf = np.zeros(nb * 256, dtype=np.uint8)
    want_bf = np.zeros(nb, dtype=np.uint8)
    for i in flagged:
        want_rf[runs[i][0] * 256 + runs[i][1]] = 1
        want_bf[runs[i][0]] = 1
    got_runs = sorted(int(x) for x in np.flatnonzero(res["run_flags"]))
    assert np.array_equal(res["run_flags"], want_rf), (
        f"{what}: runs flagged at {[(x >> 8, x & 255) for x in got_runs]}, wanted "
        f"{[(runs[i][0], runs[i][1]) for i in flagged]}")
    kr.check_equal(f"{what}: bucket_flags", res["bucket_flags"], want_bf)
    assert res["nflag"] == len(flagged)
    st = res["st"]
    sorted_runs = [r for i, r in enumerate(runs) if i not in flagged]
    assert st["ST_P5_PASSES"] == st["ST_DESC_FILL"] == len(sorted_runs), (st, len(sorted_runs))
    assert st["ST_ERR"] == 0 and st["ST_P5_ABORTS"] == 0 and st["ST_CLAIMED"] == 0
    ranges = [(lo, hi) + run_range(b, s0, e) for b, s0, e, multi, lo, hi in sorted_runs]
    if res["packed"] is None:
        segs = kr.check_segments(what, keys, ranges, res["rec_keys"], res["rec_cnts"], res["cursor"],
                                 (res["desc_key"], res["desc_start"], res["desc_len"]), st["ST_DESC_FILL"], FILL)
        kr.check_fill(res["rec_keys"][:, res["cursor"]:], FILL)
        kr.check_fill(res["rec_cnts"][res["cursor"]:], FILL)
        assert len(segs) == len(sorted_runs)
        for (b, s0, e, multi, lo, hi), (r, key, a, n, s, srt) in zip(sorted_runs, segs):
            wk, wc = kr.bucket_counts_ref(keys, lo, hi)
            assert key == run_range(b, s0, e)[0] and srt == 1 and n == wk.shape[1], (what, (b, s0, e), hex(key), n)
            kr.check_equal(f"{what}: run {(b, s0, e)} keys", res["rec_keys"][:, a:a + n], wk)
            kr.check_equal(f"{what}: run {(b, s0, e)} counts", res["rec_cnts"][a:a + n].astype(np.int64), wc)
            # the field the sorted flag leaves unused: the run's own span, never too fine for its keys
            assert s == 30 + ceil_log2(e - s0)
    return runs, sorted_runs


@pytest.mark.parametrize("W", WS)
def test_p5s_run_walk(shim, W):
    """The bisection walk is the greedy walk, on bounds made to disagree. The
    runs of one sub-bucket, (1, 255, 256) and (5, 0, 1), were flagged while the
    bin multiplier 2^32 / span was held in 32 bits (0 at span 1)."""
    rng = np.random.default_rng(600 + W)
    SP = shim.sr_keys(W)
    h = SP // 2
    # A run that holds more than MAX_SORT_BIN keys must spread them: it bins
    # its keys over its whole span, empty sub-buckets included, so the keys of
    # one sub-bucket share about 2048 / span bins. Run (1, 0, 255) below holds
    # h + 1 keys in one sub-bucket of 255: at most 2048 / 255 + 2 = 10 bins for
    # more than 1000 keys, so it is flagged whatever their low bits are.
    assert h + 1 > MAX_SORT_BIN * 10
    k = np.concatenate([
        sized_subs(rng, W, 0, {0: h, 1: SP - h, 2: 5}),                 # exactly SP keys, then the rest
        sized_subs(rng, W, 1, {254: h + 1, 255: SP - h}),               # SP + 1 keys in two sub-buckets: two runs
        sized_subs(rng, W, 2, {7: SP + 1}),                             # one sub-bucket above SP: flagged
        sized_subs(rng, W, 3, {s: 2 for s in range(256)}),              # all 256 sub-buckets in one run
        sized_subs(rng, W, 4, {0: h, 2: h, 3: h, 7: h, 8: 40}),         # spans 3, 5, 248
        sized_subs(rng, W, 5, {0: SP, 1: 1, 255: 20}),                  # span 1, then 255
    ], axis=1)
    keys, starts, sub = presplit(k, 6, rng)
    res = run_p5s(shim, W, keys, sub)
    runs, sorted_runs = check_p5s("walk", shim, W, keys, sub, res, flagged=(2, 4))
    assert [(r[0], r[1], r[2]) for r in runs] == [
        (0, 0, 2), (0, 2, 256), (1, 0, 255), (1, 255, 256), (2, 7, 8), (3, 0, 256), (4, 0, 3), (4, 3, 8), (4, 8, 256),
        (5, 0, 1), (5, 1, 256)]
    assert runs[0][5] - runs[0][4] == SP and res["cursor"] == int(sub[-1]) - (h + 1) - (SP + 1)
    assert np.all(res["rec_cnts"][:res["cursor"]] == 1)


@pytest.mark.parametrize("W", WS)
def test_p5s_lengths_and_key_offsets(shim, W):
    """Runs of 1, 2, 511, 512, 513 and SP keys; keys at the very bottom and
    the very top of a run's span."""
    rng = np.random.default_rng(700 + W)
    SP = shim.sr_keys(W)
    lens = (1, 2, 511, 512, 513, SP)
    parts = [bucket_keys(rng, W, b + 1, n) for b, n in enumerate(lens)]  # spread over the bucket: one run each
    b = len(lens) + 1
    edge = with_words(rng, W, np.array([b << 48, (b << 48) | ((1 << 48) - 1), (b << 48) | (255 << 40)], dtype=U64))
    parts.append(np.concatenate([edge, sized_subs(rng, W, b, {s: 3 for s in range(1, 255)})], axis=1))
    keys, starts, sub = presplit(np.concatenate(parts, axis=1), b + 1, rng)
    res = run_p5s(shim, W, keys, sub)
    runs, sorted_runs = check_p5s("lengths", shim, W, keys, sub, res)
    assert [r[5] - r[4] for r in runs] == list(lens) + [3 + 3 * 254]
    a = int(res["desc_start"][np.flatnonzero(res["desc_key"][:len(runs)] == U64(b << 48))[0]])
    assert int(res["rec_keys"][0, a]) == b << 48 and int(res["rec_keys"][0, a + 3 * 254 + 2]) == (b << 48) | kr.M48


def equal_keys_case(rng, W, SP):
    """Bucket 1: sub-bucket 4 between two sub-buckets above SP, so that it is a
    run of its own over a span of 1: 1100 keys with the key at position 5
    again at position 5 + 512 (one thread holds both), the largest key twice,
    and 30 keys three times. Bucket 2: a bin of exactly 8 keys, one of 9 (the
    keys differ in bits the bin digit does not see: it has 11 bits over a span
    of at least 2^40), MAX_SORT_BIN copies of a key. Bucket 3: MAX_SORT_BIN +
    1 copies of a key: flagged."""
    k1 = sized_subs(rng, W, 1, {4: 1100})
    k1[:, 5 + 512] = k1[:, 5]
    top = int(np.argmax(k1[0]))
    k1[:, (top + 1) % 1100 if (top + 1) % 1100 not in (5, 517) else (top + 2) % 1100] = k1[:, top]
    k1 = np.concatenate([sized_subs(rng, W, 1, {3: SP + 1}), k1, np.tile(k1[:, 600:630], 2),
                         sized_subs(rng, W, 1, {5: SP + 1})], axis=1)

    def cluster(b, s, n, low):
        base = np.repeat(bucket_keys(rng, W, b, 1, s), n, axis=1)
        base[0] = (base[0] & ~U64(0xff)) | (U64(low) + np.arange(n, dtype=U64))
        return base

    k2 = np.concatenate([cluster(2, 10, 8, 0), cluster(2, 20, 9, 16),
                         np.repeat(bucket_keys(rng, W, 2, 1, 30), MAX_SORT_BIN, axis=1),
                         sized_subs(rng, W, 2, {40: 25, 200: 25})], axis=1)
    k3 = np.concatenate([np.repeat(bucket_keys(rng, W, 3, 1, 30), MAX_SORT_BIN + 1, axis=1),
                         sized_subs(rng, W, 3, {40: 25, 200: 25})], axis=1)
    return np.concatenate([k1, k2, k3], axis=1)


@pytest.mark.parametrize("W", WS)
def test_p5s_equal_keys_and_bin_sizes(shim, W):
    rng = np.random.default_rng(800 + W)
    SP = shim.sr_keys(W)
    # grouped stably: the keys of a sub-bucket keep the order they were made in
    keys, starts, sub = presplit(equal_keys_case(rng, W, SP), 4)
    lo = int(sub[256 + 4])
    assert np.array_equal(keys[:, lo + 5], keys[:, lo + 517]) and int(sub[256 + 5]) - lo == 1160
    res = run_p5s(shim, W, keys, sub)
    runs, sorted_runs = check_p5s("equal keys", shim, W, keys, sub, res, flagged=(0, 2, 4))
    assert [(r[0], r[1], r[2], r[5] - r[4]) for r in runs] == [
        (1, 3, 4, SP + 1), (1, 4, 5, 1160), (1, 5, 6, SP + 1), (2, 0, 256, 8 + 9 + MAX_SORT_BIN + 50),
        (3, 0, 256, MAX_SORT_BIN + 51)]
    assert res["cursor"] == (1100 - 2) + (8 + 9 + 1 + 50)
    assert int(res["rec_cnts"][:res["cursor"]].max()) == MAX_SORT_BIN


@pytest.mark.parametrize("W", WS)
def test_p5s_direct_mode(shim, W):
    """Direct mode: a run's records land at pk_base + its first key + rank in
    the packed buffer; runs with equal keys leave gaps that packed_seg_copy
    closes; a flagged run is reported."""
    rng = np.random.default_rng(900 + W)
    SP = shim.sr_keys(W)
    rs = 8 * W + 4
    pk_base = 3
    k = np.concatenate([bucket_keys(rng, W, 0, SP // 2 + 300), bucket_keys(rng, W, 1, 2 * SP - 100),
                        sized_subs(rng, W, 2, {s: 5 for s in range(0, 256, 3)})], axis=1)
    keys, starts, sub = presplit(k, 3, rng)
    n = int(sub[-1])
    res = run_p5s(shim, W, keys, sub, packed=True, pk_base=pk_base)
    check_p5s("direct, distinct", shim, W, keys, sub, res)
    assert res["cursor"] == n and res["nflag"] == 0
    wk, wc = kr.count_keys_ref(keys[:, :n])
    kr.check_packed("direct, distinct", res["packed"], wk, wc, FILL, skip=pk_base)
    kr.check_fill(res["rec_keys"], FILL)
    kr.check_fill(res["rec_cnts"], FILL)
    nd = res["st"]["ST_DESC_FILL"]
    ln, sh, srt = kr.desc_fields(res["desc_len"][:nd])
    assert np.all(srt == 1)
    for key, a, l in zip(res["desc_key"][:nd], res["desc_start"][:nd], ln):
        assert int(a) == pk_base + int(sub[int(key >> U64(40))])  # the run's first key
    assert nd >= 4

    # equal keys: every key of two runs twice, one run distinct, one run flagged
    dup = np.concatenate([np.tile(bucket_keys(rng, W, 0, 700), 2), bucket_keys(rng, W, 1, 900),
                          np.tile(sized_subs(rng, W, 2, {s: 4 for s in range(256)}), 2),
                          sized_subs(rng, W, 3, {50: SP + 1})], axis=1)
    keys, starts, sub = presplit(dup, 4, rng)
    n = int(sub[-1])
    res = run_p5s(shim, W, keys, sub, packed=True, pk_base=pk_base)
    runs, sorted_runs = check_p5s("direct, equal keys", shim, W, keys, sub, res, flagged=(3,))
    assert res["nflag"] == 1 and res["cursor"] == 700 + 900 + 1024 < n
    nd = res["st"]["ST_DESC_FILL"]
    assert nd == 3
    ln, sh, srt = kr.desc_fields(res["desc_len"][:nd])
    order = np.argsort(res["desc_key"][:nd], kind="stable").astype(np.uint32)
    out_off = np.concatenate([[0], np.cumsum(ln[order])[:-1]]).astype(U64)
    dst = _fillbuf((res["cursor"] + 2, rs), np.uint8)
    src = np.ascontiguousarray(res["packed"])
    dstart = np.ascontiguousarray(res["desc_start"][:nd])
    dlen = np.ascontiguousarray(res["desc_len"][:nd])
    rc = shim.L.kcs_packed_seg_copy(W, src.shape[0], _p(src), dst.shape[0], _p(dst), nd, _p(order), _p(dstart),
                                    _p(dlen), _p(out_off), 0, 4, FILL)
    assert rc == 0
    wk, wc = kr.count_keys_ref(keys[:, :int(sub[3 * 256])])
    kr.check_packed("direct, after the copy", dst, wk, wc, FILL)
    # before the copy: each run's records at its first key, the gap behind them and the flagged run untouched
    for b, s0, e, multi, lo, hi in sorted_runs:
        rk, rc_ = kr.bucket_counts_ref(keys, lo, hi)
        m = rk.shape[1]
        kr.check_equal("direct, in place", src[pk_base + lo:pk_base + lo + m], kr.pack_records(rk, rc_))
        kr.check_fill(src[pk_base + lo + m:pk_base + hi], FILL)
    kr.check_fill(src[:pk_base], FILL)
    kr.check_fill(src[pk_base + runs[3][4]:], FILL)


# ---------------------------------------------------------------------------
# composition: what the finish consumes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("W", WS)
def test_p5s_then_p5_feed_the_segment_sort(shim, W):
    """P5s over every run, P5 over the runs it flagged (the same flags,
    run_per = SP, distinct, as the API launches it), then the segments of
    both in desc_key order through seg_sort_k: the sorted distinct keys with
    their counts, byte for byte, and no segment handed to the LSD kernel:
    every descriptor's shift spreads its uniform keys over the 4096 bins."""
    rng = np.random.default_rng(1000 + W)
    SP = shim.sr_keys(W)
    cluster = np.repeat(bucket_keys(rng, W, 1, 1, 101), MAX_SORT_BIN + 2, axis=1)
    k = np.concatenate([
        sized_subs(rng, W, 0, {s: SP // 40 for s in range(256)}),
        sized_subs(rng, W, 1, {5: 2 * SP + SP // 2, **{s: SP // 40 for s in range(6, 256)}}), cluster,
        np.tile(sized_subs(rng, W, 2, {s: 7 for s in range(0, 256, 5)}), 2),
    ], axis=1)
    keys, starts, sub = presplit(k, 3, rng)
    n = int(sub[-1])
    s5 = run_p5s(shim, W, keys, sub)
    runs = runs_of(sub, 3, SP)
    flagged = tuple(i for i, r in enumerate(runs) if not r[3] or (r[0] == 1 and r[1] <= 101 < r[2]))
    assert len(flagged) == 2 and any(runs[i][3] for i in flagged)
    check_p5s("composition, P5s", shim, W, keys, sub, s5, flagged=flagged)
    h5 = run_p5(shim, W, keys, starts, sub=sub, run_flags=s5["run_flags"], bucket_flags=s5["bucket_flags"],
                run_per=SP, distinct=1)
    ranges = [(runs[i][4], runs[i][5]) + run_range(*runs[i][:3]) for i in flagged]
    segs = check_p5("composition, P5", W, keys, ranges, h5)
    no_fallback(W, h5)
    multi = [s for s in segs if runs[flagged[s[0]]][3]]
    assert len(multi) == 1 and multi[0][4] == 28 + ceil_log2(runs[flagged[multi[0][0]]][2] -
                                                              runs[flagged[multi[0][0]]][1])
    # the finish: both launches' records in one buffer, descriptors in key order
    c1, c2 = s5["cursor"], h5["cursor"]
    n1, n2 = s5["st"]["ST_DESC_FILL"], h5["st"]["ST_DESC_FILL"]
    nrec = c1 + c2
    rkeys = np.ascontiguousarray(np.concatenate([s5["rec_keys"][:, :c1], h5["rec_keys"][:, :c2],
                                                 np.zeros((W, 1), dtype=U64)], axis=1))
    rcnts = np.ascontiguousarray(np.concatenate([s5["rec_cnts"][:c1], h5["rec_cnts"][:c2], [0]]).astype(np.uint32))
    dkey = np.concatenate([s5["desc_key"][:n1], h5["desc_key"][:n2]])
    dstart = np.ascontiguousarray(np.concatenate([s5["desc_start"][:n1], h5["desc_start"][:n2] + U64(c1)]))
    dlen = np.ascontiguousarray(np.concatenate([s5["desc_len"][:n1], h5["desc_len"][:n2]]))
    order = np.argsort(dkey, kind="stable").astype(np.uint32)
    ln = kr.desc_fields(dlen)[0]
    out_off = np.concatenate([[0], np.cumsum(ln[order])[:-1]]).astype(U64)
    dkey_sorted = np.ascontiguousarray(dkey[order])
    nd = n1 + n2
    out = _fillbuf((nrec, 8 * W + 4), np.uint8)
    err = ctypes.c_uint64(0)
    fb_n = ctypes.c_uint64(0)
    rc = shim.L.kcs_seg_sort(W, nrec, _p(rkeys), _p(rcnts), nrec + 1, nd, _p(order), _p(dstart), _p(dlen),
                             _p(out_off), _p(dkey_sorted), nrec, 1, FILL, _p(out), None, 0, ctypes.addressof(err),
                             ctypes.addressof(fb_n), None)
    assert rc == 0 and err.value == 0
    wk, wc = kr.count_keys_ref(keys[:, :n])
    assert nrec == wk.shape[1]
    kr.check_equal("the finished run", out, kr.pack_records(wk, wc))
    assert fb_n.value == 0, f"{fb_n.value} segments went to the LSD kernel: a descriptor shift too coarse for its keys"


# ---------------------------------------------------------------------------
# P1 / P2: count_front with the histogram and the scatter sink
# ---------------------------------------------------------------------------

PART_LK = [(100, 21), (150, 31), (150, 55), (101, 100), (90, 29)]  # (90, 29): k mod 32 = 29, with N bases


def part_geom(shim, L, k, n):
    out = np.zeros(5, dtype=U64)
    assert shim.L.kcs_part_geometry(L, k, n, out.ctypes.data) == 0
    return dict(zip(("R", "seg_tiles", "nseg", "max_win", "scap"), (int(x) for x in out)))


_part_cache = {}


def part_case(shim, L, k):
    """Reads for three segments, the last tile and the last segment partial;
    the geometry; the reference of the unfiltered walk (computed once)."""
    if (L, k) in _part_cache:
        return _part_cache[(L, k)]
    g1 = part_geom(shim, L, k, 1)
    R, st = g1["R"], g1["seg_tiles"]
    n = (2 * st + 1) * R + R // 2 + 1
    g = part_geom(shim, L, k, n)
    tiles = -(-n // R)
    assert g["R"] == R and g["seg_tiles"] == st and g["nseg"] == 3 and n % R and tiles % st, (g, n)
    assert g["max_win"] == R * (L - k + 1) and g["scap"] >= g["max_win"]
    head = skm_reads.special_reads(L, 60, k) + skm_reads.edge_reads(L, k, k) + ["N" * L]
    tail = ["A" * L, "N" * L, ("ACGTN" * L)[:L]]
    reads = head + skm_reads.genome_reads(L, n - len(head) - len(tail), k, genome=3000) + tail
    assert len(reads) == n
    text = np.frombuffer("".join(reads).encode("latin1"), dtype=np.uint8).copy()
    ref = kr.part_front_ref(reads, k, R, st, 48)
    assert ref["nseg"] == 3 and ref["key0"] > 0
    _part_cache[(L, k)] = (reads, text, g, ref)
    return _part_cache[(L, k)]


def run_front(shim, text, n, L, k, g, *, shift=48, gbits=0, flo=0, fhi=256, no_stats=0, p1=False, base=None,
              out_stride=0, aos=0, digs=True, fmid=256, base2=None, out2_stride=0):
    W = (k + 31) // 32
    nseg = g["nseg"]
    hist = None
    if p1:
        hist = _fillbuf((256, nseg), U64) if gbits == 0 else _fillbuf((nseg, 1 << gbits, 256), np.uint32)
    p2 = base is not None
    out = _fillbuf((W, out_stride) if not aos else (out_stride, W), U64) if p2 else None
    dg = _fillbuf(out_stride, np.uint8) if p2 and digs else None
    out2 = _fillbuf((W, out2_stride) if not aos else (out2_stride, W), U64) if base2 is not None else None
    dg2 = _fillbuf(out2_stride, np.uint8) if base2 is not None and digs else None
    stats = np.zeros(shim.st_n, dtype=U64)
    b1 = None if base is None else np.ascontiguousarray(base, dtype=U64).reshape(-1)
    b2 = None if base2 is None else np.ascontiguousarray(base2, dtype=U64).reshape(-1)
    rc = shim.L.kcs_part_front(_p(text), n, L, k, shift, gbits, flo, fhi, no_stats, int(p1), _p(hist), int(p2),
                               _p(b1), out_stride, aos, int(digs), fmid, _p(b2), out2_stride, FILL, _p(out), _p(dg),
                               _p(out2), _p(dg2), _p(stats))
    assert rc == 0, f"kcs_part_front: {rc} (guard clobbered: {shim.L.kcs_guard_clobbered()})"
    if aos and p2:
        out = np.ascontiguousarray(out.T)
        out2 = None if out2 is None else np.ascontiguousarray(out2.T)
    return dict(hist=hist, out=out, digs=dg, out2=out2, digs2=dg2, stats=stats)


def filtered(ref, flo, fhi):
    """The reference of a key-range pass from the unfiltered one."""
    top = (ref["keys"][0] >> U64(56)).astype(np.int64)
    m = (top >= flo) & (top < fhi)
    hist = np.zeros_like(ref["hist"])
    np.add.at(hist, (ref["dig"][m], ref["seg"][m]), 1)
    return dict(ref, keys=ref["keys"][:, m], seg=ref["seg"][m], dig=ref["dig"][m], hist=hist)


def scan_base(hist):
    """Exclusive scan of hist[d, seg] in the kernel's order (d * nseg + seg)."""
    flat = hist.reshape(-1).astype(np.int64)
    base = np.concatenate([[0], np.cumsum(flat)[:-1]])
    return base.reshape(hist.shape), int(flat.sum())


def seg_windows(g, n, L, k):
    return min(n, g["seg_tiles"] * g["R"]) * (L - k + 1)


def check_scatter(what, out, digs, ref, base, total):
    """Every (digit, segment) slice holds the reference's keys (as a
    multiset); nothing else is written; digs[i] = word0 >> 56."""
    o = np.lexsort((ref["seg"], ref["dig"]))
    bounds = np.append(base.reshape(-1), total)
    got = kr.canon_blocks(kr.as_rows(out[:, :total]), bounds)
    want = kr.canon_blocks(kr.as_rows(ref["keys"][:, o]), bounds)
    bad = np.flatnonzero(np.any(got != want, axis=1))
    assert bad.size == 0, (f"{what}: {bad.size} keys differ from the reference after sorting each slice; first at "
                           f"{int(bad[0])}: got {[hex(int(x)) for x in got[bad[0]]]}, "
                           f"want {[hex(int(x)) for x in want[bad[0]]]}")
    kr.check_fill(out[:, total:], FILL)
    if digs is not None:
        kr.check_equal(f"{what}: digit bytes", digs[:total], (out[0, :total] >> U64(56)).astype(np.uint8))
        kr.check_fill(digs[total:], FILL)


def check_stats(what, stats, ref, counted=True):
    got = (int(stats[ST_VALID]), int(stats[ST_KEY0]), int(stats[ST_KEY0_PRESENT]))
    want = (ref["valid"], ref["key0"], ref["key0_present"]) if counted else (0, 0, 0)
    assert got == want, f"{what}: ST_VALID, ST_KEY0, ST_KEY0_PRESENT {got} != {want}"
    rest = stats.copy()
    rest[[ST_VALID, ST_KEY0, ST_KEY0_PRESENT]] = 0
    assert not rest.any(), f"{what}: another statistic was touched: {stats.tolist()}"


@pytest.mark.parametrize("L,k", PART_LK)
def test_p1_histogram(shim, L, k):
    reads, text, g, ref = part_case(shim, L, k)
    n = len(reads)
    res = run_front(shim, text, n, L, k, g, p1=True)
    kr.check_equal("P1", res["hist"].astype(np.int64), ref["hist"])
    assert not res["stats"].any(), "P1 touched a statistic"
    part = filtered(ref, 64, 160)
    res = run_front(shim, text, n, L, k, g, p1=True, flo=64, fhi=160)
    kr.check_equal("P1 in [64, 160)", res["hist"].astype(np.int64), part["hist"])
    # gbits = 4: per segment 16 groups (word0 >> 60) of 256 bins
    res4 = run_front(shim, text, n, L, k, g, p1=True, gbits=4)
    want4 = np.zeros((3, 16, 256), dtype=np.int64)
    np.add.at(want4, (ref["seg"], (ref["keys"][0] >> U64(60)).astype(np.int64), ref["dig"]), 1)
    kr.check_equal("P1 grouped", res4["hist"].astype(np.int64), want4)
    assert not res4["stats"].any()
    # the pass histograms and the planner's totals from the grouped one
    h4 = np.ascontiguousarray(res4["hist"].reshape(-1))
    for g0, g1 in ((0, 16), (4, 10), (15, 16)):
        s = _fillbuf((256, 3), U64)
        tot = _fillbuf(16, U64)
        assert shim.L.kcs_hist_group(_p(h4), 3, g0, g1, FILL, _p(s), _p(tot)) == 0
        kr.check_equal(f"group sum [{g0}, {g1})", s.astype(np.int64), filtered(ref, 16 * g0, 16 * g1)["hist"])
        kr.check_equal("group totals", tot.astype(np.int64), want4.sum(axis=(0, 2)))


@pytest.mark.parametrize("nseg", (1, 31, 32, 33))
def test_hist_group_segment_counts(shim, nseg):
    """hist_group_sum_k walks 32 segments per step: one short, exact, one over."""
    rng = np.random.default_rng(nseg)
    # a segment's bins together count its windows, which a u32 holds (P1 counts in u32); the totals are u64
    h = rng.integers(0, 1 << 20, size=(nseg, 16, 256), dtype=np.uint32)
    h[nseg - 1, 15, 255] = h[0, 0, 0] = 0xf0000000
    for g0, g1 in ((0, 16), (3, 4), (14, 16)):
        s = _fillbuf((256, nseg), U64)
        tot = _fillbuf(16, U64)
        assert shim.L.kcs_hist_group(_p(h), nseg, g0, g1, FILL, _p(s), _p(tot)) == 0
        kr.check_equal("group sum", s, h[:, g0:g1, :].astype(U64).sum(axis=1).T)
        kr.check_equal("group totals", tot, h.astype(U64).sum(axis=(0, 2)))
    assert shim.L.kcs_hist_group(_p(h), nseg, 4, 4, FILL, _p(s), _p(tot)) == shim.invalid


@pytest.mark.parametrize("L,k", PART_LK)
def test_p2_scatter(shim, L, k):
    reads, text, g, ref = part_case(shim, L, k)
    n = len(reads)
    slack = seg_windows(g, n, L, k)
    base, total = scan_base(ref["hist"])
    soa = run_front(shim, text, n, L, k, g, base=base, out_stride=total + slack)
    check_scatter("P2", soa["out"], soa["digs"], ref, base, total)
    check_stats("P2", soa["stats"], ref)
    aos = run_front(shim, text, n, L, k, g, base=base, out_stride=total + slack, aos=1, no_stats=1)
    check_scatter("P2 AoS", aos["out"], aos["digs"], ref, base, total)
    check_stats("P2 no_stats", aos["stats"], ref, counted=False)
    # a base that could let a run leave the output (the last run starts less
    # than its segment's windows before the end) never reaches the kernel
    assert shim.L.kcs_part_front(_p(text), n, L, k, 48, 0, 0, 256, 0, 0, None, 1, _p(base.astype(U64).reshape(-1)),
                                 total, 0, 0, 256, None, 0, FILL, _p(soa["out"]), None, None, None,
                                 _p(soa["stats"])) == shim.invalid


@pytest.mark.parametrize("L,k", PART_LK)
def test_p2_key_ranges(shim, L, k):
    """A key-range pass writes its range only; two ranges in one walk give in
    out and out2 what two launches give."""
    reads, text, g, ref = part_case(shim, L, k)
    n = len(reads)
    slack = seg_windows(g, n, L, k)
    flo, fmid, fhi = 16, 96, 224
    lo, hi = filtered(ref, flo, fmid), filtered(ref, fmid, fhi)
    (blo, tlo), (bhi, thi) = scan_base(lo["hist"]), scan_base(hi["hist"])
    assert tlo > 0 and thi > 0
    a = run_front(shim, text, n, L, k, g, flo=flo, fhi=fmid, base=blo, out_stride=tlo + slack)
    check_scatter("range 1", a["out"], a["digs"], lo, blo, tlo)
    check_stats("range 1", a["stats"], ref)
    b = run_front(shim, text, n, L, k, g, flo=fmid, fhi=fhi, base=bhi, out_stride=thi + slack, no_stats=1)
    check_scatter("range 2", b["out"], b["digs"], hi, bhi, thi)
    check_stats("range 2", b["stats"], ref, counted=False)
    for aos in (0, 1):
        d = run_front(shim, text, n, L, k, g, flo=flo, fhi=fhi, fmid=fmid, base=blo, out_stride=tlo + slack,
                      base2=bhi, out2_stride=thi + slack, aos=aos)
        check_scatter("two ranges, out", d["out"], d["digs"], lo, blo, tlo)
        check_scatter("two ranges, out2", d["out2"], d["digs2"], hi, bhi, thi)
        check_stats("two ranges", d["stats"], ref)


# ---------------------------------------------------------------------------
# the shim's own checks: a wrong test gets hipErrorInvalidValue, never a launch
# ---------------------------------------------------------------------------

def test_shim_rejects_wrong_arguments(shim):
    rng = np.random.default_rng(1)
    keys, starts, sub = presplit(sized_subs(rng, 1, 1, {3: 20, 9: 20}), 2)
    bad = shim.invalid
    ok = dict(sub=sub)
    assert run_p5(shim, 1, keys, starts, **ok)["cursor"] == 40
    run_p5(shim, 1, keys, np.array([0, 41, 40], dtype=U64), expect=bad)                  # bounds not ascending
    run_p5(shim, 1, keys, starts, sub=sub[::-1].copy(), expect=bad)                      # sub_starts descending
    moved = sub.copy()
    moved[256 + 4] += U64(1)                                                             # a key outside its sub-bucket
    run_p5(shim, 1, keys, starts, sub=moved, expect=bad)
    run_p5(shim, 1, keys, np.array([0, 1, 40], dtype=U64), sub=sub, expect=bad)          # starts disagree with sub_starts
    for cap in ("rec_cap", "desc_cap", "table_cap", "probe_limit", "spill_cap"):
        run_p5(shim, 1, keys, starts, expect=bad, **{cap: 0})
    run_p5(shim, 1, keys, starts, run_per=100, expect=bad)                               # run_per without sub_starts
    run_p5(shim, 1, keys, starts, sub=sub, run_flags=np.zeros(512, dtype=np.uint8), expect=bad)  # one flag array only
    zero = keys.copy()
    zero[0, 7] = 0
    run_p5(shim, 1, zero, starts, expect=bad)                                            # EMPTY as a key at W = 1
    two = np.ascontiguousarray(np.concatenate([zero, zero + U64(1)]))
    assert run_p5(shim, 2, two, starts)["cursor"] == 40                                  # W = 2: word 0 may be 0
    # bounds past the keys; W out of range (the output arrays are never written)
    dummy = np.zeros(64, dtype=U64)
    past = np.array([0, 0, keys.shape[1] + 1], dtype=U64)
    assert shim.L.kcs_count_buckets(1, _p(keys), keys.shape[1], _p(past), 2, None, None, None, 0, 0, 0, 1, 8, 8, 8,
                                    8, 8, FILL, *([_p(dummy)] * 9)) == bad
    assert shim.L.kcs_count_buckets(5, _p(keys), keys.shape[1], _p(starts), 2, None, None, None, 0, 0, 0, 1, 8, 8, 8,
                                    8, 8, FILL, *([_p(dummy)] * 9)) == bad
    assert shim.L.kcs_sort_runs(0, _p(keys), keys.shape[1], _p(sub), 2, 1, 8, 8, FILL, *([_p(dummy)] * 10), 0, 0,
                                None) == bad
    assert shim.L.kcs_sort_runs(1, _p(keys), keys.shape[1], _p(moved), 2, 1, 64, 8, FILL, *([_p(dummy)] * 10), 0, 0,
                                None) == bad
    assert shim.L.kcs_bucket_lds_slots(0) == 0 and shim.L.kcs_sort_runs_keys(5) == 0
    assert shim.L.kcs_part_geometry(20, 21, 10, _p(dummy)) == bad                        # L < k
