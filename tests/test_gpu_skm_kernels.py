"""Kernel-level tests of the two ends of the super-k-mer engine: the front
ends skm_front_k<W> (F), skm_front2_k<1, K> (F2) and skm_front3_k<K> (F3)
behind launch_skm_front, P5a (count_rec_k, dedup_total_k) and P5
(count_skm_k<W>), driven through libkc_kernel_shim.so
(tools/kc_kernel_shim.cpp). The references are plain numpy
(tests/kernel_ref.py: skm_runs_ref and friends, checked on the CPU by
tests/test_kernel_ref.py against the pure-Python statement of the k-mer
semantics); everything is integers, so every comparison is exact.

The engine keeps the final counts right for any bucket assignment, any run
cutting and any dedup result, so the end-to-end byte comparisons
(test_gpu_skm.py) cannot see a wrong minimizer, a run cut early, a P5a that
stopped deduplicating or a P5 that falls back without need. These tests pin
those at the kernel.

Edge sizes come from the library (kcs_skm_geometry, kcs_skm_lds_slots,
kcs_p5a_groups, kcs_n_cu), not from constants copied here.
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
LOW48 = U64((1 << 48) - 1)
RAW = 0xffffffff   # dlen: the bucket was not deduplicated
OVER = 0x80000000  # dlen flag: the list is at dpos[b]

# Indices into a statistics array (kc_device.h enum Stat): the Shim fills them in from kcs_stat_indices
ST_NAMES = ("ST_VALID", "ST_KEY0", "ST_KEY0_PRESENT", "ST_CLAIMED", "ST_ERR", "ST_SPILL2_FILL", "ST_P5_PASSES",
            "ST_P5_ABORTS", "ST_P5_KEYS", "ST_DEDUP")
ST_VALID = ST_KEY0 = ST_KEY0_PRESENT = ST_CLAIMED = ST_ERR = ST_SPILL2_FILL = None
ST_P5_PASSES = ST_P5_ABORTS = ST_P5_KEYS = ST_DEDUP = None


class Shim:
    def __init__(self, kca):
        kca.lib()  # libkc_hip.so first: the shim links it
        if not os.path.exists(SHIM_PATH):
            raise ImportError(f"{SHIM_PATH} is missing: run `make -C kmer-counter_amd`")
        L = ctypes.CDLL(SHIM_PATH)
        vp, u64, u32, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        L.kcs_skm_lds_slots.argtypes = [i]
        L.kcs_slot_words.argtypes = [i]
        L.kcs_p5a_groups.restype = u32
        L.kcs_err_spill_overflow.restype = u64
        L.kcs_err_rec_overflow.restype = u64
        L.kcs_skm_geometry.argtypes = [i, i, vp]
        L.kcs_stat_indices.argtypes = [vp]
        L.kcs_skm_front.argtypes = [vp, u64, u64, i, i, vp, vp, u64, i, i, i, vp, vp, vp, vp, vp, vp, vp]
        L.kcs_count_rec.argtypes = [vp, u64, vp, u32, u32, u32, i, u64, u64, i, i, vp, vp, vp, vp, vp]
        L.kcs_count_skm.argtypes = [i, i, vp, u64, vp, u32, u32, u32, i, u32, i, vp, vp, vp, u64, u64, u32, u64, i,
                                    vp, vp, vp, vp, vp, vp, vp]
        self.L = L
        self.n_cu = L.kcs_n_cu()
        assert self.n_cu > 0
        self.st_n = L.kcs_st_n()
        idx = np.zeros(len(ST_NAMES), dtype=np.int32)
        assert L.kcs_stat_indices(idx.ctypes.data) == 0
        assert len(set(idx.tolist())) == idx.size and 0 <= idx.min() and idx.max() < self.st_n
        globals().update(zip(ST_NAMES, (int(x) for x in idx)))
        self.invalid = L.kcs_invalid_value()
        assert self.invalid != 0
        self.err_spill = L.kcs_err_spill_overflow()
        self.err_rec = L.kcs_err_rec_overflow()

    def geometry(self, L, k):
        out = np.zeros(7, dtype=np.int32)
        assert self.L.kcs_skm_geometry(L, k, out.ctypes.data) == 0
        return dict(zip(("ok", "m", "Kp", "nmax", "R", "f3", "G"), (int(x) for x in out)))

    def lds_slots(self, W):
        s = self.L.kcs_skm_lds_slots(W)
        assert s >= 1024 and s % 64 == 0
        return s


@pytest.fixture(scope="module")
def shim(kca):
    return Shim(kca)


def _p(a):
    return None if a is None else a.ctypes.data


# ---------------------------------------------------------------------------
# front ends
# ---------------------------------------------------------------------------

FRONTS = (("f3", ()), ("f2", ("KC_NO_F3",)), ("f", ("KC_NO_F3", "KC_NO_F2")))


def lib_geom(shim, L, k):
    """The library's geometry, which must be the reference's."""
    lg = shim.geometry(L, k)
    g = kr.skm_geom_ref(L, k)
    assert lg["ok"] == 1 and g is not None, (L, k, lg)
    assert (lg["m"], lg["Kp"], lg["nmax"]) == (g["m"], g["Kp"], g["nmax"]), (lg, g)
    assert lg["G"] == (L + 15) // 16 and lg["R"] >= 1
    return lg, g


def run_front(shim, reads, L, k, *, pool_cap, grid_cap=64, dig1=True, var=False):
    """E + F through the shim. var: the reads (of their own lengths, at most
    L) go in as newline-separated text with seq_off / seq_end."""
    n = len(reads)
    lg = shim.geometry(L, k)
    RW = (k + 31) // 32 + 1
    if var:
        text = "\n".join(reads) + "\n"
        lens = np.array([len(s) for s in reads], dtype=U64)
        off = (np.cumsum(lens + U64(1)) - lens - U64(1)).astype(U64)
        end = off + lens
    else:
        assert all(len(s) == L for s in reads)
        text, off, end = "".join(reads), None, None
    tb = np.frombuffer(text.encode("latin1"), dtype=np.uint8)
    pool = np.zeros((RW, pool_cap), dtype=U64)
    d1 = np.zeros(pool_cap, dtype=np.uint8) if dig1 else None
    cursor = ctypes.c_uint64(0)
    stats = np.zeros(shim.st_n, dtype=U64)
    codes = np.zeros(n * lg["G"], dtype=np.uint32)
    inval = np.zeros(n * lg["G"], dtype=np.uint16)
    rlen = np.zeros(n, dtype=np.uint16) if var else None
    rc = shim.L.kcs_skm_front(_p(tb), tb.size, n, L, k, _p(off), _p(end), pool_cap, int(dig1), grid_cap, FILL,
                              _p(pool), _p(d1), ctypes.addressof(cursor), _p(stats), _p(codes), _p(inval), _p(rlen))
    assert rc == 0, f"kcs_skm_front: {rc} (guard: {shim.L.kcs_guard_clobbered()})"
    return dict(pool=pool, dig1=d1, cursor=int(cursor.value), stats=stats, codes=codes, inval=inval, rlen=rlen)


def pool_room(lg, g, L, k, n_reads, grid_cap, n_records):
    """A pool that holds the records and every wave's last chunk: a wave
    takes chunks of max(1024, a tile's records) and pads the rest of its last
    one; at most 4 min(grid_cap, tiles) waves run and tiles <= reads."""
    nw = L - k + 1
    chunk = max(1024, lg["R"] * nw, 64 * -(-nw // g["nmax"]))
    return n_records + (4 * min(grid_cap, n_reads) + 2) * chunk


def check_encoding(res, ref, L, G):
    """E's code words and masks against the reference's codes (first base highest)."""
    n = ref["codes"].shape[0]
    c = ref["codes"][:, :16 * G].astype(np.uint32).copy()
    bad = np.zeros((n, 16 * G), dtype=np.uint32)
    bad[:, :L] = ~ref["ok"][:, :L]
    c[:, L:] = 0
    sh2 = (30 - 2 * np.arange(16)).astype(np.uint32)
    sh1 = (15 - np.arange(16)).astype(np.uint32)
    want_c = (c.reshape(n, G, 16) << sh2).sum(axis=2, dtype=np.uint32)
    want_i = (bad.reshape(n, G, 16) << sh1).sum(axis=2, dtype=np.uint32).astype(np.uint16)
    kr.check_equal("codes", res["codes"].reshape(n, G), want_c)
    kr.check_equal("inval", res["inval"].reshape(n, G), want_i)


def check_front(what, res, ref, g, pool_cap, *, holes_known=True):
    """One launch's pool, dig1, cursor and statistics against the reference. Returns the real records."""
    cur = res["cursor"]
    want = ref["records"]
    assert want.shape[1] <= cur <= pool_cap, f"{what}: cursor {cur}, {want.shape[1]} records, pool {pool_cap}"
    handed = res["pool"][:, :cur]
    kr.check_fill(res["pool"][:, cur:], FILL)
    bk, n = kr.record_fields(handed)
    pad = n == 0
    # padding: n = 0 in bucket 0xffff and nothing else
    assert np.all(handed[0, pad] == U64(0xffff) << U64(48)) and not handed[1:, pad].any(), f"{what}: a padding record"
    real = handed[:, ~pad]
    assert np.all(bk[~pad] < 0xffff)
    assert np.all((n[~pad] >= 1) & (n[~pad] <= g["nmax"])), f"{what}: n outside [1, nmax]"
    assert real.shape[1] == int(np.sum(-(-ref["run_len"] // g["nmax"]))), (
        f"{what}: {real.shape[1]} records, the runs need {int(np.sum(-(-ref['run_len'] // g['nmax'])))}")
    kr.check_record_multiset(what, real, want)
    # every key of a record has the record's bucket (stated on its own: a
    # record stream that is wrong in the same way as the reference's cannot pass)
    kb, keys, _ = kr.skm_expand_ref(real, g)
    assert np.array_equal(kr.bucket_of_keys_ref(keys, g), kb), f"{what}: a key outside its record's bucket"
    if res["dig1"] is not None:
        kr.check_equal(f"{what} dig1", res["dig1"][:cur], ((handed[0] >> U64(48)) & U64(255)).astype(np.uint8))
        kr.check_fill(res["dig1"][cur:], FILL)
    st = res["stats"]
    assert int(st[ST_VALID]) == ref["valid"], f"{what}: ST_VALID {int(st[ST_VALID])} != {ref['valid']}"
    assert int(st[ST_KEY0]) == ref["key0"], f"{what}: ST_KEY0 {int(st[ST_KEY0])} != {ref['key0']}"
    if holes_known:
        assert int(st[ST_KEY0_PRESENT]) == ref["key0_present"], f"{what}: ST_KEY0_PRESENT"
    assert int(st[ST_ERR]) == 0
    return real


def make_reads(L, k, n, seed):
    """n reads of L bases: the edge reads first (in order: two of them are an
    adjacent pair), then reads that take the slow paths, then genome reads."""
    edge = skm_reads.edge_reads(L, k, seed)
    if n < len(edge):
        return edge[-n:]  # the tandem repeats and the adjacent pair
    rest = n - len(edge)
    ns = min(rest, max(rest // 4, 12))
    return edge + skm_reads.special_reads(L, ns, seed) + skm_reads.genome_reads(L, rest - ns, seed, genome=3000)


def fronts_case(shim, monkeypatch, k, L, n, *, grid_cap=64, seed=None, expect_f3=None, reads=None):
    """Every front end that applies on one input, each against the reference
    and all against each other. F3's applicability is the library's answer
    (kcs_skm_geometry). F2's is its documented requirement (W = 1 and at most
    64 chunks of 8 windows); the library has no getter for it, so where F2
    is left out for its LDS budget instead, the 'f2' launch repeats F, which
    is harmless. For W >= 2 and past 64 chunks only F exists: one launch, and
    nothing to agree with but the reference."""
    lg, g = lib_geom(shim, L, k)
    if expect_f3 is not None:
        assert bool(lg["f3"]) == expect_f3, f"F3 applies: {lg['f3']}"
    reads = make_reads(L, k, n, seed if seed is not None else 1000 * k + L) if reads is None else reads
    n = len(reads)
    ref = kr.skm_runs_ref(reads, k, g)
    cap = pool_room(lg, g, L, k, n, grid_cap, ref["records"].shape[1])
    outs = {}
    for name, env in FRONTS:
        if name == "f3" and not lg["f3"]:
            continue  # the same launch as the next one
        if name == "f2" and (g["W"] > 1 or -(-(L - k + 1) // 8) > 64):
            continue  # F2 does not take this shape: KC_NO_F3 alone already runs F
        for v in env:
            monkeypatch.setenv(v, "1")
        res = run_front(shim, reads, L, k, pool_cap=cap, grid_cap=grid_cap)
        if not outs:
            check_encoding(res, ref, L, lg["G"])
        outs[name] = kr.sort_records(check_front(f"{name} k={k} L={L} n={n}", res, ref, g, cap))
    names = list(outs)
    for a in names[1:]:
        kr.check_equal(f"{names[0]} vs {a}", outs[a], outs[names[0]])
    return ref, lg, g


# k = 31, L = 150 (the headline shape: F3, 15 chunks of 8 windows, F's tile of 4 reads)
@pytest.mark.parametrize("count", ["1", "63", "64", "65", "R-1", "R", "R+1", "582", "1500/2"])
def test_front_read_counts(shim, monkeypatch, count):
    """Read counts around a wave's 64 lanes (F3's tile) and F / F2's tile of R
    reads; 582 = 9 F3 tiles + 6 reads (the last tile and the last workgroup of
    4 waves partly empty); 1500 reads on 2 workgroups (every wave walks
    several tiles and refills its pool chunk)."""
    k, L = 31, 150
    R = shim.geometry(L, k)["R"]
    assert R >= 2
    grid_cap = 64
    if "/" in count:
        count, gc = count.split("/")
        grid_cap = int(gc)
    n = {"R-1": R - 1, "R": R, "R+1": R + 1}.get(count) or int(count)
    fronts_case(shim, monkeypatch, k, L, n, grid_cap=grid_cap, expect_f3=True)


@pytest.mark.parametrize("k,dw,n,f3", [
    (31, 0, 70, True),     # nw = 1 (L = k): one window per read, a chunk of one, F3 blocks before the first window
    (31, 6, 70, True),     # nw = 7: a partly filled 8-window chunk
    (31, 7, 70, True),     # nw = 8: exactly one chunk
    (31, 8, 70, True),     # nw = 9: the second chunk holds one window (left suffix of a 1-window chunk)
    (19, 8, 70, True),     # the same at B = 8 blocks of F3 (k - 10 < 17)
    (27, 21, 70, True),    # L = 48: the last window's key ends with the last code word
    (31, 33, 130, True),   # L = 64, K' = 32: the last window's key is the last two code words
    (27, 37, 130, True),   # L = 64 masked
    (25, 512, 9, True),    # nw = 513: one chunk more than F2 takes (F3, then F twice)
    (21, 879, 3, True),    # L = 900: the longest rows F3's LDS budget holds at k = 21; R = 1
    (19, 981, 2, False),   # L = 1000: F only (F3's LDS budget and F2's 64 chunks both exceeded)
])
def test_front_window_counts(shim, monkeypatch, k, dw, n, f3):
    fronts_case(shim, monkeypatch, k, k + dw, n, expect_f3=f3)


@pytest.mark.parametrize("k,W,m,masked,L,n", [
    (19, 1, 11, True, 100, 200),    # 24-bit hash, masked last word, B = 8
    (28, 1, 11, True, 100, 200),    # the largest masked k of W = 1 (nmax = 26), B = 16
    (32, 1, 11, False, 100, 200),   # K' = 32 = k
    (18, 1, 11, True, 100, 200),    # k - m + 1 = 8: F2's smallest window, no F3
    (40, 2, 11, True, 120, 120),    # W = 2, 24-bit hash
    (50, 2, 15, True, 120, 120),    # 32-bit hash (12 < m <= 16)
    (55, 2, 24, True, 130, 120),    # folded hash (m = 24), K' = k
    (62, 2, 24, False, 130, 120),   # K' = 64
    (66, 3, 15, True, 160, 100),    # W = 3, 32-bit hash
    (80, 3, 24, True, 160, 100),    # W = 3, folded hash, K' = k
    (94, 3, 24, False, 170, 100),   # K' = 96
])
def test_front_every_regime(shim, monkeypatch, k, W, m, masked, L, n):
    """One k per key width, hash regime and key span; the regime is asserted, not assumed."""
    g = kr.skm_geom_ref(L, k)
    assert (g["W"], g["m"], g["masked"]) == (W, m, masked)
    ref, lg, g = fronts_case(shim, monkeypatch, k, L, n, expect_f3=(W == 1 and k >= 19))
    assert ref["run_len"].max() > g["nmax"], "a run longer than nmax must be split"
    assert ref["key0"] > 0 and ref["key0_present"] == 1


def test_front_adjacent_reads_do_not_share_a_run(shim, monkeypatch):
    """Copies of one read back to back: every window of read r + 1 continues
    read r's last bucket somewhere, and lanes / chunks of neighbouring reads
    sit next to each other in a tile."""
    k, L = 31, 45
    one = skm_reads.genome_reads(L, 1, 9)[0]
    rep = ("ACCGT" * L)[:L]  # one run per read (a tandem repeat's minimizer recurs every 5 windows)
    reads = [one] * 70 + [rep] * 70 + ["C" * L] * 70
    ref, lg, g = fronts_case(shim, monkeypatch, k, L, len(reads), reads=reads, expect_f3=True)
    assert np.all(ref["run_start"] + ref["run_len"] <= L - k + 1)
    assert ref["run_read"].size >= len(reads)


def test_front_production_grid(shim, monkeypatch):
    """grid_cap as count_reads_skm passes it (8 workgroups per CU): the grid is then the tile count."""
    fronts_case(shim, monkeypatch, 31, 150, 300, grid_cap=8 * shim.n_cu, expect_f3=True)


@pytest.mark.parametrize("k", [19, 31])
def test_front3_variable_length_reads(shim, monkeypatch, k):
    """Reads of their own lengths in slots of L bases (rlen): shorter than k
    gives no record, exactly k gives one, the slot padding is neither a hole
    nor part of a key. F3 takes rlen; F2 and F see only the padding's masks,
    which cuts the same records (their ST_KEY0_PRESENT also counts the
    padding as holes, so it is compared for F3 only)."""
    L = 150
    lg, g = lib_geom(shim, L, k)
    assert lg["f3"]
    base = make_reads(L, k, 150, k)
    cut = [0, 1, k - 1, k, k + 1, k + 7, k + 8, 2 * k, L - 1, L, 15, 16, 17, 64, 100]
    reads = [s[:cut[i % len(cut)]] for i, s in enumerate(base)]
    reads += ["A" * k, "A" * (k - 1), "N" * k, "ACGT" * 30]
    ref = kr.skm_runs_ref(reads, k, g, L=L)
    lens = np.array([len(s) for s in reads])
    assert not np.isin(ref["p_read"], np.flatnonzero(lens < k)).any()
    exact = np.flatnonzero((lens == k) & ref["live"][:, 0])
    assert exact.size >= 3 and all(np.sum(ref["p_read"] == r) == 1 for r in exact)
    cap = pool_room(lg, g, L, k, len(reads), 64, ref["records"].shape[1])
    outs = []
    for name, env in FRONTS:
        for v in env:
            monkeypatch.setenv(v, "1")
        res = run_front(shim, reads, L, k, pool_cap=cap, var=True)
        kr.check_equal("rlen", res["rlen"], lens.astype(np.uint16))
        outs.append(kr.sort_records(check_front(f"var {name} k={k}", res, ref, g, cap, holes_known=(name == "f3"))))
    kr.check_equal("f3 vs f2", outs[1], outs[0])
    kr.check_equal("f3 vs f", outs[2], outs[0])


@pytest.mark.parametrize("front", ["f3", "f2", "f"])
def test_front_pool_overflow(shim, monkeypatch, front):
    """A pool smaller than the records: the cursor ends past the capacity and
    nothing is written past the pool or dig1 (the shim checks the guard words
    behind both and would return KCS_GUARD_CLOBBERED)."""
    k, L, n = 31, 150, 1200
    lg, g = lib_geom(shim, L, k)
    reads = make_reads(L, k, n, 77)
    ref = kr.skm_runs_ref(reads, k, g)
    nrec = ref["records"].shape[1]
    for v in dict(FRONTS)[front]:
        monkeypatch.setenv(v, "1")
    for cap in (nrec // 2, 1000, 1):
        res = run_front(shim, reads, L, k, pool_cap=cap, grid_cap=8)
        assert res["cursor"] > cap, (res["cursor"], cap)
        # what was written inside the pool is still records or padding of this input
        bk, nn = kr.record_fields(res["pool"])
        untouched = np.all(res["pool"] == U64(int.from_bytes(bytes([FILL]) * 8, "little")), axis=0)
        assert np.all((nn <= g["nmax"]) | untouched)


def test_front_rejects_bad_arguments(shim):
    reads = ["ACGT" * 10]
    tb = np.frombuffer(reads[0].encode(), dtype=np.uint8)
    z = np.zeros(64, dtype=U64)
    c = ctypes.c_uint64(0)
    args = lambda n, L, k, cap: (_p(tb), tb.size, n, L, k, None, None, cap, 0, 64, FILL, _p(z), None,
                                 ctypes.addressof(c), _p(z), _p(z), _p(z), None)
    assert shim.L.kcs_skm_front(*args(2, 40, 31, 8)) == shim.invalid   # text shorter than the reads
    assert shim.L.kcs_skm_front(*args(1, 40, 17, 8)) == shim.invalid   # k the engine does not take
    assert shim.L.kcs_skm_front(*args(1, 40, 31, 0)) == shim.invalid   # no pool


# ---------------------------------------------------------------------------
# P5a: count_rec_k + dedup_total_k
# ---------------------------------------------------------------------------

TAIL = U64(0x5151515151515151)


def run_count_rec(shim, recs, starts, b0, b1, *, room, use_over=True, grid=0):
    """P5a over grouped records (2, n). The overflow tail is `room` records
    from the next multiple of 64 behind the records; 7 more records behind it
    belong to nobody."""
    n = recs.shape[1]
    nb = starts.size - 1
    over0 = (n + 63) & ~63
    limit = over0 + room
    stride = limit + 7
    buf = np.full((2, stride), TAIL)
    buf[:, :n] = recs
    cnt = np.zeros(stride, dtype=np.uint32)
    dlen = np.zeros(nb, dtype=np.uint32)
    dpos = np.zeros(nb, dtype=U64)
    cur, ded = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = shim.L.kcs_count_rec(_p(buf), stride, _p(starts), nb, b0, b1, int(use_over), over0, limit, grid, FILL, _p(cnt),
                              _p(dlen), _p(dpos), ctypes.addressof(cur), ctypes.addressof(ded))
    assert rc == 0, f"kcs_count_rec: {rc}"
    return dict(recs=buf, cnt=cnt, dlen=dlen, dpos=dpos, cursor=int(cur.value), dedup=int(ded.value), over0=over0,
                limit=limit, stride=stride)


def check_count_rec(res, recs, starts, b0, b1, *, cursor_moves):
    """Test 5's properties for every bucket; returns (kind per bucket: 'list', 'over', 'raw', the list lengths)."""
    n = recs.shape[1]
    nb = starts.size - 1
    out, cnt, dlen, dpos = res["recs"], res["cnt"], res["dlen"], res["dpos"]
    st = starts.astype(np.int64)
    written = np.zeros(res["stride"], dtype=bool)  # cnt entries a list owns
    kinds, lens = {}, {}
    reserved = 0
    for b in range(b0, b1):
        lo, hi = int(st[b]), int(st[b + 1])
        dl = int(dlen[b])
        own = recs[:, lo:hi]
        if dl == RAW:
            kinds[b], lens[b] = "raw", hi - lo
            kr.check_equal(f"raw bucket {b}", out[:, lo:hi], own)
            reserved += hi - lo
            continue
        if dl & OVER:
            ln, pos = dl & ~OVER, int(dpos[b])
            kinds[b] = "over"
            assert res["over0"] <= pos and pos + ln <= res["limit"], f"bucket {b}: list outside the tail"
            # the bucket's own range stays as it was (the later passes read it)
            kr.check_equal(f"bucket {b} behind its overflow list", out[:, lo:hi], own)
            reserved += hi - lo
        else:
            ln, pos = dl, lo
            kinds[b] = "list"
        lens[b] = ln
        assert ln <= hi - lo, f"bucket {b}: {ln} listed of {hi - lo} records"
        assert not written[pos:pos + ln].any(), f"bucket {b}: its list overlaps another"
        written[pos:pos + ln] = True
        lst, mult = out[:, pos:pos + ln], cnt[pos:pos + ln]
        assert np.all(lst[0] >> U64(48) == U64(b)), f"bucket {b}: a listed record of another bucket"
        assert np.all(mult >= 1)
        gk, gc = kr.count_keys_ref(lst, mult)
        wk, wc = kr.count_keys_ref(own)
        kr.check_equal(f"bucket {b} distinct records", gk, wk)
        kr.check_equal(f"bucket {b} multiplicities", gc, wc)
        assert wk.shape[1] <= ln
        if wk.shape[1] == hi - lo:
            assert ln == hi - lo  # all different: nothing to merge, nothing may vanish
    assert res["dedup"] == sum(lens.values()), (res["dedup"], sum(lens.values()))
    # neighbours: buckets outside [b0, b1), the unused tail, the words behind it, every count nobody owns
    kr.check_equal("buckets below b0", out[:, :int(st[b0])], recs[:, :int(st[b0])])
    kr.check_equal("buckets from b1 on", out[:, int(st[b1]):n], recs[:, int(st[b1]):n])
    # (what the buckets reserved in the tail, [over0, cursor), is theirs: a bucket that still overflows after
    # some split passes, or whose last attempt lists fewer entries than an earlier one, leaves records there)
    free = ~written
    free[:n] = False
    free[res["over0"]:min(res["cursor"], res["limit"])] = False
    assert np.all(out[:, free] == TAIL), "the overflow tail outside the reserved part was written"
    nobody = ~written
    nobody[res["over0"]:min(res["cursor"], res["limit"])] = False
    kr.check_fill(cnt[nobody], FILL)
    kr.check_fill(dlen[:b0], FILL)
    kr.check_fill(dlen[b1:], FILL)
    kr.check_fill(dpos[[b for b in range(nb) if kinds.get(b) != "over"]], FILL)
    assert res["cursor"] == res["over0"] + (reserved if cursor_moves else 0), (res["cursor"], res["over0"], reserved)
    return kinds, lens


def check_paths(kinds, starts, b0, b1, other, must_miss=()):
    """Which path a bucket took, asserted only as far as count_rec_k fixes it.

    A bucket of no or one record is always a list at the front of its range:
    nothing races with it. Any other bucket that fits the table is normally
    such a list too, but not always: insert gives a lane 8 steps, and a claim
    lost to another lane, or a group re-read while another wave has written
    only the first word of its entry, uses a step like a full group does. A
    lane that runs out reports the table full, and the bucket then takes the
    path of a bucket that does not fit: `other` ('over' with room in the tail,
    'raw' without a tail). That costs dedup or tail space, never a count (the
    kernel's header comment says so), and check_count_rec has verified the
    lists whichever path was taken. It was seen for about one bucket in two
    thousand. So: every bucket outside must_miss (those that cannot fit by
    counting entries) is a list or `other`, and at least half of those with
    two or more records are lists. A P5a that needlessly leaves the table
    shows as most buckets, a lost race as one or two."""
    sz = np.diff(starts.astype(np.int64))
    multi = [b for b in range(b0, b1) if sz[b] >= 2 and b not in must_miss]
    for b in range(b0, b1):
        if sz[b] <= 1:
            assert kinds[b] == "list", f"bucket {b} of {sz[b]} records is {kinds[b]}"
        elif b not in must_miss:
            assert kinds[b] in ("list", other), f"bucket {b} is {kinds[b]}"
    assert 2 * sum(kinds[b] == "list" for b in multi) >= len(multi) > 0


def p5a_input(k=25, seed=4):
    """Reference records (W = 1) regrouped into 300 designed buckets. The
    record bodies come from skm_runs_ref over genome reads; the bucket field
    is rewritten (P5a never looks at a record's content). Buckets by index:
    0..2 as they come, 3 empty, 4 one record, 5 one record 3000 times, 6 all
    different (400), 7 the largest: 3000 different records, 8 600 different
    records 3 times each, 9 empty, from 10 on 0..40 records drawn with
    repeats, the last one empty."""
    g = kr.skm_geom_ref(100, k)
    reads = skm_reads.genome_reads(100, 4000, seed, genome=30000)
    body = np.unique(kr.skm_runs_ref(reads, k, g)["records"] & np.array([[LOW48], [~U64(0)]]), axis=1)
    assert body.shape[1] >= 4000
    rng = np.random.default_rng(seed)
    body = body[:, rng.permutation(body.shape[1])]
    parts = []

    def add(b, idx):
        r = body[:, idx].copy()
        r[0] |= U64(b) << U64(48)
        parts.append(r)

    nb = 300
    for b in range(nb):
        if b in (3, 9, nb - 1):
            continue
        if b == 4:
            idx = np.array([7])
        elif b == 5:
            idx = np.full(3000, 11)
        elif b == 6:
            idx = np.arange(100, 500)
        elif b == 7:
            idx = np.arange(500, 3500)
        elif b == 8:
            idx = rng.permutation(np.repeat(np.arange(3400, 4000), 3))
        else:
            idx = rng.integers(0, 60, size=int(rng.integers(0, 41))) + 13 * b
        add(b, idx)
    recs = np.concatenate(parts, axis=1)
    grouped, starts = kr.group_records(recs, nb)
    return grouped, starts


@pytest.fixture(scope="module")
def p5a_case():
    return p5a_input()


def test_count_rec_default_table(shim, p5a_case):
    """The production table: every bucket here fits it, so buckets are lists
    at the front of their own ranges (see check_paths for the exception) and
    none stays raw: the tail has room for whatever leaves the table."""
    recs, starts = p5a_case
    entries = 2 * shim.L.kcs_p5a_groups()
    assert entries > 2 * 3000, "the largest bucket must fit the table with room to probe"
    nb = starts.size - 1
    res = run_count_rec(shim, recs, starts, 0, nb, room=8000)
    kinds, lens = check_count_rec(res, recs, starts, 0, nb, cursor_moves=True)
    check_paths(kinds, starts, 0, nb, "over")
    # path-independent: empty, one record, all different (400 and 3000)
    assert (lens[3], lens[9], lens[4], lens[6], lens[7]) == (0, 0, 1, 400, 3000)
    # one record 3000 times and 600 records 3 times each: listed, so shorter than the bucket
    assert lens[5] < 3000 and lens[8] < 1800


def test_count_rec_range_from_b0(shim, p5a_case):
    recs, starts = p5a_case
    res = run_count_rec(shim, recs, starts, 5, 200, room=8000)
    kinds, _ = check_count_rec(res, recs, starts, 5, 200, cursor_moves=True)
    check_paths(kinds, starts, 5, 200, "over")


def test_count_rec_overflow_lists(shim, p5a_case, monkeypatch):
    """A table of 128 entries. Buckets 6 and 8 (400 and 600 distinct records)
    cannot fit it, so they go to the hash-split passes, and bucket 7 (3000
    distinct records) cannot fit 16 splits of it either (some class holds at
    least 188), so it stays raw: both follow from counting entries. A split
    pass can lose races like a first attempt (check_paths), and here only
    the last level, 16 passes of about 25 and 38 records, fits with ease: a
    bucket ended raw there in about one run of ten, so for 6 and 8 'over'
    is not asserted. With 512 entries bucket 8 (600 distinct records) still
    cannot fit, and its classes fit at 2, 4, 8 and 16 splits alike: it ends
    raw only if some pass loses its races at each of the four levels (of
    the order of 1e-5 from the rate above), so there its overflow list is
    asserted."""
    recs, starts = p5a_case
    monkeypatch.setenv("KC_P5A_GROUPS", "64")
    assert shim.L.kcs_p5a_groups() > 64
    nb = starts.size - 1
    res = run_count_rec(shim, recs, starts, 0, nb, room=8000)
    kinds, lens = check_count_rec(res, recs, starts, 0, nb, cursor_moves=True)
    assert kinds[6] in ("over", "raw") and kinds[8] in ("over", "raw")
    assert lens[6] == 400 and (kinds[8] == "raw" or lens[8] < 1800)
    assert kinds[7] == "raw"
    check_paths(kinds, starts, 0, nb, "over", must_miss=(6, 7, 8))
    monkeypatch.setenv("KC_P5A_GROUPS", "256")
    res = run_count_rec(shim, recs, starts, 0, nb, room=8000)
    kinds, lens = check_count_rec(res, recs, starts, 0, nb, cursor_moves=True)
    assert kinds[8] == "over" and 600 <= lens[8] < 1800
    assert kinds[7] in ("over", "raw") and lens[7] == 3000
    check_paths(kinds, starts, 0, nb, "over", must_miss=(7, 8))


def test_count_rec_no_split(shim, p5a_case, monkeypatch):
    """KC_P5A_NO_SPLIT: a bucket that fills the table stays raw and the cursor is never moved."""
    recs, starts = p5a_case
    monkeypatch.setenv("KC_P5A_GROUPS", "64")
    monkeypatch.setenv("KC_P5A_NO_SPLIT", "1")
    nb = starts.size - 1
    res = run_count_rec(shim, recs, starts, 0, nb, room=8000)
    kinds, _ = check_count_rec(res, recs, starts, 0, nb, cursor_moves=False)
    assert kinds[6] == kinds[7] == kinds[8] == "raw"  # more distinct records than entries
    check_paths(kinds, starts, 0, nb, "raw", must_miss=(6, 7, 8))
    # the same without a cursor at all
    monkeypatch.delenv("KC_P5A_NO_SPLIT")
    res = run_count_rec(shim, recs, starts, 0, nb, room=8000, use_over=False)
    kinds, _ = check_count_rec(res, recs, starts, 0, nb, cursor_moves=False)
    assert kinds[6] == kinds[7] == kinds[8] == "raw"
    check_paths(kinds, starts, 0, nb, "raw", must_miss=(6, 7, 8))


def test_count_rec_tail_too_small(shim, p5a_case, monkeypatch):
    """An overflow tail of 300 records: no overflowing bucket here (400, 1800
    and 3000 records) finds room, all stay raw; the cursor still counts what
    they asked for."""
    recs, starts = p5a_case
    monkeypatch.setenv("KC_P5A_GROUPS", "64")
    nb = starts.size - 1
    res = run_count_rec(shim, recs, starts, 0, nb, room=300, grid=1)
    kinds, _ = check_count_rec(res, recs, starts, 0, nb, cursor_moves=True)
    assert kinds[6] == kinds[7] == kinds[8] == "raw"  # they cannot fit the table, and the tail has no room
    check_paths(kinds, starts, 0, nb, "raw", must_miss=(6, 7, 8))
    assert res["cursor"] > res["limit"]


def test_count_rec_rejects_bad_arguments(shim, p5a_case):
    recs, starts = p5a_case
    n, nb = recs.shape[1], starts.size - 1
    buf = np.zeros((2, n + 100), dtype=U64)
    cnt, dlen, dpos = np.zeros(n + 100, np.uint32), np.zeros(nb, np.uint32), np.zeros(nb, U64)
    c = ctypes.c_uint64(0)

    def call(st, stride, over0, limit):
        return shim.L.kcs_count_rec(_p(buf), stride, _p(st), nb, 0, nb, 1, over0, limit, 0, FILL, _p(cnt), _p(dlen),
                                    _p(dpos), ctypes.addressof(c), ctypes.addressof(c))

    bad = starts.copy()
    bad[5], bad[6] = bad[6], bad[5] + U64(1)
    assert call(bad, n + 100, n, n + 100) == shim.invalid          # starts not ascending
    assert call(starts, n - 1, n, n) == shim.invalid               # starts past the stride
    assert call(starts, n + 100, n, n + 101) == shim.invalid       # tail past the stride
    assert call(starts, n + 100, n - 1, n + 100) == shim.invalid   # tail inside the buckets


# ---------------------------------------------------------------------------
# P5: count_skm_k<W>
# ---------------------------------------------------------------------------

def p5_input(k, L, n_reads, seed, *, genome=2500, merge=6, fat=0):
    """Reference records of mixed reads, grouped by their own bucket (ranked
    densely and `merge` neighbours taken together, so that a key still lives
    in one bucket and a bucket holds a few hundred distinct keys), shaped for
    P5's edges: bucket 5 is empty, three of the larger buckets are cut to 1,
    64 and 65 records (the per-wave record stage holds 64), the bucket before
    the last is empty and the last holds padding records (n = 0, bucket
    0xffff), which F leaves behind the real ones and P5 must never walk. fat:
    buckets from 10 on are taken together into bucket 10 while it stays under
    `fat` distinct keys (keys of different buckets differ, so the numbers add).
    Returns (g, recs (RW, n), starts, nb, b1): count [b0, b1) with b1 = nb - 1."""
    g = kr.skm_geom_ref(L, k)
    reads = (skm_reads.edge_reads(L, k, seed) + skm_reads.special_reads(L, n_reads // 8, seed) +
             skm_reads.genome_reads(L, n_reads, seed, genome=genome))
    recs = kr.skm_runs_ref(reads, k, g)["records"]
    bk, n = kr.record_fields(recs)
    uniq, dense = np.unique(bk, return_inverse=True)
    dense = dense // merge
    dense = dense + (dense >= 5)
    if fat:
        _, keys, rec = kr.skm_expand_ref(recs, g)
        dk, _ = kr.count_keys_ref(np.concatenate([dense[rec].astype(U64)[None, :], keys], axis=0))
        nd = np.bincount(dk[0].astype(np.int64), minlength=int(dense.max()) + 1)
        j = int(np.searchsorted(np.cumsum(nd[10:]), fat, side="left"))  # buckets 10 .. 10 + j - 1 stay under fat
        assert j >= 2 and 10 + j < dense.max()
        dense[(dense >= 10) & (dense < 10 + j)] = 10
    size = np.bincount(dense)
    big = np.argsort(size, kind="stable")[-8:-5]  # (the largest stay whole: the sub-range passes need them)
    assert size[big].min() >= 65, size[big]
    keep = np.ones(recs.shape[1], dtype=bool)
    for bb, cut in zip(big, (1, 64, 65)):
        keep[np.flatnonzero(dense == bb)[cut:]] = False
    recs, dense = recs[:, keep].copy(), dense[keep]
    recs[0] = (recs[0] & LOW48) | (dense.astype(U64) << U64(48))
    nreal_b = int(dense.max()) + 2  # + one empty bucket
    grouped, starts = kr.group_records(recs, nreal_b)
    pad = np.zeros((g["RW"], 5), dtype=U64)
    pad[0] = U64(0xffff) << U64(48)
    grouped = np.concatenate([grouped, pad], axis=1)
    starts = np.append(starts, U64(grouped.shape[1]))
    nb = nreal_b + 1
    sz = np.diff(starts.astype(np.int64))
    assert sz[5] == 0 and sz[nb - 2] == 0 and sz[nb - 1] == 5 and {1, 64, 65} <= set(sz.tolist())
    return g, grouped, starts, nb, nb - 1


def run_count_skm(shim, g, recs, starts, nb, b0, b1, *, lcap=0, dd=None, rec_cap=None, table_cap=1 << 15, probe=64,
                  spill_cap=None, count_keys=True, grid=0, expect_rc=0):
    """P5 through the shim. table_cap and probe (the global table's slots and
    its probe limit) are inputs that the tests choose, not library constants."""
    W, k = g["W"], g["k"]
    stride = recs.shape[1]
    nkeys = int(kr.record_fields(recs)[1].sum())
    if dd is not None:
        stride = dd["recs"].shape[1]
        recs = dd["recs"]
    rec_cap = nkeys + 64 if rec_cap is None else rec_cap
    spill_cap = nkeys + 64 if spill_cap is None else spill_cap
    sw = shim.L.kcs_slot_words(W)
    rk = np.zeros((W, rec_cap), dtype=U64)
    rc_ = np.zeros(rec_cap, dtype=np.uint32)
    rd = np.zeros(rec_cap, dtype=np.uint8)
    table = np.zeros((table_cap, sw), dtype=U64)
    spill = np.zeros((W, spill_cap), dtype=U64)
    stats = np.zeros(shim.st_n, dtype=U64)
    cur = ctypes.c_uint64(0)
    recs = np.ascontiguousarray(recs)
    rc = shim.L.kcs_count_skm(W, k, _p(recs), stride, _p(starts), nb, b0, b1, int(count_keys), lcap, grid,
                              _p(dd["cnt"]) if dd else None, _p(dd["dlen"]) if dd else None,
                              _p(dd["dpos"]) if dd else None, rec_cap, table_cap, probe, spill_cap, FILL, _p(rk),
                              _p(rc_), _p(rd), ctypes.addressof(cur), _p(table), _p(spill), _p(stats))
    assert rc == expect_rc, f"kcs_count_skm: {rc}"
    return dict(keys=rk, cnts=rc_, dig=rd, cursor=int(cur.value), table=table, spill=spill, stats=stats,
                rec_cap=rec_cap, spill_cap=spill_cap)


def bucket_distinct(g, recs, starts, b1):
    """Distinct keys of every bucket of [0, b1)."""
    hi = int(starts[b1])
    _, keys, rec = kr.skm_expand_ref(recs[:, :hi], g)
    kb = (recs[0, :hi] >> U64(48)).astype(np.int64)[rec]
    dk, _ = kr.count_keys_ref(np.concatenate([kb.astype(U64)[None, :], keys], axis=0))
    return np.bincount(dk[0].astype(np.int64), minlength=b1)


def p5_reference(g, recs, starts, b0, b1):
    """(distinct keys, counts, number of keys) of the records of buckets [b0, b1)."""
    lo, hi = int(starts[b0]), int(starts[b1])
    _, keys, _ = kr.skm_expand_ref(recs[:, lo:hi], g)
    dk, dc = kr.count_keys_ref(keys)
    return dk, dc, keys.shape[1]


def check_count_skm(res, g, want_keys, want_cnts, *, overflow=False):
    """Test 7: emitted records + occupied table slots + spill entries sum to
    the reference counts, exactly; no key is emitted twice; rec_dig; the fill
    behind the cursor. Returns (emitted, in the table, spilled) key counts."""
    W = g["W"]
    st = res["stats"]
    cur = res["cursor"]
    assert cur <= res["rec_cap"]
    ek, ec = res["keys"][:, :cur], res["cnts"][:cur]
    kr.check_fill(res["keys"][:, cur:], FILL)
    kr.check_fill(res["cnts"][cur:], FILL)
    kr.check_fill(res["dig"][cur:], FILL)
    assert np.all(ec >= 1)
    kr.check_equal("rec_dig", res["dig"][:cur], ((ek[0] >> U64(48)) & U64(255)).astype(np.uint8))
    uk, _ = kr.count_keys_ref(ek)
    assert uk.shape[1] == cur, f"{cur - uk.shape[1]} keys emitted twice"
    t = res["table"]
    occ = t[:, 0] != 0 if W == 1 else (t[:, W] >> U64(32)) == U64(2)
    assert not t[~occ].any(), "an empty table slot holds something"
    assert int(occ.sum()) == int(st[ST_CLAIMED])
    tk, tc = t[occ, :W].T, (t[occ, W] & U64(0xffffffff)).astype(np.int64)
    ns = int(st[ST_SPILL2_FILL])
    if not overflow:
        assert ns <= res["spill_cap"] and int(st[ST_ERR]) == 0
    nsp = min(ns, res["spill_cap"])
    sk = res["spill"][:, :nsp]
    kr.check_fill(res["spill"][:, nsp:], FILL)
    if not overflow:
        gk, gc = kr.count_keys_ref(np.concatenate([ek, tk, sk], axis=1),
                                   np.concatenate([ec.astype(np.int64), tc, np.ones(nsp, dtype=np.int64)]))
        kr.check_equal("distinct keys", gk, want_keys)
        kr.check_equal("counts", gc, want_cnts)
    return cur, int(occ.sum()), nsp


P5_KS = [19, 31, 50, 62, 66, 94]  # W = 1, 2, 3, each with K' = k and K' = 32 W


@pytest.fixture(scope="module")
def p5_cases(shim):
    """One input per k, shared by the P5 tests: its fattest bucket holds just
    under a quarter of the production LDS slots in distinct keys."""
    cache = {}

    def get(k):
        if k not in cache:
            W = (k + 31) // 32
            cache[k] = p5_input(k, k + 70, {1: 2500, 2: 2000, 3: 2000}[W], k, genome={1: 2500, 2: 1500, 3: 1200}[W],
                                fat=shim.lds_slots(W) // 4)
        return cache[k]

    return get


@pytest.mark.parametrize("k", P5_KS)
def test_count_skm_counts_and_no_needless_fallback(shim, p5_cases, k):
    """The production table: every bucket's distinct keys stay under a quarter
    of the LDS slots, the fattest one just under it (checked here from the
    reference), so every bucket is
    counted in one pass in LDS: nothing claimed in the global table, nothing
    spilled, no pass aborted. Records with n = 1 and n = nmax, keys that
    straddle the record's word boundaries (key index 23, 24, 25 where nmax
    allows), buckets of 1, 64 and 65 records, empty buckets and the padding
    bucket behind b1 are all in this input."""
    g, recs, starts, nb, b1 = p5_cases(k)
    W = g["W"]
    _, n = kr.record_fields(recs[:, :int(starts[b1])])
    assert n.min() == 1 and n.max() == g["nmax"]
    assert g["nmax"] < 26 or n.max() >= 26  # key indices 23..25: bit offsets 62, 64, 66
    assert g["masked"] == (g["Kp"] == k)
    slots = shim.lds_slots(W)
    nd = bucket_distinct(g, recs, starts, b1)
    assert slots // 8 < nd.max() < slots // 4 and nd.max() == nd[10]
    wk, wc, nkeys = p5_reference(g, recs, starts, 0, b1)
    res = run_count_skm(shim, g, recs, starts, nb, 0, b1)
    emitted, in_table, spilled = check_count_skm(res, g, wk, wc)
    st = res["stats"]
    assert (int(st[ST_CLAIMED]), int(st[ST_SPILL2_FILL]), int(st[ST_P5_ABORTS])) == (0, 0, 0)
    assert in_table == 0 and spilled == 0 and emitted == wk.shape[1]
    assert int(st[ST_P5_PASSES]) == b1  # one pass per bucket, empty ones included
    assert int(st[ST_P5_KEYS]) == nkeys
    assert int(st[ST_ERR]) == 0


@pytest.mark.parametrize("k", [19, 62])
def test_count_skm_range_from_b0(shim, p5_cases, k):
    """Buckets [3, b1 - 2): only their keys are counted; count_keys off leaves ST_P5_KEYS alone."""
    g, recs, starts, nb, b1 = p5_cases(k)
    wk, wc, _ = p5_reference(g, recs, starts, 3, b1 - 2)
    res = run_count_skm(shim, g, recs, starts, nb, 3, b1 - 2, count_keys=False)
    check_count_skm(res, g, wk, wc)
    assert int(res["stats"][ST_P5_KEYS]) == 0 and int(res["stats"][ST_P5_PASSES]) == b1 - 5


@pytest.mark.parametrize("k", P5_KS)
@pytest.mark.parametrize("lcap", [64, 256])
def test_count_skm_subrange_passes(shim, p5_cases, k, lcap):
    """A small LDS table: buckets are counted in sub-range passes (more passes
    than buckets) and what still misses the table at the last level goes to
    the global table; the sums stay exact."""
    g, recs, starts, nb, b1 = p5_cases(k)
    # some bucket here holds more distinct keys than the table has slots: it cannot be counted in one pass
    assert bucket_distinct(g, recs, starts, b1).max() > lcap
    wk, wc, nkeys = p5_reference(g, recs, starts, 0, b1)
    res = run_count_skm(shim, g, recs, starts, nb, 0, b1, lcap=lcap)
    check_count_skm(res, g, wk, wc)
    st = res["stats"]
    assert int(st[ST_P5_PASSES]) > b1 and int(st[ST_P5_ABORTS]) > 0
    assert int(st[ST_P5_KEYS]) == nkeys and int(st[ST_ERR]) == 0


@pytest.mark.parametrize("k", [19, 50, 94])
def test_count_skm_last_resort(shim, p5_cases, k):
    """One LDS slot and a global table of 16 slots probed 4 deep: most keys
    reach the spill buffer, once per occurrence, and the sums stay exact. Then
    a spill buffer that is too small: ERR_SPILL_OVERFLOW and nothing written
    behind it (the shim checks the guard words)."""
    g, recs, starts, nb, b1 = p5_cases(k)
    wk, wc, nkeys = p5_reference(g, recs, starts, 0, b1)
    res = run_count_skm(shim, g, recs, starts, nb, 0, b1, lcap=1, table_cap=16, probe=4)
    emitted, in_table, spilled = check_count_skm(res, g, wk, wc)
    assert in_table == 16 and spilled > nkeys // 2
    res = run_count_skm(shim, g, recs, starts, nb, 0, b1, lcap=1, table_cap=16, probe=4, spill_cap=100)
    check_count_skm(res, g, wk, wc, overflow=True)
    assert int(res["stats"][ST_ERR]) & shim.err_spill
    assert int(res["stats"][ST_SPILL2_FILL]) > 100


@pytest.mark.parametrize("k", [31, 66])
def test_count_skm_record_overflow(shim, p5_cases, k):
    """A record buffer smaller than the distinct keys: the cursor ends past
    the capacity, ERR_REC_OVERFLOW is raised, nothing is written behind the
    buffers (the shim checks the guard words)."""
    g, recs, starts, nb, b1 = p5_cases(k)
    wk, _, _ = p5_reference(g, recs, starts, 0, b1)
    cap = wk.shape[1] // 3
    res = run_count_skm(shim, g, recs, starts, nb, 0, b1, rec_cap=cap)
    assert res["cursor"] > cap
    assert int(res["stats"][ST_ERR]) & shim.err_rec
    # what fits is still keys of this input with plausible counts
    wrote = res["cnts"] != np.uint32(int.from_bytes(bytes([FILL]) * 4, "little"))
    assert wrote.any()
    dk, _ = kr.count_keys_ref(res["keys"][:, wrote])
    both = kr.count_keys_ref(np.concatenate([dk, wk], axis=1))[0]
    assert both.shape[1] == wk.shape[1]


@pytest.mark.parametrize("mode", ["default", "overflow-lists"])
def test_count_skm_walks_dedup_lists(shim, monkeypatch, mode):
    """W = 1: P5a's lists (front-of-range lists, overflow lists in the tail
    and raw buckets together in the second mode) walked by P5 with their
    multiplicities give the counts of the original records; ST_P5_KEYS is the
    sum of n x multiplicity over the lists."""
    k = 25
    g, recs, starts, nb, b1 = p5_input(k, 100, 4000, 8, genome=1500)
    if mode == "overflow-lists":
        monkeypatch.setenv("KC_P5A_GROUPS", "16")
    room = recs.shape[1] // 2
    if mode == "overflow-lists":
        # 32 entries: a bucket of more than 32 distinct records cannot fit them and asks for a list of
        # its record count; the tail holds some of those lists and by far not all, so others stay raw
        room = 3000
        sz = np.diff(starts.astype(np.int64))[:b1]
        nd = np.array([np.unique(recs[:, int(starts[b]):int(starts[b + 1])], axis=1).shape[1] for b in range(b1)])
        # (every such bucket alone fits the tail, so whichever asks first gets its list)
        assert sz[nd > 32].sum() > 2 * room and sz[nd > 32].max() <= room and (sz == 1).any()
    dd = run_count_rec(shim, recs, starts, 0, b1, room=room)
    kinds, lens = check_count_rec(dd, recs, starts, 0, b1, cursor_moves=True)
    if mode == "default":
        check_paths(kinds, starts, 0, b1, "over")
        assert dd["dedup"] < int(starts[b1])
    else:
        assert {"list", "over", "raw"} <= set(kinds.values()), set(kinds.values())
    monkeypatch.delenv("KC_P5A_GROUPS", raising=False)
    wk, wc, nkeys = p5_reference(g, recs, starts, 0, b1)
    res = run_count_skm(shim, g, recs, starts, nb, 0, b1, dd=dd)
    check_count_skm(res, g, wk, wc)
    assert int(res["stats"][ST_P5_KEYS]) == nkeys
    assert (int(res["stats"][ST_CLAIMED]), int(res["stats"][ST_SPILL2_FILL])) == (0, 0)
    # and through sub-range passes, where a listed record is walked once per pass
    res = run_count_skm(shim, g, recs, starts, nb, 0, b1, dd=dd, lcap=64)
    check_count_skm(res, g, wk, wc)
    assert int(res["stats"][ST_P5_KEYS]) == nkeys


def test_count_skm_rejects_bad_arguments(shim, p5_cases):
    g, recs, starts, nb, b1 = p5_cases(19)
    # the padding bucket (n = 0) inside the range
    run_count_skm(shim, g, recs, starts, nb, 0, nb, expect_rc=shim.invalid)
    # a record with more keys than its bases hold
    bad = recs.copy()
    bad[-1, 3] |= U64(63)
    run_count_skm(shim, g, bad, starts, nb, 0, b1, expect_rc=shim.invalid)
    # a dedup list that leaves the buffers
    dd = dict(recs=recs, cnt=np.ones(recs.shape[1], np.uint32), dlen=np.full(nb, RAW, np.uint32),
              dpos=np.zeros(nb, U64))
    dd["dlen"][2] = OVER | 10
    dd["dpos"][2] = recs.shape[1] - 5
    run_count_skm(shim, g, recs, starts, nb, 0, b1, dd=dd, expect_rc=shim.invalid)
    # k outside W's range
    assert shim.L.kcs_count_skm(2, 31, _p(recs), recs.shape[1], _p(starts), nb, 0, b1, 0, 0, 0, None, None, None, 8, 8,
                                1, 8, FILL, *[_p(recs)] * 7) == shim.invalid
