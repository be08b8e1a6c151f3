"""Kernel-level tests of the canonical fold's two passes, canon_count_k<W> and
canon_split_k<W>, through libkc_kernel_shim.so (kcs_canon_count,
kcs_canon_split). The expected value of every record (cleared key m, reverse
complement r, stay = m <= r) comes from tests/canon_ref.py's strings; numpy
lays them out as the kernels must (the staying records packed and in order,
the flipped ones SoA and in order) and every array is compared element by
element, the untouched tails included.

Sizes: the passes work in tiles of T = kcs_filter_tile() = 1024 records, so
n = T-1, T, T+1 and 4T+1 (five tiles, the last of one record) are here beside
0, 1 and 2. k: the shift s = 64 W - 2 k is 0 at 32, 64 and 128 (the shift by
64 that must not happen), 2 at 31 and 95, 62 at 33 (the widest)."""
import ctypes
import os

import numpy as np
import pytest

import canon_ref

pytestmark = pytest.mark.gpu

FILL = 0xC7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_PATH = os.path.join(ROOT, "kmer-counter_amd", "libkc_kernel_shim.so")
KS = [31, 32, 33, 64, 95, 128]
NS = [0, 1, 2, 1023, 1024, 1025, 4097]


def rec_dtype(W):
    return np.dtype([("key", "<u8", (W,)), ("cnt", "<u4")])


@pytest.fixture(scope="module")
def shim(kca):
    kca.lib()  # libkc_hip.so first: the shim links it
    if not os.path.exists(SHIM_PATH):
        raise ImportError(f"{SHIM_PATH} is missing: run `make -C kmer-counter_amd`")
    L = ctypes.CDLL(SHIM_PATH)
    vp, u64, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    L.kcs_filter_tile.restype = u64
    L.kcs_canon_count.argtypes = [i, i, u64, vp, vp]
    L.kcs_canon_split.argtypes = [i, i, u64, vp, vp, vp, vp, vp, vp, vp, i]
    assert L.kcs_filter_tile() == 1024
    return L


def expected(data, k):
    """(stay mask, m keys, r keys, counts) of every record, from strings."""
    W = (k + 31) // 32
    recs = canon_ref.kmer_ref_py.parse_records(data, k)
    n = len(recs)
    stay = np.zeros(n, dtype=bool)
    m = np.zeros((n, W), dtype=np.uint64)
    r = np.zeros((n, W), dtype=np.uint64)
    cnt = np.zeros(n, dtype=np.uint32)
    for i, (words, c) in enumerate(recs):
        s = canon_ref.key_to_bases(words)[:k]
        rc = canon_ref.revcomp(s)
        stay[i] = s <= rc
        m[i] = canon_ref.bases_to_key(s, W)
        r[i] = canon_ref.bases_to_key(rc, W)
        cnt[i] = c
    return stay, m, r, cnt


def check(shim, data, k, n):
    W = (k + 31) // 32
    rs = 8 * W + 4
    T = 1024
    nt = (n + T - 1) // T
    assert len(data) == n * rs
    stay, m, r, cnt = expected(data, k)
    want_cnt = np.array([stay[t * T:(t + 1) * T].sum() for t in range(nt)], dtype=np.uint64)
    want_base = np.concatenate([[0], np.cumsum(want_cnt)[:-1]]).astype(np.uint64) if nt else want_cnt
    src = np.frombuffer(data, dtype=np.uint8).copy() if n else None
    p = src.ctypes.data if n else None

    tile_cnt = np.full(nt, 7, dtype=np.uint64)
    assert shim.kcs_canon_count(W, k, n, p, tile_cnt.ctypes.data if nt else None) == 0
    assert np.array_equal(tile_cnt, want_cnt)

    tile_cnt2 = np.full(nt, 7, dtype=np.uint64)
    base = np.full(nt, 7, dtype=np.uint64)
    n_stay = ctypes.c_uint64(99)
    stay_out = np.zeros(n, dtype=rec_dtype(W))
    fk = np.zeros((W, n), dtype=np.uint64)
    fc = np.zeros(n, dtype=np.uint32)
    ptr = (lambda a: a.ctypes.data) if n else (lambda a: None)
    rc = shim.kcs_canon_split(W, k, n, p, ptr(tile_cnt2), ptr(base), ctypes.addressof(n_stay), ptr(stay_out), ptr(fk),
                              ptr(fc), FILL)
    assert rc == 0, f"kcs_canon_split: {rc}"
    ns = int(stay.sum())
    nf = n - ns
    assert n_stay.value == ns
    assert np.array_equal(tile_cnt2, want_cnt) and np.array_equal(base, want_base)
    want_stay = np.frombuffer(bytes([FILL]) * (n * rs), dtype=rec_dtype(W)).copy()
    want_stay["key"][:ns] = m[stay]
    want_stay["cnt"][:ns] = cnt[stay]
    assert np.array_equal(stay_out["key"], want_stay["key"]) and np.array_equal(stay_out["cnt"], want_stay["cnt"])
    want_fk = np.full((W, n), int.from_bytes(bytes([FILL]) * 8, "little"), dtype=np.uint64)
    want_fc = np.full(n, int.from_bytes(bytes([FILL]) * 4, "little"), dtype=np.uint32)
    want_fk[:, :nf] = r[~stay].T
    want_fc[:nf] = cnt[~stay]
    assert np.array_equal(fk, want_fk) and np.array_equal(fc, want_fc)
    return ns, nf


@pytest.mark.parametrize("k", KS)
def test_all_staying(shim, k):
    for n in NS:
        ns, nf = check(shim, canon_ref.crafted(k, n, seed=k + n, kind="stay", hole=n % 2 == 1), k, n)
        assert nf == 0


@pytest.mark.parametrize("k", KS)
def test_all_flipped(shim, k):
    for n in NS:
        ns, nf = check(shim, canon_ref.crafted(k, n, seed=2 * k + n, kind="flip", tk=n > 2), k, n)
        assert ns == 0


@pytest.mark.parametrize("k", KS)
def test_mixed_with_palindromes_and_shared_words(shim, k):
    W = (k + 31) // 32
    for n in NS:
        data = canon_ref.crafted(k, n, seed=3 * k + n, kind="mixed", hole=n > 2, tk=n > 2)
        ns, nf = check(shim, data, k, n)
        if n >= 1023:
            assert ns > n // 8 and nf > n // 8
            key = np.frombuffer(data, dtype=rec_dtype(W))["key"]
            if k % 2 == 0:
                kmers = [canon_ref.key_to_bases(w)[:k] for w in key.tolist()]
                assert sum(x == canon_ref.revcomp(x) for x in kmers) > 10  # palindromes: they stay
            if W > 1:
                assert (key[1:, :W - 1] == key[:-1, :W - 1]).all(axis=1).sum() > n // 8  # words 0..W-2 shared
