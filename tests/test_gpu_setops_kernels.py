"""The set-operation passes between two packed runs (merge_split_packed_k,
setop_tile_k count and emit around the tile-count scan), driven through
libkc_kernel_shim.so's kcs_setop. Every expected value comes from setops_ref.

T = kcs_setop_tile(W) merged positions per tile (2048 at W <= 2, 1024 at
W >= 3); a thread decides 8 (W <= 2) or 4 consecutive positions of a tile. The
two records of a shared key are neighbours in the merged order, A's first, and
the position of A's record owns the pair: the cases put such pairs on tile
boundaries, on every thread's boundary, and around them.

Each call returns the whole output buffer: outside [out_skip, out_skip + n_out)
it must still hold the shim's fill, and the guard words behind the split array
and the tile counts must be intact (a negative return code otherwise)."""
import ctypes
import os

import numpy as np
import pytest

import setops_ref as sr
from setops_ref import COUNT_SUBTRACT, INTERSECT, SUBTRACT, SUM, UNION

pytestmark = pytest.mark.gpu

FILL = 0xC7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_PATH = os.path.join(ROOT, "kmer-counter_amd", "libkc_kernel_shim.so")
WS = (1, 2, 3, 4)
ALL_OPS = (UNION, INTERSECT, SUBTRACT, COUNT_SUBTRACT)
INVALID = 1  # hipErrorInvalidValue


def _p(a):
    return a.ctypes.data if a is not None and a.size else None


class SetOp:
    def __init__(self, kca):
        kca.lib()  # libkc_hip.so first: the shim links it
        if not os.path.exists(SHIM_PATH):
            raise ImportError(f"{SHIM_PATH} is missing: run `make -C kmer-counter_amd`")
        L = ctypes.CDLL(SHIM_PATH)
        vp, u64, u32, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        L.kcs_setop_tile.argtypes = [i]
        L.kcs_merge_tile.argtypes = [i]
        L.kcs_setop.argtypes = [i, vp, u64, vp, u64, u64, u64, u64, u32, u32, i, vp, u64, i, vp, vp, vp, vp]
        self.L = L
        self.guard = L.kcs_guard_clobbered()

    def tile(self, W):
        t = self.L.kcs_setop_tile(W)
        assert t >= 512 and t % 256 == 0
        return t

    def raw(self, W, a, b, op, mode, *, skips=(0, 0, 0), grid_cap=8192, slack=3):
        """kcs_setop's return code, the whole output (records x rs bytes),
        n_out, the output pointer modulo 16, tiles, workgroups."""
        rs = 8 * W + 4 if 1 <= W <= 4 else a.dtype.itemsize
        out = np.zeros((skips[2] + len(a) + len(b) + slack, rs), dtype=np.uint8)
        n_out, al = ctypes.c_uint64(1 << 40), ctypes.c_uint32(99)
        nt, wg = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = self.L.kcs_setop(W, _p(a), len(a), _p(b), len(b), skips[0], skips[1], skips[2], op, mode, grid_cap,
                              _p(out), out.shape[0], FILL, ctypes.addressof(n_out), ctypes.addressof(al),
                              ctypes.addressof(nt), ctypes.addressof(wg))
        return rc, out, n_out.value, al.value, nt.value, wg.value

    def check(self, W, a, b, mode, *, skips=(0, 0, 0), grid_cap=8192, ops=ALL_OPS):
        """All four operations of (a, b) against the reference; `mode` goes to
        UNION and INTERSECT. Returns (tiles, workgroups)."""
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        ref = sr.combine if len(a) + len(b) <= 600 else sr.combine_vec
        for op in ops:
            m = mode if op in (UNION, INTERSECT) else SUM
            want = ref(a, b, op, m)
            rc, out, n_out, al, nt, wg = self.raw(W, a, b, op, m, skips=skips, grid_cap=grid_cap)
            what = (W, len(a), len(b), op, m, skips, grid_cap)
            assert rc != self.guard, f"{what}: a guard word behind the splits or the tile counts was overwritten"
            assert rc == 0, f"{what}: hipError {rc}"
            assert al == (skips[2] * (8 * W + 4)) % 16
            assert n_out == len(want), what
            lo, hi = skips[2], skips[2] + n_out
            assert out[lo:hi].tobytes() == want.tobytes(), what
            assert (out[:lo] == FILL).all() and (out[hi:] == FILL).all(), f"{what}: a store outside the output range"
            T = self.tile(W)
            assert nt == (len(a) + len(b) + T - 1) // T and wg == min(nt, grid_cap)
        return nt, wg


@pytest.fixture(scope="module")
def so(kca):
    return SetOp(kca)


def test_tile_is_the_merge_tile(so):
    for W in WS:
        assert so.tile(W) == so.L.kcs_merge_tile(W)  # merge_split_packed_k cuts the tiles of both
    assert so.L.kcs_setop_tile(0) == 0 and so.L.kcs_setop_tile(5) == 0


@pytest.mark.parametrize("W", WS)
def test_sizes_with_a_third_of_the_keys_shared(so, W):
    T = so.tile(W)
    modes = set()
    for i, n in enumerate([1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, 5 * T + 3]):
        a, b = sr.split_runs(W, n, seed=n + W, hole=(n % 2 == 1 and n > 2, n > 2 and n % 4 == 1))
        if n > 2:
            shared = len(sr.combine_vec(a, b, INTERSECT, SUM))
            assert 0.25 < shared / (len(a) + len(b) - shared) < 0.42
        mode = i % 5
        modes.add(mode)
        so.check(W, a, b, mode)
        if n <= 2:  # both orders, and the lone pair
            so.check(W, b, a, (mode + 1) % 5)
    one = sr.run_of(sr.key_pool(W, 1, 3), 4)
    for mode in range(5):  # na + nb = 2 as one shared key: every mode on a single pair
        other = one.copy()
        other["cnt"] = sr.U32 - 1
        so.check(W, one, other, mode)
    assert modes == set(range(5))


@pytest.mark.parametrize("W", WS)
def test_one_operand_empty(so, W):
    T = so.tile(W)
    a = sr.run_of(sr.key_pool(W, T + 1, 5 + W), 6, hole=False)
    e = a[:0]
    so.check(W, a, e, 1)
    so.check(W, e, a, 2)
    hole = sr.run_of(sr.key_pool(W, T, 7 + W), 8, hole=True)
    assert len(hole) == T + 1
    so.check(W, hole, e, 3)
    so.check(W, e, hole, 4)
    # both empty: nothing is launched, nothing is written
    rc, out, n_out, _, nt, _ = so.raw(W, e, e, UNION, SUM)
    assert (rc, n_out, nt) == (0, 0, 0) and (out == FILL).all()


@pytest.mark.parametrize("W", WS)
def test_a_run_with_itself(so, W):
    """Every merged position belongs to a pair. As they stand the pairs sit
    at (0, 1), (2, 3), ...: none is cut. After one A-only or B-only record in
    front they sit at (1, 2), (3, 4), ...: every thread's last position (a
    thread decides 4 or 8) and the tile's last position hold A's record of a
    pair whose B record the next thread, or the next tile, holds."""
    T = so.tile(W)
    for hole in (False, True):
        a = sr.run_of(sr.key_pool(W, T // 2 + 1 - int(hole), 9 + W), 10, hole=hole)
        assert len(a) == T // 2 + 1
        for mode in range(5):
            so.check(W, a, a.copy(), mode)
        b = sr.run_of(a["key"][int(hole):], 11, hole=hole)  # the same keys, other counts
        so.check(W, a, b, 0)
        # shifted by one position: pairs at odd positions, on every thread boundary
        first = np.zeros(1, dtype=a.dtype)
        first["key"][0, W - 1] = 1  # below every key of the pool, above the hole
        first["cnt"] = 5
        if not hole:
            so.check(W, np.concatenate([first, a]), b, 1)
            so.check(W, a, np.concatenate([first, b]), 2)


def straddle_runs(W, p, n_total, seed):
    """Runs whose merged order has A's record of a shared key at position p and
    B's at p + 1, among A-only, B-only and shared keys at random."""
    rng = np.random.default_rng(seed)
    tags, pos = [], 0
    while pos < n_total:
        if pos == p:
            t = 2
        else:
            t = int(rng.integers(0, 3))
            limit = p if pos < p else n_total
            if t == 2 and pos + 2 > limit:
                t = int(rng.integers(0, 2))
        tags.append(t)
        pos += 2 if t == 2 else 1
    tags = np.array(tags)
    keys = sr.key_pool(W, len(tags), seed + 1)
    return sr.run_of(keys[tags != 1], seed + 2), sr.run_of(keys[tags != 0], seed + 3)


@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("tiles", [1, 2])
def test_pair_across_a_tile_boundary(so, W, tiles):
    T = so.tile(W)
    for s in range(4):
        p = tiles * T - 2 + s  # A's record at p, B's at p + 1: (T-2, T-1), (T-1, T), (T, T+1), (T+1, T+2)
        a, b = straddle_runs(W, p, (tiles + 1) * T + 5, seed=W * 100 + tiles * 10 + s)
        from_a, idx = sr.merged_positions(a, b)
        assert from_a[p] and not from_a[p + 1], "the pair is not where the test means it to be"
        assert (a["key"][idx[p]] == b["key"][idx[p + 1]]).all()
        if s == 1:  # the pair cut by the tile boundary
            assert p // T + 1 == (p + 1) // T == tiles
        # counts that tell the owner: a > b, so COUNT_SUBTRACT keeps a - b
        a["cnt"][idx[p]], b["cnt"][idx[p + 1]] = 1000, 1
        nt, _ = so.check(W, a, b, s % 5)
        assert nt == tiles + 2
        so.check(W, a, b, (s + 2) % 5, grid_cap=1)


@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("grid_cap", [1, 2])
def test_workgroups_walk_several_tiles(so, W, grid_cap):
    T = so.tile(W)
    a, b = sr.split_runs(W, 5 * T + 3, seed=31 + W, hole=(True, True))
    nt, wg = so.check(W, a, b, (grid_cap + W) % 5, grid_cap=grid_cap)
    assert (nt, wg) == (6, grid_cap)


@pytest.mark.parametrize("W", WS)
def test_alignment_of_the_runs_and_the_output(so, W):
    """skip 0: a 16-byte-aligned start; skip 1: one aligned to 4 bytes only (a
    record is 8 W + 4 bytes). The tile bases move the output's alignment as
    well, so both store paths run in every case."""
    T = so.tile(W)
    a, b = sr.split_runs(W, 2 * T + 1, seed=41 + W, hole=(False, True))
    i = 0
    for a_skip in (0, 1):
        for b_skip in (0, 1):
            for out_skip in (0, 1):
                so.check(W, a, b, i % 5, skips=(a_skip, b_skip, out_skip))
                i += 1
    so.check(W, a, b, 0, skips=(3, 2, 3), grid_cap=2)


@pytest.mark.parametrize("W", WS)
def test_keys_that_differ_in_one_word_only(so, W):
    """Leading words all equal (the last word decides), and last words all
    equal (an earlier word decides): a comparison that stops early or starts
    late merges or pairs these wrongly."""
    T = so.tile(W)
    n = T + 7
    rng = np.random.default_rng(W)
    for word in range(W):
        pool = np.full((n, W), 6, dtype=np.uint64)
        v = np.unique(rng.integers(1, 1 << 36, n + 64, dtype=np.uint64))
        assert len(v) >= n
        pool[:, word] = np.sort(rng.permutation(v)[:n]) << np.uint64(24)
        tag = rng.integers(0, 3, n)
        a, b = sr.run_of(pool[tag != 1], 50 + word), sr.run_of(pool[tag != 0], 60 + word)
        so.check(W, a, b, word % 5)
    # high and low halves of a word: the dwords of a packed key word
    pool = np.zeros((4, W), dtype=np.uint64)
    pool[:, W - 1] = [1, 1 << 31, 1 << 32, (1 << 63) + 5]
    a, b = sr.run_of(pool[[0, 2, 3]], 70), sr.run_of(pool[[1, 2, 3]], 71)
    so.check(W, a, b, 2)


def test_argument_errors_launch_nothing(so):
    a, b = sr.split_runs(2, 50, seed=1)
    for W, op, mode, cap in [(0, 0, 0, 8192), (5, 0, 0, 8192), (2, 4, 0, 8192), (2, 0, 5, 8192), (2, 0, 0, 0),
                             (2, 0xFFFFFFFF, 0, 8192), (2, 1, 0xFFFFFFFF, 8192), (2, 0, 0, -1)]:
        rc, out, n_out, *_ = so.raw(W, a, b, op, mode, grid_cap=cap)
        assert rc == INVALID, (W, op, mode, cap)
        assert (out == 0).all()  # refused before any allocation: the host buffer was never written


def test_shim_refuses_unsorted_and_repeated_keys(so):
    a, b = sr.split_runs(1, 40, seed=2)
    swapped = a.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    twice = np.concatenate([a[:5], a[4:]])
    for x, y in [(swapped, b), (b, swapped), (twice, b), (b, twice)]:
        assert so.raw(1, x, y, UNION, SUM)[0] == INVALID
    rs = 12
    out = np.zeros((len(a) + len(b) - 1, rs), dtype=np.uint8)  # one record short
    n_out = ctypes.c_uint64(0)
    assert so.L.kcs_setop(1, _p(a), len(a), _p(b), len(b), 0, 0, 0, 0, 0, 8192, _p(out), out.shape[0], FILL,
                          ctypes.addressof(n_out), None, None, None) == INVALID
