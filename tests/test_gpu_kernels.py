"""Kernel-level tests of the radix grouping passes (rp_upsweep_k,
rp_scatter_k<NW,PAY>, rp_region_pos_k, sub_starts_k) and of the segment sort
(seg_sort_k<W>, seg_sort_lsd_k<W>, bucket_bounds_k, group_desc_k), driven
through libkc_kernel_shim.so (tools/kc_kernel_shim.cpp) with inputs shaped to
reach the kernels' internal edges. The references are plain numpy
(tests/kernel_ref.py, itself checked by tests/test_kernel_ref.py); everything
is integers, so every comparison is exact.

Edge sizes come from the library (kcs_rp_tile, kcs_seg_sort_cap, kcs_n_cu),
not from constants copied here. `tile_walk` restates rp_scatter_k's tile walk
so that each test can assert which walk its launch took.
"""
import ctypes
import os

import numpy as np
import pytest

import kernel_ref as kr

pytestmark = pytest.mark.gpu

U64 = np.uint64
RP_FILL = 0xEE
SEG_FILL = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_PATH = os.path.join(ROOT, "kmer-counter_amd", "libkc_kernel_shim.so")


class Shim:
    def __init__(self, kca):
        kca.lib()  # libkc_hip.so first: the shim links it
        if not os.path.exists(SHIM_PATH):
            raise ImportError(f"{SHIM_PATH} is missing: run `make -C kmer-counter_amd`")
        L = ctypes.CDLL(SHIM_PATH)
        vp, u64, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
        L.kcs_rp_tile.argtypes = [i, i]
        L.kcs_seg_sort_cap.argtypes = [i]
        L.kcs_err_seg_too_long.restype = u64
        L.kcs_rp_pass.argtypes = [i, i, u64, vp, u64, vp, vp, i, i, vp, i, i, i, vp, vp, u64, vp, i, vp, i, vp]
        L.kcs_seg_sort.argtypes = [i, u64, vp, vp, u64, u64, vp, vp, vp, vp, vp, u64, i, i, vp, vp, i, vp, vp, vp]
        L.kcs_finish_groups.argtypes = [i, u64, vp, vp, u64, i, i, vp, vp, i, vp, vp, vp, vp]
        self.L = L
        self.n_cu = L.kcs_n_cu()
        assert self.n_cu > 0
        self.too_long = L.kcs_err_seg_too_long()

    def tile(self, nw, pay):
        t = self.L.kcs_rp_tile(nw, int(pay))
        assert t > 0 and t % 1024 == 0
        return t

    def cap(self, w):
        c = self.L.kcs_seg_sort_cap(w)
        assert c > 1025
        return c


@pytest.fixture(scope="module")
def shim(kca):
    return Shim(kca)


def _p(a):
    return None if a is None else a.ctypes.data


# ---------------------------------------------------------------------------
# grouping passes
# ---------------------------------------------------------------------------

def tile_walk(ntiles, grid, n_cu):
    """rp_scatter_k's walk for a pass of ntiles tiles launched with `grid`:
    (xcd, tiles of every workgroup). Also asserts that the walk covers every
    tile once, which the kernel's index arithmetic must guarantee."""
    if grid == 0:
        grid = 2 * n_cu
    g = min(ntiles, max(grid // 2, 1))
    xcd = g % 8 == 0 and ntiles >= 8
    per = []
    for b in range(g):
        if xcd:
            tx = (ntiles + 7) >> 3
            per.append(list(range((b & 7) * tx + (b >> 3), min(ntiles, ((b & 7) + 1) * tx), g >> 3)))
        else:
            per.append(list(range(b, ntiles, g)))
    assert sorted(t for p in per for t in p) == list(range(ntiles))
    return xcd, per


def rp_pass(shim, words, pay, rstart, *, regional=False, digs=None, shift=0, dshift=0, eshift=None, in_aos=False,
            out_aos=False, grid=0):
    """One grouping pass through the shim. SoA buffers get a stride larger
    than n (the padding must come back untouched). Returns (out_words (NW, n),
    out_pay, emit, bases, ntiles)."""
    nw, n = words.shape
    nreg = len(rstart) - 1
    if in_aos:
        kin, istride = np.ascontiguousarray(words.T), 0
    else:
        istride = n + 3
        kin = np.full((nw, istride), U64(0x5151515151515151))
        kin[:, :n] = words
    ostride = 0 if out_aos else n + 5
    kout = np.zeros((n, nw) if out_aos else (nw, ostride), dtype=U64)
    pin = None if pay is None else np.ascontiguousarray(pay, dtype=np.uint32)
    pout = None if pay is None else np.zeros(n, dtype=np.uint32)
    emit = None if eshift is None else np.zeros(n, dtype=np.uint8)
    rs = np.ascontiguousarray(rstart, dtype=U64)
    bases = np.zeros(nreg * 256 + 1 if regional else 256, dtype=U64)
    nt = ctypes.c_uint64(0)
    dg = None if digs is None else np.ascontiguousarray(digs, dtype=np.uint8)
    rc = shim.L.kcs_rp_pass(nw, int(pay is not None), n, _p(kin), istride, _p(pin), _p(rs), nreg, int(regional),
                            _p(dg), shift, dshift, 0 if eshift is None else eshift, _p(emit), _p(kout), ostride,
                            _p(pout), RP_FILL, _p(bases), grid, ctypes.addressof(nt))
    assert rc == 0, f"kcs_rp_pass: hipError {rc}"
    if out_aos:
        out = np.ascontiguousarray(kout.T)
    else:
        kr.check_fill(kout[:, n:], RP_FILL)
        out = kout[:, :n]
    return out, pout, emit, bases, nt.value


def run_and_check(shim, words, pay, rstart, *, hist_shift, use_digs, **kw):
    """A pass and all of its checks; returns (out_words, out_pay, emit, bases, ntiles)."""
    dig = kr.digit_of(words[0], hist_shift)
    digs = dig.astype(np.uint8) if use_digs else None
    out, pout, emit, bases, nt = rp_pass(shim, words, pay, rstart, digs=digs, shift=hist_shift, dshift=hist_shift,
                                         **kw)
    regional = kw.get("regional", False)
    nreg = len(rstart) - 1
    tile = shim.tile(words.shape[0], pay is not None)
    assert nt == sum(-(-(int(rstart[r + 1]) - int(rstart[r])) // tile) for r in range(nreg))
    bounds = kr.check_grouped(kr.as_rows(out, pout), kr.as_rows(words, pay), dig, rstart, regional)
    kr.check_bases(bases, bounds, nreg, regional)
    if emit is not None:
        kr.check_emit(emit, out[0], kw["eshift"])
    return out, pout, emit, bases, nt


PATTERNS = ("uniform", "all0", "all254", "all255", "pair", "grouped", "reverse")


def make_items(nw, with_pay, n, pattern, shift, seed):
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 2**64, size=(nw, n), dtype=U64)
    if pattern == "uniform":
        d = None
    elif pattern.startswith("all"):
        d = np.full(n, int(pattern[3:]), dtype=U64)
    elif pattern == "pair":  # digits d and d ^ 1 share one word of packed u16 wave counters
        d = U64(100) + rng.integers(0, 2, size=n, dtype=U64)
    else:
        d = np.sort(rng.integers(0, 256, size=n, dtype=U64))
        if pattern == "reverse":
            d = d[::-1].copy()
    if d is not None:
        words[0] = (words[0] & ~(U64(255) << U64(shift))) | (d << U64(shift))
    pay = rng.integers(0, 2**32, size=n, dtype=np.uint32) if with_pay else None
    return words, pay


# (NW, pay, AoS in, AoS out): SoA -> SoA for every instantiation; AoS in, out
# or both without payload (the layouts P2 / P3 / P3b use)
VARIANTS = [(nw, pay, False, False) for nw in (1, 2, 3, 4) for pay in (False, True)] + \
           [(nw, False, ia, oa) for nw in (1, 2, 3, 4) for ia, oa in ((True, False), (False, True), (True, True))]
GRIDS = (6, 16, 32, 0)
# (digit shift, emit shift or None), rotated over the calls: group16's level 1,
# P3b's, a digit that is not byte aligned, no emit
SHIFTS = ((48, 56), (40, 8), (13, 27), (56, None))


def _vid(v):
    return f"NW{v[0]}{'p' if v[1] else ''}-{'aos' if v[2] else 'soa'}-{'aos' if v[3] else 'soa'}"


def _sizes(T):
    return {"1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "8T": 8 * T, "8T+1": 8 * T + 1, "9T-5": 9 * T - 5}


def _one_region(shim, variant, n, grid, pattern, k):
    nw, pay, ia, oa = variant
    shift, eshift = SHIFTS[k % len(SHIFTS)]
    words, p = make_items(nw, pay, n, pattern, shift, seed=1000 + 7 * k + nw)
    # AoS items of several words: the histogram reads the digit bytes (as P3b does)
    use_digs = (ia and nw > 1) or k % 3 == 2
    return run_and_check(shim, words, p, [0, n], hist_shift=shift, use_digs=use_digs, eshift=eshift, in_aos=ia,
                         out_aos=oa, grid=grid)


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_rp_one_region_up_to_a_tile(shim, variant):
    """n in {1, T-1, T, T+1}: one or two tiles, every grid and digit pattern."""
    T = shim.tile(variant[0], variant[1])
    k = 0
    for name in ("1", "T-1", "T", "T+1"):
        n = _sizes(T)[name]
        for grid in GRIDS:
            for pattern in PATTERNS:
                k += 1
                *_, nt = _one_region(shim, variant, n, grid, pattern, k)
                assert nt == (2 if name == "T+1" else 1)
                xcd, _ = tile_walk(nt, grid, shim.n_cu)
                assert not xcd


@pytest.mark.parametrize("size", ("8T", "8T+1", "9T-5"))
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_rp_one_region_both_tile_walks(shim, variant, size):
    """8 and 9 tiles: grid 6 walks them plainly on 3 workgroups, grid 16 takes
    the xcd walk on 8 (with 9 tiles, workgroups 5..7 get none), grid 32 and
    the default grid launch one workgroup per tile. SoA variants run every
    digit pattern on every grid; the AoS layouts (which change only the item
    loads and stores) every pattern on the xcd walk and uniform digits on the
    other grids."""
    T = shim.tile(variant[0], variant[1])
    n = _sizes(T)[size]
    aos = variant[2] or variant[3]
    k = 0
    for grid in GRIDS:
        for pattern in PATTERNS:
            k += 1
            if aos and grid != 16 and pattern != "uniform":
                continue
            *_, nt = _one_region(shim, variant, n, grid, pattern, k)
            assert nt == (8 if size == "8T" else 9)
            xcd, per = tile_walk(nt, grid, shim.n_cu)
            if grid == 6:
                assert not xcd and len(per) == 3
            if grid == 16:
                assert xcd and len(per) == 8
                assert [len(p) for p in per[5:]] == ([1, 1, 1] if nt == 8 else [0, 0, 0])


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_rp_one_region_more_than_64_tiles(shim, variant):
    """65T + 3: 66 tiles, two scan chunks of the histogram's position kernels.
    grid 32 is the xcd walk with step 2 (16 workgroups, 4 or 5 tiles each, the
    last eighth shorter), grid 6 the plain walk with 22 tiles per workgroup."""
    T = shim.tile(variant[0], variant[1])
    n = 65 * T + 3
    aos = variant[2] or variant[3]
    for k, (grid, pattern) in enumerate(((32, "uniform"), (6, "pair"), (0, "reverse"))):
        if aos and k > 0:
            break
        *_, nt = _one_region(shim, variant, n, grid, pattern, k)
        assert nt == 66
        xcd, per = tile_walk(nt, grid, shim.n_cu)
        if grid == 32:
            assert xcd and len(per) == 16 and max(len(p) for p in per) == 5 and min(len(p) for p in per) == 1
        if grid == 6:
            assert not xcd and [len(p) for p in per] == [22, 22, 22]


def _level1_regions(shim, nw, pay, T, seed):
    """Items whose first pass (bits 48..55) leaves 256 regions that include
    empty ones (among them the last) and regions of exactly T, T + 1 and 1
    items; returns level 1's output, its emitted bytes and the region table."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 60, size=256)
    counts[[0, 1, 2, 3, 4, 200, 255]] = [T, T + 1, 1, 0, 2 * T + 7, 0, 0]
    n = int(counts.sum())
    d1 = rng.permutation(np.repeat(np.arange(256, dtype=U64), counts))
    words = rng.integers(0, 2**64, size=(nw, n), dtype=U64)
    words[0] = (words[0] & ~(U64(255) << U64(48))) | (d1 << U64(48))
    p = rng.integers(0, 2**32, size=n, dtype=np.uint32) if pay else None
    out, pout, emit, bases, _ = run_and_check(shim, words, p, [0, n], hist_shift=48, use_digs=False, eshift=56,
                                              grid=0)
    rstart = np.append(bases, U64(n)).astype(np.int64)
    assert np.array_equal(np.diff(rstart), counts)
    return out, pout, emit, rstart


@pytest.mark.parametrize("nw,pay", [(1, False), (2, False), (1, True), (2, True), (3, True), (4, True)])
def test_rp_level2_over_the_regions_of_a_real_first_pass(shim, nw, pay):
    T = shim.tile(nw, pay)
    words, p, emit, rstart = _level1_regions(shim, nw, pay, T, seed=50 + nw)
    for grid in (16, 0):
        # LSD over the regions from the emitted bytes, as group16's level 2
        out, pout, _, _, nt = rp_pass(shim, words, p, rstart, digs=emit, dshift=56, grid=grid)
        dig = kr.digit_of(words[0], 56)
        bounds = kr.check_grouped(kr.as_rows(out, pout), kr.as_rows(words, p), dig, rstart, False)
        assert nt == int(np.sum(-(-np.diff(rstart) // T))) and nt >= 8
        # MSD inside the regions (P3b's shape), digit bytes and word 0 as the source
        for use_digs in (True, False):
            run_and_check(shim, words, p, rstart, hist_shift=40, use_digs=use_digs, regional=True, grid=grid)
    assert bounds[-1] == words.shape[1]


@pytest.mark.parametrize("nw", (1, 2, 3, 4))
def test_rp_p3_call_over_the_regions_of_a_real_first_pass(shim, nw):
    """The partition engine's P3 as part_p3 launches it, for every key width:
    no payload, AoS keys in (P2's layout), the LSD histogram over the 256
    regions from the digit bytes the first pass emitted, the scatter on
    word0 >> 56 emitting bits 40..47 (P3b's digit), output AoS (P3b follows)
    and SoA (it does not)."""
    T = shim.tile(nw, False)
    words, _, emit, rstart = _level1_regions(shim, nw, False, T, seed=60 + nw)
    dig = kr.digit_of(words[0], 56)
    assert np.array_equal(emit, dig.astype(np.uint8))
    for out_aos in (True, False):
        for grid in (16, 0):
            out, _, e40, bases, nt = rp_pass(shim, words, None, rstart, digs=emit, dshift=56, eshift=40, in_aos=True,
                                             out_aos=out_aos, grid=grid)
            assert nt == int(np.sum(-(-np.diff(rstart) // T))) and nt >= 8
            bounds = kr.check_grouped(kr.as_rows(out), kr.as_rows(words), dig, rstart, False)
            kr.check_bases(bases, bounds, 256, False)
            kr.check_emit(e40, out[0], 40)


@pytest.mark.parametrize("regional", (False, True), ids=("lsd", "regional"))
@pytest.mark.parametrize("nw,pay", [(1, False), (2, True), (3, False), (4, True)])
def test_rp_forty_short_regions_at_unaligned_starts(shim, nw, pay, regional):
    """Regions of 1..40 items, one tile each: 1, then the even lengths (every
    one starts at an odd index), then the odd ones: 30 odd starts, 11 of the
    16 offsets inside a 16-byte line. The histogram's 16-byte digit loads meet
    unaligned heads and tails and regions shorter than 16 bytes; digit source: the byte array, then word 0."""
    lens = [1] + list(range(2, 41, 2)) + list(range(3, 41, 2))
    assert sorted(lens) == list(range(1, 41))
    rstart = np.concatenate(([0], np.cumsum(lens)))
    assert sum(int(s) % 2 for s in rstart[:-1]) == 30 and len({int(s) % 16 for s in rstart[:-1]}) == 11
    n = int(rstart[-1])
    for k, pattern in enumerate(("uniform", "pair", "all255")):
        words, p = make_items(nw, pay, n, pattern, 8, seed=70 + k)
        for use_digs in (True, False):
            *_, nt = run_and_check(shim, words, p, rstart, hist_shift=8, use_digs=use_digs, regional=regional,
                                   eshift=16, grid=(16, 6, 0)[k])
            assert nt == 40


@pytest.mark.parametrize("nw,pay", [(2, False), (1, True), (2, True), (3, True), (4, True)])
def test_rp_two_level_composition_groups_by_16_bits(shim, nw, pay):
    """group16's two passes with its parameters: level 1 on bits 48..55 emits
    bits 56..63, level 2 runs over level 1's 256 regions from those bytes. The
    result is a stable sort by word0 >> 48 up to the order inside a group."""
    T = shim.tile(nw, pay)
    n = 9 * T + 11
    rng = np.random.default_rng(90 + nw)
    words = rng.integers(0, 2**64, size=(nw, n), dtype=U64)
    # a third of the items in 300 prefixes, so some 16-bit groups are long
    hot = rng.integers(0, 2**16, size=300, dtype=U64)
    sel = rng.random(n) < 0.33
    words[0, sel] = (words[0, sel] & U64(0xffffffffffff)) | (hot[rng.integers(0, 300, size=int(sel.sum()))] << U64(48))
    p = rng.integers(0, 2**32, size=n, dtype=np.uint32) if pay else None
    b, pb, digs, bases, nt1 = run_and_check(shim, words, p, [0, n], hist_shift=48, use_digs=False, eshift=56, grid=0)
    assert nt1 == 10
    rstart = np.append(bases, U64(n)).astype(np.int64)
    a, pa, _, _, _ = rp_pass(shim, b, pb, rstart, digs=digs, dshift=56, grid=0)
    pref = (words[0] >> U64(48)).astype(np.int64)
    gb = np.searchsorted(np.sort(pref), np.arange(65537))
    want = kr.as_rows(words, p)[np.argsort(pref, kind="stable")]
    got = kr.as_rows(a, pa)
    assert np.array_equal(got[:, 0] >> U64(48), want[:, 0] >> U64(48))
    assert np.array_equal(kr.canon_blocks(got, gb), kr.canon_blocks(want, gb))


# ---------------------------------------------------------------------------
# segment sort
# ---------------------------------------------------------------------------

PREFIX = U64(0xBEEF) << U64(48)
M48 = U64(0xffffffffffff)


def seg_sort(shim, keys, cnts, dstart, dlen, out_off, nout, *, packed, grid, order=None, dkey=None):
    """launch_seg_sort through the shim; returns (out, out_cnts, err, fb sorted)."""
    W, n = keys.shape
    nd = len(dstart)
    rk = np.zeros((W, n + 1), dtype=U64)  # one record of slack: see launch_seg_sort's comment
    rk[:, :n] = keys
    rc_ = np.zeros(n + 1, dtype=np.uint32)
    rc_[:n] = cnts
    order = np.arange(nd, dtype=np.uint32) if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    ds = np.ascontiguousarray(dstart, dtype=U64)
    dl = np.ascontiguousarray(dlen, dtype=np.uint32)
    oo = np.ascontiguousarray(out_off, dtype=U64)
    dk = None if dkey is None else np.ascontiguousarray(dkey, dtype=U64)
    if packed:
        out, oc = np.zeros((nout, 8 * W + 4), dtype=np.uint8), None
    else:
        out, oc = np.zeros((W, nout), dtype=U64), np.zeros(nout, dtype=np.uint32)
    err, fbn = ctypes.c_uint64(0), ctypes.c_uint64(0)
    fb = np.zeros(nd, dtype=np.uint32)
    rc = shim.L.kcs_seg_sort(W, n, _p(rk), _p(rc_), n + 1, nd, _p(order), _p(ds), _p(dl), _p(oo), _p(dk), nout,
                             int(packed), SEG_FILL, _p(out), _p(oc), grid, ctypes.addressof(err),
                             ctypes.addressof(fbn), _p(fb))
    assert rc == 0, f"kcs_seg_sort: hipError {rc}"
    assert fbn.value <= nd
    return out, oc, err.value, sorted(int(x) for x in fb[:fbn.value])


def check_seg(out, oc, keys, cnts, segs, packed):
    if packed:
        kr.check_seg_packed(out, keys, cnts, segs, SEG_FILL)
    else:
        kr.check_seg_soa(out, oc, keys, cnts, segs, SEG_FILL)


def uniform_keys(rng, W, n):
    """Distinct keys under one 16-bit prefix, uniform in bits 0..47."""
    keys = rng.integers(0, 2**64, size=(W, n), dtype=U64)
    low = rng.choice(2**40, size=n, replace=False).astype(U64) << U64(8) | rng.integers(0, 256, size=n, dtype=U64)
    keys[0] = PREFIX | low
    return keys


def layout(lens, gap=3):
    """Segments one after the other in the records, `gap` sentinel records
    between their output ranges: (dstart, out_off, nout)."""
    dstart = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64) if len(lens) else np.zeros(0, np.int64)
    out_off = dstart + gap * (1 + np.arange(len(lens)))
    return dstart, out_off, int(sum(lens)) + gap * (len(lens) + 1)


def prefetched(shim, W):
    """Records of a segment that seg_sort_k holds in registers one segment
    ahead; a longer segment reads the rest in place."""
    C = shim.cap(W)
    return 1024 * min(-(-C // 1024), 6 // W)


@pytest.mark.parametrize("packed", (True, False), ids=("packed", "soa"))
@pytest.mark.parametrize("W", (1, 2, 3, 4))
def test_seg_sort_lengths(shim, W, packed):
    """Every edge length as its own segment of one launch. grid 2: two
    workgroups walk all of them, so the one-segment-ahead prefetch crosses
    empty, short, longer-than-prefetched and full segments; then the default
    grid. Uniform keys: the largest of 4096 bins stays far below 64, so the
    MSD kernel sorts every segment, the in-place tail loops included."""
    C, P = shim.cap(W), prefetched(shim, W)
    assert P < C
    lens = [C, 0, 1, P + 1, 2, 64, C - 1, 65, 1023, 0, P, 1024, 1025, P - 1, 1, 0]
    rng = np.random.default_rng(100 + W)
    n = sum(lens)
    keys = uniform_keys(rng, W, n)
    cnts = rng.integers(1, 2**32, size=n, dtype=np.uint32)
    dstart, out_off, nout = layout(lens)
    dlen = np.array(lens, dtype=np.uint32) | np.uint32(36 << 24)
    segs = list(zip(dstart.tolist(), lens, out_off.tolist()))
    for grid in (2, 0):
        out, oc, err, fb = seg_sort(shim, keys, cnts, dstart, dlen, out_off, nout, packed=packed, grid=grid)
        assert err == 0 and fb == []
        check_seg(out, oc, keys, cnts, segs, packed)


@pytest.mark.parametrize("W", (1, 2, 3, 4))
def test_seg_sort_skew_boundary(shim, W):
    """A largest bin of exactly 64 keys stays with the MSD kernel (the owner
    thread's insertion sort, or the rank loop for one-word keys, over a full
    bin); 65 hands the segment to the LSD kernel."""
    rng = np.random.default_rng(200 + W)
    lens = [3000, 3000, 500]
    n = sum(lens)
    keys = uniform_keys(rng, W, n)
    for s, big in ((0, 64), (1, 65)):
        lo = s * 3000
        d = ((keys[0, lo:lo + 3000] & M48) >> U64(36)).astype(np.int64)
        assert np.bincount(d, minlength=4096).max() < 20
        # bin 0x5a5 holds exactly `big` keys: the first `big` records move there, the rest leave it
        k0 = keys[0, lo:lo + 3000]
        k0[d == 0x5a5] ^= U64(1) << U64(36)
        k0[:big] = (k0[:big] & ~(U64(0xfff) << U64(36))) | (U64(0x5a5) << U64(36))
        d = ((k0 & M48) >> U64(36)).astype(np.int64)
        cnt = np.bincount(d, minlength=4096)
        assert cnt[0x5a5] == big and np.sort(cnt)[-2] < 20
    assert np.unique(keys[0]).size == n
    cnts = rng.integers(1, 2**32, size=n, dtype=np.uint32)
    dstart, out_off, nout = layout(lens)
    dlen = np.array(lens, dtype=np.uint32) | np.uint32(36 << 24)
    segs = list(zip(dstart.tolist(), lens, out_off.tolist()))
    for packed in (True, False):
        out, oc, err, fb = seg_sort(shim, keys, cnts, dstart, dlen, out_off, nout, packed=packed, grid=0)
        assert err == 0 and fb == [1]
        check_seg(out, oc, keys, cnts, segs, packed)


@pytest.mark.parametrize("W", (1, 2, 3, 4))
def test_seg_sort_lsd_shapes(shim, W):
    """Segments whose keys share bits 36..47 of word 0 (one bin, more than 64
    keys), so all of them go to seg_sort_lsd_k, whose passes run over the
    bytes that vary inside the segment only."""
    C = shim.cap(W)
    rng = np.random.default_rng(300 + W)
    const = rng.integers(0, 2**64, size=W, dtype=U64)
    const[0] = PREFIX | (const[0] & M48)

    def fixed(m):
        return np.repeat(const[:, None], m, axis=1)

    parts = []
    a = fixed(200)  # only byte 0 of word 0 varies
    a[0] = (a[0] & ~U64(255)) | rng.permutation(256)[:200].astype(U64)
    parts.append(a)
    if W >= 2:  # only bytes of the last word vary
        b = fixed(3000)
        b[W - 1] = rng.choice(2**62, size=3000, replace=False).astype(U64)
        parts.append(b)
    # C - 1 keys that differ in the two low bytes of the last word, and one that
    # also differs in a single high byte (bits 32..35 of a one-word key: the
    # bin bits above them stay shared)
    c = fixed(C)
    c[W - 1] = (c[W - 1] & ~U64(0xffff)) | rng.permutation(65536)[:C].astype(U64)
    c[W - 1, C // 3] ^= (U64(0x5) << U64(32)) if W == 1 else (U64(0x81) << U64(56))
    parts.append(c)
    # full length, everything below the bin bits random
    e = rng.integers(0, 2**64, size=(W, C), dtype=U64)
    e[0] = (const[0] & ~((U64(1) << U64(36)) - U64(1))) | rng.choice(2**36, size=C, replace=False).astype(U64)
    parts.append(e)
    lens = [p.shape[1] for p in parts]
    keys = np.concatenate(parts, axis=1)
    n = keys.shape[1]
    cnts = rng.integers(1, 2**32, size=n, dtype=np.uint32)
    dstart, out_off, nout = layout(lens)
    dlen = np.array(lens, dtype=np.uint32) | np.uint32(36 << 24)
    segs = list(zip(dstart.tolist(), lens, out_off.tolist()))
    for packed in (True, False):
        for grid in (2, 0):
            out, oc, err, fb = seg_sort(shim, keys, cnts, dstart, dlen, out_off, nout, packed=packed, grid=grid)
            assert err == 0 and fb == list(range(len(lens)))
            check_seg(out, oc, keys, cnts, segs, packed)
    # 70 identical keys with different counts: no byte varies, the counts come through
    same = fixed(70)
    sc = np.arange(1, 71, dtype=np.uint32) * np.uint32(1000003)
    out, oc, err, fb = seg_sort(shim, same, sc, [0], [70 | (36 << 24)], [2], 75, packed=False, grid=0)
    assert err == 0 and fb == [0]
    kr.check_seg_soa(out, oc, same, sc, [(0, 70, 2)], SEG_FILL)


@pytest.mark.parametrize("W", (1, 2, 3, 4))
def test_seg_sort_equal_keys_in_the_msd_kernel(shim, W):
    """Pairs and triples of equal keys with different counts (what several
    batches leave before they are summed): W = 1 ranks them by LDS position,
    W >= 2 by the insertion sort."""
    rng = np.random.default_rng(400 + W)
    lens = [3000, 1, 2500]
    n = sum(lens)
    keys = uniform_keys(rng, W, n)
    for lo, m in ((0, 3000), (3001, 2500)):
        src = lo + rng.choice(m, size=300, replace=False)
        keys[:, src[100:200]] = keys[:, src[:100]]           # 100 pairs
        keys[:, src[200:250]] = keys[:, src[:50]]            # 50 of them triples
    cnts = rng.integers(1, 2**32, size=n, dtype=np.uint32)
    dstart, out_off, nout = layout(lens)
    dlen = np.array(lens, dtype=np.uint32) | np.uint32(36 << 24)
    segs = list(zip(dstart.tolist(), lens, out_off.tolist()))
    for grid in (1, 0):
        out, oc, err, fb = seg_sort(shim, keys, cnts, dstart, dlen, out_off, nout, packed=False, grid=grid)
        assert err == 0 and fb == []
        kr.check_seg_soa(out, oc, keys, cnts, segs, SEG_FILL)


@pytest.mark.parametrize("packed", (True, False), ids=("packed", "soa"))
@pytest.mark.parametrize("W", (1, 2, 3, 4))
def test_seg_sort_explicit_descriptors_and_presorted_copy(shim, W, packed):
    """The partition engine's descriptor form: `order` a permutation, dkey the
    segment's lower bound, a shift under which the segment's key range spans
    fewer than 4096 bins (keys in base + [0, 2^42), shift 30); and presorted
    segments (bit 31), which are copied. The presorted ones share bits 36..47
    and are longer than 64, so sorting them would need the LSD kernel: an
    empty fallback list shows that they were copied.

    The copy is capped like the sort: the register prefetch clamps a segment
    longer than seg_sort_cap(W) to nothing, so its first records would all be
    copies of the first one. The library's presorted runs (sort_runs_keys(W))
    are shorter; the shim rejects such a descriptor. Lengths here: 1, P + 1
    (the in-place tail of the copy) and the capacity."""
    C, P = shim.cap(W), prefetched(shim, W)
    rng = np.random.default_rng(500 + W)
    sorted_lens = [2000, 0, P + 5, 700, 1, 300]
    pres_lens = [1, P + 1, C]
    parts, dkey_of, lens, flags = [], [], [], []
    for i, m in enumerate(sorted_lens):
        base = U64(int(rng.integers(0, 2**48 - 2**42)))
        k = rng.integers(0, 2**64, size=(W, m), dtype=U64)
        k[0] = PREFIX | (base + rng.choice(2**42, size=m, replace=False).astype(U64))
        parts.append(k)
        dkey_of.append(int(PREFIX | base))  # bits 48.. are masked off by the kernel
        lens.append(m)
        flags.append(30 << 24)
    for m in pres_lens:
        k = rng.integers(0, 2**64, size=(W, m), dtype=U64)
        k[0] = PREFIX | (U64(0x123) << U64(36)) | rng.choice(2**36, size=m, replace=False).astype(U64)
        k = k[:, np.lexsort([k[j] for j in range(W - 1, -1, -1)])]
        parts.append(k)
        dkey_of.append(0)
        lens.append(m)
        flags.append((36 << 24) | (1 << 31))
    keys = np.concatenate(parts, axis=1)
    n = keys.shape[1]
    cnts = rng.integers(1, 2**32, size=n, dtype=np.uint32)
    nd = len(lens)
    dstart = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    dlen = np.array(lens, dtype=np.uint32) | np.array(flags, dtype=np.uint32)
    order = rng.permutation(nd).astype(np.uint32)
    assert not np.array_equal(order, np.arange(nd))
    # position di sorts descriptor order[di]; out_off and dkey go by position
    plens = [lens[o] for o in order]
    _, out_off, nout = layout(plens, gap=2)
    dkey = np.array([dkey_of[o] for o in order], dtype=U64)
    segs = [(int(dstart[o]), lens[o], int(out_off[di])) for di, o in enumerate(order)]
    for grid in (2, 0):
        out, oc, err, fb = seg_sort(shim, keys, cnts, dstart, dlen, out_off, nout, packed=packed, grid=grid,
                                    order=order, dkey=dkey)
        assert err == 0 and fb == []
        check_seg(out, oc, keys, cnts, segs, packed)


def test_shim_rejects_a_presorted_segment_past_the_capacity(shim):
    """The contract above, kept by the shim before anything is launched."""
    C = shim.cap(1)
    n = C + 1
    keys = np.arange(n, dtype=U64)[None, :] | PREFIX
    rk = np.zeros((1, n + 1), dtype=U64)
    rk[:, :n] = keys
    rcn = np.ones(n + 1, dtype=np.uint32)
    order = np.zeros(1, dtype=np.uint32)
    ds, oo = np.zeros(1, dtype=U64), np.zeros(1, dtype=U64)
    dl = np.array([n | (1 << 31)], dtype=np.uint32)
    out = np.zeros((n, 12), dtype=np.uint8)
    err, fbn = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = shim.L.kcs_seg_sort(1, n, _p(rk), _p(rcn), n + 1, 1, _p(order), _p(ds), _p(dl), _p(oo), None, n, 1,
                             SEG_FILL, _p(out), None, 0, ctypes.addressof(err), ctypes.addressof(fbn), None)
    assert rc == 1  # hipErrorInvalidValue
    assert not out.any()


@pytest.mark.parametrize("packed", (True, False), ids=("packed", "soa"))
@pytest.mark.parametrize("W", (1, 2, 3, 4))
def test_seg_sort_too_long_is_a_status_code(shim, W, packed):
    """A segment of capacity + 1 without bit 31: ERR_SEG_TOO_LONG is set, its
    output range keeps the sentinel, the launch's other segments are sorted."""
    C = shim.cap(W)
    rng = np.random.default_rng(600 + W)
    lens = [500, C + 1, 700]
    n = sum(lens)
    keys = uniform_keys(rng, W, n)
    cnts = rng.integers(1, 2**32, size=n, dtype=np.uint32)
    dstart, out_off, nout = layout(lens)
    dlen = np.array(lens, dtype=np.uint32) | np.uint32(36 << 24)
    segs = [(int(dstart[i]), lens[i], int(out_off[i])) for i in (0, 2)]
    out, oc, err, fb = seg_sort(shim, keys, cnts, dstart, dlen, out_off, nout, packed=packed, grid=2)
    assert err == shim.too_long
    assert fb == []
    check_seg(out, oc, keys, cnts, segs, packed)  # the range of segment 1 counts as outside: sentinel


def finish_groups(shim, keys, cnts, packed, grid=0):
    W, n = keys.shape
    rk = np.zeros((W, n + 1), dtype=U64)
    rk[:, :n] = keys
    rcn = np.zeros(n + 1, dtype=np.uint32)
    rcn[:n] = cnts
    if packed:
        out, oc = np.zeros((n, 8 * W + 4), dtype=np.uint8), None
    else:
        out, oc = np.zeros((W, n), dtype=U64), np.zeros(n, dtype=np.uint32)
    starts = np.zeros(65537, dtype=U64)
    longest, err, fbn = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = shim.L.kcs_finish_groups(W, n, _p(rk), _p(rcn), n + 1, int(packed), SEG_FILL, _p(out), _p(oc), grid,
                                  _p(starts), ctypes.addressof(longest), ctypes.addressof(err),
                                  ctypes.addressof(fbn))
    assert rc == 0, f"kcs_finish_groups: hipError {rc}"
    return out, oc, starts, longest.value, err.value, fbn.value


def grouped_records(rng, W, n, big):
    """n records grouped by word0 >> 48: no group below prefix 5 or above
    65000, one group (prefix 0x8001) of exactly `big` records."""
    pref = rng.integers(5, 65001, size=n - big, dtype=U64)
    pref[pref == U64(0x8001)] = U64(0x8002)
    pref = np.sort(np.concatenate((pref, np.full(big, U64(0x8001)))))
    big = int(np.sum(pref == U64(0x8001)))
    keys = rng.integers(0, 2**64, size=(W, n), dtype=U64)
    keys[0] = (pref << U64(48)) | rng.choice(2**40, size=n, replace=False).astype(U64) << U64(8) | \
        rng.integers(0, 256, size=n, dtype=U64)
    return keys, pref.astype(np.int64), big


@pytest.mark.parametrize("W", (1, 2, 3, 4))
def test_finish_groups_sequence(shim, W):
    """bucket_bounds -> group_desc -> seg_sort as the skm finish runs them,
    over 70,000 grouped records with empty groups at both ends of the prefix
    range (the trailing ones read the record of slack) and one group of
    exactly the capacity; then a group of capacity + 1, which is only
    reported."""
    C = shim.cap(W)
    n = 70000
    rng = np.random.default_rng(700 + W)
    keys, pref, big = grouped_records(rng, W, n, C)
    assert big == C
    cnts = rng.integers(1, 2**32, size=n, dtype=np.uint32)
    want_starts = np.searchsorted(pref, np.arange(65537))
    assert want_starts[5] == 0 and want_starts[65001] == n
    segs = [(int(want_starts[g]), int(want_starts[g + 1] - want_starts[g]), int(want_starts[g]))
            for g in range(65536)]
    for packed in (True, False):
        out, oc, starts, longest, err, fbn = finish_groups(shim, keys, cnts, packed)
        assert np.array_equal(starts.astype(np.int64), want_starts)
        assert longest == C and err == 0
        check_seg(out, oc, keys, cnts, segs, packed)
    keys, pref, big = grouped_records(rng, W, n, C + 1)
    assert big == C + 1
    *_, longest, _, _ = finish_groups(shim, keys, cnts, True)
    assert longest == C + 1
