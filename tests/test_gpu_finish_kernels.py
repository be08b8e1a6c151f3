"""Kernel-level tests of the sort, scan, reduce, compact and merge primitives
under the finished run: scan_reduce / scan_single / scan_down, key_bits,
sort_upsweep / sort_downsweep<W, HAS_VALS>, rle_heads / rle_scatter /
rle_counts_k, reduce_add_k, pack_records, unpack_records_k, compact_count /
compact_emit / append_key0, merge_split_k / merge_tile_k, merge_split_packed_k /
merge_tile_packed_k, owner_bounds_k, bucket_bounds_k's AoS form and
packed_seg_copy_k, driven through libkc_kernel_shim.so
(tools/kc_kernel_shim.cpp). Keys are built for the purpose; the references are
plain numpy (tests/kernel_ref.py, itself checked by tests/test_kernel_ref.py).
Everything is integers and every kernel here has one right answer, order
included, so every comparison is exact and element by element.

Edge sizes come from the library's getters (kcs_merge_tile, kcs_sort_tile,
kcs_scan_tile, kcs_compact_grid, kcs_elem_grid_cap), not from constants copied
here, and each test asserts the property that makes its case an edge: the
tile count, the tiles of every workgroup, the output index of a straddling
pair, the alignment of the output pointer, scan_single's partials per thread.
The *_walk functions restate the kernels' index arithmetic for that purpose.

launch_sort_pass's hashed = true form (the digit taken from the key hash) has
no caller in the library's host files and is not tested here.
"""
import ctypes
import os

import numpy as np
import pytest

import kernel_ref as kr

pytestmark = pytest.mark.gpu

U64 = np.uint64
U32 = np.uint32
FILL = 0xC7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM_PATH = os.path.join(ROOT, "kmer-counter_amd", "libkc_kernel_shim.so")
WS = (1, 2, 3, 4)
B_BASE = U32(2**31)  # counts: A's are i, B's are 2^31 + i, so every output record names its source


def _p(a):
    return None if a is None else a.ctypes.data


class Finish:
    """The shim's entry points for the finish primitives, with the buffers
    (padded, pre-filled by the shim with FILL) allocated here."""

    def __init__(self, kca):
        kca.lib()  # libkc_hip.so first: the shim links it
        if not os.path.exists(SHIM_PATH):
            raise ImportError(f"{SHIM_PATH} is missing: run `make -C kmer-counter_amd`")
        L = ctypes.CDLL(SHIM_PATH)
        vp, u64, u32, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        for name in ("kcs_merge_tile", "kcs_sort_tile", "kcs_slot_words"):
            getattr(L, name).argtypes = [i]
        L.kcs_sort_grid.argtypes = [u64]
        L.kcs_scan.argtypes = [i, u64, vp, vp, u64, i, i]
        L.kcs_key_bits.argtypes = [i, u64, vp, u64, vp]
        L.kcs_sort_pass.argtypes = [i, u64, vp, vp, u64, i, i, i, vp, vp, i]
        L.kcs_rle_chain.argtypes = [i, u64, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, i]
        L.kcs_reduce_chain.argtypes = [i, u64, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, i]
        L.kcs_pack.argtypes = [i, u64, vp, vp, u64, vp, u64, i]
        L.kcs_unpack.argtypes = [i, u64, vp, vp, u64, vp, i]
        L.kcs_compact.argtypes = [i, u64, vp, u64, u64, i, u64, vp, vp, u64, vp, i]
        L.kcs_merge.argtypes = [i, vp, vp, u64, u64, vp, vp, u64, u64, i, u64, vp, vp, u64, i, i, vp, vp]
        L.kcs_merge_packed.argtypes = [i, vp, u64, vp, u64, u64, u64, u64, i, vp, u64, i, vp, vp, vp, vp]
        L.kcs_owner_bounds.argtypes = [i, u64, vp, u32, vp, u64, i]
        L.kcs_bucket_bounds.argtypes = [i, u64, vp, u64, i, vp, u64, i]
        L.kcs_packed_seg_copy.argtypes = [i, u64, vp, u64, vp, u64, vp, vp, vp, vp, u64, i, i]
        self.L = L
        self.guard = L.kcs_guard_clobbered()
        self.scan_tile = L.kcs_scan_tile()
        self.compact_grid = L.kcs_compact_grid()
        self.elem_cap = L.kcs_elem_grid_cap()
        assert self.scan_tile > 256 and self.scan_tile % 256 == 0 and self.compact_grid > 0 and self.elem_cap > 0

    def ok(self, what, rc):
        assert rc != self.guard, f"{what}: the guard word behind a scratch buffer of the library's own sizing was overwritten"
        assert rc == 0, f"{what}: hipError {rc}"

    def merge_tile(self, W):
        t = self.L.kcs_merge_tile(W)
        assert t >= 512 and t % 256 == 0
        return t

    def sort_tile(self, W):
        t = self.L.kcs_sort_tile(W)
        assert t >= 512 and t % 256 == 0
        return t

    # -- entry points --

    def scan(self, a, inplace):
        out = np.zeros(a.size + 5, dtype=a.dtype)
        self.ok("kcs_scan", self.L.kcs_scan(int(a.dtype == np.uint32), a.size, _p(a), _p(out), out.size, int(inplace),
                                            FILL))
        return out

    def key_bits(self, keys, stride):
        W, n = keys.shape
        buf = _strided(keys, stride)
        out = np.zeros(2 * W, dtype=U64)
        self.ok("kcs_key_bits", self.L.kcs_key_bits(W, n, _p(buf), stride, _p(out)))
        return out

    def sort_pass(self, keys, vals, word, shift, grid):
        W, n = keys.shape
        S = n + 3
        kin = _strided(keys, S)
        vin = None if vals is None else _strided1(vals, S)
        ko = np.zeros((W, S), dtype=U64)
        vo = None if vals is None else np.zeros(S, dtype=U32)
        self.ok("kcs_sort_pass", self.L.kcs_sort_pass(W, n, _p(kin), _p(vin), S, word, shift, grid, _p(ko), _p(vo),
                                                      FILL))
        return ko, vo

    def chain(self, keys, cnts=None):
        """kcs_rle_chain (cnts None) or kcs_reduce_chain: everything the chain wrote, whole buffers."""
        W, n = keys.shape
        S, OS = n + 3, n + 5
        kin = _strided(keys, S)
        r = dict(flags=np.zeros(n, dtype=U32), pos=np.zeros(n, dtype=U32), keys=np.zeros((W, OS), dtype=U64),
                 cnts=np.zeros(OS, dtype=U32), packed=np.zeros((OS, 8 * W + 4), dtype=np.uint8))
        m = ctypes.c_uint64(0)
        if cnts is None:
            r["head"] = np.zeros(OS, dtype=U32)
            rc = self.L.kcs_rle_chain(W, n, _p(kin), S, _p(r["flags"]), _p(r["pos"]), ctypes.addressof(m),
                                      _p(r["keys"]), OS, _p(r["cnts"]), _p(r["head"]), _p(r["packed"]), FILL)
        else:
            cin = _strided1(cnts, S)
            rc = self.L.kcs_reduce_chain(W, n, _p(kin), _p(cin), S, _p(r["flags"]), _p(r["pos"]),
                                         ctypes.addressof(m), _p(r["keys"]), OS, _p(r["cnts"]), _p(r["packed"]), FILL)
        self.ok("kcs_rle_chain" if cnts is None else "kcs_reduce_chain", rc)
        r["m"] = m.value
        return r

    def pack(self, keys, cnts):
        W, n = keys.shape
        S = n + 3
        out = np.zeros((n + 2, 8 * W + 4), dtype=np.uint8)
        kin, cin = _strided(keys, S), _strided1(cnts, S)
        self.ok("kcs_pack", self.L.kcs_pack(W, n, _p(kin), _p(cin), S, _p(out), n + 2, FILL))
        return out

    def unpack(self, packed, W):
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        n = packed.shape[0]
        OS = n + 4
        ko = np.zeros((W, OS), dtype=U64)
        co = np.zeros(OS, dtype=U32)
        self.ok("kcs_unpack", self.L.kcs_unpack(W, n, _p(packed), _p(ko), OS, _p(co), FILL))
        return ko, co

    def compact(self, W, table, out_cap, key0_present, key0_count, pad=7):
        table = np.ascontiguousarray(table, dtype=U64)
        cap = table.shape[0]
        ko = np.zeros(W * out_cap + pad, dtype=U64)
        co = np.zeros(out_cap + pad, dtype=U32)
        cur = ctypes.c_uint64(0)
        self.ok("kcs_compact", self.L.kcs_compact(W, cap, _p(table), table.size, out_cap, int(key0_present),
                                                  key0_count, _p(ko), _p(co), pad, ctypes.addressof(cur), FILL))
        return ko, co, cur.value

    def merge(self, ka, ca, kb, cb, *, grid_cap=8192, a_off=None, strides=None):
        """launch_merge; a_off not None: A and B adjacent in one buffer at a_off.
        Returns (ko whole, co whole, output offset, ntiles, workgroups)."""
        W, na = ka.shape
        nb = kb.shape[1]
        nt, wg = ctypes.c_uint64(0), ctypes.c_uint64(0)
        if a_off is None:
            sa, sb, so = strides or (na + 3, nb + 4, na + nb + 5)
            A, CA, Bk, CB = _strided(ka, sa), _strided1(ca, sa), _strided(kb, sb), _strided1(cb, sb)
            off, adj = 0, 0
        else:
            sa = sb = a_off + na + nb + 3
            so = a_off + na + nb + 6
            A = _strided(np.concatenate([ka, kb], axis=1), sa, at=a_off)
            CA = _strided1(np.concatenate([ca, cb]), sa, at=a_off)
            Bk = CB = None
            off, adj = a_off, 1
        ko = np.zeros((W, so), dtype=U64)
        co = np.zeros(so, dtype=U32)
        self.ok("kcs_merge", self.L.kcs_merge(W, _p(A), _p(CA), sa, na, _p(Bk), _p(CB), sb, nb, adj, off, _p(ko),
                                              _p(co), so, grid_cap, FILL, ctypes.addressof(nt), ctypes.addressof(wg)))
        return ko, co, off, nt.value, wg.value

    def merge_packed(self, W, a, b, *, a_skip=0, b_skip=0, out_skip=0, grid_cap=8192):
        """launch_merge_packed over packed records a (na, rs), b (nb, rs).
        Returns (out whole, dup, out pointer % 16, ntiles, workgroups)."""
        rs = 8 * W + 4
        a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, rs)
        b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1, rs)
        na, nb = a.shape[0], b.shape[0]
        out = np.zeros((out_skip + na + nb + 2, rs), dtype=np.uint8)
        dup, al = ctypes.c_uint32(7), ctypes.c_uint32(99)
        nt, wg = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self.ok("kcs_merge_packed",
                self.L.kcs_merge_packed(W, _p(a) if na else None, na, _p(b) if nb else None, nb, a_skip, b_skip,
                                        out_skip, grid_cap, _p(out), out.shape[0], FILL, ctypes.addressof(dup),
                                        ctypes.addressof(al), ctypes.addressof(nt), ctypes.addressof(wg)))
        return out, dup.value, al.value, nt.value, wg.value

    def owner_bounds(self, W, packed, world):
        packed = np.ascontiguousarray(packed, dtype=np.uint8).reshape(-1, 8 * W + 4)
        n = packed.shape[0]
        out = np.zeros(world + 1 + 3, dtype=U64)
        self.ok("kcs_owner_bounds", self.L.kcs_owner_bounds(W, n, _p(packed) if n else None, world, _p(out), 3, FILL))
        return out

    def bucket_bounds(self, W, buf, n, stride, bits):
        out = np.zeros((1 << bits) + 1 + 3, dtype=U64)
        self.ok("kcs_bucket_bounds", self.L.kcs_bucket_bounds(W, n, _p(buf), stride, bits, _p(out), 3, FILL))
        return out

    def seg_copy(self, W, src, ndst, order, dstart, dlen, out_off, base, grid):
        src = np.ascontiguousarray(src, dtype=np.uint8).reshape(-1, 8 * W + 4)
        dst = np.zeros((ndst, 8 * W + 4), dtype=np.uint8)
        order = np.ascontiguousarray(order, dtype=U32)
        dstart = np.ascontiguousarray(dstart, dtype=U64)
        dlen = np.ascontiguousarray(dlen, dtype=U32)
        out_off = np.ascontiguousarray(out_off, dtype=U64)
        self.ok("kcs_packed_seg_copy",
                self.L.kcs_packed_seg_copy(W, src.shape[0], _p(src), ndst, _p(dst), order.size, _p(order), _p(dstart),
                                           _p(dlen), _p(out_off), base, grid, FILL))
        return dst


@pytest.fixture(scope="module")
def fin(kca):
    return Finish(kca)


PAD64 = U64(0x5151515151515151)


def _strided(words, stride, at=0):
    """(W, n) -> (W, stride) with the records at [at, at + n) and a pattern around them."""
    W, n = words.shape
    buf = np.full((W, stride), PAD64)
    buf[:, at:at + n] = words
    return buf


def _strided1(vals, stride, at=0):
    buf = np.full(stride, 0x51515151, dtype=U32)
    buf[at:at + len(vals)] = vals
    return buf


def lexorder(keys):
    """Stable order by the full key, word 0 most significant."""
    return np.lexsort([keys[j] for j in range(keys.shape[0] - 1, -1, -1)])


def test_shim_refuses_what_could_index_out_of_bounds(fin):
    """Checked on the host before anything is launched: hipErrorInvalidValue (1)."""
    L = fin.L
    k = np.array([[1, 2, 3, 5]], dtype=U64)
    bad = np.array([[1, 3, 2, 5]], dtype=U64)  # not sorted
    c = np.arange(4, dtype=U32)
    ko, co = np.zeros((1, 16), dtype=U64), np.zeros(16, dtype=U32)
    nt = ctypes.c_uint64(0)

    def merge(ka, kb, sa=4, sb=4, so=16):
        return L.kcs_merge(1, _p(ka), _p(c), sa, 4, _p(kb), _p(c), sb, 4, 0, 0, _p(ko), _p(co), so, 8192, FILL,
                           ctypes.addressof(nt), ctypes.addressof(nt))

    assert merge(bad, k) == 1 and merge(k, bad) == 1          # an unsorted run
    assert merge(k, k, sa=3) == 1 and merge(k, k, sb=3) == 1  # a stride shorter than n
    assert merge(k, k, so=7) == 1                             # an output shorter than na + nb
    out = np.zeros((10, 12), dtype=np.uint8)
    dup = ctypes.c_uint32(0)
    pk, pbad = kr.pack_records(k, c), kr.pack_records(bad, c)

    def merge_packed(a, b, out_recs=10, out_skip=0):
        return L.kcs_merge_packed(1, _p(a), 4, _p(b), 4, 0, 0, out_skip, 8192, _p(out), out_recs, FILL,
                                  ctypes.addressof(dup), None, None, None)

    assert merge_packed(pbad, pk) == 1 and merge_packed(pk, pbad) == 1
    assert merge_packed(pk, pk, out_recs=7) == 1 and merge_packed(pk, pk, out_skip=3) == 1
    table = np.zeros(4 * 10 - 1, dtype=U64)  # one word short of 10 slots at W = 2
    cur = ctypes.c_uint64(0)
    assert L.kcs_compact(2, 10, _p(table), table.size, 4, 0, 0, _p(ko), _p(co), 0, ctypes.addressof(cur), FILL) == 1
    assert L.kcs_sort_pass(1, 4, _p(k), None, 3, 0, 0, 0, _p(ko), None, FILL) == 1  # stride < n
    assert L.kcs_sort_pass(1, 4, _p(k), None, 4, 1, 0, 0, _p(ko), None, FILL) == 1  # word >= W
    m = ctypes.c_uint64(0)
    f, p = np.zeros(4, dtype=U32), np.zeros(4, dtype=U32)
    assert L.kcs_rle_chain(1, 4, _p(k), 4, _p(f), _p(p), ctypes.addressof(m), _p(ko), 3, _p(co), _p(co), _p(out),
                           FILL) == 1  # an output stride shorter than n
    src = np.zeros((5, 12), dtype=np.uint8)

    def seg(start, ln, off, base):
        order, ds, dl, do = np.zeros(1, dtype=U32), np.array([start], dtype=U64), np.array([ln], dtype=U32), \
            np.array([off], dtype=U64)
        return L.kcs_packed_seg_copy(1, 5, _p(src), 10, _p(out), 1, _p(order), _p(ds), _p(dl), _p(do), base, 1, FILL)

    assert seg(2, 4, 0, 0) == 1 and seg(0, 5, 6, 0) == 1 and seg(0, 5, 3, 3) == 1  # past the source, past the target


# ---------------------------------------------------------------------------
# scan
# ---------------------------------------------------------------------------

def scan_walk(n, tile):
    """(tiles = partials, partials per thread of scan_single's 1024 threads)."""
    m = -(-n // tile)
    return m, -(-m // 1024)


@pytest.mark.parametrize("inplace", (False, True), ids=("out", "inplace"))
@pytest.mark.parametrize("dt", (np.uint32, np.uint64), ids=("u32", "u64"))
def test_scan_sizes(fin, dt, inplace):
    """n around a thread's items, a wave, the block and the tile; random values
    whose u32 totals wrap many times."""
    T = fin.scan_tile
    rng = np.random.default_rng(31)
    for n, tiles in ((1, 1), (255, 1), (256, 1), (257, 1), (T - 1, 1), (T, 1), (T + 1, 2), (3 * T + 5, 4)):
        assert scan_walk(n, T) == (tiles, 1)
        a = rng.integers(0, 2**32, size=n, dtype=dt)
        kr.check_scan(fin.scan(a, inplace), a, FILL)
    for n in (257, 3 * T + 5):  # all zero, and ones (the rle chain's flags at their densest)
        kr.check_scan(fin.scan(np.zeros(n, dtype=dt), inplace), np.zeros(n, dtype=dt), FILL)
        kr.check_scan(fin.scan(np.ones(n, dtype=dt), inplace), np.ones(n, dtype=dt), FILL)


@pytest.mark.parametrize("inplace", (False, True), ids=("out", "inplace"))
@pytest.mark.parametrize("dt", (np.uint32, np.uint64), ids=("u32", "u64"))
def test_scan_single_sums_two_partials_per_thread(fin, dt, inplace):
    T = fin.scan_tile
    n = 1024 * T + 1
    assert scan_walk(n, T) == (1025, 2)
    rng = np.random.default_rng(32)
    a = rng.integers(0, 1000, size=n, dtype=dt)
    a[T - 1] = 2**32 - 5 if dt == np.uint32 else 2**64 - 5  # the running sum wraps inside tile 0's partial
    out = fin.scan(a, inplace)
    kr.check_scan(out, a, FILL)
    assert int(a.astype(object).sum()) >= 2**(32 if dt == np.uint32 else 64)


def test_scan_u32_total_passes_2_32(fin):
    T = fin.scan_tile
    n = 2 * T + 9
    a = np.full(n, 2**20, dtype=np.uint32)  # sum = (2 T + 9) 2^20 > 2^32 for T >= 2048
    assert n * 2**20 > 2**32
    for inplace in (False, True):
        out = fin.scan(a, inplace)
        kr.check_scan(out, a, FILL)
        assert int(out[n - 1]) == ((n - 1) * 2**20) % 2**32


# ---------------------------------------------------------------------------
# key_bits
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("W", WS)
def test_key_bits(fin, W):
    rng = np.random.default_rng(40 + W)
    for n in (1, 63, 65, 256 * 5 + 1):
        keys = rng.integers(0, 2**64, size=(W, n), dtype=U64)
        keys[W - 1] = U64(0x0123456789abcdef)          # one word constant across all keys
        keys[0] |= U64(1 << 17)                          # one bit constant 1
        keys[0] &= ~U64(1 << 40)                         # one bit constant 0
        if n > 1:
            keys[0, 0] |= U64(1 << 63)                   # bit 63 varying
            keys[0, 1:] &= ~U64(1 << 63)
        got = fin.key_bits(keys, n + 3)
        want = kr.key_bits_ref(keys)
        kr.check_equal("key_bits", got, want)
        vary = got[:W] ^ got[W:]
        if W > 1:
            assert vary[W - 1] == 0
        assert not (int(vary[0]) >> 17) & 1 and not (int(vary[0]) >> 40) & 1
        if n > 1:
            assert (int(vary[0]) >> 63) & 1
        # the padding behind the keys (a pattern, not the keys) must not be read
        kr.check_equal("key_bits, stride n", fin.key_bits(keys, n), want)


# ---------------------------------------------------------------------------
# sort pass
# ---------------------------------------------------------------------------

PATTERNS = ("uniform", "all0", "all255", "pair", "grouped", "reverse")


def sort_walk(n, T, grid):
    """Tiles of every block of sort_upsweep / sort_downsweep."""
    tiles = -(-n // T)
    per = -(-tiles // grid)
    out = []
    for b in range(grid):
        lo, hi = min(n, b * per * T), min(n, (b + 1) * per * T)
        out.append(-(-(hi - lo) // T))
    assert sum(out) == tiles
    return out


def make_sort_input(W, n, pattern, word, shift, with_vals, seed):
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 2**64, size=(W, n), dtype=U64)
    if pattern == "uniform":
        d = None
    elif pattern.startswith("all"):
        d = np.full(n, int(pattern[3:]), dtype=U64)
    elif pattern == "pair":
        d = U64(100) + rng.integers(0, 2, size=n, dtype=U64)
    else:
        d = np.sort(rng.integers(0, 256, size=n, dtype=U64))
        if pattern == "reverse":
            d = d[::-1].copy()
    if d is not None:
        keys[word] = (keys[word] & ~(U64(255) << U64(shift))) | (d << U64(shift))
    # values = input index: with them the check sees the order among equal keys too
    vals = np.arange(n, dtype=U32) if with_vals else None
    return keys, vals


@pytest.mark.parametrize("with_vals", (False, True), ids=("keys", "vals"))
@pytest.mark.parametrize("W", WS)
def test_sort_pass_up_to_a_tile(fin, W, with_vals):
    """n in {1, one wave's share - 1, T - 1, T, T + 1}, every digit pattern,
    every word of the key and shifts 0 / 24 / 56 in rotation, default grid."""
    T = fin.sort_tile(W)
    items = T // 256
    k = 0
    for n in (1, 64 * items - 1, T - 1, T, T + 1):
        grid = fin.L.kcs_sort_grid(n)
        assert sum(sort_walk(n, T, grid)) == (2 if n == T + 1 else 1)
        for pattern in PATTERNS:
            word, shift = k % W, (0, 24, 56)[(k // W) % 3]
            k += 1
            keys, vals = make_sort_input(W, n, pattern, word, shift, with_vals, 500 + k)
            ko, vo = fin.sort_pass(keys, vals, word, shift, 0)
            kr.check_sort_pass(ko, vo, keys, vals, word, shift, FILL)


@pytest.mark.parametrize("with_vals", (False, True), ids=("keys", "vals"))
@pytest.mark.parametrize("W", WS)
def test_sort_pass_every_word_and_shift(fin, W, with_vals):
    T = fin.sort_tile(W)
    n = T + T // 2 + 3
    for word in range(W):
        for shift in (0, 24, 56):
            keys, vals = make_sort_input(W, n, "pair" if shift == 24 else "uniform", word, shift, with_vals,
                                         600 + 8 * word + shift)
            # the other words' bytes at this shift must not matter: give them a digit that would sort differently
            mirrored = U64(255) - ((keys[word] >> U64(shift)) & U64(255))
            for j in range(W):
                if j != word:
                    keys[j] = (keys[j] & ~(U64(255) << U64(shift))) | (mirrored << U64(shift))
            ko, vo = fin.sort_pass(keys, vals, word, shift, 0)
            kr.check_sort_pass(ko, vo, keys, vals, word, shift, FILL)


@pytest.mark.parametrize("with_vals", (False, True), ids=("keys", "vals"))
@pytest.mark.parametrize("W", WS)
def test_sort_pass_blocks_with_several_tiles_and_with_none(fin, W, with_vals):
    """5 T + 17 records (6 tiles, the last of 17 records) on grids 1, 2, 3 and
    8, and on the default grid."""
    T = fin.sort_tile(W)
    n = 5 * T + 17
    k = 0
    for grid, want in ((1, [6]), (2, [3, 3]), (3, [2, 2, 2]), (8, [1] * 6 + [0, 0]), (0, None)):
        g = grid or fin.L.kcs_sort_grid(n)
        walk = sort_walk(n, T, g)
        if want is not None:
            assert walk == want
        else:
            assert len(walk) == g and max(walk) >= 1
        for pattern in PATTERNS:
            word, shift = k % W, (56, 0, 24)[k % 3]
            k += 1
            keys, vals = make_sort_input(W, n, pattern, word, shift, with_vals, 700 + k)
            ko, vo = fin.sort_pass(keys, vals, word, shift, grid)
            kr.check_sort_pass(ko, vo, keys, vals, word, shift, FILL)


@pytest.mark.parametrize("W", WS)
def test_sort_two_passes_are_a_stable_sort_by_16_bits(fin, W):
    T = fin.sort_tile(W)
    n = 2 * T + 11
    rng = np.random.default_rng(80 + W)
    keys = rng.integers(0, 2**64, size=(W, n), dtype=U64)
    word = W - 1
    keys[word] &= ~U64(0xf0f0 << 24)  # 256 values of the 16 bits, each many times
    vals = np.arange(n, dtype=U32)
    k1, v1 = fin.sort_pass(keys, vals, word, 24, 0)
    k2, v2 = fin.sort_pass(np.ascontiguousarray(k1[:, :n]), v1[:n].copy(), word, 32, 3)
    p = np.argsort(((keys[word] >> U64(24)) & U64(0xffff)).astype(np.int64), kind="stable")
    kr.check_soa("two passes", k2, v2, keys[:, p], vals[p], FILL)


@pytest.mark.parametrize("W", WS)
def test_sort_full_lsd_equals_the_key_sort(fin, W):
    """3 T + 1 records sorted by every byte that key_bits reports as varying
    (last word first, as the library's sort_records walks them): the
    lexicographic key sort, equal keys in input order, values with their keys."""
    T = fin.sort_tile(W)
    n = 3 * T + 1
    rng = np.random.default_rng(90 + W)
    keys = rng.integers(0, 2**64, size=(W, n), dtype=U64)
    keys[0] &= U64(0x00000000ffff0003)            # three bytes vary in word 0
    if W > 1:
        keys[W - 1] &= U64(0xff000000000000ff)    # two in the last word
    for j in range(1, W - 1):
        keys[j] = U64(0x1111111111111111) * U64(j)  # the middle words are constant
    keys[:, n // 2:n // 2 + 500] = keys[:, :500]   # 500 keys twice
    vals = np.arange(n, dtype=U32)
    bits = fin.key_bits(keys, n + 3)
    kr.check_equal("key_bits", bits, kr.key_bits_ref(keys))
    vary = bits[:W] ^ bits[W:]
    passes = [(w, s) for w in range(W - 1, -1, -1) for s in range(0, 64, 8) if (int(vary[w]) >> s) & 255]
    assert len(passes) == (5 if W > 1 else 3)
    k, v = keys, vals
    for i, (w, s) in enumerate(passes):
        ko, vo = fin.sort_pass(np.ascontiguousarray(k), np.ascontiguousarray(v), w, s, (0, 2, 5)[i % 3])
        kr.check_fill(ko[:, n:], FILL)
        k, v = ko[:, :n], vo[:n]
    p = lexorder(keys)
    kr.check_equal("full sort keys", np.ascontiguousarray(k), keys[:, p])
    kr.check_equal("full sort values", np.ascontiguousarray(v), vals[p])


# ---------------------------------------------------------------------------
# run-length chain, reduce chain, pack, unpack
# ---------------------------------------------------------------------------

def check_rle_chain(r, keys):
    n = keys.shape[1]
    flags, pos, head, dk, lens = kr.rle_ref(keys)
    kr.check_equal("flags", r["flags"], flags)
    kr.check_equal("pos", r["pos"], pos)
    m = head.size
    assert r["m"] == m
    kr.check_equal("head", r["head"][:m], head)
    kr.check_fill(r["head"][m:], FILL)
    kr.check_soa("rle", r["keys"], r["cnts"], dk, lens, FILL)
    kr.check_packed("rle", r["packed"], dk, lens, FILL)
    return m


def check_reduce_chain(r, keys, cnts):
    flags, pos, head, _, _ = kr.rle_ref(keys)
    dk, sums = kr.segsum_ref(keys, cnts)
    kr.check_equal("flags", r["flags"], flags)
    kr.check_equal("pos", r["pos"], pos)
    assert r["m"] == head.size
    kr.check_soa("reduce", r["keys"], r["cnts"], dk, sums, FILL)
    kr.check_packed("reduce", r["packed"], dk, sums, FILL)
    return head.size


def runs_of(W, lens, seed, mode="rand"):
    """Sorted keys with run i repeated lens[i] times. mode "last": the keys
    differ only in word W - 1."""
    rng = np.random.default_rng(seed)
    m = len(lens)
    d = rng.integers(0, 2**64, size=(W, m), dtype=U64)
    if mode == "last":
        d[:W - 1] = U64(0xfedcba9876543210)
    d = d[:, lexorder(d)]
    assert m < 2 or np.all(np.any(d[:, 1:] != d[:, :-1], axis=0))
    return np.repeat(d, lens, axis=1)


def chain_cases(W):
    rng = np.random.default_rng(100 + W)
    yield "distinct", runs_of(W, np.ones(1500, dtype=np.int64), 1)
    yield "all equal", runs_of(W, [1500], 2)
    yield "runs 1..300", runs_of(W, rng.permutation(np.arange(1, 301))[:40], 3)
    yield "last word only", runs_of(W, rng.integers(1, 9, size=400), 4, mode="last")
    yield "n = 1", runs_of(W, [1], 5)
    yield "two records, equal", runs_of(W, [2], 6)
    yield "257, a run across 256", runs_of(W, [250, 7], 7)


@pytest.mark.parametrize("W", WS)
def test_rle_chain(fin, W):
    for name, keys in chain_cases(W):
        r = fin.chain(keys)
        m = check_rle_chain(r, keys)
        if name == "distinct":
            assert m == keys.shape[1]
        if name in ("all equal", "n = 1", "two records, equal"):
            assert m == 1
        if name == "257, a run across 256":
            assert r["flags"][256] == 0 and r["flags"][250] == 1


@pytest.mark.parametrize("W", WS)
def test_reduce_chain(fin, W):
    rng = np.random.default_rng(110 + W)
    for name, keys in chain_cases(W):
        n = keys.shape[1]
        cnts = rng.integers(0, 2**32, size=n, dtype=U32)  # sums of two or more wrap half of the time
        r = fin.chain(keys, cnts)
        m = check_reduce_chain(r, keys, cnts)
        if name == "all equal":
            assert m == 1 and int(cnts.astype(np.uint64).sum()) >= 2**32
        # every count 1: the segmented sum is the run-length chain's answer
        r1 = fin.chain(keys, np.ones(n, dtype=U32))
        kr.check_soa("reduce of ones", r1["keys"], r1["cnts"], *kr.rle_ref(keys)[3:], FILL)


def test_chains_past_the_grid_cap(fin):
    """n = elem_grid_cap * 256 + 3 at W = 1: the element-wise kernels take a
    second grid-stride round for the last 3 records, and a run crosses that
    boundary (and many multiples of 256)."""
    n = fin.elem_cap * 256 + 3
    rng = np.random.default_rng(120)
    lens = rng.integers(1, 301, size=n // 100)
    lens = lens[:np.searchsorted(np.cumsum(lens), n - 200)]
    lens = np.append(lens, n - lens.sum())  # the last run crosses the boundary
    assert lens[-1] > 3 and lens.sum() == n
    keys = runs_of(1, lens, 8)
    flags = kr.rle_ref(keys)[0]
    assert flags[fin.elem_cap * 256] == 0 and not flags[-3:].any()
    assert np.any(flags[256::256] == 0) and np.any(flags[256::256] == 1)
    check_rle_chain(fin.chain(keys), keys)
    cnts = rng.integers(0, 2**32, size=n, dtype=U32)
    check_reduce_chain(fin.chain(keys, cnts), keys, cnts)


@pytest.mark.parametrize("W", WS)
def test_pack_and_unpack(fin, W):
    rng = np.random.default_rng(130 + W)
    for n in (1, 255, 1000):
        keys = rng.integers(0, 2**64, size=(W, n), dtype=U64)
        cnts = rng.integers(0, 2**32, size=n, dtype=U32)
        pk = fin.pack(keys, cnts)
        kr.check_packed("pack", pk, keys, cnts, FILL)
        ko, co = fin.unpack(kr.pack_records(keys, cnts), W)
        kr.check_soa("unpack", ko, co, keys, cnts, FILL)


# ---------------------------------------------------------------------------
# compact
# ---------------------------------------------------------------------------

def compact_walk(cap, grid):
    """(slots per block, rounds of 256 a block with a full share walks, blocks that own slots)."""
    per = -(-(-(-cap // grid)) // 256) * 256
    return per, per // 256, -(-cap // per)


def make_compact_table(W, cap, density, seed):
    rng = np.random.default_rng(seed)
    keys = rng.integers(1, 2**64, size=(W, cap), dtype=U64)  # garbage in the unoccupied slots' key words (W >= 2)
    if density == 0:
        state = rng.integers(0, 2, size=cap)
    elif density == 100:
        state = np.full(cap, 2)
    else:
        state = rng.integers(0, 4, size=cap)
        state[state == 3] = 2  # half occupied, a quarter each empty and claimed-but-unfinished
    if W == 1:
        keys[0, state != 2] = 0
    cnts = rng.integers(1, 2**32, size=cap, dtype=U32)
    return kr.make_table(W, keys, cnts, state), int((state == 2).sum()), state


@pytest.mark.parametrize("W", WS)
def test_compact_small_tables(fin, W):
    for cap in (1, 255, 257, 1000):
        per, rounds, owners = compact_walk(cap, fin.compact_grid)
        assert (per, rounds, owners) == (256, 1, -(-cap // 256))
        for density in (0, 100, 50):
            table, occ, state = make_compact_table(W, cap, density, 140 + W + cap)
            if W >= 2 and density == 50 and cap >= 255:
                assert (state == 0).any() and (state == 1).any() and (state == 2).any()
            assert occ == {0: 0, 100: cap}.get(density, occ) and (cap < 255 or (0 < occ < cap) == (density == 50))
            for k0 in (False, True):
                ko, co, cur = fin.compact(W, table, occ + 1, k0, 2**32 + 41)
                m = kr.check_compact(ko, co, cur, W, table, occ + 1, k0, 2**32 + 41, FILL)
                assert m == occ + k0 and cur == occ + k0
            if occ > 5:
                # a sink shorter than the table's records: the first out_cap, nothing behind them
                ko, co, cur = fin.compact(W, table, occ - 5, False, 0)
                assert kr.check_compact(ko, co, cur, W, table, occ - 5, False, 0, FILL) == occ - 5
                assert cur == occ


@pytest.mark.parametrize("W", (1, 2))
def test_compact_blocks_walk_several_rounds(fin, W):
    cap = fin.compact_grid * 256 * 2 + 77
    per, rounds, owners = compact_walk(cap, fin.compact_grid)
    assert rounds >= 2 and owners <= fin.compact_grid and cap % per != 0
    table, occ, _ = make_compact_table(W, cap, 50, 150 + W)
    ko, co, cur = fin.compact(W, table, occ + 1, True, 9)
    assert kr.check_compact(ko, co, cur, W, table, occ + 1, True, 9, FILL) == occ + 1


# ---------------------------------------------------------------------------
# merge, SoA and packed
# ---------------------------------------------------------------------------

def merge_walk(n, T, grid_cap):
    """(tiles, workgroups, tiles of every workgroup) of merge_tile_k / merge_tile_packed_k."""
    nt = -(-n // T)
    g = min(nt, grid_cap)
    per = [len(range(b, nt, g)) for b in range(g)]
    assert sum(per) == nt
    return nt, g, per


def unique_pool(W, m, seed, mode="rand"):
    """m distinct sorted keys. rand: every word random (bit 63 of word 0 set
    in half of them); last: they differ only in word W - 1; hi32 / lo32: the
    deciding word differs only in its upper / lower 32 bits (the other half,
    and bit 63 of the lo32 keys, constant); few: word 0 takes 4 values, so the
    later words decide inside long stretches."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 2**64, size=(W, m), dtype=U64)
    if mode == "last":
        k[:W - 1] = U64(0x8000000000000001)
    elif mode == "hi32":
        k[:W - 1] = U64(5)
        k[W - 1] = (k[W - 1] & U64(0xffffffff00000000)) | U64(0x00000000deadbeef)
    elif mode == "lo32":
        k[:W - 1] = U64(0xffffffffffffffff)
        k[W - 1] = (k[W - 1] & U64(0x00000000ffffffff)) | U64(0x8000000100000000)
    elif mode == "few":
        k[0] = (k[0] & U64(3)) << U64(62)
        if W == 1:
            k[0] |= rng.integers(0, 2**62, size=m, dtype=U64)
    k = k[:, lexorder(k)]
    assert m < 2 or np.all(np.any(k[:, 1:] != k[:, :-1], axis=0)), "pool keys collide"
    return k


def split_pool(pool, na, seed, shared=()):
    """The pool's keys dealt to A (na of the unshared ones) and B at random;
    the keys at the indices `shared` go to both. Returns (ka, ca, kb, cb)."""
    m = pool.shape[1]
    rng = np.random.default_rng(seed)
    shared = np.asarray(shared, dtype=np.int64)
    rest = np.setdiff1d(np.arange(m), shared)
    in_a = np.zeros(m, dtype=bool)
    in_a[rng.permutation(rest)[:na]] = True
    in_b = ~in_a
    in_a[shared] = True
    in_b[shared] = True
    ka, kb = pool[:, in_a], pool[:, in_b]
    return ka, np.arange(ka.shape[1], dtype=U32), kb, np.arange(kb.shape[1], dtype=U32) + B_BASE


def counts_for(ka, kb):
    return np.arange(ka.shape[1], dtype=U32), np.arange(kb.shape[1], dtype=U32) + B_BASE


def run_merge(fin, ka, ca, kb, cb, *, grid_cap=8192, forms=("soa", "packed"), a_off=None, strides=None, skips=(0, 0, 0),
              want_dup=None):
    """Both forms of the merge over the same runs, checked against the stable
    merge; returns the (tiles, workgroups) both must agree on."""
    W = ka.shape[0]
    n = ka.shape[1] + kb.shape[1]
    T = fin.merge_tile(W)
    nt, g, _ = merge_walk(n, T, grid_cap)
    if "soa" in forms:
        ko, co, off, nt1, g1 = fin.merge(ka, ca, kb, cb, grid_cap=grid_cap, a_off=a_off, strides=strides)
        assert (nt1, g1) == (nt, g)
        kr.check_merge_soa(ko, co, ka, ca, kb, cb, FILL, off=off)
    if "packed" in forms:
        a_skip, b_skip, out_skip = skips
        out, dup, al, nt2, g2 = fin.merge_packed(W, kr.pack_records(ka, ca), kr.pack_records(kb, cb), a_skip=a_skip,
                                                 b_skip=b_skip, out_skip=out_skip, grid_cap=grid_cap)
        assert (nt2, g2) == (nt, g)
        # an aligned run takes 16-byte stores (with a u32 tail when n RW % 4 != 0); one
        # that starts a record (8 W + 4 bytes) into the allocation takes the u32 path
        assert al == (out_skip * (8 * W + 4)) % 16 and (al == 0) == (out_skip % 4 == 0)
        kr.check_merge_packed(out, dup, ka, ca, kb, cb, FILL, skip=out_skip)
        if want_dup is not None:
            assert dup == want_dup
    return nt, g


def merge_sizes(W, T):
    I = T // 256
    return (1, I - 1, I, I + 1, T - 1, T, T + 1, 3 * T + 5)


@pytest.mark.parametrize("W", WS)
def test_merge_sizes_random_interleave(fin, W):
    """Disjoint key sets dealt at random: every size, aligned and unaligned
    packed output, dup = 0 everywhere."""
    T = fin.merge_tile(W)
    seen_tail = set()
    for i, n in enumerate(merge_sizes(W, T)):
        for out_skip in (0, 1):
            pool = unique_pool(W, n, 200 + i, mode=("rand", "few")[i % 2])
            ka, ca, kb, cb = split_pool(pool, n // 2, 300 + i + out_skip)
            nt, g = run_merge(fin, ka, ca, kb, cb, skips=(i % 2, (i + 1) % 2, out_skip), want_dup=0)
            assert nt == -(-n // T) == g
            seen_tail.add((out_skip, (n * (2 * W + 1)) % 4 != 0))
    assert seen_tail == {(0, False), (0, True), (1, False), (1, True)}


@pytest.mark.parametrize("W", WS)
def test_merge_one_side_empty_or_apart(fin, W):
    T = fin.merge_tile(W)
    pool = unique_pool(W, 2 * T + 9, 210 + W)
    n = pool.shape[1]
    empty = pool[:, :0]
    for ka, kb in ((empty, pool), (pool, empty),                       # na = 0, nb = 0
                   (pool[:, :T + 5], pool[:, T + 5:]),                 # all of A below all of B
                   (pool[:, T + 5:], pool[:, :T + 5]),                 # all of A above all of B
                   (pool[:, :T], pool[:, T:]), (pool[:, T:], pool[:, :T])):  # ... with the change of run on a tile border
        ca, cb = counts_for(ka, kb)
        nt, _ = run_merge(fin, ka, ca, kb, cb, want_dup=0)
        assert nt == 3
        # tiles that take from one run only (la = 0 or lb = 0), splits at the ends of the search range
        src = kr.merge_ref(ka, ca, kb, cb)[2]
        from_a = src < ka.shape[1]
        assert from_a[:T].all() or not from_a[:T].any()


@pytest.mark.parametrize("W", WS)
def test_merge_long_run_with_a_single_record(fin, W):
    T = fin.merge_tile(W)
    pool = unique_pool(W, 3 * T + 1, 220 + W, mode="few")
    for where in (0, T + T // 3, 3 * T):  # B's key below, inside and above A
        ka = np.delete(pool, where, axis=1)
        kb = pool[:, where:where + 1]
        ca, cb = counts_for(ka, kb)
        nt, _ = run_merge(fin, ka, ca, kb, cb, want_dup=0)
        assert nt == 4 and ka.shape[1] == 3 * T
        assert int(np.flatnonzero(kr.merge_ref(ka, ca, kb, cb)[1] == B_BASE)[0]) == where


@pytest.mark.parametrize("W", WS)
def test_merge_ties_keep_a_first(fin, W):
    """Every key equal (T + 7 and T + 9 records), and a run of 40 equal records
    from each side laid across a tile border at three offsets: all of A's
    copies, in their order, then all of B's. Only the counts can tell."""
    T = fin.merge_tile(W)
    one = unique_pool(W, 1, 230 + W)
    ka, kb = np.repeat(one, T + 7, axis=1), np.repeat(one, T + 9, axis=1)
    ca, cb = counts_for(ka, kb)
    nt, _ = run_merge(fin, ka, ca, kb, cb, want_dup=1)
    assert nt == 3
    wc = kr.merge_ref(ka, ca, kb, cb)[1]
    assert np.array_equal(wc, np.concatenate([ca, cb]))
    for below in (T - 40, T - 60, T - 20):
        pool = unique_pool(W, 2 * T, 240 + W + below, mode="few")
        x = pool[:, below:below + 1]
        lo, hi = pool[:, :below], pool[:, below + 1:]
        la, ha = lo[:, ::2], hi[:, 1::2]
        lb, hb = lo[:, 1::2], hi[:, ::2]
        ka = np.concatenate([la, np.repeat(x, 40, axis=1), ha], axis=1)
        kb = np.concatenate([lb, np.repeat(x, 40, axis=1), hb], axis=1)
        ca, cb = counts_for(ka, kb)
        wk, wc, src = kr.merge_ref(ka, ca, kb, cb)
        eq = np.flatnonzero(np.all(wk == x, axis=0))
        assert eq[0] == below and eq.size == 80 and eq[0] < T <= eq[-1]  # the equal records straddle output T
        assert np.all(wc[eq[:40]] < B_BASE) and np.all(wc[eq[40:]] >= B_BASE)
        run_merge(fin, ka, ca, kb, cb, want_dup=1)


@pytest.mark.parametrize("mode", ("last", "hi32", "lo32", "rand"))
@pytest.mark.parametrize("W", WS)
def test_merge_comparison_rules(fin, W, mode):
    """Keys that differ only in word W - 1, only in the upper or only in the
    lower 32 bits of a word, and words with bit 63 set against words without."""
    T = fin.merge_tile(W)
    pool = unique_pool(W, T + T // 2 + 3, 250 + W, mode=mode)
    if mode == "rand":
        top = pool[0] >> U64(63)
        assert top.min() == 0 and top.max() == 1
    if mode in ("last", "hi32", "lo32") and W > 1:
        assert np.all(pool[:W - 1] == pool[:W - 1, :1])
    ka, ca, kb, cb = split_pool(pool, pool.shape[1] // 3, 260 + W)
    run_merge(fin, ka, ca, kb, cb, want_dup=0)


@pytest.mark.parametrize("grid_cap", (1, 3, 4))
@pytest.mark.parametrize("W", WS)
def test_merge_workgroups_walk_several_tiles(fin, W, grid_cap):
    """10 tiles (the last one short) on 1, 3 and 4 workgroups. In the packed
    form this is the register-prefetch pipeline, with workgroups whose last
    fetch is past the last tile (every workgroup fetches t + grid once more
    than it merges) and, on 3 and 4 workgroups, uneven tile counts."""
    T = fin.merge_tile(W)
    n = 9 * T + T // 3
    nt, g, per = merge_walk(n, T, grid_cap)
    assert nt == 10 and g == grid_cap
    assert per == {1: [10], 3: [4, 3, 3], 4: [3, 3, 2, 2]}[grid_cap]
    pool = unique_pool(W, n - 6, 270 + W + grid_cap, mode="few")
    shared = [3 * T - 1, 5 * T + 7, 8 * T + 100]  # three keys in both runs
    ka, ca, kb, cb = split_pool(pool, n // 2, 280 + W, shared=shared)
    ka = np.concatenate([ka, ka[:, -3:]], axis=1)  # and A's last three keys twice
    ka = ka[:, lexorder(ka)]
    ca, cb = counts_for(ka, kb)
    assert ka.shape[1] + kb.shape[1] == n
    for out_skip in (0, 1):
        assert run_merge(fin, ka, ca, kb, cb, grid_cap=grid_cap, skips=(1, 0, out_skip), want_dup=1) == (10, grid_cap)
    ka, ca, kb, cb = split_pool(unique_pool(W, n, 290 + W), n // 3, 291)
    assert run_merge(fin, ka, ca, kb, cb, grid_cap=grid_cap, want_dup=0) == (10, grid_cap)


@pytest.mark.parametrize("W", WS)
def test_merge_soa_offsets_and_strides(fin, W):
    """A and B as adjacent ranges of one buffer at a_off > 0 (merge_runs_list's
    layout), and three different strides; the padding of the output and the
    records before a_off keep the sentinel."""
    T = fin.merge_tile(W)
    n = 2 * T + 13
    pool = unique_pool(W, n, 300 + W, mode="few")
    ka, ca, kb, cb = split_pool(pool, T + 1, 301 + W, shared=[5, T, n - 1])
    for a_off in (1, 77, T + 3):
        run_merge(fin, ka, ca, kb, cb, forms=("soa",), a_off=a_off)
    na, nb = ka.shape[1], kb.shape[1]
    for strides in ((na, nb, na + nb), (na + 3, nb + 1001, na + nb + 64), (na + 4099, nb + 3, na + nb + 3)):
        assert len(set(strides)) == 3
        run_merge(fin, ka, ca, kb, cb, forms=("soa",), strides=strides)


DUP_PLACES = ("none", "mid tile", "tile border", "last tile border", "first and last two")


@pytest.mark.parametrize("place", DUP_PLACES)
@pytest.mark.parametrize("W", WS)
def test_merge_packed_dup_flag(fin, W, place):
    """Exactly one key in both runs (two for the first-and-last case), placed
    by its output index: in the middle of a tile (found among sout's
    neighbours), or with A's copy the last output of a tile and B's the first
    of the next (found only by the tile's first thread re-reading A[i0 - 1])."""
    T = fin.merge_tile(W)
    m = 3 * T + 4
    shared = {"none": [], "mid tile": [T + T // 2], "tile border": [T - 1], "last tile border": [3 * T - 1],
              "first and last two": [0, m - 1]}[place]
    pool = unique_pool(W, m, 310 + W, mode="few")
    ka, ca, kb, cb = split_pool(pool, m // 2, 311 + W, shared=shared)
    wk, wc, src = kr.merge_ref(ka, ca, kb, cb)
    pairs = np.flatnonzero(np.all(wk[:, 1:] == wk[:, :-1], axis=0))
    assert pairs.size == len(shared)
    if place == "mid tile":
        assert pairs[0] % T not in (0, T - 1)
    if place == "tile border":
        assert pairs[0] == T - 1 and wc[T - 1] < B_BASE <= wc[T]  # A's copy is output T - 1, B's output T
    if place == "last tile border":
        nt = -(-wk.shape[1] // T)
        assert pairs[0] == (nt - 1) * T - 1 and wc[pairs[0]] < B_BASE <= wc[pairs[0] + 1]
    if place == "first and last two":
        assert pairs.tolist() == [0, wk.shape[1] - 2]
    for out_skip in (0, 1):
        run_merge(fin, ka, ca, kb, cb, forms=("packed",), skips=(0, 1, out_skip), want_dup=int(bool(shared)))
    if place in ("tile border", "last tile border"):
        # the runs exchanged: the pair stays where it is, and the copy re-read at
        # the tile's start now comes from what was B
        cb2, ca2 = counts_for(kb, ka)
        wk2, wc2, _ = kr.merge_ref(kb, cb2, ka, ca2)
        assert np.array_equal(wk2, wk) and wc2[pairs[0]] < B_BASE <= wc2[pairs[0] + 1]
        run_merge(fin, kb, cb2, ka, ca2, forms=("packed",), want_dup=1)


@pytest.mark.parametrize("reps", (2, 4))
@pytest.mark.parametrize("W", WS)
def test_merge_packed_runs_with_repeated_keys(fin, W, reps):
    """Runs as levels 2 and 3 of a multi-run merge produce them: a key two,
    then four times inside each run. The output is the stable merge, dup = 1."""
    T = fin.merge_tile(W)
    pool = unique_pool(W, 2 * T, 320 + W, mode="few")
    x = [7, T - 3, T + T // 2]  # one of them laid across the first tile border
    lens_a = np.ones(pool.shape[1], dtype=np.int64)
    lens_a[x] = reps
    ka = np.repeat(pool, lens_a, axis=1)[:, ::2]
    ka = np.concatenate([ka, np.repeat(pool[:, x], reps, axis=1)], axis=1)
    ka = ka[:, lexorder(ka)]
    kb = np.repeat(pool, lens_a, axis=1)[:, 1::2]
    kb = np.concatenate([kb, np.repeat(pool[:, x[1:2]], reps, axis=1)], axis=1)
    kb = kb[:, lexorder(kb)]
    ca, cb = counts_for(ka, kb)
    assert kr.dup_ref(ka) == 1 and kr.dup_ref(kb) == 1
    for out_skip in (0, 1):
        run_merge(fin, ka, ca, kb, cb, skips=(0, 0, out_skip), want_dup=1)
    # repeats inside one run only, no key in both: dup = 1 all the same
    ka2 = np.repeat(pool[:, :T], np.where(np.arange(T) == T // 2, reps, 1), axis=1)
    kb2 = pool[:, T:]
    ca2, cb2 = counts_for(ka2, kb2)
    run_merge(fin, ka2, ca2, kb2, cb2, forms=("packed",), want_dup=1)


@pytest.mark.parametrize("W", WS)
def test_merge_levels_then_reduce_equal_the_sum_by_key(fin, W):
    """8 sorted deduplicated runs, each key in 1..8 of them, merged pairwise
    through three levels of kcs_merge_packed (as merge_runs_packed does) and
    summed by kcs_reduce_chain: numpy's sum by key."""
    T = fin.merge_tile(W)
    m = T + T // 2
    pool = unique_pool(W, m, 330 + W, mode="few")
    rng = np.random.default_rng(331 + W)
    member = rng.random((8, m)) < (rng.integers(1, 9, size=m) / 8.0)
    member[rng.integers(0, 8, size=m), np.arange(m)] = True  # every key in at least one run
    runs, total = [], np.zeros(m, dtype=np.uint64)
    for r in range(8):
        idx = np.flatnonzero(member[r])
        c = rng.integers(1, 2**32, size=idx.size, dtype=U32)
        total[idx] += c
        runs.append(kr.pack_records(pool[:, idx], c))
    assert member.sum(axis=0).max() >= 5 and member.sum(axis=0).min() == 1
    level = 0
    while len(runs) > 1:
        nxt = []
        for r in range(0, len(runs), 2):
            ka, ca = kr.unpack_records(runs[r], W)
            kb, cb = kr.unpack_records(runs[r + 1], W)
            # the second pair of a level goes where merge_runs_packed puts it: behind
            # the first, at a record offset that is not 16-byte aligned
            out_skip = (r // 2) % 2
            out, dup, al, _, _ = fin.merge_packed(W, runs[r], runs[r + 1], out_skip=out_skip)
            kr.check_merge_packed(out, dup, ka, ca, kb, cb, FILL, skip=out_skip)
            nxt.append(out[out_skip:out_skip + ka.shape[1] + kb.shape[1]].copy())
        runs = nxt
        level += 1
    assert level == 3
    keys, cnts = kr.unpack_records(runs[0], W)
    assert keys.shape[1] == member.sum()
    r = fin.chain(keys, cnts)
    assert check_reduce_chain(r, keys, cnts) == m
    kr.check_soa("sum by key", r["keys"], r["cnts"], pool, (total & U64(0xffffffff)).astype(U32), FILL)


# ---------------------------------------------------------------------------
# owner bounds, bucket bounds (AoS), packed segment copy
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("world", (1, 2, 3, 8, 255, 256, 1000))
def test_owner_bounds(fin, world):
    """255 fits the kernel's one block of 256 threads with one bound each, 256
    and 1000 (world + 1 > 256 bounds) take its stride loop."""
    W = 1 + world % 4
    rng = np.random.default_rng(400 + world)
    borders = [-(-(o << 32) // world) for o in range(1, world)]
    tops = np.array(borders + [b - 1 for b in borders] + [0, 2**32 - 1], dtype=np.uint64)
    tops = np.concatenate([tops, rng.integers(0, 2**32, size=300, dtype=np.uint64)])
    keys = rng.integers(0, 2**64, size=(W, tops.size), dtype=U64)
    keys[0] = (tops << U64(32)) | (keys[0] & U64(0xffffffff))
    keys = keys[:, lexorder(keys)]
    if world > 1:
        own = kr.owner_of(keys[0], world)
        o = world // 2
        assert own[np.flatnonzero((keys[0] >> U64(32)) == U64(borders[o - 1]))[0]] == o
        assert own[np.flatnonzero((keys[0] >> U64(32)) == U64(borders[o - 1] - 1))[0]] == o - 1
    cnts = np.arange(keys.shape[1], dtype=U32)
    out = fin.owner_bounds(W, kr.pack_records(keys, cnts), world)
    kr.check_equal("owner bounds", out[:world + 1], kr.owner_bounds_ref(keys[0], world))
    kr.check_fill(out[world + 1:], FILL)
    assert out[0] == 0 and out[world] == keys.shape[1]
    # n = 0, and every record with one owner
    out = fin.owner_bounds(W, np.zeros((0, 8 * W + 4), dtype=np.uint8), world)
    kr.check_equal("owner bounds, n = 0", out[:world + 1], np.zeros(world + 1, dtype=U64))
    o = world - 1
    k1 = keys.copy()
    k1[0] = (U64(-(-(o << 32) // world)) << U64(32)) | (keys[0] & U64(0xffffffff))
    k1 = k1[:, lexorder(k1)]
    assert np.all(kr.owner_of(k1[0], world) == o)
    out = fin.owner_bounds(W, kr.pack_records(k1, cnts), world)
    kr.check_equal("owner bounds, one owner", out[:world + 1], kr.owner_bounds_ref(k1[0], world))
    assert out[o] == 0 and out[world] == k1.shape[1]


@pytest.mark.parametrize("W", WS)
def test_bucket_bounds_aos(fin, W):
    """stride 0: W consecutive words per key, with the 16 bits the library passes."""
    rng = np.random.default_rng(410 + W)
    n = 3000
    keys = rng.integers(0, 2**64, size=(W, n), dtype=U64)
    # buckets 0..99 and 60000.. stay empty
    keys[0] = ((U64(100) + rng.integers(0, 59900, size=n, dtype=U64)) << U64(48)) | (keys[0] & U64(0xffffffffffff))
    keys = keys[:, np.argsort(keys[0], kind="stable")]  # grouped by word 0; the other words in any order
    aos = np.ascontiguousarray(keys.T)
    out = fin.bucket_bounds(W, aos, n, 0, 16)
    want = kr.bucket_bounds_ref(keys[0], 16)
    assert want[100] == 0 and want[60000] == n
    kr.check_equal("bucket bounds", out[:65537], want)
    kr.check_fill(out[65537:], FILL)
    # the SoA form over the same keys agrees
    kr.check_equal("bucket bounds, SoA", fin.bucket_bounds(W, _strided(keys, n + 3), n, n + 3, 16)[:65537], want)
    one = np.ascontiguousarray(keys[:, 1234:1235].T)
    out = fin.bucket_bounds(W, one, 1, 0, 16)
    kr.check_equal("bucket bounds, n = 1", out[:65537], kr.bucket_bounds_ref(keys[0, 1234:1235], 16))


@pytest.mark.parametrize("W", WS)
def test_packed_seg_copy(fin, W):
    """Segments of 0, 1 and 700 records in permuted order, a base, gaps between the targets."""
    rng = np.random.default_rng(420 + W)
    nsrc = 1500
    src = rng.integers(0, 256, size=(nsrc, 8 * W + 4), dtype=np.uint8)
    dstart = np.array([0, 700, 700, 701, 800, 1500], dtype=U64)
    length = np.array([700, 0, 1, 50, 700, 0], dtype=np.int64)
    dlen = (length | (np.array([0, 36, 0, 36, 1, 0]) << 24) | (np.array([1, 0, 0, 1, 0, 0]) << 31)).astype(U32)
    order = np.array([4, 1, 0, 5, 3, 2], dtype=U32)
    out_off = np.array([0, 705, 710, 1420, 1420, 1475], dtype=U64)  # of order[d]; gaps of 5, 10, 5 and 4
    base, ndst = 9, 1500
    for grid in (1, 4, 64):
        dst = fin.seg_copy(W, src, ndst, order, dstart, dlen, out_off, base, grid)
        want = np.full_like(dst, FILL)
        for d, o in enumerate(order):
            at = base + int(out_off[d])
            want[at:at + length[o]] = src[int(dstart[o]):int(dstart[o]) + length[o]]
        kr.check_equal("packed_seg_copy", dst, want)
        assert np.all(dst[:base] == FILL) and np.all(dst[base + 700:base + 705] == FILL) and np.all(dst[1490:] == FILL)
