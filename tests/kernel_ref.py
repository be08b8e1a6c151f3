"""Host references and comparison helpers of the kernel-level tests
(test_gpu_kernels.py, in the second half test_gpu_finish_kernels.py, in the
last part test_gpu_skm_kernels.py), plain numpy on integers: every comparison
is exact.
tests/test_kernel_ref.py checks these helpers themselves on the CPU.

Items of the grouping passes are rows (all NW words, payload); records of the
segment sort are (W key words, count). Word arrays are SoA, shape (NW, n).

What the kernels promise, which is what the references state:

* LSD pass: the output is the concatenation over digit d = 0..255, then over
  region r ascending, of the items of region r with digit d. The order inside
  one (d, r) block is unspecified (ranks come from LDS atomics), so both sides
  are canonicalised by sorting each block's rows. bases[d] = exclusive count.
* MSD-regional pass: the same with region outer and digit inner;
  sub[r * 256 + d] are the block starts, sub[last] = n.
* Segment sort: each segment's output range holds its records sorted by the
  full key (word 0 most significant), counts with their keys; among equal keys
  the order of the counts is unspecified. Everything else keeps the sentinel.
"""
import numpy as np

U64 = np.uint64


def as_rows(words, pay=None):
    """(NW, n) words (+ payload) -> (n, NW [+ 1]) u64 rows."""
    cols = [np.asarray(w, dtype=U64) for w in words]
    if pay is not None:
        cols.append(np.asarray(pay).astype(U64))
    return np.stack(cols, axis=1)


def digit_of(w0, shift):
    return ((np.asarray(w0, dtype=U64) >> U64(shift)) & U64(255)).astype(np.int64)


def region_of(rstart, n):
    """Region index of every item for bounds rstart[0..nreg] (empty regions allowed)."""
    rstart = np.asarray(rstart, dtype=np.int64)
    assert rstart[0] == 0 and rstart[-1] == n and np.all(np.diff(rstart) >= 0)
    return np.searchsorted(rstart[1:], np.arange(n, dtype=np.int64), side="right")


def rp_ref(dig, rstart, regional):
    """Reference of one grouping pass over items with digits dig and regions
    rstart: (perm, bounds). perm lists the input indices in output order
    (stable inside a block); bounds[b] is the start of block b, with
    b = d * nreg + r for the LSD pass and r * 256 + d for the regional one
    (nreg * 256 + 1 entries, the last one n)."""
    dig = np.asarray(dig, dtype=np.int64)
    n = dig.size
    nreg = len(rstart) - 1
    reg = region_of(rstart, n)
    block = reg * 256 + dig if regional else dig * nreg + reg
    perm = np.argsort(block, kind="stable")
    counts = np.bincount(block, minlength=nreg * 256)
    bounds = np.zeros(nreg * 256 + 1, dtype=np.int64)
    np.cumsum(counts, out=bounds[1:])
    return perm, bounds


def rp_bases(bounds, nreg, regional):
    """What the pass reports: the nreg * 256 + 1 sub-starts (regional) or the
    256 exclusive digit counts (LSD)."""
    return bounds.astype(U64) if regional else bounds[:-1:nreg].astype(U64)


def canon_blocks(rows, bounds):
    """rows with every block [bounds[b], bounds[b + 1]) sorted by the whole row."""
    rows = np.asarray(rows, dtype=U64)
    bounds = np.asarray(bounds, dtype=np.int64)
    assert bounds[0] == 0 and bounds[-1] == rows.shape[0]
    bid = np.repeat(np.arange(bounds.size - 1, dtype=np.int64), np.diff(bounds))
    # word 0 alone orders a block whose word-0 values are distinct (the usual
    # case); only otherwise are the other columns needed as tie-breakers
    o = np.lexsort((rows[:, 0], bid))
    w0, b = rows[o, 0], bid[o]
    if np.any((w0[1:] == w0[:-1]) & (b[1:] == b[:-1])):
        o = np.lexsort([rows[:, c] for c in range(rows.shape[1] - 1, -1, -1)] + [bid])
    return rows[o]


def check_grouped(out_rows, in_rows, dig, rstart, regional):
    """The pass's output rows against the reference, block by block."""
    perm, bounds = rp_ref(dig, rstart, regional)
    out_rows = np.asarray(out_rows, dtype=U64)
    in_rows = np.asarray(in_rows, dtype=U64)
    assert out_rows.shape == in_rows.shape, (out_rows.shape, in_rows.shape)
    got = canon_blocks(out_rows, bounds)
    want = canon_blocks(in_rows[perm], bounds)
    bad = np.flatnonzero(np.any(got != want, axis=1))
    assert bad.size == 0, (
        f"{bad.size} rows differ from the reference after sorting each block; first at canonical index "
        f"{int(bad[0])}: got {got[bad[0]].tolist()}, want {want[bad[0]].tolist()}")
    return bounds


def check_bases(got, bounds, nreg, regional):
    want = rp_bases(bounds, nreg, regional)
    got = np.asarray(got, dtype=U64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} block starts differ; first at {int(bad[0])}: {int(got[bad[0]])} != {int(want[bad[0]])}"


def check_emit(emit, out_w0, eshift):
    """emit[g] == (out_word0[g] >> eshift) & 255 for every g."""
    want = digit_of(out_w0, eshift).astype(np.uint8)
    emit = np.asarray(emit, dtype=np.uint8)
    assert emit.shape == want.shape, (emit.shape, want.shape)
    bad = np.flatnonzero(emit != want)
    assert bad.size == 0, f"{bad.size} emitted bytes wrong; first at {int(bad[0])}: {int(emit[bad[0]])} != {int(want[bad[0]])}"


def check_fill(arr, fill):
    """Every byte of arr still holds the sentinel."""
    b = np.ascontiguousarray(arr).view(np.uint8)
    bad = np.flatnonzero(b != fill)
    assert bad.size == 0, f"{bad.size} sentinel bytes clobbered; first at byte {int(bad[0])}"


# ---- segment sort ----

def _key_order(keys, cnts, seg=None):
    """lexsort by (seg, word 0, ..., word W-1, count)."""
    ks = [np.asarray(cnts, dtype=np.uint32)] + [keys[j] for j in range(keys.shape[0] - 1, -1, -1)]
    if seg is not None:
        ks.append(seg)
    return np.lexsort(ks)


def seg_sort_ref(keys, cnts, segs, nout):
    """segs: (start, length, out_off) of every segment that must come out
    sorted. Returns (want_keys (W, m), want_cnts (m), pos (m), seg (m)): the
    records in output order, their output positions and segment numbers."""
    keys = np.asarray(keys, dtype=U64)
    cnts = np.asarray(cnts, dtype=np.uint32)
    seg = np.asarray(segs, dtype=np.int64).reshape(-1, 3)
    st, ln, off = seg[:, 0], seg[:, 1], seg[:, 2]
    assert np.all(ln >= 0) and np.all(st + ln <= keys.shape[1]) and np.all(off + ln <= nout) and np.all(off >= 0)
    sid = np.repeat(np.arange(ln.size, dtype=np.int64), ln)
    within = np.arange(sid.size, dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
    src = st[sid] + within
    pos = off[sid] + within
    assert np.unique(pos).size == pos.size, "output ranges overlap"
    k, c = keys[:, src], cnts[src]
    o = _key_order(k, c, sid)  # sid ascending = pos ascending segment by segment
    return k[:, o], c[o], pos, sid


def pack_records(keys, cnts):
    """SortedKMerFile bytes: W LE u64 words + LE u32 count per record -> (m, 8 W + 4) u8."""
    keys = np.asarray(keys, dtype="<u8")
    W, m = keys.shape
    out = np.empty((m, 8 * W + 4), dtype=np.uint8)
    for j in range(W):
        out[:, 8 * j:8 * j + 8] = np.ascontiguousarray(keys[j]).view(np.uint8).reshape(m, 8)
    out[:, 8 * W:] = np.ascontiguousarray(np.asarray(cnts, dtype="<u4")).view(np.uint8).reshape(m, 4)
    return out


def check_seg_soa(out_keys, out_cnts, keys, cnts, segs, fill):
    """SoA output (W, nout) + counts against the reference. Keys must stand in
    sorted order exactly; the counts of equal keys are compared as a multiset
    (sorted (key, count) pairs); every word outside the segments' ranges holds
    the sentinel."""
    out_keys = np.asarray(out_keys, dtype=U64)
    out_cnts = np.asarray(out_cnts, dtype=np.uint32)
    nout = out_keys.shape[1]
    wk, wc, pos, sid = seg_sort_ref(keys, cnts, segs, nout)
    gk, gc = out_keys[:, pos], out_cnts[pos]
    bad = np.flatnonzero(np.any(gk != wk, axis=0))
    assert bad.size == 0, (
        f"{bad.size} keys out of place; first at output {int(pos[bad[0]])} (segment {int(sid[bad[0]])}): "
        f"got {gk[:, bad[0]].tolist()}, want {wk[:, bad[0]].tolist()}")
    o = _key_order(gk, gc, sid)
    bad = np.flatnonzero(gc[o] != wc)
    assert bad.size == 0, (
        f"{bad.size} counts not with their keys; first at output {int(pos[bad[0]])} (segment {int(sid[bad[0]])}): "
        f"got {int(gc[o][bad[0]])}, want {int(wc[bad[0]])}")
    rest = np.ones(nout, dtype=bool)
    rest[pos] = False
    check_fill(out_keys[:, rest], fill)
    check_fill(out_cnts[rest], fill)


def check_seg_packed(out_bytes, keys, cnts, segs, fill):
    """Packed output (nout, 8 W + 4) bytes against the reference, byte for
    byte (keys distinct inside a segment); the sentinel everywhere else."""
    keys = np.asarray(keys, dtype=U64)
    rs = 8 * keys.shape[0] + 4
    out = np.asarray(out_bytes, dtype=np.uint8).reshape(-1, rs)
    wk, wc, pos, sid = seg_sort_ref(keys, cnts, segs, out.shape[0])
    if wk.shape[1] > 1:
        same = np.all(wk[:, 1:] == wk[:, :-1], axis=0) & (sid[1:] == sid[:-1])
        assert not same.any(), "packed comparison needs distinct keys inside a segment"
    want = np.full_like(out, fill)
    want[pos] = pack_records(wk, wc)
    bad = np.flatnonzero(np.any(out != want, axis=1))
    assert bad.size == 0, (
        f"{bad.size} packed records differ; first at output {int(bad[0])}: "
        f"got {out[bad[0]].tobytes().hex()}, want {want[bad[0]].tobytes().hex()}")


# ---- sort, scan, reduce, compact and merge primitives (test_gpu_finish_kernels.py) ----
#
# Records are (W key words, count) with the keys SoA, shape (W, n). Everything
# here has exactly one right answer, order included, so nothing is
# canonicalised: outputs are compared element by element.

def check_equal(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} != {want.dtype}"
    bad = np.flatnonzero((got != want).reshape(-1))
    assert bad.size == 0, (
        f"{what}: {bad.size} elements differ; first at flat index {int(bad[0])}: "
        f"got {got.reshape(-1)[bad[0]]}, want {want.reshape(-1)[bad[0]]}")


def scan_ref(a):
    """Exclusive scan in a's own unsigned type (wraps modulo 2^32 or 2^64)."""
    a = np.asarray(a)
    assert a.dtype in (np.uint32, np.uint64)
    out = np.zeros_like(a)
    np.cumsum(a[:-1], dtype=a.dtype, out=out[1:])
    return out


def check_scan(out, a, fill):
    """out: the whole output buffer (at least a.size elements): the scan, then the sentinel."""
    out = np.asarray(out)
    check_equal("scan", out[:a.size], scan_ref(a))
    check_fill(out[a.size:], fill)


def key_bits_ref(keys):
    """(W, n) -> 2 W words: OR of every word, then AND of every word."""
    keys = np.asarray(keys, dtype=U64)
    return np.concatenate([np.bitwise_or.reduce(keys, axis=1), np.bitwise_and.reduce(keys, axis=1)])


def digit_sort_ref(keys, word, shift):
    """Input indices in the order a stable sort by (keys[word] >> shift) & 255 leaves them."""
    return np.argsort(digit_of(keys[word], shift), kind="stable")


def check_soa(what, out_keys, out_cnts, want_keys, want_cnts, fill, off=0):
    """out_keys (W, S), out_cnts (S) or None: records [off, off + m) equal the
    wanted ones in order; every other element holds the sentinel."""
    out_keys = np.asarray(out_keys, dtype=U64)
    want_keys = np.asarray(want_keys, dtype=U64)
    m = want_keys.shape[1]
    assert off + m <= out_keys.shape[1]
    check_equal(f"{what} keys", out_keys[:, off:off + m], want_keys)
    check_fill(out_keys[:, :off], fill)
    check_fill(out_keys[:, off + m:], fill)
    if out_cnts is not None:
        out_cnts = np.asarray(out_cnts, dtype=np.uint32)
        check_equal(f"{what} counts", out_cnts[off:off + m], np.asarray(want_cnts, dtype=np.uint32))
        check_fill(out_cnts[:off], fill)
        check_fill(out_cnts[off + m:], fill)


def check_packed(what, out_bytes, want_keys, want_cnts, fill, skip=0):
    """out_bytes: the whole packed buffer; records [skip, skip + m) equal the
    wanted ones byte for byte, every other byte holds the sentinel."""
    want_keys = np.asarray(want_keys, dtype=U64)
    W, m = want_keys.shape
    rs = 8 * W + 4
    out = np.asarray(out_bytes, dtype=np.uint8).reshape(-1, rs)
    assert skip + m <= out.shape[0]
    check_equal(f"{what} packed records", out[skip:skip + m], pack_records(want_keys, want_cnts))
    check_fill(out[:skip], fill)
    check_fill(out[skip + m:], fill)


def unpack_records(rec_bytes, W):
    """(m, 8 W + 4) u8 -> (keys (W, m) u64, cnts (m) u32)."""
    b = np.ascontiguousarray(np.asarray(rec_bytes, dtype=np.uint8).reshape(-1, 8 * W + 4))
    keys = np.stack([np.ascontiguousarray(b[:, 8 * j:8 * j + 8]).view("<u8").reshape(-1) for j in range(W)])
    cnts = np.ascontiguousarray(b[:, 8 * W:]).view("<u4").reshape(-1)
    return keys.astype(U64), cnts.astype(np.uint32)


def check_sort_pass(out_keys, out_vals, keys, vals, word, shift, fill):
    """out_keys (W, S) / out_vals (S): the n records in stable digit order, values with their keys."""
    keys = np.asarray(keys, dtype=U64)
    p = digit_sort_ref(keys, word, shift)
    check_soa("sort pass", out_keys, out_vals, keys[:, p], None if vals is None else np.asarray(vals)[p], fill)


def rle_ref(keys):
    """Sorted keys (W, n) -> (flags (n) u32: 1 at the first record of a run,
    pos (n) u32: exclusive scan of flags, head (m): index of every run's first
    record, distinct keys (W, m), run lengths (m) u32)."""
    keys = np.asarray(keys, dtype=U64)
    n = keys.shape[1]
    flags = np.ones(n, dtype=np.uint32)
    flags[1:] = np.any(keys[:, 1:] != keys[:, :-1], axis=0)
    pos = scan_ref(flags)
    head = np.flatnonzero(flags).astype(np.uint32)
    lens = np.diff(np.append(head.astype(np.int64), n)).astype(np.uint32)
    return flags, pos, head, keys[:, head], lens


def segsum_ref(keys, cnts):
    """Sorted records -> (distinct keys (W, m), the counts of each summed modulo 2^32)."""
    flags, pos, head, dk, _ = rle_ref(keys)
    sums = np.add.reduceat(np.asarray(cnts, dtype=np.uint64), head.astype(np.int64)) & U64(0xffffffff)
    return dk, sums.astype(np.uint32)


def slot_words(W):
    return 2 if W == 1 else (4 if W <= 3 else 8)


def make_table(W, keys, cnts, state):
    """Open-addressed table of cap = keys.shape[1] slots: W key words, then
    count (low u32) | state << 32 (W >= 2; W = 1 has no state: a slot is
    occupied when its key is not 0, and `state` must say 2 exactly there).
    Words of a slot past these hold a pattern that nothing may read."""
    keys = np.asarray(keys, dtype=U64)
    cap = keys.shape[1]
    t = np.full((cap, slot_words(W)), U64(0x7777777777777777))
    t[:, :W] = keys.T
    if W == 1:
        assert np.array_equal(np.asarray(state) == 2, keys[0] != 0)
        t[:, 1] = np.asarray(cnts, dtype=U64)
    else:
        t[:, W] = np.asarray(cnts, dtype=U64) | (np.asarray(state, dtype=U64) << U64(32))
    return t


def compact_ref(W, table, out_cap, key0_present, key0_count):
    """(keys (W, m), cnts (m), cursor): the occupied slots in slot order (W = 1:
    key != 0; W >= 2: state == 2), then key 0 when present, nothing at or past
    out_cap. The cursor counts every occupied slot whether it fitted or not,
    plus key 0 when it was appended."""
    t = np.asarray(table, dtype=U64).reshape(-1, slot_words(W))
    occ = t[:, 0] != 0 if W == 1 else (t[:, W] >> U64(32)) == 2
    keys = t[occ, :W].T
    cnts = (t[occ, W] & U64(0xffffffff)).astype(np.uint32)
    total = int(occ.sum())
    keys, cnts = keys[:, :out_cap], cnts[:out_cap]
    if key0_present and total < out_cap:
        keys = np.concatenate([keys, np.zeros((W, 1), dtype=U64)], axis=1)
        cnts = np.append(cnts, np.uint32(key0_count & 0xffffffff))
        total += 1
    return keys, cnts, total


def check_compact(out_keys, out_cnts, cursor, W, table, out_cap, key0_present, key0_count, fill):
    """out_keys: W x out_cap + pad words (record i's word j at j * out_cap + i), out_cnts: out_cap + pad."""
    wk, wc, total = compact_ref(W, table, out_cap, key0_present, key0_count)
    assert int(cursor) == total, f"compact cursor {int(cursor)} != {total}"
    m = wk.shape[1]
    out_keys = np.asarray(out_keys, dtype=U64)
    check_soa("compact", out_keys[:W * out_cap].reshape(W, out_cap), np.asarray(out_cnts)[:out_cap], wk, wc, fill)
    check_fill(out_keys[W * out_cap:], fill)
    check_fill(np.asarray(out_cnts)[out_cap:], fill)
    return m


def merge_ref(ka, ca, kb, cb):
    """Stable merge of two sorted runs: lexsort over the concatenation A || B,
    word 0 most significant, the concatenation index last, so that equal keys
    keep A before B and their order inside a run. Returns (keys, cnts, src):
    src[i] is the index in A || B of output record i."""
    ka, kb = np.asarray(ka, dtype=U64), np.asarray(kb, dtype=U64)
    k = np.concatenate([ka, kb], axis=1)
    c = np.concatenate([np.asarray(ca, dtype=np.uint32), np.asarray(cb, dtype=np.uint32)])
    o = np.lexsort([np.arange(k.shape[1])] + [k[j] for j in range(k.shape[0] - 1, -1, -1)])
    return k[:, o], c[o], o


def dup_ref(keys):
    """1 exactly when two adjacent records have equal keys."""
    keys = np.asarray(keys, dtype=U64)
    return int(keys.shape[1] > 1 and bool(np.any(np.all(keys[:, 1:] == keys[:, :-1], axis=0))))


def check_dup(dup, out_keys):
    assert int(dup) == dup_ref(out_keys), f"dup flag {int(dup)} over an output whose equal-neighbour flag is {dup_ref(out_keys)}"


def check_merge_soa(out_keys, out_cnts, ka, ca, kb, cb, fill, off=0):
    wk, wc, _ = merge_ref(ka, ca, kb, cb)
    check_soa("merge", out_keys, out_cnts, wk, wc, fill, off)


def check_merge_packed(out_bytes, dup, ka, ca, kb, cb, fill, skip=0):
    wk, wc, _ = merge_ref(ka, ca, kb, cb)
    check_packed("merge", out_bytes, wk, wc, fill, skip)
    check_dup(dup, wk)


def owner_of(word0, world):
    """Owner of a key: ((word0 >> 32) * world) >> 32."""
    return (((np.asarray(word0, dtype=U64) >> U64(32)) * U64(world)) >> U64(32)).astype(np.int64)


def owner_bounds_ref(word0, world):
    """bounds[o], o in [0, world]: the first record owned by o or later."""
    return np.searchsorted(owner_of(word0, world), np.arange(world + 1), side="left").astype(U64)


def bucket_bounds_ref(word0, bits):
    """starts[b], b in [0, 2^bits]: the first key of bucket b (= word0 >> (64 - bits)) or later."""
    b = (np.asarray(word0, dtype=U64) >> U64(64 - bits)).astype(np.int64)
    return np.searchsorted(b, np.arange((1 << bits) + 1), side="left").astype(U64)


# ---- super-k-mer engine: front ends, P5a and P5 (test_gpu_skm_kernels.py) ----
#
# These restate the specification in the header comment of kc_skm.inl and in
# skm_geometry, over arrays of base codes, with none of the kernels' tiling:
# * a window of a read is live when its k bases are all ACGT and its key is
#   not 0^W (the key is K' bases from the window start; bases past the read
#   end read as 0, bytes outside ACGT as 3);
# * the bucket of a live window is the low 16 bits of the minimum mmer_hash
#   over its k - m + 1 m-mers, 0xffff mapped to 0xfffe;
# * a super-k-mer is a maximal run of consecutive live windows of one read
#   with equal bucket, cut into ceil(len / nmax) pieces of nmax windows (the
#   last one shorter); a piece is one record.
# A record is RW = W + 1 words; read MSB-first as one number it holds the
# bucket (16 bits), K' + n - 1 bases of 2 bits, zeros, and n in the low 6 bits.

_CODE = np.full(256, 3, dtype=np.uint8)
_ACGT = np.zeros(256, dtype=bool)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _ACGT[_c] = True
_PAD = 128  # zero codes behind every read: a key's bases past the read end


def skm_geom_ref(L, k):
    """m, K', nmax for (L, k) as skm_geometry derives them (None: not supported)."""
    W = (k + 31) // 32
    RW = W + 1
    if W > 3 or k < 18 or L < k:
        return None
    masked = (k + 3) // 4 < 8 * W  # the last key word holds fewer than 32 bases
    Kp = k if masked else 32 * W
    nmax = min(32 * RW - 10 - Kp, 63)  # K' + n - 1 bases + 16 + 6 bits fit RW words; n fits 6 bits
    m = min(max(k - nmax + 1, 11), 24)
    if k - m + 1 < 8:
        m = k - 7
    return dict(L=L, k=k, W=W, RW=RW, m=m, Kp=Kp, nmax=nmax, masked=masked)


def mmer_hash_ref(mm, m):
    """mmer_hash of m-mers (2 m bits, first base highest), the three regimes; u64 array of 32-bit values."""
    mm = np.asarray(mm, dtype=U64)
    M32 = U64(0xffffffff)
    if m <= 12:
        return ((mm ^ U64(0xd1e995)) * U64(0x9e3779)) & M32
    if m <= 16:
        return ((mm ^ U64(0x5bd1e995)) * U64(0x9e3779b1)) & M32
    x = (mm & M32) ^ (((mm >> U64(32)) * U64(0x9e3779b1)) & M32)
    return ((x ^ U64(0x5bd1e995)) * U64(0x9e3779b1)) & M32


def encode_reads_ref(reads, L=None):
    """(codes, ok, lens): (n, L + pad) base codes (A0 C1 G2 T3, other bytes 3,
    0 past the read's own end), the ACGT mask (False past the end) and the
    reads' lengths. L: the slot length (default: the longest read)."""
    lens = np.array([len(s) for s in reads], dtype=np.int64)
    L = int(lens.max()) if L is None else L
    assert np.all(lens <= L)
    buf = np.zeros((len(reads), L + _PAD), dtype=np.uint8)
    for i, s in enumerate(reads):
        buf[i, :len(s)] = np.frombuffer(s.encode("latin1"), dtype=np.uint8)
    inside = np.arange(L + _PAD)[None, :] < lens[:, None]
    return np.where(inside, _CODE[buf], 0).astype(np.uint8), inside & _ACGT[buf], lens


def _window_sums(flags, span, nw):
    """sum of flags[:, p:p + span] for p in [0, nw)."""
    c = np.zeros((flags.shape[0], flags.shape[1] + 1), dtype=np.int64)
    np.cumsum(flags, axis=1, out=c[:, 1:])
    return c[:, span:span + nw] - c[:, :nw]


def window_buckets_ref(codes, L, k, m):
    """(n, L - k + 1) buckets of every window of reads of L bases (meaningful for live windows)."""
    npos, nw = L - m + 1, L - k + 1
    mm = np.zeros((codes.shape[0], npos), dtype=U64)
    for i in range(m):
        mm = (mm << U64(2)) | codes[:, i:i + npos].astype(U64)
    h = mmer_hash_ref(mm, m)
    mn = h[:, :nw].copy()
    for j in range(1, k - m + 1):
        np.minimum(mn, h[:, j:j + nw], out=mn)
    b = (mn & U64(0xffff)).astype(np.int64)
    b[b == 0xffff] = 0xfffe
    return b


def bucket_ref(read_codes, window, k, m):
    """Bucket of the window starting at `window` of one read's codes, stated directly."""
    c = [int(x) for x in read_codes[window:window + k]]
    assert len(c) == k
    best = None
    for j in range(k - m + 1):
        mm = 0
        for x in c[j:j + m]:
            mm = (mm << 2) | x
        h = int(mmer_hash_ref(np.array([mm], dtype=U64), m)[0])
        best = h if best is None else min(best, h)
    b = best & 0xffff
    return 0xfffe if b == 0xffff else b


def skm_record_ref(bases, bucket, n, geom):
    """The RW words of the record of n keys over `bases` (K' + n - 1 codes), stated with Python integers."""
    RW, nb = geom["RW"], geom["Kp"] + n - 1
    assert 1 <= n <= geom["nmax"] and len(bases) == nb and 0 <= bucket < 0xffff
    v = int(bucket)
    for c in bases:
        v = (v << 2) | int(c)
    v = (v << (64 * RW - 16 - 2 * nb)) | n
    return [(v >> (64 * (RW - 1 - j))) & 0xffffffffffffffff for j in range(RW)]


def _pack_bases(b, nwords):
    """(n, 32 nwords) codes -> (nwords, n) u64, first base highest."""
    out = np.zeros((nwords, b.shape[0]), dtype=U64)
    for j in range(nwords):
        w = np.zeros(b.shape[0], dtype=U64)
        for i in range(32):
            w = (w << U64(2)) | b[:, 32 * j + i].astype(U64)
        out[j] = w
    return out


def skm_records_ref(codes, p_read, p_start, p_n, p_bucket, geom):
    """skm_record_ref for many pieces at once: piece i is p_n[i] windows from
    window p_start[i] of read p_read[i]. Returns (RW, npieces) words."""
    RW, Kp = geom["RW"], geom["Kp"]
    nbases = 32 * RW - 8  # bases a record has room for behind the bucket
    p_n = np.asarray(p_n, dtype=np.int64)
    idx = np.asarray(p_start, dtype=np.int64)[:, None] + np.arange(nbases)[None, :]
    assert idx.max(initial=0) < codes.shape[1]
    b = codes[np.asarray(p_read, dtype=np.int64)[:, None], idx]
    b = np.where(np.arange(nbases)[None, :] < (Kp + p_n - 1)[:, None], b, 0).astype(np.uint8)
    full = np.zeros((b.shape[0], 32 * RW), dtype=np.uint8)
    full[:, 8:] = b
    w = _pack_bases(full, RW)
    w[0] |= np.asarray(p_bucket, dtype=U64) << U64(48)
    w[RW - 1] |= p_n.astype(U64)
    return w


def skm_runs_ref(reads, k, geom, L=None):
    """The super-k-mers of `reads` (strings; L: the slot length when they vary).
    Returns a dict: run_read / run_start / run_len / run_bucket (maximal runs),
    p_read / p_start / p_n / p_bucket (their pieces), records (RW, npieces),
    valid / key0 / key0_present (the expected ST_VALID, ST_KEY0,
    ST_KEY0_PRESENT), codes / ok / lens (the encoded reads), live and bucket
    ((n, nw) per window)."""
    codes, ok, lens = encode_reads_ref(reads, L)
    L = codes.shape[1] - _PAD
    Kp, m, nmax = geom["Kp"], geom["m"], geom["nmax"]
    nw = L - k + 1
    own = np.arange(nw)[None, :] < (lens - k + 1)[:, None]  # windows of the read's own length
    valid = own & (_window_sums(~ok, k, nw) == 0)
    zero = _window_sums(codes != 0, Kp, nw) == 0
    live = valid & ~zero
    bucket = window_buckets_ref(codes, L, k, m)
    prev_same = np.zeros_like(live)
    prev_same[:, 1:] = live[:, :-1] & (bucket[:, 1:] == bucket[:, :-1])
    next_same = np.zeros_like(live)
    next_same[:, :-1] = live[:, 1:] & (bucket[:, 1:] == bucket[:, :-1])
    sr, sp = np.nonzero(live & ~prev_same)  # row-major: the i-th start pairs with the i-th end
    er, ep = np.nonzero(live & ~next_same)
    assert np.array_equal(sr, er) and np.all(ep >= sp)
    rlen = ep - sp + 1
    pieces = -(-rlen // nmax)
    run_of = np.repeat(np.arange(rlen.size), pieces)
    off = (np.arange(run_of.size) - np.repeat(np.cumsum(pieces) - pieces, pieces)) * nmax
    p_read, p_start = sr[run_of], sp[run_of] + off
    p_n = np.minimum(nmax, rlen[run_of] - off)
    p_bucket = bucket[sr, sp][run_of]
    hole = bool(np.any(own & ~valid))
    key0 = int(np.sum(valid & zero))
    return dict(run_read=sr, run_start=sp, run_len=rlen, run_bucket=bucket[sr, sp], p_read=p_read, p_start=p_start,
                p_n=p_n, p_bucket=p_bucket,
                records=skm_records_ref(codes, p_read, p_start, p_n, p_bucket, geom),
                valid=int(valid.sum()), key0=key0, key0_present=int(hole or key0 > 0), codes=codes, ok=ok, lens=lens,
                live=live, bucket=bucket)


def record_fields(records):
    """(bucket, n) of records (RW, n)."""
    records = np.asarray(records, dtype=U64)
    return (records[0] >> U64(48)).astype(np.int64), (records[-1] & U64(63)).astype(np.int64)


def _record_bases(records):
    """(n, 32 RW - 8) base codes of records (RW, n): everything behind the bucket (n's bits included)."""
    records = np.asarray(records, dtype=U64)
    RW, n = records.shape
    out = np.zeros((n, 32 * RW), dtype=np.uint8)
    for j in range(RW):
        for i in range(32):
            out[:, 32 * j + i] = ((records[j] >> U64(62 - 2 * i)) & U64(3)).astype(np.uint8)
    return out[:, 8:]


def skm_expand_ref(records, geom):
    """Records (RW, n) -> (bucket (nkeys), keys (W, nkeys), rec (nkeys)): key i
    of a record is K' bases from base i, which leaves the last word masked
    when K' = k; rec is the record each key came from."""
    W, Kp = geom["W"], geom["Kp"]
    bk, n = record_fields(records)
    assert np.all(n <= geom["nmax"])
    bases = _record_bases(records)
    rec = np.repeat(np.arange(n.size), n)
    ki = np.arange(rec.size) - np.repeat(np.cumsum(n) - n, n)
    kb = np.zeros((rec.size, 32 * W), dtype=np.uint8)
    kb[:, :Kp] = bases[rec[:, None], ki[:, None] + np.arange(Kp)[None, :]]
    return bk[rec], _pack_bases(kb, W), rec


def bucket_of_keys_ref(keys, geom):
    """Bucket of every key (W, n): of the window that its first k bases are."""
    keys = np.asarray(keys, dtype=U64)
    k = geom["k"]
    b = np.zeros((keys.shape[1], k), dtype=np.uint8)
    for i in range(k):
        b[:, i] = ((keys[i // 32] >> U64(62 - 2 * (i % 32))) & U64(3)).astype(np.uint8)
    return window_buckets_ref(b, k, k, geom["m"])[:, 0]


def count_keys_ref(keys, weights=None):
    """Keys (W, n) (+ weights) -> (distinct keys (W, m) in word-0-major order, their summed weights)."""
    keys = np.asarray(keys, dtype=U64)
    w = np.ones(keys.shape[1], dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    if keys.shape[1] == 0:
        return keys, w
    o = np.lexsort([keys[j] for j in range(keys.shape[0] - 1, -1, -1)])
    ks, ws = keys[:, o], w[o]
    head = np.ones(ks.shape[1], dtype=bool)
    head[1:] = np.any(ks[:, 1:] != ks[:, :-1], axis=0)
    hi = np.flatnonzero(head)
    return ks[:, hi], np.add.reduceat(ws, hi)


def sort_records(records):
    """Records (RW, n) sorted by all their words (a canonical order for multiset comparison)."""
    records = np.asarray(records, dtype=U64)
    return records[:, np.lexsort([records[j] for j in range(records.shape[0] - 1, -1, -1)])]


def check_record_multiset(what, got, want):
    got, want = sort_records(got), sort_records(want)
    assert got.shape == want.shape, f"{what}: {got.shape[1]} records, the reference has {want.shape[1]}"
    bad = np.flatnonzero(np.any(got != want, axis=0))
    assert bad.size == 0, (
        f"{what}: {bad.size} records differ after sorting; first at {int(bad[0])}: "
        f"got {[hex(int(x)) for x in got[:, bad[0]]]}, want {[hex(int(x)) for x in want[:, bad[0]]]}")


def group_records(records, nb=None):
    """Records (RW, n) stably grouped by bucket: (grouped, starts (nb + 1) u64)."""
    records = np.asarray(records, dtype=U64)
    bk, _ = record_fields(records)
    nb = int(bk.max(initial=0)) + 1 if nb is None else nb
    assert np.all(bk < nb)
    o = np.argsort(bk, kind="stable")
    return records[:, o], np.searchsorted(bk[o], np.arange(nb + 1), side="left").astype(U64)


# ---- key-prefix (partition) engine: P5, P5s, P1 / P2 (test_gpu_part_kernels.py) ----
#
# P5 (count_buckets) and P5s (sort_runs_k) turn keys grouped by bucket (word 0
# >> 48) and, pre-split, by sub-bucket (key bits 40..47) into (key, count)
# records in segments. A segment is described by desc_key (the first key its
# range can hold), desc_start (its first record) and desc_len = records |
# digit shift << 24 | sorted << 31. The finish orders descriptors by desc_key
# and sorts every segment with a 12-bit digit ((key48 - desc48) >> shift), so
# the contract is: segments of one bucket are disjoint key ranges in desc_key
# order, every record's digit is below 4096, a segment flagged sorted is
# strictly ascending.

M48 = (1 << 48) - 1


def p5_runs_ref(ss, per):
    """The greedy run walk over one bucket's 257 sub-bucket bounds: the run
    from s0 ends at the last e >= s0 + 1 with ss[e] - ss[s0] <= per (so a
    single sub-bucket above `per` is a run of its own); an empty run is
    skipped. Returns [(s0, e, multi)]: multi when the run's keys are <= per."""
    ss = [int(x) for x in ss]
    assert len(ss) == 257 and all(a <= b for a, b in zip(ss, ss[1:]))
    out = []
    s0 = 0
    while s0 < 256:
        e = s0 + 1
        while e < 256 and ss[e + 1] - ss[s0] <= per:
            e += 1
        if ss[e] > ss[s0]:
            out.append((s0, e, ss[e] - ss[s0] <= per))
        s0 = e
    return out


def bucket_counts_ref(keys, lo, hi):
    """Sorted distinct keys of keys[:, lo:hi] with their counts."""
    return count_keys_ref(np.asarray(keys, dtype=U64)[:, int(lo):int(hi)])


def desc_fields(desc_len):
    """desc_len -> (records, digit shift, sorted flag). The shift field is read
    with bit 30, which nothing sets: a stray bit there shows as a shift >= 64."""
    v = np.asarray(desc_len, dtype=np.uint32).astype(np.int64)
    return v & 0xffffff, (v >> 24) & 0x7f, v >> 31


def check_segments(what, keys, ranges, rec_keys, rec_cnts, cursor, desc, desc_fill, fill, extra=None):
    """The descriptor contract, stated once.
    keys (W, n): the launch's input. ranges: [(lo, hi, klo, khi)]: the launch
    was to count keys[:, lo:hi], whose word 0 lies in [klo, khi) (a bucket, or
    a run of sub-buckets); the ranges are disjoint. rec_keys (W, cap), rec_cnts
    (cap), cursor: the records. desc = (desc_key, desc_start, desc_len), whole
    arrays of the descriptor capacity; desc_fill: ST_DESC_FILL, at most that
    capacity. extra: (keys (W, m), counts) that went to the fallback table or
    the spill. Returns [(range index, desc_key, start, len, shift, sorted)] in
    desc_key order."""
    keys = np.asarray(keys, dtype=U64)
    W = keys.shape[0]
    dk, ds, dl = (np.asarray(x) for x in desc)
    nd = int(desc_fill)
    assert nd <= dk.size, f"{what}: {nd} descriptors counted, capacity {dk.size}"
    check_fill(dk[nd:], fill)
    check_fill(ds[nd:], fill)
    check_fill(dl[nd:], fill)
    ln, sh, srt = desc_fields(dl[:nd])
    assert np.all(ln > 0), f"{what}: a descriptor of no records"
    assert np.all(sh < 64), f"{what}: a descriptor shift of {int(sh.max())}"
    # the segments tile [0, cursor)
    st = ds[:nd].astype(np.int64)
    o = np.argsort(st, kind="stable")
    ends = st[o] + ln[o]
    assert nd == 0 or st[o][0] == 0, f"{what}: the first segment starts at {int(st[o][0])}"
    assert np.array_equal(ends[:-1], st[o][1:]), f"{what}: segments overlap or leave a gap"
    assert (int(ends[-1]) if nd else 0) == int(cursor), f"{what}: segments end at {int(ends[-1]) if nd else 0}, cursor {cursor}"
    assert int(cursor) <= rec_keys.shape[1]
    # every descriptor inside one range; its key range ends at the next descriptor of the range or the range's end
    klo = np.array([r[2] for r in ranges], dtype=U64)
    khi = [int(r[3]) for r in ranges]
    assert np.all(klo[1:] > klo[:-1]), "ranges must ascend"
    ko = np.argsort(dk[:nd], kind="stable")
    segs = []
    for x, i in enumerate(ko):
        key = int(dk[i])
        r = int(np.searchsorted(klo, U64(key), side="right")) - 1
        assert r >= 0 and key < khi[r], f"{what}: desc_key {key:#x} outside every range the launch was to count"
        top = khi[r]
        if x + 1 < nd and int(dk[ko[x + 1]]) < khi[r]:
            top = int(dk[ko[x + 1]])
            assert top > key, f"{what}: two segments with desc_key {key:#x}"
        a, n, s = int(st[i]), int(ln[i]), int(sh[i])
        w0 = rec_keys[0, a:a + n]
        assert np.all(w0 >= U64(key)) and (top >= 1 << 64 or np.all(w0 < U64(top))), (
            f"{what}: a record outside its segment's key range [{key:#x}, {top:#x})")
        dig = ((w0 & U64(M48)) - U64(key & M48)) >> U64(s)
        assert np.all(dig < U64(4096)), (
            f"{what}: shift {s} of segment {key:#x} gives digit {int(dig.max())} (>= 4096)")
        if srt[i]:
            k = rec_keys[:, a:a + n]
            if n > 1:
                lt = np.zeros(n - 1, dtype=bool)
                eq = np.ones(n - 1, dtype=bool)
                for j in range(W):
                    lt |= eq & (k[j, :-1] < k[j, 1:])
                    eq &= k[j, :-1] == k[j, 1:]
                assert np.all(lt), f"{what}: segment {key:#x} is flagged sorted and is not strictly ascending"
        segs.append((r, key, a, n, s, int(srt[i])))
    # the union: every record key once, records + fallback = the full counts
    got_k = rec_keys[:, :int(cursor)]
    got_c = np.asarray(rec_cnts[:int(cursor)], dtype=np.int64)
    uk, uc = count_keys_ref(got_k)
    assert uk.shape[1] == got_k.shape[1], f"{what}: {got_k.shape[1] - uk.shape[1]} keys appear in two records"
    if extra is not None and extra[0].shape[1]:
        got_k = np.concatenate([got_k, np.asarray(extra[0], dtype=U64)], axis=1)
        got_c = np.concatenate([got_c, np.asarray(extra[1], dtype=np.int64)])
    gk, gc = count_keys_ref(got_k, got_c)
    want = np.concatenate([keys[:, int(r[0]):int(r[1])] for r in ranges], axis=1) if ranges else keys[:, :0]
    wk, wc = count_keys_ref(want)
    check_equal(f"{what}: counted keys", gk, wk)
    check_equal(f"{what}: counts", gc, wc)
    return segs


def table_entries(W, table):
    """The occupied slots of a fallback table read back: (keys (W, m), counts)."""
    t = np.asarray(table, dtype=U64).reshape(-1, slot_words(W))
    occ = t[:, 0] != 0 if W == 1 else (t[:, W] >> U64(32)) == 2
    return t[occ, :W].T.copy(), (t[occ, W] & U64(0xffffffff)).astype(np.int64)


# P1 / P2 (count_front with the histogram and the scatter sink) walk the
# windows of fixed-length reads. The key of a window is K' bases from its
# start (K' = k, the rest of the last word cleared, or 32 W when k mod 32 is
# 29..31: the bases following the k-mer, 0 past the read end); a window
# holding a byte outside ACGT is dropped; the key 0^W is counted in the
# statistics and not emitted. Reads are cut into tiles of R reads and segments
# of seg_tiles tiles (the library's geometry).

def window_keys_ref(reads, k):
    """(keys (W, n_reads, nw) u64, valid (n_reads, nw), zero (n_reads, nw))."""
    codes, ok, lens = encode_reads_ref(reads)
    L = codes.shape[1] - _PAD
    assert np.all(lens == L)
    W = (k + 31) // 32
    Kp = k if (k + 3) // 4 < 8 * W else 32 * W
    nw = L - k + 1
    valid = _window_sums(~ok, k, nw) == 0
    keys = np.zeros((W, codes.shape[0], nw), dtype=U64)
    for i in range(Kp):
        keys[i // 32] |= codes[:, i:i + nw].astype(U64) << U64(62 - 2 * (i % 32))
    zero = ~np.any(keys != 0, axis=0)
    return keys, valid, zero


def part_digits_ref(w0, shift, flo=0, fhi=256):
    """(digit (w0 >> shift) & 255, in-range mask: flo <= w0 >> 56 < fhi)."""
    w0 = np.asarray(w0, dtype=U64)
    top = (w0 >> U64(56)).astype(np.int64)
    return ((w0 >> U64(shift)) & U64(255)).astype(np.int64), (top >= flo) & (top < fhi)


def part_front_ref(reads, k, R, seg_tiles, shift, flo=0, fhi=256):
    """What P1 and P2 owe for these reads: a dict of
    keys (W, m): the emitted keys (live windows in [flo, fhi)) in read order,
    seg (m), dig (m): their segment and digit, nseg,
    hist (256, nseg): P1's counts hist[d, seg],
    valid, key0, key0_present: the statistics of all windows (no range filter)."""
    keys, valid, zero = window_keys_ref(reads, k)
    n, nw = valid.shape
    nseg = -(-(-(-n // R)) // seg_tiles)
    seg_of_read = (np.arange(n) // R) // seg_tiles
    live = valid & ~zero
    dig, inr = part_digits_ref(keys[0], shift, flo, fhi)
    emit = live & inr
    seg = np.broadcast_to(seg_of_read[:, None], emit.shape)[emit]
    hist = np.zeros((256, nseg), dtype=np.int64)
    np.add.at(hist, (dig[emit], seg), 1)
    return dict(keys=keys[:, emit], seg=seg, dig=dig[emit], nseg=nseg, hist=hist, valid=int(valid.sum()),
                key0=int((valid & zero).sum()), key0_present=int(bool((~valid).any() or (valid & zero).any())))


def part_slices_ref(ref, base):
    """P2's slices: [(d, seg, start, keys (W, c) of that slice)] for base[d, seg] = where the run of
    (digit, segment) starts."""
    out = []
    o = np.lexsort((ref["seg"], ref["dig"]))
    d, s = ref["dig"][o], ref["seg"][o]
    k = ref["keys"][:, o]
    cut = np.flatnonzero(np.r_[True, (d[1:] != d[:-1]) | (s[1:] != s[:-1]), True])
    for a, b in zip(cut[:-1], cut[1:]):
        out.append((int(d[a]), int(s[a]), int(base[d[a], s[a]]), k[:, a:b]))
    return out
