"""The checker of the kernel-level tests, checked on the CPU: kernel_ref's
references against numpy's own sorts, and every comparison helper against a
corruption it must reject (a checker that canonicalises too much would let a
wrong kernel pass)."""
import numpy as np
import pytest

import kernel_ref as kr
import kmer_ref_py as pyref
import skm_reads

U64 = np.uint64


def _items(n, nw, seed):
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 2**64, size=(nw, n), dtype=U64)
    pay = rng.integers(0, 2**32, size=n, dtype=np.uint32)
    return words, pay


def test_two_pass_lsd_reference_is_a_stable_sort_by_prefix():
    n = 5000
    words, pay = _items(n, 2, 1)
    words[0] &= U64(0x0313ffffffffffff)  # 32 prefixes, each many times
    p1, b1 = kr.rp_ref(kr.digit_of(words[0], 48), [0, n], regional=False)
    w1 = words[:, p1]
    rstart = np.append(kr.rp_bases(b1, 1, False), U64(n)).astype(np.int64)
    p2, b2 = kr.rp_ref(kr.digit_of(w1[0], 56), rstart, regional=False)
    pref = (words[0] >> U64(48)).astype(np.int64)
    assert np.array_equal(p1[p2], np.argsort(pref, kind="stable"))
    # level 2's block (digit d2, region d1) is the 16-bit group d2 << 8 | d1
    assert np.array_equal(b2, np.searchsorted(np.sort(pref), np.arange(65537)))


def test_regional_reference_sub_starts_are_searchsorted():
    n = 3000
    words, _ = _items(n, 1, 2)
    rstart = np.array([0, 0, 7, 7, 1500, 2999, 3000, 3000])
    dig = kr.digit_of(words[0], 40)
    perm, bounds = kr.rp_ref(dig, rstart, regional=True)
    reg = kr.region_of(rstart, n)
    comp = reg * 256 + dig
    assert np.array_equal(comp[perm], np.sort(comp, kind="stable"))
    assert np.array_equal(bounds, np.searchsorted(np.sort(comp), np.arange(len(rstart) * 256 - 255)))
    sub = kr.rp_bases(bounds, len(rstart) - 1, True)
    assert sub[-1] == n and sub.size == (len(rstart) - 1) * 256 + 1
    # regions stay where they are
    assert np.array_equal(np.sort(perm[7:1500]), np.arange(7, 1500))


def _grouped_case():
    n = 4000
    words, pay = _items(n, 2, 3)
    rstart = [0, 1000, 1000, 4000]
    dig = kr.digit_of(words[0], 8)
    perm, bounds = kr.rp_ref(dig, rstart, regional=False)
    rows = kr.as_rows(words, pay)
    return rows, rows[perm].copy(), dig, rstart, bounds


def test_grouped_accepts_the_reference_and_any_order_inside_a_block():
    rows, out, dig, rstart, bounds = _grouped_case()
    kr.check_grouped(out, rows, dig, rstart, False)
    b = int(np.flatnonzero(np.diff(bounds) >= 2)[0])
    lo = int(bounds[b])
    out[[lo, lo + 1]] = out[[lo + 1, lo]]
    kr.check_grouped(out, rows, dig, rstart, False)


def test_grouped_rejects_rows_swapped_across_a_block_boundary():
    rows, out, dig, rstart, bounds = _grouped_case()
    edge = int(bounds[np.flatnonzero((np.diff(bounds)[:-1] > 0) & (np.diff(bounds)[1:] > 0))[0] + 1])
    out[[edge - 1, edge]] = out[[edge, edge - 1]]
    with pytest.raises(AssertionError):
        kr.check_grouped(out, rows, dig, rstart, False)


def test_grouped_rejects_a_payload_swapped_inside_a_block():
    rows, out, dig, rstart, bounds = _grouped_case()
    lo = int(bounds[np.flatnonzero(np.diff(bounds) >= 2)[0]])
    assert out[lo, -1] != out[lo + 1, -1]
    out[[lo, lo + 1], -1] = out[[lo + 1, lo], -1]
    with pytest.raises(AssertionError):
        kr.check_grouped(out, rows, dig, rstart, False)


def test_grouped_rejects_a_row_duplicated_over_another():
    rows, out, dig, rstart, bounds = _grouped_case()
    lo = int(bounds[np.flatnonzero(np.diff(bounds) >= 2)[0]])
    out[lo + 1] = out[lo]
    with pytest.raises(AssertionError):
        kr.check_grouped(out, rows, dig, rstart, False)


def test_bases_reject_a_shifted_start():
    rows, out, dig, rstart, bounds = _grouped_case()
    good = kr.rp_bases(bounds, 3, False)
    kr.check_bases(good, bounds, 3, False)
    bad = good.copy()
    bad[17] += U64(1)
    with pytest.raises(AssertionError):
        kr.check_bases(bad, bounds, 3, False)


def test_emit_rejects_one_wrong_byte():
    words, _ = _items(1000, 1, 4)
    emit = kr.digit_of(words[0], 56).astype(np.uint8)
    kr.check_emit(emit, words[0], 56)
    emit[123] ^= 1
    with pytest.raises(AssertionError):
        kr.check_emit(emit, words[0], 56)


def _seg_case(W=2):
    rng = np.random.default_rng(5)
    n = 600
    keys = rng.integers(0, 2**64, size=(W, n), dtype=U64)
    keys[0] &= U64(0xff)  # word 0 ties, so the later words decide
    cnts = rng.integers(1, 2**32, size=n, dtype=np.uint32)
    segs = [(0, 100, 5), (100, 0, 105), (100, 1, 110), (101, 499, 120)]
    nout = 640
    wk, wc, pos, _ = kr.seg_sort_ref(keys, cnts, segs, nout)
    ok = np.full((W, nout), U64(0xabababababababab))
    oc = np.full(nout, 0xabababab, dtype=np.uint32)
    ok[:, pos] = wk
    oc[pos] = wc
    return keys, cnts, segs, ok, oc


def _packed(ok, oc):
    return kr.pack_records(ok, oc)


def test_segment_reference_is_a_full_key_sort():
    keys, cnts, segs, ok, oc = _seg_case(3)
    got = [tuple(int(x) for x in ok[:, i]) for i in range(120, 619)]
    want = sorted(tuple(int(x) for x in keys[:, i]) for i in range(101, 600))
    assert got == want
    by_key = {tuple(int(x) for x in keys[:, i]): int(cnts[i]) for i in range(101, 600)}
    assert [by_key[k] for k in got] == [int(c) for c in oc[120:619]]
    kr.check_seg_soa(ok, oc, keys, cnts, segs, 0xab)
    kr.check_seg_packed(_packed(ok, oc), keys, cnts, segs, 0xab)


def test_segment_rejects_two_adjacent_records_exchanged():
    keys, cnts, segs, ok, oc = _seg_case()
    ok[:, [300, 301]] = ok[:, [301, 300]]
    oc[[300, 301]] = oc[[301, 300]]
    with pytest.raises(AssertionError):
        kr.check_seg_soa(ok, oc, keys, cnts, segs, 0xab)
    with pytest.raises(AssertionError):
        kr.check_seg_packed(_packed(ok, oc), keys, cnts, segs, 0xab)


def test_segment_rejects_a_count_moved_to_the_neighbouring_key():
    keys, cnts, segs, ok, oc = _seg_case()
    assert oc[300] != oc[301]
    oc[[300, 301]] = oc[[301, 300]]
    with pytest.raises(AssertionError):
        kr.check_seg_soa(ok, oc, keys, cnts, segs, 0xab)
    with pytest.raises(AssertionError):
        kr.check_seg_packed(_packed(ok, oc), keys, cnts, segs, 0xab)


def test_segment_accepts_counts_of_equal_keys_in_any_order_only():
    keys, cnts, segs, ok, oc = _seg_case()
    keys[:, 201] = keys[:, 200]
    wk, wc, pos, _ = kr.seg_sort_ref(keys, cnts, segs, ok.shape[1])
    ok[:, pos] = wk
    oc[pos] = wc
    i = int(np.flatnonzero(np.all(wk[:, 1:] == wk[:, :-1], axis=0))[0])
    a, b = int(pos[i]), int(pos[i + 1])
    oc[[a, b]] = oc[[b, a]]
    kr.check_seg_soa(ok, oc, keys, cnts, segs, 0xab)
    oc[a] = oc[b]  # one count lost, the other twice
    with pytest.raises(AssertionError):
        kr.check_seg_soa(ok, oc, keys, cnts, segs, 0xab)


def test_segment_rejects_a_clobbered_sentinel():
    keys, cnts, segs, ok, oc = _seg_case()
    for where in (0, 106, 119, 639):
        k2, c2 = ok.copy(), oc.copy()
        k2[1, where] = U64(0)
        with pytest.raises(AssertionError):
            kr.check_seg_soa(k2, c2, keys, cnts, segs, 0xab)
        k2, c2 = ok.copy(), oc.copy()
        c2[where] ^= 1
        with pytest.raises(AssertionError):
            kr.check_seg_soa(k2, c2, keys, cnts, segs, 0xab)
        pk = _packed(ok, oc)
        pk[where, 3] = 0
        with pytest.raises(AssertionError):
            kr.check_seg_packed(pk, keys, cnts, segs, 0xab)
    with pytest.raises(AssertionError):
        kr.check_fill(np.array([0xabab, 0xabaa], dtype=np.uint16), 0xab)


# ---- sort, scan, reduce, compact and merge primitives ----

FILL = 0xab
FILL64 = U64(0xabababababababab)
FILL32 = np.uint32(0xabababab)


def _sorted_run(W, n, seed, ties=True):
    """A sorted run whose word 0 takes few values, so that later words decide."""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 2**64, size=(W, n), dtype=U64)
    if ties:
        keys[0] &= U64(7)
    o = np.lexsort([keys[j] for j in range(W - 1, -1, -1)])
    return keys[:, o]


def _padded(wk, wc, off=0, pad=4):
    W, m = wk.shape
    ok = np.full((W, off + m + pad), FILL64)
    oc = np.full(off + m + pad, FILL32)
    ok[:, off:off + m] = wk
    oc[off:off + m] = wc
    return ok, oc


def _packed_padded(wk, wc, skip=0, pad=2):
    m = wk.shape[1]
    out = np.full((skip + m + pad, 8 * wk.shape[0] + 4), FILL, dtype=np.uint8)
    out[skip:skip + m] = kr.pack_records(wk, wc)
    return out


def _merge_case(W=2):
    ka, kb = _sorted_run(W, 300, 11), _sorted_run(W, 200, 12)
    kb[:, 50:60] = ka[:, 100:101]  # ten B records tie with A's record 100
    kb = kb[:, np.lexsort([kb[j] for j in range(W - 1, -1, -1)])]
    ca = np.arange(300, dtype=np.uint32)
    cb = np.arange(200, dtype=np.uint32) + np.uint32(2**31)
    return ka, ca, kb, cb


def test_merge_reference_is_the_stable_merge():
    for W in (1, 3):
        ka, ca, kb, cb = _merge_case(W)
        wk, wc, src = kr.merge_ref(ka, ca, kb, cb)
        rows = [(tuple(int(x) for x in ka[:, i]), 0, i, int(ca[i])) for i in range(300)] + \
               [(tuple(int(x) for x in kb[:, i]), 1, i, int(cb[i])) for i in range(200)]
        rows.sort(key=lambda r: r[:3])  # key, then A before B, then the order inside the run
        assert [r[0] for r in rows] == [tuple(int(x) for x in wk[:, i]) for i in range(500)]
        assert [r[3] for r in rows] == [int(c) for c in wc]
        assert np.array_equal(np.sort(src), np.arange(500))
        ok, oc = _padded(wk, wc, off=3)
        kr.check_merge_soa(ok, oc, ka, ca, kb, cb, FILL, off=3)
        kr.check_merge_packed(_packed_padded(wk, wc, skip=1), 1, ka, ca, kb, cb, FILL, skip=1)


def _first_ab_tie(wk, wc):
    same = np.all(wk[:, 1:] == wk[:, :-1], axis=0)
    i = int(np.flatnonzero(same & (wc[:-1] < 2**31) & (wc[1:] >= 2**31))[0])
    return i


def test_merge_rejects_one_tie_taken_b_first():
    ka, ca, kb, cb = _merge_case()
    wk, wc, _ = kr.merge_ref(ka, ca, kb, cb)
    i = _first_ab_tie(wk, wc)
    wc[[i, i + 1]] = wc[[i + 1, i]]  # the keys are equal: only the counts tell
    ok, oc = _padded(wk, wc)
    with pytest.raises(AssertionError):
        kr.check_merge_soa(ok, oc, ka, ca, kb, cb, FILL)
    with pytest.raises(AssertionError):
        kr.check_merge_packed(_packed_padded(wk, wc), 1, ka, ca, kb, cb, FILL)


def test_merge_and_segsum_reject_two_counts_exchanged_between_neighbouring_keys():
    ka, ca, kb, cb = _merge_case()
    wk, wc, _ = kr.merge_ref(ka, ca, kb, cb)
    i = int(np.flatnonzero(np.any(wk[:, 1:] != wk[:, :-1], axis=0))[0])
    bad = wc.copy()
    bad[[i, i + 1]] = bad[[i + 1, i]]
    ok, oc = _padded(wk, bad)
    with pytest.raises(AssertionError):
        kr.check_merge_soa(ok, oc, ka, ca, kb, cb, FILL)
    with pytest.raises(AssertionError):
        kr.check_merge_packed(_packed_padded(wk, bad), 1, ka, ca, kb, cb, FILL)
    dk, ds = kr.segsum_ref(wk, wc)
    ok, oc = _padded(dk, ds)
    kr.check_soa("sum", ok, oc, dk, ds, FILL)
    assert ds[0] != ds[1]
    ok, oc = _padded(dk, ds)
    oc[[0, 1]] = oc[[1, 0]]
    with pytest.raises(AssertionError):
        kr.check_soa("sum", ok, oc, dk, ds, FILL)


def test_dup_flag_rejected_both_ways():
    ka, ca, kb, cb = _merge_case()
    wk, wc, _ = kr.merge_ref(ka, ca, kb, cb)
    one = np.array([[1, 2, 2, 3]], dtype=U64)  # exactly one equal pair
    none = np.array([[1, 2, 3, 4]], dtype=U64)
    assert kr.dup_ref(one) == 1 and kr.dup_ref(none) == 0 and kr.dup_ref(none[:, :1]) == 0
    assert kr.dup_ref(np.array([[1, 1], [5, 6]], dtype=U64)) == 0  # the last word differs
    kr.check_dup(1, one)
    kr.check_dup(0, none)
    with pytest.raises(AssertionError):
        kr.check_dup(0, one)
    with pytest.raises(AssertionError):
        kr.check_dup(1, none)
    with pytest.raises(AssertionError):
        kr.check_merge_packed(_packed_padded(wk, wc), 0, ka, ca, kb, cb, FILL)


def test_scan_reference_wraps_and_rejects_an_offset_of_one_element():
    rng = np.random.default_rng(21)
    for dt, bits in ((np.uint32, 32), (np.uint64, 64)):
        a = rng.integers(0, 2**bits, size=1000, dtype=dt)
        want, run = [], 0
        for v in a:
            want.append(run)
            run = (run + int(v)) % 2**bits
        ref = kr.scan_ref(a)
        assert ref.dtype == dt and [int(x) for x in ref] == want
        out = np.full(1005, 0xabababababababab & (2**bits - 1), dtype=dt)
        out[:1000] = ref
        kr.check_scan(out, a, FILL)
        bad = out.copy()
        bad[1:1000] = ref[:999]  # every element one place late
        with pytest.raises(AssertionError):
            kr.check_scan(bad, a, FILL)
        bad = out.copy()
        bad[:1000] = ref + a  # the inclusive scan
        with pytest.raises(AssertionError):
            kr.check_scan(bad, a, FILL)
        bad = out.copy()
        bad[1000] = 0
        with pytest.raises(AssertionError):
            kr.check_scan(bad, a, FILL)
    assert kr.scan_ref(np.array([9], dtype=np.uint32)).tolist() == [0]


def test_sort_pass_reference_is_stable_and_rejects_two_equal_digit_records_exchanged():
    rng = np.random.default_rng(22)
    keys = rng.integers(0, 2**64, size=(2, 500), dtype=U64)
    vals = np.arange(500, dtype=np.uint32)
    p = kr.digit_sort_ref(keys, 1, 24)
    dig = [(int(keys[1, i]) >> 24) & 255 for i in range(500)]
    assert p.tolist() == sorted(range(500), key=lambda i: dig[i])  # Python's sort is stable
    ok, ov = _padded(keys[:, p], vals[p])
    kr.check_sort_pass(ok, ov, keys, vals, 1, 24, FILL)
    d = np.array(dig)[p]
    i = int(np.flatnonzero(d[1:] == d[:-1])[0])
    ok[:, [i, i + 1]] = ok[:, [i + 1, i]]
    ov[[i, i + 1]] = ov[[i + 1, i]]
    with pytest.raises(AssertionError):
        kr.check_sort_pass(ok, ov, keys, vals, 1, 24, FILL)
    with pytest.raises(AssertionError):  # without values the keys alone tell
        kr.check_sort_pass(ok, None, keys, None, 1, 24, FILL)


def test_key_bits_reference():
    keys = np.array([[0b1100, 0b1010, 0b1000], [7, 7, 7]], dtype=U64)
    assert kr.key_bits_ref(keys).tolist() == [0b1110, 7, 0b1000, 7]


def test_rle_and_segsum_references():
    keys = np.array([[1, 1, 1, 2, 2, 9], [5, 5, 6, 0, 0, 0]], dtype=U64)
    flags, pos, head, dk, lens = kr.rle_ref(keys)
    assert flags.tolist() == [1, 0, 1, 1, 0, 1] and pos.tolist() == [0, 1, 1, 2, 3, 3]
    assert head.tolist() == [0, 2, 3, 5] and lens.tolist() == [2, 1, 2, 1]
    assert dk.tolist() == [[1, 1, 2, 9], [5, 6, 0, 0]]
    cnts = np.array([2**32 - 1, 3, 10, 2**31, 2**31, 7], dtype=np.uint32)
    dk2, sums = kr.segsum_ref(keys, cnts)
    assert np.array_equal(dk2, dk) and sums.tolist() == [2, 10, 0, 7]  # modulo 2^32
    f1, p1, h1, d1, l1 = kr.rle_ref(keys[:, :1])
    assert f1.tolist() == [1] and p1.tolist() == [0] and l1.tolist() == [1]


def test_pack_and_unpack_are_inverse():
    keys = _sorted_run(3, 50, 23)
    cnts = np.arange(50, dtype=np.uint32) * np.uint32(77777)
    pk = kr.pack_records(keys, cnts)
    assert pk.shape == (50, 28) and pk[1, 24:].tobytes() == (77777).to_bytes(4, "little")
    assert pk[0, :8].tobytes() == int(keys[0, 0]).to_bytes(8, "little")
    k2, c2 = kr.unpack_records(pk, 3)
    assert np.array_equal(k2, keys) and np.array_equal(c2, cnts)


def _compact_case(W):
    rng = np.random.default_rng(24 + W)
    cap = 300
    keys = rng.integers(1, 2**64, size=(W, cap), dtype=U64)
    state = rng.integers(0, 3, size=cap)
    if W == 1:
        keys[0, state != 2] = 0
    cnts = rng.integers(1, 2**32, size=cap, dtype=np.uint32)
    return kr.make_table(W, keys, cnts, state), keys, cnts, state


@pytest.mark.parametrize("W", (1, 2, 4))
def test_compact_reference_and_what_it_rejects(W):
    table, keys, cnts, state = _compact_case(W)
    occ = np.flatnonzero(state == 2)
    wk, wc, total = kr.compact_ref(W, table, occ.size + 1, True, 2**32 + 5)
    assert total == occ.size + 1
    assert np.array_equal(wk[:, :-1], keys[:, occ]) and np.array_equal(wc[:-1], cnts[occ])
    assert not wk[:, -1].any() and wc[-1] == 5
    # nothing at or past out_cap; the cursor still counts every occupied slot
    wk, wc, total = kr.compact_ref(W, table, occ.size - 5, True, 1)
    assert total == occ.size and wk.shape[1] == occ.size - 5 and np.array_equal(wc, cnts[occ][:-5])
    out_cap = occ.size + 1
    wk, wc, total = kr.compact_ref(W, table, out_cap, False, 0)
    ok = np.full(W * out_cap + 3, FILL64)
    oc = np.full(out_cap + 3, FILL32)
    ok[:W * out_cap].reshape(W, out_cap)[:, :occ.size] = wk
    oc[:occ.size] = wc
    assert kr.check_compact(ok, oc, total, W, table, out_cap, False, 0, FILL) == occ.size
    with pytest.raises(AssertionError):
        kr.check_compact(ok, oc, total + 1, W, table, out_cap, False, 0, FILL)
    bad = oc.copy()
    bad[out_cap + 1] = 0  # a clobbered sentinel behind the counts
    with pytest.raises(AssertionError):
        kr.check_compact(ok, bad, total, W, table, out_cap, False, 0, FILL)
    if W >= 2:
        # a compaction that takes a claimed-but-unfinished slot (state 1) too
        inc = np.flatnonzero(state >= 1)[:out_cap]
        ok2 = np.full(W * out_cap + 3, FILL64)
        oc2 = np.full(out_cap + 3, FILL32)
        ok2[:W * out_cap].reshape(W, out_cap)[:, :inc.size] = keys[:, inc]
        oc2[:inc.size] = cnts[inc]
        assert (state == 1).any()
        with pytest.raises(AssertionError):
            kr.check_compact(ok2, oc2, total, W, table, out_cap, False, 0, FILL)


def test_soa_and_packed_checks_reject_a_clobbered_sentinel():
    wk = _sorted_run(2, 40, 25)
    wc = np.arange(40, dtype=np.uint32)
    ok, oc = _padded(wk, wc, off=3)
    kr.check_soa("x", ok, oc, wk, wc, FILL, off=3)
    for col in (0, 2, 43, 46):
        k2 = ok.copy()
        k2[1, col] ^= U64(1 << 40)
        with pytest.raises(AssertionError):
            kr.check_soa("x", k2, oc, wk, wc, FILL, off=3)
        c2 = oc.copy()
        c2[col] ^= np.uint32(1)
        with pytest.raises(AssertionError):
            kr.check_soa("x", ok, c2, wk, wc, FILL, off=3)
    pk = _packed_padded(wk, wc, skip=1)
    kr.check_packed("x", pk, wk, wc, FILL, skip=1)
    for row, byte in ((0, 0), (0, 19), (41, 0), (42, 19)):
        p2 = pk.copy()
        p2[row, byte] = 0
        with pytest.raises(AssertionError):
            kr.check_packed("x", p2, wk, wc, FILL, skip=1)


def test_owner_and_bucket_bounds_references():
    w0 = np.sort(np.random.default_rng(26).integers(0, 2**64, size=400, dtype=U64))
    for world in (1, 3, 8, 1000):
        own = [((int(x) >> 32) * world) >> 32 for x in w0]
        b = kr.owner_bounds_ref(w0, world)
        assert b.size == world + 1 and b[0] == 0 and b[-1] == 400
        assert b.tolist() == [sum(1 for v in own if v < o) for o in range(world + 1)]
    assert kr.owner_bounds_ref(w0[:0], 4).tolist() == [0] * 5
    s = kr.bucket_bounds_ref(w0, 4)
    assert s.tolist() == [sum(1 for x in w0 if (int(x) >> 60) < b) for b in range(17)]


# ---- super-k-mer references (test_gpu_skm_kernels.py) ----

# one k per key width and m-mer hash regime, K' = k and K' = 32 W:
# (k, W, m, K' == k)
SKM_KS = [(19, 1, 11, True), (31, 1, 11, False), (50, 2, 15, True), (55, 2, 24, True), (62, 2, 24, False),
          (66, 3, 15, True), (94, 3, 24, False)]


def _mixed_reads(L, k, seed):
    return (skm_reads.special_reads(L, 60, seed) + skm_reads.edge_reads(L, k, seed) +
            skm_reads.genome_reads(L, 60, seed, genome=300))


def test_skm_geometry_reference_regimes():
    for k, W, m, masked in SKM_KS:
        g = kr.skm_geom_ref(k + 40, k)
        assert (g["W"], g["m"], g["masked"]) == (W, m, masked), (k, g)
        assert g["Kp"] == (k if masked else 32 * W)
        assert g["Kp"] + g["nmax"] - 1 <= 32 * g["RW"] - 11 and g["nmax"] <= 63 and k - g["m"] + 1 >= 8
    assert kr.skm_geom_ref(30, 31) is None and kr.skm_geom_ref(100, 17) is None and kr.skm_geom_ref(200, 97) is None


@pytest.mark.parametrize("k,W,m,masked", SKM_KS)
def test_skm_reference_records_expand_to_the_reference_counts(k, W, m, masked):
    """The reference records of mixed reads, expanded, are exactly the k-mers
    of the pure-Python statement of the reference (kmer_ref_py.count_reads)
    minus key 0^W, whose count is the reference's ST_KEY0; every expanded key
    has its record's bucket; no run continues where the bucket or liveness
    changes, and the pieces of a run are ceil(len / nmax)."""
    L = k + kr.skm_geom_ref(k, k)["nmax"] + 10  # more windows than a record holds
    g = kr.skm_geom_ref(L, k)
    reads = _mixed_reads(L, k, k)
    ref = kr.skm_runs_ref(reads, k, g)
    want = pyref.count_reads(reads, k)
    zero = tuple([0] * W)
    bk, keys, rec = kr.skm_expand_ref(ref["records"], g)
    dk, dc = kr.count_keys_ref(keys)
    got = {tuple(int(x) for x in dk[:, i]): int(dc[i]) for i in range(dk.shape[1])}
    assert zero not in got
    assert got == {key: c for key, c in want.items() if key != zero}
    assert ref["key0"] == want.get(zero, 0)
    assert ref["key0_present"] == int(zero in want)
    assert ref["valid"] == sum(want.values())
    assert np.array_equal(kr.bucket_of_keys_ref(keys, g), bk)
    assert ref["records"].shape[1] == int(np.sum(-(-ref["run_len"] // g["nmax"])))
    assert np.all(ref["p_n"] >= 1) and np.all(ref["p_n"] <= g["nmax"])
    assert ref["run_len"].max() > g["nmax"], "the reads must hold a run that is split"
    # maximal: the window before a run's start and after its end is dead or of another bucket
    live, bucket = ref["live"], ref["bucket"]
    r, s, e = ref["run_read"], ref["run_start"], ref["run_start"] + ref["run_len"] - 1
    before = s > 0
    assert not np.any(live[r[before], s[before] - 1] & (bucket[r[before], s[before] - 1] == ref["run_bucket"][before]))
    after = e + 1 < live.shape[1]
    assert not np.any(live[r[after], e[after] + 1] & (bucket[r[after], e[after] + 1] == ref["run_bucket"][after]))
    for i in range(r.size):
        assert np.all(live[r[i], s[i]:e[i] + 1]) and np.all(bucket[r[i], s[i]:e[i] + 1] == ref["run_bucket"][i])
    assert int(ref["run_len"].sum()) == int(live.sum())


@pytest.mark.parametrize("k,W,m,masked", SKM_KS)
def test_skm_reference_records_round_trip(k, W, m, masked):
    """Build -> expand -> build: the vectorised builder agrees with the
    Python-integer statement of the layout, and the bases recovered from a
    record's keys rebuild the same record."""
    L = k + 21
    g = kr.skm_geom_ref(L, k)
    ref = kr.skm_runs_ref(_mixed_reads(L, k, k + 1), k, g)
    recs = ref["records"]
    bk, keys, rec = kr.skm_expand_ref(recs, g)
    first = np.flatnonzero(np.append(True, rec[1:] != rec[:-1]))
    Kp = g["Kp"]
    for i in range(0, recs.shape[1], 7):
        n, rd, ps = int(ref["p_n"][i]), int(ref["p_read"][i]), int(ref["p_start"][i])
        bases = ref["codes"][rd, ps:ps + Kp + n - 1]
        want = kr.skm_record_ref(bases, int(ref["p_bucket"][i]), n, g)
        assert [int(x) for x in recs[:, i]] == want
        # the record's bases again from its keys: key 0 whole, then the last base of every later key
        kk = keys[:, first[i]:first[i] + n]
        got = []
        for j in range(n):
            v = 0
            for w in range(W):
                v = (v << 64) | int(kk[w, j])
            b = [(v >> (2 * (32 * W - 1 - t))) & 3 for t in range(Kp)]
            got += b if j == 0 else b[-1:]
        assert kr.skm_record_ref(got, int(bk[first[i]]), n, g) == want


def test_skm_bucket_reference_does_not_depend_on_the_window_position():
    rng = np.random.default_rng(5)
    for k, W, m, masked in SKM_KS:
        win = rng.integers(0, 4, size=k).astype(np.uint8)
        want = kr.bucket_ref(win, 0, k, m)
        for off in (1, 7, 8, 16, 33):
            read = np.concatenate([rng.integers(0, 4, size=off), win, rng.integers(0, 4, size=9)]).astype(np.uint8)
            assert kr.bucket_ref(read, off, k, m) == want
            padded = np.concatenate([read, np.zeros(128, dtype=np.uint8)])[None, :]
            assert kr.window_buckets_ref(padded, read.size, k, m)[0, off] == want


def test_skm_hash_reference_regimes():
    """The three m-mer orders, on values with bits in every byte; the low 16
    bits of the two multiplicative regimes are a bijection of the low 16 bits."""
    mm = np.array([0, 1, 0x3fffff, 0xabcdef, 0x123456], dtype=U64)
    assert [int(x) for x in kr.mmer_hash_ref(mm, 11)] == [((int(v) ^ 0xd1e995) * 0x9e3779) & 0xffffffff for v in mm]
    assert [int(x) for x in kr.mmer_hash_ref(mm, 15)] == [((int(v) ^ 0x5bd1e995) * 0x9e3779b1) & 0xffffffff for v in mm]
    big = np.array([0x0000123456789abc, 0xffffffffffff, 1 << 32], dtype=U64)
    for v, h in zip(big, kr.mmer_hash_ref(big, 24)):
        x = (int(v) & 0xffffffff) ^ (((int(v) >> 32) * 0x9e3779b1) & 0xffffffff)
        assert int(h) == ((x ^ 0x5bd1e995) * 0x9e3779b1) & 0xffffffff
    low = np.arange(65536, dtype=U64)
    for m in (11, 15):
        assert np.unique(kr.mmer_hash_ref(low, m) & U64(0xffff)).size == 65536


def test_skm_variable_length_reference():
    """Reads shorter than k give nothing, a read of exactly k one window; the
    slot padding is no hole."""
    k = 21
    g = kr.skm_geom_ref(60, k)
    reads = ["ACGT" * 5, "ACGT" * 5 + "A", "", "A" * 30, "ACGTN" * 9, "ACGTTGCA" * 7]
    ref = kr.skm_runs_ref(reads, k, g, L=60)
    want = pyref.count_reads(reads, k)
    bk, keys, rec = kr.skm_expand_ref(ref["records"], g)
    dk, dc = kr.count_keys_ref(keys)
    assert {(int(a),): int(c) for a, c in zip(dk[0], dc)} == {key: c for key, c in want.items() if key != (0,)}
    assert ref["key0"] == want[(0,)] == 10 and ref["valid"] == sum(want.values())
    assert 1 in ref["p_read"] and 0 not in ref["p_read"] and 2 not in ref["p_read"]
    only_short = kr.skm_runs_ref(["ACGT" * 5, "ACGTTGCA" * 7], k, g, L=60)
    assert only_short["key0_present"] == 0


def test_skm_record_comparison_rejects_a_changed_record():
    g = kr.skm_geom_ref(60, 25)
    ref = kr.skm_runs_ref(skm_reads.genome_reads(60, 40, 3), 25, g)
    recs = ref["records"]
    kr.check_record_multiset("same", recs[:, ::-1], recs)
    for word, bit in ((0, 48), (0, 3), (1, 0), (1, 40)):
        bad = recs.copy()
        bad[word, 5] ^= U64(1) << U64(bit)
        with pytest.raises(AssertionError):
            kr.check_record_multiset("changed", bad, recs)
    with pytest.raises(AssertionError):
        kr.check_record_multiset("one fewer", recs[:, 1:], recs)
    grouped, starts = kr.group_records(recs, 65536)
    bk, _ = kr.record_fields(grouped)
    assert np.all(np.diff(bk) >= 0) and starts[0] == 0 and starts[-1] == recs.shape[1]
    assert np.array_equal(starts, kr.bucket_bounds_ref(grouped[0], 16))


# ---- key-prefix engine references (test_gpu_part_kernels.py) ----

def _ss(counts):
    """257 bounds of 256 sub-bucket sizes given as {sub-bucket: keys}."""
    c = np.zeros(256, dtype=np.int64)
    for s, n in counts.items():
        c[s] = n
    return np.concatenate([[0], np.cumsum(c)])


def test_p5_run_walk_reference_on_hand_written_bounds():
    per = 10
    # a run of exactly `per` keys stays one run; one more key in the next sub-bucket cuts it
    assert kr.p5_runs_ref(_ss({0: 4, 1: 6}), per) == [(0, 256, True)]
    assert kr.p5_runs_ref(_ss({0: 4, 1: 7}), per) == [(0, 1, True), (1, 256, True)]
    # with `<` instead of `<=` the first walk would cut after sub-bucket 0 as well
    lt = [(0, 1, True), (1, 256, True)]
    assert kr.p5_runs_ref(_ss({0: 4, 1: 6}), per) != lt
    # one sub-bucket above per is a run of its own and not multi; the walk goes on behind it
    assert kr.p5_runs_ref(_ss({3: 11, 4: 1}), per) == [(3, 4, False), (4, 256, True)]
    # an empty leading run (sub-buckets before an oversized one) is skipped; the last run ends at 256
    assert kr.p5_runs_ref(_ss({5: 11, 255: 2}), per) == [(5, 6, False), (6, 256, True)]
    assert kr.p5_runs_ref(_ss({0: 11}), per) == [(0, 1, False)]
    assert kr.p5_runs_ref(_ss({}), per) == []
    # the end is the last e within `per`, empty sub-buckets included
    assert kr.p5_runs_ref(_ss({0: 5, 9: 5, 10: 1}), per) == [(0, 10, True), (10, 256, True)]
    # starts need not begin at 0
    assert kr.p5_runs_ref(_ss({0: 4, 1: 7}) + 1000, per) == [(0, 1, True), (1, 256, True)]


def test_desc_fields_and_bucket_counts():
    ln, sh, srt = kr.desc_fields(np.array([5 | 36 << 24, 7 | 30 << 24 | 1 << 31, 1 | 1 << 30], dtype=np.uint32))
    assert ln.tolist() == [5, 7, 1] and sh.tolist() == [36, 30, 64] and srt.tolist() == [0, 1, 0]
    keys = np.array([[9, 3, 3, 7, 3, 9]], dtype=U64)
    dk, dc = kr.bucket_counts_ref(keys, 1, 6)
    assert dk.tolist() == [[3, 7, 9]] and dc.tolist() == [3, 1, 1]


def _segments_case():
    """Two buckets (1 and 2) of W = 2 keys; bucket 1 split in two passes at half its range."""
    rng = np.random.default_rng(3)
    b1 = (U64(1) << U64(48)) | rng.integers(0, 1 << 48, size=40, dtype=np.uint64)
    b2 = (U64(2) << U64(48)) | rng.integers(0, 1 << 48, size=10, dtype=np.uint64)
    w0 = np.concatenate([b1, b1[:5], b2])  # five repeats
    keys = np.stack([w0, w0 ^ U64(0x55)])
    ranges = [(0, 45, 1 << 48, 2 << 48), (45, 55, 2 << 48, 3 << 48)]
    dk, dc = kr.count_keys_ref(keys)
    half = (1 << 48) | (1 << 47)
    lo = dk[0] < U64(half)
    b1m = dk[0] < U64(2 << 48)
    parts = [np.flatnonzero(b1m & ~lo), np.flatnonzero(~b1m), np.flatnonzero(b1m & lo)]  # records in this order
    rng.shuffle(parts[0])
    order = np.concatenate(parts)
    rk = np.full((2, 64), U64(0xEEEEEEEEEEEEEEEE))
    rc = np.full(64, 0xEEEEEEEE, dtype=np.uint32)
    rk[:, :order.size] = dk[:, order]
    rc[:order.size] = dc[order]
    st = np.cumsum([0] + [p.size for p in parts])
    desc_key = np.full(4, U64(0xEEEEEEEEEEEEEEEE))
    desc_start = np.full(4, U64(0xEEEEEEEEEEEEEEEE))
    desc_len = np.full(4, 0xEEEEEEEE, dtype=np.uint32)
    desc_key[:3] = [half, 2 << 48, 1 << 48]
    desc_start[:3] = st[:3]
    desc_len[:3] = [parts[0].size | 35 << 24, parts[1].size | 36 << 24 | 1 << 31, parts[2].size | 35 << 24]
    return keys, ranges, rk, rc, int(order.size), [desc_key, desc_start, desc_len]


def test_check_segments_accepts_the_contract_and_rejects_each_breach():
    keys, ranges, rk, rc, cur, desc = _segments_case()
    segs = kr.check_segments("ok", keys, ranges, rk, rc, cur, desc, 3, 0xEE)
    assert [(s[0], s[4], s[5]) for s in segs] == [(0, 35, 0), (0, 35, 0), (1, 36, 1)]

    def broken(**kw):
        k2, r2, rk2, rc2, c2, d2 = _segments_case()
        d2 = [x.copy() for x in d2]
        fill_n = 3
        if "shift" in kw:  # one too large a span for 4096 bins
            d2[2][0] = (int(d2[2][0]) & 0x80ffffff) | kw["shift"] << 24
        if "count" in kw:
            rc2[0] += 1
        if "swap" in kw:  # a record of the upper half into the lower half's segment
            a, b = int(d2[1][0]), int(d2[1][2])
            rk2[:, [a, b]] = rk2[:, [b, a]]
            rc2[[a, b]] = rc2[[b, a]]
        if "unsorted" in kw:  # inside the segment flagged sorted
            a = int(d2[1][1])
            rk2[:, [a, a + 1]] = rk2[:, [a + 1, a]]
            rc2[[a, a + 1]] = rc2[[a + 1, a]]
        if "gap" in kw:
            d2[1][0] += U64(1)
        if "fewer" in kw:
            fill_n = 2
        if "dup" in kw:  # a key in two records, the total right
            a = int(np.flatnonzero(rc2[:c2] == 2)[0])
            rc2[a] = 1
            rk2[:, c2] = rk2[:, a]
            rc2[c2] = 1
            last = int(np.argmax(d2[1][:3]))
            d2[2][last] += 1
            c2 += 1
        with pytest.raises(AssertionError):
            kr.check_segments("broken", k2, r2, rk2, rc2, c2, d2, fill_n, 0xEE)

    broken(shift=34)
    broken(count=1)
    broken(swap=1)
    broken(unsorted=1)
    broken(gap=1)
    broken(fewer=1)
    broken(dup=1)
    # a key missing from the records is accepted only when the fallback holds it
    k2, r2, rk2, rc2, c2, d2 = _segments_case()
    last = int(np.argmax(d2[1][:3]))
    gone_k, gone_c = rk2[:, c2 - 1:c2].copy(), rc2[c2 - 1:c2].astype(np.int64)
    d2[2][last] -= 1
    with pytest.raises(AssertionError):
        kr.check_segments("missing", k2, r2, rk2, rc2, c2 - 1, d2, 3, 0xEE)
    kr.check_segments("in the fallback", k2, r2, rk2, rc2, c2 - 1, d2, 3, 0xEE, extra=(gone_k, gone_c))


def test_table_entries_reads_what_make_table_wrote():
    for W in (1, 2, 4):
        keys = np.zeros((W, 6), dtype=U64)
        keys[:, 1] = 7
        keys[:, 4] = 9
        t = kr.make_table(W, keys, [0, 3, 0, 0, 5, 0], [0, 2, 0, 0, 2, 0])
        k, c = kr.table_entries(W, t)
        assert k.tolist() == [[7, 9]] * W and c.tolist() == [3, 5]


PART_LK = [(100, 21), (150, 31), (150, 55), (101, 100), (90, 29)]


@pytest.mark.parametrize("L,k", PART_LK)
def test_part_front_reference_is_the_python_statement(L, k):
    """Window keys, the statistics and the histogram against kmer_ref_py: the
    emitted keys are the counted k-mers minus key 0^W; every key lands in the
    (digit, segment) cell of its read."""
    W = (k + 31) // 32
    reads = (skm_reads.special_reads(L, 12, k) + skm_reads.edge_reads(L, k, k) + ["N" * L, "A" * L] +
             skm_reads.genome_reads(L, 10, k, genome=200))
    R, seg_tiles = 4, 3
    ref = kr.part_front_ref(reads, k, R, seg_tiles, 48)
    want = pyref.count_reads(reads, k)
    zero = tuple([0] * W)
    dk, dc = kr.count_keys_ref(ref["keys"])
    got = {tuple(int(x) for x in dk[:, i]): int(dc[i]) for i in range(dk.shape[1])}
    assert got == {key: c for key, c in want.items() if key != zero}
    assert ref["key0"] == want.get(zero, 0) > 0 and ref["key0_present"] == 1
    assert ref["valid"] == sum(want.values())
    assert ref["nseg"] == -(-len(reads) // (R * seg_tiles)) and int(ref["hist"].sum()) == ref["keys"].shape[1]
    # per read, directly: read r's keys are in segment r // (R * seg_tiles)
    for r in (0, len(reads) // 2, len(reads) - 1):
        mine = pyref.count_reads([reads[r]], k)
        sel = ref["keys"][:, ref["seg"] == r // (R * seg_tiles)]
        have = {tuple(int(x) for x in sel[:, i]) for i in range(sel.shape[1])}
        assert {key for key, c in mine.items() if key != zero and c > 0} <= have
    dig, inr = kr.part_digits_ref(ref["keys"][0], 48)
    assert np.array_equal(dig, ref["dig"]) and inr.all()
    assert np.array_equal(dig, (ref["keys"][0] >> U64(48)).astype(np.int64) & 255)
    # the range filter keeps exactly the keys whose top byte is inside
    part = kr.part_front_ref(reads, k, R, seg_tiles, 48, 64, 160)
    top = (ref["keys"][0] >> U64(56)).astype(np.int64)
    kr.check_record_multiset("filtered", part["keys"], ref["keys"][:, (top >= 64) & (top < 160)])
    assert (part["valid"], part["key0"]) == (ref["valid"], ref["key0"])
    # slices: each holds the keys of its (digit, segment) cell, and they cover every key
    base = np.zeros((256, ref["nseg"]), dtype=np.int64)
    flat = ref["hist"].reshape(-1)
    base.reshape(-1)[1:] = np.cumsum(flat)[:-1]
    sl = kr.part_slices_ref(ref, base)
    assert sum(s[3].shape[1] for s in sl) == ref["keys"].shape[1]
    for d, sg, start, ks in sl:
        assert ks.shape[1] == ref["hist"][d, sg] and start == base[d, sg]
        assert np.all(((ks[0] >> U64(48)) & U64(255)) == U64(d))
