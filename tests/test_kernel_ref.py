"""The checker of the kernel-level tests, checked on the CPU: kernel_ref's
references against numpy's own sorts, and every comparison helper against a
corruption it must reject (a checker that canonicalises too much would let a
wrong kernel pass)."""
import numpy as np
import pytest

import kernel_ref as kr

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
