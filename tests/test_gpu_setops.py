"""Set operations between two finished runs on the GPU, through the Python
API: Context.combine with a Context and with a tensor, and what every later
call sees afterwards. Every expected value comes from setops_ref over
hand-built records or over the CPU oracle's bytes."""
import functools

import numpy as np
import pytest

import setops_ref as sr
from setops_ref import CASES, COUNT_SUBTRACT, INTERSECT, LEFT, MIN, SUBTRACT, SUM, U32, UNION

pytestmark = pytest.mark.gpu

STATE = 6
FAMILIES = [(UNION, sr.MAX), (INTERSECT, MIN), (SUBTRACT, SUM), (COUNT_SUBTRACT, SUM)]


def np_hist(cnt, n_bins):
    return np.bincount(np.minimum(cnt.astype(np.int64), n_bins - 1), minlength=n_bins).tolist()


def tensor_of(r):
    import torch

    data = r.tobytes()
    return torch.frombuffer(bytearray(data), dtype=torch.uint8) if data else torch.empty(0, dtype=torch.uint8)


def install(ctx, r):
    """The hand-built records become the context's finished run."""
    assert ctx.merge_records(tensor_of(r), len(r)) == len(r)
    assert ctx.records() == r.tobytes()


def finished_ctx(kca, k):
    ctx = kca.Context(kmer_length=k, line_length=120)
    ctx.count_fastq(kca.synth_fastq(10, 120, seed=1))
    ctx.finish()
    return ctx


def check_after(ctx, want, W):
    """Every later call sees the result."""
    n = len(want)
    assert ctx.records() == want.tobytes()
    assert ctx.finish() == n
    assert ctx.stats()["output_records"] == n
    assert ctx.histogram(256) == np_hist(want["cnt"], 256)
    if n:
        counts, found = ctx.lookup(np.ascontiguousarray(want["key"]))
        assert found.all() and np.array_equal(counts, want["cnt"])
    absent = np.full((1, W), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    counts, found = ctx.lookup(absent)
    assert not found[0] and counts[0] == 0


@pytest.mark.parametrize("k", [31, 55, 100])
def test_every_op_and_mode(kca, k):
    W = (k + 31) // 32
    a, b = sr.split_runs(W, 5000 + k, seed=k, hole=(True, True))
    tb = tensor_of(b).cuda()
    with finished_ctx(kca, k) as ca, finished_ctx(kca, k) as cb:
        install(cb, b)
        for op, mode in CASES if k != 100 else FAMILIES:
            want = sr.combine_vec(a, b, op, mode)
            assert 0 < len(want) < len(a) + len(b)
            install(ca, a)
            assert ca.combine(cb, op, mode) == len(want), (op, mode)
            check_after(ca, want, W)
            assert cb.records() == b.tobytes()  # B is never modified
            install(ca, a)
            assert ca.combine(tb, sr.OP_NAMES[op], sr.MODE_NAMES[mode], n_records=len(b)) == len(want)
            check_after(ca, want, W)
        # a raw device pointer, and a host tensor (staged to the device)
        install(ca, a)
        assert ca.combine(tb.data_ptr(), "intersect", "min", n_records=len(b)) == len(sr.combine_vec(a, b, 1, 1))
        install(ca, a)
        assert ca.combine(tensor_of(b), kca.KC_SET_UNION, kca.KC_SETC_RIGHT, n_records=len(b))
        assert ca.records() == sr.combine_vec(a, b, UNION, sr.RIGHT).tobytes()
        assert np.frombuffer(tb.cpu().numpy().tobytes(), dtype=b.dtype).tobytes() == b.tobytes()


@pytest.mark.parametrize("k", [31, 55, 100])
def test_identities(kca, k):
    import torch

    W = (k + 31) // 32
    a, b = sr.split_runs(W, 7001, seed=3 * k, hole=(True, False))
    e = a[:0]
    with finished_ctx(kca, k) as ca, finished_ctx(kca, k) as cb:
        # UNION / SUM gives the bytes of the summing merge of the same two runs
        install(ca, a)
        n = ca.combine(tensor_of(b), "union", "sum", n_records=len(b))
        both = torch.cat([tensor_of(a), tensor_of(b)])
        assert cb.merge_runs(both, [len(a), len(b)]) == n
        assert ca.records() == cb.records() == sr.combine_vec(a, b, UNION, SUM).tobytes()
        # a run with a copy of itself
        install(ca, a)
        install(cb, a)
        assert ca.combine(cb, "intersect", "left") == len(a)
        assert ca.records() == a.tobytes()
        assert ca.combine(cb, "subtract") == 0
        check_after(ca, e, W)
        # an empty operand: the result is A, B or nothing, with no launch
        assert ca.combine(cb, "intersect", "max") == 0 and ca.records() == b""
        assert ca.combine(cb, "count_subtract") == 0 and ca.records() == b""
        assert ca.combine(cb, "union", "min") == len(a)  # UNION with an empty A is B
        check_after(ca, a, W)
        install(cb, e)
        assert ca.combine(cb, "count_subtract") == len(a)  # COUNT_SUBTRACT with an empty B is A
        assert ca.combine(cb, "subtract") == len(a) and ca.combine(cb, "union", "right") == len(a)
        assert ca.combine(tensor_of(e), "union", n_records=0) == len(a)
        assert ca.combine(0, "subtract", n_records=0) == len(a)
        check_after(ca, a, W)
        assert ca.combine(cb, "intersect") == 0
        check_after(ca, e, W)
        assert ca.combine(cb, "union") == 0 and ca.records() == b""  # both empty


@functools.lru_cache(maxsize=None)
def counts_of(k):
    """FASTQ text and the CPU oracle's count of reads [0, 2000) and
    [2000, 4000) of one synthetic genome."""
    import oracle
    from conftest import load_pkg

    kca = load_pkg()
    fq = [kca.synth_fastq(2000, 80, 77, genome_length=300000, n_rate=0.002, first_read=f) for f in (0, 2000)]
    return fq, [oracle.count_fastq(f, k) for f in fq]


@pytest.mark.parametrize("k", [31, 55])
def test_two_counts_of_one_genome(kca, orc, k):
    W = (k + 31) // 32
    fq, want = counts_of(k)
    a, b = (np.frombuffer(w, dtype=sr.rec_dtype(W)) for w in want)
    shared = len(sr.combine_vec(a, b, INTERSECT, MIN))
    assert 1000 < shared < min(len(a), len(b)) - 1000
    with kca.Context(kmer_length=k, line_length=80) as ca, kca.Context(kmer_length=k, line_length=80) as cb:
        cb.count_fastq(fq[1])
        assert cb.records() == want[1]
        for op, mode in [(INTERSECT, MIN), (SUBTRACT, SUM), (COUNT_SUBTRACT, SUM)]:
            ca.reset()
            ca.count_fastq(fq[0])
            assert ca.finish() == len(a)
            ref = sr.combine_vec(a, b, op, mode)
            assert ca.combine(cb, op, mode) == len(ref), (op, mode)
            check_after(ca, ref, W)
        assert cb.records() == want[1]


def test_fold_both_runs_then_combine(kca, orc):
    """The documented order for k-mer-only identity: canonicalize() both, then
    combine. k = 31: the keys carry a read base after the k-mer until folded."""
    import canon_ref

    k, W = 31, 1
    fq, want = counts_of(k)
    fa, fb = (np.frombuffer(canon_ref.fold_records(w, k), dtype=sr.rec_dtype(W)) for w in want)
    with kca.Context(kmer_length=k, line_length=80) as ca, kca.Context(kmer_length=k, line_length=80) as cb:
        ca.count_fastq(fq[0])
        cb.count_fastq(fq[1])
        assert ca.records() == want[0] and cb.records() == want[1]
        assert ca.canonicalize() == len(fa) and cb.canonicalize() == len(fb)
        ref = sr.combine_vec(fa, fb, INTERSECT, MIN)
        assert 0 < len(ref) < min(len(fa), len(fb))
        assert ca.combine(cb, "intersect", "min") == len(ref)
        check_after(ca, ref, W)
        # unfolded, fewer keys meet: records of one k-mer that differ in the trailing base stay apart
        unfolded = sr.combine_vec(*(np.frombuffer(w, dtype=sr.rec_dtype(W)) for w in want), INTERSECT, MIN)
        assert int(unfolded["cnt"].astype(np.uint64).sum()) <= int(ref["cnt"].astype(np.uint64).sum())


def test_chain_combine_filter_write(kca, orc, tmp_path):
    k = 55
    fq, want = counts_of(k)
    pa, pb, out, fout = tmp_path / "a.bin", tmp_path / "b.bin", tmp_path / "dev.bin", tmp_path / "file.bin"
    with kca.Context(kmer_length=k, line_length=80) as ca, kca.Context(kmer_length=k, line_length=80) as cb:
        ca.count_fastq(fq[0])
        cb.count_fastq(fq[1])
        ca.write_output(str(pa))
        cb.write_output(str(pb))
        assert pa.read_bytes() == want[0] and pb.read_bytes() == want[1]
        n = ca.combine(cb, "union", "sum")
        kept = ca.filter(2, 3)
        ca.write_output(str(out))
    assert kca.combine_files(str(pa), str(pb), str(fout), k, "union", "sum") == n
    assert kca.filter_file(str(fout), str(fout), k, 2, 3) == kept
    assert 0 < kept < n
    assert out.read_bytes() == fout.read_bytes()


def test_state_and_argument_rules(kca, orc, monkeypatch):
    k, L, W = 31, 150, 1
    b = sr.split_runs(W, 300, seed=4)[1]
    tb = tensor_of(b)
    fq = kca.synth_fastq(100, L, seed=2)
    want = orc.count_fastq(fq, k)
    with finished_ctx(kca, k) as cb, kca.Context(kmer_length=k, line_length=L) as ca:
        install(cb, b)
        ca.count_fastq(fq)
        for call in (lambda: ca.combine(cb, "union"), lambda: ca.combine(tb, "union", n_records=len(b)),
                     lambda: cb.combine(ca, "union")):  # A unfinished, B unfinished
            with pytest.raises(kca.KcError) as e:
                call()
            assert e.value.status == STATE and "kc_finish" in str(e.value)
        assert cb.records() == b.tobytes()
        assert ca.records() == want  # finishes
        with finished_ctx(kca, 55) as c55:
            calls = [lambda: ca.combine(ca, "union"), lambda: ca.combine(c55, "union"), lambda: ca.combine(cb, 4),
                     lambda: ca.combine(cb, "union", 5), lambda: ca.combine(cb, "subtract", "min"),
                     lambda: ca.combine(cb, "count_subtract", "left"), lambda: ca.combine(cb, "xor"),
                     lambda: ca.combine(cb, "union", "avg"), lambda: ca.combine(tb, 7, n_records=len(b)),
                     lambda: ca.combine(tb, "intersect", 9, n_records=len(b)),
                     lambda: ca.combine(tb, "subtract", "max", n_records=len(b))]
            for i, call in enumerate(calls):
                with pytest.raises(kca.KcError) as e:
                    call()
                assert e.value.status == kca.KC_ERR_ARG, i
                assert ca.records() == want and ca.finish() * (8 * W + 4) == len(want)
        assert cb.records() == b.tobytes()
    # host spill runs (KC_HOST_RUNS sends the cut runs to the host, as when HBM
    # is short): refused as A and as B, the file form is the route
    monkeypatch.setenv("KC_HOST_RUNS", "1")
    big = kca.synth_fastq(20000, L, seed=k, n_rate=0.001)
    with kca.Context(kmer_length=k, line_length=L, gpu_memory_limit=1 << 20, engine="partition",
                     lds_slots=1) as cs, finished_ctx(kca, k) as cb:
        install(cb, b)
        cs.count_fastq(big)
        cs.finish()
        assert cs.stats()["spill_runs"] >= 2
        for call in (lambda: cs.combine(cb, "union"), lambda: cs.combine(tb, "subtract", n_records=len(b)),
                     lambda: cb.combine(cs, "intersect")):
            with pytest.raises(kca.KcError) as e:
                call()
            assert e.value.status == STATE
        assert cb.records() == b.tobytes()


def test_second_operand_on_another_device(kca):
    if kca.lib().kc_device_count() < 2:
        pytest.skip("one device")
    k, W = 55, 2
    a, b = sr.split_runs(W, 6000, seed=12, hole=(True, True))
    with kca.Context(kmer_length=k, line_length=120, device=0) as ca, \
            kca.Context(kmer_length=k, line_length=120, device=1) as cb:
        for c in (ca, cb):
            c.count_fastq(kca.synth_fastq(10, 120, seed=1))
            c.finish()
        install(ca, a)
        install(cb, b)
        want = sr.combine_vec(a, b, INTERSECT, LEFT)
        assert ca.combine(cb, "intersect", "left") == len(want)
        check_after(ca, want, W)
        assert cb.records() == b.tobytes()
