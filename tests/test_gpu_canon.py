"""kc_canonicalize on the GPU: the finished run folded by reverse complement,
through Context.canonicalize and the CLI's canonical=1. Every expected value
comes from tests/canon_ref.py: fold_records over the bytes that were installed
and count_canonical over the read strings (tests/test_canon_host.py pins the
two to each other and to the CPU oracle).

Sizes: the fold's passes work in tiles of 1024 records, so crafted runs of
1023, 1024 and 1025 records sit on both sides of a tile edge; 65537 records are
65 tiles, more than one per workgroup's first round on a small grid, and put
the flipped part through several radix passes and the merge through many tiles."""
import os
import subprocess

import numpy as np
import pytest

import canon_ref

pytestmark = pytest.mark.gpu

STATE = 6
NS = [0, 1, 2, 1023, 1024, 1025, 65537]
L = 150


def rec_dtype(W):
    return np.dtype([("key", "<u8", (W,)), ("cnt", "<u4")])


def install(ctx, data):
    """The hand-built records become the context's finished run."""
    import torch

    n = len(data) // ctx.rs
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8) if data else torch.empty(0, dtype=torch.uint8)
    assert ctx.merge_records(src, n) == n
    assert ctx.records() == data


def finished_ctx(kca, k):
    ctx = kca.Context(kmer_length=k, line_length=L)
    ctx.count_fastq(kca.synth_fastq(10, L, seed=1))
    ctx.finish()
    return ctx


def fold_and_check(ctx, data, k, what):
    want = canon_ref.fold_records(data, k)
    install(ctx, data)
    for again in (False, True):  # idempotent: the same n and the same bytes
        assert ctx.canonicalize() * ctx.rs == len(want), (what, again)
        assert ctx.finish() * ctx.rs == len(want)
        assert ctx.records() == want, (what, again)
        assert ctx.stats()["output_records"] * ctx.rs == len(want)
    return want


@pytest.mark.parametrize("k", [1, 31, 32, 33, 55, 63, 64, 100, 128])
def test_crafted_runs(kca, k):
    """x with rc(x) (counts U32_MAX + 2 wrap to 1), palindromes at even k,
    records that differ only behind base k, the hole record with and without
    T^k: canon_ref.crafted's mixed runs at every size."""
    with finished_ctx(kca, k) as ctx:
        for i, n in enumerate(NS):
            hole, tk = bool(i & 1), bool(i & 2)
            data = canon_ref.crafted(k, n, seed=k * 7 + n, kind="mixed", hole=hole, tk=tk)
            want = fold_and_check(ctx, data, k, (n, hole, tk))
            if n >= 1023:
                assert len(want) < len(data)  # keys met
                if k > 1:  # (k = 1 has two canonical keys: everything sums into them)
                    assert 1 in np.frombuffer(want, dtype=rec_dtype(ctx.W))["cnt"]  # U32_MAX + 2
            if n >= 2 and (hole or tk):
                first = np.frombuffer(want, dtype=rec_dtype(ctx.W))[0]
                assert not first["key"].any() and first["cnt"] == (5 if tk else 0)


@pytest.mark.parametrize("k", [31, 64, 100])
@pytest.mark.parametrize("kind", ["stay", "flip"])
def test_one_sided_runs(kca, k, kind):
    """All records stay (no flipped run: the staying run alone, summed where
    cleared keys meet) or all flip (no staying run: the sorted flipped run is
    the result)."""
    with finished_ctx(kca, k) as ctx:
        for n in (1, 2, 1025, 5000):
            for hole, tk in ((False, False), (kind == "stay", kind == "flip")):
                fold_and_check(ctx, canon_ref.crafted(k, n, seed=k + n, kind=kind, hole=hole, tk=tk), k,
                               (n, kind, hole, tk))


_WANT = {}


def canonical_count(kca, k):
    if k not in _WANT:
        _WANT[k] = canon_ref.count_canonical(canon_ref.stranded_input(kca)[1], k)
    return _WANT[k]


@pytest.mark.parametrize("engine", ["auto", "table", "partition", "skm"])
@pytest.mark.parametrize("k", [21, 31, 55, 100])
def test_end_to_end(kca, k, engine):
    fq, _ = canon_ref.stranded_input(kca)
    want = canonical_count(kca, k)
    with kca.Context(kmer_length=k, line_length=L, engine=engine) as ctx:
        ctx.count_fastq(fq)
        plain = ctx.finish()
        n = ctx.canonicalize()
        assert n * ctx.rs == len(want) and n < plain
        assert ctx.records() == want
        assert ctx.canonicalize() == n and ctx.records() == want  # idempotent
        # the queries see the folded run
        r = np.frombuffer(want, dtype=rec_dtype(ctx.W))
        assert sum(ctx.histogram(256)) == n
        assert ctx.histogram(4) == np.bincount(np.minimum(r["cnt"], 3), minlength=4).tolist()
        keys = np.ascontiguousarray(r["key"])
        counts, found = ctx.lookup(keys)
        assert found.all() and np.array_equal(counts, r["cnt"])
        # the other strand of a non-palindrome is not a key of the folded run
        kmers = [canon_ref.key_to_bases(w)[:k] for w in keys.tolist()]
        other = [canon_ref.revcomp(s) for s in kmers if s != canon_ref.revcomp(s)]
        assert len(other) > 1000
        okeys = np.array([canon_ref.bases_to_key(s, ctx.W) for s in other], dtype=np.uint64)
        counts, found = ctx.lookup(np.ascontiguousarray(okeys))
        assert not found.any() and not counts.any()
        # a new count on the same context is not disturbed by the swapped run buffers
        ctx.reset()
        ctx.count_fastq(fq)
        assert ctx.finish() == plain
        assert ctx.canonicalize() == n and ctx.records() == want


SPILL_K = 31


def spilling_count(kca):
    """(fastq, canonical count at SPILL_K) of canon_ref.paired_input: about
    180 000 canonical keys, 4 MB of strand-wise records, far beyond a 1 MB
    gpu_memory_limit."""
    fq, reads = canon_ref.paired_input(kca)
    if "paired" not in _WANT:
        _WANT["paired"] = canon_ref.count_canonical(reads, SPILL_K)
    return fq, _WANT["paired"]


def test_state_rules(kca):
    with kca.Context(kmer_length=31, line_length=L) as ctx:
        ctx.count_fastq(kca.synth_fastq(100, L, seed=2))
        with pytest.raises(kca.KcError) as e:
            ctx.canonicalize()
        assert e.value.status == STATE and "kc_finish" in str(e.value)
        ctx.finish()
        assert ctx.canonicalize() > 0


def test_host_spill_runs_refuse(kca, monkeypatch, tmp_path):
    """Host spill runs (KC_HOST_RUNS sends them there as when HBM is short):
    the device fold refuses, the file form over the written output is the route."""
    monkeypatch.setenv("KC_HOST_RUNS", "1")
    fq, want = spilling_count(kca)
    with kca.Context(kmer_length=SPILL_K, line_length=L, gpu_memory_limit=1 << 20, engine="partition",
                     lds_slots=1) as ctx:
        ctx.count_fastq(fq)
        ctx.finish()
        assert ctx.stats()["spill_runs"] >= 2
        with pytest.raises(kca.KcError) as e:
            ctx.canonicalize()
        assert e.value.status == STATE
        out = tmp_path / "spilled.bin"
        out.write_bytes(ctx.output_bytes(str(tmp_path)))
    assert kca.canonicalize_file(str(out), str(out), SPILL_K) * 12 == len(want)
    assert out.read_bytes() == want


@pytest.mark.parametrize("k", [31, 55])
def test_two_contexts_fold_then_exchange_or_gather(kca, k):
    """The fold is linear: each context folds its half of the reads, then the
    exchange (runs concatenated) and the gather (context 0) both give the
    single-context result."""
    fq, reads = canon_ref.stranded_input(kca)
    want = canonical_count(kca, k)
    lines = fq.decode().split("\n")
    half = 4 * (len(reads) // 2)
    parts = ["\n".join(lines[:half]) + "\n", "\n".join(lines[half:])]
    for route in ("exchange", "gather"):
        ctxs = [kca.Context(kmer_length=k, line_length=L) for _ in parts]
        try:
            for c, text in zip(ctxs, parts):
                c.count_fastq(text.encode())
                c.finish()
                c.canonicalize()
            if route == "exchange":
                kca.exchange_contexts(ctxs)
                got = b"".join(c.records() for c in ctxs)
                assert all(c.finish() > 0 for c in ctxs)
            else:
                kca.gather_contexts(ctxs)
                got = ctxs[0].records()
            assert got == want, route
        finally:
            for c in ctxs:
                c.close()


def _parse_histo(path):
    return {int(a): int(b) for a, b in (line.split() for line in path.read_text().splitlines())}


@pytest.mark.parametrize("config", [["gpus=1"], ["gpus=2"], ["gpus=2", "exchange=alltoall"],
                                    ["gpus=1", "gpuMemoryLimit=1000000"], ["gpus=2", "gpuMemoryLimit=1000000"]],
                         ids=["one", "gather", "alltoall", "spill", "spill2"])
def test_cli_canonical(kca, orc, tmp_path, monkeypatch, request, config):
    """Device route (every context folds its run before the gather or the
    exchange) and file route (host spill runs, forced by KC_HOST_RUNS in the
    spill cases: the written output is folded in place) write the same bytes."""
    if request.node.callspec.id.startswith("spill"):
        monkeypatch.setenv("KC_HOST_RUNS", "1")
        k, W = SPILL_K, 1
        fq, want = spilling_count(kca)
    else:
        k, W = 55, 2
        fq, _ = canon_ref.stranded_input(kca)
        want = canonical_count(kca, k)
    r = np.frombuffer(want, dtype=rec_dtype(W))
    d = tmp_path / "in"
    d.mkdir()
    (d / "a.fastq").write_bytes(fq)
    cli = os.path.join(os.path.dirname(kca.LIB_PATH), "kmer-counter")
    base = [cli, f"kmerLength={k}", f"inputFileLocation={d}", f"tempFileLocation={tmp_path}", "quiet=1"] + config
    out, hist = tmp_path / "canon.bin", tmp_path / "canon.histo"
    subprocess.run(base + [f"outputFile={out}", "canonical=1", f"histogramFile={hist}"], check=True,
                   capture_output=True, timeout=300)
    assert out.read_bytes() == want
    # the histogram of the folded run
    bins = np.bincount(np.minimum(r["cnt"].astype(np.int64), 10000), minlength=10001)
    assert _parse_histo(hist) == {i: int(v) for i, v in enumerate(bins) if v}
    # the filter works on folded counts
    lo = int(r["cnt"].max())
    kept = r[r["cnt"] >= lo]
    assert 0 < len(kept) < len(r)
    subprocess.run(base + [f"outputFile={out}", "canonical=1", f"minCount={lo}"], check=True, capture_output=True,
                   timeout=300)
    assert out.read_bytes() == kept.tobytes()
    # canonical=0 and no key at all: today's bytes
    plain = orc.count_fastq(fq, k)
    for extra in (["canonical=0"], []):
        subprocess.run(base + [f"outputFile={out}"] + extra, check=True, capture_output=True, timeout=300)
        assert out.read_bytes() == plain
    assert not [x.name for x in tmp_path.iterdir() if "kccanon" in x.name]  # the file fold's temp name
