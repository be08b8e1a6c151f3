"""Queries on the finished run, on the GPU: kc_count_histogram,
kc_filter_records, kc_lookup / kc_lookup_device and the CLI keys built on them
(minCount=, maxCount=, histogramFile=, histogramBins=). Every expected value
comes from numpy over hand-built records or over the CPU oracle's bytes.

Sizes: the filter works in tiles of T = 1024 records and the histogram fills
its LDS table once per span of S = 16384 records; bins from 4096 up go to
global atomics. SIZES holds 0, 1, 2 and every power of two from 64 to 65536
with its +-1 neighbours, so T-1/T/T+1 = 1023/1024/1025 (and 2T, 4T, ...) and
S-1/S/S+1 = 16383/16384/16385 (and 2S, 4S) are all in it."""
import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32_MAX = 0xFFFFFFFF
SIZES = [0, 1, 2] + [p + d for e in range(6, 17) for p in [1 << e] for d in (-1, 0, 1)]
HIST_BINS = [2, 3, 256, 4096, 4097, 10001, 65536]
STATE = 6


def rec_dtype(W):
    return np.dtype([("key", "<u8", (W,)), ("cnt", "<u4")])


def np_hist(cnt, n_bins):
    return np.bincount(np.minimum(cnt.astype(np.int64), n_bins - 1), minlength=n_bins).tolist()


def mask(r, lo, hi):
    return r[(r["cnt"] >= lo) & (r["cnt"] <= hi)]


def crafted(W, n, seed):
    """n sorted records with distinct keys. Leading words come from {0, 1, 2},
    so many records share words 0..W-2 and differ only in the last word; last
    words are even and >= 2 (a present key +-1 in the last word is absent, and
    so is anything below the first record). Odd n: record 0 is the 0^W hole
    record with count 0. Counts sit around every histogram edge."""
    rng = np.random.default_rng(seed)
    r = np.zeros(n, dtype=rec_dtype(W))
    if n == 0:
        return r
    key = np.zeros((n, W), dtype=np.uint64)
    for j in range(W - 1):
        key[:, j] = rng.integers(0, 3, n, dtype=np.uint64)
    key[:, W - 1] = 2 * rng.choice(1 << 20, n, replace=False).astype(np.uint64) + 2
    order = np.lexsort([key[:, j] for j in range(W - 1, -1, -1)])
    r["key"] = key[order]
    pool = np.array([0, 1, 1, 1, 1, 2, 2, 3, 4, 5, 6, 7, 254, 255, 256, 257, 4094, 4095, 4096, 4097, 4098, 9999,
                     10000, 10001, 65534, 65535, 65536, U32_MAX - 1, U32_MAX], dtype=np.uint32)
    r["cnt"] = pool[rng.integers(0, len(pool), n)]
    if n % 2 == 1:
        r["key"][0] = 0
        r["cnt"][0] = 0
    return r


def install(ctx, r):
    """The hand-built records become the context's finished run."""
    import torch

    data = r.tobytes()
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8) if data else torch.empty(0, dtype=torch.uint8)
    assert ctx.merge_records(src, len(r)) == len(r)
    assert ctx.records() == data


def finished_ctx(kca, k):
    ctx = kca.Context(kmer_length=k, line_length=120)
    ctx.count_fastq(kca.synth_fastq(10, 120, seed=1))
    ctx.finish()
    return ctx


def check_lookup(ctx, r, W, seed):
    """Looks up every key of the run r (shuffled, some twice) and keys that
    are absent by construction; returns (keys, counts, found)."""
    rng = np.random.default_rng(seed)
    n = len(r)
    parts = []  # (keys, expected counts, expected found)

    def absent(keys):
        parts.append((keys, np.zeros(len(keys), dtype=np.uint32), np.zeros(len(keys), dtype=bool)))

    if n:
        idx = np.concatenate([rng.permutation(n), rng.integers(0, n, min(n, 64))])
        parts.append((r["key"][idx], r["cnt"][idx], np.ones(len(idx), dtype=bool)))
        near = r["key"][rng.integers(0, n, min(n, 512))].copy()
        near = near[near[:, W - 1] >= 2]  # not the hole record
        up, down = near.copy(), near.copy()
        up[:, W - 1] += np.uint64(1)  # last words are even: odd ones are absent
        down[:, W - 1] -= np.uint64(1)
        absent(up)
        absent(down)
        first = r["key"][:1].copy()
        if first[0, W - 1] >= 2:
            first[0, W - 1] -= np.uint64(1)  # below the first record
            absent(first)
    absent(np.full((1, W), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
    zero = np.zeros((1, W), dtype=np.uint64)
    if n and not r["key"][0].any():  # the hole record: present, with count 0
        assert r["cnt"][0] == 0
        parts.append((zero, np.zeros(1, dtype=np.uint32), np.ones(1, dtype=bool)))
    else:
        absent(zero)
    keys = np.ascontiguousarray(np.concatenate([p[0] for p in parts]))
    counts, found = ctx.lookup(keys)
    assert counts.dtype == np.uint32 and found.dtype == bool
    assert np.array_equal(found, np.concatenate([p[2] for p in parts]))
    assert np.array_equal(counts, np.concatenate([p[1] for p in parts]))
    return keys, counts, found


@pytest.mark.parametrize("k", [31, 55, 100])
def test_crafted_runs_of_exact_size(kca, k):
    W = (k + 31) // 32
    with finished_ctx(kca, k) as ctx:
        for n in SIZES:
            r = crafted(W, n, seed=n * 5 + W)
            install(ctx, r)
            for n_bins in HIST_BINS if n in (0, 2, 1025, 16385, 65537) else (256, 4097):
                h = ctx.histogram(n_bins)
                assert h == np_hist(r["cnt"], n_bins), (n, n_bins)
                assert sum(h) == n
            check_lookup(ctx, r, W, seed=n)
            assert ctx.lookup(np.zeros((0, W), dtype=np.uint64))[0].shape == (0,)  # n_keys = 0
            # filters compose: each step works on what the last one kept
            cur = r
            for lo, hi in [(0, U32_MAX), (1, U32_MAX), (2, 5), (3, 3), (9, 9)]:
                cur = mask(cur, lo, hi)
                assert ctx.filter(lo, hi) == len(cur), (n, lo, hi)
                assert ctx.finish() == len(cur)
                assert ctx.records() == cur.tobytes(), (n, lo, hi)
                assert ctx.stats()["output_records"] == len(cur)
            assert len(cur) == 0
            assert ctx.histogram(4) == [0, 0, 0, 0]
            # the other ranges straight on the whole run
            install(ctx, r)
            cur = mask(r, 2, 5)
            assert ctx.filter(2, 5) == len(cur)
            assert ctx.records() == cur.tobytes(), n
            assert ctx.histogram(256) == np_hist(cur["cnt"], 256)
            check_lookup(ctx, cur, W, seed=n + 1)
            install(ctx, r)
            cur = mask(r, U32_MAX, U32_MAX)
            assert ctx.filter(U32_MAX, U32_MAX) == len(cur)
            assert ctx.records() == cur.tobytes(), n


@pytest.mark.parametrize("shape", ["ones", "max", "uniform"])
def test_histogram_contention_shapes(kca, shape):
    """All records in one bin (64 lanes on one address without the wave
    aggregation), and counts spread over twice the bins."""
    n, n_bins = 200000, 256
    rng = np.random.default_rng(7)
    r = np.zeros(n, dtype=rec_dtype(1))
    r["key"][:, 0] = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(3)
    r["cnt"] = {"ones": np.ones(n, dtype=np.uint32), "max": np.full(n, U32_MAX, dtype=np.uint32),
                "uniform": rng.integers(0, 2 * n_bins, n).astype(np.uint32)}[shape]
    with finished_ctx(kca, 31) as ctx:
        install(ctx, r)
        for nb in (n_bins, 2, 65536):
            assert ctx.histogram(nb) == np_hist(r["cnt"], nb)


def test_lookup_device_agrees_with_lookup(kca):
    import torch

    for k in (31, 55, 100):
        W = (k + 31) // 32
        r = crafted(W, 4097, seed=k)
        with finished_ctx(kca, k) as ctx:
            install(ctx, r)
            keys, counts, found = check_lookup(ctx, r, W, seed=3)
            dk = torch.from_numpy(keys.view(np.int64)).cuda()
            dc = torch.full((len(keys),), -1, dtype=torch.int32, device="cuda")
            df = torch.full((len(keys),), 7, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            nf = ctx.lookup_device(dk.data_ptr(), len(keys), dc.data_ptr(), df.data_ptr())
            assert nf == int(found.sum())
            assert np.array_equal(dc.cpu().numpy().view(np.uint32), counts)
            assert np.array_equal(df.cpu().numpy().astype(bool), found)
            dc.fill_(-1)
            torch.cuda.synchronize()
            assert ctx.lookup_device(dk.data_ptr(), len(keys), dc.data_ptr(), 0) == nf  # found may be NULL
            assert np.array_equal(dc.cpu().numpy().view(np.uint32), counts)
            assert ctx.lookup_device(0, 0, 0, 0) == 0


@functools.lru_cache(maxsize=None)
def _oracle_count(k, seed):
    import oracle
    from conftest import load_pkg

    fq = load_pkg().synth_fastq(3000, 150, seed, genome_length=20000, n_rate=0.002)
    return fq, oracle.count_fastq(fq, k)


@pytest.mark.parametrize("engine", ["auto", "partition", "table"])
@pytest.mark.parametrize("k", [21, 55, 100])
def test_real_counts(kca, orc, k, engine):
    W = (k + 31) // 32
    fq, want = _oracle_count(k, 5)
    r = np.frombuffer(want, dtype=rec_dtype(W))
    with kca.Context(kmer_length=k, line_length=150, engine=engine) as ctx:
        ctx.count_fastq(fq)
        assert ctx.records() == want
        for nb in (256, 3):
            assert ctx.histogram(nb) == np_hist(r["cnt"], nb)
        keys = np.ascontiguousarray(r["key"])
        counts, found = ctx.lookup(keys)
        assert found.all() and np.array_equal(counts, r["cnt"])
        kept = mask(r, 2, U32_MAX)
        assert 0 < len(kept) < len(r)
        assert ctx.filter(2) == len(kept)
        assert ctx.records() == kept.tobytes()
        assert sum(ctx.owner_counts(4)) == len(kept)
        assert ctx.histogram(256) == np_hist(kept["cnt"], 256)
        counts, found = ctx.lookup(keys)
        assert np.array_equal(found, r["cnt"] >= 2)
        assert np.array_equal(counts, np.where(r["cnt"] >= 2, r["cnt"], 0))
        kept2 = mask(kept, 0, 3)  # a second filter composes with the first
        assert ctx.filter(0, 3) == len(kept2)
        assert ctx.records() == kept2.tobytes()
        # a new count on the same context is not disturbed by the swapped run buffers
        fq2, want2 = _oracle_count(k, 6)
        ctx.reset()
        ctx.count_fastq(fq2)
        assert ctx.records() == want2
        assert ctx.histogram(256) == np_hist(np.frombuffer(want2, dtype=rec_dtype(W))["cnt"], 256)


def test_state_rules(kca, orc, tmp_path, monkeypatch):
    k, L = 31, 150
    q = np.zeros((1, 1), dtype=np.uint64)
    with kca.Context(kmer_length=k, line_length=L) as ctx:
        ctx.count_fastq(kca.synth_fastq(100, L, seed=2))
        for call in (lambda: ctx.histogram(), lambda: ctx.filter(2), lambda: ctx.lookup(q),
                     lambda: ctx.lookup_device(0, 0, 0, 0)):
            with pytest.raises(kca.KcError) as e:
                call()
            assert e.value.status == STATE and "kc_finish" in str(e.value)
        ctx.finish()
        for call in (lambda: ctx.histogram(1), lambda: ctx.histogram(65537), lambda: ctx.histogram(0),
                     lambda: ctx.filter(3, 2)):
            with pytest.raises(kca.KcError) as e:
                call()
            assert e.value.status == kca.KC_ERR_ARG
    # host spill runs (a device with HBM to spare keeps its runs there and merges
    # them in kc_finish: KC_HOST_RUNS sends them to the host as when HBM is
    # short): the device calls refuse, the file form is the route
    monkeypatch.setenv("KC_HOST_RUNS", "1")
    fq = kca.synth_fastq(20000, L, seed=k, n_rate=0.001)
    with kca.Context(kmer_length=k, line_length=L, gpu_memory_limit=1 << 20, engine="partition",
                     lds_slots=1) as ctx:
        ctx.count_fastq(fq)
        ctx.finish()
        assert ctx.stats()["spill_runs"] >= 2
        for call in (lambda: ctx.histogram(), lambda: ctx.filter(2), lambda: ctx.lookup(q)):
            with pytest.raises(kca.KcError) as e:
                call()
            assert e.value.status == STATE
        out = tmp_path / "spilled.bin"
        out.write_bytes(ctx.output_bytes(str(tmp_path)))
    want = orc.count_fastq(fq, k)
    assert out.read_bytes() == want
    assert kca.histogram_file(str(out), k, 256) == np_hist(np.frombuffer(want, dtype=rec_dtype(1))["cnt"], 256)


def _truncate(r):
    t = np.zeros(len(r), dtype=rec_dtype(1))
    t["key"][:, 0] = r["key"][:, 0]
    t["cnt"] = r["cnt"]
    return t.tobytes()


def _parse_histo(path):
    return {int(a): int(b) for a, b in (line.split() for line in path.read_text().splitlines())}


@pytest.mark.parametrize("config", [["gpus=1"], ["gpus=2"], ["gpus=2", "exchange=alltoall"],
                                    ["gpus=1", "gpuMemoryLimit=1000000"], ["gpus=1", "gpuMemoryLimit=1000000"],
                                    ["gpus=2", "gpuMemoryLimit=1000000"]],
                         ids=["one", "gather", "alltoall", "small", "spill", "spill2"])
def test_cli_filter_and_histogram(kca, orc, tmp_path, monkeypatch, request, config):
    """Device route (one finished context without host spill runs) and file
    route (alltoall; host spill runs, forced by KC_HOST_RUNS in the spill
    cases; the file-merge fallback of spill2) write the same bytes."""
    if request.node.callspec.id.startswith("spill"):
        monkeypatch.setenv("KC_HOST_RUNS", "1")
    k, W = 55, 2
    fq, want = _oracle_count(k, 5)
    r = np.frombuffer(want, dtype=rec_dtype(W))
    d = tmp_path / "in"
    d.mkdir()
    (d / "a.fastq").write_bytes(fq)
    cli = os.path.join(os.path.dirname(kca.LIB_PATH), "kmer-counter")
    base = [cli, f"kmerLength={k}", f"inputFileLocation={d}", f"tempFileLocation={tmp_path}", "quiet=1"] + config
    kept = mask(r, 2, U32_MAX)
    for fmt in ("sorted", "dump"):
        out, hist = tmp_path / f"{fmt}.bin", tmp_path / f"{fmt}.histo"
        subprocess.run(base + [f"outputFile={out}", f"outputFormat={fmt}", "minCount=2", f"histogramFile={hist}"],
                       check=True, capture_output=True, timeout=300)
        assert out.read_bytes() == (kept.tobytes() if fmt == "sorted" else _truncate(kept)), fmt
        # the histogram of the complete count, taken before the filter
        assert _parse_histo(hist) == {i: v for i, v in enumerate(np_hist(r["cnt"], 10001)) if v}


def test_cli_bins_and_defaults(kca, orc, tmp_path):
    k, W = 55, 2
    fq, want = _oracle_count(k, 5)
    r = np.frombuffer(want, dtype=rec_dtype(W))
    d = tmp_path / "in"
    d.mkdir()
    (d / "a.fastq").write_bytes(fq)
    cli = os.path.join(os.path.dirname(kca.LIB_PATH), "kmer-counter")
    base = [cli, f"kmerLength={k}", f"inputFileLocation={d}", f"tempFileLocation={tmp_path}", "quiet=1"]
    out, hist = tmp_path / "few.bin", tmp_path / "few.histo"
    subprocess.run(base + [f"outputFile={out}", "maxCount=3", f"histogramFile={hist}", "histogramBins=4"],
                   check=True, capture_output=True, timeout=300)
    assert out.read_bytes() == mask(r, 0, 3).tobytes()
    assert _parse_histo(hist) == {i: v for i, v in enumerate(np_hist(r["cnt"], 4)) if v}
    # none of the new keys: the bytes of the plain count
    subprocess.run(base + [f"outputFile={out}"], check=True, capture_output=True, timeout=300)
    assert out.read_bytes() == want
