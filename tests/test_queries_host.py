"""Host-only forms of the queries on a finished count (no GPU):
kc_histogram_file / kc_filter_file and the CLI's `histo` / `filter`
subcommands over SortedKMerFile bytes on disk. Every expected value comes from
numpy over hand-built records or over the CPU oracle's bytes."""
import subprocess

import numpy as np
import pytest

U32_MAX = 0xFFFFFFFF
BINS = [2, 3, 256, 10001, 65536]


def rec_dtype(W):
    return np.dtype([("key", "<u8", (W,)), ("cnt", "<u4")])


def make_records(W, n_bins, seed, extra=400):
    """Sorted records with distinct keys; the counts hold the edges of an
    n_bins histogram (0, 1, n_bins-2, n_bins-1, n_bins, 2^32-1) and random
    values around them."""
    rng = np.random.default_rng(seed)
    edge = [0, 1, max(0, n_bins - 2), n_bins - 1, n_bins, U32_MAX, 2, 5, 3]
    cnt = np.concatenate([np.array(edge, dtype=np.uint64),
                          rng.integers(0, 2 * n_bins, extra, dtype=np.uint64),
                          rng.integers(0, 8, extra, dtype=np.uint64)]).astype(np.uint32)
    n = len(cnt)
    r = np.zeros(n, dtype=rec_dtype(W))
    # keys that share their leading words and differ only in the last one
    r["key"][:, W - 1] = np.cumsum(rng.integers(1, 1 << 30, n, dtype=np.uint64))
    if W > 1:
        r["key"][:, 0] = np.repeat(np.arange((n + 3) // 4, dtype=np.uint64), 4)[:n]
    r["cnt"] = rng.permutation(cnt)
    return r


def np_hist(cnt, n_bins):
    return np.bincount(np.minimum(cnt.astype(np.int64), n_bins - 1), minlength=n_bins).tolist()


def np_filter(data, W, lo, hi):
    r = np.frombuffer(data, dtype=rec_dtype(W))
    return r[(r["cnt"] >= lo) & (r["cnt"] <= hi)].tobytes()


def parse_histo(text):
    out = {}
    for line in text.splitlines():
        a, b = line.split()
        out[int(a)] = int(b)
    return out


@pytest.mark.parametrize("k", [31, 55, 100])
@pytest.mark.parametrize("n_bins", BINS)
def test_histogram_file_matches_numpy(kca, tmp_path, k, n_bins):
    W = (k + 31) // 32
    r = make_records(W, n_bins, seed=k * 7 + n_bins)
    p = tmp_path / "in.bin"
    p.write_bytes(r.tobytes())
    got = kca.histogram_file(str(p), k, n_bins)
    assert len(got) == n_bins
    assert sum(got) == len(r)
    assert got == np_hist(r["cnt"], n_bins)


@pytest.mark.parametrize("k", [31, 55, 100])
def test_filter_file_matches_numpy_mask(kca, tmp_path, k):
    W = (k + 31) // 32
    r = make_records(W, 256, seed=k)
    data = r.tobytes()
    p = tmp_path / "in.bin"
    p.write_bytes(data)
    out = tmp_path / "out.bin"
    for lo, hi in [(0, U32_MAX), (1, U32_MAX), (2, 5), (3, 3), (U32_MAX, U32_MAX), (0, 0)]:
        kept = kca.filter_file(str(p), str(out), k, lo, hi)
        want = np_filter(data, W, lo, hi)
        assert out.read_bytes() == want, (lo, hi)
        assert kept * (8 * W + 4) == len(want)
    assert kca.filter_file(str(p), str(out), k, 0, U32_MAX) == len(r)
    assert out.read_bytes() == data  # identity
    # a range that keeps nothing: an empty file
    absent = 1000003
    assert not (r["cnt"] == absent).any()
    assert kca.filter_file(str(p), str(out), k, absent, absent) == 0
    assert out.read_bytes() == b""
    # in place
    assert kca.filter_file(str(p), str(p), k, 2, 5) * (8 * W + 4) == len(np_filter(data, W, 2, 5))
    assert p.read_bytes() == np_filter(data, W, 2, 5)
    assert sorted(x.name for x in tmp_path.iterdir()) == ["in.bin", "out.bin"]  # no temp file left


@pytest.mark.parametrize("k", [31, 100])
def test_queries_on_an_empty_file(kca, tmp_path, k):
    p = tmp_path / "empty.bin"
    p.write_bytes(b"")
    out = tmp_path / "out.bin"
    assert kca.histogram_file(str(p), k, 256) == [0] * 256
    assert kca.filter_file(str(p), str(out), k, 1, U32_MAX) == 0
    assert out.read_bytes() == b""


def test_file_query_errors(kca, tmp_path):
    k, W = 55, 2
    r = make_records(W, 256, seed=3)
    p = tmp_path / "bad.bin"
    p.write_bytes(r.tobytes() + b"\x01" * 5)  # rs * n + 5 bytes
    out = tmp_path / "out.bin"
    with pytest.raises(kca.KcError) as e:
        kca.histogram_file(str(p), k, 256)
    assert e.value.status == kca.KC_ERR_IO
    with pytest.raises(kca.KcError) as e:
        kca.filter_file(str(p), str(out), k, 1, U32_MAX)
    assert e.value.status == kca.KC_ERR_IO
    assert not out.exists()
    with pytest.raises(kca.KcError) as e:
        kca.histogram_file(str(tmp_path / "missing.bin"), k, 256)
    assert e.value.status == kca.KC_ERR_IO
    good = tmp_path / "good.bin"
    good.write_bytes(r.tobytes())
    with pytest.raises(kca.KcError) as e:
        kca.filter_file(str(good), str(out), k, 6, 5)
    assert e.value.status == kca.KC_ERR_ARG
    for n_bins in (0, 1, 65537):
        with pytest.raises(kca.KcError) as e:
            kca.histogram_file(str(good), k, n_bins)
        assert e.value.status == kca.KC_ERR_ARG, n_bins


def test_abi_version_unchanged_by_the_queries(kca):
    L = kca.lib()
    assert L.kc_abi_version() == 7
    for name in ("kc_count_histogram", "kc_filter_records", "kc_lookup", "kc_lookup_device", "kc_histogram_file",
                 "kc_filter_file"):
        assert name in kca.header_functions()
        assert hasattr(L, name)


@pytest.mark.parametrize("k", [21, 55, 100])
def test_oracle_file_through_functions_and_cli(kca, orc, tmp_path, k):
    W = (k + 31) // 32
    data = orc.count_fastq(kca.synth_fastq(3000, 150, 11 + k, genome_length=20000, n_rate=0.002), k)
    r = np.frombuffer(data, dtype=rec_dtype(W))
    assert len(r) > 1000 and (r["cnt"] > 1).any() and (r["cnt"] == 1).any()
    p = tmp_path / "count.bin"
    p.write_bytes(data)
    for n_bins in (4, 256, 10001):
        assert kca.histogram_file(str(p), k, n_bins) == np_hist(r["cnt"], n_bins)
    out = tmp_path / "f.bin"
    assert kca.filter_file(str(p), str(out), k, 2) == int((r["cnt"] >= 2).sum())
    assert out.read_bytes() == np_filter(data, W, 2, U32_MAX)

    # the CLI's host-only subcommands (no GPU is opened)
    htxt = tmp_path / "h.txt"
    run = subprocess.run([kca.CLI_PATH, "histo", str(p), str(htxt), str(k)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    want = {i: v for i, v in enumerate(np_hist(r["cnt"], 10001)) if v}
    text = htxt.read_text()
    assert parse_histo(text) == want
    assert [int(x.split()[0]) for x in text.splitlines()] == sorted(want)  # ascending, non-empty bins only
    cout = tmp_path / "c.bin"
    run = subprocess.run([kca.CLI_PATH, "filter", str(p), str(cout), str(k), "2", "5"], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stderr
    assert cout.read_bytes() == np_filter(data, W, 2, 5)
    run = subprocess.run([kca.CLI_PATH, "filter", str(p), str(cout), str(k), "6", "5"], capture_output=True,
                         text=True)
    assert run.returncode == 1 and "above" in run.stderr


@pytest.mark.parametrize("args", [["minCount=3", "maxCount=2"], ["histogramBins=1"], ["histogramBins=65537"],
                                  ["histogramBins=0"], ["minCount=4294967296"], ["maxCount=x"]])
def test_cli_rejects_bad_query_keys(kca, tmp_path, args):
    """Checked while parsing, before any device is opened (exit 1 with a message, as one_of)."""
    run = subprocess.run([kca.CLI_PATH, "kmerLength=21", f"inputFileLocation={tmp_path}"] + args,
                         capture_output=True, text=True)
    assert run.returncode == 1
    assert "kmer-counter:" in run.stderr and args[-1].split("=")[0] in run.stderr
