"""The finish's paths through the C ABI: kc_merge_runs_device with fewer than
two runs, and the engines' finishes (sorted, radix, skm grouped with and
without summed duplicates, skm ungrouped) on one batch, each bit-exact against
the CPU oracle and each asserting the path it took. Needs an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 150


# ---- kc_merge_runs_device with fewer than two runs --------------------------

@pytest.fixture(scope="module")
def small_runs(kca, orc):
    """k -> the oracle's records of 300 reads (sorted, every key once)."""
    fq = kca.synth_fastq(300, 120, 41, n_rate=0.002, genome_length=30_000)
    return {k: orc.count_fastq(fq, k) for k in (31, 55)}


def _merge_runs(kca, k, buf, counts):
    import torch

    with kca.Context(kmer_length=k, line_length=120) as ctx:
        ctx.finish()
        src = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda() if buf else \
            torch.empty(0, dtype=torch.uint8).cuda()
        n = ctx.merge_runs(src, counts)
        return n, ctx.records()


@pytest.mark.parametrize("k", [31, 55])
def test_merge_runs_device_zero_runs(kca, k):
    assert _merge_runs(kca, k, b"", []) == (0, b"")


@pytest.mark.parametrize("k", [31, 55])
def test_merge_runs_device_one_run_comes_back_unchanged(kca, orc, small_runs, k):
    run = small_runs[k]
    rs = orc.rs_of(k)
    assert len(run) > 100 * rs
    assert _merge_runs(kca, k, run, [len(run) // rs]) == (len(run) // rs, run)


@pytest.mark.parametrize("k", [31, 55])
def test_merge_runs_device_one_run_with_repeats_is_summed(kca, orc, small_runs, k):
    """Every third record doubled in place with another count (the run stays
    sorted, repeats adjacent): each key comes back once, the counts summed as
    u32 (one sum wraps)."""
    W = (k + 31) // 32
    rec = np.dtype([("key", "<u8", (W,)), ("cnt", "<u4")])
    assert rec.itemsize == orc.rs_of(k)
    a = np.frombuffer(small_runs[k], dtype=rec)
    reps = np.where(np.arange(len(a)) % 3 == 0, 2, 1)
    b = np.repeat(a, reps)
    second = np.flatnonzero(np.r_[False, (b["key"][1:] == b["key"][:-1]).all(axis=1)])
    assert len(second) == (len(a) + 2) // 3
    b["cnt"][second] = b["cnt"][second] * np.uint32(3) + np.uint32(5)
    b["cnt"][second[0]] = 0xFFFFFFFF
    # the numpy reduction: run heads, counts summed per run modulo 2^32
    heads = np.flatnonzero(np.r_[True, (b["key"][1:] != b["key"][:-1]).any(axis=1)])
    want = b[heads].copy()
    want["cnt"] = (np.add.reduceat(b["cnt"].astype(np.uint64), heads) & 0xFFFFFFFF).astype(np.uint32)
    assert len(want) == len(a) and (want["key"] == a["key"]).all()
    assert int(want["cnt"][0]) == (int(a["cnt"][0]) - 1) & 0xFFFFFFFF
    n, got = _merge_runs(kca, k, b.tobytes(), [len(b)])
    assert n == len(a) and got == want.tobytes()


# ---- the finishes of one batch ----------------------------------------------

@pytest.fixture(scope="module")
def batch(kca):
    """2,000 reads of 150 bases from a 200k-base genome: more distinct k-mers
    than the 65,536 the skm grouped finish needs."""
    return kca.synth_fastq(2000, L, 7, n_rate=0.001, genome_length=200_000)


@pytest.fixture(scope="module")
def batch_want(orc, batch):
    return {k: orc.count_fastq(batch, k) for k in (31, 55)}


# The partition engine reports its finish in KC_TRACE lines, and KC_TRACE is
# read once per process: a child counts the batch twice, default and
# KC_NO_SEGSORT, and the trace on its stderr is cut at the "==" marks.
_CHILD = r"""
import importlib.util, os, sys
root, k, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
spec = importlib.util.spec_from_file_location("kmer_counter_amd", os.path.join(root, "kmer-counter_amd", "__init__.py"))
kca = importlib.util.module_from_spec(spec)
sys.modules["kmer_counter_amd"] = kca
spec.loader.exec_module(kca)
fq = open(os.path.join(out, "batch.fq"), "rb").read()
for name in ("default", "KC_NO_SEGSORT"):
    if name != "default":
        os.environ[name] = "1"
    sys.stderr.write("== %s\n" % name)
    sys.stderr.flush()
    with kca.Context(kmer_length=k, line_length=150, engine="partition") as ctx:
        ctx.count_fastq(fq)
        rec = ctx.records()
    with open(os.path.join(out, name + ".bin"), "wb") as f:
        f.write(rec)
"""


@pytest.mark.parametrize("k", [31, 55])
def test_partition_finishes_agree(batch, batch_want, tmp_path, k):
    """Partition engine: the sorted finish (default) and the radix finish
    (KC_NO_SEGSORT) give the oracle's bytes; the trace shows which one ran."""
    (tmp_path / "batch.fq").write_bytes(batch)
    env = dict(os.environ, KC_TEST_HOOKS="1", KC_TRACE="1")
    env.pop("KC_NO_SEGSORT", None)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(k), str(tmp_path)], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    _, default, noseg = r.stderr.split("== ")
    assert default.startswith("default") and noseg.startswith("KC_NO_SEGSORT")
    assert "finish_part:" in default and "finish_part_sorted segment sort" in default, default
    assert "finish_part:" in noseg and "finish_part_sorted" not in noseg, noseg
    assert (tmp_path / "default.bin").read_bytes() == batch_want[k]
    assert (tmp_path / "KC_NO_SEGSORT.bin").read_bytes() == batch_want[k]


def _count_skm(kca, blocks):
    with kca.Context(kmer_length=31, line_length=L, engine="skm") as ctx:
        for fq, line in blocks:
            ctx.count_fastq(fq, line)
        got = ctx.records()
        return got, ctx.stats()


@pytest.mark.parametrize("hook", [None, "KC_NO_REC_DIG", "KC_NO_SEGSORT"])
def test_skm_finishes_agree(kca, batch, batch_want, monkeypatch, hook):
    """skm engine, k = 31: the grouped finish (P5's digit bytes, or word 0 under
    KC_NO_REC_DIG) and the ungrouped one (KC_NO_SEGSORT) give the oracle's bytes;
    finish_group_ms tells the grouped finish from the other."""
    if hook:
        monkeypatch.setenv(hook, "1")
    got, st = _count_skm(kca, [(batch, L)])
    assert st["engines_used"] == 1 and st["batches"] == 1
    assert len(got) > 65536 * 12
    if hook == "KC_NO_SEGSORT":
        assert st["finish_group_ms"] == 0
    else:
        assert st["finish_group_ms"] > 0
    assert got == batch_want[31]


def test_skm_grouped_finish_sums_two_batches(kca, orc):
    """Two calls whose line lengths differ: the pending batch is flushed between
    them, so the grouped finish meets keys of two batches and sums them."""
    a = kca.synth_fastq(1100, L, 7, n_rate=0.001, genome_length=200_000)
    b = kca.synth_fastq(1100, 140, 7, n_rate=0.001, genome_length=200_000, first_read=1100)
    got, st = _count_skm(kca, [(a, L), (b, 140)])
    assert st["engines_used"] == 1 and st["batches"] == 2
    assert st["finish_group_ms"] > 0
    want = orc.count_fastq_varlen(a + b, 31)  # (reads of two lengths: one reference chunk per length)
    assert len(want) > 65536 * 12 and len(want) < 12 * (1100 * 120 + 1100 * 110)
    assert got == want
