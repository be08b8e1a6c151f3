"""bench.py on the GPU at a small size: a plain run times its steps and nothing
else, --dump-outputs writes the last step's records as float64 arrays (checked
against the oracle's count of the same seeded input), and --full adds the
file-to-file leg, the host variants and the CPU baseline. Needs an MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READS, L, K, SEED, GENOME = 3000, 150, 31, 2, 300_000
SIZE = ["--reads", str(READS), "--genome", str(GENOME), "--mem", str(1 << 30)]


def _run_bench(*extra):
    env = {k: v for k, v in os.environ.items() if k != "KC_TEST_HOOKS"}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *SIZE, *extra],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _words(records, rs):
    """SortedKMerFile bytes as one row of little-endian u32 words per record."""
    return np.frombuffer(records, dtype="<u4").reshape(-1, rs // 4)


@pytest.fixture(scope="module")
def want(kca, orc):
    return orc.count_fastq(kca.synth_fastq(READS, L, SEED, genome_length=GENOME), K)


def test_plain_run_dumps_the_last_steps_records(want, tmp_path):
    out = tmp_path / "dump"
    d = _run_bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(out))
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "k-mers/s" and d["dtype"] == "u64"
    assert d["higher_is_better"] is True
    assert d["value"] == pytest.approx(READS * (L - K + 1) / (d["ms_per_step"] / 1e3), rel=1e-9)
    # nothing but the headline figure was measured
    assert d["cpu_baseline"] is None and d["end_to_end"] is None and d["host_variants"] is None
    w = _words(want, 12)
    assert sorted(os.listdir(out)) == ["column_sums.npy", "n_records.npy", "records_sample.npy", "sample_index.npy"]
    arrays = {n[:-4]: np.load(out / n) for n in os.listdir(out)}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["n_records"].tolist() == [len(w)] and d["distinct_kmers_per_gpu"] == len(w)
    assert np.array_equal(arrays["sample_index"], np.arange(len(w)))  # fewer records than the sample: all of them
    assert np.array_equal(arrays["records_sample"], w.astype(np.float64))
    s = w.sum(axis=0, dtype=np.uint64)
    assert np.array_equal(arrays["column_sums"], np.stack([s >> np.uint64(32), s & np.uint64(0xFFFFFFFF)], axis=1))


def test_dump_samples_seeded_blocks_of_a_larger_output(kca, want, tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setattr(bench, "DUMP_BLOCK", 16)
    monkeypatch.setattr(bench, "DUMP_BLOCKS", 8)
    w = _words(want, 12)
    D = bench.Dist()
    outs = []
    for name in ("a", "b"):
        with kca.Context(kmer_length=K, line_length=L, device=0, gpu_memory_limit=1 << 30) as ctx:
            ctx.count_fastq(kca.synth_fastq(READS, L, SEED, genome_length=GENOME))
            # a host buffer of 100 records: the column sums take many pieces
            bench.dump_outputs(ctx, D, str(tmp_path / name), piece=1200)
        outs.append({n[:-4]: np.load(tmp_path / name / n) for n in os.listdir(tmp_path / name)})
    a, b = outs
    assert all(np.array_equal(a[n], b[n]) for n in a) and a.keys() == b.keys()
    idx = a["sample_index"].astype(np.int64)
    blocks = np.unique(idx // 16)  # 8 whole blocks of 16 records (the output's last block may be shorter)
    assert len(blocks) == 8 and len(w) > 8 * 16
    assert np.array_equal(idx, np.concatenate([np.arange(b * 16, min(len(w), (b + 1) * 16)) for b in blocks]))
    assert np.array_equal(a["records_sample"], w[idx].astype(np.float64))
    s = w.sum(axis=0, dtype=np.uint64)
    assert np.array_equal(a["column_sums"], np.stack([s >> np.uint64(32), s & np.uint64(0xFFFFFFFF)], axis=1))
    assert a["n_records"].tolist() == [len(w)]


def test_full_run_adds_the_other_legs(tmp_path):
    d = _run_bench("--steps", "1", "--warmup", "0", "--full", "--cpu-reads", "2000", "--workdir", str(tmp_path))
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["value_t1"] > 0
    assert d["end_to_end"]["value"] > 0 and d["end_to_end"]["output_bytes"] == 12 * d["distinct_kmers_per_gpu"]
    assert d["host_variants"]["host_memory"]["value"] > 0
    assert d["host_variants"]["reference_chunks"]["value_chunks"] > 0
    assert os.listdir(tmp_path) == []  # the legs' files are gone
