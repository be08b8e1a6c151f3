"""Canonical counts on the host (no GPU): the two Python statements of the fold
(tests/canon_ref.py) against each other over the CPU oracle's bytes, then
kc_canonicalize_file and the CLI's `canon` subcommand against them."""
import subprocess

import pytest

import canon_ref

KS = [1, 2, 29, 30, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128]


@pytest.fixture(scope="module")
def stranded(kca):
    return canon_ref.stranded_input(kca)


@pytest.fixture(scope="module")
def oracle_counts(orc, stranded):
    fq, _ = stranded
    return {k: orc.count_fastq(fq, k) for k in KS}


def rs_of(k):
    return 8 * ((k + 31) // 32) + 4


@pytest.mark.parametrize("k", KS)
def test_fold_of_the_oracle_count_is_the_canonical_count(stranded, oracle_counts, k):
    """Pins the reference of every other test: the fold of the strand-wise
    count (mask rule at k mod 32 in {29, 30, 31}, hole rule) equals counting
    canonical k-mers from the read strings."""
    _, reads = stranded
    plain = oracle_counts[k]
    want = canon_ref.count_canonical(reads, k)
    assert canon_ref.fold_records(plain, k) == want
    assert len(want) < len(plain)  # strands met
    W = (k + 31) // 32
    zero = canon_ref.kmer_ref_py.parse_records(want, k)[0]
    assert zero[0] == tuple([0] * W)
    if k >= 29:  # no other read holds A^k or T^k: the all-A and the all-T read's windows
        assert zero[1] == 2 * (150 - k + 1)


@pytest.mark.parametrize("k", KS)
def test_file_fold_and_cli_on_the_oracle_count(kca, tmp_path, stranded, oracle_counts, k):
    _, reads = stranded
    want = canon_ref.count_canonical(reads, k)
    p, out = tmp_path / "in.bin", tmp_path / "out.bin"
    p.write_bytes(oracle_counts[k])
    assert kca.canonicalize_file(str(p), str(out), k) * rs_of(k) == len(want)
    assert out.read_bytes() == want
    assert p.read_bytes() == oracle_counts[k]
    # idempotent, and in place
    assert kca.canonicalize_file(str(out), str(out), k) * rs_of(k) == len(want)
    assert out.read_bytes() == want
    cli = tmp_path / "cli.bin"
    run = subprocess.run([kca.CLI_PATH, "canon", str(p), str(cli), str(k)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert cli.read_bytes() == want
    assert sorted(x.name for x in tmp_path.iterdir()) == ["cli.bin", "in.bin", "out.bin"]  # no temp file left


CASES = [(kind, hole, tk) for kind in ("mixed", "stay", "flip") for hole, tk in ((False, False), (True, False),
                                                                                 (False, True), (True, True))]


@pytest.mark.parametrize("k", [1, 2, 31, 32, 33, 55, 63, 64, 100, 128])
def test_file_fold_of_crafted_records(kca, tmp_path, k):
    p = tmp_path / "in.bin"
    for n in (1, 2, 3, 257, 2500):
        for i, (kind, hole, tk) in enumerate(CASES):
            data = canon_ref.crafted(k, n, seed=k * 100 + n + i, kind=kind, hole=hole, tk=tk)
            assert len(data) == n * rs_of(k)
            want = canon_ref.fold_records(data, k)
            p.write_bytes(data)
            got_n = kca.canonicalize_file(str(p), str(p), k)  # in place
            assert p.read_bytes() == want, (n, kind, hole, tk)
            assert got_n * rs_of(k) == len(want)
            if kind == "stay" and not tk and k % 32 == 0:
                assert want == data  # nothing moves, nothing meets
            assert canon_ref.fold_records(want, k) == want  # the reference is idempotent too
    assert [x.name for x in tmp_path.iterdir()] == ["in.bin"]


def test_crafted_records_hold_what_they_promise():
    """x with rc(x) wrapping to 1, palindromes, records that differ only behind base k."""
    k = 31
    data = canon_ref.crafted(k, 2500, seed=1, kind="mixed", hole=True, tk=True)
    recs = canon_ref.kmer_ref_py.parse_records(data, k)
    kmers = [canon_ref.key_to_bases(w)[:k] for w, _ in recs]
    assert len(set(kmers)) < len(kmers)  # same k-mer, other bases behind it
    have = set(kmers)
    pairs = [x for x in have if canon_ref.revcomp(x) in have and canon_ref.revcomp(x) != x]
    assert len(pairs) > 100
    folded = dict(canon_ref.kmer_ref_py.parse_records(canon_ref.fold_records(data, k), k))
    assert 1 in folded.values()
    assert folded[(0,)] == 5  # the hole's 0 + T^k's 5
    even = canon_ref.crafted(64, 2500, seed=2)
    kmers = [canon_ref.key_to_bases(w)[:64] for w, _ in canon_ref.kmer_ref_py.parse_records(even, 64)]
    assert sum(x == canon_ref.revcomp(x) for x in kmers) > 50


@pytest.mark.parametrize("k", [31, 100])
def test_empty_file(kca, tmp_path, k):
    p, out = tmp_path / "empty.bin", tmp_path / "out.bin"
    p.write_bytes(b"")
    assert kca.canonicalize_file(str(p), str(out), k) == 0
    assert out.read_bytes() == b""
    assert canon_ref.fold_records(b"", k) == b""


def test_file_fold_errors(kca, tmp_path):
    k = 55
    data = canon_ref.crafted(k, 100, seed=3)
    bad, out = tmp_path / "bad.bin", tmp_path / "out.bin"
    bad.write_bytes(data + b"\x01" * 5)
    with pytest.raises(kca.KcError) as e:
        kca.canonicalize_file(str(bad), str(out), k)
    assert e.value.status == kca.KC_ERR_IO
    assert not out.exists()
    with pytest.raises(kca.KcError) as e:
        kca.canonicalize_file(str(tmp_path / "missing.bin"), str(out), k)
    assert e.value.status == kca.KC_ERR_IO
    good = tmp_path / "good.bin"
    good.write_bytes(data)
    for badk in (0, 129, -1):
        with pytest.raises(kca.KcError) as e:
            kca.canonicalize_file(str(good), str(out), badk)
        assert e.value.status == kca.KC_ERR_ARG
    assert sorted(x.name for x in tmp_path.iterdir()) == ["bad.bin", "good.bin"]
    run = subprocess.run([kca.CLI_PATH, "canon", str(bad), str(out), str(k)], capture_output=True, text=True)
    assert run.returncode == 1 and "kmer-counter:" in run.stderr


@pytest.mark.parametrize("value", ["2", "x", "-1", ""])
def test_cli_rejects_bad_canonical_key(kca, tmp_path, value):
    """Checked while parsing, before any device is opened (exit 1 with the key's name)."""
    run = subprocess.run([kca.CLI_PATH, "kmerLength=21", f"inputFileLocation={tmp_path}", f"canonical={value}"],
                         capture_output=True, text=True)
    assert run.returncode == 1
    assert "kmer-counter:" in run.stderr and "canonical" in run.stderr


def test_abi_is_additive(kca):
    L = kca.lib()
    assert L.kc_abi_version() == 7
    for name in ("kc_canonicalize", "kc_canonicalize_file"):
        assert name in kca.header_functions()
        assert hasattr(L, name)
