"""Set operations between two SortedKMerFiles on the host (no GPU):
kc_combine_files, the CLI's `combine` subcommand and the reference the GPU
tests use (setops_ref). Every expected value comes from setops_ref.combine,
which works with dicts keyed by the key tuple."""
import functools
import subprocess

import numpy as np
import pytest

import setops_ref as sr
from setops_ref import CASES, COUNT_SUBTRACT, INTERSECT, MIN, SUBTRACT, SUM, U32, UNION

K_OF_W = {1: 31, 2: 55, 3: 90, 4: 100}


@pytest.mark.parametrize("W", [1, 2, 3, 4])
def test_reference_forms_agree(W):
    for seed, n in enumerate([0, 1, 2, 3, 17, 64, 257]):
        for hole in [(False, False), (True, False), (False, True), (True, True)]:
            if n < 2 and any(hole):
                continue
            a, b = sr.split_runs(W, n, seed * 11 + W, hole=hole)
            for op, mode in CASES:
                want = sr.combine(a, b, op, mode)
                got = sr.combine_vec(a, b, op, mode)
                assert got.tobytes() == want.tobytes(), (n, hole, op, mode)
                # sorted, one record per key
                k = [tuple(int(x) for x in r) for r in want["key"]]
                assert k == sorted(set(k))
    # one operand empty, and a run against itself
    a, _ = sr.split_runs(W, 40, 5)
    e = a[:0]
    for op, mode in CASES:
        for x, y in [(a, e), (e, a), (e, e), (a, a.copy())]:
            assert sr.combine_vec(x, y, op, mode).tobytes() == sr.combine(x, y, op, mode).tobytes()


def crafted_pairs(W):
    """(name, a, b) of the crafted files: sizes are small, the cases are not."""
    pool = sr.key_pool(W, 90, seed=100 + W)
    e = np.zeros(0, dtype=sr.rec_dtype(W))
    a = sr.run_of(pool[::2], 1)
    yield "empty_a", e, a
    yield "empty_b", a, e
    yield "both_empty", e, e
    yield "same", a, a.copy()
    yield "same_keys_other_counts", a, sr.run_of(pool[::2], 2)
    yield "disjoint", a, sr.run_of(pool[1::2], 3)
    yield "apart", sr.run_of(pool[:30], 4), sr.run_of(pool[50:], 5)
    # interleaved, every third key of the pool in both runs
    i = np.arange(len(pool))
    yield "third_shared", sr.run_of(pool[(i % 3 == 0) | (i % 2 == 0)], 6), sr.run_of(pool[(i % 3 == 0) | (i % 2 == 1)], 7)
    for name, hole in [("hole_a", (True, False)), ("hole_b", (False, True)), ("hole_both", (True, True))]:
        x, y = sr.split_runs(W, 61, 8 + W, hole=hole)
        assert (not x["key"][0].any()) == hole[0] and (not y["key"][0].any()) == hole[1]
        yield name, x, y
    # every pair of counts from {0, 1, U32 - 1, U32} on shared keys: SUM wraps,
    # COUNT_SUBTRACT meets a < b, a == b and a > b
    edge = [0, 1, U32 - 1, U32]
    x = np.zeros(16, dtype=sr.rec_dtype(W))
    x["key"] = pool[:16]
    y = x.copy()
    x["cnt"] = np.repeat(edge, 4)
    y["cnt"] = np.tile(edge, 4)
    yield "count_edges", x, y


@pytest.mark.parametrize("W", [1, 2, 4])
def test_combine_files_crafted(kca, tmp_path, W):
    k, rs = K_OF_W[W], 8 * W + 4
    pa, pb, out = tmp_path / "a.bin", tmp_path / "b.bin", tmp_path / "out.bin"
    names = []
    for name, a, b in crafted_pairs(W):
        names.append(name)
        pa.write_bytes(a.tobytes())
        pb.write_bytes(b.tobytes())
        for op, mode in CASES:
            want = sr.combine(a, b, op, mode)
            n = kca.combine_files(str(pa), str(pb), str(out), k, op, mode)
            assert out.read_bytes() == want.tobytes(), (name, op, mode)
            assert n == len(want)
            # names select the same operation
            assert kca.combine_files(str(pa), str(pb), str(out), k, sr.OP_NAMES[op], sr.MODE_NAMES[mode]) == n
            assert out.read_bytes() == want.tobytes(), (name, op, mode)
        assert pa.read_bytes() == a.tobytes() and pb.read_bytes() == b.tobytes()
        if name == "count_edges":
            assert ((a["cnt"].astype(np.uint64) + b["cnt"]) > U32).any()
            assert (a["cnt"] < b["cnt"]).any() and (a["cnt"] == b["cnt"]).any() and (a["cnt"] > b["cnt"]).any()
        # the identities of the interface
        if name == "same":
            assert kca.combine_files(str(pa), str(pb), str(out), k, "intersect", "left") == len(a)
            assert out.read_bytes() == a.tobytes()
            assert kca.combine_files(str(pa), str(pb), str(out), k, "subtract") == 0
            assert out.read_bytes() == b""
        if name == "empty_b":
            assert kca.combine_files(str(pa), str(pb), str(out), k, "count_subtract") == len(a)
            assert out.read_bytes() == a.tobytes()
    assert len(names) == 12
    assert sorted(x.name for x in tmp_path.iterdir()) == ["a.bin", "b.bin", "out.bin"]  # no temp file left


@pytest.mark.parametrize("W", [1, 2, 4])
def test_output_may_be_an_input(kca, tmp_path, W):
    k = K_OF_W[W]
    a, b = sr.split_runs(W, 300, 40 + W, hole=(True, True))
    for op, mode in [(UNION, SUM), (INTERSECT, MIN), (SUBTRACT, SUM), (COUNT_SUBTRACT, SUM)]:
        want = sr.combine(a, b, op, mode).tobytes()
        for target in ("a", "b"):
            pa, pb = tmp_path / "a.bin", tmp_path / "b.bin"
            pa.write_bytes(a.tobytes())
            pb.write_bytes(b.tobytes())
            out = pa if target == "a" else pb
            assert kca.combine_files(str(pa), str(pb), str(out), k, op, mode) * (8 * W + 4) == len(want)
            assert out.read_bytes() == want, (op, mode, target)
            other = pb if target == "a" else pa
            assert other.read_bytes() == (b if target == "a" else a).tobytes()
    assert sorted(x.name for x in tmp_path.iterdir()) == ["a.bin", "b.bin"]


def test_file_errors_leave_the_output_untouched(kca, tmp_path):
    k, W = 55, 2
    a, b = sr.split_runs(W, 200, 3)
    good_a, good_b, out = tmp_path / "a.bin", tmp_path / "b.bin", tmp_path / "out.bin"
    good_a.write_bytes(a.tobytes())
    good_b.write_bytes(b.tobytes())
    out.write_bytes(b"keep me")
    bad = tmp_path / "bad.bin"
    swapped = a.copy()
    swapped[[50, 51]] = swapped[[51, 50]]
    twice = np.concatenate([a[:10], a[9:]])  # a key twice: ascending, not strictly
    late = a.copy()  # the last record out of order: seen only at the end of the pass
    late[-1] = late[0]
    for data in (a.tobytes() + b"\x01" * 5, a.tobytes()[:-1], swapped.tobytes(), twice.tobytes(), late.tobytes()):
        bad.write_bytes(data)
        for args in ((bad, good_b), (good_a, bad)):
            for op in ("union", "intersect", "subtract", "count_subtract"):
                with pytest.raises(kca.KcError) as e:
                    kca.combine_files(str(args[0]), str(args[1]), str(out), k, op)
                assert e.value.status == kca.KC_ERR_IO
                assert out.read_bytes() == b"keep me"
    with pytest.raises(kca.KcError) as e:
        kca.combine_files(str(tmp_path / "missing.bin"), str(good_b), str(out), k, "union")
    assert e.value.status == kca.KC_ERR_IO
    # in place: the bad input itself is the output and stays as it was
    bad.write_bytes(swapped.tobytes())
    with pytest.raises(kca.KcError):
        kca.combine_files(str(bad), str(good_b), str(bad), k, "union")
    assert bad.read_bytes() == swapped.tobytes()
    assert sorted(x.name for x in tmp_path.iterdir()) == ["a.bin", "b.bin", "bad.bin", "out.bin"]
    # arguments
    for kk, op, mode in [(0, 0, 0), (129, 0, 0), (k, 4, 0), (k, 0, 5), (k, SUBTRACT, MIN), (k, COUNT_SUBTRACT, 4),
                         (k, 0xFFFFFFFF, 0)]:
        with pytest.raises(kca.KcError) as e:
            kca.combine_files(str(good_a), str(good_b), str(out), kk, op, mode)
        assert e.value.status == kca.KC_ERR_ARG, (kk, op, mode)
    for op, mode in [("xor", "sum"), ("union", "avg")]:
        with pytest.raises(kca.KcError) as e:
            kca.combine_files(str(good_a), str(good_b), str(out), k, op, mode)
        assert e.value.status == kca.KC_ERR_ARG
    assert out.read_bytes() == b"keep me"


@functools.lru_cache(maxsize=None)
def oracle_pair(k):
    """The CPU oracle's counts of two disjoint read ranges of one genome."""
    import oracle
    from conftest import load_pkg

    kca = load_pkg()
    fa = kca.synth_fastq(300, 150, 21, genome_length=8000, n_rate=0.002, first_read=0)
    fb = kca.synth_fastq(300, 150, 21, genome_length=8000, n_rate=0.002, first_read=300)
    return oracle.count_fastq(fa, k), oracle.count_fastq(fb, k)


@pytest.mark.parametrize("k", [31, 55])
def test_real_counts(kca, orc, tmp_path, k):
    W = (k + 31) // 32
    da, db = oracle_pair(k)
    a, b = np.frombuffer(da, dtype=sr.rec_dtype(W)), np.frombuffer(db, dtype=sr.rec_dtype(W))
    pa, pb, out = tmp_path / "a.bin", tmp_path / "b.bin", tmp_path / "out.bin"
    pa.write_bytes(da)
    pb.write_bytes(db)
    shared = len(sr.combine(a, b, INTERSECT, MIN))
    assert 0 < shared < min(len(a), len(b))  # the same genome: the runs overlap, neither holds the other
    for op, mode in [(INTERSECT, MIN), (SUBTRACT, SUM), (UNION, SUM)]:
        want = sr.combine(a, b, op, mode)
        assert sr.combine_vec(a, b, op, mode).tobytes() == want.tobytes()
        assert kca.combine_files(str(pa), str(pb), str(out), k, op, mode) == len(want)
        assert out.read_bytes() == want.tobytes(), (op, mode)
    # UNION / SUM is the summing merge of the two files
    merged = tmp_path / "merged.bin"
    kca.merge_files([str(pa), str(pb)], str(merged), k)
    assert merged.read_bytes() == out.read_bytes()


def test_cli_combine(kca, tmp_path):
    k, W = 55, 2
    a, b = sr.split_runs(W, 500, 9, hole=(True, True))
    pa, pb, out, cout = tmp_path / "a.bin", tmp_path / "b.bin", tmp_path / "out.bin", tmp_path / "cli.bin"
    pa.write_bytes(a.tobytes())
    pb.write_bytes(b.tobytes())
    for op, mode in [("union", "max"), ("intersect", "right"), ("subtract", "sum"), ("count_subtract", "sum")]:
        n = kca.combine_files(str(pa), str(pb), str(out), k, op, mode)
        run = subprocess.run([kca.CLI_PATH, "combine", op, mode, str(pa), str(pb), str(cout), str(k)],
                             capture_output=True, text=True)
        assert run.returncode == 0, run.stderr
        assert cout.read_bytes() == out.read_bytes() == sr.combine(a, b, sr.OPS[op], sr.MODES[mode]).tobytes()
        assert f"{n} combined records" in run.stdout
    cout.write_bytes(b"keep me")
    for op, mode in [("xor", "sum"), ("union", "avg"), ("subtract", "min"), ("", "")]:
        run = subprocess.run([kca.CLI_PATH, "combine", op, mode, str(pa), str(pb), str(cout), str(k)],
                             capture_output=True, text=True)
        assert run.returncode != 0 and "kmer-counter: combine" in run.stderr, (op, mode)
        assert cout.read_bytes() == b"keep me"
    bad = tmp_path / "bad.bin"
    bad.write_bytes(a.tobytes()[:-3])
    run = subprocess.run([kca.CLI_PATH, "combine", "union", "sum", str(bad), str(pb), str(cout), str(k)],
                         capture_output=True, text=True)
    assert run.returncode != 0 and cout.read_bytes() == b"keep me"


def test_abi_version_unchanged_by_the_set_operations(kca):
    L = kca.lib()
    assert L.kc_abi_version() == 7
    for name in ("kc_combine_records_device", "kc_combine_contexts", "kc_combine_files"):
        assert name in kca.header_functions()
        assert getattr(L, name).argtypes is not None  # bound in lib()'s table
    assert (kca.KC_SET_UNION, kca.KC_SET_INTERSECT, kca.KC_SET_SUBTRACT, kca.KC_SET_COUNT_SUBTRACT) == (0, 1, 2, 3)
    assert (kca.KC_SETC_SUM, kca.KC_SETC_MIN, kca.KC_SETC_MAX, kca.KC_SETC_LEFT, kca.KC_SETC_RIGHT) == (0, 1, 2, 3, 4)
