"""The CPU oracle against the golden fixtures, the pure-Python statement and
the reference's own reader (oracle/_ref, built from /root/reference sources)."""
import json
import os
import random

import pytest

import kmer_ref_py as kp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json")))


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_oracle_matches_golden(orc, name):
    m = MANIFEST[name]
    data = open(os.path.join(GOLD, m["fastq"]), "rb").read()
    want = open(os.path.join(GOLD, m["expected"]), "rb").read()
    import hashlib
    assert hashlib.sha256(data).hexdigest() == m["sha256_fastq"]
    assert hashlib.sha256(want).hexdigest() == m["sha256_expected"]
    assert orc.count_fastq(data, m["k"], mode="spec") == want
    assert orc.count_fastq(data, m["k"], mode="ref") == want
    assert orc.refcpu(data, m["k"], threads=2)[0] == want


@pytest.mark.parametrize("name", sorted(MANIFEST))
def test_window_checksum_matches_golden(orc, name):
    """The full-size parity property (window checksums, kc_oracle.c) agrees
    with every golden output: the sums of two key hashes over the valid
    windows equal the count-weighted sums over the records."""
    m = MANIFEST[name]
    data = open(os.path.join(GOLD, m["fastq"]), "rb").read()
    want = open(os.path.join(GOLD, m["expected"]), "rb").read()
    k = m["k"]
    a = orc.window_checksum(data, k, threads=3)
    b = orc.records_checksum(want, k, threads=2)
    assert (a["h1"], a["h2"], a["valid"]) == (b["h1"], b["h2"], b["count"])
    assert b["unordered"] == 0
    rs = orc.rs_of(k)
    zero_first = want[:rs - 4] == bytes(rs - 4)
    assert a["hole"] <= zero_first  # an invalid window makes key 0^W present


def test_window_checksum_detects_moved_count(orc):
    """A count moved from one key to another, a dropped record or swapped
    records all change the record sums (or the order check)."""
    import numpy as np

    data = open(os.path.join(GOLD, MANIFEST[sorted(MANIFEST)[0]]["fastq"]), "rb").read()
    k = MANIFEST[sorted(MANIFEST)[0]]["k"]
    want = orc.count_fastq(data, k)
    rs = orc.rs_of(k)
    good = orc.records_checksum(want, k)
    recs = np.frombuffer(bytearray(want), dtype=np.uint8).reshape(-1, rs).copy()
    c = recs[:, rs - 4:].copy().view("<u4")
    i = int(np.argmax(c[:-1, 0] >= 1))
    moved = recs.copy()
    moved[i, rs - 4:] = np.frombuffer(np.uint32(c[i, 0] - 1).tobytes(), np.uint8)
    moved[i + 1, rs - 4:] = np.frombuffer(np.uint32(c[i + 1, 0] + 1).tobytes(), np.uint8)
    bad = orc.records_checksum(moved.tobytes(), k)
    assert bad["count"] == good["count"] and (bad["h1"], bad["h2"]) != (good["h1"], good["h2"])
    assert orc.records_checksum(np.delete(recs, i, axis=0).tobytes(), k)["h1"] != good["h1"]
    swapped = recs.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert orc.records_checksum(swapped.tobytes(), k)["unordered"] > 0


def _reads(rng, n, L, alphabet="ACGT", n_rate=0.0):
    out = []
    for _ in range(n):
        s = "".join(rng.choice(alphabet) for _ in range(L))
        if n_rate:
            s = "".join("N" if rng.random() < n_rate else c for c in s)
        out.append(s)
    return out


def _fq(reads):
    return "".join(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n" for i, s in enumerate(reads))


@pytest.mark.parametrize("k,L", [(1, 5), (4, 9), (16, 40), (21, 100), (28, 60), (29, 60), (30, 61), (31, 100),
                                 (32, 90), (33, 70), (55, 150), (60, 99), (63, 70), (64, 130), (65, 99), (96, 130),
                                 (97, 131), (127, 150), (128, 150)])
def test_spec_ref_python_agree(orc, k, L):
    rng = random.Random(k * 1000 + L)
    reads = _reads(rng, 40, L, n_rate=0.02) + ["A" * L, "T" * L, "N" * L]
    text = _fq(reads)
    py = kp.to_bytes(kp.count_reads(reads, k), k)
    assert orc.count_fastq(text.encode(), k, mode="spec") == py
    # the ref-structured form restates bitEncode, which is undefined for
    # L % 32 == 0 (shift by 64) and for L < 10 (the in-place 2 + 8*ceil(L/32)
    # byte encoding runs into the next read)
    if L % 32 and L >= 10:
        assert orc.count_fastq(text.encode(), k, mode="ref") == py


def test_chunking_does_not_change_counts(orc):
    rng = random.Random(7)
    text = _fq(_reads(rng, 300, 80, n_rate=0.01)).encode()
    a = orc.count_fastq(text, 25, gpu_memory_limit=100000000)
    for limit in (20000, 50000, 333333):
        assert orc.count_fastq(text, 25, gpu_memory_limit=limit) == a


def test_chunk_size_formula(orc):
    # KMerCounter.cpp:193-212 at the survey's configurations: the
    # chunk has room for n reads and readData fills n-1 of them
    assert orc.chunk_size(150, 31, 100000000) == 150 * 52110
    assert orc.chunk_size(100, 21, 100000000) == 100 * 78186
    assert orc.chunk_size(150, 55, 100000000) == 150 * 43421
    text = _fq(["ACGT" * 5] * 10).encode()
    assert [len(c) // 20 for c, _ in orc.chunks_of(text, 20 * 4)] == [3, 3, 3, 1]


def test_known_answer_single_read(orc):
    # one read "ACGT" * 8 (32 bases) at k=31: one window with the 32nd base
    # carried in the key (k % 32 = 31 -> no mask)
    text = _fq(["ACGT" * 8])
    recs = kp.parse_records(orc.count_fastq(text.encode(), 31), 31)
    assert recs == [((int("1b" * 8, 16),), 1), ((int("6c" * 8, 16),), 1)] or len(recs) == 2
    v = 0
    for c in "ACGT" * 8:
        v = (v << 2) | kp.CODE[c]
    assert (v,) in [r[0] for r in recs]
    # k = 21 (masked): the key keeps exactly 21 bases
    recs21 = kp.parse_records(orc.count_fastq(text.encode(), 21), 21)
    first = 0
    for c in ("ACGT" * 8)[:21]:
        first = (first << 2) | kp.CODE[c]
    first <<= 64 - 42
    assert (first,) in [r[0] for r in recs21]


def _weird_cases():
    rng = random.Random(5)

    def rec(i, L, hdr=None, qual=None, eol="\n"):
        seq = "".join(rng.choice("ACGTN") for _ in range(L))
        h = hdr if hdr is not None else f"@r{i}"
        q = qual if qual is not None else "I" * L
        return f"{h}{eol}{seq}{eol}+{eol}{q}{eol}"

    return {
        "normal": "".join(rec(i, 50) for i in range(40)),
        "longhdr": "".join(rec(i, 20, hdr="@" + "x" * 60) for i in range(40)),
        "blankmid": "".join(rec(i, 30) for i in range(10)) + "\n" + "".join(rec(i, 30) for i in range(10, 20)),
        "blankend": "".join(rec(i, 30) for i in range(10)) + "\n",
        "nofinalnl": "".join(rec(i, 30) for i in range(10))[:-1],
        "crlf": "".join(rec(i, 30, eol="\r\n") for i in range(12)),
        "varlen": "".join(rec(i, rng.choice([28, 30, 33])) for i in range(25)),
        "plusqual": "".join(rec(i, 30, qual="+" + "I" * 29) for i in range(12)),
    }


READER_CHUNKS = (31, 60, 61, 100, 257, 1000, 10 ** 6)


@pytest.fixture(scope="module")
def reader_golden():
    with open(os.path.join(GOLD, "ref_reader_chunks.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(_weird_cases()))
def test_reader_matches_reference_reader(orc, tmp_path, reader_golden, name):
    """The oracle's readData restatement against the reference's own
    InputFileHandler/FASTQFileReader: its recorded chunks
    (golden/ref_reader_chunks.json, written by make_ref_reader_chunks.py) and,
    where oracle/_ref/ref_reader is built, the program itself."""
    text = _weird_cases()[name]
    gold = reader_golden[name]
    assert gold["input"] == text  # the recording is of this input
    live = orc.have_ref("ref_reader")
    d = tmp_path / name
    d.mkdir()
    (d / "a.fq").write_text(text)
    for chunk in READER_CHUNKS:
        mine = orc.chunks_of(text.encode(), chunk)
        # (a recorded chunk is its text with the last byte repeated n more times)
        ref = [((c + c[-1:] * n).encode("latin-1"), ll) for c, ll, n in gold["chunks"][str(chunk)]]
        if live:
            assert orc.ref_chunks(str(d), chunk) == ref, (name, chunk)
        assert [c for c, _ in mine] == [c for c, _ in ref], (name, chunk)
        for (_, l1), (_, l2) in zip(mine, ref):
            # the reference pops a file whose last line is blank before it
            # dispatches the chunk and then takes L from the next (absent)
            # file: L = 0, a division by zero in processKMers. We keep L.
            assert l1 == l2 or (name == "blankend" and l2 == 0)
