"""Pure-Python statements of canonical k-mer counts (include/kc.h,
kc_canonicalize), written over strings and plain ints with no bit tricks, so
nothing is shared with the C and HIP code they check. TEST INFRASTRUCTURE.

fold_records(data, k): the fold of SortedKMerFile bytes. A record's key is
read as 32 W bases; only its first k bases count (bases from k on are
dropped); the record moves to min(s, rc(s)) taken as strings, which is the
word order because A < C < G < T are the codes 0..3 and the key is padded with
A; equal keys are summed as u32, wrapping; the output is sorted.

count_canonical(reads, k): the same bytes from the reads themselves. Every
all-ACGT window adds 1 to min(s, rc(s)); if any window is not all ACGT the key
0^W (A^k, its own canonical form) is present with at least count 0.
"""
from collections import Counter

import kmer_ref_py

BASES = "ACGT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s: str) -> str:
    return "".join(COMP[c] for c in reversed(s))


def canonical(s: str) -> str:
    return min(s, revcomp(s))


_DIGITS = str.maketrans("ACGT", "0123")
_BYTE_BASES = ["".join(BASES[(b // 4 ** (3 - i)) % 4] for i in range(4)) for b in range(256)]


def key_to_bases(words) -> str:
    """The 32 bases of every word, first base in the word's highest digit."""
    return "".join(_BYTE_BASES[b] for w in words for b in int(w).to_bytes(8, "big"))


def bases_to_key(s: str, W: int):
    """s padded with A to 32 W bases, every 32 of them one base-4 number."""
    t = s + "A" * (32 * W - len(s))
    return tuple(int(t[32 * j:32 * j + 32].translate(_DIGITS), 4) for j in range(W))


def fold_records(data: bytes, k: int) -> bytes:
    W = (k + 31) // 32
    cnt = Counter()
    for words, c in kmer_ref_py.parse_records(data, k):
        s = key_to_bases(words)[:k]
        cnt[bases_to_key(canonical(s), W)] += c
    return kmer_ref_py.to_bytes(cnt, k)  # counts modulo 2^32


def count_canonical(reads, k: int) -> bytes:
    W = (k + 31) // 32
    by_string = Counter()
    hole = False
    for s in reads:
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            if all(ch in COMP for ch in w):
                by_string[canonical(w)] += 1
            else:
                hole = True
    cnt = Counter({bases_to_key(s, W): c for s, c in by_string.items()})
    if hole:
        cnt[tuple([0] * W)] += 0
    return kmer_ref_py.to_bytes(cnt, k)


U32_MAX = 0xFFFFFFFF
_COUNTS = [0, 1, 1, 1, 2, 3, 7, 255, 256, 65535, 65536, U32_MAX - 1, U32_MAX]


def crafted(k: int, n: int, seed: int, kind: str = "mixed", hole: bool = False, tk: bool = False) -> bytes:
    """SortedKMerFile bytes of exactly n records with distinct keys.

    kind "stay": every k-mer is <= its reverse complement; "flip": every one
    is greater; "mixed": k-mers x with their rc(x) also present (counts
    U32_MAX and 2: the sum wraps to 1), palindromes at even k, the same k-mer
    twice with different bases behind it, and plain ones. Where 32 W > k half
    the records carry random bases from position k on (the reference's keys do
    at k mod 32 in {29, 30, 31}; the fold drops them at every k). K-mers are
    drawn both with a common head (keys that share words 0..W-2) and with a
    common tail (their reverse complements share them). hole: the 0^W record
    with count 0; tk: a T^k record."""
    import random

    rng = random.Random(seed)
    W = (k + 31) // 32
    pad = 32 * W - k
    recs = {}

    def bases(m):
        return "".join(rng.choice(BASES) for _ in range(m))

    def add(x, cnt, junk=True):
        if len(recs) < n:
            tail = bases(pad) if junk and rng.random() < 0.5 else "A" * pad
            recs.setdefault(bases_to_key(x + tail, W), cnt)

    if hole:
        add("A" * k, 0, junk=False)
    if tk:
        add("T" * k, 5, junk=False)
    t_far = min(k, 12)
    t_near = min(k, max(2, k - 32 * (W - 1)))
    fixed = [bases(k) for _ in range(3)]
    while len(recs) < n:
        t = t_far if rng.random() < 0.5 else t_near
        x = rng.choice(fixed)[:k - t] + bases(t)
        if rng.random() < 0.3:
            x = revcomp(x)  # a common tail
        r = revcomp(x)
        cnt = rng.choice(_COUNTS)
        if len(set(x)) == 1 and x[0] in "AT":
            continue  # A^k (key 0^W) and T^k only on request
        if kind == "stay":
            add(min(x, r), cnt)
        elif kind == "flip":
            if x != r:
                add(max(x, r), cnt)
        else:
            roll = rng.random()
            if roll < 0.3 and x != r:
                add(x, U32_MAX)
                add(r, 2)
            elif roll < 0.4 and k % 2 == 0:
                h = x[:k // 2]
                add(h + revcomp(h), cnt)
            elif roll < 0.6:
                add(x, cnt)
                add(x, cnt + 1 & U32_MAX)
            else:
                add(x, cnt)
    return kmer_ref_py.to_bytes(recs, k)


def paired_input(kca, n_reads=1500, read_length=150, seed=23):
    """(fastq bytes, reads): n_reads iid reads with a few N, each followed
    later by its own reverse complement: 2 n_reads (L - k + 1) windows over
    about n_reads (L - k + 1) canonical keys, enough distinct keys to outgrow a
    small gpu_memory_limit (spill runs) while every key still meets its partner."""
    key = ("paired", n_reads, read_length, seed)
    if key not in _INPUT:
        text = kca.synth_fastq(n_reads, read_length, seed, n_rate=0.001).decode()
        reads = kmer_ref_py.fastq_reads(text)
        comp = dict(COMP, N="N")
        reads = reads + ["".join(comp[c] for c in reversed(r)) for r in reads]
        fq = "".join(f"@r{i}\n{r}\n+\n{'I' * read_length}\n" for i, r in enumerate(reads)).encode()
        _INPUT[key] = (fq, reads)
    return _INPUT[key]


_INPUT = {}


def stranded_input(kca, n_reads=300, read_length=150, genome=3000, seed=17):
    """(fastq bytes, reads): reads sampled from a small genome with a few N,
    every second one replaced by its own reverse complement string (N stays N),
    so nearly every canonical key sums a staying record with a flipped one;
    read 0 is all T and read 1 all A, so key 0^W gains counts from both."""
    key = (n_reads, read_length, genome, seed)
    if key not in _INPUT:
        text = kca.synth_fastq(n_reads, read_length, seed, genome_length=genome, n_rate=0.002).decode()
        reads = kmer_ref_py.fastq_reads(text)
        assert len(reads) == n_reads and all(len(r) == read_length for r in reads)
        comp = dict(COMP, N="N")
        reads = [r if i % 2 == 0 else "".join(comp[c] for c in reversed(r)) for i, r in enumerate(reads)]
        reads[0] = "T" * read_length
        reads[1] = "A" * read_length
        fq = "".join(f"@r{i}\n{r}\n+\n{'I' * read_length}\n" for i, r in enumerate(reads)).encode()
        _INPUT[key] = (fq, reads)
    return _INPUT[key]
