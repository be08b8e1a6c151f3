"""Read sets of the super-k-mer tests (test_gpu_skm.py end to end,
test_gpu_skm_kernels.py at the kernels, test_kernel_ref.py on the CPU)."""
import random


def special_reads(L, n, seed):
    """Reads that reach F's slow path: not-ACGT bases, aligned all-A groups
    (possible key 0^W), poly-A / poly-T stretches, lowercase bases."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        s = [rng.choice("ACGT") for _ in range(L)]
        kind = i % 6
        if kind == 1:
            for _ in range(rng.randrange(1, 4)):
                s[rng.randrange(L)] = rng.choice("Nn.")
        elif kind == 2:
            a = rng.randrange(0, max(1, L - 40))
            s[a:a + 40] = "A" * min(40, L - a)
        elif kind == 3:
            s = list("A" * L)
        elif kind == 4:
            a = rng.randrange(0, max(1, L - 20))
            s[a:a + 20] = "T" * min(20, L - a)
            s[rng.randrange(L)] = "N"
        out.append("".join(s))
    return out


def genome_reads(L, n, seed, genome=4000):
    """Reads drawn from one random genome: windows repeat across reads, as at coverage."""
    rng = random.Random(seed)
    g = "".join(rng.choice("ACGT") for _ in range(genome + L))
    return [g[a:a + L] for a in (rng.randrange(genome) for _ in range(n))]


def edge_reads(L, k, seed):
    """Reads of L bases aimed at the front ends' edges: a not-ACGT base at
    position 0, at L - 1, on both sides of the first 8-window chunk edge
    (windows 7 | 8) and of the first 16-base group edge (bases 15 | 16), where
    the read has them; all-A reads and aligned all-A halves at the read end
    (key 0^W); homopolymers and short tandem repeats (runs longer than nmax);
    two adjacent reads where the first ends with the bases the second starts
    with (a run must not continue across reads)."""
    rng = random.Random(seed)

    def rnd(n=L):
        return "".join(rng.choice("ACGT") for _ in range(n))

    def put(s, i, c="N"):
        return s[:i] + c + s[i + 1:] if 0 <= i < len(s) else s

    out = []
    for i in (0, L - 1, 7, 8, 15, 16, 7 + k - 1, 8 + k - 1, L - k, L - k - 1):
        out.append(put(rnd(), i))
    out.append(put(put(rnd(), 0), L - 1, "n"))
    out += ["A" * L, "C" * L, "G" * L, "T" * L]
    h = 8 * ((L - 8) // 8)  # the last aligned 8-base half inside the read
    out += [rnd(h) + "A" * (L - h), "A" * (L - h) + rnd(h), rnd(L - h) + "A" * h if h else rnd()]
    out += [("AC" * L)[:L], ("ACG" * L)[:L], ("AAAT" * L)[:L], ("ACGTT" * L)[:L]]
    out.append(rnd(L // 2) + ("GT" * L)[:L - L // 2])
    tail = rnd(min(L, k + 5))
    out += [(rnd() + tail)[-L:], (tail + rnd())[:L]]
    assert all(len(s) == L for s in out)
    return out
