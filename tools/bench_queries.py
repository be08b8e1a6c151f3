#!/usr/bin/env python3
"""Times the queries on a finished count (kc_count_histogram, kc_filter_records,
kc_lookup_device) against the route a caller had before them: kc_copy_records
to host memory, then numpy (bincount / boolean mask / searchsorted).

Two workloads (DESIGN §5 "Queries on the finished run"):
  genome : cfg2's generator scaled to --reads x 150 bp from a --genome bp
           genome, k = 31 (the same 30x coverage as cfg2 at the defaults)
  iid    : --iid-reads x 150 bp iid reads, k = 55 — cfg5's shape, every count
           is 1: the histogram's contention worst case

Every library call ends with a synchronisation of the context's stream, so a
call's wall time is its device time plus one launch + sync round trip; that is
what is reported (median of --reps after --warmup), and it can only overstate
the device side. The host route's copy buffer is allocated and touched before
it is timed. Prints one JSON line and writes it to --out; exits 1 when a
device operation is not faster than the host route.

--ops canon times kc_canonicalize instead (profiles/canon_bench.json), on the
same two workloads with the same method, the run refilled by a recount before
every repetition. The genome workload's reads have every second read
reverse-complemented (the generator samples one strand, and a one-strand run
brings no k-mer together with its reverse complement). Beside it, in the same
process: kc_merge_records_device over the run's own bytes (the parent's unpack
+ sort of every record + reduce + pack: what a fold without the stay/flip
split costs) and the host route, kc_copy_records plus kc_canonicalize_file
over those bytes in a memory-backed directory.

--ops setops times the set operations between two finished runs
(kc_combine_contexts; profiles/setops_bench.json) on the same two workloads: A
counts the first half of the workload's reads and B the second half (same seed
and genome, disjoint first_read ranges), A's run refilled by a recount before
every repetition. Bytes moved follow DESIGN §5's model (both passes read both
runs, the emit pass writes the result; an empty result needs no emit pass). Two yardsticks from the same process:
kc_merge_runs_device over the same two runs (the existing path that does
UNION / SUM's job) and the host route, kc_copy_records of both runs plus the
operation in numpy, whose result the device's bytes are checked against.
"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8e12  # bytes/s


def load_pkg():
    spec = importlib.util.spec_from_file_location("kmer_counter_amd",
                                                  os.path.join(ROOT, "kmer-counter_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["kmer_counter_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def median_ms(fn, reps, warmup, before=None):
    times = []
    for i in range(warmup + reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if i >= warmup:
            times.append((t1 - t0) * 1e3)
    return statistics.median(times)


def host_lookup(rec, W, q):
    """found, counts of the query keys q (m, W) in the sorted records."""
    n = len(rec)
    w0 = np.ascontiguousarray(rec["key"][:, 0])
    lo = np.searchsorted(w0, q[:, 0], "left")
    at = np.minimum(lo, n - 1)
    found = w0[at] == q[:, 0]
    if W > 1:
        hi = np.searchsorted(w0, q[:, 0], "right")
        for j in np.nonzero(hi - lo > 1)[0]:  # keys that share word 0: walk the group
            for i in range(lo[j], hi[j]):
                if (rec["key"][i] == q[j]).all():
                    at[j] = i
                    break
        found &= (rec["key"][at] == q).all(axis=1)
    return found, np.where(found, rec["cnt"][at], 0)


def stranded_fastq(kca, reads, read_length, seed, genome):
    """The generator's reads with every second one reverse-complemented, as
    FASTQ bytes (numpy uint8). The generator samples one strand only, and a
    one-strand run never brings a k-mer and its reverse complement together."""
    seqs = np.frombuffer(kca.synth_fastq(reads, read_length, seed, genome_length=genome, layout=1), dtype=np.uint8)
    seqs = seqs.reshape(reads, read_length)
    comp = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    rec = np.empty((reads, 2 * read_length + 7), dtype=np.uint8)
    rec[:, :3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:3 + read_length] = seqs
    rec[1::2, 3:3 + read_length] = comp[seqs[1::2, ::-1]]
    rec[:, 3 + read_length:6 + read_length] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + read_length:-1] = ord("I")
    rec[:, -1] = ord("\n")
    return rec.reshape(-1)


def shim_stay_count(kca, packed, W, k, n):
    """Staying records of a packed run, by the fold's own counting pass
    (libkc_kernel_shim.so's kcs_canon_count: tile counts, summed here)."""
    shim = ctypes.CDLL(os.path.join(os.path.dirname(kca.LIB_PATH), "libkc_kernel_shim.so"))
    shim.kcs_filter_tile.restype = ctypes.c_uint64
    shim.kcs_canon_count.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    tile = shim.kcs_filter_tile()
    cnt = np.zeros((n + tile - 1) // tile, dtype=np.uint64)
    rc = shim.kcs_canon_count(W, k, n, packed.ctypes.data, cnt.ctypes.data)
    assert rc == 0, f"kcs_canon_count: {rc}"
    return int(cnt.sum())


def run_canon(kca, torch, ctx, recount, k, reps, warmup, host_reps):
    """kc_canonicalize on the run that recount() finishes, beside the parent's
    full sort of the same bytes (kc_merge_records_device: unpack, radix sort of
    every record, reduce, pack — what a fold without the stay/flip split costs)
    and the host route (kc_copy_records, then kc_canonicalize_file over those
    bytes: its file read, fold and file write in a memory-backed directory)."""
    import tempfile

    L = kca.lib()
    W, rs = ctx.W, ctx.rs
    n_in = recount()
    buf = np.zeros(n_in * rs, dtype=np.uint8)
    copy_ms = median_ms(lambda: ctx._chk(L.kc_copy_records(ctx._h, ctypes.c_void_p(buf.ctypes.data), n_in * rs)),
                        host_reps, 1)
    n_stay = shim_stay_count(kca, buf, W, k, n_in)
    shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    with tempfile.TemporaryDirectory(dir=shm) as d:
        src, dst = os.path.join(d, "run.bin"), os.path.join(d, "canon.bin")
        buf.tofile(src)
        fold_ms = median_ms(lambda: kca.canonicalize_file(src, dst, k), host_reps, 0)
        want = np.fromfile(dst, dtype=np.uint8)
    # the parent's route on the device: a full sort of the run's own bytes
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    sort_ms = median_ms(lambda: ctx._chk(L.kc_merge_records_device(ctx._h, ctypes.c_void_p(dev.data_ptr()), n_in)),
                        reps, warmup)
    assert ctx.finish() == n_in
    del dev
    n_out = ctypes.c_uint64()
    canon_ms = median_ms(lambda: ctx._chk(L.kc_canonicalize(ctx._h, ctypes.byref(n_out))), reps, warmup,
                         before=recount)
    assert ctx.records() == want.tobytes(), "device fold differs from kc_canonicalize_file"
    again_ms = median_ms(lambda: ctx._chk(L.kc_canonicalize(ctx._h, ctypes.byref(n_out))), reps, 0)
    host = copy_ms + fold_ms
    return {"n_in": n_in, "n_stay": n_stay, "n_flip": n_in - n_stay, "n_out": n_out.value, "ms": canon_ms,
            "records_per_s": n_in / (canon_ms * 1e-3), "second_call_ms": again_ms, "full_sort_ms": sort_ms,
            "speedup_over_full_sort": sort_ms / canon_ms, "faster_than_full_sort": canon_ms < sort_ms,
            "copy_records_ms": copy_ms, "canonicalize_file_ms": fold_ms, "host_route_ms": host,
            "speedup": host / canon_ms, "faster_than_host_route": canon_ms < host}


def run_canon_workload(kca, torch, name, k, reads, genome, seed, mem, reps, warmup, host_reps):
    res = {"workload": name, "k": k, "reads": reads, "read_length": 150, "genome": genome, "seed": seed,
           "strands": "every second read reverse-complemented" if genome else "as generated (iid)"}
    with kca.Context(kmer_length=k, line_length=150, gpu_memory_limit=mem) as ctx:
        if genome:
            fq = torch.from_numpy(stranded_fastq(kca, reads, 150, seed, genome)).cuda()
            torch.cuda.synchronize()
            ptr, nbytes, held = fq.data_ptr(), fq.numel(), None
        else:
            ptr, nbytes = ctx.synth_device(reads, 150, seed, genome)
            held = ptr

        def recount():
            ctx.reset()
            ctx.count_fastq_device(ptr, nbytes)
            return ctx.finish()

        res["canonicalize"] = run_canon(kca, torch, ctx, recount, k, reps, warmup, host_reps)
        print(f"{name}: canonicalize {res['canonicalize']}", file=sys.stderr, flush=True)
        if held:
            ctx.free_device(held)
    return res


def run_workload(kca, torch, name, k, reads, genome, seed, mem, n_keys, reps, warmup, host_reps):
    W = (k + 31) // 32
    rs = 8 * W + 4
    dt = np.dtype([("key", "<u8", (W,)), ("cnt", "<u4")])
    L = kca.lib()
    res = {"workload": name, "k": k, "reads": reads, "read_length": 150, "genome": genome, "seed": seed}
    with kca.Context(kmer_length=k, line_length=150, gpu_memory_limit=mem) as ctx:
        ptr, nbytes = ctx.synth_device(reads, 150, seed, genome)

        def recount():
            ctx.reset()
            ctx.count_fastq_device(ptr, nbytes)
            return ctx.finish()

        n = recount()
        res["records"] = n
        print(f"{name}: {n} records", file=sys.stderr, flush=True)
        res["run_bytes"] = n * rs

        # ---- the route at the parent commit: copy out, numpy ----
        buf = np.zeros(n * rs, dtype=np.uint8)
        copy_ms = median_ms(lambda: ctx._chk(L.kc_copy_records(ctx._h, ctypes.c_void_p(buf.ctypes.data), n * rs)),
                            host_reps, 1)
        rec = buf.view(dt)
        rng = np.random.default_rng(seed)
        q = np.ascontiguousarray(rec["key"][rng.integers(0, n, n_keys)])
        want_hist = [None]
        want_kept = [None]
        want_look = [None]

        def h_hist():
            want_hist[0] = np.bincount(np.minimum(rec["cnt"], 255), minlength=256)

        def h_filter():
            want_kept[0] = rec[rec["cnt"] >= 2]

        def h_lookup():
            want_look[0] = host_lookup(rec, W, q)

        host = {"copy_records_ms": copy_ms,
                "histogram_numpy_ms": median_ms(h_hist, host_reps, 0),
                "filter_numpy_ms": median_ms(h_filter, host_reps, 0),
                "lookup_numpy_ms": median_ms(h_lookup, host_reps, 0)}

        print(f"{name}: host route {host}", file=sys.stderr, flush=True)
        # ---- device ----
        bins = (ctypes.c_uint64 * 256)()
        hist_ms = median_ms(lambda: ctx._chk(L.kc_count_histogram(ctx._h, bins, 256)), reps, warmup)
        assert list(bins) == want_hist[0].tolist(), "device histogram differs from numpy"

        dq = torch.from_numpy(q.view(np.int64)).cuda()
        dc = torch.zeros(n_keys, dtype=torch.int32, device="cuda")
        df = torch.zeros(n_keys, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nf = ctypes.c_uint64()
        look_ms = median_ms(lambda: ctx._chk(L.kc_lookup_device(ctx._h, ctypes.c_void_p(dq.data_ptr()), n_keys,
                                                                ctypes.c_void_p(dc.data_ptr()),
                                                                ctypes.c_void_p(df.data_ptr()), ctypes.byref(nf))),
                            reps, warmup)
        assert nf.value == int(want_look[0][0].sum()) == n_keys
        assert np.array_equal(dc.cpu().numpy().view(np.uint32), want_look[0][1]), "device lookup differs from numpy"

        kept = ctypes.c_uint64()
        filt_ms = median_ms(lambda: ctx._chk(L.kc_filter_records(ctx._h, 2, 0xFFFFFFFF, ctypes.byref(kept))),
                            reps, warmup, before=recount)
        assert kept.value == len(want_kept[0])
        assert ctx.records() == want_kept[0].tobytes(), "device filter differs from numpy"
        ctx.free_device(ptr)

    def line(ms, read_bytes, written=0):
        return {"ms": ms, "records_per_s": n / (ms * 1e-3), "bytes_read": read_bytes, "bytes_written": written,
                "hbm_peak_fraction": (read_bytes + written) / (ms * 1e-3) / HBM_PEAK}

    res["histogram"] = line(hist_ms, n * rs)
    res["filter"] = line(filt_ms, n * rs, kept.value * rs)
    res["filter"]["kept_records"] = kept.value
    res["lookup"] = {"ms": look_ms, "keys": n_keys, "keys_per_s": n_keys / (look_ms * 1e-3)}
    res["host_route"] = host
    for op in ("histogram", "filter", "lookup"):
        h = copy_ms + host[op + "_numpy_ms"]
        res[op]["host_route_ms"] = h
        res[op]["speedup"] = h / res[op]["ms"]
        res[op]["faster_than_host_route"] = res[op]["ms"] < h
    return res


SETOPS = [("union", "sum"), ("intersect", "min"), ("subtract", "sum"), ("count_subtract", "sum")]


def host_combine(a, b, op, mode):
    """The set operation in numpy over two sorted record arrays with one record
    per key: one stable sort of both runs' keys, neighbours compared."""
    na, n = len(a), len(a) + len(b)
    key = np.concatenate([a["key"], b["key"]])
    order = np.lexsort([key[:, j] for j in range(key.shape[1] - 1, -1, -1)])
    sk = key[order]
    same = np.zeros(n, dtype=bool)
    same[1:] = (sk[1:] == sk[:-1]).all(axis=1)
    nxt_same = np.zeros(n, dtype=bool)
    nxt_same[:-1] = same[1:]
    cnt = np.concatenate([a["cnt"], b["cnt"]])[order]
    nxt = np.zeros(n, dtype=np.uint32)
    nxt[:-1] = cnt[1:]
    pair, only_a = ~same & nxt_same, ~same & ~nxt_same & (order < na)
    if op == "union":
        keep, val = ~same, np.where(pair, cnt + nxt if mode == "sum" else np.minimum(cnt, nxt), cnt)
    elif op == "intersect":
        keep, val = pair, cnt + nxt if mode == "sum" else np.minimum(cnt, nxt)
    elif op == "subtract":
        keep, val = only_a, cnt
    else:
        keep, val = only_a | (pair & (cnt > nxt)), np.where(pair, cnt - nxt, cnt)
    out = np.zeros(int(keep.sum()), dtype=a.dtype)
    out["key"] = sk[keep]
    out["cnt"] = val[keep]
    return out


def run_setops_workload(kca, torch, name, k, reads, genome, seed, mem, reps, warmup, host_reps):
    L = kca.lib()
    W = (k + 31) // 32
    rs = 8 * W + 4
    dt = np.dtype([("key", "<u8", (W,)), ("cnt", "<u4")])
    half = reads // 2
    res = {"workload": name, "k": k, "reads_a": [0, half], "reads_b": [half, 2 * half], "read_length": 150,
           "genome": genome, "seed": seed}
    with kca.Context(kmer_length=k, line_length=150, gpu_memory_limit=mem) as ca, \
            kca.Context(kmer_length=k, line_length=150, gpu_memory_limit=mem) as cb, \
            kca.Context(kmer_length=k, line_length=150) as cm:
        pa, abytes = ca.synth_device(half, 150, seed, genome, first_read=0)
        pb, bbytes = cb.synth_device(half, 150, seed, genome, first_read=half)

        def recount():
            ca.reset()
            ca.count_fastq_device(pa, abytes)
            return ca.finish()

        na = recount()
        cb.count_fastq_device(pb, bbytes)
        nb = cb.finish()
        cb.free_device(pb)
        cm.count_fastq(kca.synth_fastq(10, 150, seed=1))
        cm.finish()
        res.update({"records_a": na, "records_b": nb, "run_bytes": (na + nb) * rs})
        print(f"{name}: A {na} records, B {nb} records", file=sys.stderr, flush=True)

        # ---- the host route: both runs out, numpy ----
        bufa, bufb = np.zeros(na * rs, dtype=np.uint8), np.zeros(nb * rs, dtype=np.uint8)

        def copy_out():
            ca._chk(L.kc_copy_records(ca._h, ctypes.c_void_p(bufa.ctypes.data), na * rs))
            cb._chk(L.kc_copy_records(cb._h, ctypes.c_void_p(bufb.ctypes.data), nb * rs))

        copy_ms = median_ms(copy_out, host_reps, 1)
        ra, rb = bufa.view(dt), bufb.view(dt)

        # ---- the existing path that does UNION / SUM's job ----
        both = torch.from_numpy(np.concatenate([bufa, bufb])).cuda()
        torch.cuda.synchronize()
        counts = (ctypes.c_uint64 * 2)(na, nb)
        merge_ms = median_ms(lambda: cm._chk(L.kc_merge_runs_device(cm._h, ctypes.c_void_p(both.data_ptr()), counts, 2)),
                             reps, warmup)
        merged = cm.records()
        del both
        res["merge_runs"] = {"ms": merge_ms, "n_out": len(merged) // rs}

        res["ops"] = {}
        for op, mode in SETOPS:
            want = [None]

            def on_host():
                want[0] = host_combine(ra, rb, op, mode)

            numpy_ms = median_ms(on_host, host_reps, 0)
            n_out = ctypes.c_uint64()
            ms = median_ms(lambda: ca._chk(L.kc_combine_contexts(ca._h, cb._h, kca._SET_OPS[op], kca._SET_COUNTS[mode],
                                                                 ctypes.byref(n_out))), reps, warmup, before=recount)
            got = ca.records()
            assert got == want[0].tobytes(), f"device {op}/{mode} differs from numpy"
            # both passes read both runs; an empty result needs no emit pass
            read_b, written = (2 if n_out.value else 1) * (na + nb) * rs, n_out.value * rs
            host = copy_ms + numpy_ms
            res["ops"][f"{op}/{mode}"] = {
                "ms": ms, "n_out": n_out.value, "records_per_s": (na + nb) / (ms * 1e-3), "bytes_read": read_b,
                "bytes_written": written, "hbm_peak_fraction": (read_b + written) / (ms * 1e-3) / HBM_PEAK,
                "copy_records_ms": copy_ms, "numpy_ms": numpy_ms, "host_route_ms": host, "speedup": host / ms,
                "faster_than_host_route": ms < host}
            if (op, mode) == ("union", "sum"):
                assert got == merged, "UNION/SUM differs from kc_merge_runs_device"
                res["ops"]["union/sum"].update({"merge_runs_ms": merge_ms, "ms_over_merge_runs_ms": ms / merge_ms,
                                                "slower_than_merge_runs": ms > merge_ms})
            print(f"{name}: {op}/{mode} {res['ops'][f'{op}/{mode}']}", file=sys.stderr, flush=True)
        ca.free_device(pa)
    return res


def main_setops(kca, torch, args):
    out = {"tool": "tools/bench_queries.py --ops setops", "timing": "wall time of the synchronous call, median",
           "bytes_model": "read 2 (na + nb) rs (count pass + emit pass; 1 (na + nb) rs when the result is empty: no "
                          "emit pass), written n_out rs; rs = 8 W + 4",
           "reps": args.reps, "warmup": args.warmup, "host_reps": {"genome": args.host_reps, "iid": args.iid_host_reps},
           "workloads": []}
    for name in args.workloads.split(","):
        if name == "genome":
            out["workloads"].append(run_setops_workload(kca, torch, "genome", 31, args.reads, args.genome, 2, 32 << 30,
                                                        args.reps, args.warmup, args.host_reps))
        elif name == "iid":
            out["workloads"].append(run_setops_workload(kca, torch, "iid", 55, args.iid_reads, 0, 5, 48 << 30,
                                                        args.reps, args.warmup, args.iid_host_reps))
        else:
            raise SystemExit(f"unknown workload {name}")
    out["pass"] = all(o["faster_than_host_route"] for w in out["workloads"] for o in w["ops"].values())
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if out["pass"] else 1


def main_canon(kca, torch, args):
    out = {"tool": "tools/bench_queries.py --ops canon", "timing": "wall time of the synchronous call, median",
           "reps": args.reps, "warmup": args.warmup, "host_reps": {"genome": args.host_reps, "iid": args.iid_host_reps},
           "workloads": []}
    for name in args.workloads.split(","):
        if name == "genome":
            out["workloads"].append(run_canon_workload(kca, torch, "genome", 31, args.reads, args.genome, 2, 32 << 30,
                                                       args.reps, args.warmup, args.host_reps))
        elif name == "iid":
            out["workloads"].append(run_canon_workload(kca, torch, "iid", 55, args.iid_reads, 0, 5, 48 << 30,
                                                       args.reps, args.warmup, args.iid_host_reps))
        else:
            raise SystemExit(f"unknown workload {name}")
    out["pass"] = all(w["canonicalize"]["faster_than_host_route"] for w in out["workloads"])
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if out["pass"] else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome", type=int, default=50_000_000)
    ap.add_argument("--iid-reads", type=int, default=10_000_000)
    ap.add_argument("--keys", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--iid-host-reps", type=int, default=1, help="the iid run is large: numpy takes seconds per pass")
    ap.add_argument("--workloads", default="genome,iid")
    ap.add_argument("--ops", default="queries", choices=["queries", "canon", "setops"],
                    help="queries: histogram, filter, lookup; canon: kc_canonicalize; setops: kc_combine_contexts "
                         "(each its own JSON, --out)")
    ap.add_argument("--out", default=None, help="default: profiles/queries_bench.json, profiles/canon_bench.json, "
                                                "profiles/setops_bench.json")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", {"canon": "canon_bench.json", "setops": "setops_bench.json"}.get(
            args.ops, "queries_bench.json"))
    import torch

    torch.zeros(1, device="cuda:0")  # PyTorch's HIP runtime opens the GPU first (tests/conftest.py)
    kca = load_pkg()
    if args.ops == "canon":
        return main_canon(kca, torch, args)
    if args.ops == "setops":
        return main_setops(kca, torch, args)
    out = {"tool": "tools/bench_queries.py", "timing": "wall time of the synchronous call, median",
           "reps": args.reps, "warmup": args.warmup, "host_reps": {"genome": args.host_reps, "iid": args.iid_host_reps}, "workloads": []}
    for name in args.workloads.split(","):
        if name == "genome":
            out["workloads"].append(run_workload(kca, torch, "genome", 31, args.reads, args.genome, 2, 32 << 30,
                                                 args.keys, args.reps, args.warmup, args.host_reps))
        elif name == "iid":
            out["workloads"].append(run_workload(kca, torch, "iid", 55, args.iid_reads, 0, 5, 48 << 30, args.keys,
                                                 args.reps, args.warmup, args.iid_host_reps))
        else:
            raise SystemExit(f"unknown workload {name}")
    out["pass"] = all(w[op]["faster_than_host_route"] for w in out["workloads"]
                      for op in ("histogram", "filter", "lookup"))
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0 if out["pass"] else 1


if __name__ == "__main__":
    sys.exit(main())
