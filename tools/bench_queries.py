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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "queries_bench.json"))
    args = ap.parse_args()
    import torch

    torch.zeros(1, device="cuda:0")  # PyTorch's HIP runtime opens the GPU first (tests/conftest.py)
    kca = load_pkg()
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
