// kc_synth.inl — the synthetic FASTQ generator on the device and on the host.
// Included by kc_kernels.hip inside namespace kc.
//
// Holds: synth_k, launch_synth, synth_host, synth_bytes; the generator itself
//   is kc_synth.h, which the kernel and the host writer share.
// Uses: kc_common.inl (u64, kBlock, grid_for).
// Host callers: kc_api.cpp (kc_synth_fastq*).

// ---------------------------------------------------------------------------
// synthetic FASTQ (bench/test input)
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void synth_k(kc_synth_params p, char* out) {
    for (u64 i = (u64)blockIdx.x * kBlock + threadIdx.x; i < p.n; i += (u64)gridDim.x * kBlock) {
        u64 rec = p.first + i;
        if (p.layout == 1)
            kc_synth_sequence(p, rec, out + i * (u64)p.L);
        else
            kc_synth_record(p, rec, out + kc_synth_offset(p.first, rec, p.L));
    }
}

static kc_synth_params to_params(const SynthArgs& a) {
    kc_synth_params p;
    p.first = a.first;
    p.n = a.n;
    p.seed = a.seed;
    p.genome = a.genome;
    p.n_threshold = a.n_threshold;
    p.L = a.L;
    p.Lmin = a.Lmin;
    p.layout = a.layout;
    return p;
}

hipError_t launch_synth(const SynthArgs& a, char* out, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(synth_k, dim3(grid_for(a.n, 16384)), dim3(kBlock), 0, s, to_params(a), out);
    return hipGetLastError();
}

void synth_host(const SynthArgs& a, char* out) {
    kc_synth_params p = to_params(a);
    for (u64 i = 0; i < a.n; i++) {
        u64 rec = a.first + i;
        if (a.layout == 1)
            kc_synth_sequence(p, rec, out + i * (u64)a.L);
        else
            kc_synth_record(p, rec, out + kc_synth_offset(a.first, rec, a.L));
    }
}

uint64_t synth_bytes(uint64_t first, uint64_t n, int64_t L, int layout) {
    return layout == 1 ? n * (uint64_t)L : kc_synth_offset(first, first + n, L);
}
