// kc_sketch.inl — the coverage sketch behind the engine choice. Included by
// kc_kernels.hip inside namespace kc.
//
// Holds: sketch_k<GC> (sampled k-mer fingerprints of encoded reads) and
//   sketch_distinct_k (distinct fingerprints through a hash set).
// Uses: kc_common.inl (u32 / u64, kBlock, lane_id, mix64, grid_for) and
//   groups_per_read of kc_kernels.hip's E section.
// Host callers: kc_count.cpp (the engine choice).

// ---------------------------------------------------------------------------
// Coverage sketch (engine choice): one k-mer per read and 16-base group, the
// one starting at the group (aligned to the read, not to the genome), kept
// when a hash of its first 16 bases (its first code word) falls in 2^-rb of
// the hash space; its 56-bit fingerprint (a hash of the whole k-mer) is
// appended to `out`. The sample is a function of the k-mer, so every copy of
// a sampled k-mer is kept. Reads from a genome at coverage c repeat such a
// k-mer in ~c/16 reads (a read starting at the same position mod 16), so the
// share of distinct fingerprints estimates the coverage: iid reads ~1, cfg2's
// 30x ~0.46. The k-mer's bases are taken from the 2-bit codes (first base
// highest in each u32 of 16 bases); k-mers with a not-ACGT base are skipped.
// Per aligned position a lane loads one code word and hashes it with two u32
// multiplies; only the ~2^-rb sampled lanes load the rest of the k-mer and its
// not-ACGT masks and compute the fingerprint (the earlier form hashed every
// aligned k-mer whole with 64-bit mixes: 2.9 ms at cfg2).
// ---------------------------------------------------------------------------

__device__ __forceinline__ u32 sketch_mix32(u32 h) {  // murmur3 finaliser
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// One thread per read, every read's code row loaded at once (G u32 words,
// 8-byte aligned rows when G is even: G/2 dwordx2 loads) so a thread waits for
// one load latency per read, not one per aligned position (GC = 0: other
// row lengths, the words one by one, 64 positions at a time). The samples are
// gathered per workgroup in LDS and appended with one global atomic per
// workgroup: the earlier form took one atomic on the single output counter
// per wave that sampled anything (~2e5 same-address atomics at cfg2, which
// serialise and set the kernel's time at ~2.4 ms).
constexpr u32 kSketchBuf = 1024;  // samples a workgroup holds in LDS (~100 expected at the default rate)

template <int GC>
__global__ __launch_bounds__(kBlock) void sketch_k(const u32* __restrict__ codes, const unsigned short* __restrict__ inval,
                                                  u64 n_reads, int G, int k, int rate_bits, u64* __restrict__ out,
                                                  u64 cap, u64* __restrict__ counter) {
    __shared__ u64 sbuf[kSketchBuf];
    __shared__ u32 scnt;
    __shared__ u64 sbase;
    const int ng = (k + 15) >> 4;  // groups a k-mer spans from a group start
    const int per = G - ng + 1;    // aligned k-mers per read
    const u32 rmask = (1u << rate_bits) - 1;
    const int nb0 = min(16, k);
    const u32 keep0 = nb0 == 16 ? 0xffffffffu : ~(0xffffffffu >> (2 * nb0));
    const u32 seed = 0x9e3779b9u ^ (u32)k;
    if (threadIdx.x == 0) scnt = 0;
    __syncthreads();
    for (u64 r0 = (u64)blockIdx.x * kBlock; r0 < n_reads; r0 += (u64)gridDim.x * kBlock) {
        const u64 r = r0 + threadIdx.x;
        const bool live = r < n_reads;
        const u64 row = (live ? r : 0) * (u64)G;
        for (int g0 = 0; g0 < (GC > 0 ? 1 : per); g0 += 64) {
            // the candidates' first words: a bit per aligned position g0 + bit
            u64 cand = 0;
            if constexpr (GC > 0) {
                u32 cw[GC];
                const u64* rp = (const u64*)(codes + row);
#pragma unroll
                for (int j = 0; j < GC / 2; j++) {
                    const u64 v = __builtin_nontemporal_load(rp + j);
                    cw[2 * j] = (u32)v;
                    cw[2 * j + 1] = (u32)(v >> 32);
                }
#pragma unroll
                for (int g = 0; g < GC; g++)
                    if (g < per && live && (sketch_mix32((cw[g] & keep0) ^ seed) & rmask) == 0) cand |= 1ull << g;
            } else {
                for (int g = g0; g < min(per, g0 + 64); g++)
                    if (live && (sketch_mix32((codes[row + (u64)g] & keep0) ^ seed) & rmask) == 0)
                        cand |= 1ull << (g - g0);
            }
            // rare: the sampled k-mers whole (their words and not-ACGT masks)
            while (cand) {
                const int g = g0 + __ffsll((long long)cand) - 1;
                cand &= cand - 1;
                const u64 base = row + (u64)g;
                u64 h = 0x243f6a8885a308d3ull ^ (u64)k;
                bool ok = true;
                for (int j = 0; j < ng; j++) {
                    const int nb = min(16, k - 16 * j);  // bases of this group inside the k-mer
                    const u32 keep = nb == 16 ? 0xffffffffu : ~(0xffffffffu >> (2 * nb));
                    const unsigned short bad =
                        (unsigned short)(inval[base + j] & (nb == 16 ? 0xffffu : ~(0xffffu >> nb)));
                    ok = ok && bad == 0;
                    h = mix64(h ^ (u64)(codes[base + j] & keep) ^ ((u64)j << 40));
                }
                if (!ok) continue;
                const u32 i = atomicAdd(&scnt, 1u);
                if (i < kSketchBuf) {
                    sbuf[i] = h >> 8;
                } else {  // a full buffer: straight out (not expected at the planned rates)
                    const u64 q = atomicAdd((unsigned long long*)counter, 1ull);
                    if (q < cap) out[q] = h >> 8;
                }
            }
        }
    }
    __syncthreads();
    const u32 m = min(scnt, kSketchBuf);
    if (threadIdx.x == 0) sbase = m ? atomicAdd((unsigned long long*)counter, (unsigned long long)m) : 0ull;
    __syncthreads();
    for (u32 i = threadIdx.x; i < m; i += kBlock)
        if (sbase + i < cap) out[sbase + i] = sbuf[i];
}

hipError_t launch_sketch(const uint32_t* codes, const uint16_t* inval, uint64_t n_reads, int L, int k, int rate_bits,
                         uint64_t* out, uint64_t cap, uint64_t* counter, hipStream_t s) {
    const int G = groups_per_read(L);
    if (G <= 0 || n_reads == 0) return hipSuccess;
    // 8 workgroups per CU (the LDS sample buffers allow them), each walking
    // its share of the reads
    const int grid = grid_for(n_reads, 2048);
#define KC_SKETCH(GCV) \
    hipLaunchKernelGGL(sketch_k<GCV>, dim3(grid), dim3(kBlock), 0, s, codes, (const unsigned short*)inval, n_reads, G, \
                       k, rate_bits, out, cap, counter)
    switch (G) {  // common read lengths: the row in registers (G even: 8-byte aligned rows)
    case 2: KC_SKETCH(2); break;
    case 4: KC_SKETCH(4); break;
    case 6: KC_SKETCH(6); break;
    case 8: KC_SKETCH(8); break;
    case 10: KC_SKETCH(10); break;
    case 12: KC_SKETCH(12); break;
    case 14: KC_SKETCH(14); break;
    case 16: KC_SKETCH(16); break;
    default: KC_SKETCH(0); break;
    }
#undef KC_SKETCH
    return hipGetLastError();
}

// The sketch's distinct fingerprints: each of the min(*counter, cap) samples
// inserted into an open-addressing set of 2^set_bits slots (fingerprint + 1,
// 0 = empty; linear probing; cap <= half the slots, so every probe ends), the
// insertions that found an empty slot counted with one atomic per wave. Same
// count as sorting the samples and counting the run heads, with no host round
// trip between the sketch and the count: *counter is read on the device.
__global__ __launch_bounds__(kBlock) void sketch_distinct_k(const u64* __restrict__ fp, const u64* __restrict__ counter,
                                                            u64 cap, u64* __restrict__ set, int set_bits,
                                                            u64* __restrict__ distinct) {
    const u64 m = min(*counter, cap);
    const u64 mask = (1ull << set_bits) - 1;
    for (u64 i0 = (u64)blockIdx.x * kBlock; i0 < m; i0 += (u64)gridDim.x * kBlock) {
        const u64 i = i0 + threadIdx.x;
        bool fresh = false;
        if (i < m) {
            const u64 v = fp[i] + 1;  // fingerprints are < 2^56
            u64 slot = mix64(v) & mask;
            for (;;) {
                const u64 old = atomicCAS((unsigned long long*)&set[slot], 0ull, (unsigned long long)v);
                if (old == 0ull) {
                    fresh = true;
                    break;
                }
                if (old == v) break;
                slot = (slot + 1) & mask;
            }
        }
        const u64 b = __ballot(fresh);
        if (lane_id() == 0 && b) atomicAdd((unsigned long long*)distinct, (unsigned long long)__popcll(b));
    }
}

hipError_t launch_sketch_distinct(const uint64_t* fp, const uint64_t* counter, uint64_t cap, uint64_t* set,
                                  int set_bits, uint64_t* distinct, hipStream_t s) {
    if (set_bits < 1 || set_bits > 40 || cap > (1ull << set_bits) / 2) return hipErrorInvalidValue;
    const int grid = grid_for(cap, 1024);
    hipLaunchKernelGGL(sketch_distinct_k, dim3(grid), dim3(kBlock), 0, s, fp, counter, cap, set, set_bits, distinct);
    return hipGetLastError();
}
