// kc_query.inl — kernels over the finished run (packed SortedKMerFile
// records). Included by kc_kernels.hip inside namespace kc.
//
// Holds: count_histo_k (abundance histogram), filter_count_k / filter_scatter_k
//   (count-range filter), lookup_k (key lookup), canon_count_k / canon_split_k
//   (canonical fold by reverse complement; rev_groups).
// Uses: kc_common.inl (u32 / u64, kBlock, kWave, lane_id, lanemask_lt,
//   le64_32, hmin, dispatch_w, grid_for).
// Host callers: kc_api.cpp (histogram, filter, lookup), kc_finish.cpp (the
//   canonical fold).

// ---------------------------------------------------------------------------
// Queries on the finished run: abundance histogram, count-range
// filter, key lookup. All three walk the packed records (RW = 2W+1 dwords,
// the count last; records are only 4-byte aligned, so key words are read as
// dword pairs) and none of them waits on another workgroup of its launch.
// ---------------------------------------------------------------------------

constexpr int kHistLds = 4096;          // bins kept in the workgroup's LDS table; higher bins go to global atomics
constexpr int kHistSpan = kBlock * 64;  // records per fill of the LDS table (u32 bins cannot overflow)

__device__ __forceinline__ void histo_add(u32* tab, u64* __restrict__ bins, u32 nl, u32 b, u32 by) {
    if (b < nl)
        atomicAdd(&tab[b], by);
    else
        atomicAdd((unsigned long long*)&bins[b], (unsigned long long)by);
}

// One record's bin into the table. Real spectra are skewed (every record of an
// iid count has count 1): the wave first agrees on the bins its lanes hold, up
// to four of them, and one lane adds each one's popcount; lanes whose bin was
// none of those add for themselves.
__device__ __forceinline__ void histo_wave_add(u32* tab, u64* __restrict__ bins, u32 nl, u32 b, bool pend) {
    const u32 lane = lane_id();
    for (int round = 0; round < 4; round++) {
        const u64 m = __ballot(pend);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const u32 v = __shfl(b, leader);
        const bool same = pend && b == v;
        const u64 sm = __ballot(same);
        if ((int)lane == leader) histo_add(tab, bins, nl, v, (u32)__popcll(sm));
        pend = pend && !same;
    }
    if (pend) histo_add(tab, bins, nl, b, 1u);
}

__global__ __launch_bounds__(kBlock) void count_histo_k(const u32* __restrict__ recs, u64 n, int RW, u32 n_bins,
                                                        u64* __restrict__ bins, u64 nspans) {
    __shared__ u32 tab[kHistLds];
    const u32 tid = threadIdx.x;
    const u32 nl = n_bins < (u32)kHistLds ? n_bins : (u32)kHistLds;
    const u32 last = n_bins - 1;
    for (u64 sp = blockIdx.x; sp < nspans; sp += gridDim.x) {
        for (u32 b = tid; b < nl; b += kBlock) tab[b] = 0;
        __syncthreads();
        const u64 base = sp * (u64)kHistSpan;
        const u64 left = n - base;
        const u32 rem = le64_32(left, (u32)kHistSpan) ? (u32)left : (u32)kHistSpan;
        for (u32 o = 0; o < rem; o += 4 * kBlock) {
            u32 b[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const u32 r = o + u * kBlock + tid;
                ok[u] = r < rem;
                u32 c = 0;
                if (ok[u]) c = recs[(base + r) * (u64)RW + (u64)(RW - 1)];
                b[u] = c < last ? c : last;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) histo_wave_add(tab, bins, nl, b[u], ok[u]);
        }
        __syncthreads();
        for (u32 b = tid; b < nl; b += kBlock) {
            const u32 v = tab[b];
            if (v) atomicAdd((unsigned long long*)&bins[b], (unsigned long long)v);
        }
        __syncthreads();
    }
}

hipError_t launch_count_histo(const void* packed, int W, uint64_t n, uint32_t n_bins, uint64_t* bins,
                              hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (W < 1 || W > 4 || n_bins < 2) return hipErrorInvalidValue;
    const u64 nspans = (n + kHistSpan - 1) / kHistSpan;
    hipLaunchKernelGGL(count_histo_k, dim3((u32)hmin(nspans, 2048)), dim3(kBlock), 0, s, (const u32*)packed, n,
                       2 * W + 1, n_bins, bins, nspans);
    return hipGetLastError();
}

// Count-range filter: order-preserving compaction in three launches (kept
// records per tile, exclusive scan of the tile counts, scatter). Thread t of a
// tile holds records j * kBlock + t, j < 4, so a kept record's place in the
// tile is the kept records of earlier rounds and lower waves plus the kept
// lower lanes of its own ballot.
constexpr int kFilterTile = kBlock * 4;

uint64_t filter_tile() { return kFilterTile; }

__global__ __launch_bounds__(kBlock) void filter_count_k(const u32* __restrict__ recs, u64 n, int RW, u32 lo, u32 hi,
                                                         u64 ntiles, u64* __restrict__ tile_cnt) {
    __shared__ u32 wc[kBlock / kWave];
    const u32 tid = threadIdx.x;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        u32 mine = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u64 i = t * (u64)kFilterTile + (u64)(j * kBlock) + tid;
            if (i < n) {
                const u32 c = recs[i * (u64)RW + (u64)(RW - 1)];
                mine += (c >= lo && c <= hi) ? 1u : 0u;
            }
        }
        for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o);
        if (lane_id() == 0) wc[tid >> 6] = mine;
        __syncthreads();
        if (tid == 0) tile_cnt[t] = (u64)(wc[0] + wc[1] + wc[2] + wc[3]);
        __syncthreads();
    }
}

// The tile's kept records are compacted through LDS as dwords and leave as
// consecutive dwords from tile_base[t] * RW (coalesced whatever the record size).
__global__ __launch_bounds__(kBlock) void filter_scatter_k(const u32* __restrict__ recs, u64 n, int RW, u32 lo, u32 hi,
                                                           u64 ntiles, const u64* __restrict__ tile_base,
                                                           u32* __restrict__ out) {
    extern __shared__ u32 filter_stage[];  // kFilterTile * RW dwords
    __shared__ u32 wc[4][kBlock / kWave];
    const u32 tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        bool keep[4];
        u32 rank[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u64 i = t * (u64)kFilterTile + (u64)(j * kBlock) + tid;
            keep[j] = false;
            if (i < n) {
                const u32 c = recs[i * (u64)RW + (u64)(RW - 1)];
                keep[j] = c >= lo && c <= hi;
            }
            const u64 m = __ballot(keep[j]);
            rank[j] = (u32)__popcll(m & lanemask_lt());
            if (lane == 0) wc[j][wave] = (u32)__popcll(m);
        }
        __syncthreads();
        u32 run = 0, off[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (u32 w = 0; w < kBlock / kWave; w++) {
                if (w == wave) off[j] = run;
                run += wc[j][w];
            }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (keep[j]) {
                const u64 i = t * (u64)kFilterTile + (u64)(j * kBlock) + tid;
                const u32* __restrict__ src = recs + i * (u64)RW;
                u32* dst = filter_stage + (off[j] + rank[j]) * (u32)RW;
                for (int d = 0; d < RW; d++) dst[d] = src[d];
            }
        }
        __syncthreads();
        const u32 nd = run * (u32)RW;
        u32* __restrict__ o = out + tile_base[t] * (u64)RW;
        for (u32 d = tid; d < nd; d += kBlock) o[d] = filter_stage[d];
        __syncthreads();
    }
}

hipError_t launch_filter_count(const void* packed, int W, uint64_t n, uint32_t lo, uint32_t hi, uint64_t* tile_cnt,
                               hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (W < 1 || W > 4) return hipErrorInvalidValue;
    const u64 ntiles = (n + kFilterTile - 1) / kFilterTile;
    hipLaunchKernelGGL(filter_count_k, dim3((u32)hmin(ntiles, 8192)), dim3(kBlock), 0, s, (const u32*)packed, n,
                       2 * W + 1, lo, hi, ntiles, tile_cnt);
    return hipGetLastError();
}

hipError_t launch_filter_scatter(const void* packed, int W, uint64_t n, uint32_t lo, uint32_t hi,
                                 const uint64_t* tile_base, void* out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (W < 1 || W > 4) return hipErrorInvalidValue;
    const u64 ntiles = (n + kFilterTile - 1) / kFilterTile;
    const size_t lds = (size_t)kFilterTile * (2 * W + 1) * sizeof(u32);
    hipLaunchKernelGGL(filter_scatter_k, dim3((u32)hmin(ntiles, 8192)), dim3(kBlock), lds, s, (const u32*)packed, n,
                       2 * W + 1, lo, hi, ntiles, tile_base, (u32*)out);
    return hipGetLastError();
}

// Point lookup: one lane per query, a lower bound over the run (64-bit index)
// in the file's order — word 0 first, unsigned (KMerFileMerger.cpp:98-108).
template <int W>
__global__ __launch_bounds__(kBlock) void lookup_k(const u32* __restrict__ recs, u64 n, const u64* __restrict__ keys,
                                                   u64 nq, u32* __restrict__ counts, uint8_t* __restrict__ found,
                                                   u64* __restrict__ n_found) {
    constexpr int RW = 2 * W + 1;
    __shared__ u32 wc[kBlock / kWave];
    const u32 tid = threadIdx.x;
    u32 mine = 0;
    for (u64 q = (u64)blockIdx.x * kBlock + tid; q < nq; q += (u64)gridDim.x * kBlock) {
        u64 k[W];
#pragma unroll
        for (int j = 0; j < W; j++) k[j] = keys[q * W + j];
        u64 lo = 0, hi = n;
        while (lo < hi) {
            const u64 mid = lo + ((hi - lo) >> 1);
            const u32* __restrict__ p = recs + mid * (u64)RW;
            bool less = false, decided = false;  // record key < query key
#pragma unroll
            for (int j = 0; j < W; j++) {
                const u64 w = (u64)p[2 * j] | ((u64)p[2 * j + 1] << 32);
                if (!decided && w != k[j]) {
                    less = w < k[j];
                    decided = true;
                }
            }
            if (less)
                lo = mid + 1;
            else
                hi = mid;
        }
        bool f = false;
        u32 c = 0;
        if (lo < n) {
            const u32* __restrict__ p = recs + lo * (u64)RW;
            f = true;
#pragma unroll
            for (int j = 0; j < W; j++) f = f && ((u64)p[2 * j] | ((u64)p[2 * j + 1] << 32)) == k[j];
            if (f) c = p[2 * W];
        }
        counts[q] = c;
        if (found) found[q] = f ? 1 : 0;
        mine += f ? 1u : 0u;
    }
    for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o);
    if (lane_id() == 0) wc[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) {
        const u32 tot = wc[0] + wc[1] + wc[2] + wc[3];
        if (tot) atomicAdd((unsigned long long*)n_found, (unsigned long long)tot);
    }
}

hipError_t launch_lookup(const void* packed, int W, uint64_t n, const uint64_t* keys, uint64_t nq, uint32_t* counts,
                         uint8_t* found, uint64_t* n_found, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    const int g = grid_for(nq);
#define KC_LK(WW)                                                                                             \
    hipLaunchKernelGGL(lookup_k<WW>, dim3(g), dim3(kBlock), 0, s, (const u32*)packed, n, (const u64*)keys, nq, \
                       counts, found, n_found)
    if (const hipError_t bad = dispatch_w<4>(W, [&](auto w) { KC_LK(decltype(w)::value); })) return bad;
#undef KC_LK
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Canonical fold of the finished run: every record's key becomes
// the smaller of the k-mer and its reverse complement. A record whose own key
// is the smaller one ("stays") keeps its place among the staying records, so
// only the others ("flipped") need a sort: one counting pass, a scan of the
// tile counts, and one split pass that compacts the staying records (packed,
// in order) and writes the flipped ones (SoA, with their new keys) for the
// radix sort. Tiles, dword reads and ballot ranks as the filter above; no
// workgroup waits on another.
// ---------------------------------------------------------------------------

// The 32 two-bit groups of x in reverse order (bits reversed, then the two
// bits of each pair swapped back).
__device__ __forceinline__ u64 rev_groups(u64 x) {
    const u64 y = __builtin_bitreverse64(x);
    return ((y & 0xaaaaaaaaaaaaaaaaull) >> 1) | ((y & 0x5555555555555555ull) << 1);
}

// rec: one packed record's dwords; s = 64 W - 2 k pad bits (0..62). m: the key
// with every base from position k on cleared; r: the reverse complement of its
// k bases, left-aligned and zero below. Returns stay = (m <= r), word 0 first.
template <int W>
__device__ __forceinline__ bool canon_keys(const u32* __restrict__ rec, u32 s, u64 (&m)[W], u64 (&r)[W]) {
#pragma unroll
    for (int j = 0; j < W; j++) m[j] = (u64)rec[2 * j] | ((u64)rec[2 * j + 1] << 32);
    m[W - 1] &= ~0ull << s;  // s <= 62
    u64 t[W];
#pragma unroll
    for (int j = 0; j < W; j++) t[j] = ~rev_groups(m[W - 1 - j]);
    // left shift across the words by s: the pad's complement falls out of
    // word 0, zeros come in below (s == 0 would be a shift by 64: no shift)
#pragma unroll
    for (int j = 0; j < W; j++) {
        const u64 below = j + 1 < W ? t[j + 1] : 0ull;
        r[j] = s ? (t[j] << s) | (below >> (64u - s)) : t[j];
    }
    bool stay = true, decided = false;
#pragma unroll
    for (int j = 0; j < W; j++)
        if (!decided && m[j] != r[j]) {
            stay = m[j] < r[j];
            decided = true;
        }
    return stay;
}

template <int W>
__global__ __launch_bounds__(kBlock) void canon_count_k(const u32* __restrict__ recs, u64 n, u32 s, u64 ntiles,
                                                        u64* __restrict__ tile_cnt) {
    constexpr int RW = 2 * W + 1;
    __shared__ u32 wc[kBlock / kWave];
    const u32 tid = threadIdx.x;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        u32 mine = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u64 i = t * (u64)kFilterTile + (u64)(j * kBlock) + tid;
            if (i < n) {
                u64 m[W], r[W];
                mine += canon_keys<W>(recs + i * (u64)RW, s, m, r) ? 1u : 0u;
            }
        }
        for (int o = 32; o >= 1; o >>= 1) mine += __shfl_xor(mine, o);
        if (lane_id() == 0) wc[tid >> 6] = mine;
        __syncthreads();
        if (tid == 0) tile_cnt[t] = (u64)(wc[0] + wc[1] + wc[2] + wc[3]);
        __syncthreads();
    }
}

// Tile t's staying records (key m, same count) are compacted through LDS and
// leave as consecutive dwords from stay_base[t] * RW; its flipped records (key
// r, same count) go to the SoA arrays at t * kFilterTile - stay_base[t] + their
// rank among the tile's flipped records. Both keep the tile's record order.
template <int W>
__global__ __launch_bounds__(kBlock) void canon_split_k(const u32* __restrict__ recs, u64 n, u32 s, u64 ntiles,
                                                        const u64* __restrict__ stay_base, u32* __restrict__ stay_out,
                                                        u64* __restrict__ fkeys, u64 fstride,
                                                        u32* __restrict__ fcnts) {
    constexpr int RW = 2 * W + 1;
    extern __shared__ u32 canon_stage[];  // kFilterTile * RW dwords
    __shared__ u32 wcs[4][kBlock / kWave], wcf[4][kBlock / kWave];
    const u32 tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const u64 sb = stay_base[t];
        const u64 fb = t * (u64)kFilterTile - sb;
        u64 key[4][W];
        u32 cnt[4], rank[4];
        bool live[4], stay[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const u64 i = t * (u64)kFilterTile + (u64)(j * kBlock) + tid;
            live[j] = i < n;
            stay[j] = false;
            cnt[j] = 0;
            if (live[j]) {
                const u32* __restrict__ p = recs + i * (u64)RW;
                u64 m[W], r[W];
                stay[j] = canon_keys<W>(p, s, m, r);
                cnt[j] = p[2 * W];
#pragma unroll
                for (int w = 0; w < W; w++) key[j][w] = stay[j] ? m[w] : r[w];
            }
            const bool flip = live[j] && !stay[j];
            const u64 ms = __ballot(stay[j]), mf = __ballot(flip);
            rank[j] = (u32)__popcll((stay[j] ? ms : mf) & lanemask_lt());
            if (lane == 0) {
                wcs[j][wave] = (u32)__popcll(ms);
                wcf[j][wave] = (u32)__popcll(mf);
            }
        }
        __syncthreads();
        u32 runs = 0, runf = 0, offs[4] = {0, 0, 0, 0}, offf[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (u32 w = 0; w < kBlock / kWave; w++) {
                if (w == wave) {
                    offs[j] = runs;
                    offf[j] = runf;
                }
                runs += wcs[j][w];
                runf += wcf[j][w];
            }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!live[j]) continue;
            if (stay[j]) {
                u32* dst = canon_stage + (offs[j] + rank[j]) * (u32)RW;
#pragma unroll
                for (int w = 0; w < W; w++) {
                    dst[2 * w] = (u32)key[j][w];
                    dst[2 * w + 1] = (u32)(key[j][w] >> 32);
                }
                dst[2 * W] = cnt[j];
            } else {
                const u64 at = fb + (u64)(offf[j] + rank[j]);
#pragma unroll
                for (int w = 0; w < W; w++) fkeys[(u64)w * fstride + at] = key[j][w];
                fcnts[at] = cnt[j];
            }
        }
        __syncthreads();
        const u32 nd = runs * (u32)RW;
        u32* __restrict__ o = stay_out + sb * (u64)RW;
        for (u32 d = tid; d < nd; d += kBlock) o[d] = canon_stage[d];
        __syncthreads();
    }
}

static bool canon_args_ok(int W, int k) { return W >= 1 && W <= 4 && k >= 1 && (k + 31) / 32 == W; }

hipError_t launch_canon_count(const void* packed, int W, int k, uint64_t n, uint64_t* tile_cnt, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (!canon_args_ok(W, k)) return hipErrorInvalidValue;
    const u64 ntiles = (n + kFilterTile - 1) / kFilterTile;
    const u32 pad = (u32)(64 * W - 2 * k);
#define KC_CNC(WW)                                                                                              \
    hipLaunchKernelGGL(canon_count_k<WW>, dim3((u32)hmin(ntiles, 8192)), dim3(kBlock), 0, s, (const u32*)packed, \
                       n, pad, ntiles, tile_cnt)
    if (const hipError_t bad = dispatch_w<4>(W, [&](auto w) { KC_CNC(decltype(w)::value); })) return bad;
#undef KC_CNC
    return hipGetLastError();
}

hipError_t launch_canon_split(const void* packed, int W, int k, uint64_t n, const uint64_t* stay_base, void* stay_out,
                              uint64_t* flip_keys, uint64_t flip_stride, uint32_t* flip_cnts, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (!canon_args_ok(W, k)) return hipErrorInvalidValue;
    const u64 ntiles = (n + kFilterTile - 1) / kFilterTile;
    const u32 pad = (u32)(64 * W - 2 * k);
    const size_t lds = (size_t)kFilterTile * (2 * W + 1) * sizeof(u32);
#define KC_CNS(WW)                                                                                                \
    hipLaunchKernelGGL(canon_split_k<WW>, dim3((u32)hmin(ntiles, 8192)), dim3(kBlock), lds, s, (const u32*)packed, \
                       n, pad, ntiles, (const u64*)stay_base, (u32*)stay_out, (u64*)flip_keys, (u64)flip_stride,   \
                       flip_cnts)
    if (const hipError_t bad = dispatch_w<4>(W, [&](auto w) { KC_CNS(decltype(w)::value); })) return bad;
#undef KC_CNS
    return hipGetLastError();
}
