// kc_radix.inl — the radix grouping passes (rp_*). Included by kc_kernels.hip
// inside namespace kc: it uses kc_common.inl's lane_id, hmin, dispatch_w and
// grid_for.
//
// One pass groups items by one byte of word 0. Items are NW u64 words, SoA
// (word j of item i at kin[j * stride + i]) or AoS (stride 0: NW consecutive
// words), with an optional u32 payload; the digit is (word0 >> dshift) & 255,
// and the scatter can emit another byte of word 0 per item (the next pass's
// digit, so that pass's histogram reads 1 B per item instead of word 0).
// Callers: the partition engine's P3 (digit bits 56..63 over the 256 P2
// regions) and P3b (bits 40..47 inside each of the 65536 buckets), and
// group16 of the skm engine and of the finish (two passes over word0 >> 48).
//
// Regions and tiles (RegionTable): the input is nreg regions
// [rstart[r], rstart[r + 1]), each cut into tiles of its own (a tile never
// straddles two regions): region r holds tiles [tpre[r], tpre[r + 1]), tile
// i of r starts at rstart[r] + i * TILE, TILE = rp_tile(NW, pay). A first
// pass has one region; a second pass takes the first one's 256 digit runs.
//
// A pass is a histogram and a scatter:
//   rp_upsweep_k    tile-major counts cnt[t][d] of every tile
//   positions       pos[t][d], the global start of tile t's run of digit d:
//     LSD (launch_rp_hist): digit-major over region-ordered tiles, pos[t][d]
//       = sum_{d' < d} total(d') + sum_{t' < t} cnt[t'][d]. Over the 256
//       regions of an earlier pass this is (this digit, earlier digit) order,
//       which for P3 is exactly bucket start + offset.
//     regional (launch_rp_hist_regional, MSD): runs placed inside their own
//       region, so regions stay in order and each is sorted by the digit;
//       launch_sub_starts then lists the nreg * 256 sub-region starts.
//   rp_scatter_k    one workgroup (kRpBlock threads) per tile: the tile's items are
//     ranked by digit in LDS and written out as 256 runs long enough to fill
//     whole lines; the next tile's items and run starts are prefetched into
//     registers. Ranks inside a tile are unstable (plain LDS atomics, no
//     ballots): only grouping is needed (records, and the keys of one group
//     are distinct or summed later).

// radix-scatter LDS budget per workgroup (items) and workgroups per CU
#ifndef KC_RP_LDS
#define KC_RP_LDS 143808
#endif
#ifndef KC_RP_WPC
#define KC_RP_WPC 1
#endif

// threads per radix-scatter workgroup (variant builds: KC_RP_BLOCK=512 with
// KC_RP_WPC=2 and half the LDS budget runs two workgroups per CU)
#ifndef KC_RP_BLOCK
#define KC_RP_BLOCK 1024
#endif
constexpr int kRpBlock = KC_RP_BLOCK;
constexpr int kRpWaves = kRpBlock / 64;

template <int NW, bool PAY>
struct RpCfg {
    static constexpr int BYTES = 8 * NW + (PAY ? 4 : 0);
    static constexpr int K0 = KC_RP_LDS / (BYTES * kRpBlock);
    static constexpr int KPT = K0 > 16 ? 16 : K0;
    static constexpr int TILE = kRpBlock * KPT;
};

int rp_tile(int NW, bool pay) {
    const int bytes = 8 * NW + (pay ? 4 : 0);
    int kpt = KC_RP_LDS / (bytes * kRpBlock);
    if (kpt > 16) kpt = 16;
    return kRpBlock * kpt;
}

__device__ __forceinline__ void rp_tile_range(const u64* __restrict__ rstart, const u64* __restrict__ tpre, int nreg,
                                              u64 t, u64 TILE, u64* lo, u64* hi) {
    int a = 0, b = nreg;  // region r with tpre[r] <= t < tpre[r+1]
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (tpre[mid] <= t)
            a = mid;
        else
            b = mid;
    }
    const u64 st = rstart[a] + (t - tpre[a]) * TILE;
    *lo = st;
    *hi = min(st + TILE, rstart[a + 1]);
}

// Tile histograms (tile-major u32 counts): digit = digs[i] when digs is given,
// else (w0[i] >> shift) & 255.
__global__ __launch_bounds__(kBlock) void rp_upsweep_k(const unsigned char* __restrict__ digs,
                                                       const u64* __restrict__ w0, int shift,
                                                       const u64* __restrict__ rstart, const u64* __restrict__ tpre,
                                                       int nreg, u64 ntiles, u32 TILE, u32* __restrict__ cnt_t) {
    __shared__ u32 h[4 * 256];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        for (int i = tid; i < 4 * 256; i += kBlock) h[i] = 0;
        __syncthreads();
        u64 lo, hi;
        rp_tile_range(rstart, tpre, nreg, t, TILE, &lo, &hi);
        u32* hw = h + wave * 256;
        if (digs) {
            // 16-byte loads from the first 16-byte aligned address on
            const u64 alo = min(hi, lo + ((16u - (u32)((uintptr_t)(digs + lo) & 15u)) & 15u));
            for (u64 i = lo + tid; i < alo; i += kBlock) atomicAdd(&hw[digs[i]], 1u);
            const u64 ahi = alo + ((hi - alo) & ~15ull);
            for (u64 i = alo + 16 * (u64)tid; i < ahi; i += 16 * (u64)kBlock) {
                const v4u v = __builtin_nontemporal_load((const v4u*)(digs + i));
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const u32 x = c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w));
                    atomicAdd(&hw[x & 255u], 1u);
                    atomicAdd(&hw[(x >> 8) & 255u], 1u);
                    atomicAdd(&hw[(x >> 16) & 255u], 1u);
                    atomicAdd(&hw[x >> 24], 1u);
                }
            }
            for (u64 i = ahi + tid; i < hi; i += kBlock) atomicAdd(&hw[digs[i]], 1u);
        } else {
            for (u64 i = lo + tid; i < hi; i += kBlock)
                atomicAdd(&hw[(u32)(__builtin_nontemporal_load(w0 + i) >> shift) & 255u], 1u);
        }
        __syncthreads();
        cnt_t[t * 256 + tid] = h[tid] + h[256 + tid] + h[512 + tid] + h[768 + tid];
        __syncthreads();
    }
}

// Positions from the tile-major counts, digit-major order: pos[t][d] =
// sum_{d' < d} total(d') + sum_{t' < t} cnt[t'][d], in three streaming kernels
// over chunks of kRpChunk tiles (rows of 256 counts are read coalesced).
constexpr int kRpChunk = 64;

__global__ __launch_bounds__(256) void rp_chunk_sum_k(const u32* __restrict__ cnt_t, u64 ntiles, u64* __restrict__ csum) {
    const u64 c = blockIdx.x;
    const u64 t0 = c * kRpChunk, t1 = min(ntiles, t0 + kRpChunk);
    u64 sum = 0;
    for (u64 t = t0; t < t1; t++) sum += cnt_t[t * 256 + threadIdx.x];
    csum[c * 256 + threadIdx.x] = sum;
}

// one block per digit: exclusive scan of that digit's chunk sums (each thread
// a run of consecutive chunks); the digit total goes to dtot[d]
__global__ __launch_bounds__(256) void rp_chunk_scan_k(u64* __restrict__ csum, u64 nchunks, u64* __restrict__ dtot) {
    __shared__ u64 part[256];
    const int d = blockIdx.x, t = threadIdx.x;
    const u64 per = (nchunks + 255) / 256;
    const u64 c0 = min(nchunks, (u64)t * per), c1 = min(nchunks, c0 + per);
    u64 sum = 0;
    for (u64 c = c0; c < c1; c++) sum += csum[c * 256 + d];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        u64 acc = 0;
        for (int i = 0; i < 256; i++) {
            const u64 v = part[i];
            part[i] = acc;
            acc += v;
        }
        dtot[d] = acc;
    }
    __syncthreads();
    u64 run = part[t];
    for (u64 c = c0; c < c1; c++) {
        const u64 v = csum[c * 256 + d];
        csum[c * 256 + d] = run;
        run += v;
    }
}

__global__ __launch_bounds__(256) void rp_digit_base_k(u64* __restrict__ dtot) {
    if (threadIdx.x == 0) {
        u64 acc = 0;
        for (int i = 0; i < 256; i++) {
            const u64 v = dtot[i];
            dtot[i] = acc;
            acc += v;
        }
    }
}

__global__ __launch_bounds__(256) void rp_chunk_pos_k(const u32* __restrict__ cnt_t, const u64* __restrict__ csum,
                                                      const u64* __restrict__ dbase, u64 ntiles, u64* __restrict__ pos) {
    const u64 c = blockIdx.x;
    const u64 t0 = c * kRpChunk, t1 = min(ntiles, t0 + kRpChunk);
    u64 run = dbase[threadIdx.x] + csum[c * 256 + threadIdx.x];
    for (u64 t = t0; t < t1; t++) {
        pos[t * 256 + threadIdx.x] = run;
        run += cnt_t[t * 256 + threadIdx.x];
    }
}

// MSD form of the regional histogram: digit runs are placed inside their
// region (region start + the region's smaller digits + the region's earlier
// tiles), so a pass sorts every region by the digit and regions stay in
// order (the chunk kernels above are LSD: digit-major over all regions).
// One 256-thread workgroup (one thread per digit) per region.
__global__ __launch_bounds__(256) void rp_region_pos_k(const u32* __restrict__ cnt_t, const u64* __restrict__ rstart,
                                                       const u64* __restrict__ tpre, u32 nreg, u64* __restrict__ pos) {
    __shared__ u64 part[256];
    const int d = threadIdx.x;
    for (u32 r = blockIdx.x; r < nreg; r += gridDim.x) {
        const u64 t0 = tpre[r], t1 = tpre[r + 1];
        u64 sum = 0;
        for (u64 t = t0; t < t1; t++) sum += cnt_t[t * 256 + d];
        part[d] = sum;
        __syncthreads();
        // exclusive scan over the 256 digits (Hillis-Steele in LDS)
        for (int o = 1; o < 256; o <<= 1) {
            const u64 y = d >= o ? part[d - o] : 0ull;
            __syncthreads();
            part[d] += y;
            __syncthreads();
        }
        u64 run = rstart[r] + part[d] - sum;
        for (u64 t = t0; t < t1; t++) {
            pos[t * 256 + d] = run;
            run += cnt_t[t * 256 + d];
        }
        __syncthreads();
    }
}

// KC_RP_ABL (timing ablations of tools/rp_bench, variant builds only): bit 1
// no global stores, bit 2 no ranking / LDS scatter, bit 4 no global loads
#ifndef KC_RP_ABL
#define KC_RP_ABL 0
#endif

template <int NW, bool PAY>
__global__ __launch_bounds__(kRpBlock) void rp_scatter_k(const u64* __restrict__ kin, u64 istride,
                                                         u64* __restrict__ kout, u64 ostride,
                                                         const u32* __restrict__ pin, u32* __restrict__ pout,
                                                         const u64* __restrict__ rstart, const u64* __restrict__ tpre,
                                                         int nreg, u64 ntiles, const u64* __restrict__ pos,
                                                         int dshift, unsigned char* __restrict__ emit, int eshift) {
    constexpr int KPT = RpCfg<NW, PAY>::KPT;
    constexpr int TILE = RpCfg<NW, PAY>::TILE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* skey = (u64*)smem;                                    // NW x TILE
    u32* spay = (u32*)(skey + (size_t)NW * TILE);              // TILE (PAY)
    u32* wc = spay + (PAY ? TILE : 0);                         // kRpWaves x 128 words: two u16 counters each
    unsigned short* woff = (unsigned short*)(wc + kRpWaves * 128);  // kRpWaves x 256
    u32* dst = (u32*)(woff + kRpWaves * 256);                        // 256 digit starts in the tile
    u64* gpos = (u64*)(dst + 256);                             // 256 global run starts
    u32* wsum = (u32*)(gpos + 256);                            // 16
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    u64 nk[KPT][NW];
    u32 np[KPT];
    // tiles: with a grid of 8k workgroups, XCD x (blocks b = x mod 8) walks
    // the x-th eighth of the tiles, 8k/8 consecutive tiles at a time, so the
    // digit runs that land next to each other in the output are written
    // through the same L2 (partial lines merge there); else block b walks
    // b, b + grid, ...
    const bool xcd_map = (gridDim.x & 7u) == 0u && ntiles >= 8;
    const u64 step = xcd_map ? (u64)(gridDim.x >> 3) : (u64)gridDim.x;
    const u64 tx = (ntiles + 7) >> 3;
    const u64 t_first = xcd_map ? (u64)(blockIdx.x & 7u) * tx + (blockIdx.x >> 3) : (u64)blockIdx.x;
    const u64 t_end = xcd_map ? min(ntiles, (u64)((blockIdx.x & 7u) + 1) * tx) : ntiles;
    auto load = [&](u64 t) {
        if (t >= t_end) return;
        u64 lo = 0, hi = 0;
        rp_tile_range(rstart, tpre, nreg, t, TILE, &lo, &hi);
        // unconditional loads (clamped into the tile, which is never empty):
        // a per-element select on a load makes hipcc wait for each one
#pragma unroll
        for (int i = 0; i < KPT; i++) {
            const u64 q = min(lo + (u64)i * kRpBlock + tid, hi - 1);
            if (istride == 0) {  // AoS items (uniform branch)
                if constexpr (NW == 2) {
                    const v2u64 v = __builtin_nontemporal_load((const v2u64*)(kin + 2 * q));
                    nk[i][0] = v.x;
                    nk[i][1] = v.y;
                } else {
#pragma unroll
                    for (int j = 0; j < NW; j++) nk[i][j] = __builtin_nontemporal_load(kin + q * NW + j);
                }
            } else {
#pragma unroll
                for (int j = 0; j < NW; j++)
                    nk[i][j] = (KC_RP_ABL & 4) ? (q + 1) * 0x9e3779b97f4a7c15ull * (j + 1)
                                               : __builtin_nontemporal_load(kin + (u64)j * istride + q);
            }
            if constexpr (PAY) np[i] = (KC_RP_ABL & 4) ? (u32)q : __builtin_nontemporal_load(pin + q);
        }
    };
    load(t_first);
    // this tile's 256 global run starts, loaded one tile ahead like the items
    u64 npos = (tid < 256 && t_first < t_end) ? pos[t_first * 256 + tid] : 0ull;
    for (u64 t = t_first; t < t_end; t += step) {
        u64 lo, hi;
        rp_tile_range(rstart, tpre, nreg, t, TILE, &lo, &hi);
        const u32 len = (u32)(hi - lo);
        u64 key[KPT][NW];
        u32 pv[KPT];
#pragma unroll
        for (int i = 0; i < KPT; i++) {
#pragma unroll
            for (int j = 0; j < NW; j++) key[i][j] = nk[i][j];
            pv[i] = PAY ? np[i] : 0u;
        }
        for (int i = tid; i < kRpWaves * 128; i += kRpBlock) wc[i] = 0;
        if (tid < 256) gpos[tid] = npos;
        __syncthreads();
        load(t + step);
        if (tid < 256 && t + step < t_end) npos = pos[(t + step) * 256 + tid];
        u32 rank[KPT];
#pragma unroll
        for (int i = 0; i < KPT; i++) {
            const u32 q = (u32)i * kRpBlock + (u32)tid;
            rank[i] = 0;
            if (q < len && !(KC_RP_ABL & 2)) {
                const u32 d = (u32)(key[i][0] >> dshift) & 255u;
                const u32 sh = 16 * (d & 1);
                rank[i] = (atomicAdd(&wc[wave * 128 + (d >> 1)], 1u << sh) >> sh) & 0xffffu;
            }
        }
        __syncthreads();
        if (tid < 256) {
            u32 run = 0;
            for (int w = 0; w < kRpWaves; w++) {
                woff[w * 256 + tid] = (unsigned short)run;
                run += (wc[w * 128 + (tid >> 1)] >> (16 * (tid & 1))) & 0xffffu;
            }
            const u32 v = run;
            u32 inc = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u32 y = __shfl_up(inc, o);
                if (lane >= o) inc += y;
            }
            if (lane == 63) wsum[wave] = inc;
            dst[tid] = inc - v;
        }
        __syncthreads();
        if (tid < 256) {
            u32 add = 0;
            for (int w = 0; w < wave; w++) add += wsum[w];
            dst[tid] += add;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KPT; i++) {
            const u32 q = (u32)i * kRpBlock + (u32)tid;
            if (q < len && !(KC_RP_ABL & 2)) {
                const u32 d = (u32)(key[i][0] >> dshift) & 255u;
                const u32 at = dst[d] + woff[wave * 256 + d] + rank[i];
#pragma unroll
                for (int j = 0; j < NW; j++) skey[(size_t)j * TILE + at] = key[i][j];
                if constexpr (PAY) spay[at] = pv[i];
            }
        }
        __syncthreads();
        for (u32 q = tid; q < len; q += kRpBlock) {
            const u64 k0 = skey[q];
            const u32 d = (u32)(k0 >> dshift) & 255u;
            const u64 g = gpos[d] + (q - dst[d]);
            if (KC_RP_ABL & 1) {
                if (g == ~0ull) kout[0] = k0;  // keeps the work, writes nothing
                continue;
            }
            if (ostride == 0) {  // AoS output (uniform branch)
                if constexpr (NW == 2) {
                    v2u64 v;
                    v.x = k0;
                    v.y = skey[(size_t)TILE + q];
                    *(v2u64*)(kout + 2 * g) = v;
                } else {
                    kout[g * NW] = k0;
#pragma unroll
                    for (int j = 1; j < NW; j++) kout[g * NW + j] = skey[(size_t)j * TILE + q];
                }
            } else {
                kout[g] = k0;
#pragma unroll
                for (int j = 1; j < NW; j++) kout[(u64)j * ostride + g] = skey[(size_t)j * TILE + q];
            }
            if constexpr (PAY) pout[g] = spay[q];
            if (emit) emit[g] = (unsigned char)(k0 >> eshift);
        }
        __syncthreads();
    }
}

static size_t rp_scatter_lds(int NW, bool pay) {
    const size_t tile = (size_t)rp_tile(NW, pay);
    return (size_t)NW * tile * 8 + (pay ? tile * 4 : 0) + kRpWaves * 128 * 4 + kRpWaves * 256 * 2 + 256 * 4 +
           256 * 8 + 16 * 4 + 16;
}

u64* rp_digit_base(u64* tmp, uint64_t ntiles) {
    const u64 nchunks = (ntiles + kRpChunk - 1) / kRpChunk;
    return tmp + (ntiles * 256 + 1) / 2 + nchunks * 256;
}

uint64_t rp_tmp_elems(uint64_t ntiles) {
    return (ntiles * 256 + 1) / 2 + ((ntiles + kRpChunk - 1) / kRpChunk) * 256 + 256 + 8;
}

hipError_t launch_rp_hist(const uint8_t* digs, const uint64_t* w0, int shift, const RegionTable& rt, uint64_t* pos,
                          uint64_t* tmp, int grid, hipStream_t s) {
    const uint64_t ntiles = rt.ntiles;
    if (ntiles == 0) return hipSuccess;
    u32* cnt_t = (u32*)tmp;
    u64* csum = tmp + (ntiles * 256 + 1) / 2;
    const u64 nchunks = (ntiles + kRpChunk - 1) / kRpChunk;
    u64* dtot = csum + nchunks * 256;
    const int gu = (int)hmin(ntiles, (u64)grid * 4);
    hipLaunchKernelGGL(rp_upsweep_k, dim3(gu), dim3(kBlock), 0, s, (const unsigned char*)digs, w0, shift,
                       rt.rstart, rt.tpre, rt.nreg, ntiles, rt.tile, cnt_t);
    hipLaunchKernelGGL(rp_chunk_sum_k, dim3(nchunks), dim3(256), 0, s, (const u32*)cnt_t, ntiles, csum);
    hipLaunchKernelGGL(rp_chunk_scan_k, dim3(256), dim3(256), 0, s, csum, nchunks, dtot);
    hipLaunchKernelGGL(rp_digit_base_k, dim3(1), dim3(256), 0, s, dtot);
    hipLaunchKernelGGL(rp_chunk_pos_k, dim3(nchunks), dim3(256), 0, s, (const u32*)cnt_t, (const u64*)csum,
                       (const u64*)dtot, ntiles, pos);
    return hipGetLastError();
}

hipError_t launch_rp_hist_regional(const uint64_t* w0, int shift, const RegionTable& rt, uint64_t* pos,
                                   uint32_t* cnt_t, int grid, hipStream_t s, const uint8_t* digs) {
    const uint64_t ntiles = rt.ntiles;
    if (ntiles == 0) return hipSuccess;
    const int gu = (int)hmin(ntiles, (u64)grid * 4);
    // digs: the digit byte of every item, written by the pass that placed
    // them (1 B read per item instead of word 0)
    hipLaunchKernelGGL(rp_upsweep_k, dim3(gu), dim3(kBlock), 0, s, (const unsigned char*)digs, digs ? nullptr : w0,
                       shift, rt.rstart, rt.tpre, rt.nreg, ntiles, rt.tile, cnt_t);
    hipLaunchKernelGGL(rp_region_pos_k, dim3((u32)hmin((u64)rt.nreg, 65536)), dim3(256), 0, s, (const u32*)cnt_t,
                       rt.rstart, rt.tpre, (u32)rt.nreg, pos);
    return hipGetLastError();
}

hipError_t launch_rp_scatter(int NW, bool pay, const uint64_t* kin, uint64_t istride, uint64_t* kout,
                             uint64_t ostride, const uint32_t* pin, uint32_t* pout, const RegionTable& rt,
                             const uint64_t* pos, int dshift, uint8_t* emit, int eshift, int grid, hipStream_t s) {
    const uint64_t ntiles = rt.ntiles;
    if (ntiles == 0) return hipSuccess;
    // one persistent workgroup per CU (the LDS tile allows no second one): a
    // larger grid would run as two rounds of workgroups, each restarting its
    // prefetch pipeline
    const int g = (int)hmin(ntiles, (u64)(grid / 2 > 0 ? KC_RP_WPC * grid / 2 : 1));
    const size_t lds = (rp_scatter_lds(NW, pay) + 15) & ~(size_t)15;
#define KC_RPS(NWV, PAYV)                                                                                          \
    hipLaunchKernelGGL((rp_scatter_k<NWV, PAYV>), dim3(g), dim3(kRpBlock), lds, s, kin, istride, kout, ostride, pin, \
                       pout, rt.rstart, rt.tpre, rt.nreg, ntiles, pos, dshift, (unsigned char*)emit, eshift)
    if (pay) {
        if (const hipError_t bad = dispatch_w<4>(NW, [&](auto w) { KC_RPS(decltype(w)::value, true); })) return bad;
    } else {
        if (const hipError_t bad = dispatch_w<4>(NW, [&](auto w) { KC_RPS(decltype(w)::value, false); })) return bad;
    }
#undef KC_RPS
    return hipGetLastError();
}

// Sub-bucket starts of a pre-split partition: the regional radix pass over
// the 65536 buckets (regions) by key bits 40..47 wrote digit d of region r at
// pos[first tile of r][d], so sub-bucket r * 256 + d starts there (an empty
// region's sub-buckets start at the region's start).
__global__ __launch_bounds__(kBlock) void sub_starts_k(const u64* __restrict__ rstart, const u64* __restrict__ tpre,
                                                       const u64* __restrict__ pos, u32 nreg, u64 n,
                                                       u64* __restrict__ sub) {
    const u64 total = (u64)nreg * 256u;
    for (u64 i = (u64)blockIdx.x * kBlock + threadIdx.x; i <= total; i += (u64)gridDim.x * kBlock) {
        if (i == total) {
            sub[i] = n;
            continue;
        }
        const u32 r = (u32)(i >> 8), d = (u32)(i & 255u);
        sub[i] = tpre[r + 1] > tpre[r] ? pos[tpre[r] * 256u + d] : rstart[r];
    }
}

hipError_t launch_sub_starts(const uint64_t* rstart, const uint64_t* tpre, const uint64_t* pos, uint32_t nreg,
                             uint64_t n, uint64_t* sub, hipStream_t s) {
    const u64 total = (u64)nreg * 256u + 1;
    hipLaunchKernelGGL(sub_starts_k, dim3(grid_for(total)), dim3(kBlock), 0, s, rstart, tpre, pos, nreg, n, sub);
    return hipGetLastError();
}
