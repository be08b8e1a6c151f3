// kc_fastq.inl — K1, the FASTQ block index, in its three forms. Included by
// kc_kernels.hip inside namespace kc.
//
// Holds: the two-pass index (fq_count_k, a scan, fq_emit_k) with fq_validate_k;
//   the fused index + encode fq_encode_k<VAR, SP> for fixed and variable read
//   lengths (launch_fq_encode, launch_fq_encode_var); the one-pass speculative
//   form (launch_fq_encode_spec, fq_spec_verify_k); the KC_FQ_* build knobs.
// Uses: kc_common.inl (u32 / u64 / v4u, kBlock, lane_id, lanemask_lt,
//   FastDivU, hmin, grid_for), groups_per_read of kc_kernels.hip's E section
//   (the code layout it writes is kernel E's), and the ST_* / ERR_* counters
//   of kc_device.h.
// Host callers: kc_ingest.cpp only.

// ---------------------------------------------------------------------------
// K1: FASTQ block index. The block is viewed through 16-byte-aligned 64 KiB
// chunks of the address space; fq_count counts '\n' per chunk, a device scan
// turns counts into each chunk's first line index, and fq_emit re-reads the
// chunk and, in address order, gives every newline its line index j:
//   j % 4 == 0 (header ends)   -> seq_off[j/4] = q + 1
//   j % 4 == 1 (sequence ends) -> seq_end[j/4] = q, next byte must be '+'
//   j % 4 == 3 (quality ends)  -> next byte must be '@' (or end of block)
// For well-formed 4-line records this selects exactly the lines readData
// copies (the line before each '+' line, FASTQFileReader.cpp:57-63).
// ---------------------------------------------------------------------------

constexpr u64 kFqChunk = 16384;  // one wave: 64 lanes x 16 B x 16 iterations
constexpr int kFqWaves = kBlock / 64;

uint64_t fq_chunks(const void* base, uint64_t n) {
    u64 lead = (u64)((uintptr_t)base & 15);
    return (lead + n + kFqChunk - 1) / kFqChunk;
}

// Newline bytes of a 16-byte load as a 16-bit mask (bit b = byte b), limited
// to the bytes whose offset rel0 + b lies in [0, n).
__device__ __forceinline__ u32 nl_mask16(const uint4 v, long long rel0, u64 n) {
    u32 m = 0;
    const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
        u32 t = w[q] ^ 0x0a0a0a0au;
        u32 nz = ((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t;  // 0x80 set in non-zero bytes
        u32 z = ~nz & 0x80808080u;                      // 0x80 in '\n' bytes
#pragma unroll
        for (int b = 0; b < 4; b++)
            if (z & (0x80u << (8 * b))) m |= 1u << (4 * q + b);
    }
    if (rel0 < 0) m &= 0xffffu << (u32)(-rel0 > 16 ? 16 : -rel0);
    long long over = rel0 + 16 - (long long)n;
    if (over > 0) m &= (over >= 16) ? 0u : (0xffffu >> (u32)over);
    return m & 0xffffu;
}

// 16 bytes of the block (global address space spelled out: no FLAT load)
__device__ __forceinline__ uint4 fq_load16(uintptr_t addr) {
    const v4u w4 = *(const __attribute__((address_space(1))) v4u*)addr;
    return make_uint4(w4.x, w4.y, w4.z, w4.w);
}

// Every wave counts the newlines of its own chunks (no workgroup barrier).
__global__ __launch_bounds__(kBlock) void fq_count_k(const uint8_t* __restrict__ base, u64 n, u64 nchunks,
                                                     u64* __restrict__ counts) {
    const uintptr_t A = (uintptr_t)base & ~(uintptr_t)15;
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (u64 c = (u64)blockIdx.x * kFqWaves + wave; c < nchunks; c += (u64)gridDim.x * kFqWaves) {
        u32 cnt = 0;
#pragma unroll 4
        for (int it = 0; it < 16; it++) {
            const uintptr_t addr = A + c * kFqChunk + (u64)it * 1024 + (u64)lane * 16;
            const long long rel0 = (long long)(addr - (uintptr_t)base);
            if (rel0 + 16 <= 0 || rel0 >= (long long)n) continue;
            cnt += __popc(nl_mask16(fq_load16(addr), rel0, n));
        }
        for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0) counts[c] = cnt;
    }
}

// The byte after byte b of a 16-byte load (at block offset q): from the load
// itself, from the next lane's load (nxw: its first word) for the last byte,
// from memory only at the wave's last lane (the caller checks q + 1 < n).
__device__ __forceinline__ u32 fq_next_byte(const uint4 v, u32 nxw, int b, const uint8_t* __restrict__ base, u64 q) {
    if (b == 15) return lane_id() < 63 ? (nxw & 255u) : (u32)base[q + 1];
    const int i = b + 1;
    const u32 w = (i & 8) ? ((i & 4) ? v.w : v.z) : ((i & 4) ? v.y : v.x);
    return (w >> (8 * (i & 3))) & 255u;
}

// Every wave numbers the newlines of its own chunks from the chunk's line
// base (wave scans only, no workgroup barrier; the next 1 KiB slice is
// loaded while this one is emitted).
__global__ __launch_bounds__(kBlock) void fq_emit_k(const uint8_t* __restrict__ base, u64 n, u64 nchunks,
                                                    const u64* __restrict__ line_base, u64* __restrict__ seq_off,
                                                    u64* __restrict__ seq_end, u64 max_rec, u64* stats) {
    const uintptr_t A = (uintptr_t)base & ~(uintptr_t)15;
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    u64 err = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (n == 0 || base[0] != '@') err |= ERR_FQ_NOT_AT;
        if (n > 0 && base[n - 1] != '\n') err |= ERR_FQ_NO_FINAL_NL;
    }
    auto load = [&](u64 c, int it, long long* rel) {
        const uintptr_t addr = A + c * kFqChunk + (u64)it * 1024 + (u64)lane * 16;
        *rel = (long long)(addr - (uintptr_t)base);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (!(*rel + 16 <= 0 || *rel >= (long long)n)) v = fq_load16(addr);
        return v;
    };
    for (u64 c = (u64)blockIdx.x * kFqWaves + wave; c < nchunks; c += (u64)gridDim.x * kFqWaves) {
        u64 run = line_base[c];
        long long reln;
        uint4 vn = load(c, 0, &reln);
        for (int it = 0; it < 16; it++) {
            const uint4 v = vn;
            const long long rel0 = reln;
            if (it < 15) vn = load(c, it + 1, &reln);
            u32 m = (rel0 + 16 <= 0 || rel0 >= (long long)n) ? 0u : nl_mask16(v, rel0, n);
            const u32 nxw = (u32)__shfl_down((int)v.x, 1);
            const u32 cnt = (u32)__popc(m);
            u32 inc = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u32 y = __shfl_up(inc, o);
                if (lane >= o) inc += y;
            }
            u64 j = run + (inc - cnt);
            run += (u32)__shfl((int)inc, 63);
            while (m) {
                const int b = __ffs(m) - 1;
                m &= m - 1;
                const u64 q = (u64)(rel0 + b);
                const u64 rec = j >> 2;
                switch (j & 3) {
                case 0:
                    if (rec < max_rec) seq_off[rec] = q + 1;
                    else err |= ERR_FQ_TOO_MANY;
                    break;
                case 1:
                    if (rec < max_rec) seq_end[rec] = q;
                    else err |= ERR_FQ_TOO_MANY;
                    if (q + 1 >= n || fq_next_byte(v, nxw, b, base, q) != '+') err |= ERR_FQ_NO_PLUS;
                    break;
                case 3:
                    if (q + 1 < n && fq_next_byte(v, nxw, b, base, q) != '@') err |= ERR_FQ_NOT_AT;
                    break;
                default: break;
                }
                j++;
            }
        }
    }
    if (err) atomicOr((unsigned long long*)&stats[ST_ERR], (unsigned long long)err);
}

__global__ __launch_bounds__(kBlock) void fq_validate_k(const u64* __restrict__ seq_off,
                                                        const u64* __restrict__ seq_end, u64 n_rec, int L,
                                                        u64* stats, int at_most) {
    bool bad = false;
    for (u64 r = (u64)blockIdx.x * kBlock + threadIdx.x; r < n_rec; r += (u64)gridDim.x * kBlock) {
        const u64 len = seq_end[r] - seq_off[r];
        bad |= at_most ? len > (u64)L : len != (u64)L;
    }
    if (__ballot(bad) && lane_id() == 0)
        atomicOr((unsigned long long*)&stats[ST_ERR], (unsigned long long)ERR_FQ_SEQ_LEN);
}

// K1 emit + E fused (engines that read codes, when the block is one batch):
// fq_emit_k's newline walk and encode_reads_k's encoding with one read of the
// text. Every wave takes its chunk in two halves of 8 KiB. A half and the next
// KiB are staged in the wave's LDS. The half is walked in two rounds of 64
// bytes per lane (one 64-bit newline mask per lane; the lanes' newline counts
// are scanned by ballots of their bits); every newline gets its line index
// from the chunk's line base, the '+' / '@' checks read the staged bytes, and
// the records whose header ends in the half are listed (sequence start per
// record). Then the wave encodes those reads, one (read, 16-base group) per
// lane, from LDS (groups past the staged bytes from global memory) into codes /
// inval at the read's index. The sequence-length check of fq_validate_k is
// done inline: no newline inside [s, s + L) and a newline at s + L, which is
// exactly seq_end - seq_off == L. Nothing is written to seq_off / seq_end.
#ifndef KC_FQ_HALF
#define KC_FQ_HALF 8192  // bytes walked per step (a multiple of 4096 dividing kFqChunk)
#endif
#ifndef KC_FQ_XB
#define KC_FQ_XB 16  // bytes per lane staged past the half (8 or 16)
#endif
#ifndef KC_FQ_BLOCK
#define KC_FQ_BLOCK 256  // fq_encode_k workgroup (small groups: as many resident per CU as registers allow)
#endif
#ifndef KC_FQ_WPE
#define KC_FQ_WPE 1  // fq_encode_k: minimum waves per SIMD asked of the register allocator (1 = no limit)
#endif
constexpr int kFqHalf = KC_FQ_HALF;
constexpr int kFqRounds = kFqHalf / 4096;        // 64 lanes x 64 B per round
constexpr int kFqParts = (int)(kFqChunk / kFqHalf);  // halves per fq_count chunk
constexpr int kFqStage = kFqHalf + 64 * KC_FQ_XB;
constexpr int kFqEncBlock = KC_FQ_BLOCK;
constexpr int kFqEncWaves = kFqEncBlock / 64;
static_assert(kFqRounds >= 1 && kFqHalf % 4096 == 0 && kFqChunk % kFqHalf == 0, "fq half size");
static_assert(KC_FQ_XB == 8 || KC_FQ_XB == 16, "fq extra staging");

int fq_encode_list_cap(int L) { return kFqHalf / (L + 6) + 2; }  // records with an L-base sequence are >= L + 6 bytes

static size_t fq_encode_wave_lds(int L) {
    return (size_t)kFqStage + (((size_t)fq_encode_list_cap(L) * 2 + 15) & ~(size_t)15);
}

// bit b set when byte b of w is '\n'
__device__ __forceinline__ u32 nl_nib(u32 w) {
    const u32 t = w ^ 0x0a0a0a0au;
    const u32 z = ~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u;
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | (z >> 28);
}

// '\n' bytes of 16 bytes (4 dwords, first byte lowest) as a 16-bit mask, bit
// i = byte i: the per-byte flags (0x80 per byte) of each dword are weighted
// by v_dot4_u32_u8 (bytes 1 2 4 8 for dwords 0 and 2, 16 32 64 128 for 1 and
// 3, two dwords accumulated per half), so each half is its 8-bit mask times 128
__device__ __forceinline__ u32 nl_mask16w(u32 w0, u32 w1, u32 w2, u32 w3) {
    auto z = [](u32 w) {
        const u32 t = w ^ 0x0a0a0a0au;
        return ~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u;
    };
    const u32 lo = __builtin_amdgcn_udot4(z(w1), 0x80402010u, __builtin_amdgcn_udot4(z(w0), 0x08040201u, 0u, false), false);
    const u32 hi = __builtin_amdgcn_udot4(z(w3), 0x80402010u, __builtin_amdgcn_udot4(z(w2), 0x08040201u, 0u, false), false);
    return (lo >> 7) | (hi << 1);
}

// newline bytes among the first nv bytes of a dword (any)
__device__ __forceinline__ bool has_nl(u32 x, int nv) {
    if (nv <= 0) return false;
    const u32 t = x ^ 0x0a0a0a0au;
    const u32 z = ~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u;
    const u32 vm = nv >= 4 ? 0x80808080u : (0x80808080u >> (8 * (4 - nv)));
    return (z & vm) != 0u;
}

// bytes_to_codes by SWAR: 4 bytes -> 4 2-bit codes in the low byte (first
// byte highest; ((c >> 1) ^ (c >> 2)) & 3 is A0 C1 G2 T3) and the 4-bit
// not-ACGT mask (a byte is ACGT iff it equals the ACGT byte of its code,
// looked up by v_perm); non-ACGT bytes code 3, bytes >= nv code 0 and valid
__device__ __forceinline__ u32 swar_codes(u32 x, int nv, u32* bad4) {
    const u32 vm = nv >= 4 ? ~0u : (nv <= 0 ? 0u : (~0u >> (8 * (4 - nv))));
    u32 t = ((x >> 1) ^ (x >> 2)) & 0x03030303u;
    const u32 y = __builtin_amdgcn_perm(0u, 0x54474341u, t) ^ x;
    const u32 bad = (((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y) & 0x80808080u & vm;
    t = (t & vm) | (bad >> 7) | (bad >> 6);
    *bad4 = ((bad >> 4) & 8u) | ((bad >> 13) & 4u) | ((bad >> 22) & 2u) | (bad >> 31);
    return ((t << 6) | (t >> 4) | (t >> 14) | (t >> 24)) & 255u;
}

// 16 bytes (x0 first, lowest byte first; nb of them valid) -> the group's code
// word (base 0 in bits 31-30) and not-ACGT mask (base 0 in bit 15), as
// swar_codes per dword; each dword's four 2-bit codes and four bad-byte flags
// are packed by one v_dot4_u32_u8 each (bytes times 64 16 4 1 and 8 4 2 1:
// the first byte lands highest)
__device__ __forceinline__ u32 swar_group(u32 x0, u32 x1, u32 x2, u32 x3, int nb, u32* bad16) {
    const u32 xs[4] = {x0, x1, x2, x3};
    u32 code = 0, bm = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int nv = nb - 4 * k;
        const u32 vm = nv >= 4 ? ~0u : (nv <= 0 ? 0u : (~0u >> (8 * (4 - nv))));
        u32 t = ((xs[k] >> 1) ^ (xs[k] >> 2)) & 0x03030303u;
        const u32 y = __builtin_amdgcn_perm(0u, 0x54474341u, t) ^ xs[k];
        const u32 bad = (((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y) & 0x80808080u & vm;
        const u32 b1 = bad >> 7;  // 1 in each bad byte
        t = (t & vm) | b1 | (bad >> 6);  // bad bytes code 3, bytes past nb code 0
        code = __builtin_amdgcn_udot4(t, 0x01041040u, code << 8, false);
        bm = __builtin_amdgcn_udot4(b1, 0x01020408u, bm << 4, false);
    }
    *bad16 = bm;
    return code;
}

// VAR (KC_FLAG_VARLEN): sequences of 0..L bases. After the newline walk one
// lane per listed record finds its sequence's newline (staged dwords, global
// past the staging) and keeps its length; the encode then reads only the
// read's own bytes and marks the rest of the L-base slot not-ACGT (as
// encode_reads_var_k). The list holds lcap records per half (records of >= 32
// bytes); a denser half sets ERR_FQ_LIST.
// SP (one-pass index, fixed L): no line_base. Each chunk guesses its line
// phase (the line index of its first byte mod 4) from the first newlines of
// its text: the line after newline i is taken for a header when a line of L
// bases, a '+' line and a line of L bytes follow (a quality line starting with
// '@' is followed by a header and a sequence line, which does not start with
// '+'). The chunk's records go to its own rows [c cap, c cap + cap) (cap =
// max_rec), the rows past them are empty (rlen 0, codes 0, every base
// not-ACGT), and sp_cnt[c] / sp_phase[c] = its newlines / phase | 4 (not
// found). fq_spec_verify_k checks the phases against the scanned counts; any
// miss or error sends the block to the two-kernel index. rlen[row] = L for the
// records; stats[ST_VHOLE] is set when a read holds a not-ACGT base.
template <bool VAR, bool SP = false>
__global__ __launch_bounds__(kFqEncBlock) __attribute__((amdgpu_waves_per_eu(KC_FQ_WPE))) void fq_encode_k(const uint8_t* __restrict__ base, u64 n, u64 nchunks,
                                                      const u64* __restrict__ line_base, u64 max_rec_in, int L, int G,
                                                      int lcap, u32* __restrict__ codes,
                                                      unsigned short* __restrict__ inval, u64* stats,
                                                      unsigned short* __restrict__ rlen, int k,
                                                      u64* __restrict__ sp_cnt,
                                                      unsigned char* __restrict__ sp_phase) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uintptr_t A = (uintptr_t)base & ~(uintptr_t)15;
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u64 lt = lanemask_lt();
    const size_t wbytes = (size_t)kFqStage + (((size_t)lcap * (VAR ? 4 : 2) + 15) & ~(size_t)15);
    unsigned char* txt = smem + (size_t)wave * wbytes;
    unsigned short* lst = (unsigned short*)(txt + kFqStage);
    unsigned short* lenl = lst + lcap;  // VAR: the listed records' sequence lengths
    bool vhole = false;
    u64 vwin = 0;
    const FastDivU divg((u32)G);
    const FastDivU divg1((u32)(G > 1 ? G - 1 : 1));  // fixed L: the full groups of a read
    u64 err = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (n == 0 || base[0] != '@') err |= ERR_FQ_NOT_AT;
        if (n > 0 && base[n - 1] != '\n') err |= ERR_FQ_NO_FINAL_NL;
    }
    auto sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    };
    // the wave's halves in order: (c, 0), (c, 1), (c + stride, 0), ...; the
    // next half's text is loaded into registers while this one is walked and
    // encoded from LDS
    const u64 cstride = (u64)gridDim.x * kFqEncWaves;
    uint4 v[kFqRounds][4], x;
    auto issue = [&](u64 cc, int hh) {
        const uintptr_t hb = A + cc * kFqChunk + (u64)hh * kFqHalf;
        const long long hrel = (long long)(hb - (uintptr_t)base);
#pragma unroll
        for (int rd = 0; rd < kFqRounds; rd++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int o = rd * 4096 + lane * 64 + i * 16;
                const long long rel = hrel + o;
                v[rd][i] = (rel + 16 <= 0 || rel >= (long long)n) ? make_uint4(0, 0, 0, 0) : fq_load16(hb + (u64)o);
            }
        const int o = kFqHalf + lane * KC_FQ_XB;
        const long long rel = hrel + o;
        if constexpr (KC_FQ_XB == 16) {
            x = (rel >= (long long)n) ? make_uint4(0, 0, 0, 0) : fq_load16(hb + (u64)o);
        } else {
            const u64 y0 = rel >= (long long)n ? 0ull : *(const __attribute__((address_space(1))) u64*)(hb + (u64)o);
            x = make_uint4((u32)y0, (u32)(y0 >> 32), 0u, 0u);  // bytes 8..15: no newline
        }
    };
    // a newline mask of 64 staged bytes limited to the block's bytes
    auto trim = [&](u64 m, long long rel0) -> u64 {
        if (rel0 < 0) m = (rel0 <= -64) ? 0ull : (m & (~0ull << (u32)(-rel0)));
        if (rel0 + 64 > (long long)n) m = (rel0 >= (long long)n) ? 0ull : (m & (~0ull >> (u32)(rel0 + 64 - (long long)n)));
        return m;
    };
    u64 c = (u64)blockIdx.x * kFqEncWaves + wave;
    int h = 0;
    u64 run = 0;
    // SP: the chunk's phase, whether it was found, its first record's local
    // index ((phase + 3) >> 2) and the row of local record 0 (row = rowoff + local)
    u32 sp_phi = 0;
    bool sp_fail = false;
    u64 rbase = 0, rowoff = 0;
    u64 max_rec = max_rec_in;
    if constexpr (SP) {
        // rows per chunk for this block: records are at least 2L + 5 + h
        // bytes with h the header line's length; h from the block's first
        // header less a margin (header lengths differ by the read number's
        // digits). A chunk denser than that reports ERR_FQ_TOO_MANY and the
        // block takes the two-kernel index. max_rec_in assumes h = 1.
        u32 h0 = 1;
        bool found = false;
        for (u32 b0 = 0; b0 < 1024u && !found; b0 += 256u) {
            const u64 o = (u64)b0 + 4u * (u32)lane;
            int pos = -1;
#pragma unroll
            for (int b = 3; b >= 0; b--)
                if (o + (u64)b < n && base[o + (u64)b] == (uint8_t)'\n') pos = (int)(o + (u64)b);
            const u64 bm = __ballot(pos >= 0);
            if (bm) {
                h0 = (u32)__builtin_amdgcn_readlane(pos, __ffsll((long long)bm) - 1);
                found = true;
            }
        }
        const u64 hmin = h0 > 17u ? (u64)h0 - 16u : 1u;
        max_rec = min(max_rec_in, 1 + (kFqChunk - 1) / (2 * (u64)L + 5 + hmin));
        if (blockIdx.x == 0 && threadIdx.x == 0) sp_cnt[nchunks + 1] = max_rec;
    }
    if (c < nchunks) issue(c, 0);
    while (c < nchunks) {
        {
            const uintptr_t hb = A + c * kFqChunk + (u64)h * kFqHalf;
            const long long hrel = (long long)(hb - (uintptr_t)base);
            if constexpr (!SP) {
                if (h == 0) run = line_base[c];
            }
            // the next half: (c, 1) unless it starts past the block
            u64 cn = c;
            int hn = 1;
            if (h == kFqParts - 1 || (long long)(hrel + kFqHalf) >= (long long)n) {
                cn = c + cstride;
                hn = 0;
            } else {
                hn = h + 1;
            }
#pragma unroll
            for (int rd = 0; rd < kFqRounds; rd++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    v4u w;
                    w.x = v[rd][i].x;
                    w.y = v[rd][i].y;
                    w.z = v[rd][i].z;
                    w.w = v[rd][i].w;
                    *(v4u*)(txt + rd * 4096 + lane * 64 + i * 16) = w;
                }
            if constexpr (KC_FQ_XB == 16) {
                v4u w;
                w.x = x.x;
                w.y = x.y;
                w.z = x.z;
                w.w = x.w;
                *(v4u*)(txt + kFqHalf + lane * 16) = w;
            } else {
                *(u64*)(txt + kFqHalf + lane * 8) = (u64)x.x | ((u64)x.y << 32);
            }
            u64 mk[kFqRounds];
#pragma unroll
            for (int rd = 0; rd < kFqRounds; rd++) {
                u64 m = 0;
#pragma unroll
                for (int i = 0; i < 4; i++)
                    m |= (u64)nl_mask16w(v[rd][i].x, v[rd][i].y, v[rd][i].z, v[rd][i].w) << (16 * i);
                mk[rd] = m;
            }
            // VAR: newlines of the staged KiB past the half (the sequence end
            // of a record that straddles the half end is its first one); the
            // walk writes each listed record's sequence-end position
            u32 mx = 0;
            if constexpr (VAR) {
                mx = nl_mask16w(x.x, x.y, x.z, x.w);
                for (int i = lane; i < lcap; i += 64) lenl[i] = 0xffffu;
            }
            if (cn < nchunks) issue(cn, hn);
            sync();
            if constexpr (SP) {
                if (h == 0) {
                    // the phase from the first newlines of the chunk's first 4 KiB
                    // (the block's first chunk starts with a header: phase 0)
                    sp_phi = 0;
                    sp_fail = false;
                    if (c != 0) {
                        u64 m0 = trim(mk[0], hrel + lane * 64);
                        const u32 c0 = (u32)__popcll(m0);
                        u32 inc = c0;
#pragma unroll
                        for (int o = 1; o < 64; o <<= 1) {
                            const u32 y = __shfl_up(inc, o);
                            if (lane >= o) inc += y;
                        }
                        u32 kx = inc - c0;
                        const u32 tot0 = (u32)__shfl((int)inc, 63);
                        unsigned short* nl8 = lst;  // scratch: the walk below rewrites the list
                        while (m0 && kx < 8u) {
                            nl8[kx++] = (unsigned short)(lane * 64 + __ffsll((long long)m0) - 1);
                            m0 &= m0 - 1;
                        }
                        sync();
                        sp_fail = true;
                        int nl[8];
#pragma unroll
                        for (int i = 0; i < 8; i++) nl[i] = (u32)i < tot0 ? (int)nl8[i] : 0;
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            if (sp_fail && (u32)(i + 4) < tot0 && txt[nl[i] + 1] == (unsigned char)'@' &&
                                nl[i + 2] - nl[i + 1] - 1 == L && txt[nl[i + 2] + 1] == (unsigned char)'+' &&
                                nl[i + 4] - nl[i + 3] - 1 == L) {
                                sp_phi = (u32)(3 - i) & 3u;
                                sp_fail = false;
                            }
                        }
                        sync();
                    }
                    run = sp_phi;
                    rbase = (sp_phi + 3u) >> 2;
                    rowoff = c * max_rec - rbase;
                }
            }
            const u64 rec0 = (run + 3) >> 2;  // first record whose header may end in this half
#pragma unroll
            for (int rd = 0; rd < kFqRounds; rd++) {
                u64 m = mk[rd];
                const long long rel0 = hrel + rd * 4096 + lane * 64;
                m = trim(m, rel0);
                const u32 cnt = (u32)__popcll(m);
                u32 ex = 0, tot = 0;
                if (__ballot(cnt > 7u) == 0ull) {
                    // counts below 8: the prefix from three bit-plane ballots
#pragma unroll
                    for (int bp = 0; bp < 3; bp++) {
                        const u64 bl = __ballot((cnt >> bp) & 1u);
                        ex += (u32)__popcll(bl & lt) << bp;
                        tot += (u32)__popcll(bl) << bp;
                    }
                } else {
                    u32 inc = cnt;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const u32 y = __shfl_up(inc, o);
                        if (lane >= o) inc += y;
                    }
                    ex = inc - cnt;
                    tot = (u32)__shfl((int)inc, 63);
                }
                u64 j = run + ex;
                run += tot;
                while (m) {
                    const int b = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int o = rd * 4096 + lane * 64 + b;  // staged position of the newline
                    const u64 q = (u64)(hrel + o);
                    const u32 jc = (u32)j & 3u;
                    if (jc == 0u) {
                        const u64 li = (j >> 2) - rec0;
                        if ((j >> 2) - rbase >= max_rec) err |= ERR_FQ_TOO_MANY;
                        else if (li < (u64)lcap) lst[li] = (unsigned short)(o + 1);
                        else err |= VAR ? ERR_FQ_LIST : ERR_FQ_SEQ_LEN;  // more records than the list holds
                    } else if (jc != 2u) {
                        if (VAR && jc == 1u) {
                            const u64 li = (j >> 2) - rec0;  // wraps for records listed by the previous half
                            if (li < (u64)lcap) lenl[li] = (unsigned short)o;
                        }
                        // after the sequence: '+'; after the quality line: '@' (or the block end)
                        const u32 nx = q + 1 < n ? (u32)txt[o + 1] : 0u;
                        if (jc == 1u ? nx != (u32)'+' : (q + 1 < n && nx != (u32)'@'))
                            err |= jc == 1u ? ERR_FQ_NO_PLUS : ERR_FQ_NOT_AT;
                    }
                    j++;
                }
            }
            sync();
            // records [rec0, rec1) have their header newline in this half
            u64 rec1 = (run + 3) >> 2;
            if (rec1 - rbase > max_rec) rec1 = rbase + max_rec;
            const u32 nrec = rec1 > rec0 ? (u32)min(rec1 - rec0, (u64)lcap) : 0u;
            if constexpr (VAR) {
                // each listed record's sequence length: the walk saw its
                // sequence end, or (at most one record, the one straddling the
                // half end) it is the first newline of the staged KiB past the
                // half, or (reads past that KiB) found by a dword scan
                const u64 bx = __ballot(mx != 0u);
                int ex = -1;
                if (bx) {
                    const int fl = __ffsll((long long)bx) - 1;
                    ex = kFqHalf + KC_FQ_XB * fl + __builtin_ctz((u32)__builtin_amdgcn_readlane((int)mx, fl));
                }
                for (u32 li = (u32)lane; li < nrec; li += 64) {
                    const int s = (int)lst[li];
                    const u32 se = lenl[li];
                    int pos = s & ~3, e = se != 0xffffu ? (int)se : (s <= kFqHalf ? ex : -1);
                    while (e < 0 && pos - s <= L) {
                        u32 w;
                        if (pos + 4 <= kFqStage) {
                            w = *(const u32*)(txt + pos);
                        } else {
                            const long long q = hrel + pos;  // block offset of the dword (4-aligned address)
                            typedef __attribute__((address_space(1))) const u32 g32;
                            w = q < (long long)n ? *(const g32*)(hb + (u64)pos) : 0x0a0a0a0au;
                        }
                        u32 m = nl_nib(w);
                        if (pos < s) m &= 0xfu << (s - pos);
                        if (m) e = pos + __builtin_ctz(m);
                        pos += 4;
                    }
                    const int len = e < 0 ? L + 1 : e - s;
                    if (len > L) err |= ERR_FQ_SEQ_LEN;
                    const int lc = min(len, L);
                    lenl[li] = (unsigned short)lc;
                    if (rlen) rlen[rec0 + li] = (unsigned short)lc;
                    if (lc >= k) vwin += (u64)(lc - k + 1);
                }
                sync();
            }
            // the half's rows start at row rowoff + rec0: item (r, g) is word
            // r G + g = item past that row's first word (no per-item 64-bit math)
            u32* const hcodes = codes + (rowoff + rec0) * (u64)G;
            unsigned short* const hinval = inval + (rowoff + rec0) * (u64)G;
            // group g of listed record r (item r G + g)
            auto encode = [&](u32 r, int g, int nb0, bool lastg) {
                const u32 item = r * (u32)G + (u32)g;
                const int s0 = (int)lst[r] + 16 * g;  // staged offset of the group's first base
                const int lr = VAR ? (int)lenl[r] : L;
                const int nb = VAR ? max(0, min(nb0, lr - 16 * g)) : nb0;  // of them, bases of the read
                const int need = nb + ((lastg && !VAR) ? 1 : 0);  // the group (+ the byte after the read)
                const int sh = s0 & 3;
                u32 d[5];
                if ((s0 & ~3) + 20 <= kFqStage) {
                    const u32* lw = (const u32*)(txt + (s0 & ~3));
#pragma unroll
                    for (int i = 0; i < 5; i++) d[i] = lw[i];
                } else {
                    // past the staged bytes: global dwords holding a byte of [s0, s0 + need) below n
                    const long long gq = hrel + s0;
                    typedef __attribute__((address_space(1))) const u32 g32;
                    const g32* dw = (const g32*)((uintptr_t)(base + gq) & ~(uintptr_t)3);
#pragma unroll
                    for (int i = 0; i < 5; i++) {
                        const long long first = gq - sh + 4 * i;  // block offset of dword i
                        d[i] = (4 * i < sh + need && first < (long long)n) ? dw[i] : 0u;
                    }
                }
                const u32 x0 = __builtin_amdgcn_alignbyte(d[1], d[0], sh);
                const u32 x1 = __builtin_amdgcn_alignbyte(d[2], d[1], sh);
                const u32 x2 = __builtin_amdgcn_alignbyte(d[3], d[2], sh);
                const u32 x3 = __builtin_amdgcn_alignbyte(d[4], d[3], sh);
                u32 bad;
                const u32 cw = swar_group(x0, x1, x2, x3, nb, &bad);
                if constexpr (!VAR) {
                    // a newline is a non-ACGT byte: the exact test only for such groups
                    bool wrong = bad != 0u &&
                                 (has_nl(x0, nb) || has_nl(x1, nb - 4) || has_nl(x2, nb - 8) || has_nl(x3, nb - 12));
                    if (lastg) {
                        const int e = sh + nb;  // the byte after the read, in d
                        const u32 nxt = (d[e >> 2] >> (8 * (e & 3))) & 255u;
                        wrong = wrong || nxt != (u32)'\n' || hrel + s0 + nb >= (long long)n;
                    }
                    if (wrong) err |= ERR_FQ_SEQ_LEN;
                    if (bad != 0u) vhole = true;  // (ST_VHOLE: key 0's presence for padded / one-pass rows)
                } else {
                    if (bad != 0u && lr >= k) vhole = true;
                    bad |= ((1u << (16 - nb)) - 1u) & ~((1u << (16 - nb0)) - 1u);  // the slot past the read
                }
                hcodes[item] = cw;
                hinval[item] = (unsigned short)bad;
                if (SP && g == 0) rlen[rowoff + rec0 + r] = (unsigned short)L;
            };
            if constexpr (!VAR) {
                // fixed L: the groups before a read's last hold 16 bases each
                // (their loop has no byte masks and no end-of-read test), the
                // last group L - 16 (G - 1) and the byte after the read
#pragma unroll 1
                for (u32 item = (u32)lane; item < nrec * (u32)(G - 1); item += 64) {
                    const u32 r = divg1.div(item);
                    encode(r, (int)(item - r * (u32)(G - 1)), 16, false);
                }
#pragma unroll 1
                for (u32 r = (u32)lane; r < nrec; r += 64) encode(r, G - 1, L - 16 * (G - 1), true);
            } else {
#pragma unroll 1
                for (u32 item = (u32)lane; item < nrec * (u32)G; item += 64) {
                    const u32 r = divg.div(item);
                    const int g = (int)(item - r * (u32)G);
                    encode(r, g, min(16, L - 16 * g), g == G - 1);
                }
            }
            if constexpr (SP) {
                if (hn == 0) {
                    // the chunk is done: its empty rows, newline count and phase
                    const u64 nrec_c = min(((run + 3) >> 2) - rbase, max_rec);
                    const u64 row0 = c * max_rec;
                    for (u64 q = nrec_c * (u64)G + (u64)lane; q < max_rec * (u64)G; q += 64) {
                        codes[row0 * (u64)G + q] = 0u;
                        inval[row0 * (u64)G + q] = (unsigned short)0xffffu;
                    }
                    for (u64 q = nrec_c + (u64)lane; q < max_rec; q += 64) rlen[row0 + q] = 0;
                    if (lane == 0) {
                        sp_cnt[c] = run - sp_phi;
                        sp_phase[c] = (unsigned char)(sp_phi | (sp_fail ? 4u : 0u));
                    }
                }
            }
            sync();
            c = cn;
            h = hn;
        }
    }
    if (err) atomicOr((unsigned long long*)&stats[ST_ERR], (unsigned long long)err);
    if (__ballot(vhole) && lane == 0) atomicOr((unsigned long long*)&stats[ST_VHOLE], 1ull);
    if constexpr (VAR) {
        for (int o = 32; o >= 1; o >>= 1) vwin += __shfl_xor(vwin, o);
        if (lane == 0 && vwin) atomicAdd((unsigned long long*)&stats[ST_VWIN], (unsigned long long)vwin);
    }
}

hipError_t launch_fq_encode(const uint8_t* base, uint64_t n, const uint64_t* line_base, uint64_t max_rec, int L,
                            uint32_t* codes, uint16_t* inval, uint64_t* stats, hipStream_t s) {
    if (L < 1 || L > 32767) return hipErrorInvalidValue;
    u64 nch = fq_chunks(base, n);
    const int G = groups_per_read(L);
    const int lcap = fq_encode_list_cap(L);
    if ((u64)lcap * (u64)G >= 65536) return hipErrorInvalidValue;  // FastDivU range
    const size_t lds = (size_t)kFqEncWaves * fq_encode_wave_lds(L);
    int g = (int)hmin((nch + kFqEncWaves - 1) / kFqEncWaves, 16384);
    hipLaunchKernelGGL(fq_encode_k<false>, dim3(g ? g : 1), dim3(kFqEncBlock), lds, s, base, n, nch, line_base, max_rec,
                       L, G, lcap, codes, (unsigned short*)inval, stats, (unsigned short*)nullptr, 0, (u64*)nullptr,
                       (unsigned char*)nullptr);
    return hipGetLastError();
}

// One-pass index (fq_encode_k<false, true>): rows per chunk, the largest number
// of records whose header ends in one 16 KiB chunk (records of >= 2L + 6 bytes,
// so consecutive header ends are >= 2L + 6 bytes apart)
uint64_t fq_spec_rows_per_chunk(int L) { return 1 + (kFqChunk - 1) / (2 * (u64)L + 6); }
// the phase guess reads the first 8 newlines of a chunk's first 4 KiB
bool fq_spec_ok(int L) { return L >= 1 && 4 * (2 * L + 8) <= 4096 - 2 * L; }

hipError_t launch_fq_encode_spec(const uint8_t* base, uint64_t n, int L, uint32_t* codes, uint16_t* inval,
                                 uint16_t* rlen, uint64_t* cnt, uint8_t* phase, uint64_t* stats, hipStream_t s) {
    if (!fq_spec_ok(L)) return hipErrorInvalidValue;
    u64 nch = fq_chunks(base, n);
    const int G = groups_per_read(L);
    const int lcap = fq_encode_list_cap(L);
    if ((u64)lcap * (u64)G >= 65536 || lcap < 8) return hipErrorInvalidValue;
    const size_t lds = (size_t)kFqEncWaves * fq_encode_wave_lds(L);
    int g = (int)hmin((nch + kFqEncWaves - 1) / kFqEncWaves, 16384);
    hipLaunchKernelGGL((fq_encode_k<false, true>), dim3(g ? g : 1), dim3(kFqEncBlock), lds, s, base, n, nch,
                       (const u64*)nullptr, (u64)fq_spec_rows_per_chunk(L), L, G, lcap, codes, (unsigned short*)inval,
                       stats, (unsigned short*)rlen, 0, cnt, phase);
    return hipGetLastError();
}

// The guessed phases against the scanned newline counts (line_base = their
// exclusive scan): a chunk whose phase was not found or differs sets ERR_FQ_SPEC
__global__ __launch_bounds__(kBlock) void fq_spec_verify_k(const u64* __restrict__ line_base,
                                                           const unsigned char* __restrict__ phase, u64 nch,
                                                           u64* __restrict__ stats) {
    bool bad = false;
    for (u64 c = (u64)blockIdx.x * kBlock + threadIdx.x; c < nch; c += (u64)gridDim.x * kBlock)
        bad = bad || (phase[c] & 4u) != 0u || (u32)(line_base[c] & 3u) != (u32)(phase[c] & 3u);
    if (__ballot(bad) && lane_id() == 0) atomicOr((unsigned long long*)&stats[ST_ERR], (unsigned long long)ERR_FQ_SPEC);
}

hipError_t launch_fq_spec_verify(const uint64_t* line_base, const uint8_t* phase, uint64_t nch, uint64_t* stats,
                                 hipStream_t s) {
    if (nch == 0) return hipSuccess;
    hipLaunchKernelGGL(fq_spec_verify_k, dim3(grid_for(nch)), dim3(kBlock), 0, s, line_base,
                       (const unsigned char*)phase, nch, stats);
    return hipGetLastError();
}

// records of >= 32 bytes per half's list; denser halves: ERR_FQ_LIST
constexpr int kFqVarListCap = kFqHalf / 32 + 2;

bool fq_encode_var_ok(int L) {
    // (list entry, group) items are split by a FastDivU over lcap * G < 2^16
    return L >= 1 && L <= 32767 && (u64)kFqVarListCap * (u64)groups_per_read(L) < 65536;
}

hipError_t launch_fq_encode_var(const uint8_t* base, uint64_t n, const uint64_t* line_base, uint64_t max_rec, int L,
                                int k, uint32_t* codes, uint16_t* inval, uint16_t* rlen, uint64_t* stats,
                                hipStream_t s) {
    if (!fq_encode_var_ok(L) || k < 1) return hipErrorInvalidValue;
    u64 nch = fq_chunks(base, n);
    const int G = groups_per_read(L);
    const int lcap = kFqVarListCap;
    const size_t wl = (size_t)kFqStage + (((size_t)lcap * 4 + 15) & ~(size_t)15);
    const size_t lds = (size_t)kFqEncWaves * wl;
    int g = (int)hmin((nch + kFqEncWaves - 1) / kFqEncWaves, 16384);
    hipLaunchKernelGGL(fq_encode_k<true>, dim3(g ? g : 1), dim3(kFqEncBlock), lds, s, base, n, nch, line_base, max_rec, L,
                       G, lcap, codes, (unsigned short*)inval, stats, (unsigned short*)rlen, k, (u64*)nullptr,
                       (unsigned char*)nullptr);
    return hipGetLastError();
}

hipError_t launch_fq_count(const uint8_t* base, uint64_t n, uint64_t* counts, hipStream_t s) {
    u64 nch = fq_chunks(base, n);
    int g = (int)hmin((nch + kFqWaves - 1) / kFqWaves, 16384);
    hipLaunchKernelGGL(fq_count_k, dim3(g ? g : 1), dim3(kBlock), 0, s, base, n, nch, counts);
    return hipGetLastError();
}

hipError_t launch_fq_emit(const uint8_t* base, uint64_t n, const uint64_t* line_base, uint64_t* seq_off,
                          uint64_t* seq_end, uint64_t max_rec, uint64_t* stats, hipStream_t s) {
    u64 nch = fq_chunks(base, n);
    int g = (int)hmin((nch + kFqWaves - 1) / kFqWaves, 16384);
    hipLaunchKernelGGL(fq_emit_k, dim3(g ? g : 1), dim3(kBlock), 0, s, base, n, nch, line_base, seq_off, seq_end,
                       max_rec, stats);
    return hipGetLastError();
}

hipError_t launch_fq_validate(const uint64_t* seq_off, const uint64_t* seq_end, uint64_t n_rec, int L,
                              uint64_t* stats, hipStream_t s, bool at_most) {
    if (n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(fq_validate_k, dim3(grid_for(n_rec)), dim3(kBlock), 0, s, seq_off, seq_end, n_rec, L, stats,
                       at_most ? 1 : 0);
    return hipGetLastError();
}
