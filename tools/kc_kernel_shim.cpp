// kc_kernel_shim: the launch wrappers of the radix grouping passes (rp_*) and
// of the segment sort (tests/test_gpu_kernels.py), and of the sort, scan,
// reduce, compact and merge primitives under them
// (tests/test_gpu_finish_kernels.py), and of the two ends of the super-k-mer
// engine (tests/test_gpu_skm_kernels.py): kcs_skm_geometry, kcs_skm_front
// (E + F / F2 / F3), kcs_count_rec (P5a + dedup_total) and kcs_count_skm (P5),
// and of the canonical fold's passes (tests/test_gpu_canon_kernels.py):
// kcs_canon_count, kcs_canon_split, and of the key-prefix (partition) engine
// (tests/test_gpu_part_kernels.py): kcs_bucket_lds_slots, kcs_sort_runs_keys,
// kcs_count_buckets (P5), kcs_sort_runs (P5s, direct mode included),
// kcs_part_geometry, kcs_part_front (E + P1 / P2) and kcs_hist_group, and of
// the set-operation passes (tests/test_gpu_setops_kernels.py): kcs_setop,
// behind a C ABI. Every
// entry point takes host arrays, allocates device buffers, launches on a
// stream of its own, synchronises, copies the results back, frees the buffers
// and returns the hipError_t as an int. It uses only what kc_device.h declares
// and links libkc_hip.so; the product library knows nothing of it.
//
// The arguments are checked on the host before anything is launched (regions
// and descriptors inside their buffers, outputs inside theirs), so a wrong
// test cannot make a kernel read or write out of bounds: it gets
// hipErrorInvalidValue instead.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "kc_device.h"

namespace {

struct Dev {  // device buffers of one call, freed together
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    ~Dev() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    template <typename T>
    T* alloc(size_t n, int fill = -1) {
        void* p = nullptr;
        if (err != hipSuccess) return nullptr;
        const size_t bytes = (n ? n : 1) * sizeof(T);
        err = hipMalloc(&p, bytes);
        if (err != hipSuccess) return nullptr;
        ptrs.push_back(p);
        if (fill >= 0) err = hipMemset(p, fill, bytes);
        return (T*)p;
    }
    template <typename T>
    T* upload(const T* h, size_t n) {
        T* p = alloc<T>(n);
        if (p && n) err = hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice);
        return p;
    }
};

struct Stream {
    hipStream_t s = nullptr;
    hipError_t err;
    Stream() { err = hipStreamCreate(&s); }
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
};

#define KCS(x)                              \
    do {                                    \
        const hipError_t e_ = (x);          \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)

int n_cu() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return n;
}

// descriptors inside the records and the output; a segment longer than the
// capacity without bit 31 writes nothing, so only its records are checked
bool desc_ok(int W, uint64_t nrec, uint64_t ndesc, const uint32_t* order, const uint64_t* dstart,
             const uint32_t* dlen, const uint64_t* out_off, uint64_t nout) {
    const uint64_t cap = (uint64_t)kc::seg_sort_cap(W);
    for (uint64_t d = 0; d < ndesc; d++) {
        const uint32_t o = order[d];
        if (o >= ndesc) return false;
        const uint64_t len = dlen[o] & 0xffffffu;
        const bool pres = (dlen[o] >> 31) != 0;
        if (dstart[o] > nrec || len > nrec - dstart[o]) return false;
        // the prefetch of a presorted segment is clamped like any other's
        if (pres && len > cap) return false;
        if (len <= cap && (out_off[d] > nout || len > nout - out_off[d])) return false;
    }
    return true;
}

bool w_ok(int W) { return W >= 1 && W <= 4; }
bool fill_ok(int fill) { return fill >= 0 && fill <= 255; }

// scratch sized by a library function: that many elements + one guard word
constexpr int kGuard = 0x5c;
constexpr int KCS_GUARD_CLOBBERED = -77;  // no hipError_t is negative
int guard_check(const void* dev_word, size_t bytes) {
    uint8_t g[8];
    const hipError_t e = hipMemcpy(g, dev_word, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    for (size_t i = 0; i < bytes; i++)
        if (g[i] != kGuard) return KCS_GUARD_CLOBBERED;
    return hipSuccess;
}

// the merge kernels search their inputs: only sorted runs (word 0 most
// significant, equal neighbours allowed) reach them
bool soa_sorted(int W, const uint64_t* k, uint64_t stride, uint64_t n) {
    for (uint64_t i = 1; i < n; i++)
        for (int j = 0; j < W; j++) {
            const uint64_t x = k[(uint64_t)j * stride + i - 1], y = k[(uint64_t)j * stride + i];
            if (x < y) break;
            if (x > y) return false;
        }
    return true;
}
bool packed_sorted(int W, const uint8_t* p, uint64_t n) {
    const size_t rs = 8 * (size_t)W + 4;
    for (uint64_t i = 1; i < n; i++)
        for (int j = 0; j < W; j++) {
            uint64_t x, y;
            memcpy(&x, p + (i - 1) * rs + 8 * j, 8);
            memcpy(&y, p + i * rs + 8 * j, 8);
            if (x < y) break;
            if (x > y) return false;
        }
    return true;
}

// n elements pre-filled with `fill` (0 when negative: the kernel needs them
// clear) followed by 8 guard bytes; guarded_ok reads them back
template <typename T>
T* alloc_guarded(Dev& d, size_t n, int fill) {
    uint8_t* p = d.alloc<uint8_t>(n * sizeof(T) + 8, fill >= 0 ? fill : 0);
    if (p && d.err == hipSuccess) d.err = hipMemset(p + n * sizeof(T), kGuard, 8);
    return (T*)p;
}
template <typename T>
int guarded_ok(const T* p, size_t n) {
    return guard_check((const uint8_t*)p + n * sizeof(T), 8);
}

// bucket bounds: nb + 1 ascending entries that end inside the records
bool starts_ok(const uint64_t* starts, uint32_t nb, uint64_t stride) {
    if (!starts || nb < 1 || nb > 65536) return false;
    for (uint32_t b = 0; b < nb; b++)
        if (starts[b] > starts[b + 1]) return false;
    return starts[nb] <= stride;
}

}  // namespace

extern "C" {

int kcs_rp_tile(int NW, int pay) { return (NW < 1 || NW > 4) ? 0 : kc::rp_tile(NW, pay != 0); }
int kcs_seg_sort_cap(int W) { return (W < 1 || W > 4) ? 0 : kc::seg_sort_cap(W); }
int kcs_n_cu(void) { return n_cu(); }
uint64_t kcs_err_seg_too_long(void) { return (uint64_t)kc::ERR_SEG_TOO_LONG; }

// One grouping pass over n items of NW words (+ u32 payload when pay).
//   kin      NW x istride words (SoA, istride >= n), or n x NW words (istride 0: AoS)
//   rstart   nreg + 1 region bounds, ascending, rstart[0] = 0, rstart[nreg] = n
//   regional 0: LSD pass (digit-major over all regions), bases = 256 exclusive digit counts
//            1: MSD pass (every region sorted by the digit), bases = nreg * 256 + 1 sub-starts
//   digs     optional n digit bytes for the histogram (else (word0 >> shift) & 255;
//            AoS items of more than one word need digs: the histogram reads word 0 as an array)
//   dshift   the scatter's digit, (word0 >> dshift) & 255: must be the histogram's digit
//   emit     optional n bytes out: (word0 >> eshift) & 255 of the item placed at each index
//   kout     NW x ostride words (ostride >= n), or n x NW (ostride 0); pre-filled with `fill`
//   grid     as kc_count.cpp passes it (0: 2 x CUs); the scatter runs min(tiles, grid / 2) workgroups
//   ntiles   out: tiles of the pass (ceil(len / tile) per region, as group16 derives them)
int kcs_rp_pass(int NW, int pay, uint64_t n, const uint64_t* kin, uint64_t istride, const uint32_t* pin,
                const uint64_t* rstart, int nreg, int regional, const uint8_t* digs, int shift, int dshift,
                int eshift, uint8_t* emit, uint64_t* kout, uint64_t ostride, uint32_t* pout, int fill,
                uint64_t* bases, int grid, uint64_t* ntiles_out) {
    if (NW < 1 || NW > 4 || n == 0 || nreg < 1 || !kin || !kout || !rstart || !bases) return hipErrorInvalidValue;
    if ((pay != 0) != (pin != nullptr) || (pay != 0) != (pout != nullptr)) return hipErrorInvalidValue;
    if ((istride && istride < n) || (ostride && ostride < n)) return hipErrorInvalidValue;
    if (!digs && istride == 0 && NW > 1) return hipErrorInvalidValue;
    if (shift < 0 || shift > 56 || dshift < 0 || dshift > 56 || eshift < 0 || eshift > 56 || fill < 0 || fill > 255)
        return hipErrorInvalidValue;
    if (rstart[0] != 0 || rstart[nreg] != n) return hipErrorInvalidValue;
    for (int r = 0; r < nreg; r++)
        if (rstart[r + 1] < rstart[r]) return hipErrorInvalidValue;
    if (grid == 0) grid = 2 * n_cu();
    if (grid < 2) return hipErrorInvalidValue;
    const uint64_t tile = (uint64_t)kc::rp_tile(NW, pay != 0);
    std::vector<uint64_t> rt(2 * ((size_t)nreg + 1));
    uint64_t* tp = rt.data() + nreg + 1;
    for (int r = 0; r <= nreg; r++) rt[r] = rstart[r];
    tp[0] = 0;
    for (int r = 0; r < nreg; r++) tp[r + 1] = tp[r] + (rstart[r + 1] - rstart[r] + tile - 1) / tile;
    const uint64_t nt = tp[nreg];
    if (ntiles_out) *ntiles_out = nt;
    const size_t isz = (size_t)NW * (istride ? istride : n), osz = (size_t)NW * (ostride ? ostride : n);

    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* din = d.upload(kin, isz);
    uint64_t* dout = d.alloc<uint64_t>(osz, fill);
    uint32_t* dpin = pay ? d.upload(pin, n) : nullptr;
    uint32_t* dpout = pay ? d.alloc<uint32_t>(n, fill) : nullptr;
    uint8_t* ddigs = digs ? d.upload(digs, n) : nullptr;
    uint8_t* demit = emit ? d.alloc<uint8_t>(n, fill) : nullptr;
    uint64_t* drt = d.upload(rt.data(), rt.size());
    uint64_t* pos = d.alloc<uint64_t>(256 * nt);
    uint64_t* tmp = d.alloc<uint64_t>(regional ? (256 * nt + 1) / 2 : kc::rp_tmp_elems(nt));
    uint64_t* sub = regional ? d.alloc<uint64_t>((size_t)nreg * 256 + 1) : nullptr;
    KCS(d.err);
    const kc::RegionTable reg = {drt, drt + nreg + 1, nreg, nt, (uint32_t)tile};
    if (regional)
        KCS(kc::launch_rp_hist_regional(din, shift, reg, pos, (uint32_t*)tmp, grid, st.s, ddigs));
    else
        KCS(kc::launch_rp_hist(ddigs, ddigs ? nullptr : din, shift, reg, pos, tmp, grid, st.s));
    KCS(kc::launch_rp_scatter(NW, pay != 0, din, istride, dout, ostride, dpin, dpout, reg, pos, dshift, demit, eshift,
                              grid, st.s));
    if (regional) KCS(kc::launch_sub_starts(drt, drt + nreg + 1, pos, (uint32_t)nreg, n, sub, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(kout, dout, osz * 8, hipMemcpyDeviceToHost));
    if (pay) KCS(hipMemcpy(pout, dpout, n * 4, hipMemcpyDeviceToHost));
    if (emit) KCS(hipMemcpy(emit, demit, n, hipMemcpyDeviceToHost));
    if (regional)
        KCS(hipMemcpy(bases, sub, ((size_t)nreg * 256 + 1) * 8, hipMemcpyDeviceToHost));
    else
        KCS(hipMemcpy(bases, kc::rp_digit_base(tmp, nt), 256 * 8, hipMemcpyDeviceToHost));
    return hipSuccess;
}

// launch_seg_sort with explicit descriptors over nrec SoA records.
//   rkeys    W x rstride words, rcnts rstride counts; rstride >= nrec + 1 (seg_sort_k reads
//            record dstart of a zero-length segment, which is index nrec for a trailing one)
//   order, dstart, dlen (length | shift << 24 | presorted << 31), out_off, dkey (optional): ndesc each
//   out      packed: nout records of 8 W + 4 bytes; else W x nout words with out_cnts nout counts;
//            pre-filled with the byte `fill`
//   grid     0: one workgroup per CU
//   err      out: stats[ST_ERR]; fb_n out: segments handed to the LSD kernel; fb (optional,
//            ndesc entries out): their descriptor positions, in no particular order
int kcs_seg_sort(int W, uint64_t nrec, const uint64_t* rkeys, const uint32_t* rcnts, uint64_t rstride,
                 uint64_t ndesc, const uint32_t* order, const uint64_t* dstart, const uint32_t* dlen,
                 const uint64_t* out_off, const uint64_t* dkey, uint64_t nout, int packed, int fill, void* out,
                 uint32_t* out_cnts, int grid, uint64_t* err, uint64_t* fb_n, uint32_t* fb) {
    if (W < 1 || W > 4 || ndesc == 0 || !rkeys || !rcnts || !order || !dstart || !dlen || !out_off || !out || !err ||
        !fb_n)
        return hipErrorInvalidValue;
    if (rstride < nrec + 1 || (!packed && !out_cnts) || fill < 0 || fill > 255 || grid < 0) return hipErrorInvalidValue;
    if (!desc_ok(W, nrec, ndesc, order, dstart, dlen, out_off, nout)) return hipErrorInvalidValue;
    if (grid == 0) grid = n_cu();
    if (grid < 1) return hipErrorInvalidValue;
    const size_t rs = 8 * (size_t)W + 4;
    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* dk = d.upload(rkeys, (size_t)W * rstride);
    uint32_t* dc = d.upload(rcnts, rstride);
    uint32_t* dord = d.upload(order, ndesc);
    uint64_t* dst = d.upload(dstart, ndesc);
    uint32_t* dln = d.upload(dlen, ndesc);
    uint64_t* dof = d.upload(out_off, ndesc);
    uint64_t* dky = dkey ? d.upload(dkey, ndesc) : nullptr;
    uint8_t* dpk = packed ? d.alloc<uint8_t>(nout * rs, fill) : nullptr;
    uint64_t* dok = packed ? nullptr : d.alloc<uint64_t>((size_t)W * nout, fill);
    uint32_t* doc = packed ? nullptr : d.alloc<uint32_t>(nout, fill);
    uint64_t* stats = d.alloc<uint64_t>(kc::ST_N, 0);
    uint32_t* dfb = d.alloc<uint32_t>(ndesc, 0xff);
    uint64_t* dfbn = d.alloc<uint64_t>(1, 0);
    KCS(d.err);
    KCS(kc::launch_seg_sort(W, {dk, dc, rstride, nullptr}, dord, {dky, dst, dln, ndesc}, dof, ndesc,
                            {dok, doc, nout, nullptr}, stats, dfb, dfbn, grid, st.s, dpk));
    KCS(hipStreamSynchronize(st.s));
    if (packed) {
        KCS(hipMemcpy(out, dpk, nout * rs, hipMemcpyDeviceToHost));
    } else {
        KCS(hipMemcpy(out, dok, (size_t)W * nout * 8, hipMemcpyDeviceToHost));
        KCS(hipMemcpy(out_cnts, doc, nout * 4, hipMemcpyDeviceToHost));
    }
    KCS(hipMemcpy(err, stats + kc::ST_ERR, 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(fb_n, dfbn, 8, hipMemcpyDeviceToHost));
    if (fb) KCS(hipMemcpy(fb, dfb, ndesc * 4, hipMemcpyDeviceToHost));
    return hipSuccess;
}

// The skm finish's sequence over n records already grouped by word0 >> 48:
// launch_bucket_bounds(bits 16) -> launch_group_desc(tag 36) -> launch_seg_sort
// (every group a segment, sorted where it stands). starts: 65537 out; longest
// out. A group longer than seg_sort_cap(W) is only reported (the library then
// takes its radix sort): no sort is launched and the output keeps `fill`.
// rkeys / rcnts / out / out_cnts as in kcs_seg_sort with nout = n.
int kcs_finish_groups(int W, uint64_t n, const uint64_t* rkeys, const uint32_t* rcnts, uint64_t rstride, int packed,
                      int fill, void* out, uint32_t* out_cnts, int grid, uint64_t* starts, uint64_t* longest,
                      uint64_t* err, uint64_t* fb_n) {
    if (W < 1 || W > 4 || n == 0 || !rkeys || !rcnts || !out || !starts || !longest || !err || !fb_n)
        return hipErrorInvalidValue;
    if (rstride < n + 1 || (!packed && !out_cnts) || fill < 0 || fill > 255 || grid < 0) return hipErrorInvalidValue;
    if (grid == 0) grid = n_cu();
    if (grid < 1) return hipErrorInvalidValue;
    const uint32_t nb = 1u << 16;
    const size_t rs = 8 * (size_t)W + 4;
    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* dk = d.upload(rkeys, (size_t)W * rstride);
    uint32_t* dc = d.upload(rcnts, rstride);
    uint64_t* dstarts = d.alloc<uint64_t>((size_t)nb + 1);
    uint32_t* dord = d.alloc<uint32_t>(nb);
    uint32_t* dln = d.alloc<uint32_t>(nb);
    uint64_t* dlong = d.alloc<uint64_t>(1, 0);
    uint8_t* dpk = packed ? d.alloc<uint8_t>(n * rs, fill) : nullptr;
    uint64_t* dok = packed ? nullptr : d.alloc<uint64_t>((size_t)W * n, fill);
    uint32_t* doc = packed ? nullptr : d.alloc<uint32_t>(n, fill);
    uint64_t* stats = d.alloc<uint64_t>(kc::ST_N, 0);
    uint32_t* dfb = d.alloc<uint32_t>(nb, 0xff);
    uint64_t* dfbn = d.alloc<uint64_t>(1, 0);
    KCS(d.err);
    KCS(kc::launch_bucket_bounds(W, dk, rstride, n, 16, dstarts, st.s));
    KCS(kc::launch_group_desc(dstarts, nb, 36u, dord, dln, dlong, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(starts, dstarts, ((size_t)nb + 1) * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(longest, dlong, 8, hipMemcpyDeviceToHost));
    // the sort trusts the bounds: only monotone starts that end at n reach it
    bool sane = starts[0] == 0 && starts[nb] == n;
    for (uint32_t b = 0; b < nb && sane; b++) sane = starts[b] <= starts[b + 1];
    if (sane && *longest <= (uint64_t)kc::seg_sort_cap(W)) {
        KCS(kc::launch_seg_sort(W, {dk, dc, rstride, nullptr}, dord, {nullptr, dstarts, dln, nb}, dstarts, nb,
                                {dok, doc, n, nullptr}, stats, dfb, dfbn, grid, st.s, dpk));
        KCS(hipStreamSynchronize(st.s));
    }
    if (packed) {
        KCS(hipMemcpy(out, dpk, n * rs, hipMemcpyDeviceToHost));
    } else {
        KCS(hipMemcpy(out, dok, (size_t)W * n * 8, hipMemcpyDeviceToHost));
        KCS(hipMemcpy(out_cnts, doc, n * 4, hipMemcpyDeviceToHost));
    }
    KCS(hipMemcpy(err, stats + kc::ST_ERR, 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(fb_n, dfbn, 8, hipMemcpyDeviceToHost));
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// The sort, scan, reduce and merge primitives of the finish
// (tests/test_gpu_finish_kernels.py). Output arrays are whole host buffers of
// a size the caller states (larger than what the kernels write): the device
// copy is pre-filled with the byte `fill` and comes back whole, so padding
// and neighbours can be checked untouched. Scratch that a library function
// sizes (scan_tmp_elems, sort_hist_elems, merge_split_elems,
// merge_packed_split_elems, compact_tmp_elems) gets exactly that many
// elements plus one guard word; a call that finds the guard changed returns
// KCS_GUARD_CLOBBERED instead of a hipError_t. Index arrays that one kernel
// produces for another (flags, pos, head, split) are never taken from the
// caller: the entry points run the library's chains and hand the
// intermediates back.
// ---------------------------------------------------------------------------

int kcs_guard_clobbered(void) { return KCS_GUARD_CLOBBERED; }
int kcs_merge_tile(int W) { return w_ok(W) ? kc::merge_tile(W) : 0; }
int kcs_sort_tile(int W) { return w_ok(W) ? kc::sort_tile(W) : 0; }
int kcs_sort_grid(uint64_t n) { return kc::sort_grid(n); }
int kcs_scan_tile(void) { return kc::scan_tile(); }
int kcs_compact_grid(void) { return kc::compact_grid(); }
int kcs_elem_grid_cap(void) { return kc::elem_grid_cap(); }
int kcs_slot_words(int W) { return w_ok(W) ? kc::slot_words(W) : 0; }

// Exclusive scan of n u32 (bits32) or u64 elements. out: out_elems >= n
// elements, all returned. inplace: the input is copied to the front of the
// output buffer and scanned where it stands.
int kcs_scan(int bits32, uint64_t n, const void* in, void* out, uint64_t out_elems, int inplace, int fill) {
    if (n == 0 || !in || !out || out_elems < n || !fill_ok(fill)) return hipErrorInvalidValue;
    const size_t es = bits32 ? 4 : 8;
    Stream st;
    KCS(st.err);
    Dev d;
    uint8_t* din = inplace ? nullptr : d.upload((const uint8_t*)in, n * es);
    uint8_t* dout = d.alloc<uint8_t>(out_elems * es, fill);
    const uint64_t te = kc::scan_tmp_elems(n);
    uint8_t* tmp = d.alloc<uint8_t>((te + 1) * es, kGuard);
    KCS(d.err);
    if (inplace) {
        KCS(hipMemcpy(dout, in, n * es, hipMemcpyHostToDevice));
        din = dout;
    }
    if (bits32)
        KCS(kc::launch_scan_u32((const uint32_t*)din, (uint32_t*)dout, n, (uint32_t*)tmp, st.s));
    else
        KCS(kc::launch_scan_u64((const uint64_t*)din, (uint64_t*)dout, n, (uint64_t*)tmp, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(out, dout, out_elems * es, hipMemcpyDeviceToHost));
    return guard_check(tmp + te * es, es);
}

// OR / AND of every key word: or_and_out = 2 W words (or[0..W), and[W..2W)).
int kcs_key_bits(int W, uint64_t n, const uint64_t* keys, uint64_t stride, uint64_t* or_and_out) {
    if (!w_ok(W) || n == 0 || !keys || !or_and_out || stride < n) return hipErrorInvalidValue;
    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* dk = d.upload(keys, (size_t)W * stride);
    std::vector<uint64_t> init(2 * (size_t)W, 0);
    for (int j = 0; j < W; j++) init[W + j] = ~0ull;
    uint64_t* db = d.upload(init.data(), init.size());
    KCS(d.err);
    KCS(kc::launch_key_bits(W, dk, stride, n, db, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(or_and_out, db, 2 * (size_t)W * 8, hipMemcpyDeviceToHost));
    return hipSuccess;
}

// One launch_sort_pass (hashed = false) over n SoA records at `stride` (input
// and output share it, as in the library). vals_in / vals_out both or neither.
// grid 0: sort_grid(n). keys_out: W x stride words, vals_out: stride, all
// returned.
int kcs_sort_pass(int W, uint64_t n, const uint64_t* keys_in, const uint32_t* vals_in, uint64_t stride, int word,
                  int shift, int grid, uint64_t* keys_out, uint32_t* vals_out, int fill) {
    if (!w_ok(W) || n == 0 || !keys_in || !keys_out || stride < n || !fill_ok(fill)) return hipErrorInvalidValue;
    if ((vals_in != nullptr) != (vals_out != nullptr)) return hipErrorInvalidValue;
    if (word < 0 || word >= W || shift < 0 || shift > 56 || grid < 0 || grid > 4096) return hipErrorInvalidValue;
    if (grid == 0) grid = kc::sort_grid(n);
    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* dk = d.upload(keys_in, (size_t)W * stride);
    uint64_t* dko = d.alloc<uint64_t>((size_t)W * stride, fill);
    uint32_t* dv = vals_in ? d.upload(vals_in, stride) : nullptr;
    uint32_t* dvo = vals_in ? d.alloc<uint32_t>(stride, fill) : nullptr;
    const uint64_t he = kc::sort_hist_elems(grid);
    uint64_t* hist = d.alloc<uint64_t>(he + 1, kGuard);
    KCS(d.err);
    KCS(kc::launch_sort_pass(W, dk, dko, dv, dvo, stride, n, word, shift, hist, grid, false, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(keys_out, dko, (size_t)W * stride * 8, hipMemcpyDeviceToHost));
    if (vals_out) KCS(hipMemcpy(vals_out, dvo, stride * 4, hipMemcpyDeviceToHost));
    return guard_check(hist + he, 8);
}

// heads -> scan -> (rle_scatter -> rle_counts | memset -> reduce_add) -> pack
// over n SoA records (cnts == nullptr: the run-length chain of flush_keys, the
// counts are run lengths; else the segmented sum of reduce_pack). All of
// flags_out, pos_out (n each), out_keys (W x ostride), out_cnts (ostride),
// head_out (ostride, run-length chain only) and packed_out (ostride records)
// come back whole; ostride >= n, so no key sequence can index past them.
static int reduce_chain(int W, uint64_t n, const uint64_t* keys, const uint32_t* cnts, uint64_t stride,
                        uint32_t* flags_out, uint32_t* pos_out, uint64_t* m_out, uint64_t* out_keys,
                        uint64_t ostride, uint32_t* out_cnts, uint32_t* head_out, uint8_t* packed_out, int fill) {
    if (!w_ok(W) || n == 0 || n > 0xffffffffull || !keys || !flags_out || !pos_out || !m_out || !out_keys ||
        !out_cnts || !packed_out || stride < n || ostride < n || !fill_ok(fill))
        return hipErrorInvalidValue;
    if (!cnts && !head_out) return hipErrorInvalidValue;
    const size_t rs = 8 * (size_t)W + 4;
    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* dk = d.upload(keys, (size_t)W * stride);
    uint32_t* dc = cnts ? d.upload(cnts, stride) : nullptr;
    uint32_t* flags = d.alloc<uint32_t>(n, fill);
    uint32_t* pos = d.alloc<uint32_t>(n, fill);
    const uint64_t te = kc::scan_tmp_elems(n);
    uint32_t* tmp = d.alloc<uint32_t>(te + 1, kGuard);
    uint64_t* dko = d.alloc<uint64_t>((size_t)W * ostride, fill);
    uint32_t* dco = d.alloc<uint32_t>(ostride, fill);
    uint32_t* head = cnts ? nullptr : d.alloc<uint32_t>(ostride, fill);
    uint8_t* dpk = d.alloc<uint8_t>(ostride * rs, fill);
    KCS(d.err);
    KCS(kc::launch_rle_heads(W, dk, stride, n, flags, st.s));
    KCS(kc::launch_scan_u32(flags, pos, n, tmp, st.s));
    uint32_t last[2];
    KCS(hipMemcpyAsync(&last[0], pos + (n - 1), 4, hipMemcpyDeviceToHost, st.s));
    KCS(hipMemcpyAsync(&last[1], flags + (n - 1), 4, hipMemcpyDeviceToHost, st.s));
    KCS(hipStreamSynchronize(st.s));
    const uint64_t m = (uint64_t)last[0] + last[1];
    *m_out = m;
    // the scatter trusts flags / pos: only a result that cannot leave the output reaches it
    if (m >= 1 && m <= n) {
        if (cnts) {
            KCS(hipMemsetAsync(dco, 0, m * 4, st.s));
            KCS(kc::launch_reduce_add(W, dk, stride, dc, n, flags, pos, dko, ostride, dco, st.s));
        } else {
            KCS(kc::launch_rle_scatter(W, dk, stride, n, flags, pos, dko, ostride, head, st.s));
            KCS(kc::launch_rle_counts(head, m, n, dco, st.s));
        }
        KCS(kc::launch_pack(W, dko, ostride, dco, m, dpk, st.s));
        KCS(hipStreamSynchronize(st.s));
    }
    KCS(hipMemcpy(flags_out, flags, n * 4, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(pos_out, pos, n * 4, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(out_keys, dko, (size_t)W * ostride * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(out_cnts, dco, ostride * 4, hipMemcpyDeviceToHost));
    if (head) KCS(hipMemcpy(head_out, head, ostride * 4, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(packed_out, dpk, ostride * rs, hipMemcpyDeviceToHost));
    return guard_check(tmp + te, 4);
}

int kcs_rle_chain(int W, uint64_t n, const uint64_t* keys, uint64_t stride, uint32_t* flags_out, uint32_t* pos_out,
                  uint64_t* m_out, uint64_t* out_keys, uint64_t ostride, uint32_t* out_cnts, uint32_t* head_out,
                  uint8_t* packed_out, int fill) {
    if (!head_out) return hipErrorInvalidValue;
    return reduce_chain(W, n, keys, nullptr, stride, flags_out, pos_out, m_out, out_keys, ostride, out_cnts, head_out,
                        packed_out, fill);
}

// reduce_pack's memset clears the n counts of its buffer; here only the m
// that are summed into, so that the rest keeps the sentinel
int kcs_reduce_chain(int W, uint64_t n, const uint64_t* keys, const uint32_t* cnts, uint64_t stride,
                     uint32_t* flags_out, uint32_t* pos_out, uint64_t* m_out, uint64_t* out_keys, uint64_t ostride,
                     uint32_t* out_cnts, uint8_t* packed_out, int fill) {
    if (!cnts) return hipErrorInvalidValue;
    return reduce_chain(W, n, keys, cnts, stride, flags_out, pos_out, m_out, out_keys, ostride, out_cnts, nullptr,
                        packed_out, fill);
}

// SoA -> packed: out holds out_recs >= n records, all returned.
int kcs_pack(int W, uint64_t n, const uint64_t* keys, const uint32_t* cnts, uint64_t stride, uint8_t* out,
             uint64_t out_recs, int fill) {
    if (!w_ok(W) || n == 0 || !keys || !cnts || !out || stride < n || out_recs < n || !fill_ok(fill))
        return hipErrorInvalidValue;
    const size_t rs = 8 * (size_t)W + 4;
    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* dk = d.upload(keys, (size_t)W * stride);
    uint32_t* dc = d.upload(cnts, stride);
    uint8_t* dpk = d.alloc<uint8_t>(out_recs * rs, fill);
    KCS(d.err);
    KCS(kc::launch_pack(W, dk, stride, dc, n, dpk, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(out, dpk, out_recs * rs, hipMemcpyDeviceToHost));
    return hipSuccess;
}

// packed -> SoA: keys_out W x ostride words, cnts_out ostride, all returned.
int kcs_unpack(int W, uint64_t n, const uint8_t* packed, uint64_t* keys_out, uint64_t ostride, uint32_t* cnts_out,
               int fill) {
    if (!w_ok(W) || n == 0 || !packed || !keys_out || !cnts_out || ostride < n || !fill_ok(fill))
        return hipErrorInvalidValue;
    const size_t rs = 8 * (size_t)W + 4;
    Stream st;
    KCS(st.err);
    Dev d;
    uint8_t* dpk = d.upload(packed, n * rs);
    uint64_t* dk = d.alloc<uint64_t>((size_t)W * ostride, fill);
    uint32_t* dc = d.alloc<uint32_t>(ostride, fill);
    KCS(d.err);
    KCS(kc::launch_unpack(W, dpk, n, dk, ostride, dc, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(keys_out, dk, (size_t)W * ostride * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(cnts_out, dc, ostride * 4, hipMemcpyDeviceToHost));
    return hipSuccess;
}

// launch_compact then launch_append_key0 over a table of cap slots
// (table_words >= cap * slot_words(W) words). The records go to W arrays at
// stride out_cap, so keys_out holds W x out_cap + pad words and cnts_out
// out_cap + pad, all returned; cursor_out: the records counted (+ key 0 when
// it was appended).
int kcs_compact(int W, uint64_t cap, const uint64_t* table, uint64_t table_words, uint64_t out_cap, int key0_present,
                uint64_t key0_count, uint64_t* keys_out, uint32_t* cnts_out, uint64_t pad, uint64_t* cursor_out,
                int fill) {
    if (!w_ok(W) || cap == 0 || !table || !keys_out || !cnts_out || !cursor_out || !fill_ok(fill))
        return hipErrorInvalidValue;
    if (table_words / (uint64_t)kc::slot_words(W) < cap) return hipErrorInvalidValue;
    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* dt = d.upload(table, table_words);
    uint64_t* dk = d.alloc<uint64_t>((size_t)W * out_cap + pad, fill);
    uint32_t* dc = d.alloc<uint32_t>(out_cap + pad, fill);
    uint64_t* cursor = d.alloc<uint64_t>(1, fill);
    const uint64_t te = kc::compact_tmp_elems();
    uint64_t* tmp = d.alloc<uint64_t>(te + 1, kGuard);
    std::vector<uint64_t> stats(kc::ST_N, 0);
    stats[kc::ST_KEY0] = key0_count;
    stats[kc::ST_KEY0_PRESENT] = key0_present ? 1 : 0;
    uint64_t* dstats = d.upload(stats.data(), stats.size());
    KCS(d.err);
    KCS(kc::launch_compact(W, dt, cap, dk, dc, out_cap, cursor, tmp, st.s));
    KCS(kc::launch_append_key0(W, dk, dc, out_cap, cursor, dstats, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(keys_out, dk, ((size_t)W * out_cap + pad) * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(cnts_out, dc, (out_cap + pad) * 4, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(cursor_out, cursor, 8, hipMemcpyDeviceToHost));
    return guard_check(tmp + te, 8);
}

// launch_merge of two sorted SoA runs. adjacent == 0: A = ka / ca (W x sa, sa
// >= na), B = kb / cb (W x sb), output at index 0 of ko / co. adjacent != 0:
// ka / ca is one buffer of stride sa holding A at [a_off, a_off + na) and B
// right behind it (kb, cb null, sb ignored), and the output goes to
// [a_off, a_off + na + nb) of ko / co: offset base pointers into shared
// buffers, as merge_runs_list passes them. ko: W x so words, co: so, all
// returned. ntiles_out, wgs_out: the tiles and the workgroups that walk them.
int kcs_merge(int W, const uint64_t* ka, const uint32_t* ca, uint64_t sa, uint64_t na, const uint64_t* kb,
              const uint32_t* cb, uint64_t sb, uint64_t nb, int adjacent, uint64_t a_off, uint64_t* ko, uint32_t* co,
              uint64_t so, int grid_cap, int fill, uint64_t* ntiles_out, uint64_t* wgs_out) {
    if (!w_ok(W) || na + nb == 0 || !ka || !ca || !ko || !co || grid_cap < 1 || !fill_ok(fill))
        return hipErrorInvalidValue;
    if (adjacent) {
        if (kb || cb || a_off > sa || na + nb > sa - a_off || a_off > so || na + nb > so - a_off)
            return hipErrorInvalidValue;
        sb = sa;
    } else {
        if (!kb || !cb || a_off != 0 || sa < na || sb < nb || so < na + nb) return hipErrorInvalidValue;
    }
    const uint64_t* hb = adjacent ? ka + a_off + na : kb;
    if (!soa_sorted(W, ka + a_off, sa, na) || !soa_sorted(W, hb, sb, nb)) return hipErrorInvalidValue;
    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* dka = d.upload(ka, (size_t)W * sa);
    uint32_t* dca = d.upload(ca, sa);
    uint64_t* dkb = adjacent ? dka + a_off + na : d.upload(kb, (size_t)W * sb);
    uint32_t* dcb = adjacent ? dca + a_off + na : d.upload(cb, sb);
    uint64_t* dko = d.alloc<uint64_t>((size_t)W * so, fill);
    uint32_t* dco = d.alloc<uint32_t>(so, fill);
    const uint64_t se = kc::merge_split_elems(na + nb);
    uint64_t* split = d.alloc<uint64_t>(se + 1, kGuard);
    KCS(d.err);
    const uint64_t tile = (uint64_t)kc::merge_tile(W), nt = (na + nb + tile - 1) / tile;
    if (nt + 1 > se) return hipErrorInvalidValue;
    if (ntiles_out) *ntiles_out = nt;
    if (wgs_out) *wgs_out = nt < (uint64_t)grid_cap ? nt : (uint64_t)grid_cap;
    KCS(kc::launch_merge(W, dka + a_off, dca + a_off, sa, na, dkb, dcb, sb, nb, dko + a_off, dco + a_off, so, split,
                         st.s, grid_cap));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(ko, dko, (size_t)W * so * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(co, dco, so * 4, hipMemcpyDeviceToHost));
    return guard_check(split + se, 8);
}

// launch_merge_packed of two sorted packed runs (repeated keys allowed). Each
// of A, B and the output starts *_skip records into a 16-byte-aligned
// allocation: skip 0 gives a 16-byte-aligned run, skip 1 one aligned to 4
// bytes only (a record is 8 W + 4 bytes). out: out_recs >= out_skip + na + nb
// records, all returned (the skipped ones and the tail must keep `fill`).
// out_align: the output pointer's address modulo 16; dup_out: the flag.
int kcs_merge_packed(int W, const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t nb, uint64_t a_skip,
                     uint64_t b_skip, uint64_t out_skip, int grid_cap, uint8_t* out, uint64_t out_recs, int fill,
                     uint32_t* dup_out, uint32_t* out_align, uint64_t* ntiles_out, uint64_t* wgs_out) {
    if (!w_ok(W) || na + nb == 0 || (na && !a) || (nb && !b) || !out || !dup_out || grid_cap < 1 || !fill_ok(fill))
        return hipErrorInvalidValue;
    if (out_skip > out_recs || na + nb > out_recs - out_skip || a_skip > 64 || b_skip > 64)
        return hipErrorInvalidValue;
    const size_t rs = 8 * (size_t)W + 4;
    if (!packed_sorted(W, a, na) || !packed_sorted(W, b, nb)) return hipErrorInvalidValue;
    Stream st;
    KCS(st.err);
    Dev d;
    uint8_t* da = d.alloc<uint8_t>((a_skip + na) * rs, fill);
    uint8_t* db = d.alloc<uint8_t>((b_skip + nb) * rs, fill);
    uint8_t* dout = d.alloc<uint8_t>(out_recs * rs, fill);
    const uint64_t se = kc::merge_packed_split_elems(W, na + nb);
    uint64_t* split = d.alloc<uint64_t>(se + 1, kGuard);
    uint32_t* dup = d.alloc<uint32_t>(1, 0);
    KCS(d.err);
    if (((uintptr_t)da | (uintptr_t)db | (uintptr_t)dout) & 15u) return hipErrorInvalidValue;
    if (na) KCS(hipMemcpy(da + a_skip * rs, a, na * rs, hipMemcpyHostToDevice));
    if (nb) KCS(hipMemcpy(db + b_skip * rs, b, nb * rs, hipMemcpyHostToDevice));
    const uint64_t tile = (uint64_t)kc::merge_tile(W), nt = (na + nb + tile - 1) / tile;
    if (nt + 1 > se) return hipErrorInvalidValue;
    if (ntiles_out) *ntiles_out = nt;
    if (wgs_out) *wgs_out = nt < (uint64_t)grid_cap ? nt : (uint64_t)grid_cap;
    if (out_align) *out_align = (uint32_t)((uintptr_t)(dout + out_skip * rs) & 15u);
    KCS(kc::launch_merge_packed(W, da + a_skip * rs, na, db + b_skip * rs, nb, dout + out_skip * rs, split, dup, st.s,
                                grid_cap));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(out, dout, out_recs * rs, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(dup_out, dup, 4, hipMemcpyDeviceToHost));
    return guard_check(split + se, 8);
}

// The set-operation passes over two sorted packed runs with one record per key
// (launch_setop_count, scan, launch_setop_emit), placed like kcs_merge_packed's
// runs: A, B and the output start *_skip records into 16-byte-aligned
// allocations. out: out_recs >= out_skip + na + nb records, all returned (only
// [out_skip, out_skip + *n_out) may lose `fill`). Guard words sit behind the
// split array and behind the tile counts / bases / scan scratch.
int kcs_setop_tile(int W) { return w_ok(W) ? kc::setop_tile(W) : 0; }

int kcs_setop(int W, const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t nb, uint64_t a_skip, uint64_t b_skip,
              uint64_t out_skip, uint32_t op, uint32_t mode, int grid_cap, uint8_t* out, uint64_t out_recs, int fill,
              uint64_t* n_out, uint32_t* out_align, uint64_t* ntiles_out, uint64_t* wgs_out) {
    if ((na && !a) || (nb && !b) || !out || !n_out || !fill_ok(fill)) return hipErrorInvalidValue;
    // the launcher refuses these itself, before any launch
    if (!w_ok(W) || op > 3 || mode > 4 || grid_cap < 1)
        return (int)kc::launch_setop_count(W, nullptr, 0, nullptr, 0, op, mode, nullptr, nullptr, nullptr, grid_cap);
    if (out_skip > out_recs || na + nb > out_recs - out_skip || a_skip > 64 || b_skip > 64)
        return hipErrorInvalidValue;
    const size_t rs = 8 * (size_t)W + 4;
    if (!packed_sorted(W, a, na) || !packed_sorted(W, b, nb)) return hipErrorInvalidValue;
    for (int r = 0; r < 2; r++) {  // distinct: no equal neighbours
        const uint8_t* p = r ? b : a;
        const uint64_t n = r ? nb : na;
        for (uint64_t i = 1; i < n; i++)
            if (memcmp(p + (i - 1) * rs, p + i * rs, 8 * (size_t)W) == 0) return hipErrorInvalidValue;
    }
    Stream st;
    KCS(st.err);
    Dev d;
    uint8_t* da = d.alloc<uint8_t>((a_skip + na) * rs, fill);
    uint8_t* db = d.alloc<uint8_t>((b_skip + nb) * rs, fill);
    uint8_t* dout = d.alloc<uint8_t>(out_recs * rs, fill);
    const uint64_t se = kc::merge_packed_split_elems(W, na + nb);
    uint64_t* split = d.alloc<uint64_t>(se + 1, kGuard);
    const uint64_t tile = (uint64_t)kc::setop_tile(W), nt = (na + nb + tile - 1) / tile;
    // tile counts, bases, the total, the scan's scratch, a guard word
    const uint64_t te = 2 * nt + 1 + kc::scan_tmp_elems(nt);
    uint64_t* cnt = d.alloc<uint64_t>(te + 1, kGuard);
    KCS(d.err);
    if (((uintptr_t)da | (uintptr_t)db | (uintptr_t)dout) & 15u) return hipErrorInvalidValue;
    if (na) KCS(hipMemcpy(da + a_skip * rs, a, na * rs, hipMemcpyHostToDevice));
    if (nb) KCS(hipMemcpy(db + b_skip * rs, b, nb * rs, hipMemcpyHostToDevice));
    if (nt + 1 > se) return hipErrorInvalidValue;
    if (ntiles_out) *ntiles_out = nt;
    if (wgs_out) *wgs_out = nt < (uint64_t)grid_cap ? nt : (uint64_t)grid_cap;
    if (out_align) *out_align = (uint32_t)((uintptr_t)(dout + out_skip * rs) & 15u);
    *n_out = 0;
    if (nt) {
        uint64_t* base = cnt + nt;
        uint64_t* total = base + nt;
        uint64_t* tmp = total + 1;
        KCS(kc::launch_setop_count(W, da + a_skip * rs, na, db + b_skip * rs, nb, op, mode, split, cnt, st.s,
                                   grid_cap));
        KCS(kc::launch_scan_u64(cnt, base, nt, tmp, st.s));
        KCS(kc::launch_sum_last(base, cnt, nt, total, st.s));
        KCS(hipMemcpyAsync(n_out, total, 8, hipMemcpyDeviceToHost, st.s));
        KCS(hipStreamSynchronize(st.s));
        // the emit pass trusts the bases: they must end inside the output
        if (*n_out > na + nb) return hipErrorInvalidValue;
        KCS(kc::launch_setop_emit(W, da + a_skip * rs, na, db + b_skip * rs, nb, op, mode, split, base,
                                  dout + out_skip * rs, st.s, grid_cap));
        KCS(hipStreamSynchronize(st.s));
    }
    KCS(hipMemcpy(out, dout, out_recs * rs, hipMemcpyDeviceToHost));
    const int g = guard_check(split + se, 8);
    return g ? g : guard_check(cnt + te, 8);
}

// bounds_out[o] for o in [0, world]: the first of n packed records owned by o or later.
int kcs_owner_bounds(int W, uint64_t n, const uint8_t* packed, uint32_t world, uint64_t* bounds_out, uint64_t pad,
                     int fill) {
    if (!w_ok(W) || (n && !packed) || world < 1 || world > 65536 || !bounds_out || !fill_ok(fill))
        return hipErrorInvalidValue;
    const size_t rs = 8 * (size_t)W + 4;
    Stream st;
    KCS(st.err);
    Dev d;
    uint8_t* dpk = d.alloc<uint8_t>(n * rs, fill);
    uint64_t* db = d.alloc<uint64_t>((size_t)world + 1 + pad, fill);
    KCS(d.err);
    if (n) KCS(hipMemcpy(dpk, packed, n * rs, hipMemcpyHostToDevice));
    KCS(kc::launch_owner_bounds(dpk, (int)rs, n, world, db, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(bounds_out, db, ((size_t)world + 1 + pad) * 8, hipMemcpyDeviceToHost));
    return hipSuccess;
}

// starts_out[b] for b in [0, 2^bits] (+ pad words). stride 0: the keys are n
// items of W consecutive words (AoS); else W arrays at stride >= n.
int kcs_bucket_bounds(int W, uint64_t n, const uint64_t* keys, uint64_t stride, int bits, uint64_t* starts_out,
                      uint64_t pad, int fill) {
    if (!w_ok(W) || n == 0 || !keys || (stride && stride < n) || bits < 1 || bits > 20 || !starts_out ||
        !fill_ok(fill))
        return hipErrorInvalidValue;
    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* dk = d.upload(keys, (size_t)W * (stride ? stride : n));
    const size_t ns = ((size_t)1 << bits) + 1 + pad;
    uint64_t* ds = d.alloc<uint64_t>(ns, fill);
    KCS(d.err);
    KCS(kc::launch_bucket_bounds(W, dk, stride, n, bits, ds, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(starts_out, ds, ns * 8, hipMemcpyDeviceToHost));
    return hipSuccess;
}

// launch_packed_seg_copy: segment order[d] of src (nsrc records) moves to
// record base + out_off[d] of dst (ndst records, all returned).
int kcs_packed_seg_copy(int W, uint64_t nsrc, const uint8_t* src, uint64_t ndst, uint8_t* dst, uint64_t ndesc,
                        const uint32_t* order, const uint64_t* dstart, const uint32_t* dlen, const uint64_t* out_off,
                        uint64_t base, int grid, int fill) {
    if (!w_ok(W) || nsrc == 0 || ndst == 0 || ndesc == 0 || !src || !dst || !order || !dstart || !dlen || !out_off ||
        grid < 1 || grid > 4096 || base > ndst || !fill_ok(fill))
        return hipErrorInvalidValue;
    for (uint64_t i = 0; i < ndesc; i++) {
        const uint32_t o = order[i];
        if (o >= ndesc) return hipErrorInvalidValue;
        const uint64_t len = dlen[o] & 0xffffffu;
        if (dstart[o] > nsrc || len > nsrc - dstart[o]) return hipErrorInvalidValue;
        if (out_off[i] > ndst - base || len > ndst - base - out_off[i]) return hipErrorInvalidValue;
    }
    const size_t rs = 8 * (size_t)W + 4;
    Stream st;
    KCS(st.err);
    Dev d;
    uint8_t* ds = d.upload(src, nsrc * rs);
    uint8_t* dd = d.alloc<uint8_t>(ndst * rs, fill);
    uint32_t* dord = d.upload(order, ndesc);
    uint64_t* dst0 = d.upload(dstart, ndesc);
    uint32_t* dln = d.upload(dlen, ndesc);
    uint64_t* dof = d.upload(out_off, ndesc);
    KCS(d.err);
    KCS(kc::launch_packed_seg_copy(W, ds, dd, dord, dst0, dln, dof, ndesc, base, grid, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(dst, dd, ndst * rs, hipMemcpyDeviceToHost));
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// The two ends of the super-k-mer engine (tests/test_gpu_skm_kernels.py): the
// front ends F / F2 / F3 behind launch_skm_front, P5a (count_rec_k,
// dedup_total_k) and P5 (count_skm_k<W>). Every output buffer is pre-filled
// with `fill` and followed by 8 guard bytes (KCS_GUARD_CLOBBERED when they
// change); the buffers the kernels need clear (statistics, cursors, the
// global table) start at 0.
// ---------------------------------------------------------------------------

int kcs_skm_lds_slots(int W) { return (W >= 1 && W <= 3) ? kc::skm_lds_slots(W) : 0; }
uint32_t kcs_p5a_groups(void) { return kc::rec_dedup_groups(); }
uint64_t kcs_err_spill_overflow(void) { return (uint64_t)kc::ERR_SPILL_OVERFLOW; }
uint64_t kcs_err_rec_overflow(void) { return (uint64_t)kc::ERR_REC_OVERFLOW; }
int kcs_st_n(void) { return (int)kc::ST_N; }
int kcs_invalid_value(void) { return (int)hipErrorInvalidValue; }
// out[0..10): the indices of ST_VALID, ST_KEY0, ST_KEY0_PRESENT, ST_CLAIMED, ST_ERR, ST_SPILL2_FILL,
// ST_P5_PASSES, ST_P5_ABORTS, ST_P5_KEYS, ST_DEDUP in a statistics array. Its callers hold exactly ten
// entries: it writes no more, and further indices have entry points of their own (below).
int kcs_stat_indices(int* out) {
    if (!out) return hipErrorInvalidValue;
    const int idx[10] = {kc::ST_VALID,       kc::ST_KEY0,      kc::ST_KEY0_PRESENT, kc::ST_CLAIMED, kc::ST_ERR,
                         kc::ST_SPILL2_FILL, kc::ST_P5_PASSES, kc::ST_P5_ABORTS,    kc::ST_P5_KEYS, kc::ST_DEDUP};
    for (int i = 0; i < 10; i++) out[i] = idx[i];
    return hipSuccess;
}
// out[0..2): the indices of ST_P5_MAXM, ST_DESC_FILL
int kcs_stat_indices_p5(int* out) {
    if (!out) return hipErrorInvalidValue;
    out[0] = kc::ST_P5_MAXM;
    out[1] = kc::ST_DESC_FILL;
    return hipSuccess;
}

// out[0..7): ok, m, K', nmax, R of skm_geometry(L, k), skm_f3_applies(L, k), groups_per_read(L)
int kcs_skm_geometry(int L, int k, int* out) {
    if (!out || L < 1 || k < 1) return hipErrorInvalidValue;
    const kc::SkmGeom g = kc::skm_geometry(L, k);
    out[0] = g.ok ? 1 : 0;
    out[1] = g.ok ? g.m : 0;
    out[2] = g.ok ? g.Kp : 0;
    out[3] = g.ok ? g.nmax : 0;
    out[4] = g.ok ? g.R : 0;
    out[5] = kc::skm_f3_applies(L, k) ? 1 : 0;
    out[6] = kc::groups_per_read(L);
    return hipSuccess;
}

// E + F over n_reads reads. seq_off == seq_end == nullptr: read r is the L
// bytes at text + r L (launch_encode_reads); else read r is text
// [seq_off[r], seq_end[r]) of at most L bytes (launch_encode_reads_var, its
// rlen handed to the front end). The front end is launch_skm_front's choice
// (KC_NO_F3 / KC_NO_F2 select it, as in production). The code and mask rows
// get the slack the library's own buffers have (16 bytes).
//   pool_out   RW x pool_cap words (RW = W + 1), dig1_out pool_cap bytes (want_dig1)
//   cursor_out the final *pool_cursor, stats_out ST_N counters
//   codes_out / inval_out  n_reads x groups_per_read(L) each; rlen_out n_reads (variable form)
int kcs_skm_front(const uint8_t* text, uint64_t text_len, uint64_t n_reads, int L, int k, const uint64_t* seq_off,
                  const uint64_t* seq_end, uint64_t pool_cap, int want_dig1, int grid_cap, int fill,
                  uint64_t* pool_out, uint8_t* dig1_out, uint64_t* cursor_out, uint64_t* stats_out,
                  uint32_t* codes_out, uint16_t* inval_out, uint16_t* rlen_out) {
    if (!text || n_reads == 0 || n_reads > (1u << 20) || L < 1 || L > 65535 || k < 1 || pool_cap == 0 ||
        pool_cap > (1u << 26) || !pool_out || !cursor_out || !stats_out || !codes_out || !inval_out ||
        grid_cap < 1 || grid_cap > 4096 || !fill_ok(fill))
        return hipErrorInvalidValue;
    if ((seq_off != nullptr) != (seq_end != nullptr) || (seq_off && !rlen_out) || (want_dig1 && !dig1_out))
        return hipErrorInvalidValue;
    const kc::SkmGeom g = kc::skm_geometry(L, k);
    if (!g.ok) return hipErrorInvalidValue;
    if (seq_off) {
        for (uint64_t r = 0; r < n_reads; r++)
            if (seq_off[r] > seq_end[r] || seq_end[r] > text_len || seq_end[r] - seq_off[r] > (uint64_t)L)
                return hipErrorInvalidValue;
    } else if (text_len < n_reads * (uint64_t)L) {
        return hipErrorInvalidValue;
    }
    const int RW = (k + 31) / 32 + 1;
    const uint64_t ng = n_reads * (uint64_t)kc::groups_per_read(L);
    Stream st;
    KCS(st.err);
    Dev d;
    uint8_t* dtext = d.alloc<uint8_t>(text_len + 16, 0);
    uint64_t* doff = seq_off ? d.upload(seq_off, n_reads) : nullptr;
    uint64_t* dend = seq_off ? d.upload(seq_end, n_reads) : nullptr;
    uint32_t* codes = d.alloc<uint32_t>(ng + 4, 0);
    uint16_t* inval = d.alloc<uint16_t>(ng + 8, 0);
    uint16_t* rlen = seq_off ? d.alloc<uint16_t>(n_reads + 8, 0) : nullptr;
    uint64_t* pool = alloc_guarded<uint64_t>(d, (size_t)RW * pool_cap, fill);
    uint8_t* dig1 = want_dig1 ? alloc_guarded<uint8_t>(d, pool_cap, fill) : nullptr;
    uint64_t* cursor = d.alloc<uint64_t>(1, 0);
    uint64_t* stats = d.alloc<uint64_t>(kc::ST_N, 0);
    KCS(d.err);
    KCS(hipMemcpy(dtext, text, text_len, hipMemcpyHostToDevice));
    kc::CountLaunch l{};
    l.base = dtext;
    l.seq_off = nullptr;
    l.read0 = 0;
    l.n_reads = n_reads;
    l.L = L;
    l.k = k;
    l.stats = stats;
    l.codes = codes;
    l.inval = inval;
    l.rlen = rlen;
    if (seq_off)
        KCS(kc::launch_encode_reads_var(dtext, doff, dend, n_reads, L, k, codes, inval, rlen, stats, st.s));
    else
        KCS(kc::launch_encode_reads(l, codes, inval, st.s));
    KCS(kc::launch_skm_front(l, g, pool, pool_cap, cursor, grid_cap, st.s, dig1));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(pool_out, pool, (size_t)RW * pool_cap * 8, hipMemcpyDeviceToHost));
    if (dig1) KCS(hipMemcpy(dig1_out, dig1, pool_cap, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(cursor_out, cursor, 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(stats_out, stats, kc::ST_N * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(codes_out, codes, ng * 4, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(inval_out, inval, ng * 2, hipMemcpyDeviceToHost));
    if (rlen) KCS(hipMemcpy(rlen_out, rlen, n_reads * 2, hipMemcpyDeviceToHost));
    const int gp = guarded_ok(pool, (size_t)RW * pool_cap);
    if (gp != hipSuccess) return gp;
    return dig1 ? guarded_ok(dig1, pool_cap) : (int)hipSuccess;
}

// P5a over buckets [b0, b1) of W = 1 records grouped by bucket, then
// launch_dedup_total over the same buckets.
//   recs       2 x stride words, in and out; starts: nb + 1 bounds (b1 <= nb)
//   use_over   the overflow tail [over_start, over_limit) of recs / cnt: it
//              must lie behind every bucket (over_start >= starts[nb]) and
//              inside the records (over_limit <= stride)
//   cnt_out    stride; dlen_out, dpos_out: nb each (only [b0, b1) are written)
//   over_cursor_out  the final *over_cursor (over_start when !use_over)
//   dedup_out  stats[ST_DEDUP]
int kcs_count_rec(uint64_t* recs, uint64_t stride, const uint64_t* starts, uint32_t nb, uint32_t b0, uint32_t b1,
                  int use_over, uint64_t over_start, uint64_t over_limit, int grid, int fill, uint32_t* cnt_out,
                  uint32_t* dlen_out, uint64_t* dpos_out, uint64_t* over_cursor_out, uint64_t* dedup_out) {
    if (!recs || stride == 0 || stride > (1u << 26) || !starts_ok(starts, nb, stride) || b0 >= b1 || b1 > nb ||
        grid < 0 || grid > 4096 || !fill_ok(fill) || !cnt_out || !dlen_out || !dpos_out || !over_cursor_out ||
        !dedup_out)
        return hipErrorInvalidValue;
    if (use_over && (over_limit > stride || over_start < starts[nb])) return hipErrorInvalidValue;
    if (grid == 0) grid = n_cu();
    if (grid < 1) return hipErrorInvalidValue;
    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* drecs = alloc_guarded<uint64_t>(d, 2 * (size_t)stride, fill);
    uint64_t* dstarts = d.upload(starts, (size_t)nb + 1);
    uint32_t* cnt = alloc_guarded<uint32_t>(d, stride, fill);
    uint32_t* dlen = alloc_guarded<uint32_t>(d, nb, fill);
    uint64_t* dpos = alloc_guarded<uint64_t>(d, nb, fill);
    uint64_t* cursor = d.upload(&over_start, 1);
    uint64_t* stats = d.alloc<uint64_t>(kc::ST_N, 0);
    KCS(d.err);
    KCS(hipMemcpy(drecs, recs, 2 * (size_t)stride * 8, hipMemcpyHostToDevice));
    KCS(kc::launch_count_rec(drecs, stride, dstarts, b0, b1, cnt, dlen, grid, st.s, use_over ? cursor : nullptr,
                             use_over ? over_limit : 0, dpos));
    KCS(kc::launch_dedup_total(dlen + b0, dstarts + b0, b1 - b0, stats, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(recs, drecs, 2 * (size_t)stride * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(cnt_out, cnt, stride * 4, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(dlen_out, dlen, (size_t)nb * 4, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(dpos_out, dpos, (size_t)nb * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(over_cursor_out, cursor, 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(dedup_out, stats + kc::ST_DEDUP, 8, hipMemcpyDeviceToHost));
    int g = guarded_ok(drecs, 2 * (size_t)stride);
    if (g == hipSuccess) g = guarded_ok(cnt, stride);
    if (g == hipSuccess) g = guarded_ok(dlen, nb);
    if (g == hipSuccess) g = guarded_ok(dpos, nb);
    return g;
}

// P5 over buckets [b0, b1) of records of W + 1 words grouped by bucket.
//   recs       (W + 1) x stride words; starts: nb + 1 bounds (b1 <= nb)
//   dcnt / dlen / dpos  P5a's lists (all or none, W = 1): stride, nb, nb entries
//   lcap       LDS slots (0: skm_lds_slots(W)); grid 0: one workgroup per CU
//   rec_keys_out W x rec_cap, rec_cnts_out rec_cap, rec_dig_out rec_cap bytes,
//   cursor_out the final *rec.cursor; table_out table_cap x slot_words(W)
//   words (starts clear); spill_out W x spill_cap; stats_out ST_N counters
// Every record the launch walks must hold 1 <= n <= nmax keys, so that its
// bases fit the record and the walk finds a key in every record it enters.
int kcs_count_skm(int W, int k, const uint64_t* recs, uint64_t stride, const uint64_t* starts, uint32_t nb,
                  uint32_t b0, uint32_t b1, int count_keys, uint32_t lcap, int grid, const uint32_t* dcnt,
                  const uint32_t* dlen, const uint64_t* dpos, uint64_t rec_cap, uint64_t table_cap,
                  uint32_t probe_limit, uint64_t spill_cap, int fill, uint64_t* rec_keys_out, uint32_t* rec_cnts_out,
                  uint8_t* rec_dig_out, uint64_t* cursor_out, uint64_t* table_out, uint64_t* spill_out,
                  uint64_t* stats_out) {
    if (W < 1 || W > 3 || k <= 32 * (W - 1) || k > 32 * W || !recs || stride == 0 || stride > (1u << 26) ||
        !starts_ok(starts, nb, stride) || b0 >= b1 || b1 > nb || grid < 0 || grid > 4096 || !fill_ok(fill))
        return hipErrorInvalidValue;
    if (rec_cap == 0 || rec_cap > (1u << 26) || table_cap == 0 || table_cap > (1u << 24) || probe_limit == 0 ||
        probe_limit > (1u << 20) || spill_cap == 0 || spill_cap > (1u << 26) || !rec_keys_out || !rec_cnts_out ||
        !rec_dig_out || !cursor_out || !table_out || !spill_out || !stats_out)
        return hipErrorInvalidValue;
    const bool dd = dcnt != nullptr;
    if (dd != (dlen != nullptr) || dd != (dpos != nullptr) || (dd && W != 1)) return hipErrorInvalidValue;
    const kc::SkmGeom g = kc::skm_geometry(k, k);
    if (!g.ok) return hipErrorInvalidValue;
    const int RW = W + 1;
    for (uint32_t b = b0; b < b1; b++) {
        uint64_t lo = starts[b], hi = starts[b + 1];
        if (dd && dlen[b] != 0xffffffffu) {
            const uint64_t len = dlen[b] & 0x7fffffffu;
            lo = (dlen[b] & 0x80000000u) ? dpos[b] : starts[b];
            if (lo > stride || len > stride - lo) return hipErrorInvalidValue;
            hi = lo + len;
        }
        for (uint64_t i = lo; i < hi; i++) {
            const uint64_t n = recs[(size_t)(RW - 1) * stride + i] & 63u;
            if (n < 1 || n > (uint64_t)g.nmax) return hipErrorInvalidValue;
        }
    }
    if (grid == 0) grid = n_cu();
    if (grid < 1) return hipErrorInvalidValue;
    const size_t sw = (size_t)kc::slot_words(W);
    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* drecs = d.upload(recs, (size_t)RW * stride);
    uint64_t* dstarts = d.upload(starts, (size_t)nb + 1);
    uint32_t* ddcnt = dd ? d.upload(dcnt, stride) : nullptr;
    uint32_t* ddlen = dd ? d.upload(dlen, nb) : nullptr;
    uint64_t* ddpos = dd ? d.upload(dpos, nb) : nullptr;
    uint64_t* rkeys = alloc_guarded<uint64_t>(d, (size_t)W * rec_cap, fill);
    uint32_t* rcnts = alloc_guarded<uint32_t>(d, rec_cap, fill);
    uint8_t* rdig = alloc_guarded<uint8_t>(d, rec_cap, fill);
    uint64_t* cursor = d.alloc<uint64_t>(1, 0);
    uint64_t* table = alloc_guarded<uint64_t>(d, sw * table_cap, -1);
    uint64_t* spill = alloc_guarded<uint64_t>(d, (size_t)W * spill_cap, fill);
    uint64_t* stats = d.alloc<uint64_t>(kc::ST_N, 0);
    KCS(d.err);
    const kc::SkmDedup sdd = {ddcnt, ddlen, ddpos};
    KCS(kc::launch_count_skm(W, k, drecs, stride, dstarts, b0, b1, count_keys != 0, {rkeys, rcnts, rec_cap, cursor},
                             {table, table_cap, spill, spill_cap, stats, probe_limit}, lcap, grid, st.s,
                             dd ? &sdd : nullptr, rdig));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(rec_keys_out, rkeys, (size_t)W * rec_cap * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(rec_cnts_out, rcnts, rec_cap * 4, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(rec_dig_out, rdig, rec_cap, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(cursor_out, cursor, 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(table_out, table, sw * table_cap * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(spill_out, spill, (size_t)W * spill_cap * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(stats_out, stats, kc::ST_N * 8, hipMemcpyDeviceToHost));
    int gc = guarded_ok(rkeys, (size_t)W * rec_cap);
    if (gc == hipSuccess) gc = guarded_ok(rcnts, rec_cap);
    if (gc == hipSuccess) gc = guarded_ok(rdig, rec_cap);
    if (gc == hipSuccess) gc = guarded_ok(table, sw * table_cap);
    if (gc == hipSuccess) gc = guarded_ok(spill, (size_t)W * spill_cap);
    return gc;
}

// ---------------------------------------------------------------------------
// The key-prefix (partition) engine (tests/test_gpu_part_kernels.py): P5
// (count_buckets<W>) and P5s (sort_runs_k<W>, direct mode included; its gaps
// are closed by kcs_packed_seg_copy above, driven by the descriptors this
// returns). Keys are W x stride words SoA, grouped by bucket (starts) and,
// pre-split, by sub-bucket = key bits 40..47 (sub_starts). Outputs are
// pre-filled with `fill` behind 8 guard bytes; statistics, cursors and the
// fallback table start at 0.
// ---------------------------------------------------------------------------

int kcs_bucket_lds_slots(int W) { return w_ok(W) ? kc::bucket_lds_slots(W) : 0; }
int kcs_sort_runs_keys(int W) { return w_ok(W) ? kc::sort_runs_keys(W) : 0; }

namespace {

constexpr uint32_t kMaxTestBuckets = 4096;

// nb * 256 + 1 ascending sub-bucket bounds that agree with the bucket bounds,
// and every key stands in the sub-bucket its bits 40..47 name
bool sub_starts_ok(const uint64_t* sub, const uint64_t* starts, uint32_t nb, const uint64_t* w0) {
    for (uint32_t b = 0; b < nb; b++) {
        if (sub[(size_t)b * 256] != starts[b] || sub[(size_t)b * 256 + 256] != starts[b + 1]) return false;
        for (uint32_t d = 0; d < 256; d++) {
            const uint64_t lo = sub[(size_t)b * 256 + d], hi = sub[(size_t)b * 256 + d + 1];
            if (lo > hi || hi > starts[b + 1]) return false;
            for (uint64_t i = lo; i < hi; i++)
                if (((w0[i] >> 40) & 255u) != d) return false;
        }
    }
    return true;
}

// W = 1: the LDS table and the fallback table use key 0 as EMPTY
bool no_zero_key(int W, const uint64_t* keys, uint64_t lo, uint64_t hi) {
    if (W != 1) return true;
    for (uint64_t i = lo; i < hi; i++)
        if (keys[i] == 0) return false;
    return true;
}

}  // namespace

// launch_count_buckets over nb buckets.
//   keys       W x stride words; starts: nb + 1 bounds, starts[nb] <= stride
//   sub_starts optional nb * 256 + 1 bounds; run_flags (nb * 256), bucket_flags (nb): optional, pre-split only
//   lcap       as the API passes it (0 or above bucket_lds_slots(W): the maximum); grid 0: one workgroup per CU
//   rec_keys_out W x rec_cap, rec_cnts_out rec_cap, cursor_out the final *rec.cursor
//   desc_*_out desc_cap each; table_out table_cap x slot_words(W) words; spill_out W x spill_cap; stats_out ST_N
int kcs_count_buckets(int W, const uint64_t* keys, uint64_t stride, const uint64_t* starts, uint32_t nb,
                      const uint64_t* sub_starts, const uint8_t* run_flags, const uint8_t* bucket_flags,
                      uint32_t run_per, int distinct, uint32_t lcap, int grid, uint64_t rec_cap, uint64_t desc_cap,
                      uint64_t table_cap, uint32_t probe_limit, uint64_t spill_cap, int fill, uint64_t* rec_keys_out,
                      uint32_t* rec_cnts_out, uint64_t* cursor_out, uint64_t* desc_key_out, uint64_t* desc_start_out,
                      uint32_t* desc_len_out, uint64_t* table_out, uint64_t* spill_out, uint64_t* stats_out) {
    if (!w_ok(W) || !keys || stride == 0 || stride > (1u << 26) || nb > kMaxTestBuckets ||
        !starts_ok(starts, nb, stride) || grid < 0 || grid > 4096 || !fill_ok(fill))
        return hipErrorInvalidValue;
    if (rec_cap == 0 || rec_cap > (1u << 26) || desc_cap == 0 || desc_cap > (1u << 24) || table_cap == 0 ||
        table_cap > (1u << 24) || probe_limit == 0 || probe_limit > (1u << 20) || spill_cap == 0 ||
        spill_cap > (1u << 26) || run_per > (1u << 24))
        return hipErrorInvalidValue;
    if (!rec_keys_out || !rec_cnts_out || !cursor_out || !desc_key_out || !desc_start_out || !desc_len_out ||
        !table_out || !spill_out || !stats_out)
        return hipErrorInvalidValue;
    if (!sub_starts && (run_flags || bucket_flags || run_per)) return hipErrorInvalidValue;
    if ((run_flags != nullptr) != (bucket_flags != nullptr)) return hipErrorInvalidValue;
    if (sub_starts && !sub_starts_ok(sub_starts, starts, nb, keys)) return hipErrorInvalidValue;
    if (!no_zero_key(W, keys, starts[0], starts[nb])) return hipErrorInvalidValue;
    if (grid == 0) grid = n_cu();
    if (grid < 1) return hipErrorInvalidValue;
    const size_t sw = (size_t)kc::slot_words(W);
    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* dk = d.upload(keys, (size_t)W * stride);
    uint64_t* dstarts = d.upload(starts, (size_t)nb + 1);
    uint64_t* dsub = sub_starts ? d.upload(sub_starts, (size_t)nb * 256 + 1) : nullptr;
    uint8_t* drf = run_flags ? d.upload(run_flags, (size_t)nb * 256) : nullptr;
    uint8_t* dbf = bucket_flags ? d.upload(bucket_flags, (size_t)nb) : nullptr;
    uint64_t* rkeys = alloc_guarded<uint64_t>(d, (size_t)W * rec_cap, fill);
    uint32_t* rcnts = alloc_guarded<uint32_t>(d, rec_cap, fill);
    uint64_t* cursor = d.alloc<uint64_t>(1, 0);
    uint64_t* dky = alloc_guarded<uint64_t>(d, desc_cap, fill);
    uint64_t* dst = alloc_guarded<uint64_t>(d, desc_cap, fill);
    uint32_t* dln = alloc_guarded<uint32_t>(d, desc_cap, fill);
    uint64_t* table = alloc_guarded<uint64_t>(d, sw * table_cap, -1);
    uint64_t* spill = alloc_guarded<uint64_t>(d, (size_t)W * spill_cap, fill);
    uint64_t* stats = d.alloc<uint64_t>(kc::ST_N, 0);
    KCS(d.err);
    KCS(kc::launch_count_buckets(W, dk, stride, dstarts, nb, {rkeys, rcnts, rec_cap, cursor},
                                 {table, table_cap, spill, spill_cap, stats, probe_limit}, lcap, grid,
                                 {dky, dst, dln, desc_cap}, st.s, distinct != 0, dsub, drf, dbf, run_per));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(rec_keys_out, rkeys, (size_t)W * rec_cap * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(rec_cnts_out, rcnts, rec_cap * 4, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(cursor_out, cursor, 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(desc_key_out, dky, desc_cap * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(desc_start_out, dst, desc_cap * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(desc_len_out, dln, desc_cap * 4, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(table_out, table, sw * table_cap * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(spill_out, spill, (size_t)W * spill_cap * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(stats_out, stats, kc::ST_N * 8, hipMemcpyDeviceToHost));
    int gc = guarded_ok(rkeys, (size_t)W * rec_cap);
    if (gc == hipSuccess) gc = guarded_ok(rcnts, rec_cap);
    if (gc == hipSuccess) gc = guarded_ok(dky, desc_cap);
    if (gc == hipSuccess) gc = guarded_ok(dst, desc_cap);
    if (gc == hipSuccess) gc = guarded_ok(dln, desc_cap);
    if (gc == hipSuccess) gc = guarded_ok(table, sw * table_cap);
    if (gc == hipSuccess) gc = guarded_ok(spill, (size_t)W * spill_cap);
    return gc;
}

// launch_sort_runs over nb pre-split buckets (sub_starts: nb * 256 + 1 bounds
// over keys W x stride, sub_starts[nb * 256] <= stride).
//   grid 0: two workgroups per CU, as the API launches it
//   rec_keys_out W x rec_cap, rec_cnts_out rec_cap, cursor_out; desc_*_out desc_cap each
//   run_flags_out nb * 256, bucket_flags_out nb (both start clear), nflag_out, stats_out ST_N
//   packed != 0: direct mode. packed_out holds pk_base + sub_starts[nb * 256]
//   records of 8 W + 4 bytes as the kernel left them (pre-filled with `fill`;
//   desc_start then indexes it); rec_keys_out / rec_cnts_out keep `fill`.
//   The gaps that runs with equal keys leave are closed by kcs_packed_seg_copy
//   with packed_out as its source.
int kcs_sort_runs(int W, const uint64_t* keys, uint64_t stride, const uint64_t* sub_starts, uint32_t nb, int grid,
                  uint64_t rec_cap, uint64_t desc_cap, int fill, uint64_t* rec_keys_out, uint32_t* rec_cnts_out,
                  uint64_t* cursor_out, uint64_t* desc_key_out, uint64_t* desc_start_out, uint32_t* desc_len_out,
                  uint8_t* run_flags_out, uint8_t* bucket_flags_out, uint32_t* nflag_out, uint64_t* stats_out,
                  int packed, uint64_t pk_base, uint8_t* packed_out) {
    if (!w_ok(W) || !keys || stride == 0 || stride > (1u << 26) || nb < 1 || nb > kMaxTestBuckets || !sub_starts ||
        grid < 0 || grid > 4096 || !fill_ok(fill))
        return hipErrorInvalidValue;
    if (rec_cap == 0 || rec_cap > (1u << 26) || desc_cap == 0 || desc_cap > (1u << 24) || pk_base > (1u << 20))
        return hipErrorInvalidValue;
    if (!rec_keys_out || !rec_cnts_out || !cursor_out || !desc_key_out || !desc_start_out || !desc_len_out ||
        !run_flags_out || !bucket_flags_out || !nflag_out || !stats_out || (packed && !packed_out))
        return hipErrorInvalidValue;
    std::vector<uint64_t> starts((size_t)nb + 1);
    for (uint32_t b = 0; b <= nb; b++) starts[b] = sub_starts[(size_t)b * 256];
    if (!starts_ok(starts.data(), nb, stride) || !sub_starts_ok(sub_starts, starts.data(), nb, keys))
        return hipErrorInvalidValue;
    const uint64_t n = starts[nb];
    if (grid == 0) grid = 2 * n_cu();
    if (grid < 1) return hipErrorInvalidValue;
    const size_t rs = 8 * (size_t)W + 4;
    const size_t npk = packed ? (size_t)(pk_base + n) : 0;
    Stream st;
    KCS(st.err);
    Dev d;
    uint64_t* dk = d.upload(keys, (size_t)W * stride);
    uint64_t* dsub = d.upload(sub_starts, (size_t)nb * 256 + 1);
    uint64_t* rkeys = alloc_guarded<uint64_t>(d, (size_t)W * rec_cap, fill);
    uint32_t* rcnts = alloc_guarded<uint32_t>(d, rec_cap, fill);
    uint64_t* cursor = d.alloc<uint64_t>(1, 0);
    uint64_t* dky = alloc_guarded<uint64_t>(d, desc_cap, fill);
    uint64_t* dst = alloc_guarded<uint64_t>(d, desc_cap, fill);
    uint32_t* dln = alloc_guarded<uint32_t>(d, desc_cap, fill);
    uint8_t* drf = alloc_guarded<uint8_t>(d, (size_t)nb * 256, -1);
    uint8_t* dbf = alloc_guarded<uint8_t>(d, (size_t)nb, -1);
    uint32_t* nflag = d.alloc<uint32_t>(1, 0);
    uint64_t* stats = d.alloc<uint64_t>(kc::ST_N, 0);
    uint8_t* dpk = packed ? alloc_guarded<uint8_t>(d, npk * rs, fill) : nullptr;
    KCS(d.err);
    KCS(kc::launch_sort_runs(W, dk, stride, dsub, nb, {rkeys, rcnts, rec_cap, cursor}, stats,
                             {dky, dst, dln, desc_cap}, drf, dbf, nflag, grid, st.s, dpk, pk_base));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(rec_keys_out, rkeys, (size_t)W * rec_cap * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(rec_cnts_out, rcnts, rec_cap * 4, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(cursor_out, cursor, 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(desc_key_out, dky, desc_cap * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(desc_start_out, dst, desc_cap * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(desc_len_out, dln, desc_cap * 4, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(run_flags_out, drf, (size_t)nb * 256, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(bucket_flags_out, dbf, (size_t)nb, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(nflag_out, nflag, 4, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(stats_out, stats, kc::ST_N * 8, hipMemcpyDeviceToHost));
    if (packed) KCS(hipMemcpy(packed_out, dpk, npk * rs, hipMemcpyDeviceToHost));
    int gc = guarded_ok(rkeys, (size_t)W * rec_cap);
    if (gc == hipSuccess) gc = guarded_ok(rcnts, rec_cap);
    if (gc == hipSuccess) gc = guarded_ok(dky, desc_cap);
    if (gc == hipSuccess) gc = guarded_ok(dst, desc_cap);
    if (gc == hipSuccess) gc = guarded_ok(dln, desc_cap);
    if (gc == hipSuccess) gc = guarded_ok(drf, (size_t)nb * 256);
    if (gc == hipSuccess) gc = guarded_ok(dbf, (size_t)nb);
    if (gc == hipSuccess && packed) gc = guarded_ok(dpk, npk * rs);
    return gc;
}

// P1 / P2 (count_front with the histogram and the scatter sink) and the group
// histograms of the key-range passes.

// out[0..5): R, seg_tiles, nseg, max_win, scap of part_geometry(L, k, n_reads)
int kcs_part_geometry(int L, int k, uint64_t n_reads, uint64_t* out) {
    if (!out || k < 1 || k > 128 || L < k || L > 4096 || n_reads == 0 || n_reads > (1u << 22))
        return hipErrorInvalidValue;
    const kc::PartGeom pg = kc::part_geometry(L, k, n_reads);
    out[0] = (uint64_t)pg.geom.R;
    out[1] = (uint64_t)pg.seg_tiles;
    out[2] = pg.nseg;
    out[3] = (uint64_t)pg.max_win;
    out[4] = (uint64_t)pg.scap;
    return hipSuccess;
}

namespace {

// P2 writes the run of (digit d, segment s) from base[d * nseg + s] on; a
// segment holds at most its reads' windows, so a run that starts that far
// before the end of the output cannot leave it, whatever the kernel counts
bool bases_ok(const uint64_t* base, const kc::PartGeom& pg, uint64_t n_reads, int nw, uint64_t out_stride) {
    const uint64_t per_seg = (uint64_t)pg.seg_tiles * (uint64_t)pg.geom.R;
    for (uint64_t sg = 0; sg < pg.nseg; sg++) {
        const uint64_t r0 = sg * per_seg;
        const uint64_t nr = n_reads - r0 < per_seg ? n_reads - r0 : per_seg;
        const uint64_t win = nr * (uint64_t)nw;
        for (uint32_t d = 0; d < 256; d++) {
            const uint64_t b = base[(uint64_t)d * pg.nseg + sg];
            if (b > out_stride || win > out_stride - b) return false;
        }
    }
    return true;
}

}  // namespace

// E (launch_encode_reads) over n_reads reads of L bytes at text + r L, then P1
// (run_p1) and / or P2 (run_p2) with the library's geometry.
//   shift, gbits, flo, fhi, no_stats  as launch_part_hist / launch_part_scatter take them
//   hist_out   P1: gbits 0: 256 x nseg u64 (hist[d * nseg + seg]); else nseg x (256 << gbits) u32
//   base       P2: 256 x nseg run starts, every run inside out_stride (checked
//              against the segment's windows); out: W x out_stride words (SoA,
//              or out_stride items of W words when aos), digs_out out_stride bytes (want_digs)
//   base2      optional second range [fmid, fhi): out2 W x out2_stride, digs2_out
//   stats_out  ST_N counters after both kernels
int kcs_part_front(const uint8_t* text, uint64_t n_reads, int L, int k, int shift, int gbits, uint32_t flo,
                   uint32_t fhi, int no_stats, int run_p1, void* hist_out, int run_p2, const uint64_t* base,
                   uint64_t out_stride, int aos, int want_digs, uint32_t fmid, const uint64_t* base2,
                   uint64_t out2_stride, int fill, uint64_t* out, uint8_t* digs_out, uint64_t* out2,
                   uint8_t* digs2_out, uint64_t* stats_out) {
    if (!text || k < 1 || k > 128 || L < k || L > 4096 || n_reads == 0 || n_reads > (1u << 22) || shift < 0 ||
        shift > 56 || gbits < 0 || gbits > 4 || flo >= fhi || fhi > 256 || !fill_ok(fill) || !stats_out ||
        (!run_p1 && !run_p2))
        return hipErrorInvalidValue;
    if (run_p1 && !hist_out) return hipErrorInvalidValue;
    const int W = (k + 31) / 32, nw = L - k + 1;
    const kc::PartGeom pg = kc::part_geometry(L, k, n_reads);
    if (run_p2) {
        if (!base || !out || out_stride == 0 || out_stride > (1u << 26) || (want_digs && !digs_out))
            return hipErrorInvalidValue;
        if (!bases_ok(base, pg, n_reads, nw, out_stride)) return hipErrorInvalidValue;
        if (base2) {
            if (!out2 || out2_stride == 0 || out2_stride > (1u << 26) || (want_digs && !digs2_out) || fmid <= flo ||
                fmid >= fhi || !bases_ok(base2, pg, n_reads, nw, out2_stride))
                return hipErrorInvalidValue;
        }
    } else if (base2) {
        return hipErrorInvalidValue;
    }
    const uint64_t ng = n_reads * (uint64_t)kc::groups_per_read(L);
    const size_t hbytes = gbits == 0 ? (size_t)256 * pg.nseg * 8 : ((size_t)256 << gbits) * pg.nseg * 4;
    Stream st;
    KCS(st.err);
    Dev d;
    uint8_t* dtext = d.alloc<uint8_t>(n_reads * (uint64_t)L + 16, 0);
    uint32_t* codes = d.alloc<uint32_t>(ng + 4, 0);
    uint16_t* inval = d.alloc<uint16_t>(ng + 8, 0);
    uint8_t* hist = run_p1 ? alloc_guarded<uint8_t>(d, hbytes, fill) : nullptr;
    uint64_t* dbase = run_p2 ? d.upload(base, (size_t)256 * pg.nseg) : nullptr;
    uint64_t* dout = run_p2 ? alloc_guarded<uint64_t>(d, (size_t)W * out_stride, fill) : nullptr;
    uint8_t* ddig = run_p2 && want_digs ? alloc_guarded<uint8_t>(d, out_stride, fill) : nullptr;
    uint64_t* dbase2 = base2 ? d.upload(base2, (size_t)256 * pg.nseg) : nullptr;
    uint64_t* dout2 = base2 ? alloc_guarded<uint64_t>(d, (size_t)W * out2_stride, fill) : nullptr;
    uint8_t* ddig2 = base2 && want_digs ? alloc_guarded<uint8_t>(d, out2_stride, fill) : nullptr;
    uint64_t* stats = d.alloc<uint64_t>(kc::ST_N, 0);
    KCS(d.err);
    KCS(hipMemcpy(dtext, text, n_reads * (uint64_t)L, hipMemcpyHostToDevice));
    kc::CountLaunch l{};
    l.base = dtext;
    l.seq_off = nullptr;
    l.read0 = 0;
    l.n_reads = n_reads;
    l.L = L;
    l.k = k;
    l.stats = stats;
    l.codes = codes;
    l.inval = inval;
    l.flo = flo;
    l.fhi = fhi;
    l.no_stats = no_stats != 0;
    KCS(kc::launch_encode_reads(l, codes, inval, st.s));
    if (run_p1) KCS(kc::launch_part_hist(l, pg, (uint64_t*)hist, shift, st.s, gbits));
    if (run_p2)
        KCS(kc::launch_part_scatter(l, pg, dbase, dout, out_stride, shift, ddig, st.s, dbase2, dout2, out2_stride,
                                    ddig2, base2 ? fmid : 256u, aos != 0));
    KCS(hipStreamSynchronize(st.s));
    if (run_p1) KCS(hipMemcpy(hist_out, hist, hbytes, hipMemcpyDeviceToHost));
    if (run_p2) KCS(hipMemcpy(out, dout, (size_t)W * out_stride * 8, hipMemcpyDeviceToHost));
    if (ddig) KCS(hipMemcpy(digs_out, ddig, out_stride, hipMemcpyDeviceToHost));
    if (dout2) KCS(hipMemcpy(out2, dout2, (size_t)W * out2_stride * 8, hipMemcpyDeviceToHost));
    if (ddig2) KCS(hipMemcpy(digs2_out, ddig2, out2_stride, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(stats_out, stats, kc::ST_N * 8, hipMemcpyDeviceToHost));
    int gc = hipSuccess;
    if (hist) gc = guarded_ok(hist, hbytes);
    if (gc == hipSuccess && dout) gc = guarded_ok(dout, (size_t)W * out_stride);
    if (gc == hipSuccess && ddig) gc = guarded_ok(ddig, out_stride);
    if (gc == hipSuccess && dout2) gc = guarded_ok(dout2, (size_t)W * out2_stride);
    if (gc == hipSuccess && ddig2) gc = guarded_ok(ddig2, out2_stride);
    return gc;
}

// launch_hist_group_sum over groups [g0, g1) and launch_hist_group_totals of
// a gbits = 4 histogram h (nseg x 4096 u32: group g, digit d of segment s at
// s * 4096 + g * 256 + d). sum_out: 256 x nseg u64 (out[d * nseg + s]); tot_out: 16.
int kcs_hist_group(const uint32_t* h, uint64_t nseg, uint32_t g0, uint32_t g1, int fill, uint64_t* sum_out,
                   uint64_t* tot_out) {
    if (!h || nseg == 0 || nseg > 4096 || g0 >= g1 || g1 > 16 || !fill_ok(fill) || !sum_out || !tot_out)
        return hipErrorInvalidValue;
    Stream st;
    KCS(st.err);
    Dev d;
    uint32_t* dh = d.upload(h, (size_t)nseg * 4096);
    uint64_t* dsum = alloc_guarded<uint64_t>(d, (size_t)256 * nseg, fill);
    uint64_t* dtot = alloc_guarded<uint64_t>(d, 16, fill);
    KCS(d.err);
    KCS(kc::launch_hist_group_sum((const uint64_t*)dh, nseg, g0, g1, dsum, st.s));
    KCS(kc::launch_hist_group_totals((const uint64_t*)dh, nseg, 16, dtot, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(sum_out, dsum, (size_t)256 * nseg * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(tot_out, dtot, 16 * 8, hipMemcpyDeviceToHost));
    int gc = guarded_ok(dsum, (size_t)256 * nseg);
    if (gc == hipSuccess) gc = guarded_ok(dtot, 16);
    return gc;
}

// ---------------------------------------------------------------------------
// The canonical fold's two passes (tests/test_gpu_canon_kernels.py) over n
// packed records of W words holding k bases. Tiles of kcs_filter_tile()
// records. Only whole packed records reach the kernels, and the split gets the
// tile bases from the library's own count and scan, so a staying record lands
// below n in stay_out and a flipped one below n in the SoA arrays: both are
// sized n behind a guard.
// ---------------------------------------------------------------------------

uint64_t kcs_filter_tile(void) { return kc::filter_tile(); }

static bool canon_ok(int W, int k, uint64_t n, const void* packed) {
    return w_ok(W) && k >= 1 && (k + 31) / 32 == W && (n == 0 || packed);
}

// tile_cnt: ceil(n / tile) staying-record counts out.
int kcs_canon_count(int W, int k, uint64_t n, const uint8_t* packed, uint64_t* tile_cnt) {
    if (!canon_ok(W, k, n, packed) || (n && !tile_cnt)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const size_t rs = 8 * (size_t)W + 4;
    const uint64_t nt = (n + kc::filter_tile() - 1) / kc::filter_tile();
    Stream st;
    KCS(st.err);
    Dev d;
    uint8_t* dp = d.upload(packed, n * rs);
    uint64_t* dc = alloc_guarded<uint64_t>(d, nt, 0xff);
    KCS(d.err);
    KCS(kc::launch_canon_count(dp, W, k, n, dc, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(tile_cnt, dc, nt * 8, hipMemcpyDeviceToHost));
    return guarded_ok(dc, nt);
}

// count -> scan -> split. tile_cnt, stay_base: ceil(n / tile) each out;
// stay_out: n packed records, flip_keys: W x n words, flip_cnts: n, all
// pre-filled with the byte `fill` and returned whole; *n_stay out.
int kcs_canon_split(int W, int k, uint64_t n, const uint8_t* packed, uint64_t* tile_cnt, uint64_t* stay_base,
                    uint64_t* n_stay, uint8_t* stay_out, uint64_t* flip_keys, uint32_t* flip_cnts, int fill) {
    if (!canon_ok(W, k, n, packed) || !n_stay || !fill_ok(fill)) return hipErrorInvalidValue;
    if (n && (!tile_cnt || !stay_base || !stay_out || !flip_keys || !flip_cnts)) return hipErrorInvalidValue;
    *n_stay = 0;
    if (n == 0) return hipSuccess;
    const size_t rs = 8 * (size_t)W + 4;
    const uint64_t nt = (n + kc::filter_tile() - 1) / kc::filter_tile();
    Stream st;
    KCS(st.err);
    Dev d;
    uint8_t* dp = d.upload(packed, n * rs);
    uint64_t* dc = alloc_guarded<uint64_t>(d, nt, 0xff);
    uint64_t* db = alloc_guarded<uint64_t>(d, nt, 0xff);
    uint64_t* dtot = d.alloc<uint64_t>(1, 0);
    const uint64_t te = kc::scan_tmp_elems(nt);
    uint64_t* tmp = d.alloc<uint64_t>(te + 1, kGuard);
    uint8_t* ds = alloc_guarded<uint8_t>(d, n * rs, fill);
    uint64_t* dfk = alloc_guarded<uint64_t>(d, (size_t)W * n, fill);
    uint32_t* dfc = alloc_guarded<uint32_t>(d, n, fill);
    KCS(d.err);
    KCS(kc::launch_canon_count(dp, W, k, n, dc, st.s));
    KCS(kc::launch_scan_u64(dc, db, nt, tmp, st.s));
    KCS(kc::launch_sum_last(db, dc, nt, dtot, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(n_stay, dtot, 8, hipMemcpyDeviceToHost));
    if (*n_stay > n) return hipErrorInvalidValue;  // nothing is split with a total that cannot be
    KCS(kc::launch_canon_split(dp, W, k, n, db, ds, dfk, n, dfc, st.s));
    KCS(hipStreamSynchronize(st.s));
    KCS(hipMemcpy(tile_cnt, dc, nt * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(stay_base, db, nt * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(stay_out, ds, n * rs, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(flip_keys, dfk, (size_t)W * n * 8, hipMemcpyDeviceToHost));
    KCS(hipMemcpy(flip_cnts, dfc, n * 4, hipMemcpyDeviceToHost));
    int gc = guard_check(tmp + te, 8);
    if (gc == hipSuccess) gc = guarded_ok(dc, nt);
    if (gc == hipSuccess) gc = guarded_ok(db, nt);
    if (gc == hipSuccess) gc = guarded_ok(ds, n * rs);
    if (gc == hipSuccess) gc = guarded_ok(dfk, (size_t)W * n);
    if (gc == hipSuccess) gc = guarded_ok(dfc, n);
    return gc;
}

}  // extern "C"
