// kc_kernel_shim: the launch wrappers of the radix grouping passes (rp_*) and
// of the segment sort behind a C ABI, for tests/test_gpu_kernels.py. Every
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
//   grid     as kc_api.cpp passes it (0: 2 x CUs); the scatter runs min(tiles, grid / 2) workgroups
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
    uint64_t* tmp = d.alloc<uint64_t>(regional ? (256 * nt + 1) / 2 : kc::p3_tmp_elems(nt));
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

}  // extern "C"
