// kc_common.inl — what every other device module builds on. Included first by
// kc_kernels.hip inside namespace kc; it takes nothing from another module.
//
// Holds: the u64 / u32 / vector typedefs, load_key, kBlock / kWave, the wave
// helpers (lane_id, lanemask_lt, uni32 / uni64, le64_32, wave_reserve,
// wave_add), FastDivU, mix64 / hash_key, block_excl_scan, and the host helpers
// of the launch wrappers: hmin, dispatch_w (runtime key width -> template
// argument) and grid_for (element-wise grid, capped at elem_grid_cap()).
// Host callers: only elem_grid_cap() is declared in kc_device.h (the kernel
// tests size their inputs past it).

typedef uint64_t u64;
typedef unsigned int u32;
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef unsigned long long v2u64 __attribute__((ext_vector_type(2)));
// a volatile 16-byte LDS load (ds_read_b128): the cast pins the LDS address
// space, which a generic volatile pointer loses (it would become a FLAT load)
typedef __attribute__((address_space(3))) volatile v2u64 lds_v2u64;

// key i of a key array into k: W word arrays at `stride`, or (stride 0) W
// consecutive words per key (AoS; one 16-byte load at W = 2)
template <int W>
__device__ __forceinline__ void load_key(const u64* __restrict__ keys, u64 stride, u64 i, u64 (&k)[W]) {
    if (stride == 0) {
        if constexpr (W == 2) {
            const v2u64 v = *(const v2u64*)(keys + 2 * i);
            k[0] = v.x;
            k[1] = v.y;
        } else {
#pragma unroll
            for (int j = 0; j < W; j++) k[j] = keys[i * W + j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < W; j++) k[j] = keys[(u64)j * stride + i];
    }
}

constexpr int kBlock = 256;  // 4 waves of 64
constexpr int kWave = 64;

static inline u64 hmin(u64 a, u64 b) { return a < b ? a : b; }

// ---------------------------------------------------------------------------
// wave helpers (wave64)
// ---------------------------------------------------------------------------

__device__ __forceinline__ u32 lane_id() { return __lane_id(); }

__device__ __forceinline__ u64 lanemask_lt() { return (1ull << lane_id()) - 1ull; }

// Block-uniform values read from LDS, made scalar so the branches (and the
// barriers under them) are uniform to the compiler as well.
__device__ __forceinline__ u32 uni32(u32 v) { return __builtin_amdgcn_readfirstlane(v); }
// v <= lim for a 64-bit uniform v as two 32-bit compares: hipcc (ROCm 7.2)
// lowers a uniform 64-bit unsigned compare to a VALU compare in VCC and can
// then select on SCC (a stale carry) — seen in sort_runs_k's run length
__device__ __forceinline__ bool le64_32(u64 v, u32 lim) { return (u32)(v >> 32) == 0u && (u32)v <= lim; }
__device__ __forceinline__ u64 uni64(u64 v) {
    return ((u64)(u32)__builtin_amdgcn_readfirstlane((u32)(v >> 32)) << 32) |
           (u64)(u32)__builtin_amdgcn_readfirstlane((u32)v);
}


// Wave-aggregated atomicAdd of `mine` (per lane) to *ctr; returns this lane's
// exclusive position (ctr_old + prefix of lower active lanes).
__device__ __forceinline__ u64 wave_reserve(u64* ctr, bool want) {
    u64 m = __ballot(want);
    u64 base = 0;
    if (m) {
        int leader = __ffsll((long long)m) - 1;
        if ((int)lane_id() == leader) base = atomicAdd((unsigned long long*)ctr, (unsigned long long)__popcll(m));
        base = __shfl(base, leader);
    }
    return base + (u64)__popcll(m & lanemask_lt());
}

__device__ __forceinline__ void wave_add(u64* ctr, u64 v) {
    // reduce v over the active lanes, one atomic per wave
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    u64 act = __ballot(1);
    if ((int)lane_id() == __ffsll((long long)act) - 1 && v) atomicAdd((unsigned long long*)ctr, v);
}

// n / d for n, d < 2^16 with one mul_hi (m = ceil(2^32 / d) is exact there)
struct FastDivU {
    u32 d, m;
    __device__ __forceinline__ explicit FastDivU(u32 dd) : d(dd), m((u32)((0x100000000ull + dd - 1) / dd)) {}
    __device__ __forceinline__ u32 div(u32 v) const { return d == 1 ? v : __umulhi(v, m); }
};

__device__ __forceinline__ u64 mix64(u64 x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

template <int W>
__device__ __forceinline__ u64 hash_key(const u64 (&key)[W]) {
    u64 h = mix64(key[0] ^ 0x9e3779b97f4a7c15ull);
#pragma unroll
    for (int j = 1; j < W; j++) h = mix64(h ^ key[j]);
    return h;
}

// Block-wide exclusive scan of one u32 per thread (256 threads). `lds` holds
// >= 4 u32. Returns the exclusive prefix; *total receives the block sum.
__device__ __forceinline__ u32 block_excl_scan(u32 v, u32* lds, u32* total) {
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    u32 x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        u32 y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    u32 w0 = lds[0], w1 = lds[1], w2 = lds[2], w3 = lds[3];
    u32 before = (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0);
    *total = w0 + w1 + w2 + w3;
    __syncthreads();
    return before + x - v;
}

// Host-side dispatch of a runtime key width to a template argument: calls
// f(std::integral_constant<int, W>()) for W in [1, MAX] (a generic lambda that
// launches kernel<decltype(w)::value>), hipErrorInvalidValue outside. MAX is
// the widest instantiation the caller's kernel has (4, or 3 in the skm engine).
template <int MAX, class F>
static hipError_t dispatch_w(int W, F&& f) {
    static_assert(MAX == 3 || MAX == 4, "the kernels are instantiated for W = 1..3 or 1..4");
    switch (W) {
    case 1: f(std::integral_constant<int, 1>()); return hipSuccess;
    case 2: f(std::integral_constant<int, 2>()); return hipSuccess;
    case 3: f(std::integral_constant<int, 3>()); return hipSuccess;
    case 4:
        if constexpr (MAX == 4) {
            f(std::integral_constant<int, 4>());
            return hipSuccess;
        }
        return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
    }
}

constexpr int kElemGridCap = 8192;  // element-wise kernels walk past it with a grid stride

static int grid_for(u64 n, int cap = kElemGridCap) {
    u64 g = (n + kBlock - 1) / kBlock;
    if (g > (u64)cap) g = cap;
    return (int)(g ? g : 1);
}
int elem_grid_cap() { return kElemGridCap; }
