// Shared by the conv-stack kernels of libpam_hip.so (and the bf16 converters of the image / detector kernels): vector types, bf16
// helpers, the MFMA / LDS-read interleave, the XCD-contiguous work order, the LDS-DMA ring's wait and the launch helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <mutex>
#include <unordered_map>
#include <utility>

typedef __attribute__((ext_vector_type(8))) short bf16x8;     // 8 bf16 = one MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(2))) short s16x2;
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_void;

constexpr unsigned OOB_OFFSET = 0x80000000u;     // beyond any buffer's num_records: the hardware bounds check returns zeros

__device__ __forceinline__ float bf16_to_f32(uint16_t v) { return __builtin_bit_cast(float, ((uint32_t)v) << 16); }
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {        // round-to-nearest-even (v_cvt_pk_bf16_f32 on gfx950)
    return __builtin_bit_cast(uint16_t, (__bf16)f);
}
__device__ __forceinline__ float bf16_lo(uint32_t d) { return __builtin_bit_cast(float, d << 16); }           // low bf16 of a pair
__device__ __forceinline__ float bf16_hi(uint32_t d) { return __builtin_bit_cast(float, d & 0xffff0000u); }   // high bf16 of a pair
// two floats -> one dword of two bf16: one v_cvt_pk_bf16_f32 (RNE).  The element-wise cast form compiles to two converts + a permute;
// an asm statement is one instruction too, but the compiler does not pad it against the MFMA that wrote lo / hi (k_stem_fused met that)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){lo, hi}, bf16x2_t));
}
__device__ __forceinline__ uint32_t relu_bf16x2(uint32_t v) {     // bf16 is sign-magnitude: max(int16, 0) clears the negatives
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, v), (s16x2){0, 0}));
}

// The fuse-layer sum of 8 channels, the one statement of what "bit-identical" means for k_upsample_add, k_fuse_sum and k_fuse_sum_lds:
// eight fp32 sums start from the base, every term is added in the caller's order (plain terms, then up terms in ascending shift), then
// the optional ReLU and ONE bf16 rounding.  Which loads are in flight before which add stays each kernel's own business.  k_upsample_add
// and k_fuse_sum call these; k_fuse_sum_lds spells the same three steps out (with the calls it needs 34 more VGPRs).
// sum8_finish writes through a reference: returned by value, all 33 k_fuse_sum instantiations allocate their registers otherwise.
__device__ __forceinline__ void sum8_start(float (&v)[8], bf16x8 base) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = bf16_to_f32((uint16_t)base[e]);
}
__device__ __forceinline__ void sum8_add(float (&v)[8], bf16x8 term) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += bf16_to_f32((uint16_t)term[e]);
}
__device__ __forceinline__ void sum8_finish(const float (&v)[8], int relu, bf16x8& o) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (short)f32_to_bf16(relu ? fmaxf(v[e], 0.0f) : v[e]);
}

__device__ __forceinline__ int fdiv_small(int x, float inv) { return (int)(((float)x + 0.5f) * inv); }   // exact for x < 2^16

// Work item of workgroup v among n items.  Workgroups v, v + 8, ... share an XCD and its L2, so every XCD gets a contiguous run of
// items (neighbouring tiles re-read each other's halo, the slabs of one pixel block the same pixels: those reads then hit one L2).
__device__ __forceinline__ int xcd_order(int v, int n) {
    const int q = n >> 3, r = n & 7, xcd = v & 7, loc = v >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

// Issue order of one k-step: the next step's NR LDS fragment reads alternate with the first NR of this step's NM MFMAs, the other
// MFMAs follow (slack for the last read's latency); the builtin takes literal counts.  Callers that must not pass NM < NR guard the
// call; k_conv_gs with one M tile per wave passes it, and its tail count stays as it is.
template <int NM, int NR, int... R>
__device__ __forceinline__ void spread(std::integer_sequence<int, R...>) {
    (((void)R, __builtin_amdgcn_sched_group_barrier(0x008, 1, 0), __builtin_amdgcn_sched_group_barrier(0x100, 1, 0)), ...);
    __builtin_amdgcn_sched_group_barrier(0x008, NM - NR, 0);
}
template <int NM, int NR>
__device__ __forceinline__ void spread() { spread<NM, NR>(std::make_integer_sequence<int, NR>{}); }

// Loader wave of an LDS-DMA ring of NBUF chunk buffers (NPER DMA pieces per wave and chunk): wait until every chunk but the `fly`
// youngest (fly <= NBUF - 2) has landed.  The counts of fly 3 and 4 are 0 in rings too short to reach them (vmcnt's range is 0-63).
template <int NPER, int NBUF>
__device__ __forceinline__ void dma_ring_wait(int fly) {
    if (fly <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (fly == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPER) : "memory");
    else if (fly == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NPER) : "memory");
    else if (fly == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NBUF >= 5 ? 3 * NPER : 0) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NBUF >= 6 ? 4 * NPER : 0) : "memory");
}

// One lane's row piece of 4*NTW contiguous bf16 channels (8*NTW bytes, 8-byte aligned; 16-byte aligned when NTW is even or the lane
// group g is even) as 16-byte stores where possible.  NTW = 3 (24 bytes) splits 16 + 8 for even g and 8 + 16 for odd g, so the
// 16-byte half is always aligned.
template <int NTW>
__device__ __forceinline__ void row_store(uint16_t* p, int g, const uint32_t* d) {
    if constexpr (NTW == 1) {
        *(u32x2*)p = (u32x2){d[0], d[1]};
    } else if constexpr (NTW == 2) {
        *(u32x4*)p = (u32x4){d[0], d[1], d[2], d[3]};
    } else if constexpr (NTW == 4) {
        *(u32x4*)p = (u32x4){d[0], d[1], d[2], d[3]}; *(u32x4*)(p + 8) = (u32x4){d[4], d[5], d[6], d[7]};
    } else if constexpr (NTW == 6) {
#pragma unroll
        for (int k = 0; k < 3; ++k) *(u32x4*)(p + 8 * k) = (u32x4){d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]};
    } else {
        static_assert(NTW == 3, "slab width");
        const bool odd = g & 1;
        *(u32x4*)(p + (odd ? 4 : 0)) = odd ? (u32x4){d[2], d[3], d[4], d[5]} : (u32x4){d[0], d[1], d[2], d[3]};
        *(u32x2*)(p + (odd ? 0 : 8)) = odd ? (u32x2){d[0], d[1]} : (u32x2){d[4], d[5]};
    }
}

// Every kernel of the conv stack takes ONE argument struct, so a launch is (function, grid, block, LDS bytes, struct).
template <typename A>
static inline void pam_launch(void (*kernel)(A), dim3 grid, dim3 block, size_t lds, hipStream_t s, const A& a) {
    hipLaunchKernelGGL(kernel, grid, block, lds, s, a);
}

// Compute units of the current device, for the kernels whose grid is one persistent workgroup per CU.  The answer is kept per thread and
// asked again when the thread's current device changes; 256 (an MI355X) where HIP cannot name the device.
static inline int pam_cu_count() {
    static thread_local int cached_dev = -1, cached_cu = 256;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev != cached_dev) {
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) { cached_cu = pr.multiProcessorCount; cached_dev = dev; }
    }
    return cached_cu;
}

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to a DEVICE's copy of a function: set it once per (function, device) -- a process that
// drives a second GPU would otherwise launch with > 64 KB of LDS without the attribute and fail.  Returns false on a HIP error.
static inline bool pam_max_dynamic_lds(const void* func, int bytes) {
    static std::mutex mu;
    static std::unordered_map<const void*, unsigned long long> done;      // function -> bit per device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> g(mu);
    unsigned long long& m = done[func];
    if (dev < 64 && ((m >> dev) & 1)) return true;
    if (hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    if (dev < 64) m |= 1ull << dev;
    return true;
}
