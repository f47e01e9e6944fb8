// Shared helpers for the gfx950 kernels of liboryon_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>
#include "../../include/oryon_hip.h"

namespace oryon {

void set_error(const char *fmt, ...);
// measurement hook (oryon_profile_events): HIP events recorded around the dominant kernel launch of the next matcher call
// kernel_name (a string literal): what oryon_dominant_kernel() reports for the launch the events bracket
void profile_begin(hipStream_t st, const char *kernel_name = nullptr);
void profile_end(hipStream_t st);

#define ORYON_CHECK_ARG(cond)                                                           \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            oryon::set_error("%s: invalid argument: %s", __func__, #cond);              \
            return ORYON_ERR_INVALID_ARG;                                               \
        }                                                                               \
    } while (0)

// the one refusal of a missing or short caller-provided workspace: prefix (a literal; its own format arguments follow `need`) + the common text
#define ORYON_CHECK_WORKSPACE(prefix, ptr, given, need, ...)                            \
    do {                                                                                \
        const size_t given_ = (given), need_ = (need);                                  \
        if (!(ptr) || given_ < need_) {                                                 \
            oryon::set_error(prefix "workspace too small (%zu < %zu)", ##__VA_ARGS__, given_, need_); \
            return ORYON_ERR_WORKSPACE;                                                 \
        }                                                                               \
    } while (0)

#define ORYON_CHECK_LAUNCH()                                                            \
    do {                                                                                \
        hipError_t e_ = hipGetLastError();                                              \
        if (e_ != hipSuccess) {                                                         \
            oryon::set_error("%s: launch failed: %s", __func__, hipGetErrorString(e_)); \
            return ORYON_ERR_HIP;                                                       \
        }                                                                               \
    } while (0)

#define ORYON_CHECK_HIP(expr)                                                           \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            oryon::set_error("%s: %s failed: %s", __func__, #expr, hipGetErrorString(e_)); \
            return ORYON_ERR_HIP;                                                       \
        }                                                                               \
    } while (0)

// Development switches.  The SHIPPED library (make all) reads no environment variable: dev_env_* return their defaults.  The dev build
// (make dev -> liboryon_hip_dev.so, -DORYON_DEV; what the A/B scripts under tools/ load) reads them.
// A switch exists only while a test, a tool without a round number in its name, or README / DESIGN / INTEGRATION.md sets or documents it
// (tests/test_dev_switches.py holds the list); one that nothing uses any more goes, together with the code only it reached.
#ifdef ORYON_DEV
static inline int dev_env_int(const char *name, int dflt) { const char *s = getenv(name); return s ? atoi(s) : dflt; }
static inline bool dev_env_set(const char *name) { return getenv(name) != nullptr; }
#else
static inline int dev_env_int(const char *, int dflt) { return dflt; }
static inline bool dev_env_set(const char *) { return false; }
#endif

// Range flag of the fp16x3 kernels (round 5).  An fp32 operand of magnitude >= 65520 splits into hi = +-inf (lo = -+inf or NaN) and every
// product it enters comes out inf or NaN, so a kernel that looks at the magnitude bits of its raw ACCUMULATORS (pre-activation) sees an
// overflow of any of its inputs - and one that merely produced a value outside float16's range flags it before the next kernel splits
// it.  The flag is one word per (device, stream), set with atomicOr, reset at the start and read at the end of a forward on that stream
// by oryon_x3_range_flag.
constexpr unsigned X3_RANGE_LIMIT_BITS = 0x476a6000u;            // 60000.0f: below float16's 65504 with room for the rounding of hi
unsigned *x3_range_flag(hipStream_t st);                         // the flag word of (current device, stream) (util.hip); nullptr = no memory, error set
__device__ __forceinline__ unsigned x3_mag(float v) { return __float_as_uint(v) & 0x7fffffffu; }     // NaN / inf compare above any finite value
__device__ __forceinline__ void x3_raise(unsigned *flag, unsigned mag_max)
{
    if (mag_max >= X3_RANGE_LIMIT_BITS) atomicOr(flag, 1u);
}

static inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }
static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
// workspace carving: every block starts on a 256-byte boundary; float64 / int64 arguments must be 8-byte aligned (NULL is)
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// ------------------------------------------------------------------------------------------------ caller-provided workspaces
// One allocation, 256-byte aligned buffers, one line per buffer: carve(w.ws_max, B * S * cap_a) assigns the pointer (typed by it) and
// advances to the next multiple of 256; a buffer of zero elements gets the next buffer's address and leaves the offset where it is.
// The carve_* functions are walked twice with the same code: on a null base every pointer comes out null and only the size (off, or
// end where the site does not pad its last buffer) is of interest.  A nested workspace starts its Carver at the inner one's size.
struct Carver {
    char *base;
    size_t off, end;                    // start of the next buffer; unpadded end of the last one
    explicit Carver(void *b, size_t start = 0) : base(static_cast<char *>(b)), off(start), end(start) {}
    template <class T> void operator()(T *&p, size_t count)             // count elements (bytes for a void pointer)
    {
        p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        end = off + count * sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
        off = align256(end);
    }
};

// 64-bit mix (splitmix64 finaliser): the counter-based RNG of the batched sampling kernels.
__host__ __device__ static inline uint64_t mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__host__ __device__ static inline uint32_t rng_u32(uint64_t seed, uint64_t key, uint32_t stream, uint32_t i)
{
    return (uint32_t)(mix64(mix64(seed ^ (key * 0xD1B54A32D192ED03ull)) + ((uint64_t)stream << 32 | i)) >> 32);
}

// The bin walk of a radix select over a 256-bin histogram, by ONE complete wave (all 64 lanes call it, after the barrier that closes the
// histogram): the first bin b with hist[0] + .. + hist[b] >= remaining, and `below` = hist[0] + .. + hist[b - 1].  What the serial walk
//     for (b = 0; b < 256; ++b) { if (cum + hist[b] >= remaining) break; cum += hist[b]; }
// leaves in (b, cum) for every histogram - b = 256 and the whole sum where no bin gets there.  Four bins per lane, a wave prefix sum of
// the lanes' totals, a ballot for the first lane whose inclusive sum reaches `remaining`, and that lane's four bins walked in order.
// Every lane returns the same pair.  hist must be 16-byte aligned.
#ifdef __HIPCC__
__device__ __forceinline__ int radix_pick(const unsigned *hist, unsigned remaining, unsigned &below)
{
    const int lane = threadIdx.x & 63;
    const uint4 h = *reinterpret_cast<const uint4 *>(hist + lane * 4);
    const unsigned tot = h.x + h.y + h.z + h.w;
    unsigned incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o);
        incl += (lane >= o) ? v : 0u;
    }
    const unsigned long long reach = __ballot(incl >= remaining);
    if (reach == 0ull) {                                   // no bin gets there: the walk runs off the end with the whole sum
        below = __shfl(incl, 63);
        return 256;
    }
    const int src = __ffsll(reach) - 1;
    unsigned cum = incl - tot;
    int j = 3;
    if (cum + h.x >= remaining) j = 0;
    else if ((cum += h.x) + h.y >= remaining) j = 1;
    else if ((cum += h.y) + h.z >= remaining) j = 2;
    else cum += h.z;                                       // lane `src` reaches it in its last bin at the latest
    below = __shfl(cum, src);
    return src * 4 + __shfl(j, src);
}
#endif

// Raise a kernel's dynamic-LDS limit once per (kernel, device): thread-safe, and right when one process drives several GPUs
// (the attribute belongs to the device's copy of the function).
inline void allow_dynamic_lds(const void *kernel, int bytes)
{
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    if (done.insert({kernel, dev}).second) (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// Correctly rounded fp32 square root.  NOT __fsqrt_rn: this toolchain's HIP headers define it as __ocml_native_sqrt_f32 (the
// approximate one) unless OCML_BASIC_ROUNDED_OPERATIONS is set, and whether the compiler then emits the IEEE fix-up after
// v_sqrt_f32 depends on the surrounding code.  sqrtf is __ocml_sqrt_f32: correctly rounded with the (default, and explicit in the
// Makefile) -fhip-fp32-correctly-rounded-divide-sqrt.
__device__ __forceinline__ float sqrt_rn(float x) { return sqrtf(x); }

}  // namespace oryon
