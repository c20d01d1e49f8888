// image_pairs.h -- what the ops that score every image of a set a against every image of a set b share (ssim.hip, dtw.hip):
// the three modes and their refusals, a row's best value as one 64-bit key per (row, split), the kernel that takes the
// splits in order, and the launch sequence around an op's own pairs kernel.  gfx950 only.
//
// A pairs kernel runs on a grid (row tiles, S).  Split s owns columns [s * per, min(nb, (s + 1) * per)) (pair_plan.h); in
// PAIRED mode there is one split and a row's only column is its own number.  The wave that owns row i keeps the best key
// of its columns and writes it to keys[i * S + s]; equal values go to the lower column, inside a split by the key's low
// half and across splits by k_pair_best's order.  No atomics anywhere.  (A split's range and "j == i in SAME_SET" stay
// written out in the two kernels: as functions they changed the kernels' instructions, profiles/image_pairs_resources.md.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/siggan_dtw.h"
#include "../../include/siggan_ssim.h"
#include "host.h"
#include "pair_plan.h"

namespace {

enum { PAIRS_ALL, PAIRS_SAME_SET, PAIRS_PAIRED };
static_assert(SIGGAN_SSIM_ALL == PAIRS_ALL && SIGGAN_SSIM_SAME_SET == PAIRS_SAME_SET && SIGGAN_SSIM_PAIRED == PAIRS_PAIRED &&
                  SIGGAN_DTW_ALL == PAIRS_ALL && SIGGAN_DTW_SAME_SET == PAIRS_SAME_SET && SIGGAN_DTW_PAIRED == PAIRS_PAIRED,
              "both headers' mode enums are 0, 1, 2");

// An fp32 bit pattern as an unsigned integer of the same order (SSIM lies in [-1, 1]).
__device__ __forceinline__ uint32_t ordered_bits(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered_bits(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }

// The two orders of a key, "better value, then lower column": value bits << 32 | (column ^ COLUMN_XOR).
struct HighestF32 {                       // the LARGEST key wins; no finite value maps to 0
    using Value = float;
    static constexpr unsigned long long NONE = 0ull; static constexpr float NO_VALUE = -1.0f; static constexpr uint32_t COLUMN_XOR = ~0u;
    static __device__ __forceinline__ unsigned long long key(float value, int j) {
        return ((unsigned long long)ordered_bits(value) << 32) | (unsigned long long)(~(uint32_t)j);
    }
    static __device__ __forceinline__ unsigned long long better(unsigned long long k, unsigned long long m) { return k > m ? k : m; }
    static __device__ __forceinline__ float value(unsigned long long k) { return unordered_bits((uint32_t)(k >> 32)); }
};
struct LowestI32 {                        // the SMALLEST key wins, of values >= 0
    using Value = int32_t;
    static constexpr unsigned long long NONE = ~0ull; static constexpr int32_t NO_VALUE = -1; static constexpr uint32_t COLUMN_XOR = 0u;
    static __device__ __forceinline__ unsigned long long key(int32_t value, int j) {
        return ((unsigned long long)(uint32_t)value << 32) | (unsigned long long)(uint32_t)j;
    }
    static __device__ __forceinline__ unsigned long long better(unsigned long long k, unsigned long long m) { return k < m ? k : m; }
    static __device__ __forceinline__ int32_t value(unsigned long long k) { return (int32_t)(k >> 32); }
};

// Where pair (i, j) goes in `matrix`: (na, nb) row-major, (na) in PAIRED mode.
__device__ __forceinline__ size_t matrix_slot(bool paired, int i, int j, int nb) { return paired ? (size_t)i : (size_t)i * nb + j; }
template <typename Key>                  // best: the wave's key so far, Key::NONE at the start
__device__ __forceinline__ void keep_better(unsigned long long& best, typename Key::Value value, int j) { best = Key::better(Key::key(value, j), best); }

template <typename Key>
__global__ void k_pair_best(const unsigned long long* __restrict__ keys, int na, int S, typename Key::Value* __restrict__ best,
                            int32_t* __restrict__ best_index) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= na) return;
    unsigned long long m = Key::NONE;
    for (int s = 0; s < S; ++s) m = Key::better(keys[(size_t)i * S + s], m);
    if (best) best[i] = m != Key::NONE ? Key::value(m) : Key::NO_VALUE;
    if (best_index) best_index[i] = m != Key::NONE ? (int32_t)((uint32_t)m ^ Key::COLUMN_XOR) : -1;
}

// The refusals both entry points state, in their order: na / nb -- the op's sizes -- mode, no output -- null a -- SAME_SET --
// null b -- PAIRED -- alignment.  The order is part of the ABI, so these are several functions with the op's own checks
// between them.  prefix: "SIGGAN_SSIM" / "SIGGAN_DTW", as the messages name the enum.
inline int pairs_refuse_counts(int na, int nb) {
    return na < 1 || nb < 1 ? FAIL(SIGGAN_E_INVALID, "na = %d, nb = %d: both must be >= 1", na, nb) : SIGGAN_OK;
}
inline int pairs_refuse_mode_or_no_output(const char* prefix, int mode, bool any_output) {
    if (mode != PAIRS_ALL && mode != PAIRS_SAME_SET && mode != PAIRS_PAIRED)
        return FAIL(SIGGAN_E_INVALID, "mode = %d is none of %s_ALL, %s_SAME_SET, %s_PAIRED", mode, prefix, prefix, prefix);
    return any_output ? SIGGAN_OK : FAIL(SIGGAN_E_INVALID, "no output: give matrix, best or best_index");
}
// b_is_a: every pointer of b is null or a's.  as: "a's pointer" / "a's pointers".  The caller then lets b be a.
inline int pairs_refuse_same_set(const char* prefix, int mode, bool b_is_a, int na, int nb, const char* as) {
    const bool bad = mode == PAIRS_SAME_SET && (!b_is_a || nb != na);
    return bad ? FAIL(SIGGAN_E_INVALID, "%s_SAME_SET: b must be a (null or %s, nb == na)", prefix, as) : SIGGAN_OK;
}
inline int pairs_refuse_paired(const char* prefix, int mode, int na, int nb, bool want_best) {
    if (mode == PAIRS_PAIRED && nb != na) return FAIL(SIGGAN_E_INVALID, "%s_PAIRED: na = %d != nb = %d", prefix, na, nb);
    if (mode == PAIRS_PAIRED && want_best) return FAIL(SIGGAN_E_INVALID, "%s_PAIRED has no best / best_index", prefix);
    return SIGGAN_OK;
}

// The launch sequence: the keys when a best is wanted, the op's pairs kernel (launch_pairs(keys) enqueues it on `st`; keys
// is null when no best is wanted), k_pair_best, the keys freed in stream order.  Returns the first launch error.
template <typename Key, typename LaunchPairs>
int pairs_launch(hipStream_t st, int na, int S, typename Key::Value* best, int32_t* best_index, LaunchPairs launch_pairs) {
    const bool want_best = best || best_index;
    unsigned long long* keys = nullptr;
    if (want_best) {
        const size_t bytes = (size_t)na * S * sizeof(unsigned long long);
        hipError_t e = hipMallocAsync((void**)&keys, bytes, st);
        if (e != hipSuccess) return FAIL(SIGGAN_E_NOMEM, "hipMallocAsync(%zu) -> %s", bytes, hipGetErrorString(e));
    }
    launch_pairs(keys);
    hipError_t launched = hipGetLastError();
    if (want_best && launched == hipSuccess) {
        hipLaunchKernelGGL(k_pair_best<Key>, dim3(blocks(na)), dim3(256), 0, st, keys, na, S, best, best_index);
        launched = hipGetLastError();
    }
    if (want_best) (void)hipFreeAsync(keys, st);
    HIPCHK(launched);
    return SIGGAN_OK;
}

}  // namespace
