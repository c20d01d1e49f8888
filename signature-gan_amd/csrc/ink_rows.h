// ink_rows.h -- what the byte-image ops components.hip and strokes.hip share: a row's ink mask by wave64 ballot, the walk
// over a row-major grid without a division per item, and the refusals of the image arguments.  gfx950 only.
// (strokes_word.h is the arithmetic ON such masks, and compiles for the host.)
//
// Ink is byte < threshold.  A row's mask is two 64-bit words, bit x & 63 of word x >> 6 for column x; bits at and beyond
// the width are 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "../../include/siggan.h"
#include "host.h"

namespace {

// Word `seg` of the ink mask of row y of an image of width w (its bytes in LDS or global).  A whole wave calls it, lane = 0 .. 63.
__device__ __forceinline__ uint64_t ink_word(const uint8_t* img, int w, int y, int seg, int lane, int thr) {
    const int x = seg * 64 + lane;
    const bool ink = x < w && (int)img[y * w + x] < thr;
    return __ballot(ink);
}

__device__ __forceinline__ int bit_at(const uint64_t* m, int y, int x) { return (int)(m[2 * y + (x >> 6)] >> (x & 63)) & 1; }

// Items first, first + stride, ... of a row-major grid with per_row items in a row, as (row y, place x in the row), with
// the two divisions paid once.  stride may exceed per_row; x stays below it.  (k_strokes keeps walks of its own.)
struct RowWalk {
    int i, y, x, stride, dy, dx, per_row;
    __device__ RowWalk(int first, int stride_, int per_row_)
        : i(first), y(first / per_row_), x(first % per_row_), stride(stride_), dy(stride_ / per_row_), dx(stride_ % per_row_), per_row(per_row_) {}
    __device__ void next() { i += stride; y += dy; x += dx; if (x >= per_row) { x -= per_row; ++y; } }
};

// The refusals of (u8_dev, batch, height, width, threshold), in the order both entry points state them.  no_output: the
// message when the caller asked for no output at all, else null -- it stands between the null image and the sizes.
inline int ink_refuse_images(const void* u8_dev, const char* no_output, int batch, int height, int width, int max_size, int threshold) {
    if (!u8_dev) return FAIL(SIGGAN_E_INVALID, "null image tensor");
    if (no_output) return FAIL(SIGGAN_E_INVALID, "%s", no_output);
    if (batch < 1) return FAIL(SIGGAN_E_INVALID, "batch = %d < 1", batch);
    if (height < 1 || height > max_size) return FAIL(SIGGAN_E_INVALID, "height = %d outside [1, %d]", height, max_size);
    if (width < 4 || width > max_size || (width & 3))
        return FAIL(SIGGAN_E_INVALID, "width = %d must be a multiple of 4 in [4, %d]", width, max_size);
    if (threshold < 1 || threshold > 255) return FAIL(SIGGAN_E_INVALID, "threshold = %d outside [1, 255]", threshold);
    return SIGGAN_OK;
}

// why: what the fill byte stands for, e.g. "the paper must not be ink"
inline int ink_refuse_fill(int fill, int threshold, const char* why) {
    if (fill < threshold || fill > 255) return FAIL(SIGGAN_E_INVALID, "fill = %d outside [threshold = %d, 255]: %s", fill, threshold, why);
    return SIGGAN_OK;
}

// names: the pointers as the message lists them, e.g. "u8_dev, stats_dev and clean_dev"; null pointers pass
inline int ink_refuse_unaligned(std::initializer_list<const void*> ptrs, const char* names) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
    if (bits & 3) return FAIL(SIGGAN_E_INVALID, "%s must be 4-byte aligned", names);
    return SIGGAN_OK;
}

}  // namespace
