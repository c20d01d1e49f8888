// moments.hip -- streaming fp64 feature moments (include/siggan_moments.h): s += sum_r x[r,:], G += x^T x over batches of
// fp32 feature rows, on v_mfma_f64_16x16x4_f64.  gfx950 only.
//
// One launch per update, k_moments_update: one wave (one block of 64 threads) per 16x16 tile (bi, bj) of G's upper
// triangle, bi <= bj.  The K loop runs over the rows four at a time: lane l holds feature l & 15 of row r0 + (l >> 4) for
// both operands (A = a 16-feature x 4-row slice of x^T, B = the 4-row x 16-feature slice of x), widened fp32 -> fp64 on
// load.  The f64 MFMA's C/D map is col = l & 15, row = (l >> 4) + 4 * reg -- NOT the f32 16x16 map.  Rows past n_rows and
// features past dim load as 0.0; lanes whose element lies outside G store nothing.  The diagonal-tile waves also own
// the sum vector.  Accumulation across calls is a read-add-write by the tile's one owner; the store writes the element
// and its mirror image, so the lower triangle always equals the upper one bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "../../include/siggan_moments.h"
#include "host.h"
#include "rows_f64.h"                                    // double4_t, nothing else: the operand layout here differs

struct siggan_moments {
    int device, dim;
    int64_t count;          // rows of every update enqueued since create / reset (host side)
    double* sum;            // (dim), device
    double* gram;           // (dim, dim), device; sum and gram are one allocation
};

namespace {

constexpr int MT = 16;                                   // tile edge

// grid: T * (T + 1) / 2 blocks of one wave, T = ceil(dim / 16); block t is the t-th tile of the upper triangle, row-major
__global__ __launch_bounds__(64) void k_moments_update(const float* __restrict__ x, int n_rows, int dim, int tiles,
                                                       double* __restrict__ sum, double* __restrict__ gram) {
    int t = blockIdx.x, bi = 0;
    for (int len = tiles; t >= len; t -= len, --len) ++bi;               // wave-uniform: at most 64 steps
    const int bj = bi + t;
    const int lane = threadIdx.x, f = lane & 15, q = lane >> 4;
    const int fa = bi * MT + f, fb = bj * MT + f;
    const bool ina = fa < dim, inb = fb < dim;

    double4_t acc = {0.0, 0.0, 0.0, 0.0};
    double colsum = 0.0;                                                  // this lane's rows of feature fa
    for (int r0 = 0; r0 < n_rows; r0 += 4) {
        const int r = r0 + q;
        const bool inr = r < n_rows;
        const size_t row = (size_t)r * (size_t)dim;
        const double a = (inr && ina) ? (double)x[row + fa] : 0.0;
        const double b = (inr && inb) ? (double)x[row + fb] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        colsum += a;
    }

    const int col = bj * MT + f;
    if (bi == bj) {
        // sum vector: the four row groups of a feature, always in the same order
        colsum += __shfl_xor(colsum, 16);
        colsum += __shfl_xor(colsum, 32);
        if (q == 0 && ina) sum[fa] += colsum;
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int row = bi * MT + q + 4 * reg;
        // a diagonal tile holds both triangles: its upper half is stored and mirrored like every other tile
        if (row < dim && col < dim && row <= col) {
            const double v = gram[(size_t)row * dim + col] + acc[reg];
            gram[(size_t)row * dim + col] = v;
            if (row != col) gram[(size_t)col * dim + row] = v;
        }
    }
}

}  // namespace

extern "C" int siggan_moments_create(int32_t device, int32_t dim, siggan_moments** out) {
    if (!out) return FAIL(SIGGAN_E_INVALID, "siggan_moments_create: null argument");
    *out = nullptr;
    if (dim < 1 || dim > SIGGAN_MOMENTS_MAX_DIM)
        return FAIL(SIGGAN_E_INVALID, "siggan_moments_create: dim %d outside [1, %d]", dim, SIGGAN_MOMENTS_MAX_DIM);
    DevGuard dg(device); HIPCHK(dg.err);
    siggan_moments* m = new (std::nothrow) siggan_moments();
    if (!m) return FAIL(SIGGAN_E_NOMEM, "out of host memory");
    m->device = device; m->dim = dim; m->count = 0; m->sum = nullptr; m->gram = nullptr;
    const size_t bytes = sizeof(double) * (size_t)dim * ((size_t)dim + 1);
    hipError_t e = hipMalloc((void**)&m->sum, bytes);
    if (e != hipSuccess) { delete m; return FAIL(SIGGAN_E_NOMEM, "hipMalloc(%zu) -> %s", bytes, hipGetErrorString(e)); }
    m->gram = m->sum + dim;
    e = hipMemset(m->sum, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();                      // zeroed before any stream's first update
    if (e != hipSuccess) {
        (void)hipFree(m->sum); delete m;
        return FAIL(SIGGAN_E_HIP, "siggan_moments_create: clearing the accumulator -> %s", hipGetErrorString(e));
    }
    *out = m;
    return SIGGAN_OK;
}

extern "C" int siggan_moments_destroy(siggan_moments* m) {
    if (!m) return SIGGAN_OK;
    DevGuard dg(m->device);
    (void)hipDeviceSynchronize();
    if (m->sum) (void)hipFree(m->sum);
    delete m;
    return SIGGAN_OK;
}

extern "C" int siggan_moments_reset(siggan_moments* m, void* stream) {
    if (!m) return FAIL(SIGGAN_E_INVALID, "siggan_moments_reset: null argument");
    DevGuard dg(m->device); HIPCHK(dg.err);
    HIPCHK(hipMemsetAsync(m->sum, 0, sizeof(double) * (size_t)m->dim * ((size_t)m->dim + 1), (hipStream_t)stream));
    m->count = 0;
    return SIGGAN_OK;
}

extern "C" int siggan_moments_update(siggan_moments* m, const float* x_dev, int32_t n_rows, void* stream) {
    if (!m || !x_dev) return FAIL(SIGGAN_E_INVALID, "siggan_moments_update: null argument");
    if (n_rows < 1) return FAIL(SIGGAN_E_INVALID, "siggan_moments_update: n_rows must be >= 1, got %d", n_rows);
    DevGuard dg(m->device); HIPCHK(dg.err);
    const int tiles = (m->dim + MT - 1) / MT;
    hipLaunchKernelGGL(k_moments_update, dim3((unsigned)(tiles * (tiles + 1) / 2)), dim3(64), 0, (hipStream_t)stream, x_dev,
                       n_rows, m->dim, tiles, m->sum, m->gram);
    if (hipGetLastError() != hipSuccess) return FAIL(SIGGAN_E_HIP, "siggan_moments_update: kernel launch failed");
    m->count += n_rows;
    return SIGGAN_OK;
}

extern "C" int siggan_moments_read(siggan_moments* m, double* sum_dev, double* gram_dev, int64_t* count, void* stream) {
    if (!m) return FAIL(SIGGAN_E_INVALID, "siggan_moments_read: null argument");
    DevGuard dg(m->device); HIPCHK(dg.err);
    const size_t d = (size_t)m->dim;
    if (sum_dev) HIPCHK(hipMemcpyAsync(sum_dev, m->sum, sizeof(double) * d, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (gram_dev) HIPCHK(hipMemcpyAsync(gram_dev, m->gram, sizeof(double) * d * d, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (count) *count = m->count;
    return SIGGAN_OK;
}
