// twosample.hip -- quadratic forms of an implicit kernel matrix with 0/1 group indicators, for many label columns at once
// (include/siggan_twosample.h), on v_mfma_f64_16x16x4_f64.  gfx950 only.
//
// forms = diag(L^T K0 L): two chained MFMA products.  A workgroup of four waves owns ROWS = 32 rows i (two tiles of 16,
// one after the other) and 256 label columns; wave w owns the 64 columns 64 w .. 64 w + 63 of them.  Per step over the rows
// j the four waves each form ONE 16 x 16 tile of K -- wave w against the j-tile 4 step + w --, apply the kernel function,
// zero the diagonal by row number and everything past n, and store the tile in LDS.  After one barrier every wave reads all
// four tiles and multiplies each with the 0/1 operands of its own columns, both groups, into Z = K0 [A | B]: at dim 128 a
// wave spends 32 MFMAs on K and 128 on Z per step.  The LDS tiles are double buffered, so one
// barrier per step is enough: a wave that writes buffer b again has passed the barrier of the step between, which every
// wave reaches only after its reads of b.
//
// The chaining needs no layout shuffle.  The K MFMA takes the j-rows as A and the i-rows as B, so by the f64 C/D map
// (rows_f64.h) lane l holds k(x_j, x_i) for i = i0 + (l & 15) and j = j0 + (l >> 4) + 4 * reg.  The A operand of an MFMA step is A[m = l & 15][k = l >> 4]: accumulator register v IS the
// A operand of the k-slice j = j0 + 4 v .. j0 + 4 v + 3 of Z[i][c] += sum_j K[i][j] L[j][c].  The B operand of that step is
// L[j0 + 4 v + (l >> 4)][column of lane l & 15].  Which column a lane's slot stands for is free as long as the epilogue
// agrees: slot x of sub-tile s is column c0 + 4 x + s, so one 4-byte load gives a lane the labels of all four sub-tiles.
// Z comes out as row i0 + (l >> 4) + 4 * reg, column slot l & 15; the epilogue multiplies it with the labels of those rows
// and sums over reg, the two i-tiles, then the four lane groups (xor 16, 32).  Partial forms per (row block, column) go to
// the workspace; k_forms_reduce adds them in ascending row-block order.  No atomics; every word has one writer.
//
// Dot products and norms: rows_f64.h's scheme, the one neighbors.hip is built from.  The RBF norms are the diagonals of the
// MFMA products X X^T of every 16-row tile against itself over the same chunk and step order, so a row against a
// bit-identical row gives d2 = 0.0 and k = 1.0 exactly; k_norms forms them once per call into the workspace (behind the
// partial forms) instead of once per workgroup and tile.  k(x_i, x_i) for diag[] is the diagonal tile's value before it is
// zeroed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/siggan_twosample.h"
#include "host.h"
#include "rows_f64.h"

namespace {

constexpr int WAVES = 4;
constexpr int ROWS = SIGGAN_TWOSAMPLE_ROW_BLOCK;         // rows i per workgroup
constexpr int ITILES = ROWS / NT;
constexpr int SUB = 4;                                   // column sub-tiles of 16 per wave
constexpr int WAVE_COLS = NT * SUB;                      // 64
constexpr int WG_COLS = WAVE_COLS * WAVES;               // 256
static_assert(ROWS % NT == 0, "a row block is whole tiles");

// the label bytes of row `row`, columns c .. c + 3, byte s in bits 8 s ..; rows past n and columns past cols read as 0.
// vec: cols % 4 == 0 and a 4-byte aligned base (c is a multiple of 4, so c < cols covers all four)
__device__ __forceinline__ uint32_t load_labels(const uint8_t* __restrict__ labels, int row, int n, int c, int cols, bool vec) {
    if (row >= n || c >= cols) return 0u;
    const uint8_t* p = labels + (size_t)row * (size_t)cols + c;
    if (vec) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t v = p[0];
    if (c + 1 < cols) v |= (uint32_t)p[1] << 8;
    if (c + 2 < cols) v |= (uint32_t)p[2] << 16;
    if (c + 3 < cols) v |= (uint32_t)p[3] << 24;
    return v;
}

__device__ __forceinline__ double is_label(uint32_t word, int s, uint32_t which) {
    return ((word >> (8 * s)) & 0xffu) == which ? 1.0 : 0.0;
}

// |x_i|^2 of every row as the diagonal of its tile's X X^T; grid: ceil(n / 16) workgroups of one wave
template <bool VEC>
__global__ __launch_bounds__(64) void k_norms(const float* __restrict__ xs, int n, int dim, double* __restrict__ norms) {
    const int lane = threadIdx.x, x = lane & 15, g = lane >> 4;
    const int i = blockIdx.x * NT + x;
    const bool i_ok = i < n;
    const float* irow = xs + (size_t)(i_ok ? i : 0) * (size_t)dim;
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
    for (int f0 = 0; f0 < dim; f0 += CHUNK) {
        const float4 b = load4<VEC>(irow, i_ok, f0 + 4 * g, dim);
        chunk_mfma(acc, b, b);
    }
    const double d = diagonal_of(acc, x);
    if (g == 0 && i_ok) norms[i] = d;
}

// grid: (ceil(n / ROWS), ceil(cols / 256)) workgroups of 256 threads.  partial: (gridDim.x, cols, 3).  norms (n): RBF only.
template <bool RBF, bool VEC>
__global__ __launch_bounds__(64 * WAVES) void k_forms(const float* __restrict__ xs, int n, int dim, int degree, double gamma, double coef0,
                                                      const uint8_t* __restrict__ labels, int cols, int labels_vec,
                                                      double* __restrict__ partial, const double* __restrict__ norms,
                                                      double* __restrict__ diag) {
    __shared__ double s_k[2][WAVES][4][64];              // [buffer][tile][accumulator register][lane]: 16 KiB

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = lane & 15, g = lane >> 4;
    const int c0 = blockIdx.y * WG_COLS + wave * WAVE_COLS + 4 * x;       // this lane's columns c0 .. c0 + 3 (sub-tiles 0 .. 3)
    const bool lvec = labels_vec != 0;
    const int tiles = (n + NT - 1) / NT;
    const int steps = (tiles + WAVES - 1) / WAVES;

    double faa[SUB], fbb[SUB], fab[SUB];
#pragma unroll
    for (int s = 0; s < SUB; ++s) faa[s] = fbb[s] = fab[s] = 0.0;

    int buf = 0;
    for (int it = 0; it < ITILES; ++it) {
        const int i0 = (blockIdx.x * ITILES + it) * NT;
        if (i0 >= n) break;                              // the whole workgroup leaves together
        const int i = i0 + x;                            // this lane's row as B operand of the K product
        const bool i_ok = i < n;
        const float* irow = xs + (size_t)(i_ok ? i : 0) * (size_t)dim;

        const double qn = RBF && i_ok ? norms[i] : 0.0;  // |x_i|^2

        double4_t za[SUB], zb[SUB];
#pragma unroll
        for (int s = 0; s < SUB; ++s) { za[s] = double4_t{0.0, 0.0, 0.0, 0.0}; zb[s] = double4_t{0.0, 0.0, 0.0, 0.0}; }

        uint32_t word[4];                                // the label words of the j-tile the Z product takes next: rows 4 v + g
#pragma unroll
        for (int v = 0; v < 4; ++v) word[v] = load_labels(labels, 4 * v + g, n, c0, cols, lvec);

        for (int step = 0; step < steps; ++step, buf ^= 1) {
            // ---- this wave's tile of K: rows j0 .. j0 + 15 against rows i0 .. i0 + 15
            const int t = step * WAVES + wave;
            if (t < tiles) {
                const int j0 = t * NT;
                const bool j_ok = j0 + x < n;
                const float* jrow = xs + (size_t)(j_ok ? j0 + x : 0) * (size_t)dim;
                double4_t dot = {0.0, 0.0, 0.0, 0.0};
                for (int f0 = 0; f0 < dim; f0 += CHUNK) {
                    const int kb = f0 + 4 * g;
                    const float4 a = load4<VEC>(jrow, j_ok, kb, dim);
                    const float4 b = load4<VEC>(irow, i_ok, kb, dim);
                    chunk_mfma(dot, a, b);
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int row = g + 4 * reg, j = j0 + row;               // the row j this register holds against row i
                    double k;
                    if (RBF) {
                        const double rn = j < n ? norms[j] : 0.0;
                        k = exp(-gamma * fmax((qn + rn) - 2.0 * dot[reg], 0.0));
                    } else {
                        const double v = gamma * dot[reg] + coef0;
                        k = degree == 1 ? v : degree == 2 ? v * v : (v * v) * v;
                    }
                    if (j == i) {                                            // by row number, whatever the values are
                        if (diag && i_ok && blockIdx.y == 0) diag[i] = k;
                        k = 0.0;
                    }
                    if (!i_ok || j >= n) k = 0.0;
                    s_k[buf][wave][reg][lane] = k;
                }
            }
            __syncthreads();
            // ---- every tile of this step against this wave's columns: Z += K0 [A | B]
#pragma unroll 1
            for (int w = 0; w < WAVES; ++w) {
                const int tw = step * WAVES + w;
                if (tw >= tiles) break;
                // the next tile's label words (this step's or the next one's; past n they read as 0) are on their way while
                // this tile's 32 MFMAs run
                uint32_t next[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) next[v] = load_labels(labels, (tw + 1) * NT + 4 * v + g, n, c0, cols, lvec);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const double a = s_k[buf][w][v][lane];
#pragma unroll
                    for (int s = 0; s < SUB; ++s) {
                        za[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, is_label(word[v], s, 1u), za[s], 0, 0, 0);
                        zb[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, is_label(word[v], s, 2u), zb[s], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) word[v] = next[v];
            }
        }

        // ---- Z holds rows i0 + g + 4 reg, column slot x: times those rows' labels, summed over reg
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const uint32_t word = load_labels(labels, i0 + g + 4 * reg, n, c0, cols, lvec);
#pragma unroll
            for (int s = 0; s < SUB; ++s) {
                const double la = is_label(word, s, 1u), lb = is_label(word, s, 2u);
                faa[s] += la * za[s][reg];
                fbb[s] += lb * zb[s][reg];
                fab[s] += la * zb[s][reg];
            }
        }
    }

    // the four lane groups hold different rows of the same columns
#pragma unroll
    for (int s = 0; s < SUB; ++s) {
        faa[s] += __shfl_xor(faa[s], 16); faa[s] += __shfl_xor(faa[s], 32);
        fbb[s] += __shfl_xor(fbb[s], 16); fbb[s] += __shfl_xor(fbb[s], 32);
        fab[s] += __shfl_xor(fab[s], 16); fab[s] += __shfl_xor(fab[s], 32);
        const int c = c0 + s;
        if (g == 0 && c < cols) {
            double* out = partial + ((size_t)blockIdx.x * (size_t)cols + (size_t)c) * 3;
            out[0] = faa[s];
            out[1] = fbb[s];
            out[2] = fab[s];
        }
    }
}

// forms[e] = sum over the row blocks, ascending, of partial[block][e]; e runs over cols * 3
__global__ __launch_bounds__(256) void k_forms_reduce(const double* __restrict__ partial, int row_blocks, int entries,
                                                      double* __restrict__ forms) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= entries) return;
    double sum = 0.0;
    for (int b = 0; b < row_blocks; ++b) sum += partial[(size_t)b * (size_t)entries + e];
    forms[e] = sum;
}

bool sizes_ok(int n, int cols) {
    return n >= 1 && n <= SIGGAN_TWOSAMPLE_MAX_N && cols >= 1 && cols <= SIGGAN_TWOSAMPLE_MAX_COLS;
}

int row_blocks_of(int n) { return (n + ROWS - 1) / ROWS; }

}  // namespace

extern "C" size_t siggan_kernel_forms_workspace(int32_t n, int32_t cols) {
    if (!sizes_ok(n, cols)) return 0;
    return ((size_t)row_blocks_of(n) * (size_t)cols * 3 + (size_t)n) * sizeof(double);       // the partial forms, then the norms
}

extern "C" int siggan_kernel_forms(int32_t device, const float* x_dev, int32_t n, int32_t dim, const siggan_kernel_spec* spec,
                                   const uint8_t* labels_dev, int32_t cols, double* forms_dev, double* diag_dev, void* workspace_dev,
                                   size_t workspace_bytes, void* stream) {
    const char* who = "siggan_kernel_forms";
    if (n < 1 || n > SIGGAN_TWOSAMPLE_MAX_N) return FAIL(SIGGAN_E_INVALID, "%s: n = %d outside [1, %d]", who, n, SIGGAN_TWOSAMPLE_MAX_N);
    if (cols < 1 || cols > SIGGAN_TWOSAMPLE_MAX_COLS)
        return FAIL(SIGGAN_E_INVALID, "%s: cols = %d outside [1, %d]", who, cols, SIGGAN_TWOSAMPLE_MAX_COLS);
    if (dim < 1 || dim > SIGGAN_TWOSAMPLE_MAX_DIM)
        return FAIL(SIGGAN_E_INVALID, "%s: dim %d outside [1, %d]", who, dim, SIGGAN_TWOSAMPLE_MAX_DIM);
    if (!x_dev || !labels_dev || !forms_dev || !spec) return FAIL(SIGGAN_E_INVALID, "%s: null tensor or spec", who);
    if (spec->kind != SIGGAN_KERNEL_POLY && spec->kind != SIGGAN_KERNEL_RBF)
        return FAIL(SIGGAN_E_INVALID, "%s: kernel kind %d is neither POLY (0) nor RBF (1)", who, spec->kind);
    if (!(spec->gamma > 0.0) || !isfinite(spec->gamma)) return FAIL(SIGGAN_E_INVALID, "%s: gamma = %g must be finite and > 0", who, spec->gamma);
    const bool rbf = spec->kind == SIGGAN_KERNEL_RBF;
    if (!rbf && (spec->degree < 1 || spec->degree > 3)) return FAIL(SIGGAN_E_INVALID, "%s: degree = %d outside [1, 3]", who, spec->degree);
    if (!rbf && !isfinite(spec->coef0)) return FAIL(SIGGAN_E_INVALID, "%s: coef0 = %g must be finite", who, spec->coef0);
    const size_t need = siggan_kernel_forms_workspace(n, cols);
    if (!workspace_dev) return FAIL(SIGGAN_E_INVALID, "%s: null workspace", who);
    if (reinterpret_cast<uintptr_t>(workspace_dev) & 7) return FAIL(SIGGAN_E_INVALID, "%s: workspace is not 8-byte aligned", who);
    if (workspace_bytes < need)
        return FAIL(SIGGAN_E_INVALID, "%s: workspace of %zu bytes, n = %d and cols = %d need %zu", who, workspace_bytes, n, cols, need);
    DevGuard dg(device); HIPCHK(dg.err);
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = rows_allow_16_byte_loads(dim, x_dev);
    const int labels_vec = (cols & 3) == 0 && (reinterpret_cast<uintptr_t>(labels_dev) & 3) == 0;
    double* partial = static_cast<double*>(workspace_dev);
    const int row_blocks = row_blocks_of(n);
    double* norms = partial + (size_t)row_blocks * (size_t)cols * 3;
    if (rbf) {
        if (vec) hipLaunchKernelGGL((k_norms<true>), dim3((unsigned)((n + NT - 1) / NT)), dim3(64), 0, st, x_dev, n, dim, norms);
        else     hipLaunchKernelGGL((k_norms<false>), dim3((unsigned)((n + NT - 1) / NT)), dim3(64), 0, st, x_dev, n, dim, norms);
        HIPCHK(hipGetLastError());
    }
    const dim3 grid((unsigned)row_blocks, (unsigned)((cols + WG_COLS - 1) / WG_COLS)), block(64 * WAVES);
    const int degree = rbf ? 0 : spec->degree;
    const double gamma = spec->gamma, coef0 = rbf ? 0.0 : spec->coef0;
#define TWOSAMPLE_LAUNCH(R, V) \
    hipLaunchKernelGGL((k_forms<R, V>), grid, block, 0, st, x_dev, n, dim, degree, gamma, coef0, labels_dev, cols, labels_vec, partial, norms, diag_dev)
    if (rbf) { if (vec) TWOSAMPLE_LAUNCH(true, true); else TWOSAMPLE_LAUNCH(true, false); }
    else     { if (vec) TWOSAMPLE_LAUNCH(false, true); else TWOSAMPLE_LAUNCH(false, false); }
#undef TWOSAMPLE_LAUNCH
    HIPCHK(hipGetLastError());
    const int entries = cols * 3;
    hipLaunchKernelGGL(k_forms_reduce, dim3(blocks(entries)), dim3(256), 0, st, partial, row_blocks, entries, forms_dev);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}
