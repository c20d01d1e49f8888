/*
 * siggan_twosample.h -- C ABI of the one primitive kernel two-sample statistics are made of, on the MI355X in fp64:
 * quadratic forms of an implicit kernel matrix with 0/1 group-indicator vectors, for many groupings at once.  The unbiased
 * MMD^2 estimator (the Kernel Inception Distance of Binkowski et al. 2018, over subsets) and a permutation test of the
 * same statistic (over label permutations) both reduce to it.  The rows this package feeds it are the Siamese verifier's
 * embeddings, which siggan_verifier_embed leaves on the device; the (n, n) kernel matrix is never materialised: a launch
 * writes three numbers per grouping.
 *
 * The calls are context-free, like siggan_neighbors.h: `device` is the HIP ordinal the pointers belong to.  Conventions
 * are those of siggan.h: plain pointers and sizes, every call enqueues on `stream` and never synchronises the host, no
 * call allocates, 0 = OK / negative = SIGGAN_E_* with the message in siggan_last_error(), the caller's current device is
 * restored.  Adding this header did not change SIGGAN_ABI_VERSION: it only adds symbols.
 *
 * Arithmetic: dot products and squared norms run on v_mfma_f64_16x16x4_f64 over the fp32 values widened to fp64 (exact,
 * and so is every product), in the same order of the feature index; d2 = max(0, (|a|^2 + |b|^2) - 2 a.b) as in
 * siggan_neighbors.h; the polynomial's power is formed by plain multiplications, exp is the device library's fp64 exp.
 * The sums over rows run on the same MFMA against the 0/1 operands, then in a fixed order over the workgroups' partial
 * results: no atomics, equal input gives bit-equal output.  When every k(x_i, x_j) and every partial sum is an integer
 * below 2^53 the result is exact.
 *
 * Shape of the work: a workgroup of four waves owns SIGGAN_TWOSAMPLE_ROW_BLOCK rows i and 256 label columns.  Per step
 * each wave forms one 16 x 16 tile of K against a different tile of rows j, the four tiles are shared through LDS, and
 * every wave multiplies all four with the 0/1 operands of its own 64 columns (both groups).  The per-workgroup partial
 * forms go to the caller's workspace; a second kernel adds them in ascending row-block order.  For the RBF kernel a first
 * kernel forms every row's squared norm once, into the workspace too.
 */
#ifndef SIGGAN_TWOSAMPLE_H
#define SIGGAN_TWOSAMPLE_H

#include <stddef.h>

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SIGGAN_KERNEL_POLY = 0, SIGGAN_KERNEL_RBF = 1 };
typedef struct siggan_kernel_spec {
    int32_t kind;      /* POLY: k(a,b) = (gamma * a.b + coef0)^degree     RBF: k(a,b) = exp(-gamma * d2(a,b)) */
    int32_t degree;    /* POLY: 1, 2 or 3 (RBF: ignored) */
    double  gamma;     /* finite, > 0 */
    double  coef0;     /* POLY only, finite */
} siggan_kernel_spec;

#define SIGGAN_TWOSAMPLE_MAX_N     16384
#define SIGGAN_TWOSAMPLE_MAX_COLS  4096
#define SIGGAN_TWOSAMPLE_MAX_DIM   1024
#define SIGGAN_TWOSAMPLE_ROW_BLOCK 32        /* rows i per workgroup: the workspace holds one partial per block and column */

/* Bytes of workspace siggan_kernel_forms needs for these sizes: 24 * ceil(n / SIGGAN_TWOSAMPLE_ROW_BLOCK) * cols for the
 * partial forms plus 8 * n for the rows' squared norms (3 MiB + 32 KiB at n = 4096, cols = 1024); 0 for sizes the call
 * refuses. */
size_t siggan_kernel_forms_workspace(int32_t n, int32_t cols);

/* x_dev (n, dim) fp32 row-major.  labels_dev (n, cols) uint8 row-major: 0 = row i is in neither group of column p,
 * 1 = group A, 2 = group B, any other value is treated as 0.  forms_dev (cols, 3) fp64; with K0 the kernel matrix of the
 * rows of x, its diagonal removed BY ROW NUMBER, not by value (two bit-identical rows still see each other):
 *   forms[p][0] = sum_{i != j, both in A_p} k(x_i, x_j)
 *   forms[p][1] = sum_{i != j, both in B_p} k(x_i, x_j)
 *   forms[p][2] = sum_{i in A_p, j in B_p} k(x_i, x_j)
 * over ORDERED pairs, so [0] and [1] are twice the sums over unordered pairs.  diag_dev (n) fp64, may be NULL: receives
 * k(x_i, x_i) (what the biased V-statistic adds).  workspace_dev: 8-byte aligned, at least
 * siggan_kernel_forms_workspace(n, cols) bytes; its contents on entry do not matter.
 * 1 <= n <= SIGGAN_TWOSAMPLE_MAX_N, 1 <= cols <= SIGGAN_TWOSAMPLE_MAX_COLS, 1 <= dim <= SIGGAN_TWOSAMPLE_MAX_DIM, a spec
 * as described above, else SIGGAN_E_INVALID.  NaN / Inf inputs are not part of the contract. */
int siggan_kernel_forms(int32_t device, const float *x_dev, int32_t n, int32_t dim, const siggan_kernel_spec *spec,
                        const uint8_t *labels_dev, int32_t cols, double *forms_dev, double *diag_dev,
                        void *workspace_dev, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_TWOSAMPLE_H */
