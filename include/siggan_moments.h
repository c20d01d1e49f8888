/*
 * siggan_moments.h -- C ABI of the streaming fp64 feature moments on the MI355X: the sum vector and the Gram matrix of
 * fp32 feature rows, accumulated on the device batch by batch.  Mean and covariance of N embeddings (what a Frechet
 * distance between two sets needs) follow from them on the host: mu = s / N, cov = (G - N mu mu^T) / (N - 1).
 *
 * An accumulator holds s (dim) and G (dim, dim) in device memory, both fp64, and a row count on the host (every call
 * knows its n_rows, so nothing is read back for it).  update is ONE launch: G is tiled 16x16, one wave per tile of the
 * upper triangle, K loop over the rows four at a time on v_mfma_f64_16x16x4_f64; the fp32 values are widened on load,
 * which is exact, and so is every product.  A tile is added to by its one owning wave with a plain read-add-write: no
 * atomics, a fixed order, bit-identical from run to run.  The store mirrors the upper triangle into the lower one, so G
 * is a full, exactly symmetric matrix at every moment.
 *
 * Conventions are those of siggan.h: plain pointers and sizes, every call enqueues on `stream` and never synchronises
 * the host (create and destroy excepted), 0 = OK / negative = SIGGAN_E_* with the message in siggan_last_error(), entry
 * points run on the accumulator's device and restore the caller's current device.  Calls on one stream are ordered; an
 * accumulator is used from one stream at a time.  Adding this header did not change SIGGAN_ABI_VERSION: it only adds
 * symbols.
 */
#ifndef SIGGAN_MOMENTS_H
#define SIGGAN_MOMENTS_H

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_MOMENTS_MAX_DIM 1024

typedef struct siggan_moments siggan_moments;

/* dim in 1..SIGGAN_MOMENTS_MAX_DIM, else SIGGAN_E_INVALID.  Allocates 8 * dim * (dim + 1) bytes, zeroed. */
int siggan_moments_create(int32_t device, int32_t dim, siggan_moments **out);
int siggan_moments_destroy(siggan_moments *m);
/* s = 0, G = 0, count = 0 */
int siggan_moments_reset(siggan_moments *m, void *stream);
/* x_dev: (n_rows, dim) fp32 row-major, n_rows >= 1:  s += sum_r x[r,:],  G += x^T x  (fp32 -> fp64 on load, exact) */
int siggan_moments_update(siggan_moments *m, const float *x_dev, int32_t n_rows, void *stream);
/* sum_dev (dim) and gram_dev (dim, dim) fp64 device buffers, either may be NULL; gram_dev receives the full symmetric
 * matrix.  *count (host, may be NULL) = rows of every update enqueued so far.  The two copies are enqueued on `stream`. */
int siggan_moments_read(siggan_moments *m, double *sum_dev, double *gram_dev, int64_t *count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_MOMENTS_H */
