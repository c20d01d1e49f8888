/*
 * siggan_neighbors.h -- C ABI of exact k-nearest-neighbour queries between two sets of fp32 feature rows on the MI355X, in
 * fp64: what improved precision / recall (Kynkaanniemi et al. 2019), density / coverage (Naeem et al. 2020) and a
 * memorisation check (generated -> nearest real against the real set's own leave-one-out distances) are made of.  The rows
 * this package feeds it are the Siamese verifier's embeddings, which siggan_verifier_embed leaves on the device; the
 * (nq, nr) distance matrix is never materialised: a launch writes k numbers (or one count) per query row.
 *
 * Both calls are context-free, like siggan_select.h: `device` is the HIP ordinal the pointers belong to.  Conventions are
 * those of siggan.h: plain pointers and sizes, every call enqueues on `stream` and never synchronises the host, no call
 * allocates, 0 = OK / negative = SIGGAN_E_* with the message in siggan_last_error(), the caller's current device is
 * restored.  Adding this header did not change SIGGAN_ABI_VERSION: it only adds symbols.
 *
 * Arithmetic: d2(i, j) = max(0, (|q_i|^2 + |r_j|^2) - 2 q_i.r_j).  All three sums run on v_mfma_f64_16x16x4_f64 over the
 * fp32 values widened to fp64 (exact, and so is every product), in the same order of the feature index, so a row against
 * a bit-identical row gives exactly 0.0 and bit-identical reference rows give bit-equal distances.  No atomics, a fixed
 * order of every merge: equal input gives bit-equal output.
 *
 * Shape of the work: one workgroup of four waves per 16 query rows; the waves split the reference rows and merge through
 * LDS, so no workspace is needed.  The price is thin parallelism when nq is small and nr large (nq = 16 keeps one compute
 * unit busy however many reference rows there are), and every workgroup forms the reference rows' norms again.
 */
#ifndef SIGGAN_NEIGHBORS_H
#define SIGGAN_NEIGHBORS_H

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_KNN_MAX_K   16
#define SIGGAN_KNN_MAX_DIM 1024

/* For every row i of q (nq, dim) fp32: the k smallest squared Euclidean distances to the rows of r (nr, dim) fp32,
 * ascending, in dist2_dev (nq, k) fp64, with their row numbers in index_dev (nq, k) int32 (either may be NULL, not both).
 * Equal distances: lower row number first.  exclude_diagonal != 0 skips j == i (q and r are then the same set; the
 * exclusion is by row number, not by value).  d2 is clamped at 0.
 * 1 <= k <= SIGGAN_KNN_MAX_K, k <= nr - (exclude_diagonal ? 1 : 0), 1 <= dim <= SIGGAN_KNN_MAX_DIM, nq, nr >= 1,
 * else SIGGAN_E_INVALID.  NaN / Inf inputs are not part of the contract. */
int siggan_knn(int32_t device, const float *q_dev, int32_t nq, const float *r_dev, int32_t nr, int32_t dim, int32_t k,
               int32_t exclude_diagonal, double *dist2_dev, int32_t *index_dev, void *stream);

/* count_dev[i] = #{ j in [0, nr) : d2(q_i, r_j) <= radius2_dev[j] }, radius2_dev (nr) fp64: in how many of the balls
 * around the rows of r the row q_i lies.  d2 is siggan_knn's, bit for bit.  Sizes as above, else SIGGAN_E_INVALID. */
int siggan_ball_count(int32_t device, const float *q_dev, int32_t nq, const float *r_dev, int32_t nr, int32_t dim,
                      const double *radius2_dev, int32_t *count_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_NEIGHBORS_H */
