/*
 * siggan_diverse.h -- C ABI of diversity-aware selection on the MI355X: greedy farthest-point picks among fp32 feature rows,
 * in fp64.  Where siggan_select_topk (siggan_select.h) ranks a generated pool by one score -- and so lets near-duplicates
 * through together --, this call chooses the n_select rows that are mutually farthest apart: every pick is the eligible row
 * farthest from everything picked so far (and, optionally, from a set of anchors the caller has measured the distances to).
 * The rows this package feeds it are the Siamese verifier's embeddings of the pool; the eligibility mask carries the
 * realism and memorisation tests; siggan_gather_u8 then fetches the picked images.
 *
 * The call is context-free, like siggan_select.h: `device` is the HIP ordinal the pointers belong to.  Conventions are those
 * of siggan.h: plain pointers and sizes, the call enqueues on `stream` and never synchronises the host, it does not allocate
 * (the caller owns the workspace), 0 = OK / negative = SIGGAN_E_* with the message in siggan_last_error(), the caller's
 * current device is restored.  Adding this header did not change SIGGAN_ABI_VERSION: it only adds symbols.
 *
 * Semantics.  State: m[i] = anchor_d2[i] (+inf without anchors), taken[i] = 0.  For t = 0 .. n_select - 1:
 *   p = the row with the largest m[i] among those with eligible[i] && !taken[i]; equal values go to the lowest row number
 *       (+inf equals +inf).  If t == 0 and first >= 0, p = first instead, taken as given: neither the mask nor min_gain2
 *       applies to it.
 *   Stop (never for a forced first) when there is no such row or m[p] < min_gain2.
 *   Otherwise order[t] = p, gain2[t] = m[p] (+inf is a legal value), taken[p] = 1, and for EVERY row i, eligible or not,
 *       m[i] = min(m[i], d2(i, p)).
 * After a stop at t: count = t, order[t ..] = -1, gain2[t ..] = 0.0; without one count = n_select.  min_d2 (when given)
 * receives the final m: every row's squared distance to the nearest pick or anchor.  Picked rows are excluded by flag, not
 * by value: a duplicate of a picked row has m = 0 and is still pickable when min_gain2 == 0.
 *
 * Arithmetic: d2(i, p) = sum_k (x_ik - x_pk)^2 in fp64 over the widened fp32 values, formed as differences (not as norms
 * minus a dot product), so identical rows give exactly 0.0 and a near-duplicate keeps its relative accuracy.  Summation
 * order, fixed: lane l of a 64-lane wave adds the squares of the features k = l, l + 64, l + 128, ... in ascending k, starting
 * from 0.0; the 64 lane sums are then folded by a butterfly, s = s + s(lane ^ o) for o = 32, 16, 8, 4, 2, 1.  No fused
 * multiply-add (the library is built with -ffp-contract=off).  Every value is within (dim + 2) * 2^-53 * d2 of the exact sum.
 *
 * Determinism: no atomics; every maximum is taken under the total order (larger m first, then lower row), so the order of a
 * merge cannot show.  Equal input gives bit-equal order, gain2, count and min_d2.
 *
 * Shape of the work: one plain launch per pick, enqueued blindly by the host (n_select + 2 launches in all), no grid-wide
 * barrier, no cooperative launch, no workgroup ever waits for another.  A workgroup of four waves owns
 * SIGGAN_DIVERSE_ROW_TILE consecutive rows.  Launch t: every workgroup folds the per-workgroup (max m, row) partials the
 * previous launch left into the pick p (workgroup 0 also records order[t] and gain2[t]), stages row p in LDS, updates m for
 * its own rows -- one wave per row, lanes across features --, and writes its new partial.  The partials live in two buffers
 * used alternately, because a fast workgroup writes its new partial while a slow one still reads the old ones.  A stop is
 * passed on through the partials themselves (a marker every workgroup copies forward), so every later launch returns after
 * one load.  A last small launch writes the tail, the count and min_d2.
 */
#ifndef SIGGAN_DIVERSE_H
#define SIGGAN_DIVERSE_H

#include <stddef.h>

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_DIVERSE_MAX_N    65536      /* = SIGGAN_SELECT_MAX */
#define SIGGAN_DIVERSE_MAX_DIM  1024       /* = SIGGAN_KNN_MAX_DIM */
#define SIGGAN_DIVERSE_ROW_TILE 32         /* rows per workgroup: eight per wave */

/* Bytes of workspace a selection among n rows needs; 0 for an n outside [1, SIGGAN_DIVERSE_MAX_N].  Needs no device. */
size_t siggan_select_diverse_workspace(int32_t n);

/* x_dev (n, dim) fp32 rows; eligible_dev (n) uint8 0 / 1, or NULL: every row is eligible; anchor_d2_dev (n) fp64 >= 0, or
 * NULL: +inf everywhere; first: -1, or the row taken as pick 0 as it is; order_dev (n_select) int32, gain2_dev (n_select)
 * fp64, count_dev (1) int32; min_d2_dev (n) fp64 or NULL; workspace_dev: 8-byte aligned, at least
 * siggan_select_diverse_workspace(n) bytes, its content on entry does not matter.
 * SIGGAN_E_INVALID with nothing launched: n outside [1, SIGGAN_DIVERSE_MAX_N], dim outside [1, SIGGAN_DIVERSE_MAX_DIM],
 * n_select outside [1, n], first outside [-1, n), min_gain2 negative or NaN, a NULL x_dev, order_dev, gain2_dev, count_dev or
 * workspace_dev, a workspace that is too small or not 8-byte aligned.  NaN / Inf in x are not part of the contract. */
int siggan_select_diverse(int32_t device, const float *x_dev, int32_t n, int32_t dim, const uint8_t *eligible_dev,
                          const double *anchor_d2_dev, int32_t first, int32_t n_select, double min_gain2, int32_t *order_dev,
                          double *gain2_dev, int32_t *count_dev, double *min_d2_dev, void *workspace_dev, size_t workspace_bytes,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_DIVERSE_H */
