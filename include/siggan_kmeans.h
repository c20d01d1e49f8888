/*
 * siggan_kmeans.h -- C ABI of k-means on fp32 feature rows that stay on the MI355X: k-means++ seeding (D^2 sampling) and
 * Lloyd passes, in fp64.  What the number of statistically different bins (NDB, Richardson & Weiss 2018) is made of: the
 * real set is clustered into k bins, every generated row goes to its nearest bin, and the host compares the two histograms.
 * The assignment is siggan_knn (siggan_neighbors.h) with k = 1; the row-difference distance of the seeding is
 * siggan_select_diverse's (siggan_diverse.h); this header adds the seeding and the centre update.
 *
 * The calls are context-free, like siggan_neighbors.h and siggan_diverse.h: `device` is the HIP ordinal the pointers belong
 * to.  Conventions are those of siggan.h: plain pointers and sizes, every call enqueues on `stream` and never synchronises
 * the host, no call allocates (the caller owns the workspace), 0 = OK / negative = SIGGAN_E_* with the message in
 * siggan_last_error(), the caller's current device is restored.  No atomics on global memory.  Adding this header did not
 * change SIGGAN_ABI_VERSION: it only adds symbols.
 *
 * The two-level sum.  Seeding, inertia and the prefix all use ONE sum of n fp64 values v[0 .. n):
 *   rows are taken in blocks of SIGGAN_KMEANS_SUM_BLOCK = 64 consecutive rows;
 *   within block b:  S_b = ((0.0 + v[64 b]) + v[64 b + 1]) + ..., ascending (the last block stops at n);
 *   across blocks:   Q_b = Q_(b-1) + S_b, ascending, Q_(-1) = 0.0; the total is the last Q_b;
 *   the prefix at row i of block b is Q_(b-1) + r_i, r_i the running sum inside block b up to and including row i, formed in
 *   the same ascending order from 0.0 (so the prefix at a block's last row is Q_b, and prefixes of values >= 0 never decrease).
 * No fused multiply-add anywhere (the library is built with -ffp-contract=off).
 *
 * siggan_kmeans_seed.  The random word of step s is draw_raw(seed, ctr = s, idx = 0, SIGGAN_KMEANS_STREAM) of csrc/rng.h
 * (Philox4x32-10), w; the uniform is u_s = ((w.x >> 5) * 2^26 + (w.y >> 6)) * 2^-53, a double in [0, 1).
 *   Step 0: row_0 = min(n - 1, (int)floor(u_0 * n)); m[i] = +inf.
 *   Step s >= 1: for every row i, m[i] = min(m[i], d2(i, row_(s-1))), d2 in siggan_diverse.h's form and order (differences
 *     of the widened fp32 values; lane l takes the features l, l + 64, ... ascending; then the xor butterfly 32 .. 1), so a
 *     chosen row -- and every copy of it -- gets exactly 0.0 and carries no weight.  T = the two-level sum of m,
 *     target = u_s * T (one fp64 multiply).  row_s = the first row whose prefix is > target.  If no prefix exceeds target
 *     (possible only through the rounding of u_s * T), row_s = the last row with m > 0.  If T == 0.0 every row coincides with
 *     a chosen one; row_s is then the lowest row number not chosen so far.
 *   centres[s] is a bit copy of x[row_s]; seed_rows[s] = row_s.
 * Shape of the work: one single-workgroup launch for step 0 and two plain launches per later step, enqueued blindly
 * (2 k - 1 in all): one workgroup per 64-row block updates m and writes S_b, reading the previous pick from centres[s - 1];
 * one workgroup folds the S_b, draws, locates the row and copies it.  Ordering comes from the stream.
 *
 * siggan_kmeans_lloyd.  For t = 0 .. iterations:
 *   Assign: label[i] = the nearest centre, equal distances to the lower centre; mind2[i] = its squared distance.  Both are
 *     bit for bit what siggan_knn(x, centres, k = 1) writes: the launcher enqueues that very kernel.
 *   changed[t] = #{i : label[i] differs from pass t - 1's}; before pass 0 every label counts as -1, so changed[0] = n.
 *   inertia[t] = the two-level sum of mind2.  count[j] = #{i : label[i] == j}.
 *   Update (not after the last assignment, t == iterations): for every centre j with count[j] > 0 and every feature f,
 *     sum = ((0.0 + x[i1][f]) + x[i2][f]) + ... over the rows of label j in ASCENDING ROW NUMBER, in fp64 on the widened
 *     values; centre[j][f] = (float)(sum / (double)count[j]), IEEE division and round-to-nearest conversion.  A centre
 *     with count 0 keeps its bits.
 * With iterations = 0 the call is a pure assignment that leaves the centres untouched: how a second set is put into
 * existing bins.  Consequences: the returned labels, distances and counts belong to the returned centres; once
 * changed[t] == 0 every later pass leaves every output bit as it is; equal input gives equal bits.
 * Shape of the work: four plain launches per pass.  The update gives one workgroup a (centre, slab of
 * SIGGAN_KMEANS_FEATURE_SLAB features) pair: threads across features, so a row is one coalesced read; the workgroup walks
 * the label array in 64-row steps with a ballot.  A centre's sum is strictly sequential in its rows.
 *
 * NaN / Inf in x are not part of the contract.
 */
#ifndef SIGGAN_KMEANS_H
#define SIGGAN_KMEANS_H

#include <stddef.h>

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_KMEANS_MAX_N 65536          /* = SIGGAN_DIVERSE_MAX_N */
#define SIGGAN_KMEANS_MAX_DIM 1024         /* = SIGGAN_KNN_MAX_DIM */
#define SIGGAN_KMEANS_MAX_K 256
#define SIGGAN_KMEANS_MAX_ITERATIONS 1000
#define SIGGAN_KMEANS_SUM_BLOCK 64         /* rows per block of the two-level sum */
#define SIGGAN_KMEANS_FEATURE_SLAB 256     /* features per workgroup of the centre update */
#define SIGGAN_KMEANS_STREAM 0x4B4D5050u   /* "KMPP": the seeding's random stream ("Random streams") */

/* Bytes of workspace either call below needs; 0 for n outside [1, SIGGAN_KMEANS_MAX_N], dim outside
 * [1, SIGGAN_KMEANS_MAX_DIM] or k outside [1, min(n, SIGGAN_KMEANS_MAX_K)].  A multiple of 8.  Needs no device. */
size_t siggan_kmeans_workspace(int32_t n, int32_t dim, int32_t k);

/* x_dev (n, dim) fp32 rows; centres_dev (k, dim) fp32 and seed_rows_dev (k) int32: outputs; workspace_dev: 8-byte aligned,
 * at least siggan_kmeans_workspace(n, dim, k) bytes, its content on entry does not matter.
 * SIGGAN_E_INVALID with nothing launched: sizes outside the limits above (k > n among them), a NULL x_dev, centres_dev,
 * seed_rows_dev or workspace_dev, a workspace that is too small or not 8-byte aligned. */
int siggan_kmeans_seed(int32_t device, const float *x_dev, int32_t n, int32_t dim, int32_t k, uint64_t seed, float *centres_dev,
                       int32_t *seed_rows_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* x_dev (n, dim) fp32 rows; centres_dev (k, dim) fp32, in and out; label_dev (n) int32; mind2_dev (n) fp64 or NULL;
 * count_dev (k) int32; inertia_dev (iterations + 1) fp64; changed_dev (iterations + 1) int32; workspace_dev as above.
 * SIGGAN_E_INVALID with nothing launched: sizes outside the limits above (k > n among them), iterations outside
 * [0, SIGGAN_KMEANS_MAX_ITERATIONS], a NULL pointer other than mind2_dev, a workspace that is too small or not 8-byte
 * aligned. */
int siggan_kmeans_lloyd(int32_t device, const float *x_dev, int32_t n, int32_t dim, float *centres_dev, int32_t k, int32_t iterations,
                        int32_t *label_dev, double *mind2_dev, int32_t *count_dev, double *inertia_dev, int32_t *changed_dev,
                        void *workspace_dev, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_KMEANS_H */
