/*
 * siggan_verifier_pairs.h -- C ABI of the Siamese signature verifier's all-pairs scoring on the MI355X: the pair head of
 * siggan_verifier.h (|e1 - e2| -> Linear(E,64) + ReLU -> Linear(64,1) -> sigmoid) over EVERY (query, reference) pair of two
 * sets of embeddings, as one GEMM on v_mfma_f32_32x32x2_f32 whose A operand is formed on load, on a siggan_verifier context
 * (create / bind / destroy are that header's).  A test directory's pair population is finite and known: N signatures give
 * N (N - 1) / 2 pairs, and the standard protocol scores all of them.  The (nq, nr) score matrix is formed only when it is asked
 * for: per-class histograms over a threshold grid (from which FAR / FRR / ROC / EER follow exactly at the grid's values) and each
 * query row's best genuine and best impostor match come from the same pass over the score tiles.
 *
 * score[i][j] is bit for bit siggan_verifier_compare on the pair (q_i, r_j).
 *
 * Conventions are those of siggan_verifier.h.  Adding this header did not change SIGGAN_ABI_VERSION: it only adds symbols.
 */
#ifndef SIGGAN_VERIFIER_PAIRS_H
#define SIGGAN_VERIFIER_PAIRS_H

#include "siggan_verifier.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_PAIR_MAX_DIM 1024          /* embedding_dim above this is refused here (the context itself allows more) */
#define SIGGAN_PAIR_MAX_THRESHOLDS 4096

/* Optional outputs; at least one group must be requested.  A group is requested when any of its pointers is non-null (the
 * counts also when n_thresholds != 0), and then needs all of the pointers this comment calls required.
 *   score_dev            (nq, nr) fp32, always the full matrix whatever same_set says.
 *   threshold_dev        T = n_thresholds ascending fp32 values, 1 <= T <= SIGGAN_PAIR_MAX_THRESHOLDS (required for the counts).
 *                        ASCENDING IS THE CALLER'S CONTRACT: it cannot be checked without a host synchronisation.
 *   genuine_count_dev, impostor_count_dev   (T + 1) int64 each, both required: bin b counts the pairs with
 *                        t[b-1] <= s < t[b] (t[-1] = -inf, t[T] = +inf), compared on the fp32 score exactly as score_dev
 *                        stores it, so #{s >= t_k} = sum of bins k+1 .. T is exact.  A pair is genuine when
 *                        q_id[i] == r_id[j]; with either id array NULL every pair is an impostor pair.  With same_set the
 *                        counts cover j > i only (each unordered pair once).
 *   best_genuine_dev / best_genuine_index_dev, best_impostor_dev / best_impostor_index_dev   (nq) fp32 / int32, each optional:
 *                        per query row the maximum score over its genuine / impostor candidates and that candidate's row in
 *                        r; equal scores resolve to the lower row; j == i is no candidate with same_set; a row without a
 *                        candidate of a class gets -1.0f and -1. */
typedef struct siggan_pair_outputs {
    float *score_dev;
    const float *threshold_dev;
    int32_t n_thresholds;
    int64_t *genuine_count_dev, *impostor_count_dev;
    float *best_genuine_dev;
    int32_t *best_genuine_index_dev;
    float *best_impostor_dev;
    int32_t *best_impostor_index_dev;
} siggan_pair_outputs;

/* Allocates, once, the repacked copy of classifier.0.weight (64 x E rounded up to 32, in the MFMA B operand's lane order;
 * every later bind refreshes it) and the row-maxima workspace for up to max_queries query rows (512 bytes per row).  A set-up
 * call: it may synchronise the device.  Calling it again with a max_queries that fits is a no-op; a larger one reallocates.
 * SIGGAN_E_ARG: embedding_dim above SIGGAN_PAIR_MAX_DIM, max_queries < 1. */
int siggan_verifier_pairs_enable(siggan_verifier *v, int32_t max_queries);

/* Scores every pair (q_i, r_j).  Launches: one memset per count array, the tile kernel, and one merge kernel when row maxima
 * are requested; nothing is allocated, the host is never synchronised, and the call can be captured.  Integer counters are the
 * only atomics; the row maxima are merged in a fixed order: equal inputs give equal bits from run to run.
 * same_set != 0: q and r are the same rows (nq == nr is required; the caller passes the same embeddings and ids): counts cover
 * j > i, row maxima skip j == i, and when only the counts are requested the tiles wholly on or below the diagonal are not
 * computed at all.
 * SIGGAN_E_ARG, nothing enqueued: a call before bind or before enable, embedding_dim > SIGGAN_PAIR_MAX_DIM, a null embedding
 * pointer or `out`, nq or nr < 1, nq * nr >= 2^62, same_set with nq != nr, no output requested, a partly given counts group,
 * n_thresholds outside [1, 4096], row maxima with nq > max_queries, an embedding pointer that is not 16-byte aligned when
 * embedding_dim is a multiple of 4 (the rows are then loaded four floats at a time), an output pointer not aligned to its type.
 * NaN / Inf embeddings are not part of the contract. */
int siggan_verifier_pairs(siggan_verifier *v,
        const float *q_emb_dev, const int32_t *q_id_dev, int32_t nq,   /* (nq,E), (nq) or NULL */
        const float *r_emb_dev, const int32_t *r_id_dev, int32_t nr,   /* (nr,E), (nr) or NULL */
        int32_t same_set, const siggan_pair_outputs *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_VERIFIER_PAIRS_H */
