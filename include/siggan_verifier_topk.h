/*
 * siggan_verifier_topk.h -- C ABI of per-row top-k lists out of the all-pairs pass of siggan_verifier_pairs.h: for every query
 * row the k highest-scoring impostor candidates and the k lowest- or highest-scoring genuine candidates, each with its score and
 * its row in r, 1 <= k <= SIGGAN_PAIR_TOPK_MAX.  The (nq, nr) matrix is not formed.  What the lists are for: mining the pairs a
 * trained head still gets wrong (the impostors it scores highest, the genuine pairs it scores lowest) without leaving the device.
 *
 * Every score is bit for bit siggan_verifier_pairs' score[i][j] (and so siggan_verifier_compare's).  A list of highest scores is
 * ordered by (score descending, row ascending), a list of lowest scores by (score ascending, row ascending): total orders, so the
 * lists do not depend on the grid, the split of the reference range or the run.  Positions beyond a row's number of candidates
 * hold -1.0f and -1.  With k = 1 the highest lists are siggan_verifier_pairs' row maxima.
 *
 * Conventions are those of siggan_verifier.h.  Adding this header did not change SIGGAN_ABI_VERSION: it only adds symbols.
 */
#ifndef SIGGAN_VERIFIER_TOPK_H
#define SIGGAN_VERIFIER_TOPK_H

#include "siggan_verifier_pairs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_PAIR_TOPK_MAX 16

/* Outputs, each (nq, k) row-major, fp32 scores and int32 rows of r.  A class (impostor, genuine) is computed when either of its
 * pointers is non-null; at least one class must be requested.  A pair is genuine when q_id[i] == r_id[j]; with either id array
 * NULL every pair is an impostor pair.  j == i is no candidate with same_set. */
typedef struct siggan_pair_topk {
    float *impostor_score_dev;
    int32_t *impostor_index_dev;
    float *genuine_score_dev;
    int32_t *genuine_index_dev;
} siggan_pair_topk;

/* Allocates, once, the key slots of the lists: max_queries * 32 * 2 * max_k * 8 bytes.  Needs siggan_verifier_pairs_enable first
 * (the lists are scored with that call's weight pack).  A set-up call: it may synchronise the device.  Calling it again with
 * values that fit is a no-op; a larger max_queries or max_k reallocates.
 * SIGGAN_E_ARG: siggan_verifier_pairs_enable has not been called, max_queries < 1, max_k outside [1, SIGGAN_PAIR_TOPK_MAX]. */
int siggan_verifier_pairs_topk_enable(siggan_verifier *v, int32_t max_queries, int32_t max_k);

/* The lists of every query row.  Launches: the tile kernel and one merge kernel; nothing is allocated, the host is never
 * synchronised, and the call can be captured.  There are no atomics: equal inputs give equal bits from run to run.
 * genuine_lowest != 0: the genuine list holds the k LOWEST scores (the hard genuine pairs); 0: the k highest.  The impostor list
 * always holds the k highest.
 * SIGGAN_E_ARG, nothing enqueued: a call before bind or before either enable, a null embedding pointer or `out`, nq or nr < 1,
 * nq * nr >= 2^62, k outside [1, max_k], nq > max_queries, same_set with nq != nr, no output requested, an embedding pointer
 * that is not 16-byte aligned when embedding_dim is a multiple of 4, an id or output pointer not aligned to its type. */
int siggan_verifier_pairs_topk(siggan_verifier *v,
        const float *q_emb_dev, const int32_t *q_id_dev, int32_t nq,   /* (nq,E), (nq) or NULL */
        const float *r_emb_dev, const int32_t *r_id_dev, int32_t nr,   /* (nr,E), (nr) or NULL */
        int32_t same_set, int32_t k, int32_t genuine_lowest, const siggan_pair_topk *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_VERIFIER_TOPK_H */
