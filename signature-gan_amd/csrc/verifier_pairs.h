// verifier_pairs.h -- device parts of siggan_verifier_pairs (include/siggan_verifier_pairs.h): the verifier's pair head over every
// (query, reference) pair as a GEMM on v_mfma_f32_32x32x2_f32 whose A operand |q_i - r_j| is formed on load, with the score
// matrix, the per-class threshold histograms and the per-row best matches taken from the score tiles in one pass.
//
// Block = 256 threads = 4 waves over a PQ (16 queries) x PR (32 references) tile; wave w owns queries 4w .. 4w+3, each against
// the tile's 32 references: the GEMM's M rows are the 32 references of ONE query, its N columns the 64 hidden units (two 32-wide
// accumulators that share the A operand), K = E in steps of 2.  Eight accumulators per wave.  K is walked in chunks of PBK = 32
// staged in LDS: the reference rows k-major (lane li reads reference li), the query rows k-major (one b128 broadcast read gives a
// wave its four queries), and classifier.0.weight from a pack that already has the B operand's lane order, zero-padded to a
// multiple of PBK -- a zero term leaves an fmaf chain's bits alone, so E need not be a multiple of anything.
//
// Bits: the accumulator of hidden unit j is fmaf(|q[k] - r[k]|, w0[j][k], acc) from 0 with k ascending -- head_score's loop.  The
// epilogue is head_hidden / head_sigmoid of verifier_parts.h, and the sum over the 64 hidden units is wave_sum's tree: level
// "xor 32" is one add between the two accumulators, levels 16 .. 1 are cross-lane adds inside a 32-lane half.  Those levels are
// done on all 16 accumulator registers at once by halving: at level "xor m" a lane keeps the half of its registers its own bit
// m selects and adds the partner's copy of the same registers, so five levels cost 8 + 4 + 2 + 1 + 1 exchanges instead of 80, and
// each lane ends with ONE pair's logit (lanes li and li ^ 1 hold the same one): row (li >> 1) of the register order.
//
// Grid (ceil(nq / 16), S): block (x, y) walks the reference tiles of split y.  S > 1 only when nq is too small to fill the
// device; every (row, split) has its own slot for the row maxima and k_vpairs_best merges the slots in split order.
//
// LIST (siggan_verifier_pairs_topk, include/siggan_verifier_topk.h): instead of one maximum per (query, class) the wave keeps the k
// best keys, k <= 16, distributed over its lanes 0 .. k-1 in descending order -- the same eight 64-bit registers per lane the row
// maxima use.  A tile's 32 candidates of one query all sit in the writer lanes of the wave that owns the query: the lanes whose
// key beats the current k-th entry are balloted and inserted one at a time (one ballot-popcount for the position, one shfl_up
// for the shift); after the first tiles that ballot is almost always empty.  Keys are unique (the row is in the key), so the list
// is the exact top k of the total order whatever the insertion order, the split count or the grid.  Every (row, split, class)
// writes its k keys to its own slot and k_vpairs_topk_merge takes the S k <= 512 keys of a (row, class) into one wave.
#pragma once
#include "verifier_parts.h"

namespace {

constexpr int PQ = 16, PR = 32, PBK = 32;
constexpr int PSPLIT_MAX = 32;          // most splits of the reference range; the key workspace holds this many slots per row
constexpr uint32_t PKEY_IDX = 0xFFFFFFFFu;

// classifier.0.weight (64, E) -> [s][t][lh][li] = w0[32 t + li][2 s + lh], s < Kp / 2, zeros for k >= E: lane (li, lh) of a wave
// reads its B operand of k-step s, hidden tile t, at s * 128 + t * 64 + lh * 32 + li -- consecutive lanes, consecutive words.
__global__ void k_vpairs_pack(const float* __restrict__ w0, int E, int Kp, float* __restrict__ pk) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Kp * VHID) return;
    const int li = i & 31, lh = (i >> 5) & 1, t = (i >> 6) & 1, s = i >> 7;
    const int k = 2 * s + lh;
    pk[i] = k < E ? w0[(size_t)(32 * t + li) * E + k] : 0.f;
}

// four consecutive k of one embedding row; zeros outside the row set or past E.  VEC: E % 4 == 0 and a 16-byte aligned base.
template <bool VEC>
__device__ __forceinline__ f32x4 pair_load4(const float* __restrict__ base, int64_t row, int E, int k, bool valid) {
    f32x4 v{0.f, 0.f, 0.f, 0.f};
    if (!valid || k >= E) return v;
    const float* p = base + (size_t)row * E + k;
    if (VEC) return *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (k + e < E) v[e] = p[e];
    return v;
}

// (score, candidate row) as one integer whose order is "higher score, then lower row": scores are in [0, 1], where the fp32
// bit pattern is monotone.  0 = no candidate.
__device__ __forceinline__ unsigned long long pair_key(float s, int j) {
    return ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(PKEY_IDX - (uint32_t)j);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}
// pair_key with the order of the scores reversed: "lower score, then lower row"; never 0 for a score in [0, 1]
__device__ __forceinline__ unsigned long long pair_key_low(float s, int j) {
    return ((unsigned long long)(~__float_as_uint(s)) << 32) | (unsigned long long)(PKEY_IDX - (uint32_t)j);
}
// One list per wave: lane l < k holds the l-th largest key seen so far (0 = empty), lanes >= k hold 0.  Inserts every lane's
// `cand` (0 = none) that belongs to the k largest; all 64 lanes must be active.  The loop is wave-uniform.
__device__ __forceinline__ void pair_list_insert(unsigned long long& list, unsigned long long cand, int k, int lane) {
    const unsigned long long kth = __shfl(list, k - 1, 64);
    unsigned long long m = __ballot(cand > kth);
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const unsigned long long c = __shfl(cand, src, 64);
        const int pos = __popcll(__ballot(lane < k && list > c));       // the list descends: exactly lanes 0 .. pos-1 stay
        const unsigned long long up = __shfl_up(list, 1, 64);
        if (lane < k && lane >= pos) list = lane == pos ? c : up;       // pos == k (the list moved on since the ballot): nothing
    }
}

struct PairOut {
    float* score;                        // (nq, nr) or null
    const float* thr;                    // T ascending thresholds or null
    int T;
    unsigned long long *gcnt, *icnt;     // T + 1 bins each (zeroed before the launch) or null
    unsigned long long* keys;            // [nq][S][2] or null; LIST: [nq][S][2][list_k]
    int list_k, list_flags;              // LIST only: k; bit 0 / 1: the genuine / impostor list is wanted, bit 2: genuine lowest
};

// dynamic LDS: T thresholds, then 2 (T + 1) counters (nothing when the counts are not asked for).  Two workgroups per CU (two
// waves per SIMD: 256 registers, a few spilled in the epilogue): the second hides the first one's barriers, chunk-opening LDS
// reads and epilogue -- measured 18 % faster at 16384^2 than the 374-register build that runs one wave per SIMD.
// LIST: the k best per (query, class) instead of the maximum (file comment); the same budget -- the lists live in best[][].
template <bool VEC, int LIST = 0>
__global__ __launch_bounds__(256, 2) void k_vpairs(const float* __restrict__ q, const int32_t* __restrict__ qid, int nq,
                                                const float* __restrict__ r, const int32_t* __restrict__ rid, int nr, int E, int Kp,
                                                const float* __restrict__ wpk, const float* __restrict__ b0,
                                                const float* __restrict__ w3, const float* __restrict__ b3, int same, int upper_only,
                                                int tiles_per_split, PairOut o) {
    extern __shared__ uint32_t dyn[];
    __shared__ __attribute__((aligned(16))) float sW[PBK * VHID];
    __shared__ __attribute__((aligned(16))) float sR[PBK * PR];
    __shared__ __attribute__((aligned(16))) float sQ[PBK * PQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int T = o.thr ? o.T : 0;
    float* sthr = reinterpret_cast<float*>(dyn);
    uint32_t* hist = dyn + T;
    if (T) {
        for (int i = tid; i < T; i += 256) sthr[i] = o.thr[i];
        for (int i = tid; i < 2 * (T + 1); i += 256) hist[i] = 0u;
    }
    __syncthreads();

    const int64_t i0 = (int64_t)blockIdx.x * PQ;
    const int split = blockIdx.y, S = gridDim.y;
    const int ntiles = (nr + PR - 1) / PR;
    int jt = split * tiles_per_split;
    const int jt_end = min(jt + tiles_per_split, ntiles);
    // same_set counts alone: tile jt holds a pair with j > i only when 32 jt + 31 > i0, i.e. jt >= i0 / 32
    if (upper_only) jt = max(jt, (int)(i0 / PR));

    const float b0a = b0[li], b0b = b0[32 + li], w3a = w3[li], w3b = w3[32 + li], b3v = b3[0];
    const bool has_ids = qid && rid;
    // staging roles
    const int rrow = tid & 31, rk = (tid >> 5) * 4;              // references: 32 rows x 8 groups of 4 k
    const int qrow = tid & 15, qk = ((tid >> 4) & 7) * 4;        // queries: 16 rows x 8 groups (threads 0 .. 127)
    const bool qvalid = tid < 128 && i0 + qrow < nq;
    // the pair this lane ends up with in every 32-pair epilogue, and the wave's four queries
    const int rr = li >> 1, jl = (rr & 3) + 8 * (rr >> 2) + 4 * lh;
    const bool writer = !(li & 1);
    int32_t myqid[4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
        const int64_t i = i0 + 4 * wave + qq;
        myqid[qq] = (has_ids && i < nq) ? qid[i] : 0;
    }
    unsigned long long best[4][2];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) best[qq][0] = best[qq][1] = 0ull;

    for (; jt < jt_end; ++jt) {
        const int64_t j0 = (int64_t)jt * PR;
        const bool rvalid = j0 + rrow < nr;
        f32x16 acc[4][2];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int x = 0; x < 16; ++x) acc[qq][t][x] = 0.f;
        f32x4 fw[2], fr, fq;
        auto fetch = [&](int k0) {
#pragma unroll
            for (int u = 0; u < 2; ++u) fw[u] = *reinterpret_cast<const f32x4*>(wpk + (size_t)k0 * VHID + (tid + 256 * u) * 4);
            fr = pair_load4<VEC>(r, j0 + rrow, E, k0 + rk, rvalid);
            fq = pair_load4<VEC>(q, i0 + qrow, E, k0 + qk, qvalid);
        };
        fetch(0);
        for (int k0 = 0; k0 < Kp; k0 += PBK) {
#pragma unroll
            for (int u = 0; u < 2; ++u) *reinterpret_cast<f32x4*>(&sW[(tid + 256 * u) * 4]) = fw[u];
#pragma unroll
            for (int e = 0; e < 4; ++e) sR[(rk + e) * PR + rrow] = fr[e];
            if (tid < 128) {
#pragma unroll
                for (int e = 0; e < 4; ++e) sQ[(qk + e) * PQ + qrow] = fq[e];
            }
            __syncthreads();
            if (k0 + PBK < Kp) fetch(k0 + PBK);
#pragma unroll
            for (int s = 0; s < PBK / 2; ++s) {
                const int k = 2 * s + lh;
                const float rv = sR[k * PR + li];
                const f32x4 q4 = *reinterpret_cast<const f32x4*>(&sQ[k * PQ + 4 * wave]);
                const float wa = sW[s * 128 + lh * 32 + li], wb = sW[s * 128 + 64 + lh * 32 + li];
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) {
                    const float a = fabsf(q4[qq] - rv);
                    acc[qq][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wa, acc[qq][0], 0, 0, 0);
                    acc[qq][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wb, acc[qq][1], 0, 0, 0);
                }
            }
            __syncthreads();
        }

        const int64_t j = j0 + jl;
        const int32_t myrid = (has_ids && j < nr) ? rid[j] : 0;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            // wave_sum's tree over the 64 hidden units, for the 16 pairs of this lane's half at once
            float t16[16];
#pragma unroll
            for (int x = 0; x < 16; ++x)
                t16[x] = head_hidden(acc[qq][0][x], b0a) * w3a + head_hidden(acc[qq][1][x], b0b) * w3b;      // xor 32
            float t8[8], t4[4], t2[2];
            const bool h16 = li & 16, h8 = li & 8, h4 = li & 4, h2 = li & 2;
#pragma unroll
            for (int x = 0; x < 8; ++x) t8[x] = (h16 ? t16[8 + x] : t16[x]) + __shfl_xor(h16 ? t16[x] : t16[8 + x], 16, 64);
#pragma unroll
            for (int x = 0; x < 4; ++x) t4[x] = (h8 ? t8[4 + x] : t8[x]) + __shfl_xor(h8 ? t8[x] : t8[4 + x], 8, 64);
#pragma unroll
            for (int x = 0; x < 2; ++x) t2[x] = (h4 ? t4[2 + x] : t4[x]) + __shfl_xor(h4 ? t4[x] : t4[2 + x], 4, 64);
            float t1 = (h2 ? t2[1] : t2[0]) + __shfl_xor(h2 ? t2[0] : t2[1], 2, 64);
            t1 += __shfl_xor(t1, 1, 64);
            const float sc = head_sigmoid(t1, b3v);

            const int64_t i = i0 + 4 * wave + qq;
            const bool live = writer && i < nq && j < nr;
            const bool genuine = has_ids && myqid[qq] == myrid;
            if (o.score && live) o.score[(size_t)i * nr + j] = sc;
            if (T && live && (!same || j > i)) {
                int lo = 0, hi = T;                                   // #{k : thr[k] <= sc}
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sthr[mid] <= sc) lo = mid + 1; else hi = mid;
                }
                atomicAdd(&hist[(genuine ? 0 : T + 1) + lo], 1u);
            }
            if constexpr (LIST) {
                const bool cand = live && !(same && j == i);
                if (o.list_flags & 1) {
                    const unsigned long long key = (o.list_flags & 4) ? pair_key_low(sc, (int)j) : pair_key(sc, (int)j);
                    pair_list_insert(best[qq][0], cand && genuine ? key : 0ull, o.list_k, lane);
                }
                if (o.list_flags & 2) pair_list_insert(best[qq][1], cand && !genuine ? pair_key(sc, (int)j) : 0ull, o.list_k, lane);
            } else
            if (o.keys && live && !(same && j == i)) {
                const unsigned long long key = pair_key(sc, (int)j);
                const unsigned long long kg = genuine ? key : 0ull, ki = genuine ? 0ull : key;
                best[qq][0] = kg > best[qq][0] ? kg : best[qq][0];
                best[qq][1] = ki > best[qq][1] ? ki : best[qq][1];
            }
        }
    }

    if constexpr (LIST) {
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int64_t i = i0 + 4 * wave + qq;
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if (lane < o.list_k && i < nq) o.keys[(((size_t)i * S + split) * 2 + c) * o.list_k + lane] = best[qq][c];
        }
    } else
    if (o.keys) {
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int64_t i = i0 + 4 * wave + qq;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const unsigned long long m = wave_max_u64(best[qq][c]);
                if (lane == 0 && i < nq) o.keys[((size_t)i * S + split) * 2 + c] = m;
            }
        }
    }
    if (T) {
        __syncthreads();
        for (int b = tid; b < 2 * (T + 1); b += 256) {
            const uint32_t n = hist[b];
            if (n) atomicAdd(b <= T ? &o.gcnt[b] : &o.icnt[b - (T + 1)], (unsigned long long)n);
        }
    }
}

// per query row: the S slots of each class merged in split order, decoded; no candidate -> (-1.0f, -1)
__global__ void k_vpairs_best(const unsigned long long* __restrict__ keys, int nq, int S, float* __restrict__ bg,
                              int32_t* __restrict__ bgi, float* __restrict__ bi, int32_t* __restrict__ bii) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        unsigned long long m = 0ull;
        for (int s = 0; s < S; ++s) {
            const unsigned long long k = keys[((size_t)i * S + s) * 2 + c];
            m = k > m ? k : m;
        }
        const float sc = m ? __uint_as_float((uint32_t)(m >> 32)) : -1.0f;
        const int32_t idx = m ? (int32_t)(PKEY_IDX - (uint32_t)m) : -1;
        float* so = c ? bi : bg;
        int32_t* io = c ? bii : bgi;
        if (so) so[i] = sc;
        if (io) io[i] = idx;
    }
}

// One wave per (query row, class): the S k <= 512 keys of the row's slots, up to eight per lane, and k rounds of "take the wave's
// maximum, clear it where it came from" (keys are unique: a reference row lies in one split).  Decoded as k_vpairs_best does;
// `low`: the genuine keys carry the complemented score bits.  A class without an output pointer is skipped.
__global__ __launch_bounds__(256) void k_vpairs_topk_merge(const unsigned long long* __restrict__ keys, int nq, int S, int k, int low,
                                                         float* __restrict__ gs, int32_t* __restrict__ gi, float* __restrict__ is,
                                                         int32_t* __restrict__ ii) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t i = w >> 1;
    const int c = (int)(w & 1);
    if (i >= nq) return;
    float* so = c ? is : gs;
    int32_t* io = c ? ii : gi;
    if (!so && !io) return;
    const bool flip = low && c == 0;
    const int n = S * k;
    unsigned long long v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int e = lane + 64 * t;                                   // slot e / k, entry e % k
        v[t] = e < n ? keys[(((size_t)i * S + e / k) * 2 + c) * k + e % k] : 0ull;
    }
    for (int p = 0; p < k; ++p) {
        unsigned long long m = v[0];
#pragma unroll
        for (int t = 1; t < 8; ++t) m = v[t] > m ? v[t] : m;
        m = wave_max_u64(m);
        if (m) {
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = v[t] == m ? 0ull : v[t];
        }
        if (lane == 0) {
            const uint32_t hi = (uint32_t)(m >> 32);
            if (so) so[(size_t)i * k + p] = m ? __uint_as_float(flip ? ~hi : hi) : -1.0f;
            if (io) io[(size_t)i * k + p] = m ? (int32_t)(PKEY_IDX - (uint32_t)m) : -1;
        }
    }
}

}  // namespace
