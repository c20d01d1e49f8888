// gconv_parts.h -- the device code the implicit-GEMM kernels of gconv.hip (fp32) and gconv16.hip (bf16 / f16) are built
// from, each part once: the XCD remap, the block setup (GconvBlock), the per-row staging coordinates and tap cursor
// (GconvRows), the KQ = 2 accumulator hand-over, the fused epilogues with their statistics reduction (epi_*), and the
// weight-gradient tail (wgrad_tail).  What the two files keep to themselves is the operand path (LDS tile layout,
// global->LDS staging, fragment reads, the MFMA) and the loop that moves the accumulator tile through LDS to epi_apply.
#pragma once
#include "gconv.h"

namespace siggan {

static constexpr int BK = 32;    // K-tile (elements; restated in tests/evalpaths.py)

// XCD-aware bijective remap (8 XCDs, blocks b and b+8 share an L2): consecutive logical tiles,
// which share an A row-panel, land on one XCD.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// ---- block setup of k_gconv / k_gconv16: tile origin, parity class and split-K range of this workgroup --------------
template <int BM, int BN, int KQ>
struct GconvBlock {
    int quad, tid;               // wave quad (KQ = 2), thread index inside the quad
    int tiles_n, bid, m0, n0, cls, ph, pw, Hr, Wr, Ktot, lgcpt;
    int k_lo, nk;                // this block's (this quad's) K-tiles [k_lo, k_lo + nk)
    __device__ __forceinline__ explicit GconvBlock(const GConvArgs& a) {
        quad = KQ > 1 ? (int)(threadIdx.x >> 8) : 0;
        tid = threadIdx.x & 255;
        tiles_n = a.Co / BN;
        bid = xcd_remap(blockIdx.x, gridDim.x);
        m0 = (bid / tiles_n) * BM; n0 = (bid % tiles_n) * BN;
        cls = blockIdx.z; ph = cls >> 1; pw = cls & 1;
        Hr = 1 << a.lgHr; Wr = 1 << a.lgWr;
        const int ntaps = a.form == 0 ? 16 : 4;
        Ktot = ntaps * a.Ci;
        lgcpt = 31 - __builtin_clz(a.Ci / BK);      // K-tiles per tap = Ci / 32, a power of two
        const int nk_all = ntaps << lgcpt;
        // split-K: this block (this quad of it) owns K-tiles [k_lo, k_hi); with KQ = 2 the launcher guarantees equal halves,
        // so both quads pass the same number of barriers
        const int kper = (nk_all + gridDim.y * KQ - 1) / (gridDim.y * KQ);
        k_lo = (blockIdx.y * KQ + quad) * kper;
        nk = min(nk_all, k_lo + kper) - k_lo;
    }
};

// Per-row staging coordinates and the load cursor of the A operand.  A thread stages the 16-byte chunk kc (EPC elements)
// of the K-tile rows `row(p)`, p < PA; T = operand element type.
template <class T, int PA>
struct GconvRows {
    const T* base[PA];           // &in[n, 0, 0, kc * EPC] of the row's image
    int ih0[PA], iw0[PA];
    // load cursor: walks (tap, channel chunk) in K order; per-row source pointers are rebuilt only
    // when the tap changes, otherwise they advance by a K-tile (0 for out-of-image taps, which
    // read a 16-byte page of zeros so that the loads stay unconditional)
    const T* cur[PA];
    int step[PA];
};
template <class T, int PA, class Blk>
__device__ __forceinline__ void gconv_row(const GConvArgs& a, const Blk& b, GconvRows<T, PA>& r, int p, int m, int koff) {
    const T* const in = static_cast<const T*>(a.in);
    if (m < a.M) {
        const int n = m >> (a.lgHr + a.lgWr);
        const int rh = (m >> a.lgWr) & (b.Hr - 1), rw = m & (b.Wr - 1);
        r.base[p] = in + (size_t)n * a.Hi * a.Wi * a.Ci + koff;
        if (a.form == 0) { r.ih0[p] = 2 * rh - 1; r.iw0[p] = 2 * rw - 1; }
        else             { r.ih0[p] = rh + b.ph;  r.iw0[p] = rw + b.pw; }
    } else {
        r.base[p] = in; r.ih0[p] = -(1 << 20); r.iw0[p] = -(1 << 20);
    }
}
template <class T, int PA>
__device__ __forceinline__ void gconv_set_tap(const GConvArgs& a, GconvRows<T, PA>& r, int l_tap, int l_cc) {
    int dh, dw;
    if (a.form == 0) { dh = l_tap >> 2; dw = l_tap & 3; } else { dh = -(l_tap >> 1); dw = -(l_tap & 1); }
#pragma unroll
    for (int p = 0; p < PA; ++p) {
        const int ih = r.ih0[p] + dh, iw = r.iw0[p] + dw;
        const bool ok = (unsigned)ih < (unsigned)a.Hi && (unsigned)iw < (unsigned)a.Wi;
        r.cur[p] = ok ? r.base[p] + ((size_t)(ih * a.Wi + iw) * a.Ci + l_cc * BK) : reinterpret_cast<const T*>(a.zeros);
        r.step[p] = ok ? BK : 0;
    }
}

// ---- KQ = 2: quad 1's accumulators -> LDS (red: its own staging area) -> added to quad 0's, lane for lane -------------
template <int TM, int TN>
__device__ __forceinline__ void kq_handover(float* red, int quad, int wave, int lane, f32x16 (&acc)[TM][TN]) {
    if (quad == 1) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[(((wave * TM + i) * TN + j) * 16 + r) * 64 + lane] = acc[i][j][r];
    }
    __syncthreads();
    if (quad == 0) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += red[(((wave * TM + i) * TN + j) * 16 + r) * 64 + lane];
    }
}

// ---- the fused epilogues ----------------------------------------------------------------------------------------
// per-channel operands of the epilogue `epi` for the four channels co .. co + 3 (16-byte aligned), and the running
// BatchNorm-backward sums of EPI_BN_BWD_STATS
struct EpiState {
    f32x4 bias, sc, sh;
    BnBwdParams bq;
    bool bias_lrelu, affine, lrelu_bwd, stats, use_noise;      // which epilogue; use_noise: it has dropout multipliers to apply
    f32x4 st0, st1;
};
__device__ __forceinline__ EpiState epi_load(const GConvArgs& a, int epi, int co) {
    EpiState q;
    q.bias_lrelu = epi == EPI_BIAS_LRELU_DROP; q.affine = epi == EPI_AFFINE_RELU; q.lrelu_bwd = epi == EPI_LRELU_BWD;
    q.stats = epi == EPI_BN_BWD_STATS;
    q.bias = q.bias_lrelu ? *reinterpret_cast<const f32x4*>(a.bias + co) : f32x4{0.f, 0.f, 0.f, 0.f};
    q.sc = f32x4{1.f, 1.f, 1.f, 1.f}; q.sh = f32x4{0.f, 0.f, 0.f, 0.f};
    if (q.affine) { q.sc = *reinterpret_cast<const f32x4*>(a.scale + co); q.sh = *reinterpret_cast<const f32x4*>(a.shift + co); }
    q.use_noise = (q.bias_lrelu || q.lrelu_bwd) && a.noise != nullptr;
    if (q.stats) q.bq = bn_bwd_params(a.bnp, a.Co, co);
    q.st0 = f32x4{0.f, 0.f, 0.f, 0.f}; q.st1 = q.st0;
    return q;
}
// the Discriminator's dropout multipliers of image n, applied behind the activation (forward) / its mask (backward)
__device__ __forceinline__ f32x4 epi_dropout(const GConvArgs& a, f32x4 v, int n, int co) {
    const f32x4 nz = *reinterpret_cast<const f32x4*>(a.noise + (size_t)n * a.Co + co);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= nz[e];
    return v;
}
// v = four consecutive channels of the accumulator at output offset o (elements), image n; returns what is stored.
// T = element type of aref.  EPI_BN_BWD_STATS stores v itself and adds its terms to q.st0 / q.st1.
template <class T, bool LK>
__device__ __forceinline__ f32x4 epi_apply(const GConvArgs& a, EpiState& q, f32x4 v, size_t o, int n, int co) {
    if (q.stats) {
        bn_bwd_stat_terms<T, LK>(v, ld4<T>(static_cast<const T*>(a.aref) + o), q.bq, a.gslope, q.st0, q.st1);   // (v as it is stored: rounded to T)
    } else if (q.bias_lrelu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { float t = v[e] + q.bias[e]; v[e] = t > 0.f ? t : t * a.slope; }
        if (q.use_noise) v = epi_dropout(a, v, n, co);
    } else if (q.affine) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = g_act<LK>(fmaf(v[e], q.sc[e], q.sh[e]), a.gslope);
    } else if (q.lrelu_bwd) {
        const f32x4 ar = ld4<T>(static_cast<const T*>(a.aref) + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= ar[e] > 0.f ? 1.f : a.slope;
        if (q.use_noise) v = epi_dropout(a, v, n, co);
    }
    return v;
}
// The column sums of EPI_BN_BWD_STATS: a workgroup's threads hold RPP row lanes (r0 = tid / C4) of C4 channel groups
// (c4 = tid % C4).  The lanes meet in LDS (sh: 256 * 8 floats, free) and lane r0 == 0 adds rows 1 .. RPP-1 in that
// order -- the workgroup's partial row prow of stat0 / stat1, channels co .. co + 3, a fixed sum order.  `active`: this thread
// holds sums.
__device__ __forceinline__ void epi_stats_reduce(const GConvArgs& a, EpiState& q, float* sh, int tid, bool active, int c4, int r0,
                                                 int C4, int RPP, size_t prow, int co) {
    if (active) {
        *reinterpret_cast<f32x4*>(sh + (size_t)tid * 8) = q.st0;
        *reinterpret_cast<f32x4*>(sh + (size_t)tid * 8 + 4) = q.st1;
    }
    __syncthreads();
    if (active && r0 == 0) {
#pragma unroll 4
        for (int k = 1; k < RPP; ++k) {
            q.st0 += *reinterpret_cast<const f32x4*>(sh + (size_t)(k * C4 + c4) * 8);
            q.st1 += *reinterpret_cast<const f32x4*>(sh + (size_t)(k * C4 + c4) * 8 + 4);
        }
        *reinterpret_cast<f32x4*>(a.stat0 + prow * a.Co + co) = q.st0;
        *reinterpret_cast<f32x4*>(a.stat1 + prow * a.Co + co) = q.st1;
    }
}

// ---- k_wgrad / k_wgrad16 behind the K loop (its last barrier has passed: LDS, fsm, is free) -----------------------
// bias column sums (thread t holds the slice kq = t / BM of column t % BM in bsum), then the accumulators: a single
// split un-permutes straight into the torch layout, column j = tap*Cl + l -> dw[(row*Cl + l)*16 + tap]; otherwise the
// split's slab.
template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void wgrad_tail(const WgradArgs& a, float* fsm, bool bias_blk, float bsum, int i0, int j0, int bz,
                                           const f32x16 (&acc)[BM / (32 * WM)][BN / (32 * WN)]) {
    constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN), NQ = 256 / BM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int N = 16 << a.lgCl, Cl = 1 << a.lgCl;
    if (bias_blk) {
        fsm[tid] = bsum;                              // = fsm[kq * BM + column]
        __syncthreads();
        if (tid < BM) {
            float t = fsm[tid];
#pragma unroll
            for (int q = 1; q < NQ; ++q) t += fsm[q * BM + tid];
            if (gridDim.z == 1) a.db[i0 + tid] = t;
            else a.slab[(size_t)gridDim.z * a.Cs * N + (size_t)bz * a.Cs + i0 + tid] = t;
        }
    }
    if (gridDim.z == 1 && a.dw) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i0 + wm * (32 * TM) + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int col = j0 + wn * (32 * TN) + 32 * j + li;
                    a.dw[((size_t)row * Cl + (col & (Cl - 1))) * 16 + (col >> a.lgCl)] = acc[i][j][r];
                }
            }
        return;
    }
    float* const out = a.slab + (size_t)bz * a.Cs * N;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = i0 + wm * (32 * TM) + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
#pragma unroll
            for (int j = 0; j < TN; ++j)
                out[(size_t)row * N + j0 + wn * (32 * TN) + 32 * j + li] = acc[i][j][r];
        }
}

}  // namespace siggan
