// gconv.hip -- fp32 MFMA implicit-GEMM kernels for the 4x4 / stride-2 / pad-1 convolution family
// of the signature GAN (gfx950 only).
//
//   "down" form : Conv2d forward (discriminator_vanilla_gan.py:51-58) and the input-gradient of
//                 ConvTranspose2d (generator_vanilla_gan.py:46-54)
//   "up"   form : ConvTranspose2d forward and the input-gradient of Conv2d, as four sub-pixel
//                 (output-parity) classes of 2x2 taps each -- no col2im scatter
//   wgrad       : weight gradient of both, split over the pixel (K) axis into partial slabs
//
// GEMM view: C[m][n] = sum_k A[m][k] * Bw[n][k];  m = output pixel (down) / input pixel (up),
// n = output channel, k = (tap, input channel).  One workgroup = 4 waves (256 threads); each wave
// owns TM x TN tiles of 32x32 computed with v_mfma_f32_32x32x2_f32 (exact fp32, 64 FLOP/clk/SIMD).
// LDS tiles are stored k-major ([k][row]) so a fragment read is one conflict-free ds_read_b32 per
// lane (lane l reads row l&31 of k-row 2s + (l>>5)); the fp32 MFMA takes 64 cycles, so LDS and
// VALU have a large budget and the kernels are MFMA-bound once the grid fills the chip.
// Global->LDS staging is register-staged and software-pipelined one K-tile ahead (loads for tile
// t+1 are issued before the MFMAs of tile t, written to the other LDS buffer after them).
//
// Shared with the 16-bit kernels (gconv16.hip) and kept in gconv_parts.h: the XCD remap, the block setup (GconvBlock),
// the per-row staging coordinates and tap cursor (GconvRows), the KQ = 2 accumulator hand-over (kq_handover), the fused
// epilogues and their statistics reduction (epi_load / epi_apply / epi_stats_reduce, also k_splitk_epilogue's) and the
// weight-gradient tail (wgrad_tail).  This file keeps the fp32 operand path -- LDS layouts, staging, fragment reads,
// MFMA -- and the one-pass move of the accumulator tile through LDS.
#include "gconv_parts.h"
#include "host.h"
#include <hip/hip_ext.h>

namespace siggan {

static constexpr int PAD = 4;    // LDS row padding (floats)

// KQ = 2: two wave quads per workgroup, each running the whole pipeline on its own half of the workgroup's K range and its
// own LDS buffers; the second quad's accumulators are added to the first's through LDS before the epilogue.  This is a
// two-way K split WITHOUT slabs or a second kernel (sum order quad 0 + quad 1 = slab 0 + slab 1 of the split-K protocol:
// bit-identical); used for the launches that would otherwise be split in two.
template <int BM, int BN, int WM, int WN, int KQ = 1, bool LK = false>   // LK: g_act's variant
__global__ __launch_bounds__(256 * KQ) void k_gconv(const GConvArgs a) {
    constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
    constexpr int PA = BM / 32, PB = BN / 32;
    // LDS tiles are [row][k] with a row stride of 36 floats (= 4 * odd): a staged float4 is ONE
    // ds_write_b128 (8 lanes cover a row's 128 B), and a lane's MFMA operands for 4 consecutive
    // sub-steps are ONE conflict-free ds_read_b128 (the 16 lanes of a b128 group hit 16 distinct
    // 16-byte slots because rows differ by 9 slots).  K is consumed in the permuted pairing
    // k = 8c + 4*(lane>>5) + t, identical for A and B, so only the fp32 summation order changes.
    constexpr int LD = BK + 4;
    __shared__ __attribute__((aligned(16))) float smem[KQ * 2 * LD * (BM + BN)];
    const GconvBlock<BM, BN, KQ> b(a);
    const int nk = b.nk;
    float* const sA = smem + b.quad * (2 * LD * (BM + BN));
    float* const sB = sA + 2 * LD * BM;

    const int lane = b.tid & 63, wave = b.tid >> 6;      // wave index inside the quad
    const int li = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const float* const a_wp = static_cast<const float*>(a.wp);

    // ---- per-thread staging coordinates: row rloc + 32p, 16-byte chunk kc of the 32-float k-row ------
    const int kc = b.tid & 7, rloc = b.tid >> 3;
    GconvRows<float, PA> rows;
#pragma unroll
    for (int p = 0; p < PA; ++p) gconv_row(a, b, rows, p, b.m0 + rloc + 32 * p, kc * 4);
    const float* wcur = a_wp + ((size_t)b.cls * a.Co + b.n0 + rloc) * b.Ktot + kc * 4 + (size_t)b.k_lo * BK;
    int l_tap = b.k_lo >> b.lgcpt, l_cc = b.k_lo & ((1 << b.lgcpt) - 1);
    auto set_tap = [&]() __attribute__((always_inline)) { gconv_set_tap(a, rows, l_tap, l_cc); };
    f32x4 ra[2][PA], rb[2][PB];          // two register sets: tile t waits in set t & 1 (the short path uses set 0 alone)
    auto load_tile = [&](int set) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < PA; ++p) {
            ra[set][p] = *reinterpret_cast<const f32x4*>(rows.cur[p]);      // (zero page: 256 B)
            rows.cur[p] += rows.step[p];
        }
#pragma unroll
        for (int p = 0; p < PB; ++p) rb[set][p] = *reinterpret_cast<const f32x4*>(wcur + (size_t)(32 * p) * b.Ktot);
        wcur += BK;
        if (++l_cc == (1 << b.lgcpt)) { l_cc = 0; ++l_tap; set_tap(); }
    };
    auto store_tile = [&](int buf, int set) __attribute__((always_inline)) {
        float* dA = sA + buf * LD * BM + rloc * LD + kc * 4;
        float* dB = sB + buf * LD * BN + rloc * LD + kc * 4;
#pragma unroll
        for (int p = 0; p < PA; ++p) *reinterpret_cast<f32x4*>(dA + 32 * p * LD) = ra[set][p];
#pragma unroll
        for (int p = 0; p < PB; ++p) *reinterpret_cast<f32x4*>(dB + 32 * p * LD) = rb[set][p];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // one K-tile out of LDS buffer h; st: the LDS write of the next tile out of register set `sset` rides along behind the
    // first MFMAs, ld: the loads of a later tile into that set behind the second chunk's
    auto tile = [&](const int h, const int sset, const bool st, const bool ld) __attribute__((always_inline)) {
        const float* pA = sA + h * LD * BM + (wm * (32 * TM) + li) * LD + 4 * lh;
        const float* pB = sB + h * LD * BN + (wn * (32 * TN) + li) * LD + 4 * lh;
        f32x4 fa[2][TM], fb[2][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[0][i] = *reinterpret_cast<const f32x4*>(pA + 32 * i * LD);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[0][j] = *reinterpret_cast<const f32x4*>(pB + 32 * j * LD);
#pragma unroll
        for (int c = 0; c < BK / 8; ++c) {
            const int cur = c & 1, nxt = cur ^ 1;
            if (c + 1 < BK / 8) {
#pragma unroll
                for (int i = 0; i < TM; ++i) fa[nxt][i] = *reinterpret_cast<const f32x4*>(pA + 32 * i * LD + 8 * (c + 1));
#pragma unroll
                for (int j = 0; j < TN; ++j) fb[nxt][j] = *reinterpret_cast<const f32x4*>(pB + 32 * j * LD + 8 * (c + 1));
            }
            __builtin_amdgcn_sched_barrier(0);   // keep the next chunk's reads ahead of these MFMAs
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][i][t], fb[cur][j][t], acc[i][j], 0, 0, 0);
            if (c == 0 && st) store_tile(h ^ 1, sset);
            if (c == 1 && ld) load_tile(sset);
        }
        __syncthreads();
    };
    // The register set always holds the NEXT tile: it is written to the other LDS buffer right
    // behind the first MFMAs of a tile and immediately re-loaded with the tile after that, so every
    // global load has a full K-tile of MFMA time to land (hipcc drains vmcnt to 0 at the LDS write
    // whatever is newer in flight, so the write sits where nothing newer is).
    if (nk >= 5) {
        // Two tiles ahead: the loads of tile t are issued while tile t-3 is multiplied and are needed (LDS write) while tile
        // t-1 is -- two K-tiles of time to land instead of one.  A K-tile of this kernel lasts about as long as a load
        // that misses L2 takes, so with one tile of slack every tile waited for its slowest load.  Two register sets; the
        // loop is unrolled by two so that set and buffer indices are compile-time, and the steady part issues its loads
        // unconditionally: only then can hipcc count the loads in flight and wait for the OLDER set alone (vmcnt(4));
        // one conditional load anywhere on the path and it drains the queue (vmcnt(0)) at every LDS write.
        // tile kt (buffer kt & 1) writes out tile kt+1 (set (kt+1) & 1, loaded two tiles ago) and loads tile kt+3 into that set.
        set_tap();
        load_tile(0);
        load_tile(1);
        store_tile(0, 0);
        load_tile(0);
        __syncthreads();
        int kt = 0;
        for (; kt + 4 < nk; kt += 2) {           // both halves have a tile kt+3 to load
            tile(0, 1, true, true);
            tile(1, 0, true, true);
        }
        for (; kt < nk; kt += 2) {               // the last three or four tiles
            tile(0, 1, kt + 1 < nk, kt + 3 < nk);
            if (kt + 1 < nk) tile(1, 0, kt + 2 < nk, kt + 4 < nk);
        }
    } else {
        // one tile ahead: tile kt+1 was loaded a tile ago, tile kt+2 lands during this tile
        if (nk > 0) {
            set_tap();
            load_tile(0);
            store_tile(0, 0);
            if (nk > 1) load_tile(0);
        }
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) tile(kt & 1, 0, kt + 1 < nk, kt + 2 < nk);
    }

    // ---- epilogue ----------------------------------------------------------------------
    // The accumulators go through LDS once (the main loop's last barrier has passed: the staging buffers are free) so that the
    // fused arithmetic and the stores work on four consecutive channels per lane: a quarter of the store / aref-load
    // instructions, each covering a row's BN * 4 contiguous bytes.  Same values, same operations per element.
    float* const outp = gridDim.y > 1 ? a.slab + (size_t)blockIdx.y * a.slab_stride : static_cast<float*>(a.out);
    const int epi = gridDim.y > 1 ? (int)EPI_RAW : a.epi;
    constexpr int LDT = BN + 4;                      // 16-byte slots per row: odd multiple for BN = 32, 64, 128
    static_assert(BM * LDT <= 2 * LD * (BM + BN), "output tile must fit the staging buffers");
    float* const sT = smem;
    if (KQ > 1) kq_handover(smem + 2 * LD * (BM + BN), b.quad, wave, lane, acc);      // (red: b.quad 1's own staging area)
    if (b.quad == 0) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    sT[(wm * (32 * TM) + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh) * LDT + wn * (32 * TN) + 32 * j + li] = acc[i][j][r];
    }
    __syncthreads();
    if (b.quad != 0 && epi != EPI_BN_BWD_STATS) return;       // (with the statistics every wave stays for the barriers below)
    constexpr int C4 = BN / 4, RPP = 256 / C4;       // float4 columns per row, rows per pass
    const int c4 = b.tid % C4, r0 = b.tid / C4;
    const int co = b.n0 + c4 * 4;
    EpiState q = epi_load(a, epi, co);
#pragma unroll
    for (int p = 0; p < BM / RPP; ++p) {
        const int row = r0 + RPP * p, m = b.m0 + row;
        if (m >= a.M || b.quad != 0) continue;
        const int n = m >> (a.lgHr + a.lgWr);
        size_t opix;
        if (a.form == 0) {
            opix = (size_t)m;
        } else {
            const int rh = (m >> a.lgWr) & (b.Hr - 1), rw = m & (b.Wr - 1);
            opix = ((size_t)n * a.Ho + 2 * rh + b.ph) * a.Wo + 2 * rw + b.pw;
        }
        const size_t o = opix * a.Co + co;
        const f32x4 v = epi_apply<float, LK>(a, q, *reinterpret_cast<const f32x4*>(sT + row * LDT + c4 * 4), o, n, co);
        *reinterpret_cast<f32x4*>(outp + o) = v;
    }
    if (q.stats) {
        __syncthreads();                             // the tile is stored: sT is free
        epi_stats_reduce(a, q, sT, b.tid, b.quad == 0, c4, r0, C4, RPP, (size_t)b.cls * (gridDim.x / b.tiles_n) + b.bid / b.tiles_n, co);
    }
}

// ------------------------------------------------------------------------------------------
// "up" form with all four output-parity classes in one workgroup, for the short-K layers with 32 output channels
// (Generator blocks 3-4: K = 4 taps x 32-64 channels per class, i.e. 4-8 K-tiles -- the per-class kernel above spends
// most of its time in prologue and epilogue there).  The four classes of an input pixel read a 3x3 neighbourhood
// between them, each a 2x2 corner of it: input offset (oh, ow) in {-1,0,1}^2 feeds the classes with
// ph in P(oh), pw in P(ow), P(-1) = {0}, P(0) = {0,1}, P(1) = {1}, through tap th = ph - oh, tw = pw - ow.
// One workgroup = 128 consecutive input pixels of one image x 32 channels x 4 classes.  Its whole input -- the pixel
// rows it covers plus a one-pixel halo, all CI channels -- is brought into LDS ONCE (one burst of independent loads,
// zero outside the image); the nine taps are then shifted views of that patch, so the K loop stages only the small
// weight tiles.  Four accumulators per wave; the 2x2 output pixels of the 128 input pixels form one contiguous 64 KB
// range of the NHWC output, assembled in LDS and stored with 16-byte lanes.
// ------------------------------------------------------------------------------------------
template <int CI, bool LK>
__global__ __launch_bounds__(256) void k_gconv_up4(const GConvArgs a) {
    constexpr int BM = 128, BN = 32, LD = BK + 4, LP = CI + 4, NCC = CI / BK;
    constexpr int PATCH_PIX = 264;                   // (128 / Wr + 2) * (Wr + 2) for Wr = 16, 32, 64: 180, 204, 264
    constexpr int SMEM = (PATCH_PIX * LP + 2 * 4 * BN * LD) > (BM * 4 * BN) ? (PATCH_PIX * LP + 2 * 4 * BN * LD) : (BM * 4 * BN);
    __shared__ __attribute__((aligned(16))) float smem[SMEM];
    float* const sP = smem;                          // [patch pixel][LP]
    float* const sB = smem + PATCH_PIX * LP;         // [2][4 classes][BN][LD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int m0 = xcd_remap(blockIdx.x, gridDim.x) * BM;
    const int Hr = 1 << a.lgHr, Wr = 1 << a.lgWr, Wp = Wr + 2;
    const int Ktot = 4 * CI;
    const int n_img = m0 >> (a.lgHr + a.lgWr), rh0 = (m0 >> a.lgWr) & (Hr - 1), rows = BM >> a.lgWr;

    // ---- the input patch: rows rh0-1 .. rh0+rows, columns -1 .. Wr, every channel ----------------------------
    {
        const float* const img = static_cast<const float*>(a.in) + (size_t)n_img * a.Hi * a.Wi * CI;
        const int nchunk = (rows + 2) * Wp * (CI / 4);
        constexpr int NI = (PATCH_PIX * (CI / 4) + 255) / 256;      // loads per thread, all issued before the first LDS write
        f32x4 v[NI];
#pragma unroll
        for (int q = 0; q < NI; ++q) {
            const int i = tid + 256 * q;
            const int pix = i / (CI / 4), ch = i - pix * (CI / 4);
            const int pr = pix / Wp, pc = pix - pr * Wp;
            const int ih = rh0 - 1 + pr, iw = pc - 1;
            const bool ok = i < nchunk && (unsigned)ih < (unsigned)a.Hi && (unsigned)iw < (unsigned)a.Wi;
            const float* src = ok ? img + ((size_t)ih * a.Wi + iw) * CI + ch * 4 : a.zeros;
            v[q] = *reinterpret_cast<const f32x4*>(src);
        }
#pragma unroll
        for (int q = 0; q < NI; ++q) {
            const int i = tid + 256 * q;
            if (i < nchunk) {
                const int pix = i / (CI / 4), ch = i - pix * (CI / 4);
                *reinterpret_cast<f32x4*>(sP + pix * LP + ch * 4) = v[q];
            }
        }
    }
    // ---- weight tiles: K-tile kt = (class, channel chunk); its four taps' [32 co][32 ci] tiles are staged together by
    // thread (rloc = output channel, kc = 16-byte chunk), one tile ahead of the MFMAs ----------------------------------
    const int kc = tid & 7, rloc = tid >> 3;
    const float* const w_row = static_cast<const float*>(a.wp) + (size_t)rloc * Ktot + kc * 4;
    f32x4 rb[4];
    int l_k = 0;
    auto load_tile = [&]() __attribute__((always_inline)) {
        const int cls = l_k / NCC, cc = l_k - cls * NCC;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            rb[t] = *reinterpret_cast<const f32x4*>(w_row + (size_t)cls * a.Co * Ktot + t * CI + cc * BK);
        ++l_k;
    };
    auto store_tile = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            *reinterpret_cast<f32x4*>(sB + ((buf * 4 + t) * BN + rloc) * LD + kc * 4) = rb[t];
    };

    f32x16 acc[4];
#pragma unroll
    for (int cls = 0; cls < 4; ++cls)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cls][r] = 0.f;

    load_tile();
    store_tile(0);
    load_tile();
    __syncthreads();

    // this lane's pixel (A-operand row) inside the patch
    const int ml = wave * 32 + li;
    const float* const pP = sP + (((ml >> a.lgWr) + 1) * Wp + (ml & (Wr - 1)) + 1) * LP + 4 * lh;

#pragma unroll
    for (int cls = 0; cls < 4; ++cls) {
        const int ph = cls >> 1, pw = cls & 1;
        for (int cc = 0; cc < NCC; ++cc) {
            const int kt = cls * NCC + cc, buf = kt & 1;
            // tap t = (th, tw) reads the patch at input offset (ph - th, pw - tw)
            const float* pA[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) pA[t] = pP + ((ph - (t >> 1)) * Wp + (pw - (t & 1))) * LP + cc * BK;
            const float* pB = sB + (buf * 4 * BN + li) * LD + 4 * lh;
            f32x4 fa[2][4], fb[2][4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                fa[0][t] = *reinterpret_cast<const f32x4*>(pA[t]);
                fb[0][t] = *reinterpret_cast<const f32x4*>(pB + t * BN * LD);
            }
#pragma unroll
            for (int c = 0; c < BK / 8; ++c) {
                const int cur = c & 1, nxt = cur ^ 1;
                if (c + 1 < BK / 8) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        fa[nxt][t] = *reinterpret_cast<const f32x4*>(pA[t] + 8 * (c + 1));
                        fb[nxt][t] = *reinterpret_cast<const f32x4*>(pB + t * BN * LD + 8 * (c + 1));
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        acc[cls] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][t][u], fb[cur][t][u], acc[cls], 0, 0, 0);
                if (c == 0 && kt + 1 < 4 * NCC) store_tile(buf ^ 1);
                if (c == 1 && kt + 2 < 4 * NCC) load_tile();
            }
            __syncthreads();
        }
    }

    // ---- epilogue: assemble the contiguous output range in LDS in memory order, store with 16-byte lanes ---------
    const float sc = a.epi == EPI_AFFINE_RELU ? a.scale[li] : 1.f, sf = a.epi == EPI_AFFINE_RELU ? a.shift[li] : 0.f;
    const int Wo = 2 * Wr;
    float* const so = smem;                              // 128 * 4 * 32 floats; the main loop's last barrier has passed
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int mr = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const int rl = mr >> a.lgWr, rw = mr & (Wr - 1);
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) {
            float v = acc[cls][r];
            if (a.epi == EPI_AFFINE_RELU) v = g_act<LK>(fmaf(v, sc, sf), a.gslope);
            so[(((2 * rl + (cls >> 1)) * Wo) + 2 * rw + (cls & 1)) * BN + li] = v;
        }
    }
    __syncthreads();
    f32x4* const dst = reinterpret_cast<f32x4*>(static_cast<float*>(a.out) + ((size_t)n_img * a.Ho + 2 * rh0) * a.Wo * BN);
    const f32x4* const src = reinterpret_cast<const f32x4*>(so);
#pragma unroll
    for (int q = 0; q < (BM * 4 * BN / 4) / 256; ++q) dst[q * 256 + tid] = src[q * 256 + tid];
}

// split-K tail: out = epilogue(sum_z slab[z]) over the NHWC output (4 channels per thread; the epilogues of gconv_parts.h)
template <class T, bool LK>
__global__ __launch_bounds__(256) void k_splitk_epilogue(const GConvArgs a, int nsplit, int64_t total4) {
    __shared__ __attribute__((aligned(16))) float sh[256 * 8];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int C4 = a.Co / 4;
    const int64_t per_img = (int64_t)C4 * a.Ho * a.Wo;
    const bool p2 = (C4 & (C4 - 1)) == 0 && (per_img & (per_img - 1)) == 0;       // every layer: shifts instead of 64-bit divisions
    const int c4 = p2 ? (int)(i & (C4 - 1)) : (int)(i % C4);
    const int64_t n = p2 ? i >> (63 - __builtin_clzll(per_img)) : i / per_img;
    EpiState q = epi_load(a, a.epi, c4 * 4);
    if (i >= total4 && !q.stats) return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (i < total4) {
        const f32x4* sl = reinterpret_cast<const f32x4*>(a.slab);
        const size_t stride4 = a.slab_stride / 4;
        v = sl[i];
        for (int z = 1; z < nsplit; ++z) v += sl[(size_t)z * stride4 + i];
        v = epi_apply<T, LK>(a, q, v, (size_t)i * 4, (int)n, c4 * 4);
        st4<T>(static_cast<T*>(a.out) + i * 4, v);
    }
    if (q.stats) {
        // 256 consecutive float4 = 256 / C4 rows of all C4 channel groups (launch_gconv checks C4 | 256): one partial row per
        // workgroup; a ragged last workgroup's idle threads bring zeros
        epi_stats_reduce(a, q, sh, threadIdx.x, true, c4, (int)threadIdx.x / C4, C4, 256 / C4, blockIdx.x, c4 * 4);
        return;
    }
    if (a.cls_w) {
        // the classifier's dot product over the values just stored (as stored: rounded to T), 1024 of them per workgroup; every
        // thread is here (launch_gconv: total4 % 256 == 0, per_img % 256 == 0)
        __shared__ float shc[4];
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(a.cls_w + (size_t)(p2 ? (i & (per_img - 1)) : (i % per_img)) * 4);
        float d = (float)(T)v[0] * w4[0];
        d = fmaf((float)(T)v[1], w4[1], d); d = fmaf((float)(T)v[2], w4[2], d); d = fmaf((float)(T)v[3], w4[3], d);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d += __shfl_down(d, o, 64);
        if ((threadIdx.x & 63) == 0) shc[threadIdx.x >> 6] = d;
        __syncthreads();
        if (threadIdx.x == 0) a.cls_part[blockIdx.x] = ((shc[0] + shc[1]) + shc[2]) + shc[3];
    }
}

Prof* g_prof = nullptr;

const char* Prof::name(int id) {
    static const char* n[NID] = {"k_gconv<128,128>", "k_gconv<128,64>", "k_gconv<64,64>", "k_gconv<128,32>",
                                 "k_wgrad<64,64>", "k_gconv_up4", "k_wgrad<32,128>", "?"};
    return n[id < 0 || id >= NID ? NID - 1 : id];
}
// The two events of a record are handed to hipExtLaunchKernelGGL, which stamps them with the
// kernel's own begin / end (the dispatch's completion-signal timestamps), so a record's elapsed time
// is the kernel duration rocprofv3 reports -- not the launch-to-launch gap a plain
// hipEventRecord pair would include.
void Prof::begin(int id, double flops, double bytes, hipStream_t) {
    Rec r; r.id = id; r.flops = flops; r.bytes = bytes;
    r.form = r.epi_req = r.epi = r.M = r.Ci = r.Co = r.slabs = r.kq = -1;
    (void)hipEventCreate(&r.e0); (void)hipEventCreate(&r.e1);
    recs.push_back(r);
}
void Prof::shape(const GConvArgs& a, int epi_req, int slabs, int kq) {
    Rec& r = recs.back();
    r.form = a.form; r.epi_req = epi_req; r.epi = a.epi; r.M = a.M; r.Ci = a.Ci; r.Co = a.Co; r.slabs = slabs; r.kq = kq;
}
void Prof::clear() {
    for (auto& r : recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    recs.clear();
}

// algorithmic HBM bytes of one implicit-GEMM launch: input tensor and packed weights read once, output written once
// (+ the stored activation the fused LeakyReLU-backward epilogue reads); split-K slabs and tile re-reads are not counted
static double gconv_bytes(const GConvArgs& a) {
    const double es = (double)dt_size(a.dt);
    const double in = (double)a.B * a.Hi * a.Wi * a.Ci, out = (double)a.B * a.Ho * a.Wo * a.Co, w = 16.0 * a.Ci * a.Co;
    return es * (in + w + out * (a.epi == EPI_LRELU_BWD ? 2.0 : 1.0));
}
static double wgrad_bytes(const WgradArgs& a) {
    const double es = (double)dt_size(a.dt);
    return es * ((double)a.K * a.Cs + 4.0 * a.K * a.Cl) + 4.0 * 16.0 * a.Cs * a.Cl;
}

template <int BM, int BN, int WM, int WN, int KQ = 1>
static int launch_cfg(const GConvArgs& a_in, hipStream_t st, int id, int nsplit) {
    GConvArgs a = a_in;
    const int tiles = ((a.M + BM - 1) / BM) * (a.Co / BN);
    const int ncls = a.form == 0 ? 1 : 4;
    const int64_t total4 = (int64_t)a.B * a.Ho * a.Wo * a.Co / 4;
    int rows = 0;
    if (a.epi == EPI_BN_BWD_STATS) {
        // one partial row per workgroup of whichever kernel runs the epilogue; k_splitk_epilogue needs whole rows per workgroup
        if (nsplit > 1 && (256 % (a.Co / 4)) != 0) nsplit = 1;
        rows = nsplit > 1 ? (int)((total4 + 255) / 256) : ((a.M + BM - 1) / BM) * ncls;
        if ((int64_t)2 * rows * a.Co > a.stat_cap) { a.epi = EPI_RAW; rows = 0; }     // (a batch whose partial rows outgrow the carve)
        else a.stat1 = a.stat0 + (size_t)rows * a.Co;
    }
    if (a.cls_w) {
        const int64_t per_img4 = (int64_t)a.Ho * a.Wo * a.Co / 4;
        if (nsplit > 1 && a.epi != EPI_BN_BWD_STATS && total4 % 256 == 0 && per_img4 % 256 == 0) rows = (int)(per_img4 / 256);
        else a.cls_w = nullptr;
    }
    dim3 grid(tiles, nsplit, ncls);
    // algorithmic FLOPs = 2 * M * Co * (taps * Ci) per class (== 2 * conv MACs, padding taps included)
    if (g_prof) {
        g_prof->begin(id, 2.0 * a.M * a.Co * (double)((a.form == 0 ? 16 : 4) * a.Ci) * ncls, gconv_bytes(a), st);
        g_prof->shape(a, a_in.epi, nsplit, KQ);
    }
    hipEvent_t e0 = g_prof ? g_prof->recs.back().e0 : nullptr, e1 = g_prof ? g_prof->recs.back().e1 : nullptr;
    if (a.dt != DT_F32) {
        launch_gconv16(id, a, grid, st, e0, e1, KQ);
    } else if (gen_lk(a)) {
        hipExtLaunchKernelGGL((k_gconv<BM, BN, WM, WN, KQ, true>), grid, dim3(256 * KQ), 0, st, e0, e1, 0, a);
    } else if (g_prof) {
        hipExtLaunchKernelGGL((k_gconv<BM, BN, WM, WN, KQ>), grid, dim3(256 * KQ), 0, st, e0, e1, 0, a);
    } else {
        hipLaunchKernelGGL((k_gconv<BM, BN, WM, WN, KQ>), grid, dim3(256 * KQ), 0, st, a);
    }
    if (nsplit > 1)
        SIGGAN_GS_SWITCH(gen_lk(a) ? 1.f : 0.f, LK, SIGGAN_DT_SWITCH(a.dt, T, hipLaunchKernelGGL((k_splitk_epilogue<T, LK>),
            dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, a, nsplit, total4)));
    return rows;
}

int launch_gconv(const GConvArgs& a_in, hipStream_t st) {
    // Tile choice: the fp32 MFMA is slow enough that a 32x32 accumulator per wave already runs the
    // matrix pipe at full rate, so what matters is having >= 2 workgroups per CU (512 on the chip)
    // to cover each other's barrier / first-fragment bubbles.  Take the largest tile that still
    // gives that; when even 64x64 tiles cannot, split K into slabs (summed by k_splitk_epilogue).
    GConvArgs a = a_in;
    // The BatchNorm-backward sums need a carve to land in.  A launch without one (a caller that did not set stat0 /
    // stat_cap) is refused before anything is enqueued: with stat_cap <= 0 it would quietly take the raw-store fallback
    // below (meant for a batch that outgrows a real carve) on every launch, and with a null stat0 and a positive cap the
    // epilogue would store its partial rows through a null pointer.
    if (a.epi == EPI_BN_BWD_STATS && (a.stat0 == nullptr || a.stat_cap <= 0)) return -1;
    const int ncls = a.form == 0 ? 1 : 4;
    auto blocks = [&](int bm, int bn) { return ((a.M + bm - 1) / bm) * (a.Co / bn) * ncls; };
    const int nk = (a.form == 0 ? 16 : 4) * (a.Ci / BK);
    // (the tile and split rules from here to the end of the function are restated in tests/evalpaths.py, matched as text by tests/test_eval_paths_cpu.py)
    auto splits = [&](int nblk) {
        int ns = 1;
        if (a.slab && nblk < 384) {
            ns = (512 + nblk - 1) / nblk;
            if (ns > nk / 4) ns = nk / 4;
            if (ns > 8) ns = 8;
            const int64_t out_floats = (int64_t)a.B * a.Ho * a.Wo * a.Co;
            if (ns > 1 && (int64_t)ns * out_floats > a.slab_floats) ns = (int)(a.slab_floats / out_floats);
            if (ns < 1) ns = 1;
        }
        a.slab_stride = (size_t)a.B * a.Ho * a.Wo * a.Co;
        return ns;
    };
    if (a.Co >= 64) {
        // 128x128 (four accumulators per wave, 82 % MFMA-busy) only when it still yields two workgroups per CU; the
        // 128x64 middle size measured below 64x64 on every shape of the step (86 vs 93 TFLOP/s) and is not built
        if (a.Co >= 128 && blocks(128, 128) >= 512) return launch_cfg<128, 128, 2, 2>(a, st, 0, 1);
        const int ns = splits(blocks(64, 64));
        // a two-way split runs as ONE launch of 8-wave workgroups (no slabs, no k_splitk_epilogue); nk is a power of two,
        // so the halves are equal
        if (ns == 2 && (nk & 1) == 0) return launch_cfg<64, 64, 2, 2, 2>(a, st, 2, 1);
        // 16-bit: a four-way split too (unless the classifier rides in the slab epilogue) -- the K loop is twice as long but
        // short either way, the epilogue launch is what counts: bf16 step 0.6172 -> 0.6077 ms (fp32: step unchanged, the
        // Generator's eval forward 87.7 -> 90.4 us: stays split)
        if (ns == 4 && !a.cls_w && a.dt != DT_F32 && (nk & 1) == 0) return launch_cfg<64, 64, 2, 2, 2>(a, st, 2, 1);
        return launch_cfg<64, 64, 2, 2>(a, st, 2, ns);
    }
    if (a.dt == DT_F32 && a.form == 1 && a.Co == 32 && (a.epi == EPI_RAW || a.epi == EPI_AFFINE_RELU) && (a.Ci == 32 || a.Ci == 64) &&
        a.M / 128 >= (a.Ci == 32 ? 384 : 768) && a.M % 128 == 0 &&
        ((1 << (a.lgHr + a.lgWr)) % 128) == 0 && a.lgWr >= 4 && a.lgWr <= 6) {
        // all four parity classes per workgroup, input patch resident in LDS (k_gconv_up4): the short-K Generator blocks
        dim3 grid(a.M / 128);
        if (g_prof) {
            g_prof->begin(5, 2.0 * a.M * a.Co * (double)(4 * a.Ci) * 4, gconv_bytes(a), st);
            g_prof->shape(a, a.epi);
        }
        hipEvent_t e0 = g_prof ? g_prof->recs.back().e0 : nullptr, e1 = g_prof ? g_prof->recs.back().e1 : nullptr;
        if (gen_lk(a)) {
            if (a.Ci == 32) hipExtLaunchKernelGGL((k_gconv_up4<32, true>), grid, dim3(256), 0, st, e0, e1, 0, a);
            else hipExtLaunchKernelGGL((k_gconv_up4<64, true>), grid, dim3(256), 0, st, e0, e1, 0, a);
        } else {
            if (a.Ci == 32) hipExtLaunchKernelGGL((k_gconv_up4<32, false>), grid, dim3(256), 0, st, e0, e1, 0, a);
            else hipExtLaunchKernelGGL((k_gconv_up4<64, false>), grid, dim3(256), 0, st, e0, e1, 0, a);
        }
        return 0;
    }
    const int ns = splits(blocks(128, 32));
    return launch_cfg<128, 32, 4, 1>(a, st, 3, ns);   // Co == 32
}

// ------------------------------------------------------------------------------------------
// weight gradient: C[i][j] = sum_pix S[pix][i] * Lg[pix][j],  j = tap*Cl + l
// ------------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void k_wgrad(const WgradArgs a) {
    constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
    constexpr int LDA = BM + PAD, LDB = BN + PAD;
    constexpr int CA = BM / 4, RA = 256 / CA, PA = BK / RA;     // float4 chunks per k-row, rows per pass
    constexpr int CB = BN / 4, RB = 256 / CB, PB = BK / RB;
    __shared__ __attribute__((aligned(16))) float smem[2 * BK * (LDA + LDB)];
    float* const sA = smem;
    float* const sB = smem + 2 * BK * LDA;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int N = 16 << a.lgCl;
    const int tiles_n = N / BN;
    // Workgroups are handed out round-robin over the 8 XCDs; remapped, a run of consecutive logical ids -- the tiles of ONE K
    // split, which share its S rows and its gathered L pixels -- lands on one XCD and meets in that L2: 84.4 -> 40.1 MB of HBM
    // traffic per launch (32x128: 108 -> 51.5; the step 2.60 -> 2.28 GB).  The kernel's own time does not move (50.6 us: its
    // loads are not what it waits for, round 2 found the same), the pipelined step gains 0.2-1 %: the bytes it no longer
    // moves are there for the kernels beside it.
    const int lin = blockIdx.z * gridDim.x + blockIdx.x;
    const int lid = xcd_remap(lin, gridDim.x * gridDim.z);
    const int bx = lid % gridDim.x, bz = lid / gridDim.x;
    const int i0 = (bx / tiles_n) * BM, j0 = (bx % tiles_n) * BN;
    const int kbeg = bz * a.kchunk;
    const int kend = min(a.K, kbeg + a.kchunk);
    const int nk = (kend - kbeg + BK - 1) / BK;
    const int Hs = 1 << a.lgHs, Ws = 1 << a.lgWs, Hl = 2 * Hs, Wl = 2 * Ws, Cl = 1 << a.lgCl;

    const int ca = tid % CA, ka = tid / CA;
    const int cb = tid % CB, kb = tid / CB;
    const float* const a_S = static_cast<const float*>(a.S);
    const float* const a_L = static_cast<const float*>(a.L);
    const int jj = j0 + cb * 4, tap = jj >> a.lgCl, lch = jj & (Cl - 1);
    const int kh = tap >> 2, kw = tap & 3;

    f32x4 ra[2][PA], rb[2][PB];          // two register sets: tile t waits in set t & 1 (second set: the deep path only)
    // Tiles are loaded strictly in K order, so the loader keeps running state instead of deriving addresses from the tile
    // index: the S pointer advances by a constant, and the gathered L address is a handful of shifts (every extent is a power
    // of two) off the running pixel index.  The first version recomputed both from scratch with 64-bit multiplies: 1100 cycles
    // of VALU work per K-tile, which the matrix pipe does not hide (a wave's VALU instructions queue behind its own MFMAs).
    // (offsets from the kernel-argument pointers, not running pointers: a loop-carried pointer loses its address space and
    // hipcc falls back to flat loads, whose counter semantics also cost the exact vmcnt waits of the deep path)
    size_t a_off[PA];
    int a_pix[PA], b_pix[PB];
#pragma unroll
    for (int p = 0; p < PA; ++p) { a_pix[p] = kbeg + ka + RA * p; a_off[p] = (size_t)a_pix[p] * a.Cs + i0 + ca * 4; }
#pragma unroll
    for (int p = 0; p < PB; ++p) b_pix[p] = kbeg + kb + RB * p;
    const int a_adv = BK * a.Cs;
    const int lgWl = a.lgWs + 1;
    // (macros, not lambdas: hipcc left the staged float4 arrays in scratch when these were lambdas)
#define WG_LOAD_TILE(KT, SET)                                                                         \
    {                                                                                                 \
        _Pragma("unroll") for (int p = 0; p < PA; ++p) {                                              \
            const float* src = a_pix[p] < kend ? a_S + a_off[p] : a.zeros;                            \
            ra[SET][p] = *reinterpret_cast<const f32x4*>(src);                                       \
            a_off[p] += a_adv; a_pix[p] += BK;                                                        \
        }                                                                                             \
        _Pragma("unroll") for (int p = 0; p < PB; ++p) {                                              \
            const int pix = b_pix[p];                                                                 \
            const int y = pix >> a.lgWs;                       /* n * Hs + py */                       \
            const int ih = 2 * (y & (Hs - 1)) - 1 + kh, iw = 2 * (pix & (Ws - 1)) - 1 + kw;           \
            const bool ok = pix < kend && (unsigned)ih < (unsigned)Hl && (unsigned)iw < (unsigned)Wl; \
            /* n * Hl + ih = 2 * y - 1 + kh: the large-image row index is linear in y */              \
            const unsigned off = (((unsigned)(2 * y - 1 + kh) << lgWl) + (unsigned)iw) << a.lgCl;     \
            const float* src = ok ? a_L + ((size_t)off + lch) : a.zeros;                              \
            rb[SET][p] = *reinterpret_cast<const f32x4*>(src);                                       \
            b_pix[p] += BK;                                                                           \
        }                                                                                             \
    }
#define WG_STORE_TILE(BUF, SET)                                                                       \
    {                                                                                                 \
        _Pragma("unroll") for (int p = 0; p < PA; ++p)                                                \
            *reinterpret_cast<f32x4*>(sA + (BUF) * BK * LDA + (ka + RA * p) * LDA + ca * 4) = ra[SET][p]; \
        _Pragma("unroll") for (int p = 0; p < PB; ++p)                                                \
            *reinterpret_cast<f32x4*>(sB + (BUF) * BK * LDB + (kb + RB * p) * LDB + cb * 4) = rb[SET][p]; \
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // column sums of S (the bias gradient when S is d(pre-activation)) ride along in the first column tile: thread t
    // owns column t % BM and the k rows [kq * KQ, kq * KQ + KQ) of every K-tile, the slices are added at the end
    constexpr int NQ = 256 / BM, KQ = BK / NQ;
    const bool bias_blk = a.db != nullptr && j0 == 0;
    const int bcol = tid % BM, kq = tid / BM;
    float bsum = 0.f;
    // one K-tile out of LDS buffer BUF; ST / LD: an LDS write / a global load of a later tile rides along (see below)
#define WG_TILE(BUF, ST, LD)                                                                          \
    {                                                                                                 \
        if (bias_blk) {                                                                               \
            const float* col = sA + (BUF) * BK * LDA + kq * KQ * LDA + bcol;                          \
            _Pragma("unroll") for (int k = 0; k < KQ; ++k) bsum += col[k * LDA];                      \
        }                                                                                             \
        const float* pA = sA + (BUF) * BK * LDA + lh * LDA + wm * (32 * TM) + li;                     \
        const float* pB = sB + (BUF) * BK * LDB + lh * LDB + wn * (32 * TN) + li;                     \
        /* fragments are fetched a chunk of four k-steps ahead of the MFMAs that use them (256 cycles of matrix-pipe time to   \
           cover the LDS latency; one step ahead -- 64 cycles -- left every MFMA waiting for its operands) */                  \
        float fa[2][4][TM], fb[2][4][TN];                                                             \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                               \
            _Pragma("unroll") for (int i = 0; i < TM; ++i) fa[0][q][i] = pA[(2 * q) * LDA + 32 * i];  \
            _Pragma("unroll") for (int j = 0; j < TN; ++j) fb[0][q][j] = pB[(2 * q) * LDB + 32 * j];  \
        }                                                                                             \
        _Pragma("unroll") for (int c = 0; c < BK / 8; ++c) {                                          \
            const int cur = c & 1, nxt = cur ^ 1;                                                     \
            if (c + 1 < BK / 8) {                                                                     \
                _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                       \
                    _Pragma("unroll") for (int i = 0; i < TM; ++i) fa[nxt][q][i] = pA[(8 * c + 8 + 2 * q) * LDA + 32 * i]; \
                    _Pragma("unroll") for (int j = 0; j < TN; ++j) fb[nxt][q][j] = pB[(8 * c + 8 + 2 * q) * LDB + 32 * j]; \
                }                                                                                     \
            }                                                                                         \
            __builtin_amdgcn_sched_barrier(0);                                                        \
            _Pragma("unroll") for (int q = 0; q < 4; ++q)                                             \
                _Pragma("unroll") for (int i = 0; i < TM; ++i)                                        \
                    _Pragma("unroll") for (int j = 0; j < TN; ++j)                                    \
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][q][i], fb[cur][q][j], acc[i][j], 0, 0, 0); \
            if (c == 0) { ST }                                                                        \
            if (c == 1) { LD }                                                                        \
        }                                                                                             \
        __syncthreads();                                                                              \
    }
    if (nk >= 5) {
        // two tiles ahead (see k_gconv): tile t is loaded while tile t-3 is multiplied and written to LDS while tile t-1 is;
        // the steady loop issues its loads unconditionally so that the LDS write waits for the older register set only
        WG_LOAD_TILE(0, 0)
        WG_LOAD_TILE(1, 1)
        WG_STORE_TILE(0, 0)
        WG_LOAD_TILE(2, 0)
        __syncthreads();
        int kt = 0;
        for (; kt + 4 < nk; kt += 2) {
            WG_TILE(0, WG_STORE_TILE(1, 1), WG_LOAD_TILE(kt + 3, 1))
            WG_TILE(1, WG_STORE_TILE(0, 0), WG_LOAD_TILE(kt + 4, 0))
        }
        for (; kt < nk; kt += 2) {
            WG_TILE(0, if (kt + 1 < nk) WG_STORE_TILE(1, 1), if (kt + 3 < nk) WG_LOAD_TILE(kt + 3, 1))
            if (kt + 1 < nk) WG_TILE(1, if (kt + 2 < nk) WG_STORE_TILE(0, 0), if (kt + 4 < nk) WG_LOAD_TILE(kt + 4, 0))
        }
    } else {
        if (nk > 0) {
            WG_LOAD_TILE(0, 0)
            WG_STORE_TILE(0, 0)
            if (nk > 1) WG_LOAD_TILE(1, 0)
        }
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            if (kt & 1) WG_TILE(1, if (kt + 1 < nk) WG_STORE_TILE(0, 0), if (kt + 2 < nk) WG_LOAD_TILE(kt + 2, 0))
            else WG_TILE(0, if (kt + 1 < nk) WG_STORE_TILE(1, 0), if (kt + 2 < nk) WG_LOAD_TILE(kt + 2, 0))
        }
    }
#undef WG_TILE

#undef WG_LOAD_TILE
#undef WG_STORE_TILE
    wgrad_tail<BM, BN, WM, WN>(a, smem, bias_blk, bsum, i0, j0, bz, acc);
}

static void launch_wgrad_reduce(const float* slab, float* dw, float* db, int nsplit, int Cs, int Cl, hipStream_t st);

int launch_wgrad(WgradArgs a, int max_splits, hipStream_t st) {
    // 64x64 tiles (one 32x32 accumulator per wave keeps the fp32 MFMA pipe full): many tiles,
    // hence few K splits and little slab traffic; Cs == 32 uses a 32x128 tile.
    // (measured and dropped in round 3, DESIGN 4: 64x128 tiles; three / four workgroups per CU through more K splits)
    const int N = 16 << a.lgCl;
    const bool small = a.Cs < 64;
    const int tiles = small ? (N / 128) : (a.Cs / 64) * (N / 64);
    int ktiles = (a.K + BK - 1) / BK;
    int nsplit = (512 + tiles - 1) / tiles;                  // ~2 workgroups per CU
    if (nsplit > ktiles / 4) nsplit = ktiles / 4;            // at least 4 K-tiles per split
    if (nsplit > max_splits) nsplit = max_splits;
    if (nsplit < 1) nsplit = 1;
    int per = (ktiles + nsplit - 1) / nsplit;
    a.kchunk = per * BK;
    nsplit = (ktiles + per - 1) / per;
    dim3 grid(tiles, 1, nsplit);
    if (g_prof) g_prof->begin(small ? 6 : 4, 2.0 * a.Cs * (double)N * a.K, wgrad_bytes(a), st);
    hipEvent_t e0 = g_prof ? g_prof->recs.back().e0 : nullptr, e1 = g_prof ? g_prof->recs.back().e1 : nullptr;
    if (a.dt != DT_F32) {
        launch_wgrad16(small, a, grid, st, e0, e1);
    } else if (g_prof) {
        if (small) hipExtLaunchKernelGGL((k_wgrad<32, 128, 1, 4>), grid, dim3(256), 0, st, e0, e1, 0, a);
        else hipExtLaunchKernelGGL((k_wgrad<64, 64, 2, 2>), grid, dim3(256), 0, st, e0, e1, 0, a);
    } else if (small) {
        hipLaunchKernelGGL((k_wgrad<32, 128, 1, 4>), grid, dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((k_wgrad<64, 64, 2, 2>), grid, dim3(256), 0, st, a);
    }
    if (nsplit > 1) launch_wgrad_reduce(a.slab, a.dw, a.db, nsplit, a.Cs, 1 << a.lgCl, st);
    return nsplit;
}

// dw[(s*Cl + l)*16 + tap] = sum_z slab[z][s][tap*Cl + l].  A block owns 64 consecutive slab columns;
// SL lanes per column each add every SL-th slab, then LDS combines the lanes in lane order (the sum
// order is fixed by (nsplit, SL) alone: bitwise reproducible).
__global__ __launch_bounds__(1024) void k_wgrad_reduce(const float* __restrict__ slab, float* __restrict__ dw, float* __restrict__ db,
                                                       int nsplit, int Cs, int lgCl) {
    __shared__ float sh[16][64];
    const int N = 16 << lgCl, Cl = 1 << lgCl;
    const size_t total = (size_t)Cs * N;
    const int cl = threadIdx.x & 63, zl = threadIdx.x >> 6, SL = blockDim.x >> 6;
    const size_t wblocks = total / 64;
    const bool bias = blockIdx.x >= wblocks;                       // the blocks behind the weight columns: db
    const size_t idx = bias ? (size_t)(blockIdx.x - wblocks) * 64 + cl : (size_t)blockIdx.x * 64 + cl;
    const float* src = bias ? slab + (size_t)nsplit * total : slab;
    const size_t zstride = bias ? (size_t)Cs : total;
    const bool live = !bias || idx < (size_t)Cs;
    float acc = 0.f;
    if (live) {
#pragma unroll 8
        for (int z = zl; z < nsplit; z += SL) acc += src[(size_t)z * zstride + idx];
    }
    if (SL > 1) {
        sh[zl][cl] = acc;
        __syncthreads();
        if (zl != 0) return;
        for (int k = 1; k < SL; ++k) acc += sh[k][cl];
    }
    if (!live) return;
    if (bias) { db[idx] = acc; return; }
    const int j = (int)(idx & (size_t)(N - 1)), s_ = (int)(idx >> (4 + lgCl));      // N = 16 << lgCl
    const int tap = j >> lgCl, l = j & (Cl - 1);
    dw[((size_t)s_ * Cl + l) * 16 + tap] = acc;
}

static void launch_wgrad_reduce(const float* slab, float* dw, float* db, int nsplit, int Cs, int Cl, hipStream_t st) {
    const size_t total = (size_t)Cs * 16 * Cl;                 // a multiple of 64 (Cs, Cl >= 32)
    int SL = 1;
    while (SL < 16 && SL < nsplit) SL *= 2;
    const unsigned blocks = (unsigned)(total / 64) + (db ? (unsigned)((Cs + 63) / 64) : 0u);
    hipLaunchKernelGGL(k_wgrad_reduce, dim3(blocks), dim3(64 * SL), 0, st, slab, dw, db, nsplit, Cs, ilog2(Cl));
}

}  // namespace siggan
