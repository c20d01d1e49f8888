// ctx.h -- what the engine's host files (siggan.hip, passes.hip, step.hip, eval.hip, extras.hip) share: the context, the state a
// step carries between calls, the lanes, and the prototypes of the functions that cross those files.  Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>

#include "../../include/siggan.h"
#include "gconv.h"
#include "host.h"
#include "ops.h"

using namespace siggan;

static const float BN_MOMENTUM = 0.1f, BN_EPS = 1e-5f;   // nn.BatchNorm defaults (generator_vanilla_gan.py:58,126)
static const int MAXL = 6;
// (restated in tests/evalpaths.py, matched as text by tests/test_eval_paths_cpu.py)
static const int64_t PARTIAL_FLOATS = (int64_t)2 << 20;   // each of the three reduction-partial regions (partial, partial_b, partial_c)
static const float SN_EPS = 1e-12f;        // torch.nn.utils.spectral_norm's eps
// Events that order the library's own lanes against each other on ONE device carry no system-scope fence: with the default
// flags every record writes back / invalidates caches for the host and for peer devices, which showed up as a ~6 us hole
// behind each fork on the recording lane (-1.5 % step time at fp32, -3.8 % at bf16 without it).  Kernel boundaries
// still release at agent scope, which is all a kernel on another lane of the same device needs.  The events in front of an
// RCCL collective (peer devices read the gradient arena over xGMI) keep the fence: while a communicator exists the lanes use
// the fenced ring (ev_fenced), and ev_sys / ev_ar are always fenced.
#define EV_FLAGS (hipEventDisableTiming | hipEventDisableSystemFence)
#define LAUNCHCHK()                                                                                 \
    do {                                                                                            \
        hipError_t e_ = hipGetLastError();                                                          \
        if (e_ != hipSuccess) return FAIL(SIGGAN_E_HIP, "kernel launch -> %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define ENTER(c)                                                     \
    if (!(c)) return FAIL(SIGGAN_E_INVALID, "null context");          \
    DevGuard dg_((c)->cfg.device);                                    \
    HIPCHK(dg_.err)

// RCCL (the collective of the data-parallel step).  The library does not link librccl: the
// process that loads it normally holds one already (torch bundles its own copy), and a second HIP/RCCL runtime in one
// process is what SURVEY 7 warns about.  The five entry points used are resolved with dlsym from the copy that is
// loaded (RTLD_NOLOAD), else from the first librccl the loader finds.  Declarations follow the stable NCCL C API.
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId_t;
enum { NCCL_SUCCESS = 0, NCCL_CHAR = 0, NCCL_FLOAT32 = 7, NCCL_SUM = 0 };
struct Rccl {
    void* h = nullptr;
    int (*GetUniqueId)(ncclUniqueId_t*) = nullptr;
    int (*CommInitRank)(ncclComm_t*, int, ncclUniqueId_t, int) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*Broadcast)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    const char* err = nullptr;
};
namespace siggan { Rccl* rccl(); }    // extras.hip

struct PhaseKey {
    int phase, B, has_z, has_masks, g_dirty, d_dirty, spec_g, has_zg, pre_real, variant, coll;   // coll: an apply call follows (collectives may start early)
    float* mt;   // where the phase writes its metrics (caller's buffer, or the workspace one)
    double lr, beta1, beta2, eps;
    double fused_t;   // > 0: the step count (after the increment) of a one-launch optimiser update; 0: k_adam_prepare path
    int pack;         // apply: that launch also rebuilds the weight packs / eval tables (k_adam_pack)
    int ride;         // D apply: ... and runs the first Discriminator block of the pending G step's `ride` images (its riders)
    int rode;         // G grads: the preceding D apply did
    float ls, clip, gs;
    // what an earlier call left in flight, as far as THIS phase reads it (Carried, below; 0 where the phase does not look)
    int dreal_joined, dreal_noise2, lP0;   // pre_real == 2: the staged D(real) forward's lane state and its classifier form
    int gfwd_joined;                       // G grads after step_begin / D apply with riders: ev_gfwd was already waited for
    int early_ar;                          // D apply: the tail of the bucket is already being reduced
    const float* staged_src;               // pre_real: where the staged real batch lies
    bool operator==(const PhaseKey& o) const {
        return phase == o.phase && B == o.B && has_z == o.has_z && has_masks == o.has_masks && g_dirty == o.g_dirty &&
               d_dirty == o.d_dirty && spec_g == o.spec_g && has_zg == o.has_zg && pre_real == o.pre_real && variant == o.variant && coll == o.coll && mt == o.mt && lr == o.lr && beta1 == o.beta1 && beta2 == o.beta2 && eps == o.eps && ls == o.ls &&
               clip == o.clip && gs == o.gs && fused_t == o.fused_t && pack == o.pack && ride == o.ride && rode == o.rode &&
               dreal_joined == o.dreal_joined && dreal_noise2 == o.dreal_noise2 && lP0 == o.lP0 && gfwd_joined == o.gfwd_joined &&
               early_ar == o.early_ar && staged_src == o.staged_src;
    }
};

// What one training step leaves in flight for the next C-ABI call.  Three kinds of code write it and no other: the entry
// points (their own bookkeeping), run_phase (commits a phase's PhaseResult -- eagerly after the enqueue, on every replay in
// graph mode) and invalidate() (whatever makes work in flight worthless).  The phase bodies only enqueue: they see the context
// as const, read carried state through their PhaseKey and report what they left behind in their PhaseResult.
//
//   field          set by                                    consumed by                              invalidated by
//   pending        *_grads (1 D, 2 G)                        *_apply (-> 0), set_step_variant         rebind
//   metrics_last   *_grads                                   *_apply (the step's one metrics buffer)  --
//   staged_B/_src  stage_real                                d_grads (-> 0), g_grads (pre_real)       rebind (src: with B)
//   dreal_B        g_grads that ran D(real) ahead            d_grads (pre_real 2, -> 0)               drop_dreal: every reason but comm
//   dreal_orphan   drop_dreal                                settle (next enqueue waits for ev_dreal) --
//   dreal_joined   phase G grads (16-bit: lane c joined)     phase D grads (-> 0)                     --
//   dreal_noise2   phase G grads (drew D(fake)'s tables)     phase D grads (-> 0)                     --
//   g_fwd_pending  step_begin (G forward enqueued)           g_grads (-> 0), D apply (riders)         --
//   gfwd_joined    phase D grads, phase D apply (riders)     phase G grads (-> 0)                     --
//   zg_stash       step_begin that could not pipeline        g_grads (-> 0)                           --
//   conv1_rode     D apply (riders ran block 1)              g_grads (-> 0)                           weights, rows, rebind
//   abl_masks      d_grads (ablation, explicit masks)        g_grads (-> 0)                           --
//   early_ar       phase D grads (tail all-reduce started)   phase D apply (-> 0)                     weights, rebind, comm
//   lP[2]          every d_forward_rows (phases, d_forward)  the next phase D grads (lP[0], pre_real 2)  --
//   g_r0           phase G grads                             debug_tensor("d_a_g")                    --
//   ga_last_B      every Generator forward                   debug_tensor("g_a", Lg)                  --
//   g_rode, g_pre_real  g_grads                              debug_tensor("rode" / "pre_real")        --
struct Carried {
    int pending;         // last *_grads call (for *_apply): 0 none, 1 D, 2 G
    float* metrics_last; // metrics target of the last *_grads call
    int staged_B;        // batch of a real batch staged for the NEXT D step by siggan_stage_real (0: none)
    const float* staged_src;   // where that batch lies: the caller's own tensor (borrowed until the D step that consumes it)
    int dreal_B;         // batch whose D(real) forward siggan_g_grads already enqueued on lane c (0: none)
    bool dreal_orphan;   // a D(real) forward enqueued on lane c was abandoned: the next enqueue waits for ev_dreal first
    bool dreal_joined;   // the lane of that early forward was already joined into the caller's stream (end of the G step)
    bool dreal_noise2;   // its launch also drew the dropout tables of the D(fake) pass
    int g_fwd_pending;   // batch of a Generator training forward already enqueued by siggan_step_begin (0: none)
    bool gfwd_joined;    // the pipelined Generator forward's lane was already joined into the caller's stream (end of the D grads phase)
    int zg_stash;        // batch of an explicit G-step z handed to siggan_step_begin when the forward was not pipelined
    int conv1_rode;      // batch whose first-Discriminator-block forward (workspace rows [B, 2B), updated weights) the last D apply ran
    bool abl_masks;      // ablation step: the D half was given explicit masks, the third set waits in mask_stage for the G half
    bool early_ar;       // the last D block's weight gradient is already being all-reduced on s_n (ev_ar marks its end)
    int lP[2];           // partial classifier dot products per image of workspace half h, left in lparts by the last block's
                         //   split-K epilogue (0: that half's logits are in `logits`, written by k_cls_fwd)
    int g_r0;            // first workspace row of the Discriminator pass of the last G step (0, or B: beside an early D(real))
    int ga_last_B;       // batch of the last TRAINING Generator forward: the last block's activation was not materialised
                         // (siggan_debug_tensor("g_a", Lg) forms it on demand)
    int g_rode, g_pre_real;    // what the last siggan_g_grads did (test hook "rode" / "pre_real"): batch whose first-block rows
                               // the riders had run (0: none), batch whose D(real) it started ahead (0: none)
};
// The carried fields a phase body produces; < 0: the phase left that one as it was.
struct PhaseResult {
    int early_ar = -1, dreal_joined = -1, dreal_noise2 = -1, gfwd_joined = -1, g_r0 = -1, ga_last_B = -1, lP[2] = {-1, -1};
};
struct CachedPhase { PhaseKey key; hipGraphExec_t exec; PhaseResult res; };

// What the kernels read besides a parameter arena is derived from it, and THIS is where that is said: one record per arena
// tensor (or adjacent pair of tensors), in arena order, covering the whole arena.  Both job tables are built from the list --
// prep_table for k_prepare / k_prepare_conv1 (graph mode, fp16, spectral norm, after siggan_params_changed) and ap_table for
// k_adam_pack (the eager update that rebuilds the derived state in its own launch) -- so a derived tensor is on both paths or
// on neither.  build_layout fills in shapes and offsets, siggan_create the destinations and whether the network's update can
// be the packed one; pointers that exist only after siggan_bind (arenas, running statistics) are resolved per table.
//   DV_FLAT  nothing derived: the Discriminator's biases
//   DV_FC    Generator.fc weight [F][A] + bias, Bc = C0 -> dst: the k-major copy of the generic fc kernel (null when fc_fused)
//   DV_CONV  weight [A][Bc][4][4] -> dst: the down pack (O = A, I = Bc), dst2: the up pack (I = A, O = Bc), element type dt.
//            The same for the Generator's (Cin, Cout) and the Discriminator's (Cout, Cin) layout: a forward pass contracts
//            Cin, so G runs on the up pack and D on the down pack, and each input-gradient on the other one
//   DV_BN    gamma + beta of A channels, Bc = perm_c0, running statistics at bn_off -> dst: [scale | shift | mean | rstd]
//   DV_TAPS  one-channel convolution weight [A][Bc taps] + bias (k_adam_pack: both ranges belong to ONE workgroup, the one
//            the riders wait on) -> dst: [tap][c]; dst2 (spectral norm): an fp32 scaled copy in the weight's own layout
//   DV_T16   classifier weight [A][16] -> dst: [16][A], the last block's NHWC order
enum DvKind : int { DV_FLAT = 0, DV_FC, DV_CONV, DV_BN, DV_TAPS, DV_T16 };
struct Derived {
    int kind, layer, A, Bc;      // layer: the block; a Discriminator weight's spectral-norm layer is layer - 1
    int64_t off, n, off2, n2;    // arena span of the tensor and of the second one of a pair (bias / beta; n2 = 0: none)
    int64_t bn_off;              // BN: offset of the layer's running statistics
    float *dst, *dst2;
};

struct siggan_ctx {
    siggan_config cfg;
    int S, latent, Lg, Ld, Bm;
    int dt;             // element type of the activation / gradient tensors and of the MFMA weight packs (act.h)
    size_t es;          // its size in bytes
    bool sn;            // spectral normalisation of every Discriminator weight (sn.hip)
    SnTable snt;        // its layer table (pointers into the bound arenas are refreshed by siggan_bind)
    float *sn_tbuf, *sn_wbuf, *sn_sig, *sn_us, *sn_vs, *sn_dots, *sn_g[2], *d_w1s;
    int variant;        // SIGGAN_STEP_TRAINER / SIGGAN_STEP_ABLATION (siggan_set_step_variant)
    bool fc_fused;      // Generator.fc runs as the one-launch MFMA kernels of fc.hip (max_batch <= 256, latent % 4 == 0)
    float gscale;       // gradient scale of the backward chains (fp16: keeps small gradients out of the subnormals; else 1)
    int gC[MAXL + 1];   // generator channel chain gC[0..Lg]  (generator_vanilla_gan.py:131-149)
    int dC[MAXL + 1];   // discriminator chain dC[0]=1, dC[1..Ld] (discriminator_vanilla_gan.py:131-194)
    int F;              // gC[0]*16
    // flat-arena spans (offset, numel) in parameters() order
    std::vector<int64_t> g_off, g_num, d_off, d_num;
    int64_t g_total, d_total, bn_total;
    int64_t g_bn_off[MAXL + 1];
    std::vector<Derived> rec[2];   // what is derived from each arena ([0] G, [1] D)
    bool packable[2];   // the network's eager update can be k_adam_pack: fc_fused, channel counts the 16 x 16 tiles divide,
                        // one-channel convs that fit one workgroup, no spectral norm (the packs then follow sigma, not the update)
    siggan_storage st;
    bool bound;
    bool g_dirty, d_dirty;
    // workspace
    char* ws; size_t ws_bytes;
    // (element type dt: fc_y, g_y, g_a, g_da, d_a, d_dv and the MFMA weight packs g_up, g_dn, d_dn, d_up; fp32: the rest)
    float *z, *g_bn[MAXL + 1], *g_bne[MAXL + 1];
    char *fc_y, *g_y[MAXL + 1], *g_a[MAXL + 1], *g_da[MAXL + 1];
    char *g_ae[MAXL + 1];     // 16-bit contexts: activations of the EVAL-mode Generator forward (it runs beside the training forward)
    float *img, *dpre;
    char *d_a[MAXL + 1], *d_dv[MAXL + 1];
    float *d_noise[MAXL + 1];
    float *logits, *probs, *dlogit;
    float* lparts;       // partial classifier dot products left by the last block's split-K epilogue (Carried::lP per image)
    char *g_up[MAXL + 1], *g_dn[MAXL + 1], *d_dn[MAXL + 1], *d_up[MAXL + 1];
    float *wcp;
    float *slab, *slab_k, *slab_k2, *slab_k3, *partial, *partial_b, *partial_c, *z_g, *img_g, *metrics, *zeros, *wfc_t, *wfin_t, *d_w1t, *real_stage, *mask_stage;
    float* deq_lut;      // the 256 dequantised byte values (siggan_dequant_table), read by siggan_d_score_u8's first block
    float* ones;         // 64 floats of 1.0f: a BatchNorm scale row that leaves a gradient as it is (siggan_g_param_grad)
    float* lg_tab;       // siggan_g_latent_grad: per-image copies [B][C_l] of the eval-mode BatchNorm scale rows of blocks 1 .. Lg-1
    char *op_pack;
    int64_t slab_floats, slab_k_floats;
    DevState* dev;
    Carried cs;          // what is in flight between two calls (the table above)
    // lanes / graphs
    static constexpr int NEV = 96;
    int mode;
    hipStream_t s_m, s_a, s_b, s_c, s_n;      // s_n: the lane of an all-reduce issued while the backward pass is still running
    hipEvent_t ev_gfwd, ev_dreal, ev_ar, ev_sys[2];
    hipError_t lane_err; // first failed event record / wait of a fork or join (checked after every phase)
    const char* refused; // sticky: a launcher refused a launch of a step (nothing was enqueued for it; lane_check reports it)
    // data-parallel communicator (siggan_comm_init): world 1 = none
    ncclComm_t comm; int comm_rank, comm_world; int comm_err;
    float* slab_b;       // second weight-gradient slab region (a weight gradient on the main lane beside lane a's)
    float* ride_ctr;     // k_adam_pack's rider count (one word, zero between launches)
    unsigned* ride_late; // host-visible, sticky: a k_adam_pack owner stopped waiting for its riders (lane_check reports it)
    unsigned* ride_late_dev;   // (the same word as the device addresses it)
    double adam_t[2];    // step count of the network's Adam state as the HOST knows it ([0] G, [1] D); valid while adam_t_known
    bool adam_t_known[2];// (reset by siggan_bind / siggan_params_changed: the caller may have written the step tensors)
    hipEvent_t ev[NEV], ev_fenced[NEV], ev_bridge[2];   // ev_fenced: the same ring with the system-scope fence (used while a communicator exists)
    int evi;
    std::vector<CachedPhase> graphs;
};

// parameter tensor indices
static inline int gi_fc_w() { return 0; }
static inline int gi_fc_b() { return 1; }
static inline int gi_bn0_w() { return 2; }
static inline int gi_bn0_b() { return 3; }
static inline int gi_up_w(int l) { return 4 + 3 * (l - 1); }       // l = 1..Lg
static inline int gi_bn_w(int l) { return l == 0 ? 2 : 5 + 3 * (l - 1); }
static inline int gi_bn_b(int l) { return l == 0 ? 3 : 6 + 3 * (l - 1); }
static inline int gi_fin_w(const siggan_ctx* c) { return 4 + 3 * c->Lg; }
static inline int gi_fin_b(const siggan_ctx* c) { return 5 + 3 * c->Lg; }
static inline int di_w(int l) { return 2 * (l - 1); }              // l = 1..Ld
static inline int di_b(int l) { return 2 * (l - 1) + 1; }
static inline int di_cls_w(const siggan_ctx* c) { return 2 * c->Ld; }
static inline int di_cls_b(const siggan_ctx* c) { return 2 * c->Ld + 1; }

#define GP(c, i) ((c)->st.g_params + (c)->g_off[i])
#define GG(c, i) ((c)->st.g_grads + (c)->g_off[i])
#define DP(c, i) ((c)->st.d_params + (c)->d_off[i])
#define DG(c, i) ((c)->st.d_grads + (c)->d_off[i])

// The ONE place that says what an outside event makes worthless.  The ORDER matters: each reason down to INV_STREAM also
// drops everything the reasons below it drop (the switch falls through), so a field added to one reason is dropped by every
// reason above it as well -- put it at the lowest reason that must drop it.
enum Inval {
    INV_INIT,      // siggan_create: nothing in flight, nothing derived from the arenas yet
    INV_REBIND,    // siggan_bind: ... a pending *_apply and a staged batch belonged to the old arenas
    INV_WEIGHTS,   // siggan_params_changed: ... packs / eval tables are stale, the caller may have written the Adam step tensors,
                   //   an early all-reduce whose apply never ran is abandoned with the gradients it covered
    INV_ROWS,      // siggan_d_forward: ... the rows of a first-block forward the last D apply ran ahead are overwritten (or used old weights)
    INV_STREAM,    // siggan_seed (dropout tables drawn from the old RNG stream) / siggan_stage_real (the staged batch is replaced):
                   //   a D(real) forward started ahead of time is abandoned
    INV_COMM,      // siggan_comm_destroy: only the early all-reduce
};

// lanes: where a phase enqueues its kernels.  m is the main lane; a and b are side lanes that run
// independent work (weight gradients, bias / BatchNorm reductions) beside the main chain.  With
// overlap off all three are the same stream and fork/join are no-ops.  Forks and joins are plain
// event record / wait pairs, so the same code runs eagerly and under stream capture (hipGraph).
// Lanes is also the one door through which an enqueue writes the context -- the event ring's index and the sticky
// diagnostics lane_err / refused / comm_err; the passes see everything else as const.
class Lanes {
    siggan_ctx* c;
public:
    Lanes(siggan_ctx* c_, hipStream_t m_, hipStream_t a_, hipStream_t b_, bool ext_) : c(c_), m(m_), a(a_), b(b_), ext(ext_), tail_wait(nullptr) {}
    Lanes(siggan_ctx* c_, hipStream_t s) : Lanes(c_, s, s, s, false) {}       // one stream: the entry points outside a step
    hipStream_t m, a, b;
    // ext: a fork may ride on the producing kernel's own completion signal (ops.h, SIGGAN_LAUNCH_EV) instead of a marker packet
    // behind it -- eager launches only (not under stream capture, not with the profiler's own events on the launch)
    bool ext;
    hipEvent_t tail_wait;        // d_backward_pass: one more event the main lane waits for where it is idle anyway (before its last join)
    // the event to hand the producing launch as `done` (nullptr: fork_after records one the classic way)
    hipEvent_t fork_event(hipStream_t to) { return (ext && to != m) ? next() : nullptr; }
    void fork_after(hipStream_t to, hipEvent_t done) {      // `to` waits for the launch that was given `done` (and all before it on m)
        if (to == m) return;
        if (done) note(hipStreamWaitEvent(to, done, 0)); else fork(to);
    }
    // with a communicator every lane event keeps its system-scope fence: peers read this device's gradient arena over xGMI
    hipEvent_t next() { hipEvent_t e = (c->comm ? c->ev_fenced : c->ev)[c->evi]; c->evi = (c->evi + 1) % siggan_ctx::NEV; return e; }
    void fork(hipStream_t to) {          // `to` waits for everything enqueued on m so far
        if (to == m) return;
        hipEvent_t e = next();
        note(hipEventRecord(e, m)); note(hipStreamWaitEvent(to, e, 0));
    }
    void join(hipStream_t from) {        // m waits for everything enqueued on `from`
        if (from == m) return;
        hipEvent_t e = next();
        note(hipEventRecord(e, from)); note(hipStreamWaitEvent(m, e, 0));
    }
    // a failed record / wait would silently drop an ordering edge: remember the first one, run_phase reports it
    void note(hipError_t e) { if (e != hipSuccess && c->lane_err == hipSuccess) c->lane_err = e; }
    void refuse(const char* why) { c->refused = why; }       // a launcher refused a launch (sticky, lane_check)
    void comm_fail(int rc) { c->comm_err = rc; }             // a collective failed (sticky until siggan_comm_destroy)
    void record(hipEvent_t e, hipStream_t s) { note(hipEventRecord(e, s)); }
    void wait(hipStream_t s, hipEvent_t e) { note(hipStreamWaitEvent(s, e, 0)); }
};

struct WgradCall { WgradArgs w; int max_splits; };
struct BceSpec { int n0; float y0, y1; float* mt; int is_g; };   // rows < n0: target y0, the rest y1 (each segment's mean)
// What g_forward_pass takes beyond its tensors; the defaults are the plain eval-mode forward.
struct GFwdOpt {
    bool training = false;
    float *partial = nullptr, *slab_k = nullptr;   // a pass beside another one: its own BatchNorm partials / split-K slab (null: c->partial / c->slab_k)
    uint32_t rng_sid = 0; float* z_out = nullptr;  // z == nullptr: the latent batch is drawn inside the fc kernel from this RNG stream and left in z_out
    hipEvent_t done = nullptr;                     // completion event of the pass' last launch
    uint8_t* u8 = nullptr; int32_t* stats = nullptr; float thr = 0.f;    // eval only: see launch_final_fwd
    bool keep_y = false;   // eval only (siggan_g_param_grad): the blocks run in the training forward's shape -- raw GEMM output kept
};                         // in g_y[l], then the apply with the EVAL table -- no statistics
// ... and d_forward_rows; the defaults are the eval-mode forward of fp32 images with stored logits.
struct DFwdOpt {
    bool dropout = false;
    bool fuse_cls = false;      // the classifier's dot product rides in the last block's split-K epilogue where it can
    bool conv1_done = false;    // the first block already ran (it rode in the launch that re-packed D's weights, see repack)
    const uint8_t* u8 = nullptr; int binarize = -1; float* x_out = nullptr;   // siggan_d_score_u8: the first block fed from bytes
};

namespace siggan {       // siggan.hip, then passes.hip
void drop_dreal(siggan_ctx* c);
int settle(siggan_ctx* c, hipStream_t s);
void invalidate(siggan_ctx* c, Inval why);
int check_bn_batch(const siggan_ctx* c, int batch);
int check_call(siggan_ctx* c, int batch, bool need_bound = true);
int lane_check(siggan_ctx* c);
void repack(const siggan_ctx* c, Lanes& L, hipStream_t sg, hipStream_t sd, bool do_g, bool do_d, int sn_slot = 0, const float* conv1_x = nullptr,
            int conv1_r0 = 0, int conv1_B = 0);
void ap_table(const siggan_ctx* c, int which, int nride, ApTable& t);
GConvArgs gconv_args(const siggan_ctx* c, int form, int B, int h_in, int c_in, int c_out);
WgradCall wgrad_args(const siggan_ctx* c, const void* small, const void* large, float* dw, float* slab, int B, int h_small, int c_small, int c_large);
int g_forward_pass(const siggan_ctx* c, const float* z, int B, float* img, hipStream_t s, const GFwdOpt& o = GFwdOpt());
int d_forward_rows(const siggan_ctx* c, const float* x, int r0, int nB, hipStream_t s, float* slab_k, const DFwdOpt& o = DFwdOpt());
bool d_backward_pass(const siggan_ctx* c, Lanes& L, const float* x0, int n0, const float* x1, int Bd, bool dropout, bool want_wgrad,
                     bool want_dimage, const BceSpec& bce, int P, int r0 = 0, float* garena = nullptr, bool early_allreduce = false);
void g_backward_pass(const siggan_ctx* c, Lanes& L, const float* z, int B);
void make_noise(const siggan_ctx* c, const float* masks, int B, int p0, int p1, hipStream_t s, uint32_t ctr_add = 0);
void objective_seeds(siggan_ctx* c, const float* img, int B, const uint8_t* target_u8_dev, const float* target_f32_dev, float wr, float wd,
                     float* realism, float* probs_dev, hipStream_t s);
int check_hyper(const siggan_hyper* hp);   // step.hip
}  // namespace siggan
