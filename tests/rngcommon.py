"""The library's counter-based RNG (csrc/rng.h) restated in numpy, independent of the kernels: Philox4x32-10 in uint64 with
masks, the counter / key layout of draw_raw, u01 in float32 with the kernel's three operations, the keep decision, and
Box-Muller in float64 (the yardstick) and in float32 numpy (only to size the parity bound).  SITES says which stream id,
element index and call counter every consumer uses; the constants below it are the (seed, offset, shape) cases the GPU tests run,
shared with the CPU tests that show those cases can tell a mistaken generator from the right one."""
from collections import namedtuple

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
F32 = np.float32
TWO_PI = 6.283185307179586


def _u64(a):
    """int or integer array (values below 2^64) -> uint64 array"""
    if isinstance(a, (int, np.integer)):
        return np.asarray(int(a) & 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    return np.asarray(a).astype(np.uint64)


def philox4x32_10(counter4, key2, rounds=10):
    """Philox4x32 (Salmon et al., SC'11; Random123): counter4 = four and key2 = two 32-bit words (ints or arrays that
    broadcast).  Returns uint32 of shape (..., 4)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_u64(c) & M32 for c in counter4])
    k0, k1 = _u64(key2[0]) & M32, _u64(key2[1]) & M32
    for _ in range(rounds):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2                   # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def draw_raw(seed, ctr, idx, sid, rounds=10, key_high=True):
    """The four words of group idx of stream sid at call counter ctr: counter = (idx lo, idx hi, sid, ctr lo),
    key = (seed lo, seed hi ^ ctr hi).  rounds / key_high=False build the mutants of test_rng_cpu."""
    seed, ctr, idx = _u64(seed), _u64(ctr), _u64(idx)
    hi = ((seed >> np.uint64(32)) ^ (ctr >> np.uint64(32))) if key_high else np.uint64(0)
    return philox4x32_10((idx & M32, idx >> np.uint64(32), sid, ctr & M32), (seed & M32, hi), rounds)


def u01(x):
    """((float)(x >> 8) + 0.5f) * 2^-24 in float32, one rounding per operation as on the device (no contraction: an add
    followed by a multiply is no fma).  Range [2^-25, 1.0]: from x >> 8 = 2^23 on the sum needs 25 bits and rounds to even,
    so 0xFFFFFF + 0.5 becomes 2^24 and u01 reaches exactly 1.0f."""
    t = (np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(F32)
    return (t + F32(0.5)) * F32(1.0 / 16777216.0)


def words(seed, ctr, sid, e0, n, **mut):
    """Raw words of elements [e0, e0 + n) of a stream (element e = word e & 3 of group e >> 2), uint32 of shape (n,).
    mut: rounds=, key_high=, group_add= (mutants)."""
    group_add = mut.pop("group_add", 0)
    g0, g1 = e0 >> 2, (e0 + n + 3) >> 2
    w = draw_raw(seed, ctr, np.arange(g0, g1, dtype=np.uint64) + np.uint64(group_add), sid, **mut).reshape(-1)
    return w[e0 - 4 * g0:e0 - 4 * g0 + n]


def keep(seed, ctr, i, sid, keep_prob_f32, strict=True, **mut):
    """Keep decision of element(s) i of a dropout site: u01(word i & 3 of group i >> 2) < keep (strict=False: the <= mutant)."""
    i = _u64(i)
    w = draw_raw(seed, ctr, (i >> np.uint64(2)) + np.uint64(mut.pop("group_add", 0)), sid, **mut)
    u = np.take_along_axis(w, (i & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]
    return u01(u) < F32(keep_prob_f32) if strict else u01(u) <= F32(keep_prob_f32)


def keep_range(seed, ctr, sid, e0, n, keep_prob_f32, strict=True, **mut):
    """keep() of the contiguous elements [e0, e0 + n)."""
    u = u01(words(seed, ctr, sid, e0, n, **mut))
    return u < F32(keep_prob_f32) if strict else u <= F32(keep_prob_f32)


def normal4(w):
    """The yardstick: Box-Muller in float64 on the exact float32 u values of raw words w (..., 4):
    (r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1), r = sqrt(-2 ln u(x or z)), a = 2 pi u(y or w)."""
    u = u01(w).astype(np.float64)
    r0, r1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    a0, a1 = TWO_PI * u[..., 1], TWO_PI * u[..., 3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)


def normal4_f32(w):
    """The same formula with every operation in numpy float32: how far float32 arithmetic alone strays from normal4 (the
    d32 of the parity bound).  Not a model of the device's v_log / v_sin / v_cos."""
    u = u01(w)
    r0, r1 = np.sqrt(F32(-2.0) * np.log(u[..., 0])), np.sqrt(F32(-2.0) * np.log(u[..., 2]))
    a0, a1 = F32(TWO_PI) * u[..., 1], F32(TWO_PI) * u[..., 3]
    out = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)
    assert out.dtype == np.float32
    return out


def normals(seed, ctr, sid, n, f32=False, **mut):
    """Elements [0, n) of a normal stream: what k_randn writes for launch_randn(out, n, sid) at counter ctr."""
    group_add = mut.pop("group_add", 0)
    w = draw_raw(seed, ctr, np.arange((n + 3) >> 2, dtype=np.uint64) + np.uint64(group_add), sid, **mut)
    return (normal4_f32 if f32 else normal4)(w).reshape(-1)[:n]


# ---- who draws what ---------------------------------------------------------------------------------------------------------
SID_Z, SID_ZG, SID_RANDN, SID_DROP0 = 1, 2, 3, 16                 # Discriminator block l (1-based) draws stream 16 + l
SID_FC1, SID_FC2, SID_CLS = 0x56540001, 0x56540002, 0x56540003    # verifier trainer: fc dropout of x1, of x2, classifier
KEEP_D = F32(1.0) - F32(0.25)                                     # Engine's default dropout = 0.25
KEEP_FC, KEEP_CLS = F32(1.0) - F32(0.5), F32(1.0) - F32(0.3)      # verifier_train.hip: 1.0f - P_FC, 1.0f - P_CLS
VFC1_N, VHID = 512, 64

Site = namedtuple("Site", "sid counter element value")
# counter: in terms of c, the context's call counter when the call starts (seed(s, o) sets c = o; every optimiser update,
# siggan_op_randn and a mask-less training siggan_d_forward add one); the verifier trainer's counter is offset + k, k the
# number of _grads / _step calls since the seed call, with or without masks handed in.
SITES = {
    "engine.z": Site(SID_Z, "c of the D phase (siggan_d_grads / siggan_step_begin)", "row * latent + col",
                     "normal; the eval-mode forward of the D step"),
    "engine.z_g": Site(SID_ZG, "c of the D phase when pipelined (siggan_step_begin, batch > 1); c of siggan_g_grads when that "
                       "call runs the forward itself (then one more than its D step's, and the values land in the 'z' buffer)",
                       "row * latent + col", "normal; the G step's training forward"),
    "op_randn": Site(SID_RANDN, "c + 1 (ticks first)", "t", "normal"),
    "d_dropout": Site("16 + l", "c of the D phase, passes 0 and 1; a G phase that stages the next real batch draws the NEXT D "
                      "step's tables ahead at c + 1 (= that step's c); training siggan_d_forward without masks: c + 1 "
                      "(ticks first), pass 0 only",
                      "pass * B * dC[l] + row * dC[l] + channel (pass 0 = D(real), 1 = D(fake))",
                      "1.0f / keep if u01 < keep else 0, keep = 1.0f - dropout"),
    "verifier.fc_x1": Site(SID_FC1, "offset + k", "row * 512 + j", "u01 < 1.0f - 0.5f"),
    "verifier.fc_x2": Site(SID_FC2, "offset + k", "(row - n_pairs) * 512 + j", "u01 < 1.0f - 0.5f"),
    "verifier.cls": Site(SID_CLS, "offset + k", "pair * 64 + j", "u01 < 1.0f - 0.3f"),
}

Draw = namedtuple("Draw", "site sid ctr e0 n")


def engine_step_draws(c, batch, latent, d_chans, staged=False):
    """Every draw of one Engine.train_step whose call counter starts at c (pipelined: z_g is drawn in the D phase; staged:
    next_real given, so the G phase also draws the next step's tables at that step's counter c + 2)."""
    out = [Draw("engine.z", SID_Z, c, 0, batch * latent), Draw("engine.z_g", SID_ZG, c, 0, batch * latent)]
    for when in ([c, c + 2] if staged else [c]):
        for l, ch in enumerate(d_chans, 1):
            for p in (0, 1):
                out.append(Draw(f"d_dropout[{l}] pass {p}", SID_DROP0 + l, when, p * batch * ch, batch * ch))
    return out


def trainer_step_draws(offset, k, n_pairs):
    c = offset + k
    return [Draw("verifier.fc_x1", SID_FC1, c, 0, n_pairs * VFC1_N), Draw("verifier.fc_x2", SID_FC2, c, 0, n_pairs * VFC1_N),
            Draw("verifier.cls", SID_CLS, c, 0, n_pairs * VHID)]


def randn_draws(c, n):
    return [Draw("op_randn", SID_RANDN, c + 1, 0, n)]


# ---- restated outputs of the calls the GPU tests make -------------------------------------------------------------------------
def trainer_masks(seed, ctr, n_pairs, strict=True, sid_add=0, **mut):
    """(fc_keep (2n, 512), cls_keep (n, 64)) as uint8 0 / 1 of a verifier train call at counter ctr."""
    fc = [keep_range(seed, ctr, sid + sid_add, 0, n_pairs * VFC1_N, KEEP_FC, strict, **dict(mut)) for sid in (SID_FC1, SID_FC2)]
    cls = keep_range(seed, ctr, SID_CLS + sid_add, 0, n_pairs * VHID, KEEP_CLS, strict, **dict(mut))
    return np.concatenate(fc).reshape(2 * n_pairs, VFC1_N).astype(np.uint8), cls.reshape(n_pairs, VHID).astype(np.uint8)


def d_noise(seed, ctr, layer, batch, ch, passes=(0, 1), keep_prob=KEEP_D, strict=True, sid_add=0, **mut):
    """Rows of Discriminator block `layer`'s multiplier table for the given passes, float32 (len(passes) * batch, ch)."""
    inv = F32(1.0) / F32(keep_prob)
    rows = [keep_range(seed, ctr, SID_DROP0 + layer + sid_add, p * batch * ch, batch * ch, keep_prob, strict, **dict(mut)) for p in passes]
    return np.where(np.concatenate(rows), inv, F32(0.0)).astype(np.float32).reshape(len(passes) * batch, ch)


# ---- the GPU tests' cases -------------------------------------------------------------------------------------------------------
# (seed, offset, steps): a plain pair; a seed with a high half; a counter whose second step is 2^32 (the low counter word
# wraps to 0 and the key's high word flips a bit)
SEEDS = [(1234, 5, 1), ((1 << 32) + 7, 0, 1), (9, (1 << 32) - 1, 2)]
TRAINER_E, TRAINER_PAIRS = 40, (1, 3, 33)                       # one row per half, an odd count, more than one 64-row tile
NOISE_SIZE, NOISE_LATENT, NOISE_BATCHES = 64, 100, (3, 16)
D_CHANS = (64, 128, 256, 512)                                   # layout.D_CHAIN[64]
LATENT_BATCHES, LATENT_FALLBACK = (2, 5, 64), 257               # the fused fc kernel; the generic kernel (max_batch > 256)
LATENT_SEED = (77, 3)
RANDN_N = (1, 2, 3, 5, 4099)
RANDN_SEED = (4321, 9)

# ---- planted edges (profiles/rng_edge_search.py found them; test_rng_cpu re-verifies each in O(1)) ---------------------------
# op_randn after Engine.seed(seed, offset) draws at counter offset + 1.  element: the first normal of the half-group whose
# radius word has x >> 8 == 0xFFFFFF (u01 == 1.0, radius 0), == 0 (u01 == 2^-25, radius sqrt(50 ln 2)), resp. == 0xFFFFFD or
# 0xFFFFFE (u01 == 1 - 2^-23, the largest value below 1: log must come out negative, radius about 2^-11).
#   python profiles/rng_edge_search.py
EDGE_U_ONE = dict(seed=7464, offset=0, element=2020)
EDGE_U_MIN = dict(seed=1350, offset=0, element=3088)
EDGE_U_TOP = dict(seed=69, offset=0, element=938)
EDGE_N = 4096
# verifier trainer, n_pairs = 3: an fc element with x >> 8 == 0x800000, i.e. u01 == 0.5f == keep exactly (dropped by <, kept
# by the <= mutant): site 0 = x1, 1 = x2
EDGE_KEEP_TIE = dict(seed=1732, offset=0, n_pairs=3, site=0, element=30)
