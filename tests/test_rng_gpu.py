"""The device RNG (csrc/rng.h) held to its numpy restatement (rngcommon.py): every consumer listed in rngcommon.SITES draws the
bits, from the stream, element and call counter that table says.

Keep masks and dropout tables are compared for exact equality (Philox is integer arithmetic, u01 and the comparison are
exact in IEEE float32).  Normals are compared with Box-Muller in float64 on the restated words; the bound is the project's
rule (verifiercommon): absolute min(32 x d32, 1e-4), d32 the largest deviation of the same formula in numpy float32 from
float64 over the same draws -- the float32 angle alone carries 2^-24 x 2 pi of phase error on a radius of up to 5.9, so d32
is about 1e-6.  profiles/rng_parity.py records every such comparison (profiles/rng_parity.json)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rngcommon as R
import verifiertraincommon as TC
from common import I, SEED
from verifiertraincommon import TI, VC

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd import signature_verifier_eval as SV
from signature_gan_amd import signature_verifier_train as ST

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PARITY = None                                          # profiles/rng_parity.py collects the comparisons here
SEED_IDS = ["plain", "seed-high-half", "counter-crosses-2^32"]


# ---- a. verifier trainer masks --------------------------------------------------------------------------------------------------
class Rig:
    """A verifier trainer on caller-owned arenas loaded with verifier_inputs' state (the Rig of test_verifier_train_gpu)."""

    def __init__(self, e, n_pairs):
        self.n = n_pairs
        self.t = ST._Trainer(DEV, e, n_pairs)
        P, Rn = TC.state(e, torch.float32)
        self.arenas = [torch.zeros(self.t.count, dtype=torch.float32, device=DEV) for _ in range(4)]
        for (off, n), k in zip(self.t.spans, P):
            self.arenas[0][off:off + n].copy_(P[k].reshape(-1))
        self.running = [Rn[k].to(DEV).contiguous() for k in TI.running_names()]
        self.t.bind(self.arenas, self.running, VC.BN_EPS, 0)
        b = TC.case_batch(n_pairs, torch.float32)
        self.batch = {k: v.to(DEV).contiguous() for k, v in b.items()}

    def grads(self, masks=False):
        b, p = self.batch, SV._ptr
        fk, ck = (b["fc_keep"], b["cls_keep"]) if masks else (None, None)
        m = torch.zeros(4, dtype=torch.float32, device=DEV)
        _lib.check(self.t.lib.siggan_verifier_train_grads(self.t._h, p(b["x1"]), p(b["x2"]), _lib.VFMT_F32, p(b["labels"]), self.n,
                                                          p(fk), p(ck), 1, p(m), self.t.stream()))
        return self.t.debug("fc_keep", (2 * self.n, 512)).cpu().numpy(), self.t.debug("cls_keep", (self.n, 64)).cpu().numpy()

    def close(self):
        self.t.close()


def _same_masks(got, want, what):
    for name, g, w in zip(("fc_keep", "cls_keep"), got, want):
        assert g.shape == w.shape and g.dtype == np.uint8
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what} {name}: {len(bad)} of {g.size} decisions differ, first at {bad[0].tolist()}"


@pytest.mark.parametrize("seed,offset,steps", R.SEEDS, ids=SEED_IDS)
@pytest.mark.parametrize("n_pairs", R.TRAINER_PAIRS)
def test_trainer_masks(n_pairs, seed, offset, steps):
    rig = Rig(R.TRAINER_E, n_pairs)
    try:
        rig.t.seed(seed, offset)
        for k in range(steps):
            _same_masks(rig.grads(), R.trainer_masks(seed, offset + k, n_pairs), f"n_pairs {n_pairs} counter {offset + k}")
    finally:
        rig.close()


def test_trainer_counter_advances_past_a_call_with_masks():
    n, (seed, offset, _) = 3, R.SEEDS[0]
    rig = Rig(R.TRAINER_E, n)
    try:
        rig.t.seed(seed, offset)
        given = rig.grads(masks=True)
        _same_masks(given, (TI.fc_keep(n).astype(np.uint8), TI.cls_keep(n).astype(np.uint8)), "handed in")
        _same_masks(rig.grads(), R.trainer_masks(seed, offset + 1, n), "drawn after a call with masks")
    finally:
        rig.close()


def test_trainer_keep_is_strict_at_a_tie():
    """The planted seed has one fc element whose u01 equals the keep probability 0.5f exactly: `<` drops it."""
    e = R.EDGE_KEEP_TIE
    rig = Rig(R.TRAINER_E, e["n_pairs"])
    try:
        rig.t.seed(e["seed"], e["offset"])
        got = rig.grads()
        _same_masks(got, R.trainer_masks(e["seed"], e["offset"], e["n_pairs"]), "planted tie")
        assert got[0][e["site"] * e["n_pairs"] + e["element"] // 512, e["element"] % 512] == 0
    finally:
        rig.close()


# ---- b. Discriminator dropout tables ------------------------------------------------------------------------------------------
def _engine(batch, warm=True):
    from hipcommon import make_engine
    return make_engine(R.NOISE_SIZE, R.NOISE_LATENT, batch, warm=warm)


def _real(batch, seed=SEED["real"]):
    return torch.from_numpy(I.gen_real(batch, R.NOISE_SIZE, seed)).to(DEV)


def _tables(eng, batch):
    return [eng.debug_tensor("d_noise", l, (2 * batch, ch)).cpu().numpy() for l, ch in enumerate(R.D_CHANS, 1)]


def _same_tables(got, seed, ctr, batch, rows, passes, what):
    for l, ch in enumerate(R.D_CHANS, 1):
        g, w = got[l - 1][rows], R.d_noise(seed, ctr, l, batch, ch, passes=passes)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what} block {l}: {len(bad)} of {g.size} entries differ, first at {bad[0].tolist()}"


NOISE_CASES = [(R.NOISE_BATCHES[0],) + s for s in R.SEEDS] + [(R.NOISE_BATCHES[1],) + R.SEEDS[0]]


@pytest.mark.parametrize("batch,seed,offset,steps", NOISE_CASES, ids=[f"b{c[0]}-{i}" for c, i in zip(NOISE_CASES, SEED_IDS + SEED_IDS[:1])])
def test_d_step_tables(batch, seed, offset, steps):
    eng, real = _engine(batch), _real(batch)
    try:
        assert tuple(eng.d_chans) == R.D_CHANS and eng.dropout == 0.25
        eng.seed(seed, offset)
        for k in range(steps):
            eng.d_step(real)
            _same_tables(_tables(eng, batch), seed, offset + k, batch, slice(None), (0, 1), f"d_step at counter {offset + k}")
            assert eng.rng_state() == (seed, offset + k + 1)
        # a training forward without masks ticks, then draws pass 0 only: rows [B, 2B) stay the last step's
        eng.d_forward(real, training=True)
        got = _tables(eng, batch)
        _same_tables(got, seed, offset + steps + 1, batch, slice(0, batch), (0,), "d_forward(training)")
        _same_tables(got, seed, offset + steps - 1, batch, slice(batch, None), (1,), "rows [B, 2B) after d_forward(training)")
        assert eng.rng_state() == (seed, offset + steps + 1)
    finally:
        eng.close()


def test_staged_step_tables_and_latents():
    """train_step(real, next_real=real2): the G step draws the next D step's tables ahead, at that step's counter (this
    step's + 2: one tick per update); the next step uses them, and draws nothing else into the table."""
    batch, (seed, offset, _) = R.NOISE_BATCHES[0], R.SEEDS[0]
    eng, real, real2 = _engine(batch), _real(batch), _real(batch, SEED["real"] + 1)
    try:
        eng.seed(seed, offset)
        eng.train_step(real, next_real=real2)
        assert int(eng.debug_tensor("pre_real", 0, (1,)).item()) == batch, "the G step did not stage the next D(real) forward"
        got = _tables(eng, batch)
        _same_tables(got, seed, offset + 2, batch, slice(0, batch), (0,), "drawn ahead, D(real)")
        _same_tables(got, seed, offset + 2, batch, slice(batch, None), (1,), "drawn ahead, D(fake)")
        n = batch * R.NOISE_LATENT
        for name, sid in (("z", R.SID_Z), ("z_g", R.SID_ZG)):           # pipelined: both drawn in the D phase, counter offset
            _check_normals(f"staged step 1 {name} b{batch}", eng.debug_tensor(name, 0, (n,)), seed, offset, sid, n)
        eng.train_step(real2)
        _same_tables(_tables(eng, batch), seed, offset + 2, batch, slice(None), (0, 1), "the staged step")
        for name, sid in (("z", R.SID_Z), ("z_g", R.SID_ZG)):
            _check_normals(f"staged step 2 {name} b{batch}", eng.debug_tensor(name, 0, (n,)), seed, offset + 2, sid, n)
        assert eng.rng_state() == (seed, offset + 4)
    finally:
        eng.close()


# ---- c. latents and op_randn ---------------------------------------------------------------------------------------------------
def _check_normals(case, got, seed, ctr, sid, n):
    """got: n device normals of stream sid at counter ctr, against float64 Box-Muller of the restated words."""
    got = got.detach().reshape(-1).cpu().numpy()
    assert got.shape == (n,) and got.dtype == np.float32
    want = R.normals(seed, ctr, sid, n)
    d32 = float(np.abs(R.normals(seed, ctr, sid, n, f32=True).astype(np.float64) - want).max())
    bound = min(VC.MARGIN * d32, VC.CAP)
    assert np.all(np.isfinite(got)), f"{case}: non-finite normal at {np.argwhere(~np.isfinite(got))[0].tolist()}"
    dev = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{case}: d32 {d32:.3e} device deviation {dev:.3e} bound {bound:.3e}")
    if PARITY is not None:
        PARITY.append({"case": case, "d32": d32, "device_deviation": dev, "bound": bound})
    assert dev <= bound, f"{case}: deviation {dev:.3e} exceeds bound {bound:.3e} (worst element {int(np.abs(got - want).argmax())})"
    return got


@pytest.mark.parametrize("batch", R.LATENT_BATCHES)
def test_latents_from_the_fused_fc_kernel(batch):
    """z of a D step (stream 1) and the latent batch of the G step that follows (stream 2, one tick later; a G step that runs
    its own forward leaves it in the 'z' buffer)."""
    seed, offset = R.LATENT_SEED
    eng, n = _engine(batch), batch * R.NOISE_LATENT
    try:
        eng.seed(seed, offset)
        eng.d_step(_real(batch))
        _check_normals(f"z fused b{batch}", eng.debug_tensor("z", 0, (n,)), seed, offset, R.SID_Z, n)
        eng.g_step(batch)
        _check_normals(f"z_g fused b{batch}", eng.debug_tensor("z", 0, (n,)), seed, offset + 1, R.SID_ZG, n)
        assert eng.rng_state() == (seed, offset + 2)
    finally:
        eng.close()


def test_latents_from_the_generic_fc_kernel_are_the_same_bits():
    """A context for more than 256 rows draws z in the generic fc kernel (ops.hip), a smaller one in the MFMA kernel (fc.hip):
    same values from either, bit for bit -- the element index does not depend on the batch."""
    seed, offset = R.LATENT_SEED
    big, small = R.LATENT_FALLBACK, 5
    eng = _engine(big)
    try:
        eng.seed(seed, offset)
        eng.d_step(_real(big))
        z_big = _check_normals(f"z generic b{big}", eng.debug_tensor("z", 0, (big * R.NOISE_LATENT,)), seed, offset, R.SID_Z,
                               big * R.NOISE_LATENT)
    finally:
        eng.close()
    eng = _engine(small)
    try:
        eng.seed(seed, offset)
        eng.d_step(_real(small))
        z_small = eng.debug_tensor("z", 0, (small * R.NOISE_LATENT,)).cpu().numpy()
    finally:
        eng.close()
    diff = np.argwhere(z_big[:small * R.NOISE_LATENT].view(np.uint32) != z_small.view(np.uint32))
    assert len(diff) == 0, f"{len(diff)} of {z_small.size} latents differ in bits between the two fc kernels, first at {diff[0].tolist()}"


POISON, PAD = 12345.0, 64


def _op_randn(eng, n):
    """siggan_op_randn into the head of a poisoned buffer; the tail must stay untouched."""
    buf = torch.full((n + PAD,), POISON, dtype=torch.float32, device=DEV)
    _lib.check(eng.lib.siggan_op_randn(eng._h, C.c_void_p(buf.data_ptr()), n, eng._stream()))
    out = buf.cpu()
    assert bool((out[n:] == POISON).all()), f"op_randn({n}) wrote past its {n} elements"
    return out[:n]


def _plain_engine():
    from hipcommon import Engine
    return Engine(latent_dim=R.NOISE_LATENT, image_size=R.NOISE_SIZE, max_batch=2, device="cuda:0", seed=1)


@pytest.mark.parametrize("n", R.RANDN_N)
def test_op_randn(n):
    seed, offset = R.RANDN_SEED
    eng = _plain_engine()
    try:
        eng.seed(seed, offset)
        _check_normals(f"op_randn n{n}", _op_randn(eng, n), seed, offset + 1, R.SID_RANDN, n)      # ticks, then draws
        assert eng.rng_state() == (seed, offset + 1)
    finally:
        eng.close()


# ---- d. edges of u01 in the radius ---------------------------------------------------------------------------------------------
def test_radius_word_at_u_one_gives_zeros():
    """u01 == 1.0f (x >> 8 == 0xFFFFFF): log(1) = 0, so both normals of the half-group are +-0 -- not NaN."""
    e = R.EDGE_U_ONE
    eng = _plain_engine()
    try:
        eng.seed(e["seed"], e["offset"])
        z = _check_normals("op_randn u01 == 1", _op_randn(eng, R.EDGE_N), e["seed"], e["offset"] + 1, R.SID_RANDN, R.EDGE_N)
    finally:
        eng.close()
    assert z[e["element"]] == 0.0 and z[e["element"] + 1] == 0.0, (z[e["element"]], z[e["element"] + 1])


def test_radius_word_at_u_min_gives_the_largest_radius():
    """u01 == 2^-25 (x >> 8 == 0): radius sqrt(50 ln 2) = 5.887.  Each normal is within the bound, so the radius formed from
    the pair is within sqrt(2) x the bound."""
    e = R.EDGE_U_MIN
    eng = _plain_engine()
    try:
        eng.seed(e["seed"], e["offset"])
        z = _check_normals("op_randn u01 == 2^-25", _op_randn(eng, R.EDGE_N), e["seed"], e["offset"] + 1, R.SID_RANDN, R.EDGE_N)
    finally:
        eng.close()
    r = math.hypot(float(z[e["element"]]), float(z[e["element"] + 1]))
    assert abs(r - math.sqrt(50.0 * math.log(2.0))) <= math.sqrt(2.0) * VC.CAP, r
    assert float(np.abs(z).max()) <= r + VC.CAP, "no draw can lie outside the largest radius"


def test_radius_word_at_the_largest_u_below_one():
    """u01 == 1 - 2^-23: the device's log must come out negative (a positive one would put a NaN under the root); the radius is
    sqrt(-2 ln(1 - 2^-23)) = 4.9e-4, the smallest above 0."""
    e = R.EDGE_U_TOP
    eng = _plain_engine()
    try:
        eng.seed(e["seed"], e["offset"])
        z = _check_normals("op_randn u01 == 1 - 2^-23", _op_randn(eng, R.EDGE_N), e["seed"], e["offset"] + 1, R.SID_RANDN, R.EDGE_N)
    finally:
        eng.close()
    r = math.hypot(float(z[e["element"]]), float(z[e["element"] + 1]))
    assert r > 0.0 and abs(r - math.sqrt(-2.0 * math.log1p(-2.0 ** -23))) <= math.sqrt(2.0) * VC.CAP, r
