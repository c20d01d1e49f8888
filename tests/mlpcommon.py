"""The yardstick of the fully-connected GAN's step tests (tests/test_mlp_steps_gpu.py, tests/test_mlp_gpu.py and their CPU
proof tests/test_mlp_cpu.py): oracle/mlp_oracle.py run in fp64 and in fp32 from one state, the bound, the near-tie list and the
update check.  PARITY UNPINNED, as everything about this model: the reference has no fully-connected GAN.

A step is always checked as ONE step from the state the path under test held before it (read back whole), so every
comparison is at the one-step bound however long the chain is.

Bound (per tensor, relative to the fp64 tensor's max-abs): verifiercommon's rule -- MARGIN x the fp32 oracle's own deviation
from the fp64 oracle, never looser than CAP.  The reference of every comparison is the fp64 oracle.  Two kinds of value need
a word more:
  * The gradient of a Generator Linear bias is the column sum of dL/dy over a Linear output y that a train-mode BatchNorm
    follows.  That sum is zero in exact arithmetic: the fp64 oracle holds ~1e-18 for it, every fp32 implementation (the fp32
    oracle included) the rounding of its terms, ~1e-9.  "Relative to the fp64 tensor's max-abs" would compare rounding noise
    with rounding noise, so the scale of these tensors is the size of what is summed -- the largest column sum of |dL/dy|
    (mlp_oracle.g_step's aux["lin_bias_terms"]) -- and the rule is otherwise the same.
  * A metric is one fp32 number.  One sample of the fp32 oracle's deviation can be arbitrarily close to zero by chance, so a
    scalar's deviation estimate is floored at one fp32 rounding of its value (2^-24 relative): the value is delivered as an
    fp32, which alone costs that much.  Bound: min(MARGIN x max(deviation, 2^-24 |value|), CAP |value|).

Near ties: a Generator post-BatchNorm value or a Discriminator pre-LeakyReLU value whose fp64 magnitude is below NEAR_TIE
(verifier_train_inputs') of its layer's max-abs may fall on the other side in an fp32 implementation and then moves whole
gradient sums.  Every step checked here is one for which the fp64 oracle has NO near tie (check_step asserts it), so the
Generator's gradients get the same bound as everything else: no ReLU allowance.  How such steps are found: the small
geometries have under a thousand decisions a step and almost any seed is free of ties; the benchmark's geometry has 49152 a
step, about four near ties per D + G pair, so a chain of three pairs from ONE seed is free of them about once in 2e5 seeds --
and from the second pair on the state is the path's own, which a seed search on the CPU cannot know (a Linear bias in front
of a train-mode BatchNorm walks by +-lr on the sign of rounding noise, and the eval-mode Generator of the next D step sees
it).  So the inputs are drawn per step (pick_inputs): from the state read back before the step, the first seed of a fixed
sequence whose inputs give the fp64 oracle no near tie.  The choice depends on the path under test only through its state,
never through its errors; it costs a few fp64 oracle steps on the CPU.

Update check: p / exp_avg / exp_avg_sq after a step equal oracle.adam_update in fp64 applied to the path's OWN parameters and
moments from before the step and its OWN gradient arena as read back after it, at the step number the test counts.  The bounds
are tests/test_ops_gpu.py::test_adam's (which pins the kernel on random data): 2e-7 + 1e-6 lr absolute for the parameter, 1e-5
of the tensor's max-abs for the moments.  Feeding the path's own gradient leaves no discontinuity at |g| ~ eps: no element is
left out.  p_after is NOT also compared with the oracle's own p_after (an element whose gradient is within rounding of eps may
flip there; the gradient check and this one cover what that comparison could catch)."""
import os
import sys
from collections import OrderedDict, namedtuple

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import verifier_train_inputs as TI                   # noqa: E402
import verifiercommon as VC                          # noqa: E402
from oracle import mlp_oracle as M                   # noqa: E402
from oracle.siggan_oracle import AdamState, adam_update  # noqa: E402
from signature_gan_amd.mlp_gan import d_entries, g_entries  # noqa: E402

MARGIN, CAP, NEAR_TIE = VC.MARGIN, VC.CAP, TI.NEAR_TIE
F32_ROUNDING = 2.0 ** -24
HP = dict(lr=2e-4, beta1=0.5, beta2=0.999, label_smoothing=0.9)          # MLPGAN's defaults
ARENAS = ("params", "grads", "exp_avg", "exp_avg_sq", "adam_steps")
BN_KEYS = ("g_bn_mean", "g_bn_var", "g_bn_batches")
STATE_KEYS = tuple(f"{w}_{a}" for w in "gd" for a in ARENAS) + BN_KEYS   # MLPGAN's attribute names
D_METRICS = ("d_loss", "d_loss_real", "d_loss_fake", "d_real_mean", "d_fake_mean")
G_METRICS = ("g_loss", "g_fake_mean")
ROUNDS = 3

Case = namedtuple("Case", "name size hidden max_batch batch latent seed")
# (size, hidden, max_batch, batch) are the issue's; the latent width is chosen here.  seed: of the initial state and the base of
# the input seeds (pick_inputs).
CASES = (
    Case("ragged", 8, (12, 100), 16, 7, 17, 0),       # widths that are no power of two, C <= 32, B < max_batch, K = 17
    Case("bench", 28, (256, 512), 32, 32, 100, 0),    # bench.py --model mlp
    Case("c4_75", 12, (300,), 8, 8, 10, 0),          # C4 = 75: two column blocks, the second ragged; K = 10 < one K-tile
)
STALE = Case("stale", 8, (12, 100), 32, 5, 17, 0)      # batch 5 on a workspace carved for 32 (compared bit for bit)
ONE = Case("one", 8, (12, 100), 16, 1, 17, 0)          # M = 1 GEMMs; R = 2 rows in the D step


def case_id(c):
    return c.name


def spans(case, which):
    ent = g_entries(case.latent, case.size, case.hidden) if which == "g" else d_entries(case.size, case.hidden)
    sp, off = OrderedDict(), 0
    for key, shape in ent:
        n = int(np.prod(shape))
        sp[key] = (off, n, tuple(shape))
        off += n
    return sp, off


def make_state(case, seed=None):
    """A whole state (STATE_KEYS -> CPU tensor): parameters N(0, 0.05) (BatchNorm weights N(1, 0.05)), biases included, running
    statistics away from (0, 1), everything else zero."""
    gen = torch.Generator().manual_seed(case.seed if seed is None else seed)
    st = {}
    for w in "gd":
        sp, total = spans(case, w)
        p = torch.empty(total)
        for k, (o, n, _) in sp.items():
            p[o:o + n].normal_(1.0 if ".bn.weight" in k else 0.0, 0.05, generator=gen)
        st[f"{w}_params"] = p
        for a in ARENAS[1:4]:
            st[f"{w}_{a}"] = torch.zeros(total)
        st[f"{w}_adam_steps"] = torch.zeros(len(sp))
    nbn = sum(case.hidden)
    st["g_bn_mean"] = torch.rand(nbn, generator=gen) * 0.5 - 0.25
    st["g_bn_var"] = torch.rand(nbn, generator=gen) * 0.5 + 0.75
    st["g_bn_batches"] = torch.zeros(len(case.hidden), dtype=torch.int64)
    return st


def make_inputs(case, batch=None, rounds=ROUNDS, seed=None):
    """[(real, z of the D step, z of the G step)] per round."""
    b = case.batch if batch is None else batch
    gen = torch.Generator().manual_seed((case.seed if seed is None else seed) + 1000003)
    return [(torch.rand(b, 1, case.size, case.size, generator=gen) * 2 - 1, torch.randn(b, case.latent, generator=gen),
             torch.randn(b, case.latent, generator=gen)) for _ in range(rounds)]


def clone_state(st):
    return {k: v.clone() for k, v in st.items()}


# ---- the oracle from a state --------------------------------------------------------------------------------------------
def oracle_from(st, case, dtype):
    """(g_sd, d_sd, g_opt, d_opt) of oracle/mlp_oracle.py holding state `st` in `dtype`."""
    out = []
    for w in "gd":
        sp, _ = spans(case, w)
        sd = OrderedDict((k, st[f"{w}_params"][o:o + n].view(shape).to(dtype).clone()) for k, (o, n, shape) in sp.items())
        opt = AdamState(list(sp), sd)
        opt.m = {k: st[f"{w}_exp_avg"][o:o + n].view(shape).to(dtype).clone() for k, (o, n, shape) in sp.items()}
        opt.v = {k: st[f"{w}_exp_avg_sq"][o:o + n].view(shape).to(dtype).clone() for k, (o, n, shape) in sp.items()}
        opt.step = int(st[f"{w}_adam_steps"][0])
        out.append((sd, opt))
    (g_sd, g_opt), (d_sd, d_opt) = out
    off = 0
    for i, h in enumerate(case.hidden):
        g_sd[f"net.{i}.bn.running_mean"] = st["g_bn_mean"][off:off + h].to(dtype).clone()
        g_sd[f"net.{i}.bn.running_var"] = st["g_bn_var"][off:off + h].to(dtype).clone()
        g_sd[f"net.{i}.bn.num_batches_tracked"] = st["g_bn_batches"][i].clone()
        off += h
    return g_sd, d_sd, g_opt, d_opt


def run_oracle(kind, st, case, real, z, dtype, clip=None, hp=HP):
    """One D ('d') or G ('g') step of the oracle in `dtype` from state `st` (left unchanged).  Returns metrics, grads (by name,
    clipped if clip), aux, and the oracle's state after the step (g_sd, d_sd, opt)."""
    g_sd, d_sd, g_opt, d_opt = oracle_from(st, case, dtype)
    aux = {}
    kw = dict(lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], clip=clip, aux=aux)
    if kind == "d":
        met, grads = M.d_step(g_sd, d_sd, d_opt, real.to(dtype), z.to(dtype), case.hidden, case.size,
                              label_smoothing=hp["label_smoothing"], **kw)
    else:
        met, grads = M.g_step(g_sd, d_sd, g_opt, z.to(dtype), case.hidden, case.size, **kw)
    if clip is not None:
        met[f"{kind}_grad_norm"] = aux["grad_norm"]
    return dict(metrics=met, grads=grads, aux=aux, g_sd=g_sd, d_sd=d_sd, opt=d_opt if kind == "d" else g_opt)


def near_ties(aux):
    """{layer: count} of the decisions of a step's fp64 run that lie within NEAR_TIE of their layer's max-abs (empty: none)."""
    out = {}
    for key in ("g_post_bn", "d_pre"):
        for i, t in enumerate(aux.get(key, ())):
            n = int((t.abs() < NEAR_TIE * t.abs().max()).sum())
            if n:
                out[f"{key}[{i}]"] = n
    return out


def decisions(aux):
    return sum(t.numel() for key in ("g_post_bn", "d_pre") for t in aux.get(key, ()))


# ---- comparisons ----------------------------------------------------------------------------------------------------------
def _f64(t):
    return torch.as_tensor(t).detach().double().reshape(-1)


def check_tensor(got, ref64, ref32, what, margins=None, scale=None):
    """The bound rule: max|got - ref64| / scale <= min(MARGIN x max|ref32 - ref64| / scale, CAP); scale: max|ref64| unless given."""
    got, ref64, ref32 = _f64(got), _f64(ref64), _f64(ref32)
    if scale is None:
        scale = float(ref64.abs().max())
    assert scale > 0.0 and got.shape == ref64.shape, what
    b = min(MARGIN * float((ref32 - ref64).abs().max()) / scale, CAP)
    d = float((got - ref64).abs().max()) / scale
    print(f"{what}: relative deviation {d:.3e} bound {b:.3e}")
    if margins is not None:
        margins[what] = {"deviation": d, "bound": b}
    assert d <= b, f"{what}: relative deviation {d:.3e} exceeds bound {b:.3e}"


def check_scalar(got, ref64, ref32, what, margins=None):
    """A metric (see the module docstring): the deviation estimate is floored at one fp32 rounding of the value."""
    got, ref64, ref32 = float(got), float(ref64), float(ref32)
    scale = abs(ref64)
    assert scale > 0.0, what
    b = min(MARGIN * max(abs(ref32 - ref64) / scale, F32_ROUNDING), CAP)
    d = abs(got - ref64) / scale
    print(f"{what}: relative deviation {d:.3e} bound {b:.3e}")
    if margins is not None:
        margins[what] = {"deviation": d, "bound": b}
    assert d <= b, f"{what}: relative deviation {d:.3e} exceeds bound {b:.3e}"


def check_update(which, case, before, after, count, what, hp=HP):
    """The update check of the module docstring, on network `which`; count: the Adam step this update is."""
    sp, _ = spans(case, which)
    lr = hp["lr"]
    for k, (o, n, _) in sp.items():
        p, g = before[f"{which}_params"][o:o + n].double(), after[f"{which}_grads"][o:o + n].double()
        m, v = before[f"{which}_exp_avg"][o:o + n].double(), before[f"{which}_exp_avg_sq"][o:o + n].double()
        adam_update(p, g, m, v, count, lr, hp["beta1"], hp["beta2"])
        dp = float((after[f"{which}_params"][o:o + n].double() - p).abs().max())
        assert dp <= 2e-7 + 1e-6 * lr, f"{what} {k}: parameter is {dp:.3e} from Adam step {count} of its own gradient"
        for name, want in (("exp_avg", m), ("exp_avg_sq", v)):
            d = float((after[f"{which}_{name}"][o:o + n].double() - want).abs().max())
            assert d <= 1e-5 * float(want.abs().max()) + 1e-30, f"{what} {k}: {name} is {d:.3e} from Adam step {count} (max {float(want.abs().max()):.3e})"
    steps = after[f"{which}_adam_steps"]
    assert torch.equal(steps, torch.full_like(steps, float(count))), f"{what}: adam_steps {steps.tolist()} != {count}"


def check_step(kind, case, before, after, got_metrics, real, z, count, clip=None, margins=None, what="", hp=HP):
    """Everything one step is checked for.  before / after: the whole state of the path under test around the step;
    got_metrics: its metrics; count: the number of this update of network `kind` as the test counts it."""
    other = "g" if kind == "d" else "d"
    r64 = run_oracle(kind, before, case, real, z, torch.float64, clip, hp)
    r32 = run_oracle(kind, before, case, real, z, torch.float32, clip, hp)
    ties = near_ties(r64["aux"])
    assert not ties, f"{what}: the fp64 oracle has near ties {ties} among {decisions(r64['aux'])} decisions"

    for k in (D_METRICS if kind == "d" else G_METRICS) + ((f"{kind}_grad_norm",) if clip is not None else ()):
        check_scalar(got_metrics[k], r64["metrics"][k], r32["metrics"][k], f"{what} {k}", margins)

    sp, _ = spans(case, kind)
    terms = {f"net.{i}.linear.bias": s for i, s in enumerate(r64["aux"].get("lin_bias_terms", ()))}
    for k, (o, n, _) in sp.items():
        check_tensor(after[f"{kind}_grads"][o:o + n], r64["grads"][k], r32["grads"][k], f"{what} grad {k}", margins, scale=terms.get(k))

    check_update(kind, case, before, after, count, what, hp)
    for a in ARENAS:
        assert torch.equal(after[f"{other}_{a}"], before[f"{other}_{a}"]), f"{what}: the step changed {other}_{a}"

    if kind == "d":
        for k in BN_KEYS:
            assert torch.equal(after[k], before[k]), f"{what}: a Discriminator step changed {k}"
    else:
        off = 0
        for i, h in enumerate(case.hidden):
            for key, name in (("g_bn_mean", "running_mean"), ("g_bn_var", "running_var")):
                check_tensor(after[key][off:off + h], r64["g_sd"][f"net.{i}.bn.{name}"], r32["g_sd"][f"net.{i}.bn.{name}"],
                             f"{what} net.{i}.bn.{name}", margins)
            off += h
        assert torch.equal(after["g_bn_batches"], before["g_bn_batches"] + 1), f"{what}: num_batches_tracked {after['g_bn_batches'].tolist()}"
    return r64


MAX_TRIES = 400       # (the benchmark geometry's D step accepts about one draw in 14: 400 refusals in a row are a 1e-13 event)


def pick_inputs(kind, case, before, step_index):
    """(real, z) for step number step_index of a test: the first draw of the seed sequence of that step for which the fp64 oracle,
    run from state `before`, has no near tie (see the module docstring).  real is None for a G step."""
    for t in range(MAX_TRIES):
        gen = torch.Generator().manual_seed(1000003 + 7919 * case.seed + 1000 * step_index + t)
        real = torch.rand(case.batch, 1, case.size, case.size, generator=gen) * 2 - 1 if kind == "d" else None
        z = torch.randn(case.batch, case.latent, generator=gen)
        if not near_ties(run_oracle(kind, before, case, real, z, torch.float64)["aux"]):
            return real, z
    raise AssertionError(f"{case.name} step {step_index}: no tie-free inputs in {MAX_TRIES} draws")


def run_chain(backend, case, margins=None, rounds=ROUNDS):
    """ROUNDS x (D step, G step) with given noise on `backend` (HipBackend, or the fp32 stand-in of tests/test_mlp_cpu.py), every
    step checked by check_step from the backend's own state before it."""
    backend.load(make_state(case))
    last = spans(case, "d")[1] - 1                       # D's out.bias: the last element of an odd-length arena (k_adam's tail lanes)
    for r in range(rounds):
        before = backend.snapshot()
        real, zd = pick_inputs("d", case, before, 2 * r)
        met = backend.d_step(real, zd)
        after = backend.snapshot()
        check_step("d", case, before, after, met, real, zd, r + 1, margins=margins, what=f"{case.name} round {r + 1} D")
        assert float(after["d_params"][last]) != float(before["d_params"][last]), f"{case.name} round {r + 1}: D's out.bias did not move"
        before = after
        _, zg = pick_inputs("g", case, before, 2 * r + 1)
        met = backend.g_step(case.batch, zg)
        after = backend.snapshot()
        check_step("g", case, before, after, met, None, zg, r + 1, margins=margins, what=f"{case.name} round {r + 1} G")


def run_clipped(backend, case, factor, margins=None):
    """One D step and one G step with clip = factor x the fp64 oracle's gradient norm of that step (factor < 1: the clip
    bites; > 1: it does not): the written-back gradient arena against the oracle's clipped gradient, the grad-norm metric
    against its pre-clip norm, the update check on what was written back."""
    backend.load(make_state(case))
    for i, kind in enumerate("dg"):
        before = backend.snapshot()
        r, z = pick_inputs(kind, case, before, i)
        clip = factor * run_oracle(kind, before, case, r, z, torch.float64, clip=1.0)["aux"]["grad_norm"]
        met = backend.d_step(r, z, clip=clip) if kind == "d" else backend.g_step(case.batch, z, clip=clip)
        after = backend.snapshot()
        r64 = check_step(kind, case, before, after, met, r, z, 1, clip=clip, margins=margins, what=f"{case.name} clip x{factor} {kind.upper()}")
        want = torch.cat([r64["grads"][k].reshape(-1) for k in spans(case, kind)[0]])
        assert (float(want.norm()) < 0.999 * r64["aux"]["grad_norm"]) == (factor < 1.0)      # the clip bit exactly when it should


# ---- the paths under test -------------------------------------------------------------------------------------------------
def snapshot_model(m):
    """The whole state of an MLPGAN, on the host."""
    torch.cuda.synchronize()
    return {k: getattr(m, k).cpu().clone() for k in STATE_KEYS}


class HipBackend:
    """signature_gan_amd.mlp_gan.MLPGAN behind the interface run_chain / check_step use."""

    def __init__(self, case, seed=1, **kw):
        from signature_gan_amd.mlp_gan import MLPGAN
        self.case = case
        self.m = MLPGAN(latent_dim=case.latent, image_size=case.size, hidden=case.hidden, max_batch=case.max_batch, device="cuda:0",
                        seed=seed, **kw)

    def load(self, st):
        for k in STATE_KEYS:
            getattr(self.m, k).copy_(st[k])

    def snapshot(self):
        return snapshot_model(self.m)

    def metrics(self):
        from signature_gan_amd import _lib
        host = self.m.metrics.cpu()
        return {k: float(host[i]) for k, i in _lib.METRIC_INDEX.items()}

    def d_step(self, real, z, clip=None):
        self.m.train_discriminator_step(real.cuda(), noise=None if z is None else z.cuda(), clip=clip)
        return self.metrics()

    def g_step(self, batch, z, clip=None):
        self.m.train_generator_step(batch, noise=None if z is None else z.cuda(), clip=clip)
        return self.metrics()

    def close(self):
        self.m.close()


class OracleBackend:
    """The fp32 oracle as a stand-in for the HIP path: it holds a state in fp32 arenas and steps it with oracle/mlp_oracle.py in
    fp32.  tests/test_mlp_cpu.py runs the comparisons above on it (they must pass) and on mutants of it (they must not).
    mutate(kind, before, after, batch): optional, edits `after` in place; hp: what the stand-in computes with."""

    def __init__(self, case, hp=HP, mutate=None):
        self.case, self.hp, self.mutate, self.st = case, dict(hp), mutate, None

    def load(self, st):
        self.st = clone_state(st)

    def snapshot(self):
        return clone_state(self.st)

    def _step(self, kind, real, z, clip):
        before = self.st
        r = run_oracle(kind, before, self.case, real, z, torch.float32, clip, self.hp)
        after = clone_state(before)
        sp, _ = spans(self.case, kind)
        for k, (o, n, _) in sp.items():
            after[f"{kind}_params"][o:o + n] = (r["d_sd"] if kind == "d" else r["g_sd"])[k].reshape(-1)
            after[f"{kind}_grads"][o:o + n] = r["grads"][k].reshape(-1)
            after[f"{kind}_exp_avg"][o:o + n] = r["opt"].m[k].reshape(-1)
            after[f"{kind}_exp_avg_sq"][o:o + n] = r["opt"].v[k].reshape(-1)
        after[f"{kind}_adam_steps"].fill_(float(r["opt"].step))
        if kind == "g":
            off = 0
            for i, h in enumerate(self.case.hidden):
                after["g_bn_mean"][off:off + h] = r["g_sd"][f"net.{i}.bn.running_mean"]
                after["g_bn_var"][off:off + h] = r["g_sd"][f"net.{i}.bn.running_var"]
                after["g_bn_batches"][i] = r["g_sd"][f"net.{i}.bn.num_batches_tracked"]
                off += h
        if self.mutate is not None:
            self.mutate(kind, before, after, z.shape[0])
        self.st = after
        return r["metrics"]

    def d_step(self, real, z, clip=None):
        return self._step("d", real, z, clip)

    def g_step(self, batch, z, clip=None):
        assert batch == z.shape[0]
        return self._step("g", None, z, clip)
