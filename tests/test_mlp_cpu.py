"""The fully-connected GAN's step checks (tests/mlpcommon.py) have teeth, shown without a GPU: the fp32 oracle stands in for
the HIP path.  As it is, it passes every comparison against the fp64 oracle for the three cases of
tests/test_mlp_steps_gpu.py, and the no-near-tie condition holds for every step (mlpcommon.pick_inputs finds tie-free inputs
for each) -- the proof that such inputs exist and that the bound is attainable by the reference alone.  Each mutant of it is
rejected, by the check that is meant to catch it.

The first two mutants (the update skipped; the update's sign flipped) PASS the assertion tests/test_mlp_gpu.py used to make
about the updated weights, |w_after - oracle w_after| <= 2.5 x 2e-4: Adam's first step moves every element by about lr = 2e-4,
so skipping it is 2e-4 off and reversing it 4e-4 (test_the_old_update_assertion_could_not_fail)."""
import pytest
import torch
import torch.nn.functional as F

import mlpcommon as MC
from oracle import mlp_oracle as M
from oracle.siggan_oracle import adam_update


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_fp32_oracle_meets_every_bound_and_seeds_have_no_near_tie(case):
    margins = {}
    MC.run_chain(MC.OracleBackend(case), case, margins)
    assert all(v["deviation"] <= v["bound"] <= MC.CAP for v in margins.values())
    # six steps, each with its metrics, every gradient tensor and (G steps) both running statistics of every BatchNorm
    n_d, n_g = len(MC.spans(case, "d")[0]) + len(MC.D_METRICS), len(MC.spans(case, "g")[0]) + len(MC.G_METRICS) + 2 * len(case.hidden)
    assert len(margins) == MC.ROUNDS * (n_d + n_g)


@pytest.mark.parametrize("factor", [0.5, 2.0])
def test_clipped_steps_are_attainable_and_tie_free(factor):
    MC.run_clipped(MC.OracleBackend(MC.CASES[0]), MC.CASES[0], factor)


def test_batch_one_d_step_is_attainable_and_tie_free():
    backend = MC.OracleBackend(MC.ONE)
    backend.load(MC.make_state(MC.ONE))
    before = backend.snapshot()
    real, zd = MC.pick_inputs("d", MC.ONE, before, 0)
    met = backend.d_step(real, zd)
    MC.check_step("d", MC.ONE, before, backend.snapshot(), met, real, zd, 1, what="one D")
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):      # what the library mirrors
        backend.g_step(1, zd)


# ---- mutants of the stand-in ----------------------------------------------------------------------------------------------
def _skip_update(kind, before, after, batch):
    for a in ("params", "exp_avg", "exp_avg_sq"):
        after[f"{kind}_{a}"].copy_(before[f"{kind}_{a}"])


def _flip_sign(kind, before, after, batch):
    after[f"{kind}_params"].copy_(2 * before[f"{kind}_params"] - after[f"{kind}_params"])


def _wrong_bias_correction(kind, before, after, batch):
    p, m, v = (before[f"{kind}_{a}"].clone() for a in ("params", "exp_avg", "exp_avg_sq"))
    adam_update(p, after[f"{kind}_grads"], m, v, int(after[f"{kind}_adam_steps"][0]) + 1, MC.HP["lr"], MC.HP["beta1"], MC.HP["beta2"])
    after[f"{kind}_params"].copy_(p)


def _biased_running_var(kind, before, after, batch):
    if kind == "g":
        unbiased = (after["g_bn_var"] - 0.9 * before["g_bn_var"]) / 0.1
        after["g_bn_var"].copy_(0.9 * before["g_bn_var"] + 0.1 * unbiased * (batch - 1) / batch)


def _d_out_bias_left(kind, before, after, batch):
    if kind == "d":
        after["d_params"][-1] = before["d_params"][-1]


class _BatchNormWithoutInvB(torch.autograd.Function):
    """Train-mode BatchNorm1d whose backward takes SUMS where the means of dy and dy * xhat belong."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        rstd = (x.var(0, unbiased=False) + eps).rsqrt()
        xhat = (x - x.mean(0)) * rstd
        ctx.save_for_backward(xhat, gamma, rstd)
        return xhat * gamma + beta

    @staticmethod
    def backward(ctx, g):
        xhat, gamma, rstd = ctx.saved_tensors
        dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
        return gamma * rstd * (g - dbeta - xhat * dgamma), dgamma, dbeta, None


class _FWithMutantBatchNorm:
    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def batch_norm(x, rm, rv, w, b, training, momentum, eps):
        if not training:
            return F.batch_norm(x, rm, rv, w, b, training, momentum, eps)
        F.batch_norm(x.detach(), rm, rv, None, None, True, momentum, eps)          # the running statistics, as they should be
        return _BatchNormWithoutInvB.apply(x, w, b, eps)


MUTANTS = {
    # name: (mutate hook, hyper-parameters of the stand-in, the check that must reject it)
    "update skipped": (_skip_update, MC.HP, r"round 1 D net\.0\.weight: parameter is"),
    "update's sign flipped": (_flip_sign, MC.HP, r"round 1 D net\.0\.weight: parameter is"),
    "bias correction at the wrong step": (_wrong_bias_correction, MC.HP, r"round 1 D net\.0\.weight: parameter is"),
    "biased variance in running_var": (_biased_running_var, MC.HP, r"round 1 G net\.0\.bn\.running_var: relative deviation"),
    "label smoothing 1.0": (None, dict(MC.HP, label_smoothing=1.0), r"round 1 D d_loss: relative deviation"),
    "D out.bias not updated": (_d_out_bias_left, MC.HP, r"round 1 D out\.bias: parameter is"),
}


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_is_rejected(case, mutant):
    mutate, hp, by = MUTANTS[mutant]
    with pytest.raises(AssertionError, match=by):
        MC.run_chain(MC.OracleBackend(case, hp=hp, mutate=mutate), case, rounds=1)


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_batchnorm_backward_without_inv_b_is_rejected(case, monkeypatch):
    monkeypatch.setattr(M, "F", _FWithMutantBatchNorm())
    backend = MC.OracleBackend(case)
    backend.load(MC.make_state(case))
    before = backend.snapshot()
    _, zg = MC.pick_inputs("g", case, before, 1)
    met = backend.g_step(case.batch, zg)
    after = backend.snapshot()
    monkeypatch.undo()                                                             # the yardstick is the real BatchNorm
    with pytest.raises(AssertionError, match=r"grad net\.\d\.(linear|bn)\.\w+: relative deviation"):
        MC.check_step("g", case, before, after, met, None, zg, 1, what="mutant G")


@pytest.mark.parametrize("mutant", ["update skipped", "update's sign flipped"])
def test_the_old_update_assertion_could_not_fail(mutant):
    case = MC.CASES[1]
    backend = MC.OracleBackend(case, mutate=MUTANTS[mutant][0])
    backend.load(MC.make_state(case))
    real, zd, _ = MC.make_inputs(case, rounds=1)[0]
    before = backend.snapshot()
    backend.d_step(real, zd)
    after = backend.snapshot()
    want = MC.run_oracle("d", before, case, real, zd, torch.float32)["d_sd"]
    for k, (o, n, _) in MC.spans(case, "d")[0].items():
        assert float((after["d_params"][o:o + n] - want[k].reshape(-1)).abs().max()) <= 2.5 * 2e-4, k       # the old assertion: passes
    with pytest.raises(AssertionError, match="parameter is"):
        MC.check_update("d", case, before, after, 1, "mutant")
