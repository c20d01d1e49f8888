"""The yardstick of the saturated-head tests, pinned against torch on the CPU in fp32 (no GPU): headcommon's p_ref,
loss_ref and dlogit_ref against torch.sigmoid, F.binary_cross_entropy and autograd over the whole sweep X0 for every target
the steps use, and the regime table of DESIGN.md as exact values.  A wrong reference therefore cannot make the GPU tests pass.

Bounds: p within 1 ulp (torch's expf is good to 1 ulp; the add and the divide are the same roundings on both sides); loss
and gradient within 8 ulp of the fp64 formulas evaluated FROM TORCH'S fp32 p (the bound the GPU tests put on the kernels: at
most five fp32 roundings in either expression, doubled).

One rounding separates loss_ref from the installed torch and is counted here, not hidden: loss_ref forms q = 1 - p in fp32
and takes log(q) -- the formula the HIP heads hold, and older torch releases' -- while a current torch's BCE forward takes
log1p(-p), which never rounds 1 - p.  For p >= 0.5 the subtraction is exact (Sterbenz) and both agree; below, q lies in
[0.5, 1], where fp32 is spaced 2^-24, so q is off by at most 2^-25 and its log by at most 2^-25 / 0.5 = 2^-24: the loss of
a sample may differ from torch's by (1 - y) 2^-24 = 6e-8 ABSOLUTE (at x = -17, y = 0: 5.96e-8 against 4.14e-8), never more.
That is 3 % of the absolute tolerance the parity tests give a loss (2e-6) and touches no gradient: the backward formulas
do not contain the log.  test_reference_head_is_torchs_over_the_sweep allows exactly this term on top of the 8 ulp, and
test_loss_formula_is_the_clamped_log_form pins loss_ref to 8 ulp against the log(1 - p) form evaluated by torch in fp32."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import headcommon as H

ULP_P, ULP = 1, 8


def _torch_head(x, y, reduction):
    x = torch.tensor(np.asarray(x, np.float32), requires_grad=True)
    p = torch.sigmoid(x)
    t = torch.full_like(p, float(y))
    per = F.binary_cross_entropy(p, t, reduction="none")
    red = F.binary_cross_entropy(p, t, reduction=reduction)
    g, = torch.autograd.grad(red, x)
    return p.detach().numpy(), per.detach().numpy(), g.numpy()


def test_sweep_holds_the_required_logits_and_all_are_admissible():
    need = (-120, -104, -100, -89, -88, -60, -30, -27.7, -27.5, -17, -8, 0, 8, 12, 16.5, 16.7, 17, 27.5, 27.7, 30, 60, 89, 120)
    assert set(need) <= set(H.X0) and len(H.X0) >= 23
    for x in H.X0:
        for y in H.TARGETS:
            assert H.regime(x, y).admissible, x
    assert abs(H.X_ONE - 16.6355) < 1e-4 and abs(H.X_ZERO + 88.7228) < 1e-4 and abs(H.X_FLOOR + 27.631) < 1e-3
    # inadmissible: within 0.05 of either decision point; the regimes on both sides of each
    assert not H.regime(16.6, 0).admissible and not H.regime(16.68, 0).admissible and not H.regime(-88.7, 1).admissible
    assert H.regime(16.7, 0).name == "one" and H.regime(16.5, 0).name == "coarse" and H.regime(12.0, 0).name == "middle"
    assert H.regime(-89, 1).name == "zero" and H.regime(-88, 1).name == "subnormal" and H.regime(-60, 1).name == "floor"
    assert H.regime(-27.7, 1).name == "floor" and H.regime(-27.5, 1).name == "middle"
    assert H.regime(30, 0).dead and H.regime(-95, 1).dead and not H.regime(-88, 1).dead and not H.regime(16.5, 0).dead


@pytest.mark.parametrize("y", H.TARGETS)
def test_reference_head_is_torchs_over_the_sweep(y):
    n = len(H.X0)
    p, loss, grad = _torch_head(H.X0, y, "mean")
    mine = H.p_ref(H.X0)
    assert mine.dtype == np.float32
    d = H.ulp_distance32(mine, p)
    assert d.max() <= ULP_P, [(x, a, b) for x, a, b, k in zip(H.X0, mine, p, d) if k > ULP_P]
    want = H.loss_ref(p, y)
    log1p_term = np.where(p < 0.5, (1.0 - float(np.float32(y))) * 2.0 ** -24, 0.0)      # module docstring
    excess = np.abs(loss - want) - ULP * H.spacing32(want) - log1p_term
    assert excess.max() <= 0, list(zip(H.X0, loss, want))
    assert (np.abs(loss - want)[p >= 0.5] <= ULP * H.spacing32(want)[p >= 0.5]).all()
    gu = H.ulps(grad, H.dlogit_ref(p, y, n))
    assert gu.max() <= ULP, list(zip(H.X0, gu))
    # and from the reference's own p: the whole chain, so that p_ref's one ulp cannot hide a wrong formula
    assert np.isfinite(H.loss_ref(mine, y)).all() and np.isfinite(H.dlogit_ref(mine, y, n)).all()
    same = d == 0
    assert np.array_equal(H.loss_ref(mine, y)[same], H.loss_ref(p, y)[same])


@pytest.mark.parametrize("y", H.TARGETS)
def test_loss_formula_is_the_clamped_log_form(y):
    """loss_ref against -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)) evaluated by torch in fp32, 8 ulp."""
    p = torch.sigmoid(torch.tensor(np.asarray(H.X0, np.float32)))
    t = torch.tensor(float(y))
    loss = -(t * torch.log(p).clamp(min=-100.0) + (1.0 - t) * torch.log(1.0 - p).clamp(min=-100.0))
    lu = H.ulps(loss.numpy(), H.loss_ref(p.numpy(), y))
    assert lu.max() <= ULP, list(zip(H.X0, lu))


def test_the_regime_table():
    """The table of DESIGN.md 3 ("Saturated heads"), as torch computes it on the CPU and as the reference functions do."""
    xs = np.array([16.63, 16.64, 30.0, 120.0, -27.5, -30.0, -88.0, -89.0, -120.0], np.float32)
    for head in ("torch", "ref"):
        if head == "torch":
            p, l0, g0 = _torch_head(xs, 0.0, "sum")
            _, l1, g1 = _torch_head(xs, 1.0, "sum")
            _, l9, g9 = _torch_head(xs, 0.9, "sum")
        else:
            p = H.p_ref(xs)
            l0, l1, l9 = (H.loss_ref(p, y) for y in (0.0, 1.0, 0.9))
            g0, g1, g9 = (H.dlogit_ref(p, y, 1) for y in (0.0, 1.0, 0.9))
        assert p[0] == np.float32(1.0) - np.float32(2.0 ** -23) and abs(l0[0] - 15.942385) < 2e-6 and abs(g0[0] - 0.9999999) < 1e-7
        assert (p[1:4] == 1.0).all() and (l0[1:4] == 100.0).all() and (g0[1:4] == 0.0).all(), head     # the jump at 24 ln 2
        assert (l1[1:4] == 0.0).all() and (g1[1:4] == 0.0).all() and (g9[1:4] == 0.0).all()
        assert np.allclose(l9[1:4], 10.000002, rtol=0, atol=1e-6) and (l9[1:4] > 10.0).all()            # 100 (1 - 0.9f)
        assert abs(p[4] / 1.14e-12 - 1) < 1e-2 and abs(g0[4] / p[4] - 1) < 1e-6                         # floor not yet active
        assert abs(p[5] / 9.36e-14 - 1) < 1e-3 and abs(g0[5] / (float(p[5]) ** 2 * 1e12) - 1) < 1e-6    # the floor regime: p p 1e12
        assert abs(g0[5] / 8.76e-15 - 1) < 1e-3 and abs(g1[5] / -(float(p[5]) * 1e12) - 1) < 1e-6       # y = 1: -p 1e12, not -1
        assert 0 < p[6] < 2.0 ** -126 and abs(p[6] / 6.0546e-39 - 1) < 1e-4                             # the subnormal p is kept
        assert abs(l1[6] - 88.0) < 1e-5 and l0[6] < 1e-38 and abs(g0[6]) < 2.0 ** -149                    # 88, not 100
        assert (p[7:] == 0.0).all() and (l1[7:] == 100.0).all() and (l0[7:] == 0.0).all()
        assert (g0[7:] == 0.0).all() and (g1[7:] == 0.0).all() and (np.asarray(l9[7:], np.float32) == 90.0).all()    # 100 * 0.9f rounds to 90


def test_ulp_helpers():
    one = np.float32(1.0)
    assert H.ulp_distance32(one, np.nextafter(one, np.float32(2))) == 1
    assert H.ulp_distance32(np.float32(0.0), np.float32(-0.0)) == 0
    assert H.ulp_distance32(np.float32(2.0 ** -149), np.float32(-2.0 ** -149)) == 2
    assert H.ulps(1.0 + 2.0 ** -23, 1.0) == 1.0 and H.ulps(2.0 ** -149, 0.0) == 1.0
    assert H.ulps(3 * 2.0 ** -149, 2.0 ** -140) == (2.0 ** -140 - 3 * 2.0 ** -149) / 2.0 ** -149
    assert H.ulps(0.5 - 2.0 ** -25, 0.5) == 0.5          # at a power of two the spacing above it counts
