"""The sigmoid / BCE head as the reference computes it in fp32, restated in plain numpy fp64 -- the yardstick of the
saturated-head tests (test_saturated_heads_cpu.py pins it against torch on the CPU; test_saturated_heads_gpu.py holds the
four HIP copies of the head to it).

The reference's head is three lines of fp32 (nn.Sigmoid, nn.BCELoss, autograd):

    p        = 1 / (1 + expf(-x))
    loss     = -(y max(log p, -100) + (1 - y) max(log(1 - p), -100))
    d(logit) = (p - y) / max((1 - p) p, 1e-12) / count  *  (1 - p) p

and what is sharp about it comes from the fp32 roundings, not from the mathematics: 1 + expf(-x) rounds to 1 as soon as
expf(-x) < 2^-24 (x > 24 ln 2 = 16.6355: p is exactly 1, the loss jumps to the clamp, the gradient to 0), expf(-x) overflows
above ln(FLT_MAX) (x < -88.7228: p is exactly 0), and below ln(1e-12) = -27.63 the floor under (1 - p) p takes the gradient
from p - y to (p - y) p 1e12.  The mathematical fp64 sigmoid saturates at 36.7 and never reaches 0: it would be the wrong
yardstick, so p_ref follows the fp32 steps (with a correctly rounded exp), and loss_ref / dlogit_ref start from an fp32 p."""
import math
from collections import namedtuple

import numpy as np

F32 = np.float32
X_ONE = 24.0 * math.log(2.0)                    # 16.6355: above it 1 + expf(-x) == 1 in fp32, p == 1
X_ZERO = -math.log(float(np.finfo(F32).max))    # -88.7228: below it expf(-x) overflows, p == 0
X_FLOOR = math.log(1e-12)                       # -27.631: below it (1 - p) p < 1e-12, the floor is active
X_SUBNORMAL = math.log(2.0 ** -126)             # -87.3365: below it p is a subnormal
MARGIN = 0.05                                   # admissible logits keep this distance from X_ONE and X_ZERO
FLOOR = F32(1e-12)                              # torch's EPSILON, as the fp32 constant the kernels hold
LOG_CLAMP = -100.0

# the sweep: both exact ends, the subnormal p, the floor's two sides, the coarse 1 - p below X_ONE, the middle
X0 = (-120.0, -104.0, -100.0, -89.0, -88.0, -60.0, -30.0, -27.7, -27.5, -17.0, -8.0, 0.0, 8.0, 12.0, 16.5, 16.7, 17.0, 27.5,
      27.7, 30.0, 60.0, 89.0, 120.0)
TARGETS = (0.0, 0.9, 1.0)

Regime = namedtuple("Regime", "name admissible dead")


def regime(x, y):
    """Which regime of the fp32 head the logit ``x`` is in for target ``y``: name, whether x is admissible (not within MARGIN
    of a decision point of expf / the add, where one ulp of expf decides between two regimes), and whether d(logit) is exactly
    zero there (p == 1 or p == 0: the factor (1 - p) p is 0)."""
    x = float(F32(x))
    admissible = abs(x - X_ONE) >= MARGIN and abs(x - X_ZERO) >= MARGIN
    if x > X_ONE:
        return Regime("one", admissible, True)                  # p == 1: loss 100 (1 - y), gradient 0
    if x < X_ZERO:
        return Regime("zero", admissible, True)                 # p == 0: loss 100 y, gradient 0
    if x < X_SUBNORMAL:
        return Regime("subnormal", admissible, False)           # p kept: loss -x y, gradient (p - y) p 1e12
    if x < X_FLOOR:
        return Regime("floor", admissible, False)               # gradient (p - y) p 1e12
    if x > 12.0:
        return Regime("coarse", admissible, False)              # 1 - p is a handful of fp32 quanta
    return Regime("middle", admissible, False)


def p_ref(x):
    """The sigmoid of fp32 logits by the reference's fp32 steps with a correctly rounded exp (fp64 exp rounded to fp32), the
    add and the divide rounded to fp32 -- float32 array.  A kernel whose expf is good to 1 ulp lands within 2 ulp."""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(-x.astype(np.float64)).astype(F32)             # inf above FLT_MAX, as expf
        return (F32(1.0) / (F32(1.0) + e)).astype(F32)


def _parts(p32, y):
    p32 = np.asarray(p32)
    assert p32.dtype == F32, "loss_ref / dlogit_ref start from the fp32 p"
    q32 = (F32(1.0) - p32).astype(F32)                            # formed in fp32: 0 as soon as p == 1
    y64 = np.asarray(y, F32).astype(np.float64)                   # the target(s) as the fp32 tensor holds them (0.9f)
    return p32.astype(np.float64), q32.astype(np.float64), y64


def loss_ref(p32, y):
    """BCE of an fp32 p against target y, torch's formula in fp64: logs clamped at -100, 1 - p and 1 - y as fp32 forms them."""
    p, q, y = _parts(p32, y)
    with np.errstate(divide="ignore"):
        lp, lq = np.maximum(np.log(p), LOG_CLAMP), np.maximum(np.log(q), LOG_CLAMP)
    return -(y * lp + (1.0 - y) * lq)


def dlogit_ref(p32, y, count):
    """d(mean BCE over ``count`` samples) / d(logit) from an fp32 p, torch's two backward formulas in fp64: the floor 1e-12
    (the fp32 constant) under (1 - p) p, then times (1 - p) p."""
    p, q, y = _parts(p32, y)
    qp = q * p
    return (p - y) / np.maximum(qp, np.float64(FLOOR)) / float(count) * qp


def spacing32(ref):
    """The fp32 spacing (one ulp) at the magnitude of fp64 values: 2^(e - 23), and 2^-149 throughout the subnormals."""
    a = np.abs(np.asarray(ref, np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a > 0, np.maximum(np.exp2(e - 23.0), 2.0 ** -149), 2.0 ** -149)


def ulps(got, ref):
    """|got - ref| in fp32 ulps of ref (fp64 arrays; subnormal references count in quanta of 2^-149)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / spacing32(ref)


def ulp_distance32(a, b):
    """Number of fp32 values between two float32 arrays (0: the same bits up to the sign of zero)."""
    def key(v):
        i = np.asarray(v, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
