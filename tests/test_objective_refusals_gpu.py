"""The refusals of the four objective entry points -- siggan_g_latent_grad, siggan_g_latent_objective_grad,
siggan_g_latent_objective_grad_seeded, siggan_g_param_grad -- through the C ABI: which reason a bad call is refused for, in
which words, and that nothing ran.

The entry points share one validation (eval.hip) around checks of their own, and the ORDER of the checks is part of the
contract: a call that is wrong in two ways is refused for the earlier reason.  Every case below is one violation, or two that
stand next to each other in that entry point's order (the expected text is then the earlier one's).  The texts are the
library's own, character for character.  Nothing is enqueued: every output buffer holds a sentinel and still does after a
synchronize.  The Python wrappers refuse most of these calls before the library sees them, hence the raw calls."""
import ctypes as C
import math

import pytest
import torch

from common import I, SEED
from objectivecommon import objective_engine

pytestmark = pytest.mark.gpu
SIZE, LATENT, BATCH = 64, 100, 2         # four Generator blocks: first_layer runs over [0, 5]
INVALID = -1                             # SIGGAN_E_INVALID

LG, OG, SG, PG = "siggan_g_latent_grad", "siggan_g_latent_objective_grad", "siggan_g_latent_objective_grad_seeded", "siggan_g_param_grad"
CTX = "null context"
FP32 = "{} needs an fp32 context (16-bit activations are not built for it)"
W_NULL = "null weights"
W_BAD = "the objective's weights must be finite and >= 0, got ({}, {}, {})"
ALL0 = "all three weights of the objective are 0"
ONE = "recon_weight > 0 needs exactly one of target_u8_dev and target_f32_dev"
T0 = "a target was given but recon_weight is 0"
PROBS = "probs_dev needs realism_weight > 0"
NULLT = "null tensor"
U8A = "target_u8_dev must be 4-byte aligned"
F32A = "target_f32_dev and images_dev must be 16-byte aligned"
LG_ONE = "exactly one of target_u8_dev and target_f32_dev must be given"
SEED0 = "null image_grad_dev (use siggan_g_latent_objective_grad without a seed)"
SEEDA = "image_grad_dev must be 16-byte aligned"
PRIOR = "prior_weight must be 0: the prior does not depend on the parameters, got 0.5"
BOTH0 = "both weights of the objective are 0"
FL = "first_layer {} outside [0, 5]"
DPA = "dparams_dev must be 16-byte aligned"


def batch_msg(b):
    return f"batch {b} outside [1, max_batch={BATCH}]"


# A case: (entry point, what differs from a valid call, the refusal's text).  Argument values: None (null), a number, a
# weight triple, or a buffer's name with an optional byte offset ("f32+4": misaligned).  ctx: "f32" / "bf16" / None.
# The valid call: realism alone, no target (siggan_g_latent_grad: the uint8 target), no probs, no images, first_layer 0.
CASES = []


def case(entry, text, **diff):
    CASES.append(pytest.param(entry, diff, text, id=f"{entry[7:]}-{len(CASES)}"))


# ---- siggan_g_latent_grad: context, batch, fp32, exactly one target, tensors, alignment
case(LG, CTX, ctx=None)
case(LG, batch_msg(0), batch=0)
case(LG, batch_msg(3), batch=3)
case(LG, FP32.format(LG), ctx="bf16")
case(LG, LG_ONE, tu8=None)
case(LG, LG_ONE, tf32="f32")
for k in ("z", "out", "obj"):
    case(LG, NULLT, **{k: None})
case(LG, U8A, tu8="u8+1")
case(LG, F32A, tu8=None, tf32="f32+4")
case(LG, F32A, img="img+4")
case(LG, batch_msg(0), batch=0, ctx="bf16")                       # pairs, in the order above
case(LG, FP32.format(LG), ctx="bf16", tu8=None)
case(LG, LG_ONE, tu8=None, out=None)
case(LG, NULLT, z=None, tu8="u8+1")
case(LG, U8A, tu8="u8+1", img="img+4")

# ---- what the three objective calls share: context, batch, fp32, null weights, the weights' values [their own checks] the
# target count against recon_weight, probs against realism_weight, tensors, alignment
for E in (OG, SG, PG):
    case(E, CTX, ctx=None)
    case(E, batch_msg(0), batch=0)
    case(E, batch_msg(3), batch=3)
    case(E, FP32.format(E), ctx="bf16")
    case(E, W_NULL, w=None)
    case(E, W_BAD.format("-1", "1", "0"), w=(-1.0, 1.0, 0.0), tu8=None)
    case(E, W_BAD.format("0", "-0.5", "0"), w=(0.0, -0.5, 0.0))
    case(E, W_BAD.format("0", "1", "-2"), w=(0.0, 1.0, -2.0))
    case(E, W_BAD.format("inf", "1", "0"), w=(math.inf, 1.0, 0.0), tu8="u8")
    case(E, W_BAD.format("0", "nan", "0"), w=(0.0, math.nan, 0.0))
    case(E, ONE, w=(1.0, 1.0, 0.0))
    case(E, ONE, w=(1.0, 1.0, 0.0), tu8="u8", tf32="f32")
    case(E, T0, tu8="u8")
    case(E, T0, tf32="f32")
    case(E, PROBS, w=(1.0, 0.0, 0.0), tu8="u8", probs="probs")
    for k in ("z", "out"):
        case(E, NULLT, **{k: None})
    case(E, U8A, w=(1.0, 1.0, 0.0), tu8="u8+1")
    case(E, F32A, w=(1.0, 1.0, 0.0), tf32="f32+4")
    case(E, F32A, img="img+4")
    case(E, batch_msg(0), batch=0, ctx="bf16")                    # pairs
    case(E, FP32.format(E), ctx="bf16", w=None)
    case(E, W_BAD.format("1", "-1", "0"), w=(1.0, -1.0, 0.0))     # a negative weight and no target
    case(E, ONE, w=(1.0, 0.0, 0.0), probs="probs")                # no target; probs without the realism term
    case(E, NULLT, z=None, w=(1.0, 1.0, 0.0), tu8="u8+1")
    case(E, U8A, w=(1.0, 1.0, 0.0), tu8="u8+1", img="img+4")
case(OG, NULLT, obj=None)
case(SG, NULLT, obj=None)

# ---- siggan_g_latent_objective_grad's own: all three weights 0, behind the weights' values
case(OG, ALL0, w=(0.0, 0.0, 0.0))
case(OG, ALL0, w=(0.0, 0.0, 0.0), tu8="u8")                       # ... and a target without recon_weight
case(OG, T0, w=(0.0, 0.0, 1.0), tu8="u8", probs="probs")          # a target without recon_weight; probs without realism
case(OG, PROBS, w=(0.0, 0.0, 1.0), probs="probs", out=None)       # probs without realism; a null tensor

# ---- siggan_g_latent_objective_grad_seeded's own: the seed, behind the weights' values
case(SG, SEED0, seed=None)
case(SG, SEEDA, seed="seed+4")
case(SG, W_BAD.format("0", "-1", "0"), w=(0.0, -1.0, 0.0), seed=None)
case(SG, SEED0, seed=None, w=(1.0, 1.0, 0.0))                     # a null seed and no target
case(SG, SEEDA, seed="seed+4", w=(1.0, 1.0, 0.0), tu8="u8", tf32="f32")      # a misaligned seed and two targets
case(SG, T0, w=(0.0, 0.0, 1.0), tu8="u8", probs="probs")
case(SG, PROBS, w=(0.0, 0.0, 1.0), probs="probs", out=None)

# ---- siggan_g_param_grad's own: the prior and "both weights" behind the weights' values; first_layer and dparams' alignment
# behind probs
case(PG, PRIOR, w=(1.0, 0.0, 0.5), tu8="u8")
case(PG, BOTH0, w=(0.0, 0.0, 0.0))
case(PG, FL.format(-1), fl=-1)
case(PG, FL.format(6), fl=6)
case(PG, DPA, out="out+4")
case(PG, W_BAD.format("1", "-1", "0.5"), w=(1.0, -1.0, 0.5), tu8="u8")       # a negative weight and a prior
case(PG, PRIOR, w=(0.0, 0.0, 0.5))                                # a prior and both other weights 0
case(PG, BOTH0, w=(0.0, 0.0, 0.0), tu8="u8")                      # both weights 0 and a target without recon_weight
case(PG, PROBS, w=(1.0, 0.0, 0.0), tu8="u8", probs="probs", fl=-1)
case(PG, FL.format(-1), fl=-1, out="out+4")
case(PG, DPA, out="out+4", z=None)
case(PG, NULLT, out=None, w=(1.0, 1.0, 0.0), tu8="u8+1")


@pytest.fixture(scope="module")
def world():
    engines = {"f32": objective_engine(SIZE, LATENT, BATCH), "bf16": objective_engine(SIZE, LATENT, BATCH, dtype="bf16")}
    n_out = max(engines["f32"].g_params.numel(), 4 * LATENT) + 4
    sentinel = lambda n: torch.full((n,), 7.0, device="cuda")
    bufs = {"z": torch.from_numpy(I.gen_z(4, LATENT, SEED["z"])).cuda(),
            "u8": torch.zeros(4 * SIZE * SIZE + 4, dtype=torch.uint8, device="cuda"),
            "f32": torch.zeros(4 * SIZE * SIZE + 4, device="cuda"),
            "seed": torch.zeros(4 * SIZE * SIZE + 4, device="cuda"),
            "out": sentinel(n_out), "obj": sentinel(4), "terms": sentinel(12), "probs": sentinel(4),
            "img": sentinel(4 * SIZE * SIZE + 4)}
    yield engines, bufs
    for eng in engines.values():
        eng.close()


def _arg(bufs, v):
    if not isinstance(v, str):
        return v
    name, _, off = v.partition("+")
    return C.c_void_p(bufs[name].data_ptr() + int(off or 0))


def _raw_call(engines, bufs, entry, diff):
    from signature_gan_amd import _lib
    a = dict(ctx="f32", z="z", batch=BATCH, tu8="u8" if entry == LG else None, tf32=None, w=(0.0, 1.0, 0.0), seed="seed", fl=0,
             out="out", obj="obj", terms="terms", probs=None, img=None)
    a.update(diff)
    eng = engines[a["ctx"] or "f32"]
    h = eng._h if a["ctx"] else None
    p = {k: _arg(bufs, a[k]) for k in ("z", "tu8", "tf32", "seed", "out", "obj", "terms", "probs", "img")}
    w = C.byref(_lib.LatentObjective(*a["w"])) if a["w"] is not None else None
    head = (h, p["z"], a["batch"], p["tu8"], p["tf32"])
    tail = (p["obj"], p["terms"], p["probs"], p["img"], eng._stream())
    if entry == LG:
        rc = eng.lib.siggan_g_latent_grad(*head, p["out"], p["obj"], p["img"], eng._stream())
    elif entry == OG:
        rc = eng.lib.siggan_g_latent_objective_grad(*head, w, p["out"], *tail)
    elif entry == SG:
        rc = eng.lib.siggan_g_latent_objective_grad_seeded(*head, w, p["seed"], p["out"], *tail)
    else:
        rc = eng.lib.siggan_g_param_grad(*head, w, a["fl"], p["out"], *tail)
    return rc, eng.lib.siggan_last_error().decode()


@pytest.mark.parametrize("entry, diff, text", CASES)
def test_refusal(world, entry, diff, text):
    engines, bufs = world
    rc, msg = _raw_call(engines, bufs, entry, diff)
    torch.cuda.synchronize()
    print(entry, diff, rc, repr(msg))
    assert rc == INVALID
    assert msg == text
    for k in ("out", "obj", "terms", "probs", "img"):
        assert bool((bufs[k] == 7.0).all()), k                     # nothing ran
