"""siggan_d_score_u8: the eval-mode Discriminator forward whose first block reads bytes (Engine.d_score_u8), the scoring step
of realism-filtered generation.

Held, exactly, to the parent path: the fp32 tensor is formed on the CPU by the reference's expression
(torch.from_numpy(bytes).float() / 127.5 - 1.0, after numpy binarisation where asked) and uploaded; ``x`` must equal it and
``probs`` must equal d_forward's on it, bit for bit.  Every case scores five images -- two seeded full-range random ones, one
holding all 256 byte values, one all 0 and one all 255 (borders and padding: a halo of byte 0 instead of 0.0f moves every
border pixel's sum) -- in calls of the case's batch size, the last one ragged."""
import ctypes as C

import numpy as np
import pytest
import torch

from common import I, SEED

pytestmark = pytest.mark.gpu

#        dtype  size batch spectral norm
CASES = [("f32", 64, 5, False), ("f32", 128, 3, False), ("bf16", 64, 4, False), ("f32", 64, 4, True), ("f32", 64, 1, False)]
BINARIZE = (None, 1, 127, 128, 255, 0)
LATENT = 100


def _engine(dtype, size, batch, sn, seed=0):
    from hipcommon import load_engine_state
    from signature_gan_amd.engine import Engine
    eng = Engine(latent_dim=LATENT, image_size=size, max_batch=batch, device="cuda:0", seed=seed, dtype=dtype, spectral_norm=sn)
    load_engine_state(eng, size, LATENT, warm=True)
    if sn:
        # the fresh weight_u / weight_v are random directions, whose sigma is far below the spectral norm: the weights divided
        # by it saturate every score at exactly 0 or 1.  Eight power iterations (train()-mode forwards) bring sigma to the
        # spectral norm, where the scores spread.
        x = torch.from_numpy(I.gen_real(batch, size, SEED["real"])).cuda()
        for _ in range(8):
            eng.d_forward(x, training=True)
    return eng


def _images(size):
    rng = np.random.default_rng(SEED["real"])
    rand = rng.integers(0, 256, size=(2, size, size), dtype=np.uint8)
    ramp = np.resize(np.arange(256, dtype=np.uint8), (1, size, size))
    return np.concatenate([rand, ramp, np.zeros((1, size, size), np.uint8), np.full((1, size, size), 255, np.uint8)])


def _x_cpu(u8, binarize):
    from signature_gan_amd.utils.inference import binarize_uint8, dequantize_uint8
    return dequantize_uint8(u8 if binarize is None else binarize_uint8(u8, binarize))


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-s{c[1]}-b{c[2]}" + ("-sn" if c[3] else ""))
def run(request):
    """One engine per case; for every binarisation the expected input, d_forward's probabilities on it, and what d_score_u8
    returned, all on the CPU."""
    dtype, size, batch, sn = request.param
    eng = _engine(dtype, size, batch, sn)
    u8 = _images(size)
    out = {"case": request.param, "u8": u8, "want_x": {}, "want_p": {}, "x": {}, "p": {}, "p_alone": {}, "launches": {}}
    for bz in BINARIZE:
        want_x = _x_cpu(u8, bz)
        want_p, got_p, got_x, alone, launches = [], [], [], [], []
        for a in range(0, len(u8), batch):
            xb = want_x[a:a + batch].cuda()
            ub = torch.from_numpy(u8[a:a + batch]).cuda()
            eng.prof_enable(True)
            want_p.append(eng.d_forward(xb).reshape(-1).cpu())
            n_fwd = len(eng.prof_launches())
            eng.prof_enable(True)
            p, x = eng.d_score_u8(ub, binarize=bz, want_input=True)
            launches.append((n_fwd, len(eng.prof_launches())))
            eng.prof_enable(False)
            got_p.append(p.cpu()); got_x.append(x.cpu())
            dest = torch.full((len(ub) + 2,), -7.0, device="cuda")        # out=: a slice of a larger score vector
            eng.d_score_u8(ub, binarize=bz, out=dest[1:1 + len(ub)])
            alone.append(dest.cpu())
        out["want_x"][bz], out["want_p"][bz] = want_x, torch.cat(want_p)
        out["x"][bz], out["p"][bz], out["p_alone"][bz], out["launches"][bz] = torch.cat(got_x), torch.cat(got_p), alone, launches
    eng.close()
    return out


@pytest.mark.parametrize("bz", BINARIZE)
def test_input_is_the_cpu_tensor(run, bz):
    assert run["x"][bz].shape == run["want_x"][bz].shape and run["x"][bz].dtype == torch.float32
    assert torch.equal(run["x"][bz], run["want_x"][bz])


@pytest.mark.parametrize("bz", BINARIZE)
def test_probabilities_are_d_forwards(run, bz):
    print(run["case"], bz, run["p"][bz].tolist(), run["want_p"][bz].tolist())
    assert run["p"][bz].shape == (5,)
    assert torch.equal(run["p"][bz], run["want_p"][bz])


@pytest.mark.parametrize("bz", BINARIZE)
def test_out_receives_the_same_scores_and_nothing_else(run, bz):
    got = torch.cat([d[1:-1] for d in run["p_alone"][bz]])
    assert torch.equal(got, run["want_p"][bz])
    assert all(float(d[0]) == -7.0 and float(d[-1]) == -7.0 for d in run["p_alone"][bz])


def test_the_scores_are_not_trivial(run):
    """What keeps the equalities above from holding on flat data: the two random images score differently, and binarising
    changes their scores."""
    p = run["want_p"]
    assert float(p[None][0]) != float(p[None][1])
    assert not torch.equal(p[None][:2], p[127][:2]) and not torch.equal(p[127][:2], p[0][:2])
    rand = torch.cat([v[:2] for v in p.values()])
    assert ((rand > 0) & (rand < 1)).all()                               # not saturated: equal bits mean equal arithmetic


def test_launch_counts_equal_d_forwards(run):
    """The profiler's launch table (the implicit-GEMM launches) of one d_score_u8 against one d_forward of the same batch."""
    for bz, pairs in run["launches"].items():
        for n_fwd, n_score in pairs:
            assert n_fwd == n_score and n_fwd > 0, (bz, pairs)


@pytest.mark.parametrize("dtype,sn", [("f32", False), ("bf16", False), ("f32", True)])
def test_carried_state_is_what_d_forward_leaves(dtype, sn):
    """Two engines in the same state, a staged step behind them (a D(real) forward started ahead, first-block rows that rode
    with the update); one calls d_forward, the other d_score_u8; one more train_step on the same inputs leaves them in the
    same state bit for bit."""
    from hipcommon import assert_same_state, full_state
    size, batch = 64, 4
    reals = [torch.from_numpy(I.gen_real(batch, size, SEED["real"] + t)).cuda() for t in range(3)]
    u8 = _images(size)[:batch]
    states, probs = [], []
    for use_u8 in (False, True):
        eng = _engine(dtype, size, batch, sn)
        eng.seed(77)
        eng.train_step(reals[0], clip=0.5, next_real=reals[1])
        if use_u8:
            probs.append(eng.d_score_u8(torch.from_numpy(u8).cuda(), binarize=127).clone())
        else:
            probs.append(eng.d_forward(_x_cpu(u8, 127).cuda()).reshape(-1).clone())
        eng.train_step(reals[1], clip=0.5, next_real=reals[2])
        eng.train_step(reals[2], clip=0.5)
        states.append(full_state(eng))
        eng.close()
    assert torch.equal(probs[0], probs[1])
    assert_same_state(states[0], states[1], "d_forward vs d_score_u8")


def test_batch_growth_and_refusals():
    size = 64
    eng = _engine("f32", size, 2, False)
    u8 = torch.from_numpy(_images(size)).cuda()
    p = eng.d_score_u8(u8)                                                # five images: the context grows like d_forward's
    assert eng.max_batch >= 5
    assert torch.equal(p, eng.d_forward(_x_cpu(_images(size), None).cuda()).reshape(-1))
    probs = torch.empty(5, device="cuda")
    call = lambda u, b, bz, pr: eng.lib.siggan_d_score_u8(eng._h, C.c_void_p(u), b, bz, C.c_void_p(pr), None, eng._stream())
    assert call(u8.data_ptr(), 5, -1, probs.data_ptr()) == 0
    assert call(0, 5, -1, probs.data_ptr()) == -1                         # null u8_dev
    assert call(u8.data_ptr(), 5, -1, 0) == -1                            # null probs_dev
    assert call(u8.data_ptr(), 5, -2, probs.data_ptr()) == -1             # binarize outside -1..255
    assert call(u8.data_ptr(), 5, 256, probs.data_ptr()) == -1
    assert call(u8.data_ptr(), 0, -1, probs.data_ptr()) == -1             # batch checks as siggan_d_forward
    assert call(u8.data_ptr(), eng.max_batch + 1, -1, probs.data_ptr()) == -1
    for bad in (256, -1):
        with pytest.raises(ValueError):
            eng.d_score_u8(u8, binarize=bad)
    with pytest.raises(ValueError):
        eng.d_score_u8(u8.float())
    with pytest.raises(ValueError):
        eng.d_score_u8(u8[:, :32])
    with pytest.raises(ValueError):
        eng.d_score_u8(u8, out=torch.empty(4, device="cuda"))
    eng.close()


def test_discriminator_score_u8_is_eval_mode_only():
    from signature_gan_amd.discriminator_vanilla_gan import Discriminator
    torch.manual_seed(3)
    d = Discriminator(input_size=64).to("cuda").eval()
    u8 = torch.from_numpy(_images(64)).cuda()
    assert torch.equal(d.score_u8(u8, binarize=128), d(_x_cpu(_images(64), 128).cuda()).reshape(-1))
    d.train()
    with pytest.raises(RuntimeError):
        d.score_u8(u8)
