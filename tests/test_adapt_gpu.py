"""utils.inference.adapt_generator / restore_generator and the CLI's --adapt on the GPU: few-shot adaptation of the Generator's
weights around Engine.g_param_grad (pivotal tuning).

The case: latentcommon.projection_case() (64x64, latent 100, three targets = the bytes of G(z*)) with the final-conv gain 32 of
the gradient tests, z0 = z* + 0.25 n as FIXED pivots; Adam lr 1e-4, betas (0.9, 0.999), 12 steps, first_layer 0 and 3.  The loop
is held bit for bit to a hand-written chain of Engine.g_param_grad / op_anchor / op_adam / params_changed calls; its first
gradient to the fp64 oracle (test_param_grad_gpu's per-tensor bound); its descent to the same loop on the CPU through the oracle
in fp64 under torch.optim.Adam on the same trainable set -- that run takes the mean loss at the start of the last iteration to
0.23 of the first for both values of first_layer; the device must drop by at least half as much (test_projection_gpu's rule: a
sign, moment, scale or step-count error misses it by far; accuracy is the gradient tests' business)."""
import json

import numpy as np
import pytest
import torch

from adaptcommon import A_BETAS, A_GAIN, A_LR, A_STEPS, BOUND, oracle_adapt, oracle_param_grads, split_arena, tensor_margins
from latentcommon import P_LATENT, P_N, P_SIZE, oracle_sd64, projection_case
from objectivecommon import lut_f32

pytestmark = pytest.mark.gpu
FIRST = (0, 3)


def _state():
    sd = {k: v.clone() for k, v in projection_case()[0].items()}
    sd["final_conv.0.weight"] = sd["final_conv.0.weight"] * A_GAIN
    sd["final_conv.0.bias"] = sd["final_conv.0.bias"] * A_GAIN
    return sd


def _generator():
    from signature_gan_amd.generator_vanilla_gan import Generator
    g = Generator(latent_dim=P_LATENT, output_size=P_SIZE).to("cuda:0")
    g.load_state_dict(_state())
    return g.eval()


def compute_adaptation():
    """The loops, the hand-written chain and the first gradient on the case, computed once."""
    from hipcommon import hip_signs_g
    from signature_gan_amd.utils.inference import adapt_generator, generate_uint8, restore_generator
    _, z_star, z0 = projection_case()
    g = _generator()
    eng = g._require_engine()
    t_np = generate_uint8(g, z_star.cuda())
    t_u8 = torch.from_numpy(t_np).cuda()
    zc = z0.cuda()
    out = {"z0": z0, "t_np": t_np, "t64": lut_f32(t_u8)[:, 0].double(), "theta0": eng.g_params.cpu().clone()}
    out["img0"] = eng.g_forward(zc, training=False).cpu()
    d0 = eng.g_param_grad(zc, t_u8)[0]
    out["d0"], out["signs0"] = split_arena(eng, d0), hip_signs_g(eng, P_SIZE, P_N)
    for fl in FIRST:
        res = adapt_generator(g, t_np, z=z0, steps=A_STEPS, lr=A_LR, betas=A_BETAS, first_layer=fl)
        out[fl] = {"history": res["history"].cpu(), "before": res["loss_before"].cpu(), "after": res["loss_after"].cpu(),
                   "theta": eng.g_params.cpu().clone(), "snapshot": res["snapshot"].cpu(), "recon": res["recon"], "z": res["z"].cpu(),
                   "trainable": res["trainable"], "span": eng.layer_span(fl)}
        restore_generator(g, res["snapshot"])
        out[fl]["img_restored"] = eng.g_forward(zc, training=False).cpu()
        out[fl]["theta_restored"] = eng.g_params.cpu().clone()
    # the hand-written chain: five iterations, first_layer 3, an anchor
    steps, fl, aw = 5, 3, 0.5
    off, num = eng.layer_span(fl)
    snap = eng.g_params.clone()
    p, p0 = eng.g_params[off:], snap[off:]
    d = torch.empty_like(eng.g_params)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    hist = []
    for k in range(steps):
        hist.append(eng.g_param_grad(zc, t_u8, first_layer=fl, dparams_out=d)[1].clone())
        eng.op_anchor(d[off:], p, p0, aw)
        eng.op_adam(p, d[off:], m, v, k + 1, lr=A_LR, beta1=A_BETAS[0], beta2=A_BETAS[1], grad_scale=1.0 / P_N)
        eng.params_changed()
    final = eng.g_param_grad(zc, t_u8, first_layer=fl)[1]
    out["hand"] = (eng.g_params.cpu().clone(), torch.stack(hist).cpu(), final.cpu(), generate_uint8(g, zc))
    restore_generator(g, snap)
    res = adapt_generator(g, t_np, z=z0, steps=steps, lr=A_LR, betas=A_BETAS, first_layer=fl, anchor_weight=aw)
    out["loop"] = (eng.g_params.cpu().clone(), res["history"].cpu(), res["loss_after"].cpu(), res["recon"])
    restore_generator(g, res["snapshot"])
    # the anchor: the same run with a strong pull stays closer to theta0
    for aw in (0.0, 10.0):
        res = adapt_generator(g, t_np, z=z0, steps=A_STEPS, lr=A_LR, betas=A_BETAS, anchor_weight=aw)
        out[("anchor", aw)] = float((eng.g_params.cpu().double() - out["theta0"].double()).norm())
        restore_generator(g, res["snapshot"])
    out["g"] = g
    return out


@pytest.fixture(scope="module")
def run():
    return compute_adaptation()


def test_loop_is_the_hand_chain_bit_for_bit(run):
    (hp, hh, hf, hu), (lp, lh, lf, lu) = run["hand"], run["loop"]
    assert lh.shape == (5, P_N) and lu.shape == (P_N, P_SIZE, P_SIZE) and lu.dtype == np.uint8
    assert torch.equal(lp, hp) and torch.equal(lh, hh) and torch.equal(lf, hf) and np.array_equal(lu, hu)
    assert not torch.equal(lp, run["theta0"])


def test_first_gradient_is_the_oracles(run):
    from hipcommon import count_sign_flips
    rec = []
    g_recon, _, _, _ = oracle_param_grads(oracle_sd64(P_SIZE, P_LATENT, A_GAIN), None, run["z0"], run["t64"], P_SIZE, P_LATENT,
                                          run["signs0"], None, 0.0, rec)
    count_sign_flips(run["signs0"], rec)
    for k, (err, scale) in tensor_margins(run["d0"], g_recon).items():
        print(f"{k}: max|d - ref| / max|ref| = {err:.3e}  (max|ref| {scale:.3e})")
        assert scale > 0 and err <= BOUND, (k, err)


@pytest.mark.parametrize("fl", FIRST)
def test_descent_matches_the_oracles(run, fl):
    ref = oracle_adapt(run["z0"], run["t64"], fl)
    dev = run[fl]["history"].double()
    assert dev.shape == (A_STEPS, P_N) and torch.equal(run[fl]["before"].double(), dev[0])
    r0, r1, d0, d1 = float(ref[0].mean()), float(ref[-1].mean()), float(dev[0].mean()), float(dev[-1].mean())
    print(json.dumps({"first_layer": fl, "oracle_first": r0, "oracle_last": r1, "oracle_ratio": r1 / r0, "device_first": d0,
                      "device_last": d1, "device_ratio": d1 / d0, "device_after": float(run[fl]["after"].mean())}))
    assert r1 / r0 < 0.5                                  # the case descends at all
    assert d0 - d1 >= (r0 - r1) / 2, (d0, d1, r0, r1)
    assert float(run[fl]["after"].mean()) < d0


def test_frozen_layers_are_bit_identical(run):
    off, num = run[3]["span"]
    assert 0 < off and off + num == run["theta0"].numel()
    assert torch.equal(run[3]["theta"][:off], run["theta0"][:off])
    assert not torch.equal(run[3]["theta"][off:], run["theta0"][off:])
    assert run[3]["trainable"][0] == "upsample_blocks.2.block.0.weight" and run[0]["trainable"][0] == "fc.0.weight"
    assert run[0]["span"] == (0, run["theta0"].numel()) and not torch.equal(run[0]["theta"][:off], run["theta0"][:off])


def test_anchor_keeps_the_weights_closer(run):
    free, held = run[("anchor", 0.0)], run[("anchor", 10.0)]
    print(f"|theta - theta0|: {free:.4e} without the anchor, {held:.4e} with anchor_weight 10")
    assert 0 < held < free


def test_restore_gives_back_the_forward_bits(run):
    for fl in FIRST:
        assert torch.equal(run[fl]["snapshot"], run["theta0"]) and torch.equal(run[fl]["theta_restored"], run["theta0"])
        assert torch.equal(run[fl]["img_restored"], run["img0"])
        assert torch.equal(run[fl]["z"], run["z0"])


def test_arguments_are_checked(run):
    from signature_gan_amd.utils.inference import adapt_generator
    g, t_np, z0 = run["g"], run["t_np"], run["z0"]
    mb = g._require_engine().max_batch
    with pytest.raises(ValueError, match="few-shot"):
        adapt_generator(g, np.zeros((mb + 1, P_SIZE, P_SIZE), np.uint8), z=torch.zeros(mb + 1, P_LATENT), steps=1)
    with pytest.raises(ValueError, match="eval"):
        adapt_generator(g.train(), t_np, z=z0, steps=1)
    g.eval()
    for bad in (dict(steps=0), dict(lr=0.0), dict(first_layer=6), dict(anchor_weight=-1.0), dict(realism_weight=0.5)):
        with pytest.raises(ValueError):
            adapt_generator(g, t_np, z=z0, **{**dict(steps=1), **bad})
    with pytest.raises(ValueError):
        adapt_generator(g, t_np, z=z0[:2], steps=1)
    assert torch.equal(g._require_engine().g_params.cpu(), run["theta0"])          # a refusal changes nothing


def test_cli_adapt(run, tmp_path):
    from PIL import Image
    from signature_gan_amd import generate_signatures as cli
    from signature_gan_amd.utils.inference import load_generator
    ck = tmp_path / "gan.pt"
    torch.save({"epoch": 1, "generator_state_dict": _state(), "config": {"latent_dim": P_LATENT, "image_size": P_SIZE}}, ck)
    src = tmp_path / "real"
    src.mkdir()
    for i in range(P_N):
        Image.fromarray(run["t_np"][i], mode="L").save(src / f"sig_{i}.png")
    out, saved = tmp_path / "out", tmp_path / "adapted.pt"
    cli.main(["--checkpoint", str(ck), "--output_dir", str(out), "--seed", "3", "--n_samples", "5", "--adapt", str(src),
              "--adapt_steps", "4", "--adapt_first_layer", "3", "--adapt_anchor", "0.1", "--project_steps", "8", "--adapt_save", str(saved)])
    rep = json.load(open(out / "signature_adapt.json"))
    assert set(rep) == {"steps", "lr", "first_layer", "anchor_weight", "realism_weight", "sigma", "trainable", "targets"}
    assert (rep["steps"], rep["lr"], rep["first_layer"], rep["sigma"]) == (4, 1e-4, 3, 0.25)
    assert rep["trainable"][0] == "upsample_blocks.2.block.0.weight" and rep["trainable"][-1] == "final_conv.0.bias"
    assert [t["file"] for t in rep["targets"]] == [f"sig_{i}.png" for i in range(P_N)]
    for t in rep["targets"]:
        assert set(t) == {"file", "loss_before", "loss_after"} and 0.0 < t["loss_after"] < t["loss_before"]
    files = sorted(out.glob("signature_0*.png"))
    assert len(files) == 5 and Image.open(files[0]).size == (P_SIZE, P_SIZE)
    g2, latent = load_generator(str(saved), torch.device("cuda:0"))
    assert latent == P_LATENT and g2.output_size == P_SIZE
    theta = g2._require_engine().g_params.cpu()
    off = g2._require_engine().layer_span(3)[0]
    assert torch.equal(theta[:off], run["theta0"][:off]) and not torch.equal(theta[off:], run["theta0"][off:])
