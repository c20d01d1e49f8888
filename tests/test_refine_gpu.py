"""utils.inference.refine_latents / generate_signatures_refined, the realism-guided project_signatures and the CLI flags on
top of them, on the GPU.

The case: latentcommon.projection_case() (64x64, latent 100, three vectors, no final-conv gain), the cold synthetic
Discriminator, z0 as given; Adam lr 0.02, 20 steps.  The loop is held bit for bit to a hand-written chain of
Engine.g_latent_objective_grad and Engine.op_adam calls; the gradient it follows to the fp64 oracle at the loop's own z_k (steps
0, 10 and 19, the bound of test_latent_objective_gpu); its descent to the same loop run on the CPU through the oracle in fp64
under torch.optim.Adam -- that run takes the per-image objective from 0.702 / 0.725 / 0.728 to 0.523 / 0.540 / 0.549 at the start
of its last iteration (0.518 / 0.533 / 0.543 after it; the logits rise by about 0.39); the device must drop by at least half as much (test_projection_gpu's rule: a sign, moment or step-count error
misses it by far; accuracy is the gradient tests' business)."""
import json

import numpy as np
import pytest
import torch

from common import oracle_states
from latentcommon import P_BETAS, P_LATENT, P_N, P_SIZE, oracle_sd64, projection_case
from objectivecommon import R_LR, R_STEPS, hip_signs_d_rows, oracle_d_sd64, oracle_objective, oracle_refine

pytestmark = pytest.mark.gpu
GRAD_STEPS = (0, 10, 19)


def _d_state():
    return oracle_states(P_SIZE, P_LATENT, warm=False)[1]


def _modules(shared=False, sn=False):
    """(Generator, Discriminator) in eval mode on the case's states: each on an engine of its own, or both on one."""
    from signature_gan_amd.discriminator_vanilla_gan import Discriminator
    from signature_gan_amd.engine import Engine
    from signature_gan_amd.generator_vanilla_gan import Generator
    sd = projection_case()[0]
    if shared:
        eng = Engine(latent_dim=P_LATENT, image_size=P_SIZE, max_batch=4, device="cuda:0", seed=0)
        g, d = Generator(latent_dim=P_LATENT, output_size=P_SIZE, _engine=eng), Discriminator(input_size=P_SIZE, _engine=eng)
    else:
        g = Generator(latent_dim=P_LATENT, output_size=P_SIZE).to("cuda:0")
        d = Discriminator(input_size=P_SIZE, use_spectral_norm=sn).to("cuda:0")
    g.load_state_dict(sd)
    if not sn:
        d.load_state_dict(_d_state())
    return g.eval(), d.eval()


def compute_refinement():
    """The hand-written chain and the loop on the case, computed once (also what profiles/latent_objective_parity_margins.py
    records)."""
    from hipcommon import hip_signs_g
    from signature_gan_amd.utils.inference import adopt_discriminator, generate_uint8, refine_latents
    _, _, z0 = projection_case()
    g, d = _modules()
    eng = adopt_discriminator(g, d)
    out = {"g": g, "d": d, "z0": z0}
    out["want_before"] = eng.d_forward(eng.g_forward(z0.cuda(), training=False), training=False).reshape(-1).cpu()
    z = z0.clone().cuda()
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    hist, probes = [], {}
    for k in range(R_STEPS):
        dz, obj = eng.g_latent_objective_grad(z)
        if k in GRAD_STEPS:
            probes[k] = (z.cpu().clone(), dz.cpu().clone(), hip_signs_g(eng, P_SIZE, P_N), hip_signs_d_rows(eng, P_SIZE, P_N))
        hist.append(obj)
        eng.op_adam(z, dz, m, v, k + 1, lr=R_LR, beta1=P_BETAS[0], beta2=P_BETAS[1])
    _, _, after = eng.g_latent_objective_grad(z, want_probs=True)
    out["hand"] = (z.cpu(), torch.stack(hist).cpu(), after.cpu(), generate_uint8(g, z))
    out["probes"] = probes
    zl, u8, before, after, history = refine_latents(g, d, z0, steps=R_STEPS, lr=R_LR, betas=P_BETAS)
    out["loop"] = (zl.cpu(), history.cpu(), after.cpu(), u8, before.cpu())
    zp = refine_latents(g, d, z0, steps=R_STEPS, lr=R_LR, betas=P_BETAS, prior_weight=0.1)[0]
    out["z_prior"] = zp.cpu()
    return out


@pytest.fixture(scope="module")
def run():
    return compute_refinement()


@pytest.fixture(scope="module")
def oracle_runs(run):
    """The same loop on the CPU through the fp64 oracle, without and with the prior: computed once."""
    return oracle_refine(run["z0"], R_STEPS, R_LR), oracle_refine(run["z0"], R_STEPS, R_LR, prior_weight=0.1)


def test_loop_is_the_hand_chain_bit_for_bit(run):
    (hz, hh, ha, hu), (lz, lh, la, lu, lb) = run["hand"], run["loop"]
    assert lz.shape == (P_N, P_LATENT) and lh.shape == (R_STEPS, P_N) and la.shape == (P_N,) and lb.shape == (P_N,)
    assert lu.shape == (P_N, P_SIZE, P_SIZE) and lu.dtype == np.uint8
    assert torch.equal(lz, hz) and torch.equal(lh, hh) and torch.equal(la, ha) and np.array_equal(lu, hu)
    assert not torch.equal(lz, run["z0"])


def test_scores_rise_and_start_at_the_forward_passes(run):
    _, _, after, _, before = run["loop"]
    print(f"probs before {before.tolist()} after {after.tolist()}")
    assert torch.equal(before, run["want_before"])       # bit for bit d_forward of g_forward(z0)
    assert bool((after > before).all())


@pytest.mark.parametrize("k", GRAD_STEPS)
def test_gradient_along_the_path(run, k):
    from hipcommon import count_sign_flips
    z_k, dz, signs_g, signs_d = run["probes"][k]
    rec_g, rec_d = [], []
    _, grads, _ = oracle_objective(oracle_sd64(P_SIZE, P_LATENT), oracle_d_sd64(P_SIZE), z_k, None, P_SIZE, signs_g, signs_d, 0.0,
                                   rec_g, rec_d)
    count_sign_flips(signs_g, rec_g); count_sign_flips(signs_d, rec_d)
    ref = grads[1]
    err = float((dz.double() - ref).abs().max()) / float(ref.abs().max())
    print(f"step {k}: max|dz - dz_ref| / max|dz_ref| = {err:.3e}  (max|dz_ref| {float(ref.abs().max()):.3e})")
    assert err <= 1e-4, err


def test_descent_matches_the_oracles(run, oracle_runs):
    ref, logits, _ = oracle_runs[0]
    dev = run["loop"][1].double()
    drop_ref, drop_dev = (ref[0] - ref[-1]).numpy(), (dev[0] - dev[-1]).numpy()
    print(json.dumps({"oracle_obj0": ref[0].tolist(), "oracle_obj19": ref[-1].tolist(), "oracle_logit_rise": (logits[-1] - logits[0]).tolist(),
                      "device_obj0": dev[0].tolist(), "device_obj19": dev[-1].tolist()}))
    assert (drop_ref > 0.1).all(), drop_ref              # the case descends at all
    assert (drop_dev >= drop_ref / 2).all(), (drop_dev, drop_ref)


def test_prior_keeps_z_smaller(run, oracle_runs):
    ms = lambda z: float((z.double() ** 2).mean())
    z_ref0, z_ref1 = oracle_runs[0][2], oracle_runs[1][2]
    print(f"rms of z: device {ms(run['loop'][0]) ** 0.5:.4f} -> {ms(run['z_prior']) ** 0.5:.4f} with the prior; "
          f"oracle {ms(z_ref0) ** 0.5:.4f} -> {ms(z_ref1) ** 0.5:.4f}")
    assert ms(z_ref1) < ms(z_ref0)
    assert ms(run["z_prior"]) < ms(run["loop"][0])


def test_generate_signatures_refined_is_reproducible(run):
    from signature_gan_amd.utils.inference import generate_signatures_refined
    g, d = run["g"], run["d"]
    dev = torch.device("cuda:0")
    kw = dict(seed=9, batch_size=4, steps=3, lr=R_LR)
    a = generate_signatures_refined(g, d, 5, P_LATENT, dev, **kw)
    b = generate_signatures_refined(g, d, 5, P_LATENT, dev, **kw)
    assert len(a[0]) == len(a[1]) == len(a[2]) == 5 and a[0][0].mode == "L" and a[0][0].size == (P_SIZE, P_SIZE)
    assert a[1] == b[1] and a[2] == b[2] and all(np.array_equal(np.array(x), np.array(y)) for x, y in zip(a[0], b[0]))
    assert all(0.0 < p < 1.0 for p in a[1] + a[2]) and a[1] != a[2]
    c = generate_signatures_refined(g, d, 5, P_LATENT, dev, seed=10, batch_size=4, steps=3, lr=R_LR)
    assert c[2] != a[2]
    u = generate_signatures_refined(g, d, 2, P_LATENT, dev, **kw)
    t = generate_signatures_refined(g, d, 2, P_LATENT, dev, threshold=127, **kw)       # the same run, its bytes binarised
    assert t[1] == u[1] and t[2] == u[2]
    assert all(np.array_equal(np.array(x), np.where(np.array(y) < 127, 0, 255)) for x, y in zip(t[0], u[0]))


def test_guided_projection_is_its_hand_chain_and_the_defaults_are_todays(run):
    from signature_gan_amd.utils.inference import adopt_discriminator, generate_uint8, project_signatures
    g, d, z0 = run["g"], run["d"], run["z0"]
    z_star = projection_case()[1]
    t_np = generate_uint8(g, z_star.cuda())
    t_u8 = torch.from_numpy(t_np).cuda()
    steps, lr = 6, 0.02
    eng = adopt_discriminator(g, d)
    z = z0.clone().cuda()
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    hist = []
    for k in range(steps):
        dz, obj = eng.g_latent_objective_grad(z, t_u8, 1.0, 0.5, 0.0)
        hist.append(obj)
        eng.op_adam(z, dz, m, v, k + 1, lr=lr, beta1=P_BETAS[0], beta2=P_BETAS[1])
    final = eng.g_latent_objective_grad(z, t_u8, 1.0, 0.5, 0.0)[1]
    zl, recon, loss, history = project_signatures(g, t_np, steps=steps, lr=lr, betas=P_BETAS, z0=z0, discriminator=d, realism_weight=0.5)
    assert torch.equal(zl, z) and torch.equal(history, torch.stack(hist)) and torch.equal(loss, final)
    assert np.array_equal(recon, generate_uint8(g, z))
    # the defaults: today's function on the same arguments, i.e. the chain of g_latent_grad
    z = z0.clone().cuda()
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    for k in range(steps):
        dz, _ = eng.g_latent_grad(z, t_u8)
        eng.op_adam(z, dz, m, v, k + 1, lr=lr, beta1=P_BETAS[0], beta2=P_BETAS[1])
    plain = project_signatures(g, t_np, steps=steps, lr=lr, betas=P_BETAS, z0=z0)
    zero = project_signatures(g, t_np, steps=steps, lr=lr, betas=P_BETAS, z0=z0, discriminator=None, realism_weight=0.0, prior_weight=0.0)
    assert torch.equal(plain[0], z) and torch.equal(zero[0], z) and torch.equal(plain[2], zero[2]) and torch.equal(plain[3], zero[3])
    with pytest.raises(ValueError):
        project_signatures(g, t_np, steps=steps, realism_weight=0.5)          # no Discriminator


def test_adoption(run):
    from signature_gan_amd.utils.inference import refine_latents
    g_s, d_s = _modules(shared=True)
    assert g_s._require_engine() is d_s._require_engine()
    zs = refine_latents(g_s, d_s, run["z0"], steps=R_STEPS, lr=R_LR, betas=P_BETAS)
    lz, lh, la, lu, lb = run["loop"]                     # a Discriminator on its own engine: the same bits
    assert torch.equal(zs[0].cpu(), lz) and np.array_equal(zs[1], lu) and torch.equal(zs[2].cpu(), lb) and torch.equal(zs[3].cpu(), la)
    assert torch.equal(zs[4].cpu(), lh)
    _, d_sn = _modules(sn=True)
    with pytest.raises(ValueError, match="_engine"):
        refine_latents(run["g"], d_sn, run["z0"], steps=2)
    with pytest.raises(ValueError, match="eval"):
        refine_latents(run["g"], run["d"].train(), run["z0"], steps=2)
    run["d"].eval()


def test_cli_refine_and_guided_projection(run, tmp_path):
    from PIL import Image
    from signature_gan_amd import generate_signatures as cli
    from signature_gan_amd.utils.inference import generate_uint8
    sd = projection_case()[0]
    ck = tmp_path / "gan.pt"
    torch.save({"epoch": 1, "generator_state_dict": sd, "discriminator_state_dict": _d_state(),
                "config": {"latent_dim": P_LATENT, "image_size": P_SIZE}}, ck)
    out = tmp_path / "out"
    cli.main(["--checkpoint", str(ck), "--output_dir", str(out), "--seed", "3", "--n_samples", "5", "--batch_size", "4",
              "--refine_by_realism", "--refine_steps", "3"])
    rec = json.load(open(out / "signature_refine.json"))
    assert len(list(out.glob("signature_0*.png"))) == 5 and [r["file"] for r in rec] == [f"signature_{i + 1:06d}.png" for i in range(5)]
    for r in rec:
        assert set(r) == {"file", "before", "after"} and 0.0 < r["before"] < 1.0 and 0.0 < r["after"] < 1.0
        assert Image.open(out / r["file"]).size == (P_SIZE, P_SIZE)
    src = tmp_path / "real"
    src.mkdir()
    t_np = generate_uint8(run["g"], projection_case()[1].cuda())
    for i in range(2):
        Image.fromarray(t_np[i], mode="L").save(src / f"sig_{i}.png")
    base = ["--checkpoint", str(ck), "--output_dir", str(out), "--seed", "3", "--project", str(src), "--project_steps", "4"]
    cli.main(base + ["--prefix", "w", "--project_realism_weight", "0.5", "--project_prior_weight", "0.1"])
    for r in json.load(open(out / "w_projection.json")):
        assert set(r) == {"file", "reconstruction", "loss", "z", "realism"} and 0.0 < r["realism"] < 1.0
    cli.main(base + ["--prefix", "p", "--project_prior_weight", "0.1"])
    assert all("realism" not in r for r in json.load(open(out / "p_projection.json")))        # only when W > 0
    g_only = tmp_path / "g.pt"
    torch.save({"generator_state_dict": sd, "config": {"latent_dim": P_LATENT, "image_size": P_SIZE}}, g_only)
    with pytest.raises(SystemExit, match="holds no discriminator_state_dict: --refine_by_realism needs the Discriminator's weights"):
        cli.main(["--checkpoint", str(g_only), "--output_dir", str(out), "--refine_by_realism"])
    for other in (["--filter_by_realism"], ["--project", str(src)], ["--morph"]):
        with pytest.raises(SystemExit):
            cli.main(["--checkpoint", str(ck), "--refine_by_realism"] + other)
