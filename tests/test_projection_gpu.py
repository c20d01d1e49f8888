"""utils.inference.project_signatures / morph_sequence and the CLI flags on top of them, on the GPU.

The case (latentcommon): 64x64, latent 100, three targets -- the bytes of G at z* --, starts z* + 0.25 n, Adam lr 0.02, 40 steps.
The loop is held bit for bit to a hand-written chain of Engine.g_latent_grad and Engine.op_adam calls; the gradient it follows
to the fp64 oracle at the loop's own z_k (steps 0, 20 and 39, the bound of test_latent_grad_gpu); its descent to the same loop
run on the CPU through the oracle in fp64 under torch.optim.Adam (at least half that run's reduction of the loss: a loop that
does not descend -- a sign error, stale moments, a wrong step count -- misses it by far; accuracy is the gradient tests'
business).  The oracle run on the CPU, with the targets taken as the bytes of its own images, reduces the three losses by factors
of 12.4, 10.3 and 13.8 (2.5e-4 -> 2.0e-5, the quantisation floor); profiles/projection_parity_margins.py records both runs."""
import json

import numpy as np
import pytest
import torch

from latentcommon import (P_BETAS, P_LATENT, P_LR, P_N, P_SIZE, P_STEPS, oracle_descent, oracle_latent_grad, oracle_sd64,
                          projection_case)

pytestmark = pytest.mark.gpu
GRAD_STEPS = (0, 20, 39)


def _generator(sd):
    from signature_gan_amd.generator_vanilla_gan import Generator
    g = Generator(latent_dim=P_LATENT, output_size=P_SIZE).to("cuda:0")
    g.load_state_dict(sd)
    g.eval()
    return g


def compute_projection():
    """The hand-written chain and the loop on the case, computed once (also what profiles/projection_parity_margins.py records)."""
    from hipcommon import hip_signs_g
    from signature_gan_amd import _lib
    from signature_gan_amd.utils.inference import generate_uint8, project_signatures
    sd, z_star, z0 = projection_case()
    g = _generator(sd)
    eng = g._require_engine()
    t_np = generate_uint8(g, z_star.cuda())
    t_u8 = torch.from_numpy(t_np).cuda()
    out = {"g": g, "t_np": t_np, "z0": z0, "t64": torch.from_numpy(_lib.dequant_table())[torch.from_numpy(t_np).long()].double()}
    # the hand-written chain
    z = z0.clone().cuda()
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    hist, probes = [], {}
    for k in range(P_STEPS):
        dz, loss = eng.g_latent_grad(z, t_u8)
        if k in GRAD_STEPS:
            probes[k] = (z.cpu().clone(), dz.cpu().clone(), hip_signs_g(eng, P_SIZE, P_N))
        hist.append(loss)
        eng.op_adam(z, dz, m, v, k + 1, lr=P_LR, beta1=P_BETAS[0], beta2=P_BETAS[1])
    _, final = eng.g_latent_grad(z, t_u8)
    out["hand"] = (z.cpu(), torch.stack(hist).cpu(), final.cpu(), generate_uint8(g, z))
    out["probes"] = probes
    zl, recon, loss, history = project_signatures(g, t_np, steps=P_STEPS, lr=P_LR, betas=P_BETAS, z0=z0)
    out["loop"] = (zl.cpu(), history.cpu(), loss.cpu(), recon)
    return out


@pytest.fixture(scope="module")
def run():
    return compute_projection()


def test_loop_is_the_hand_chain_bit_for_bit(run):
    (hz, hh, hl, hr), (lz, lh, ll, lr) = run["hand"], run["loop"]
    assert lz.shape == (P_N, P_LATENT) and lh.shape == (P_STEPS, P_N) and ll.shape == (P_N,)
    assert lr.shape == (P_N, P_SIZE, P_SIZE) and lr.dtype == np.uint8
    assert torch.equal(lz, hz) and torch.equal(lh, hh) and torch.equal(ll, hl) and np.array_equal(lr, hr)
    assert not torch.equal(lz, run["z0"])


@pytest.mark.parametrize("k", GRAD_STEPS)
def test_gradient_along_the_path(run, k):
    z_k, dz, signs = run["probes"][k]
    rec = []
    ref, _ = oracle_latent_grad(oracle_sd64(P_SIZE, P_LATENT), z_k, run["t64"], P_SIZE, signs, 0.0, rec)
    from hipcommon import count_sign_flips
    count_sign_flips(signs, rec)
    err = float((dz.double() - ref).abs().max()) / float(ref.abs().max())
    print(f"step {k}: max|dz - dz_ref| / max|dz_ref| = {err:.3e}  (max|dz_ref| {float(ref.abs().max()):.3e})")
    assert err <= 1e-4, err


def test_descent_matches_the_oracles(run):
    ref = oracle_descent(run["t64"], run["z0"])
    r_ref = (ref[0] / ref[-1]).numpy()
    dev = run["loop"][1].double()
    r_dev = (dev[0] / dev[-1]).numpy()
    print(json.dumps({"oracle_loss0": ref[0].tolist(), "oracle_loss39": ref[-1].tolist(), "oracle_R": r_ref.tolist(),
                      "device_loss0": dev[0].tolist(), "device_loss39": dev[-1].tolist(), "device_R": r_dev.tolist()}))
    assert (r_ref > 2).all(), r_ref                      # the case descends at all
    assert (r_dev >= r_ref / 2).all(), (r_dev, r_ref)


def test_restarts_keep_the_lower_loss(run):
    from signature_gan_amd.utils.inference import project_signatures
    g, t = run["g"], run["t_np"]
    z, recon, loss, hist, cand = project_signatures(g, t, steps=P_STEPS, lr=P_LR, betas=P_BETAS, seed=7, restarts=2, return_candidates=True)
    cl, cz, ch, choice = cand["loss"].cpu(), cand["z"].cpu(), cand["history"].cpu(), cand["choice"].cpu()
    assert cl.shape == (2, P_N) and cz.shape == (2, P_N, P_LATENT) and ch.shape == (2, P_STEPS, P_N)
    assert torch.equal(loss.cpu(), cl.min(dim=0).values)
    for i in range(P_N):
        assert float(cl[choice[i], i]) == float(cl[:, i].min())
        assert torch.equal(z.cpu()[i], cz[choice[i], i]) and torch.equal(hist.cpu()[:, i], ch[choice[i], :, i])
    assert not torch.equal(cz[0], cz[1])
    z1, recon1, loss1, hist1 = project_signatures(g, t, steps=P_STEPS, lr=P_LR, betas=P_BETAS, seed=7, restarts=1)
    assert torch.equal(z1.cpu(), cz[0]) and torch.equal(loss1.cpu(), cl[0]) and torch.equal(hist1.cpu(), ch[0])
    z2, _, loss2, _ = project_signatures(g, t, steps=P_STEPS, lr=P_LR, betas=P_BETAS, seed=8, restarts=1)
    assert torch.equal(z2.cpu(), cz[1]) and torch.equal(loss2.cpu(), cl[1])      # restart 1 of seed 7 = the run seeded 8


def test_morph_frames_are_generate_uint8_at_the_blend(run):
    from signature_gan_amd.utils.inference import generate_uint8, morph_sequence
    g = run["g"]
    gen = torch.Generator().manual_seed(23)
    z_a, z_b = torch.randn(1, P_LATENT, generator=gen), torch.randn(1, P_LATENT, generator=gen)
    n = 6
    frames = morph_sequence(g, z_a.cuda(), z_b.cuda(), n)
    assert frames.shape == (n, P_SIZE, P_SIZE) and frames.dtype == np.uint8
    assert np.array_equal(frames[0], generate_uint8(g, z_a.cuda())[0]) and np.array_equal(frames[-1], generate_uint8(g, z_b.cuda())[0])
    for i in range(n):
        a = i / (n - 1)
        z = (1 - a) * z_a + a * z_b                      # the app's expression, on the CPU
        assert np.array_equal(frames[i], generate_uint8(g, z.cuda())[0]), i
    assert not np.array_equal(frames[0], frames[-1])


def test_cli_morph_and_project(run, tmp_path):
    from PIL import Image
    from signature_gan_amd import generate_signatures as cli
    sd, _, _ = projection_case()
    ck = tmp_path / "g.pt"
    torch.save({"epoch": 1, "generator_state_dict": sd, "config": {"latent_dim": P_LATENT, "image_size": P_SIZE}}, ck)
    out = tmp_path / "out"
    cli.main(["--checkpoint", str(ck), "--output_dir", str(out), "--seed", "3", "--morph", "--morph_frames", "4"])
    strip = Image.open(out / "signature_morph.png")
    assert strip.mode == "L" and strip.size == (4 * P_SIZE, P_SIZE)
    assert not (out / "signature_morph.json").exists() and not list(out.glob("signature_0*.png"))
    src = tmp_path / "real"
    src.mkdir()
    for i in range(2):
        Image.fromarray(run["t_np"][i], mode="L").save(src / f"sig_{i}.png")
    cli.main(["--checkpoint", str(ck), "--output_dir", str(out), "--seed", "3", "--prefix", "p", "--project", str(src),
              "--project_steps", "5", "--project_lr", "0.02", "--project_restarts", "2"])
    rec = json.load(open(out / "p_projection.json"))
    assert [r["file"] for r in rec] == ["sig_0.png", "sig_1.png"]
    for r in rec:
        assert set(r) == {"file", "reconstruction", "loss", "z"} and len(r["z"]) == P_LATENT and r["loss"] > 0
        im = Image.open(out / r["reconstruction"])
        assert im.mode == "L" and im.size == (P_SIZE, P_SIZE)
    cli.main(["--checkpoint", str(ck), "--output_dir", str(out), "--seed", "3", "--prefix", "m", "--morph", str(src / "sig_0.png"),
              str(src / "sig_1.png"), "--morph_frames", "3", "--project_steps", "5", "--threshold", "127", "--transparent"])
    info = json.load(open(out / "m_morph.json"))
    assert set(info) == {"files", "losses", "z"} and info["files"] == ["sig_0.png", "sig_1.png"]
    assert len(info["losses"]) == 2 and len(info["z"]) == 2 and len(info["z"][0]) == P_LATENT
    strip = Image.open(out / "m_morph.png")
    assert strip.mode == "RGBA" and strip.size == (3 * P_SIZE, P_SIZE)
