"""Realism-filtered generation end to end (utils.inference.generate_signatures_filtered and the CLI's --filter_by_realism):
the device route -- bytes into an HBM pool, scores from the byte-reading Discriminator, one select_topk, one gather_u8 --
against the host route, the reference's loop on the parent pieces (bytes to the host, numpy binarisation, CPU
dequantisation, Discriminator.forward, Python's sort).  n = 10 at ratio 2.5 and batch size 8: 25 images in four batches,
the last of one image.

The networks are reference_init's under a fixed seed, with two gains on top, as tests/test_generate_u8_gpu.py does: a fresh
Generator's pre-tanh values are about 1e-3, so every byte is 127 (the CPU oracle), and a fresh Discriminator's logits are
about 1e-4, where all 25 scores are the same float (measured: 0.4999774098396301 each) and only the tie rule is exercised.
The Generator's final conv is multiplied by 1024 (the oracle's bytes then span 32..222) and the Discriminator's classifier
weight by 1024 (logits of order 1 to 10)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, RATIO, BATCH, LATENT, SEEDV = 10, 2.5, 8, 100, 1234
SETTINGS = {"plain": dict(), "threshold": dict(threshold=127), "noise": dict(noise_scale=0.8),
            "both": dict(threshold=127, noise_scale=0.8)}


@pytest.fixture(scope="module")
def nets():
    from signature_gan_amd.discriminator_vanilla_gan import Discriminator
    from signature_gan_amd.generator_vanilla_gan import Generator
    torch.manual_seed(7)                                                  # reference_init draws from torch's generator
    g = Generator(latent_dim=LATENT, output_size=64).to("cuda").eval()
    d = Discriminator(input_size=64).to("cuda").eval()
    with torch.no_grad():
        g.state_dict()["final_conv.0.weight"].mul_(1024.0)
        d.state_dict()["classifier.0.weight"].mul_(1024.0)
    g._engine.params_changed(); d._engine.params_changed()
    return g, d


@pytest.fixture(scope="module")
def runs(nets):
    from signature_gan_amd.utils.inference import generate_signatures_filtered
    g, d = nets
    out = {}
    for name, kw in SETTINGS.items():
        for route in ("device", "host"):
            ticks = []
            images, scores = generate_signatures_filtered(g, d, N, LATENT, torch.device("cuda"), seed=SEEDV, batch_size=BATCH,
                                                          oversampling_ratio=RATIO, route=route, progress_callback=ticks.append, **kw)
            out[name, route] = ([np.array(im) for im in images], scores, ticks, [im.mode for im in images])
    return out


@pytest.mark.parametrize("name", list(SETTINGS))
def test_device_route_is_the_host_route(runs, name):
    dev, host = runs[name, "device"], runs[name, "host"]
    print(name, dev[1], host[1])
    assert len(dev[0]) == len(host[0]) == N and len(dev[1]) == len(host[1]) == N
    assert set(dev[3]) == set(host[3]) == {"L"}
    for a, b in zip(dev[0], host[0]):
        assert a.shape == (64, 64) and a.dtype == np.uint8 and np.array_equal(a, b)
    assert dev[1] == host[1]                                              # exact: the same float32 values
    assert all(isinstance(s, float) for s in dev[1])
    assert dev[2] == host[2] == [8 / 25, 16 / 25, 24 / 25, 1.0]


@pytest.mark.parametrize("name", list(SETTINGS))
def test_scores_do_not_increase_and_the_selection_is_real(runs, name):
    images, scores, _, _ = runs[name, "device"]
    assert all(a >= b for a, b in zip(scores, scores[1:]))
    assert len(set(scores)) > 1                                           # 25 different images: the ranking had something to rank
    if "threshold" in SETTINGS[name]:
        assert all(set(np.unique(im)) <= {0, 255} for im in images)
    else:
        assert any(len(np.unique(im)) > 16 for im in images)


def test_the_settings_change_the_result(runs):
    assert runs["plain", "device"][1] != runs["threshold", "device"][1]
    assert runs["plain", "device"][1] != runs["noise", "device"][1]


def test_selection_is_the_top_of_the_whole_pool(nets):
    """Keeping everything (n = total) returns the pool itself in rank order, and the top 10 of that are what n = 10 returns."""
    from signature_gan_amd.utils.inference import generate_signatures_filtered
    g, d = nets
    full = generate_signatures_filtered(g, d, 25, LATENT, torch.device("cuda"), seed=SEEDV, batch_size=BATCH, oversampling_ratio=1.0)
    # 25 images at ratio 1.0 in batches of 8 with the same seeds: the same pool as 10 at ratio 2.5
    top = generate_signatures_filtered(g, d, N, LATENT, torch.device("cuda"), seed=SEEDV, batch_size=BATCH, oversampling_ratio=RATIO)
    assert len(full[0]) == 25 and full[1][:N] == top[1]
    assert all(np.array_equal(np.array(a), np.array(b)) for a, b in zip(full[0][:N], top[0]))


def test_train_mode_generator_falls_back_to_the_host_route(nets):
    from signature_gan_amd.utils.inference import generate_signatures_filtered
    g, d = nets
    state = {k: v.clone() for k, v in g.state_dict().items()}
    g.train()
    try:
        images, scores = generate_signatures_filtered(g, d, 3, LATENT, torch.device("cuda"), seed=1, batch_size=4, oversampling_ratio=2.0)
    finally:
        g.eval()
        g.load_state_dict(state)                                          # the BatchNorm running statistics moved
    assert len(images) == 3 and all(a >= b for a, b in zip(scores, scores[1:]))


def test_cli_writes_the_selection_in_rank_order(nets, tmp_path, capsys):
    from PIL import Image
    from signature_gan_amd import generate_signatures as cli
    from signature_gan_amd.utils.inference import generate_signatures_filtered
    g, d = nets
    ck = tmp_path / "checkpoint.pth"
    torch.save({"generator_state_dict": g.state_dict(), "discriminator_state_dict": d.state_dict(),
                "config": {"latent_dim": LATENT, "image_size": 64}}, ck)
    out = tmp_path / "out"
    cli.main(["--checkpoint", str(ck), "--n_samples", str(N), "--output_dir", str(out), "--batch_size", str(BATCH), "--seed", str(SEEDV),
              "--prefix", "sig", "--filter_by_realism", "--oversampling_ratio", str(RATIO), "--threshold", "127"])
    records = json.load(open(out / "sig_scores.json"))
    names = [f"sig_{i + 1:06d}.png" for i in range(N)]
    assert [r["file"] for r in records] == names
    assert sorted(os.listdir(out)) == sorted(names + ["sig_scores.json"])
    want_images, want_scores = generate_signatures_filtered(g, d, N, LATENT, torch.device("cuda"), seed=SEEDV, batch_size=BATCH,
                                                            oversampling_ratio=RATIO, threshold=127, route="host")
    assert [r["score"] for r in records] == want_scores
    for name, want in zip(names, want_images):
        img = Image.open(out / name)
        assert img.mode == "1" and np.array_equal(np.array(img.convert("L")), np.array(want))
    # a checkpoint without Discriminator weights: a clear message and a non-zero exit, not an unfiltered run
    gonly = tmp_path / "generator_only.pth"
    torch.save({"generator_state_dict": g.state_dict(), "config": {"latent_dim": LATENT, "image_size": 64}}, gonly)
    with pytest.raises(SystemExit) as e:
        cli.main(["--checkpoint", str(gonly), "--output_dir", str(tmp_path / "none"), "--filter_by_realism"])
    assert e.value.code not in (0, None) and "discriminator_state_dict" in str(e.value.code)
    assert not (tmp_path / "none").exists()
