"""Diverse selection behind the device resize on the MI355X: a 128x128 Generator's pool reaches the 64x64 verifier through
SiameseNetwork.embed_resized (utils.inference.generate_signatures_diverse(verifier_resize=True)).  The case stands beside the
resize's other consumers (tests/test_resize_gpu.py) and not in tests/test_diverse_gpu.py because it creates the process-wide
resize context, and tests/test_resize_cpu.py -- which sorts between the two files -- asserts that its refusals have created
none.  Networks: reference_init under a fixed seed with the two gains of tests/test_realism_filter_gpu.py, the E = 40 verifier
of verifiercommon."""
import numpy as np
import pytest
import torch

import verifiercommon as VC

pytestmark = pytest.mark.gpu

DEV, LATENT, SEEDV, E = "cuda", 100, 1234, 40


def test_pipeline_reads_a_128_generator_through_the_resize():
    """A 128x128 Generator needs verifier_resize (embed_resized); the picks are select_diverse's on those embeddings."""
    from signature_gan_amd import signature_verifier_eval as SV
    from signature_gan_amd.discriminator_vanilla_gan import Discriminator
    from signature_gan_amd.generator_vanilla_gan import Generator
    from signature_gan_amd.utils.diverse import select_diverse
    from signature_gan_amd.utils.inference import generate_signatures_diverse
    v = SV.SiameseNetwork(E, max_images=16)
    v.load_state_dict(VC.torch_state(E), strict=True)
    v = v.to(DEV).eval()
    torch.manual_seed(9)
    g = Generator(latent_dim=LATENT, output_size=128).to(DEV).eval()
    d = Discriminator(input_size=128).to(DEV).eval()
    with torch.no_grad():
        g.state_dict()["final_conv.0.weight"].mul_(1024.0)
        d.state_dict()["classifier.0.weight"].mul_(1024.0)
    g._engine.params_changed(); d._engine.params_changed()
    args = (g, d, v, 4, LATENT, torch.device(DEV))
    kw = dict(seed=SEEDV, batch_size=8, oversampling_ratio=3.0, keep_ratio=1.0)
    with pytest.raises(ValueError, match="verifier_resize"):
        generate_signatures_diverse(*args, **kw)
    images, scores, report = generate_signatures_diverse(*args, verifier_resize=True, return_pool=True, **kw)
    dev = report["_device"]
    assert tuple(dev["pool"].shape) == (12, 128, 128) and torch.equal(dev["embeddings"], v.embed_resized(dev["pool"]))
    order = select_diverse(dev["embeddings"], 4, dev["eligible"], None, int(torch.argmax(dev["scores"])), 0.0)[0].cpu().tolist()
    assert [p["pool_index"] for p in report["picks"]] == order and len(images) == 4
    assert all(np.array_equal(np.array(im), dev["pool"][p].cpu().numpy()) for im, p in zip(images, order))
