"""The ablation study's LeakyReLU Generator on the host: the oracle's restatement (oracle.siggan_oracle with g_slope /
slope = common.SLOPE) against the fixtures the reference's own AblationGANTrainer.train_epoch wrote
(tests/golden/make_golden_ablation_leaky.py), and host checks of the drop-in module.  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

from common import (GOLDEN, SLOPE, I, O, SEED, ablation_groups, assert_close, census_signs, d_chans, oracle_states,
                    oracle_states_sn, probe)
from test_oracle_golden import _check_step

import signature_gan_amd  # noqa: F401  (import shim for signature-gan_amd/)

# (size, latent, batch, spectral norm): z = 50 (latent % 4 != 0) runs the Generator fc's generic kernels
LEAKY_CASES = [(64, 200, 8, False), (64, 50, 8, True), (128, 128, 4, False)]


@pytest.fixture(autouse=True)
def _fixture_thread_count():
    n = torch.get_num_threads()
    torch.set_num_threads(8)              # the reference run's thread count (fixture meta 'threads'): same summation order
    yield
    torch.set_num_threads(n)


def _fixture():
    return np.load(os.path.join(GOLDEN, "golden_ablation_leaky.npz"))


@pytest.mark.parametrize("size,latent,batch,sn", LEAKY_CASES)
def test_restatement_reproduces_reference_iteration(size, latent, batch, sn):
    """restatement(fixture census) == the reference's first ablation iteration with ConfigurableGenerator(leaky_relu)."""
    f = _fixture()
    tag = f"s{size}_z{latent}_b{batch}" + ("_sn" if sn else "")
    masks = [torch.from_numpy(m) for m in I.unpack_masks(f[f"{tag}/masks"], batch, d_chans(size) * 3)]
    nb = len(masks) // 3
    z = torch.from_numpy(f[f"{tag}/z"])
    real = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))
    g_sd, d_sd, g_opt, d_opt, sn_uv = oracle_states_sn(size, latent, sn)
    preds = []
    met, d_grads, g_grads = O.ablation_step(g_sd, d_sd, g_opt, d_opt, real, z, masks[:nb], masks[nb:2 * nb], masks[2 * nb:],
                                            size, signs=ablation_groups(size, census_signs(f, tag)), g_slope=SLOPE, sn=sn_uv,
                                            preds=preds)
    assert_close(torch.stack(preds).numpy(), f[f"{tag}/preds"], 1e-4, 1e-6, f"{tag} D predictions")
    if sn:
        for k, v in sn_uv.items():                     # three power iterations later
            assert_close(probe(v, k), f[f"{tag}/d/sn/{k}"], 1e-4, 1e-6, f"{tag} {k}")
    _check_step(f, f"{tag}/d", d_opt.names, {k: v for k, v in met.items() if k.startswith("d_")}, d_grads, d_sd, d_opt)
    bufs = [k for k in g_sd if k not in g_opt.names]
    _check_step(f, f"{tag}/g", g_opt.names, {"g_loss": met["g_loss"]}, g_grads, g_sd, g_opt, bufs)
    # generate_samples after the iteration: eval mode on the updated weights and running statistics
    with torch.no_grad():
        img = O.g_forward(g_sd, torch.from_numpy(f[f"{tag}/eval/z"]), False, size, slope=SLOPE)
    want = f[f"{tag}/eval/img"]
    assert_close(img.numpy(), want, 0, 1e-4 * float(np.abs(want).max()), f"{tag} eval image")


def test_restatement_reproduces_reference_epoch_means():
    """Three iterations of train_epoch from the fixture's z and masks: the four epoch means the reference returned."""
    f = _fixture()
    size, latent, batch, n = (int(v) for v in f["epoch/case"])
    masks = [torch.from_numpy(m) for m in I.unpack_masks(f["epoch/masks"], batch, d_chans(size) * 3 * n)]
    per = len(masks) // n
    nb = per // 3
    g_sd, d_sd, g_opt, d_opt = oracle_states(size, latent, warm=True)
    sums = np.zeros(4)
    for k in range(n):
        real = torch.from_numpy(I.gen_real(batch, size, SEED["real"] + k))
        ms = masks[k * per:(k + 1) * per]
        met, _, _ = O.ablation_step(g_sd, d_sd, g_opt, d_opt, real, torch.from_numpy(f["epoch/z"][k]), ms[:nb], ms[nb:2 * nb],
                                    ms[2 * nb:], size, g_slope=SLOPE)
        sums += [met["g_loss"], met["d_loss"], met["d_real_mean"], met["d_fake_mean"]]
    # own sign decisions here (no census for iterations 2-3): a borderline flip moves a chained mean by far less than 1e-4
    assert_close(sums / n, f["epoch/means"], 1e-4, 1e-6, "epoch means")
    assert np.array_equal(f["epoch/lists"][:, 0], f["epoch/means"])


def test_slope_zero_is_the_relu_oracle():
    """The oracle's Generator with its default slope is the ReLU network -- slope=0.0 bit for bit -- and slope=SLOPE is another
    one."""
    size, latent, batch = 64, 100, 4
    g_sd, *_ = oracle_states(size, latent, warm=False)
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    a = O.g_forward({k: v.clone() for k, v in g_sd.items()}, z, True, size, slope=0.0)
    b = O.g_forward({k: v.clone() for k, v in g_sd.items()}, z, True, size)
    assert torch.equal(a, b)
    c = O.g_forward({k: v.clone() for k, v in g_sd.items()}, z, True, size, slope=SLOPE)
    assert not torch.equal(a, c)


def test_configurable_generator_keys_and_activation_rule():
    """ConfigurableGenerator: the reference's state_dict keys (fixture manifest) and attributes; any activation other than
    'leaky_relu' is ReLU (ablation...py:198-201, 283-286)."""
    from signature_gan_amd.ablation_vanilla_gan_signatures import ConfigurableGenerator
    from signature_gan_amd.generator_vanilla_gan import Generator
    meta = json.loads(str(_fixture()["meta"]))
    for size, latent, _, _ in LEAKY_CASES:
        g = ConfigurableGenerator(latent_dim=latent, output_size=size, activation="leaky_relu")
        assert list(g.state_dict()) == meta["g_state_dict_keys"][f"s{size}_z{latent}"]
        assert list(g.state_dict()) == list(Generator(latent_dim=latent, output_size=size).state_dict())
        for k, t in g.state_dict().items():
            assert tuple(t.shape) == tuple(O.g_state_specs(latent, size)[k][0]), k
        assert (g.latent_dim, g.output_size, g.output_channels, g.base_features, g.activation) == (latent, size, 1, 256, "leaky_relu")
        assert (g.init_size, g.init_channels) == (4, 256 if size == 64 else 512)
    lk = ConfigurableGenerator(activation="leaky_relu", leaky_slope=0.1)._engine_kwargs()
    assert lk["g_activation"] == "leaky_relu" and lk["g_leaky_slope"] == 0.1
    for act in ("relu", "ReLU", "leaky", "elu", ""):
        assert ConfigurableGenerator(activation=act)._engine_kwargs()["g_activation"] == "relu", act


def test_configurable_generator_constructor_errors():
    from signature_gan_amd.ablation_vanilla_gan_signatures import ConfigurableGenerator
    with pytest.raises(ValueError, match="output_size must be 64 or 128"):
        ConfigurableGenerator(output_size=32)
    with pytest.raises(ValueError):
        ConfigurableGenerator(output_channels=3)
    with pytest.raises(ValueError):
        ConfigurableGenerator(base_features=128)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ConfigurableGenerator(activation="leaky_relu")(torch.zeros(2, 100))


def test_ablation_config_and_result():
    from signature_gan_amd.ablation_vanilla_gan_signatures import AblationConfig, AblationResult
    c = AblationConfig(name="x", latent_dim=200, activation="leaky_relu", use_spectral_norm=True)
    assert c.get_short_name() == "z200_LReLU_SN"
    assert AblationConfig(name="y", latent_dim=50).get_short_name() == "z50_ReLU_noSN"
    d = c.to_dict()
    assert (d["batch_size"], d["epochs"], d["g_lr"], d["beta1"], d["label_smoothing"]) == (64, 50, 2e-4, 0.5, 0.9)
    r = AblationResult(config=c, g_losses=[1.0, 2.0, 3.0], d_losses=[0.5, 0.5])
    r.compute_stability_metrics()
    assert r.final_g_loss == 3.0 and r.loss_variance_g == pytest.approx(2.0 / 3.0) and r.loss_variance_d == 0.0
    assert r.to_dict()["config"]["name"] == "x" and r.to_dict()["fid_score"] is None


def test_engine_rejects_unknown_g_activation():
    from signature_gan_amd.engine import Engine
    with pytest.raises(ValueError, match="g_activation"):
        Engine(g_activation="elu", device="cuda:0")


def test_abi_carries_the_generator_slope():
    """siggan_config ends with the float g_leaky_slope (ABI 4)."""
    from signature_gan_amd import _lib
    assert _lib.ABI_VERSION == 4
    assert _lib.Config._fields_[-1] == ("g_leaky_slope", _lib.C.c_float)
    assert _lib.load().siggan_abi_version() == 4
