"""The fully-connected GAN extension (include/siggan_mlp.h; BASELINE.json configs[0]) on the MI355X against the build's own
CPU restatement (oracle/mlp_oracle.py).  PARITY UNPINNED: the reference has no such model, so these tests show that the HIP
path computes what the extension is defined to compute, nothing about the reference."""
import numpy as np
import pytest
import torch

import mlpcommon as MC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout,m,n,k", [("NT", 32, 256, 100), ("NT", 64, 784, 512), ("NT", 5, 1, 256), ("NN", 32, 512, 784),
                                          ("NN", 64, 100, 256), ("TN", 784, 512, 32), ("TN", 256, 100, 64), ("TN", 1, 256, 37)])
def test_gemm_layouts(layout, m, n, k):
    from signature_gan_amd.mlp_gan import op_gemm
    g = torch.Generator().manual_seed(m * 7 + n * 3 + k)
    if layout == "NT":
        a, b = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g); want = a @ b.t()
    elif layout == "NN":
        a, b = torch.randn(m, k, generator=g), torch.randn(k, n, generator=g); want = a @ b
    else:
        a, b = torch.randn(k, m, generator=g), torch.randn(k, n, generator=g); want = a.t() @ b
    got = op_gemm(layout, a.cuda(), b.cuda()).cpu()
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max()) + 1e-6


GEMM_EXACT_SHAPES = [(65, 63, 17), (1, 1, 1), (64, 64, 16), (33, 129, 15), (130, 5, 100)]


@pytest.mark.parametrize("m,n,k", GEMM_EXACT_SHAPES)
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
def test_gemm_layouts_exact_integers_and_bounds(layout, m, n, k):
    """Small integers from asymmetric index patterns: every product and sum is exact in fp32, so the result equals an int64
    matmul bit for bit, and a wrong lane-to-element map, a transposed operand or a mishandled ragged tile (a second row tile of
    one row, K below / just above one K-tile) cannot survive.  C lies between two sentinel-filled guard bands, each longer than
    a whole 64-row tile of C: rows past M and columns past N must not be written."""
    import ctypes as C
    from signature_gan_amd import _lib
    lay = {"NT": 0, "NN": 1, "TN": 2}[layout]
    a_shape = (k, m) if layout == "TN" else (m, k)
    b_shape = (n, k) if layout == "NT" else (k, n)
    ia, ib = torch.arange(a_shape[0] * a_shape[1], dtype=torch.int64), torch.arange(b_shape[0] * b_shape[1], dtype=torch.int64)
    a, b = ((7 * ia + 3) % 5 - 2).view(a_shape), ((11 * ib + 1) % 7 - 3).view(b_shape)
    want = (a.t() if layout == "TN" else a) @ (b.t() if layout == "NT" else b)
    assert int(want.abs().max()) < 2 ** 24
    guard, sentinel = 64 * n + 64, -12345.0
    buf = torch.full((guard + m * n + guard,), sentinel, dtype=torch.float32, device="cuda:0")
    da, db = a.float().cuda(), b.float().cuda()
    _lib.check(_lib.load().mlpgan_op_gemm(0, lay, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()),
                                          C.c_void_p(buf.data_ptr() + 4 * guard), m, n, k,
                                          C.c_void_p(torch.cuda.current_stream(buf.device).cuda_stream)))
    host = buf.cpu()
    assert torch.equal(host[guard:guard + m * n].view(m, n), want.float())
    assert bool((host[:guard] == sentinel).all()) and bool((host[guard + m * n:] == sentinel).all()), "written outside C"


def _states(model, seed):
    from oracle import mlp_oracle as M
    from oracle.siggan_oracle import AdamState
    gen = torch.Generator().manual_seed(seed)
    g_sd, d_sd = {}, {}
    for which, sd in (("g", g_sd), ("d", d_sd)):
        for k, v in model.views(which).items():
            t = torch.empty(v.shape).normal_(1.0 if ".bn.weight" in k else 0.0, 0.05, generator=gen)
            v.copy_(t); sd[k] = t.clone()
    for k, v in model.bn_views().items():
        if "num_batches" in k:
            g_sd[k] = torch.zeros((), dtype=torch.int64)
        else:
            t = torch.rand(v.shape, generator=gen) * 0.5 + (0.75 if "var" in k else -0.25)
            v.copy_(t); g_sd[k] = t.clone()
    return g_sd, d_sd, AdamState(list(model.g_spans), g_sd), AdamState(list(model.d_spans), d_sd), M


@pytest.mark.parametrize("size,hidden,batch", [(28, (256, 512), 32), (64, (256, 512, 1024), 64), (28, (128,), 5)])
def test_mlp_steps_vs_own_oracle(size, hidden, batch):
    """configs[0] (28x28, 100-256-512-784, batch 32) and two other geometries: forward, one D step, one G step -- losses,
    predictions, gradients, BatchNorm buffers, updated weights -- against oracle/mlp_oracle.py (parity unpinned)."""
    from signature_gan_amd.mlp_gan import MLPGAN
    m = MLPGAN(latent_dim=100, image_size=size, hidden=hidden, max_batch=batch, device="cuda:0", seed=1)
    g_sd, d_sd, g_opt, d_opt, M = _states(m, 7)
    gen = torch.Generator().manual_seed(3)
    z, z2 = torch.randn(batch, 100, generator=gen), torch.randn(batch, 100, generator=gen)
    real = torch.rand(batch, 1, size, size, generator=gen) * 2 - 1

    img = m.generate(z.cuda()).cpu()
    want = M.g_forward(dict(g_sd), z, hidden, size, training=False)
    assert float((img - want).abs().max()) <= 2e-4
    p = m.discriminate(real.cuda()).cpu()
    assert float((p - M.d_forward(d_sd, real, len(hidden))).abs().max()) <= 2e-5

    case = MC.Case("own", size, hidden, batch, batch, 100, 0)
    before = MC.snapshot_model(m)
    met = m.train_discriminator_step(real.cuda(), noise=z.cuda())
    after = MC.snapshot_model(m)
    o_met, o_grads = M.d_step(g_sd, d_sd, d_opt, real, z, hidden, size)
    for k, v in o_met.items():
        assert abs(met[k] - v) <= 2e-4 * abs(v) + 2e-6, (k, met[k], v)
    gs = max(float(g.abs().max()) for g in o_grads.values())
    for k, g in m.views("d", "grads").items():
        assert float((g.cpu() - o_grads[k]).abs().max()) <= 2e-4 * max(float(o_grads[k].abs().max()), 1e-3 * gs), k
    # the update: Adam step 1 (fp64) of HIP's own gradients on HIP's own parameters and moments (mlpcommon's update check;
    # "within 2.5 lr of the oracle's weights", which stood here, holds for a step that is skipped or reversed as well)
    MC.check_update("d", case, before, after, 1, "D step")
    for k in [f"g_{a}" for a in MC.ARENAS] + list(MC.BN_KEYS):
        assert torch.equal(after[k], before[k]), f"the D step changed {k}"

    before = after
    met = m.train_generator_step(batch, noise=z2.cuda())
    after = MC.snapshot_model(m)
    o_met, o_grads = M.g_step(g_sd, d_sd, g_opt, z2, hidden, size)
    for k, v in o_met.items():
        assert abs(met[k] - v) <= 2e-4 * abs(v) + 2e-6, (k, met[k], v)
    gs = max(float(g.abs().max()) for g in o_grads.values())
    for k, g in m.views("g", "grads").items():
        # (a ReLU whose pre-activation is within rounding of zero may fall on either side: bounded as in the conv tests)
        assert float((g.cpu() - o_grads[k]).abs().max()) <= 5e-3 * max(float(o_grads[k].abs().max()), 1e-2 * gs), k
    for k, v in m.bn_views().items():
        ref = g_sd[k].float()
        assert float((v.float().cpu() - ref).abs().max()) <= 2e-4 * float(ref.abs().max()) + 1e-6, k
    MC.check_update("g", case, before, after, 1, "G step")
    for a in MC.ARENAS:
        assert torch.equal(after[f"d_{a}"], before[f"d_{a}"]), f"the G step changed d_{a}"
    assert after["g_bn_batches"].tolist() == [1] * len(hidden) and float(after["d_adam_steps"][0]) == 1.0
    # a few more steps from the library RNG: finite, losses move
    for _ in range(3):
        t = m.train_step(real.cuda())
    assert all(np.isfinite(v) for v in t.values())
    m.close()
