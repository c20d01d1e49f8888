"""The fully-connected GAN's training steps on the MI355X where tests/test_mlp_gpu.py does not take them: chains of steps,
widths that are no power of two, a batch below max_batch, batch 1, clipping, the library's own noise, and every refusal of the
mlpgan_* entry points.  The yardstick (fp64 oracle, bound, near ties, update check) is tests/mlpcommon.py; tests/test_mlp_cpu.py
shows on the CPU that it is attainable and that it rejects wrong updates.  PARITY UNPINNED: the reference has no such model."""
import ctypes as C

import pytest
import torch

import mlpcommon as MC

pytestmark = pytest.mark.gpu

MARGINS = None                                         # profiles/mlp_parity_margins.py collects the observed margins here
STALE, ONE = MC.STALE, MC.ONE


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_chained_steps(case):
    """Three D + G pairs with given noise; every step is compared, as one step from the state read back before it, with the
    fp64 oracle: metrics, every gradient, the update (and that D's out.bias, the odd-length arena's last element, moved), the
    running statistics and counters.  The D steps of rounds 2 and 3 run G in eval mode on statistics a G step has just moved."""
    b = MC.HipBackend(case)
    try:
        MC.run_chain(b, case, MARGINS)
    finally:
        b.close()


@pytest.mark.parametrize("factor", [0.5, 2.0])
def test_clipping(factor):
    b = MC.HipBackend(MC.CASES[0])
    try:
        MC.run_clipped(b, MC.CASES[0], factor, MARGINS)
    finally:
        b.close()


def _pair(b, real, zd, zg):
    """D + G step; returns the raw metrics buffer after each."""
    out = []
    b.m.train_discriminator_step(real.cuda(), noise=zd.cuda())
    out.append(b.m.metrics.cpu().clone())
    b.m.train_generator_step(real.shape[0], noise=zg.cuda())
    out.append(b.m.metrics.cpu().clone())
    return out


def test_smaller_batch_after_larger_is_bitwise_a_fresh_context():
    """The workspace is carved for max_batch and addressed by the call's batch: after a batch-32 pair stale rows lie behind the
    five live ones.  Nothing may read them."""
    st = MC.make_state(STALE)
    big = MC.make_inputs(STALE, batch=STALE.max_batch, rounds=1, seed=11)[0]
    small = MC.make_inputs(STALE, rounds=1)[0]
    used, fresh = MC.HipBackend(STALE), MC.HipBackend(STALE)
    try:
        used.load(st)
        _pair(used, *big)
        used.load(st)
        used.m.metrics.zero_()
        fresh.load(st)
        got, want = _pair(used, *small), _pair(fresh, *small)
        for g, w, name in zip(got, want, ("D", "G")):
            assert torch.equal(g, w), f"metrics after the {name} step differ: {g.tolist()} vs {w.tolist()}"
        a, c = used.snapshot(), fresh.snapshot()
        assert float(a["d_adam_steps"][0]) == 1.0 and float(a["g_adam_steps"][0]) == 1.0 and not torch.equal(a["g_params"], st["g_params"])
        for k in MC.STATE_KEYS:
            assert torch.equal(a[k], c[k]), f"{k} differs from the fresh context's"
    finally:
        used.close(); fresh.close()


def test_batch_one():
    """Eval-mode generation, discrimination and a D step at batch 1 are ordinary; BatchNorm batch statistics over one row
    are refused as torch's BatchNorm1d refuses them, before anything is enqueued."""
    from oracle import mlp_oracle as M
    b = MC.HipBackend(ONE)
    try:
        st = MC.make_state(ONE)
        b.load(st)
        real, zd, zg = MC.make_inputs(ONE, rounds=1)[0]
        ref = {}
        for dt in (torch.float64, torch.float32):
            g_sd, d_sd, _, _ = MC.oracle_from(st, ONE, dt)
            ref[dt] = (M.g_forward(g_sd, zd.to(dt), ONE.hidden, ONE.size, training=False), M.d_forward(d_sd, real.to(dt), len(ONE.hidden)))
        MC.check_tensor(b.m.generate(zd.cuda()).cpu(), ref[torch.float64][0], ref[torch.float32][0], "one generate", MARGINS)
        MC.check_tensor(b.m.discriminate(real.cuda()).cpu(), ref[torch.float64][1], ref[torch.float32][1], "one discriminate", MARGINS)
        assert all(torch.equal(v, st[k]) for k, v in b.snapshot().items()), "a forward pass changed the state"

        before = b.snapshot()
        real, zd = MC.pick_inputs("d", ONE, before, 0)
        met = b.d_step(real, zd)
        after = b.snapshot()
        MC.check_step("d", ONE, before, after, met, real, zd, 1, margins=MARGINS, what="one D")

        raw = b.m.metrics.cpu().clone()
        with pytest.raises(ValueError, match="BatchNorm.*Expected more than 1 value per channel when training"):
            b.m.train_generator_step(1, noise=zg.cuda())
        with pytest.raises(ValueError, match="BatchNorm.*Expected more than 1 value per channel when training"):
            b.m.train_generator_step(1)                                            # (nor is any library noise drawn)
        with pytest.raises(ValueError, match="BatchNorm.*Expected more than 1 value per channel when training"):
            b.m.generate(zg.cuda(), training=True)
        for k, v in b.snapshot().items():
            assert torch.equal(v, after[k]), f"a refused call changed {k}"
        assert torch.equal(b.m.metrics.cpu(), raw)
        assert b.m.generate(zg.cuda(), training=False).shape == (1, 1, ONE.size, ONE.size)
    finally:
        b.close()


def test_library_noise():
    """noise=None: D draws from stream 1, G from stream 2, and every optimiser update starts a new RNG epoch.  With both learning
    rates 0 the weights stay put, so whatever moves between calls is the noise."""
    case = MC.CASES[0]
    st = MC.make_state(case)
    real = MC.make_inputs(case, rounds=1)[0][0].cuda()
    runs = {}
    for name, seed in (("a", 5), ("b", 5), ("other", 6)):
        b = MC.HipBackend(case, seed=seed, g_lr=0.0, d_lr=0.0)
        try:
            b.load(st)
            out = []
            for _ in range(3):
                b.m.train_step(real)
                out.append(b.m.metrics.cpu().clone())
            # two D steps with no G step between: weights and running statistics stand still, only the noise can move d_fake_mean
            twice = [b.m.train_discriminator_step(real)["d_fake_mean"] for _ in range(2)]
            assert twice[0] != twice[1], f"d_fake_mean of successive D steps {twice}: the noise did not advance"
            snap = b.snapshot()
            assert torch.equal(snap["g_params"], st["g_params"]) and torch.equal(snap["d_params"], st["d_params"])
            assert float(snap["d_adam_steps"][0]) == 5.0 and float(snap["g_adam_steps"][0]) == 3.0
            runs[name] = torch.stack(out)
        finally:
            b.close()
    from signature_gan_amd._lib import METRIC_INDEX as MI
    assert torch.isfinite(runs["a"]).all()
    assert torch.equal(runs["a"], runs["b"]), "the same seed must give the same noise"
    for k in ("d_fake_mean", "g_fake_mean"):
        assert not torch.equal(runs["a"][:, MI[k]], runs["other"][:, MI[k]]), f"{k}: another seed gave the same noise"
    col = runs["a"][:, MI["g_fake_mean"]].tolist()      # (batch statistics and a D that stands still: only the noise moves it)
    assert len(set(col)) == 3, f"g_fake_mean of successive steps {col}: the noise did not advance"
    assert torch.equal(runs["a"][:, MI["d_real_mean"]], runs["other"][:, MI["d_real_mean"]])       # (no noise in the real half)


def test_refusals():
    """Every refusal of the mlpgan_* entry points: the stated code, a message in siggan_last_error(), and nothing written --
    a sentinel-filled output and every bound arena are unchanged after each."""
    from signature_gan_amd import _lib
    lib = _lib.load()
    OK, E_INVALID, E_STATE = 0, -1, -2
    dev = torch.device("cuda:0")
    latent, size, hidden, bm = 10, 8, (12, 8), 4

    def create(latent_dim=latent, image_size=size, n_hidden=len(hidden), widths=hidden, max_batch=bm):
        hid = (C.c_int32 * 4)(*(list(widths) + [0] * (4 - len(widths))))
        cfg = _lib.MlpConfig(0, latent_dim, image_size, n_hidden, hid, max_batch, 0.2, 0)
        h = C.c_void_p()
        return lib.mlpgan_create(C.byref(cfg), C.byref(h)), h

    def message():
        return lib.siggan_last_error().decode("utf-8", "replace")

    for kw, text in ((dict(n_hidden=0), "n_hidden"), (dict(n_hidden=5), "n_hidden"), (dict(widths=(6, 8)), "hidden widths"),
                     (dict(widths=(12, 0)), "hidden widths"), (dict(widths=(8196, 8)), "hidden widths"), (dict(image_size=3), "geometry"),
                     (dict(latent_dim=0), "geometry"), (dict(max_batch=0), "geometry")):
        rc, h = create(**kw)
        assert rc == E_INVALID and h.value is None and text in message(), (kw, rc, h.value, message())

    rc, h = create()
    assert rc == OK and h.value
    try:
        ng, nd, nbn = lib.mlpgan_param_count(h, 0), lib.mlpgan_param_count(h, 1), lib.mlpgan_bn_count(h)
        assert nbn == sum(hidden)
        gen = torch.Generator().manual_seed(0)
        f = lambda n: torch.randn(n, generator=gen).to(dev)                          # noqa: E731
        arenas = dict(g_params=f(ng), g_grads=f(ng), g_exp_avg=f(ng), g_exp_avg_sq=f(ng).abs(), g_adam_steps=torch.full((lib.mlpgan_param_tensors(h, 0),), 3.0, device=dev),
                      g_bn_running_mean=f(nbn), g_bn_running_var=f(nbn).abs() + 0.5, g_bn_batches=torch.full((len(hidden),), 7, dtype=torch.int64, device=dev),
                      d_params=f(nd), d_grads=f(nd), d_exp_avg=f(nd), d_exp_avg_sq=f(nd).abs(), d_adam_steps=torch.full((lib.mlpgan_param_tensors(h, 1),), 3.0, device=dev))
        z, x = f(bm * latent).view(bm, latent), f(bm * size * size).view(bm, 1, size, size)
        img, probs, metrics = torch.full((bm, 1, size, size), -7.0, device=dev), torch.full((bm,), -7.0, device=dev), torch.full((_lib.M_COUNT,), -7.0, device=dev)
        watched = dict(arenas, z=z, x=x, img=img, probs=probs, metrics=metrics)
        torch.cuda.synchronize()
        saved = {k: v.clone() for k, v in watched.items()}
        hp = _lib.Hyper(2e-4, 0.5, 0.999, 1e-8, 0.9, 0.0, 1.0)
        p = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def g_forward(z_=z, batch=2, training=0, img_=img):
            return lib.mlpgan_g_forward(h, p(z_) if z_ is not None else None, batch, training, p(img_) if img_ is not None else None, stream)

        def d_forward(x_=x, batch=2, probs_=probs):
            return lib.mlpgan_d_forward(h, p(x_) if x_ is not None else None, batch, p(probs_) if probs_ is not None else None, stream)

        def d_step(real=x, batch=2, z_=z, hp_=hp):
            return lib.mlpgan_d_step(h, p(real) if real is not None else None, batch, p(z_) if z_ is not None else None,
                                     C.byref(hp_) if hp_ is not None else None, p(metrics), stream)

        def g_step(batch=2, z_=z, hp_=hp):
            return lib.mlpgan_g_step(h, batch, p(z_) if z_ is not None else None, C.byref(hp_) if hp_ is not None else None, p(metrics), stream)

        def refused(rc, code, text, what):
            assert rc == code and text in message(), (what, rc, message())
            torch.cuda.synchronize()
            for k, v in watched.items():
                assert torch.equal(v, saved[k]), f"{what}: refused, but {k} changed"

        for name, call in (("g_forward", g_forward), ("d_forward", d_forward), ("d_step", d_step), ("g_step", g_step)):
            refused(call(), E_STATE, "mlpgan_bind has not been called", f"{name} before bind")

        def bind(without=()):
            st = _lib.MlpStorage(*[None if k in without else arenas[k].data_ptr() for k, _ in _lib.MlpStorage._fields_])
            return lib.mlpgan_bind(h, C.byref(st))

        refused(bind(without=("g_params",)), E_INVALID, "mlpgan_bind", "bind without g_params")
        refused(bind(without=("g_bn_running_var",)), E_INVALID, "mlpgan_bind", "bind without running_var")
        assert bind() == OK
        for batch in (0, bm + 1):
            for name, call in (("g_forward", g_forward), ("d_forward", d_forward), ("d_step", d_step), ("g_step", g_step)):
                refused(call(batch=batch), E_INVALID, f"batch {batch} outside", f"{name} batch {batch}")
        refused(g_forward(z_=None), E_INVALID, "null", "g_forward null z")
        refused(g_forward(img_=None), E_INVALID, "null", "g_forward null img")
        refused(d_forward(x_=None), E_INVALID, "null", "d_forward null x")
        refused(d_forward(probs_=None), E_INVALID, "null", "d_forward null probs")
        refused(d_step(real=None), E_INVALID, "null", "d_step null real")
        refused(d_step(hp_=None), E_INVALID, "null", "d_step null hp")
        refused(g_step(hp_=None), E_INVALID, "null", "g_step null hp")
        refused(g_step(batch=1), E_INVALID, "BatchNorm", "g_step batch 1")
        refused(g_forward(batch=1, training=1), E_INVALID, "BatchNorm", "training g_forward batch 1")

        for which, call in (("d", d_step), ("g", g_step)):
            for a in ("grads", "exp_avg", "exp_avg_sq", "adam_steps"):
                assert bind(without=(f"{which}_{a}",)) == OK
                refused(call(), E_STATE, "arenas were not bound", f"{which}_step without {which}_{a}")
        # (the forwards need none of them, and a bind without the other network's arenas does not stop a step)
        assert bind(without=("g_grads", "g_exp_avg", "g_exp_avg_sq", "g_adam_steps")) == OK
        assert g_forward() == OK and d_forward() == OK and d_step() == OK
        torch.cuda.synchronize()
        assert not torch.equal(img, saved["img"]) and not torch.equal(probs, saved["probs"]) and not torch.equal(arenas["d_params"], saved["d_params"])
        assert float(arenas["d_adam_steps"][0]) == 4.0
        for k in ("g_params", "g_grads", "g_exp_avg", "g_exp_avg_sq", "g_adam_steps", "g_bn_running_mean", "g_bn_running_var", "g_bn_batches"):
            assert torch.equal(arenas[k], saved[k]), k
    finally:
        assert lib.mlpgan_destroy(h) == OK
