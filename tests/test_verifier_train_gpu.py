"""Verifier train step on the MI355X (include/siggan_verifier_train.h) against the reference's fixtures and the torch
restatement (verifiertraincommon).

The backward pass jumps at every ReLU and max decision, so the check is a chain: (1) the HIP path's decisions may differ from
the fixture's fp64 decisions in at most MAX_FLIPS positions per case, each of them on the fixture's near-tie list (the
reference's own fp32 differs in none); (2) the restatement in fp64, given HIP's decisions, is compared with HIP's losses,
embeddings, gradients, running tensors and, after the update, parameters and moments; (3) where no decision differs the
same comparison is made against the fixture directly.  Bound: verifiercommon's rule (32 x the reference's own fp32-vs-fp64
deviation per tensor relative to its max-abs, never looser than 1e-4).  Conv-bias gradients are exactly 0."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch
from PIL import Image

import verifiertraincommon as TC
from verifiertraincommon import TI, VC

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd import signature_verifier_eval as SV
from signature_gan_amd import signature_verifier_train as ST

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MAX_FLIPS = 4
VARIANTS = [(n, e, steps, prefix, use_c) for n, e, steps, _ in TI.CASES
            for prefix, use_c in ([("", True)] + ([("nc_", False)] if (n, e) == TI.NO_CONTRASTIVE else []))]
MARGINS = None                                         # profiles/verifier_train_parity.py collects the observed margins here
ROUTES = {"route1": (32, 32, 32), "route2": (64, 16, 16), "route3": (128, 8, 8)}


class Rig:
    """The C ABI with caller-owned arenas, loaded with verifier_inputs' state."""

    def __init__(self, e, max_pairs):
        self.e = e
        self.t = ST._Trainer(DEV, e, max_pairs)
        P, R = TC.state(e, torch.float32)
        self.names = list(P)
        self.arenas = [torch.zeros(self.t.count, dtype=torch.float32, device=DEV) for _ in range(4)]
        for (off, n), k in zip(self.t.spans, self.names):
            assert P[k].numel() == n
            self.arenas[0][off:off + n].copy_(P[k].reshape(-1))
        self.shapes = {k: P[k].shape for k in P}
        self.running = [R[k].to(DEV).contiguous() for k in TI.running_names()]
        self.t.bind(self.arenas, self.running, VC.BN_EPS, 0)

    def views(self, which):
        a = self.arenas[("params", "grads", "exp_avg", "exp_avg_sq").index(which)].cpu()
        return {k: a[off:off + n].view(self.shapes[k]) for (off, n), k in zip(self.t.spans, self.names)}

    def running_cpu(self):
        return {k: t.cpu() for k, t in zip(TI.running_names(), self.running)}

    def grads(self, x1, x2, labels, fc_keep, cls_keep, use_c, fmt=_lib.VFMT_F32):
        self.hold = [t.to(DEV).contiguous() if t is not None else None for t in (x1, x2, labels, fc_keep, cls_keep)]
        x1, x2, labels, fk, ck = self.hold
        self.n = labels.numel()
        m = torch.zeros(4, dtype=torch.float32, device=DEV)
        p = SV._ptr
        _lib.check(self.t.lib.siggan_verifier_train_grads(self.t._h, p(x1), p(x2), fmt, p(labels), self.n, p(fk), p(ck),
                                                          1 if use_c else 0, p(m), self.t.stream()))
        return m

    def apply(self):
        _lib.check(self.t.lib.siggan_verifier_train_apply(self.t._h, TI.LR, TI.BETAS[0], TI.BETAS[1], TI.EPS, self.t.stream()))

    def decisions(self):
        n = self.n
        out = {k: self.t.debug(k, (2 * n,) + s).cpu() for k, s in ROUTES.items()}
        out["fc1_mask"] = self.t.debug("fc1_mask", (2 * n, 512)).cpu()
        out["cls_mask"] = self.t.debug("cls_mask", (n, 64)).cpu()
        return out

    def outputs(self):
        n = self.n
        f32 = lambda k, s: self.t.debug(k, s, torch.float32).cpu()
        return dict(e1=f32("e1", (n, self.e)), e2=f32("e2", (n, self.e)), similarity=f32("similarity", (n,)), distance=f32("distance", (n,)))


def batch32(n_pairs, step=0):
    return TC.case_batch(n_pairs, torch.float32, step)


def run_grads(rig, b, use_c):
    return rig.grads(b["x1"], b["x2"], b["labels"], b["fc_keep"], b["cls_keep"], use_c)


def flips(dec, want, ties, what):
    """Positions where the HIP decisions differ from `want`; every one must be a listed near tie."""
    total = 0
    for name in TI.DECISIONS:
        d = np.nonzero(dec[name].numpy().reshape(-1) != np.asarray(want[name]).reshape(-1))[0]
        print(f"{what} {name}: {d.size} decisions differ ({np.asarray(ties[name]).size} near ties listed)")
        stray = np.setdiff1d(d, np.asarray(ties[name]))
        assert stray.size == 0, f"{what} {name}: decisions differ away from any near tie, first at flat position {stray[:8]}"
        total += d.size
    assert total <= MAX_FLIPS, f"{what}: {total} decisions differ, more than {MAX_FLIPS}"
    return total


def compare(rig, metrics, ref, f, k, what, pick=False):
    """HIP against ref (the restatement's output dict, or the fixture itself when pick) with fixture f's bounds under key
    prefix k."""
    sel = (lambda a, name: TI.pick(np.asarray(a), name)) if pick else (lambda a, name: np.asarray(a))
    got = dict(zip(TC.METRICS, metrics.cpu().tolist()))
    got.update(rig.outputs())
    for name in TC.METRICS + ("e1", "e2", "similarity", "distance"):
        TC.check(got[name], ref[name], f, f"{k}{name}", what, MARGINS)
    g = rig.views("grads")
    for name in rig.names:
        if name in TC.CONV_BIAS:
            assert float(g[name].abs().max()) == 0.0, f"{name}: the conv-bias gradient must be exactly 0"
            continue
        TC.check(sel(g[name], name), ref["grads"][name], f, f"{k}grad:{name}", what, MARGINS)
    r = rig.running_cpu()
    for name in TI.running_names():
        TC.check(r[name], ref["running"][name], f, f"{k}{name}", what, MARGINS)


def compare_state(rig, ref, f, k, what, bias0, pick=False):
    """Parameters and moments after the update.  Gradients and moments are compared over the whole tensor.  The updated
    parameters of a large tensor are compared at the positions the fixture stores: Adam's first steps move an element by
    lr * g / (|g| + eps), which for the few of 4 M elements whose gradient is of the size of fp32 rounding (|g| near eps = 1e-8)
    is not continuous in g at any fp32 accuracy, and the bound -- the reference's own fp32-vs-fp64 deviation -- is only known
    where the fixture stores both."""
    sel = (lambda a, name: TI.pick(np.asarray(a), name)) if pick else (lambda a, name: np.asarray(a))
    for which in ("params", "exp_avg", "exp_avg_sq"):
        got = rig.views(which)
        key = "param" if which == "params" else which
        for name in rig.names:
            if name in TC.CONV_BIAS:                      # never moved: bit-unchanged bias, zero moments
                want = bias0[name] if which == "params" else torch.zeros_like(bias0[name])
                assert torch.equal(got[name], want), f"{which} {name} moved"
                continue
            g_, w_ = sel(got[name], name), ref[which][name]
            if which == "params" and not pick:            # at the positions the fixture's bound was measured on (see docstring)
                g_, w_ = TI.pick(g_, name), TI.pick(np.asarray(w_), name)
            TC.check(g_, w_, f, f"{k}{key}:{name}", what, MARGINS)


def fixture_ref(f, k, names):
    ref = {name: f[f"{k}{name}_f64"] for name in TC.METRICS + ("e1", "e2", "similarity", "distance")}
    ref["grads"] = {n: f[f"{k}grad:{n}_f64"] for n in names}
    ref["running"] = {n: f[f"{k}{n}_f64"] for n in TI.running_names()}
    for which, key in (("params", "param"), ("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq")):
        ref[which] = {n: f[f"{k}{key}:{n}_f64"] for n in names}
    return ref


@pytest.mark.parametrize("n_pairs,e,steps,prefix,use_c", VARIANTS)
def test_fixture_case(n_pairs, e, steps, prefix, use_c):
    f = TC.load_case(n_pairs, e)
    rig = Rig(e, n_pairs)
    P, R = TC.state(e)
    bias0 = {k: P[k].float().clone() for k in TC.CONV_BIAS}
    m, v = TC.zero_moments(P)
    clean = True
    for step in range(steps):
        k, what = f"{prefix}s{step}_", f"hip pairs={n_pairs} E={e} {prefix}step {step}"
        metrics = run_grads(rig, batch32(n_pairs, step), use_c)
        dec = rig.decisions()
        want = {name: f[f"s{step}_{name}"] for name in TI.DECISIONS}
        ties = {name: f[f"s{step}_tie:{name}"] for name in TI.DECISIONS}
        clean = flips(dec, want, ties, what) == 0 and clean
        out = TC.train_grads(P, R, TC.case_batch(n_pairs, step=step), use_c, decisions=dec)
        out["running"] = R
        compare(rig, metrics, out, f, k, what + " vs restatement")
        rig.apply()
        with torch.no_grad():
            TC.adam_apply(P, out["grads"], m, v, step + 1)
        compare_state(rig, dict(params=P, exp_avg=m, exp_avg_sq=v), f, k, what + " vs restatement", bias0)
        if clean:                                          # same decisions as the reference: the fixture itself is the yardstick
            ref = fixture_ref(f, k, rig.names)
            compare(rig, metrics, ref, f, k, what + " vs fixture", pick=True)
            compare_state(rig, ref, f, k, what + " vs fixture", bias0, pick=True)
    rig.t.close()


def test_u8_input_and_repeat_are_bitwise():
    n = 3
    b = batch32(n)
    _, _, bytes2 = VC.case_inputs(n)
    runs = []
    for x1, fmt in ((b["x2"], _lib.VFMT_F32), (b["x2"], _lib.VFMT_F32), (bytes2, _lib.VFMT_U8)):
        rig = Rig(40, n)
        m = rig.grads(x1, x1.flip(0), b["labels"], b["fc_keep"], b["cls_keep"], True, fmt)
        rig.apply()
        runs.append((m.cpu(), rig.arenas[1].cpu(), rig.arenas[0].cpu(), [t.cpu() for t in rig.running], rig.decisions()["route1"]))
        rig.t.close()
    for other, what in ((runs[1], "a repeated call"), (runs[2], "uint8 input")):
        assert torch.equal(runs[0][0], other[0]), f"{what}: metrics differ"
        assert torch.equal(runs[0][1], other[1]), f"{what}: gradients differ"
        assert torch.equal(runs[0][2], other[2]), f"{what}: updated parameters differ"
        assert all(torch.equal(a, b_) for a, b_ in zip(runs[0][3], other[3])), f"{what}: running tensors differ"
        assert torch.equal(runs[0][4], other[4])
    assert float(runs[0][1].abs().max()) > 0


@functools.lru_cache(maxsize=None)
def big_reference():
    """The 33-pair case has no fixture: the restatement on the CPU (pinned by the CPU tests) decides and is the yardstick."""
    n, e = TI.BIG
    P, R = TC.state(e)
    margins = {}
    out = TC.train_grads(P, R, TC.case_batch(n), True, margins=margins)
    out["running"] = R
    ties = {k: np.nonzero(margins[k].reshape(-1).numpy() < TI.NEAR_TIE)[0] for k in TI.DECISIONS}
    return out, ties


def test_big_batch_against_the_restatement():
    n, e = TI.BIG                                          # 66 images: more than one fc1 tile, 528 conv2 tiles
    ref, ties = big_reference()
    rig = Rig(e, n)
    metrics = run_grads(rig, batch32(n), True)
    dec = rig.decisions()
    what = f"hip pairs={n} E={e}"
    if flips(dec, ref["decisions"], ties, what):
        P, R = TC.state(e)
        ref = TC.train_grads(P, R, TC.case_batch(n), True, decisions=dec)
        ref["running"] = R
    P32, R32 = TC.state(e, torch.float32)
    r32 = TC.train_grads(P32, R32, batch32(n), True, decisions=dec)
    r32["running"] = R32
    got = dict(zip(TC.METRICS, metrics.cpu().tolist()))
    got.update(rig.outputs())
    g = rig.views("grads")
    got.update({f"grad:{k}": g[k] for k in rig.names})
    got.update(rig.running_cpu())

    def pairs():
        for name in TC.METRICS + ("e1", "e2", "similarity", "distance"):
            yield name, ref[name], r32[name]
        for name in rig.names:
            if name not in TC.CONV_BIAS:
                yield f"grad:{name}", ref["grads"][name], r32["grads"][name]
        for name in TI.running_names():
            yield name, ref["running"][name], r32["running"][name]

    for name, r64, rf32 in pairs():
        r64 = np.asarray(r64, np.float64).reshape(-1)
        scale = float(np.abs(r64).max())
        bound = min(TC.MARGIN * float(np.abs(np.asarray(rf32, np.float64).reshape(-1) - r64).max()) / scale, TC.CAP)
        d = float(np.abs(np.asarray(got[name], np.float64).reshape(-1) - r64).max()) / scale
        print(f"{what} {name}: relative deviation {d:.3e} bound {bound:.3e}")
        assert d <= bound, f"{what} {name}: relative deviation {d:.3e} exceeds bound {bound:.3e}"
    for name in TC.CONV_BIAS:
        assert float(g[name].abs().max()) == 0.0
    rig.t.close()


def test_drawn_masks():
    n, steps = 8, 3
    b = batch32(n)

    def run(seed):
        rig = Rig(128, n)
        rig.t.seed(seed, 5)
        out = []
        for _ in range(steps):
            m = rig.grads(b["x1"], b["x2"], b["labels"], None, None, True)
            out.append((rig.t.debug("fc_keep", (2 * n, 512)).cpu(), rig.t.debug("cls_keep", (n, 64)).cpu(), m.cpu()))
        rig.t.close()
        return out

    a, again, other = run(1234), run(1234), run(1235)
    for (f1, c1, m1), (f2, c2, m2) in zip(a, again):
        assert torch.equal(f1, f2) and torch.equal(c1, c2) and torch.equal(m1, m2), "re-seeding does not reproduce the run"
    assert not torch.equal(a[0][0], other[0][0])
    fc = torch.stack([s[0] for s in a]).float()            # (steps, 2n, 512)
    cl = torch.stack([s[1] for s in a]).float()
    assert set(fc.unique().tolist()) <= {0.0, 1.0}
    for half, name in ((fc[:, :n], "fc x1"), (fc[:, n:], "fc x2")):
        cnt = half.numel()
        assert abs(float(half.mean()) - 0.5) <= 5 * (0.25 / cnt) ** 0.5, name
    assert abs(float(cl.mean()) - 0.7) <= 5 * (0.21 / cl.numel()) ** 0.5
    assert not torch.equal(fc[0, :n], fc[0, n:]), "x1 and x2 share one dropout mask"
    assert not torch.equal(fc[0], fc[1]) and not torch.equal(cl[0], cl[1]), "the RNG does not advance between steps"


def write_users(root, users=3, sigs=3, seed=5):
    rng = np.random.default_rng(seed)
    for u in range(users):
        (root / f"user{u}").mkdir(parents=True)
        for k in range(sigs):
            a = np.where(rng.uniform(size=(48, 96)) < 0.1, rng.integers(0, 128, (48, 96)), 255).astype(np.uint8)
            Image.fromarray(a).save(str(root / f"user{u}" / f"sig{k}.png"))


def test_dropin_trains_and_its_checkpoint_loads(tmp_path, capsys):
    data = tmp_path / "real"
    write_users(data)
    random.seed(3)
    torch.manual_seed(3)
    ds = ST.SignaturePairDataset(str(data), pairs_per_user=4)
    loader = torch.utils.data.DataLoader(ds, batch_size=8, shuffle=False, num_workers=0)
    model = ST.SiameseNetwork(embedding_dim=40, max_pairs=8).to(DEV)
    model.seed_dropout(7)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = ST.Adam(model, lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=10, gamma=0.5)
    tm = ST.train_epoch(model, loader, opt, torch.nn.BCELoss(), ST.ContrastiveLoss(2.0), DEV)
    sched.step()
    assert set(tm) == {"loss", "bce_loss", "contrastive_loss", "accuracy"}
    assert np.isfinite(list(tm.values())).all() and 0.0 <= tm["accuracy"] <= 1.0 and tm["loss"] > tm["bce_loss"] > 0
    after = model.state_dict()
    assert int(after["encoder.bn1.num_batches_tracked"]) == 2 * len(loader)
    assert not torch.equal(after["encoder.fc1.weight"], before["encoder.fc1.weight"])
    assert torch.equal(after["encoder.conv2.bias"], before["encoder.conv2.bias"])
    assert not torch.equal(after["encoder.bn2.running_mean"], before["encoder.bn2.running_mean"])
    ev = ST.evaluate(model, loader, torch.nn.BCELoss(), DEV)
    assert set(ev) == {"loss", "accuracy"} and np.isfinite(ev["loss"]) and 0.0 <= ev["accuracy"] <= 1.0
    # the optimiser's state loads into a plain torch.optim.Adam
    plain = torch.optim.Adam([torch.nn.Parameter(torch.zeros_like(p)) for p in model.parameters()], lr=1.0)
    plain.load_state_dict(opt.state_dict())
    assert plain.param_groups[0]["lr"] == 1e-3 and float(plain.state[plain.param_groups[0]["params"][0]]["step"]) == len(loader)
    # the live model's checkpoint, loaded by the eval module, scores bit for bit as the live model
    path = str(tmp_path / "live.pth")
    torch.save(ST.checkpoint_dict(model, 40, ev["accuracy"], 1), path)
    loaded, meta = SV.load_model(path, DEV)
    assert meta["embedding_dim"] == 40 and meta["epoch"] == 1
    x1 = torch.stack([ds[i][0] for i in range(6)]).to(DEV)
    x2 = torch.stack([ds[i][1] for i in range(6)]).to(DEV)
    live = model.eval()(x1, x2)
    for a, b in zip(live, loaded(x1, x2)):
        assert torch.equal(a, b)
    with pytest.raises(RuntimeError, match="eval"):
        model.train()(x1, x2)
    # train_model: the reference's files and dictionary
    capsys.readouterr()
    random.seed(4)
    torch.manual_seed(4)
    syn = tmp_path / "syn"
    syn.mkdir()
    for k in range(2):
        Image.fromarray(np.full((64, 64), 255 - 40 * k, np.uint8)).save(str(syn / f"gen{k}.png"))
    saved = ST.train_model(str(data), str(syn), 1, str(tmp_path / "models"), batch_size=16, embedding_dim=40, device="cuda")
    text = capsys.readouterr().out
    assert "Training BASELINE model (real signatures only)" in text and "Training AUGMENTED model (real + synthetic signatures)" in text
    assert "Epoch [1/1] Train Loss:" in text
    assert list(saved) == ["baseline", "augmented"]
    for name, extra in (("baseline", []), ("augmented", ["includes_synthetic"])):
        assert saved[name].endswith(f"{name}_siamese_model.pth")
        ck = torch.load(saved[name], map_location="cpu", weights_only=False)
        assert list(ck) == ["model_state_dict", "embedding_dim", "val_accuracy", "epoch"] + extra
        m2, meta = SV.load_model(saved[name], DEV)
        s = m2(x1, x2)[2]
        assert s.shape == (6, 1) and bool(torch.isfinite(s).all())


def test_argument_errors():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.siggan_verifier_trainer_create(0, 0, 4, C.byref(h)) == _lib.E_ARG and not h.value
    assert lib.siggan_verifier_trainer_create(0, 128, 0, C.byref(h)) == _lib.E_ARG and not h.value
    t = ST._Trainer(DEV, 128, 2)
    x = torch.zeros(4, 1, 64, 64, device=DEV)
    y = torch.zeros(4, device=DEV)
    p, st = SV._ptr, t.stream()
    assert lib.siggan_verifier_train_grads(t._h, p(x), p(x), 0, p(y), 2, None, None, 1, None, st) == _lib.E_ARG
    assert "bind" in lib.siggan_last_error().decode()
    rig = Rig(128, 2)
    g0 = rig.arenas[1].clone()
    for args, text in (((p(x), p(x), 0, p(y), 3), "n_pairs"), ((p(x), p(x), 0, p(y), 0), "n_pairs"), ((p(x), p(x), 5, p(y), 2), "fmt"),
                       ((None, p(x), 0, p(y), 2), "null"), ((p(x), p(x), 0, None, 2), "null")):
        assert lib.siggan_verifier_train_grads(rig.t._h, *args, None, None, 1, None, rig.t.stream()) == _lib.E_ARG
        assert text in lib.siggan_last_error().decode()
    assert lib.siggan_verifier_train_debug(rig.t._h, b"route1", p(x), 4, rig.t.stream()) == _lib.E_ARG      # no _grads call yet
    assert lib.siggan_verifier_train_apply(rig.t._h, -1.0, 0.9, 0.999, 1e-8, rig.t.stream()) == _lib.E_ARG
    torch.cuda.synchronize()
    assert torch.equal(rig.arenas[1], g0)
    with pytest.raises(ValueError):
        _lib.check(lib.siggan_verifier_train_debug(rig.t._h, b"nothing", p(x), 4, rig.t.stream()))
    t.close()
    rig.t.close()
