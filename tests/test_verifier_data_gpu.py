"""Verifier trainer's input pipeline on the MI355X: siggan_pairs_augment against Pillow, bit for bit; the device loader against
the host route (the reference's DataLoader over a Pillow transform with the literal torch draws); one epoch of training fed by
either route ends in the same bits; train_model(input_pipeline="device") writes the reference's checkpoints."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

import verifierdatacommon as DC

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd import signature_verifier_eval as SV
from signature_gan_amd import signature_verifier_train as ST
from signature_gan_amd import verifier_data as VD

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S = 64
PAD = 0xA5                                               # what the output buffer holds before a call


def augment(cache, index, prm, tab, n=None, size=S, fill=0, null_cache=False):
    """-> (return code, the (n + 2, 64, 64) buffer whose images 1..n were handed in as out_dev)."""
    lib = _lib.load()
    n = len(index) if n is None else n
    c = torch.from_numpy(cache).to(DEV)
    i = torch.from_numpy(np.asarray(index, np.int32)).to(DEV)
    p = torch.from_numpy(prm).to(DEV) if prm is not None else None
    t = torch.from_numpy(tab).to(DEV) if tab is not None else None
    big = torch.full((len(index) + 2, S, S), PAD, dtype=torch.uint8, device=DEV)
    out = big[1:]
    rc = lib.siggan_pairs_augment(0, None if null_cache else c.data_ptr(), c.shape[0], i.data_ptr(), SV._ptr(p), SV._ptr(t),
                                  out.data_ptr(), n, size, fill, None)
    torch.cuda.synchronize()
    return rc, big.cpu().numpy()


# (angle, tx, ty, scale, flip) per output image: both Pillow paths, the flip on either, content pushed off each of the four
# edges on either path; row 0 is turned into a mode-0 copy below
CASES = [(0.0, 0, 0, 1.0, True), (0.0, 6, 0, 1.0, False), (0.0, -6, 0, 0.9, True), (0.0, 0, 6, 1.1, False), (0.0, -6, -6, 1.0, False),
         (5.0, 6, -6, 0.9, False), (-5.0, -6, 6, 1.1, True), (3.3, -6, 6, 1.0, False), (-2.1, 0, -6, 1.05, True), (1e-9, 6, 0, 1.0, False)]
INDEX = [3, 0, 3, 6, -1, 7, 2, 5, 1, 3]                   # repeated, out of order, one below and one above the cache


def kernel_case():
    rng = np.random.default_rng(21)
    cache = rng.integers(0, 256, (7, S, S), dtype=np.uint8)
    prm, tab = VD.build_pair_params(*(np.array([c[k] for c in CASES]) for k in range(5)))
    prm[0, :7] = 0                                         # mode 0 + flip
    tab[0] = -1
    assert sorted(set(prm[:, 0])) == [0, 1, 2] and set(prm[:, 7]) == {0, 1}
    src = cache[np.clip(INDEX, 0, 6)]
    return cache, prm, tab, src


@pytest.mark.parametrize("fill", [0, 77])
def test_kernel_is_pillow(fill):
    cache, prm, tab, src = kernel_case()
    rc, big = augment(cache, INDEX, prm, tab, fill=fill)
    assert rc == 0
    n = len(INDEX)                                         # 10 images: 5 "pairs", odd per half
    emptied = set()                                        # (mode, edge) whose whole row / column of the output is fill
    for i, (a, tx, ty, s, f) in enumerate(CASES):
        want = np.ascontiguousarray(src[i][:, ::-1]) if i == 0 else DC.pil_affine(src[i], a, tx, ty, s, f, fill)
        assert np.array_equal(big[1 + i], want), (i, CASES[i])
        assert np.array_equal(big[1 + i], DC.emulate(src[i], prm[i], tab[i], fill))
        z = want == fill
        emptied |= {(int(prm[i, 0]), e) for e, hit in (("top", z[0].all()), ("bottom", z[-1].all()), ("left", z[:, 0].all()),
                                                       ("right", z[:, -1].all())) if hit}
    assert emptied == {(m, e) for m in (1, 2) for e in ("top", "bottom", "left", "right")}, "a path never pushes content off an edge"
    assert (big[0] == PAD).all() and (big[n + 1] == PAD).all(), "the kernel wrote outside its n images"


def test_plain_gather_and_missing_tables():
    cache, prm, tab, src = kernel_case()
    rc, big = augment(cache, INDEX, None, None)
    assert rc == 0 and np.array_equal(big[1:-1], src)
    assert (big[0] == PAD).all() and (big[-1] == PAD).all()
    rc, big = augment(cache, INDEX, None, tab)             # tables without parameters: still the plain gather
    assert rc == 0 and np.array_equal(big[1:-1], src)
    rc, big = augment(cache, INDEX, prm, None, fill=9)     # a mode-2 image without tables is all fill, the others are unchanged
    assert rc == 0
    for i in range(len(INDEX)):
        assert np.array_equal(big[1 + i], DC.emulate(src[i], prm[i], None, 9)), i
    rc, big = augment(cache, INDEX, prm, tab, n=4)         # a shorter batch stops after its n images
    assert rc == 0 and (big[5:] == PAD).all() and not (big[4] == PAD).all()


def test_argument_errors():
    cache, prm, tab, _ = kernel_case()
    lib = _lib.load()
    for kw, text in ((dict(size=128), "size"), (dict(n=0), "n must"), (dict(null_cache=True), "null"), (dict(fill=256), "fill")):
        rc, big = augment(cache, INDEX, prm, tab, **kw)
        assert rc == _lib.E_ARG and text in lib.siggan_last_error().decode()
        assert (big == PAD).all(), "a refused call launched"
    with pytest.raises(ValueError):
        _lib.check(rc)


# ------------------------------------------------------------------------------------------------------------------
# the loader against the host route
# ------------------------------------------------------------------------------------------------------------------
def reference_transform(img):
    """The reference's train chain on one PIL 'L' image with Pillow and torchvision's literal draws:
    Resize -> Grayscale -> RandomAffine(5, (0.1, 0.1), (0.9, 1.1)) -> RandomHorizontalFlip(0.1) -> ToTensor -> Normalize."""
    img = img.resize((S, S), Image.BILINEAR)
    angle = float(torch.empty(1).uniform_(-5.0, 5.0).item())
    tx = int(round(torch.empty(1).uniform_(-6.4, 6.4).item()))
    ty = int(round(torch.empty(1).uniform_(-6.4, 6.4).item()))
    scale = float(torch.empty(1).uniform_(0.9, 1.1).item())
    m = DC.A.tv_inverse_affine_matrix([S * 0.5, S * 0.5], angle, [tx, ty], scale, [0.0, 0.0])
    img = img.transform((S, S), Image.AFFINE, m, Image.NEAREST, fillcolor=0)
    if torch.rand(1) < 0.1:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return torch.from_numpy(SV.normalize_uint8(np.asarray(img, dtype=np.uint8))[None])


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("verifier_data") / "real"
    DC.write_users(root)
    return root


def datasets(tree, capsys):
    random.seed(3)
    host = ST.SignaturePairDataset(str(tree), transform=reference_transform, pairs_per_user=2)
    random.seed(3)
    plain = ST.SignaturePairDataset(str(tree), pairs_per_user=2)
    capsys.readouterr()
    assert len(host) == 12 and host.pairs == plain.pairs
    return host, plain


def host_loaders(host, plain):
    DL = torch.utils.data.DataLoader
    return DL(host, batch_size=5, shuffle=True, num_workers=0), DL(plain, batch_size=5, shuffle=False, num_workers=0)


def device_loaders(plain):
    return VD.DevicePairLoader(plain, 5, shuffle=True, augment=True, device=DEV), VD.DevicePairLoader(plain, 5, shuffle=False, augment=False)


def normalized(x):
    return ((x.cpu().float() / 255) - 0.5) / 0.5


def test_loader_is_the_host_route(tree, capsys):
    host, plain = datasets(tree, capsys)
    ht, hv = host_loaders(host, plain)
    dt, dv = device_loaders(plain)
    assert len(dt) == len(ht) == 3 and len(dv) == 3 and dt.batch_size == 5 and dt.dataset is plain
    assert dt.cache.shape == (9, S, S) and dt.cache.dtype == torch.uint8 and dt.cache.device == DEV
    torch.manual_seed(11)
    want = [list(ht), list(hv), list(ht)]
    want_next = torch.rand(1)
    torch.manual_seed(11)
    got = [list(dt), list(dv), list(dt)]
    assert torch.equal(torch.rand(1), want_next)
    moved = 0
    for w_pass, g_pass in zip(want, got):
        assert [b[2].numel() for b in g_pass] == [5, 5, 2] == [b[2].numel() for b in w_pass]
        for (w1, w2, wl), (g1, g2, gl) in zip(w_pass, g_pass):
            assert g1.dtype == g2.dtype == torch.uint8 and g1.device == g2.device == gl.device == DEV
            assert g1.shape == g2.shape == (wl.numel(), S, S) and gl.dtype == torch.float32
            assert torch.equal(gl.cpu(), wl)
            assert torch.equal(normalized(g1), w1[:, 0]) and torch.equal(normalized(g2), w2[:, 0])
            moved += int((g1 == 0).sum())
    assert moved > 0                                       # the affine's black corners are there
    assert not torch.equal(want[0][0][0], want[2][0][0])  # and the two epochs differ


def test_training_is_the_same_training(tree, capsys):
    host, plain = datasets(tree, capsys)
    ht, _ = host_loaders(host, plain)
    dt, _ = device_loaders(plain)
    torch.manual_seed(2)
    first = ST.SiameseNetwork(embedding_dim=40, max_pairs=5).to(DEV)
    start = {k: v.detach().clone() for k, v in first.state_dict().items()}
    states = []
    for loader in (ht, dt):
        model = ST.SiameseNetwork(embedding_dim=40, max_pairs=5).to(DEV)
        model.load_state_dict(start)
        model.seed_dropout(7)
        torch.manual_seed(13)
        metrics = ST.train_epoch(model, loader, ST.Adam(model, lr=1e-3), None, None, DEV)
        assert np.isfinite(list(metrics.values())).all()
        states.append(({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, metrics))
    (a, ma), (b, mb) = states
    assert ma == mb
    assert not torch.equal(a["encoder.fc1.weight"], start["encoder.fc1.weight"].cpu())
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: the uint8 route and the fp32 route train to different bits"


def test_train_model_on_the_device_pipeline(tree, tmp_path, capsys):
    syn = tmp_path / "syn"
    syn.mkdir()
    for k in range(2):
        Image.fromarray(np.full((64, 64), 255 - 40 * k, np.uint8)).save(str(syn / f"gen{k}.png"))
    random.seed(4)
    torch.manual_seed(4)
    capsys.readouterr()
    saved = ST.train_model(str(tree), str(syn), 1, str(tmp_path / "models"), batch_size=16, embedding_dim=40, device="cuda",
                           input_pipeline="device")
    text = capsys.readouterr().out
    assert "Epoch [1/1] Train Loss:" in text and "torchvision is not available" not in text
    assert "Training BASELINE model (real signatures only)" in text and "Training AUGMENTED model (real + synthetic signatures)" in text
    assert list(saved) == ["baseline", "augmented"]
    x = torch.from_numpy(np.stack([SV.normalize_uint8(SV.load_uint8(p)) for p in sorted(tree.glob("user0/*.png"))])).to(DEV)
    for name, extra in (("baseline", []), ("augmented", ["includes_synthetic"])):
        assert saved[name].endswith(f"{name}_siamese_model.pth")
        ck = torch.load(saved[name], map_location="cpu", weights_only=False)
        assert list(ck) == ["model_state_dict", "embedding_dim", "val_accuracy", "epoch"] + extra
        model, meta = SV.load_model(saved[name], DEV)
        assert meta["embedding_dim"] == 40
        s = model(x, x.flip(0))[2]
        assert s.shape == (3, 1) and bool(torch.isfinite(s).all())
