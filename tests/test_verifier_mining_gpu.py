"""Hard-pair mining on the MI355X (signature_gan_amd/verifier_mining.py): mine_hard_pairs against a numpy restatement on
embed_u8 + score_matrix, before and after a train step; MiningPairLoader against DevicePairLoader (no mined pairs) and against
the kernel's numpy emulation on the planned draws (with mined pairs); the trainer's --hard_mining end to end."""
import random

import numpy as np
import pytest
import torch
from PIL import Image

import verifierdatacommon as DC

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import signature_verifier_train as ST
from signature_gan_amd import verifier_data as VD
from signature_gan_amd import verifier_mining as VM

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
E = 40


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    base = tmp_path_factory.mktemp("verifier_mining")
    DC.write_users(base / "real")
    (base / "syn").mkdir()
    rng = np.random.default_rng(9)
    for k in range(4):
        a = np.where(rng.uniform(size=(64, 64)) < 0.1, rng.integers(0, 128, (64, 64)), 255).astype(np.uint8)
        Image.fromarray(a).save(str(base / "syn" / f"gen{k}.png"))
    return base / "real", base / "syn"


def dataset(dirs, capsys, seed=3):
    random.seed(seed)
    ds = ST.SignaturePairDataset(str(dirs[0]), str(dirs[1]), pairs_per_user=2)
    capsys.readouterr()
    assert len(ds) == 12 and list(ds.user_signatures)[-1] == "_synthetic_"
    return ds


def new_model(seed=2, max_images=4):
    torch.manual_seed(seed)
    return ST.SiameseNetwork(embedding_dim=E, max_images=max_images, max_pairs=5).to(DEV)


def restated(model, cache, ids, synthetic, k_imp, k_gen, exclude):
    """mine_hard_pairs from the score matrix, written out plainly; also returns the matrix."""
    was = model.training
    model.eval()
    emb = model.embed_u8(cache)
    s = model.score_matrix(emb, emb).cpu().numpy()
    model.train(was)
    bits = s.view(np.int32).astype(np.int64)
    n = len(ids)
    seen = {frozenset(e) for e in exclude}
    out = []
    for i in range(n):
        if synthetic[i]:
            continue
        others = np.array([j for j in range(n) if j != i])
        imp = others[ids[others] != ids[i]]
        gen = others[ids[others] == ids[i]]
        imp = imp[np.lexsort((imp, -bits[i, imp]))][:k_imp]           # highest score first, then the lower row
        gen = gen[np.lexsort((gen, bits[i, gen]))][:k_gen]            # lowest score first, then the lower row
        for j, label in [(j, 0) for j in imp] + [(j, 1) for j in gen]:
            if frozenset((i, int(j))) not in seen:
                seen.add(frozenset((i, int(j))))
                out.append((i, int(j), label))
    return np.asarray(out, np.int64).reshape(-1, 3), s


def test_mine_hard_pairs_is_the_numpy_restatement(dirs, capsys):
    ds = dataset(dirs, capsys)
    loader = VM.MiningPairLoader(ds, 5, shuffle=True, augment=True, k_impostor=3, k_genuine=2, device=DEV)
    files, ids, synthetic = VM.signature_table(ds)
    assert loader.cache.shape == (13, 64, 64) and loader.files == files and synthetic.sum() == 4
    assert torch.equal(loader.ids.cpu(), torch.from_numpy(ids)) and np.array_equal(loader.anchor_ok, ~synthetic)
    model = new_model()                                               # 13 images through a context of 4: four embed calls
    model.train()
    exclude = [(0, 9), (4, 1), (5, 3)]
    got = VM.mine_hard_pairs(model, loader.cache, loader.ids, loader.anchor_ok, 3, 2, exclude)
    assert model.training                                             # the mode is restored
    want, _ = restated(model, loader.cache, ids, synthetic, 3, 2, exclude)
    assert got.dtype == np.int64 and np.array_equal(got, want), f"{got}\n{want}"
    assert not synthetic[got[:, 0]].any()                             # no synthetic anchor
    syn_neg = synthetic[got[:, 1]]
    assert syn_neg.any() and (got[syn_neg, 2] == 0).all()             # synthetic rows are there, as impostors only
    pairs = {frozenset(p) for p in got[:, :2].tolist()}
    assert len(pairs) == len(got) and not pairs & {frozenset(e) for e in exclude}
    assert (ids[got[:, 0]] == ids[got[:, 1]]).tolist() == (got[:, 2] == 1).tolist()
    # one class alone, and the loader's own route
    only = VM.mine_hard_pairs(model, loader.cache, loader.ids, loader.anchor_ok, 2, 0)
    assert np.array_equal(only, restated(model, loader.cache, ids, synthetic, 2, 0, [])[0]) and (only[:, 2] == 0).all()
    assert loader.remine(model) == (len(loader.mined), int((loader.mined[:, 2] == 0).sum()), int((loader.mined[:, 2] == 1).sum()))
    assert np.array_equal(loader.mined, restated(model, loader.cache, ids, synthetic, 3, 2, [])[0])
    with pytest.raises(ValueError):
        VM.mine_hard_pairs(model, loader.cache, loader.ids, loader.anchor_ok, 0, 0)


def test_mining_sees_the_stepped_weights(dirs, capsys):
    ds = dataset(dirs, capsys)
    loader = VM.MiningPairLoader(ds, 5, shuffle=False, augment=False, k_impostor=2, device=DEV)
    _, ids, synthetic = VM.signature_table(ds)
    model = new_model(max_images=16)
    model.seed_dropout(7)
    model.eval()
    emb = model.embed_u8(loader.cache)
    before = model.pair_topk(emb, loader.ids, emb, loader.ids, 2, same_set=True)
    model.train()
    x1, x2, labels = next(iter(loader))
    model.train_step(x1, x2, labels, ST.Adam(model, lr=1e-2))
    mined = VM.mine_hard_pairs(model, loader.cache, loader.ids, loader.anchor_ok, 2, 2)
    want, s = restated(model, loader.cache, ids, synthetic, 2, 2, [])
    assert np.array_equal(mined, want)
    model.eval()
    emb = model.embed_u8(loader.cache)
    after = model.pair_topk(emb, loader.ids, emb, loader.ids, 2, same_set=True)
    for c in ("impostor", "genuine"):
        sc, ix = after[f"{c}_score"].cpu().numpy(), after[f"{c}_index"].cpu().numpy()
        ok = ix >= 0
        rows = np.broadcast_to(np.arange(13)[:, None], ix.shape)
        assert np.array_equal(sc[ok].view(np.int32), s[rows[ok], ix[ok]].view(np.int32))          # a fresh score_matrix's bits
        assert (sc[~ok] == -1.0).all()
    assert not torch.equal(after["impostor_score"], before["impostor_score"])                     # and not the old weights'


def loaders(ds, **kw):
    return (VD.DevicePairLoader(ds, 5, shuffle=True, augment=True, device=DEV),
            VM.MiningPairLoader(ds, 5, shuffle=True, augment=True, k_impostor=2, device=DEV, **kw))


def test_loader_without_mined_pairs_is_the_device_loader(dirs, capsys):
    ds = dataset(dirs, capsys)
    plain, mining = loaders(ds)
    assert len(mining) == len(plain) == 3 and mining.cache.shape[0] == 13 and plain.cache.shape[0] <= 13
    torch.manual_seed(11)
    want = [list(plain), list(plain)]
    want_next = torch.rand(1)
    torch.manual_seed(11)
    got = [list(mining), list(mining)]
    assert torch.equal(torch.rand(1), want_next)                      # the same consumption of torch's generator
    for w_pass, g_pass in zip(want, got):
        assert len(w_pass) == len(g_pass) == 3
        for (w1, w2, wl), (g1, g2, gl) in zip(w_pass, g_pass):
            assert torch.equal(g1, w1) and torch.equal(g2, w2) and torch.equal(gl, wl)
    assert not torch.equal(want[0][0][0], want[1][0][0])


def test_batches_with_mined_pairs_are_the_emulation(dirs, capsys):
    ds = dataset(dirs, capsys)
    train, val = torch.utils.data.Subset(ds, list(range(9))), torch.utils.data.Subset(ds, [9, 10, 11])
    mining = VM.MiningPairLoader(train, 5, shuffle=True, augment=True, k_impostor=2, k_genuine=1, exclude_dataset=val, device=DEV)
    row = {p: r for r, p in enumerate(mining.files)}
    assert mining.exclude == [(row[p1], row[p2]) for p1, p2, _ in ds.pairs[9:]]
    model = new_model()
    count, n_imp, n_gen = mining.remine(model)
    assert count == n_imp + n_gen == len(mining.mined) and n_imp > 0 and n_gen > 0
    assert not {frozenset(p) for p in mining.mined[:, :2].tolist()} & {frozenset(p) for p in mining.exclude}
    slots, labels = mining._epoch_pairs()
    n = 9 + count
    assert slots.shape == (n, 2) and len(mining) == (n + 4) // 5
    assert np.array_equal(slots[:9], [[row[p1], row[p2]] for p1, p2, _ in ds.pairs[:9]]) and np.array_equal(slots[9:], mining.mined[:, :2])
    assert labels[9:].tolist() == mining.mined[:, 2].tolist()
    torch.manual_seed(17)
    batches, draws = VD.plan_pair_epoch(n, 5, True, False, True)
    torch.manual_seed(17)
    got = list(mining)
    cache = mining.cache.cpu().numpy()
    assert [len(b) for b in batches] == [g[2].numel() for g in got]
    t, moved, from_mined = 0, 0, 0
    for b, (x1, x2, y) in zip(batches, got):
        assert y.cpu().tolist() == labels[b].tolist()
        for pos, p in enumerate(b):
            for half, x in enumerate((x1, x2)):
                prm, tab = VD.build_pair_params(*(draws[k][t, half] for k in ("angle", "tx", "ty", "scale", "flip")))
                want = DC.emulate(cache[slots[p, half]], prm[0], tab[0])
                assert np.array_equal(x[pos].cpu().numpy(), want), (p, half)
                moved += int((want != cache[slots[p, half]]).any())
            from_mined += p >= 9
            t += 1
    assert t == n and from_mined == count and moved > 0


def test_cli_with_hard_mining(dirs, tmp_path, capsys):
    random.seed(4)
    torch.manual_seed(4)
    capsys.readouterr()
    saved = ST.main(["--data_dir", str(dirs[0]), "--epochs", "2", "--model_output", str(tmp_path / "models"), "--batch_size", "16",
                     "--embedding_dim", str(E), "--input_pipeline", "device", "--hard_mining", "2"])
    text = capsys.readouterr().out
    assert text.count("  -> Mined ") == 1
    line = [ln for ln in text.splitlines() if ln.startswith("  -> Mined ")][0]
    h, i, g = (int(w) for w in line.replace("(", "").split() if w.isdigit())
    # (nine files have 9 genuine and 27 impostor pairs in all, and the validation split's 24 draws are excluded: few are left)
    assert h == i + g and h > 0 and line == f"  -> Mined {h} hard pairs ({i} impostor, {g} genuine)"
    assert text.index("Epoch [1/2]") < text.index("  -> Mined ") < text.index("Epoch [2/2]")       # from epoch 2 on
    assert list(saved) == ["baseline"]
    ck = torch.load(saved["baseline"], map_location="cpu", weights_only=False)
    assert list(ck) == ["model_state_dict", "embedding_dim", "val_accuracy", "epoch"]
    assert list(ck["model_state_dict"]) == list(ST.SiameseNetwork(E).state_dict())
    # mining from the first epoch, every second epoch, impostors only
    ST.main(["--data_dir", str(dirs[0]), "--epochs", "3", "--model_output", str(tmp_path / "models2"), "--batch_size", "16",
             "--embedding_dim", str(E), "--input_pipeline", "device", "--hard_mining", "1", "--hard_mining_genuine", "0",
             "--hard_mining_start", "1", "--hard_mining_every", "2"])
    text = capsys.readouterr().out
    lines = text.splitlines()
    mined = [n for n, ln in enumerate(lines) if ln.startswith("  -> Mined ")]
    epochs = [n for n, ln in enumerate(lines) if ln.startswith("Epoch [")]
    assert len(mined) == 2 and len(epochs) == 3 and mined[0] < epochs[0] and epochs[1] < mined[1] < epochs[2]
    assert all(lines[n].endswith(", 0 genuine)") for n in mined)
