"""The device resize on the MI355X (include/siggan_resize.h, resize.py) and what is built on it.

resize_u8 is held to Pillow itself, byte for byte, on the smallest shapes that reach every branch: clamped windows at both
borders, odd sizes, upsampling (filterscale clamped to 1), a skipped pass, both passes skipped, n > 1 with images that
differ -- and, beyond 64x64 outputs, the shapes at which the kernel stages nothing in LDS because not even one output row's
halo fits (1024 rows into one), splits an image into bands (a 128-wide output off 1024 rows) and tiles columns.

resize_f32 and its adjoint are held to fp64 dense matrices of the restatement's DOUBLE weights.  The bound is derived: a pass
is a sum of at most ksize products with non-negative fp32 weights (each a rounding of the double weight, relative error u =
2^-24) that sum to 1 +- ksize u; with one rounding per product and per addition its error is at most (ksize + 2) u max|x|,
the second pass doubles that and sees the first one's error once more: 4 (ksize + 2) u max|x| per element, ksize the larger
of the two axes'.  The adjoint's sums run over at most as many terms with weights that sum to at most 1 at the downscaling
shapes used here, so the same bound holds with max|dy|.  profiles/resize_parity_margins.py writes the worst observed ratios.

Against the byte path: for bytes b, resize_f32(b / 127.5 - 1) is the exact affine image of the un-rounded resize of b (the
weights sum to 1), and resize_u8 differs from that by at most half a byte per pass plus the coefficient quantisation
(ksize 2^-23 of 255 per pass, far below 0.01 byte): 1.01 / 127.5.
"""
import glob
import json
import math

import numpy as np
import pytest
import torch

import identitycommon as IC
import resizecommon as RC
import verifiercommon as VC
from common import I, O, SEED
from latentcommon import P_BETAS, P_LATENT, P_LR, P_SIZE, projection_case

import signature_gan_amd  # noqa: F401
from signature_gan_amd import resize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

U8_SHAPES = [(5, 128, 128), (3, 96, 150), (2, 40, 50), (1, 65, 127), (2, 64, 128), (2, 128, 64), (2, 64, 64), (1, 1, 1)]
KINDS = ["random", "strokes", "zeros", "full"]
# (n, h, w) -> (h_out, w_out): nothing staged (one row's halo is 1024 x 64 bytes), bands (1024 x 128 bytes do not fit one
# workgroup), the largest output off an odd input, an upscale in both axes, one axis kept at a non-64 size
OTHER_SIZES = [((1, 1024, 80), (1, 64)), ((2, 1024, 300), (128, 128)), ((1, 301, 257), (128, 128)), ((2, 20, 30), (64, 48)),
               ((2, 64, 64), (64, 32)), ((1, 1024, 1024), (3, 5))]
F32_SHAPES = [(3, 128, 128), (2, 96, 150)]
# nothing staged forwards; bands forwards; an upscale in both axes; nothing staged in the ADJOINT (128 halo rows x 128 columns)
F32_OTHER = [((1, 1024, 80), (1, 64)), ((1, 700, 40), (128, 64)), ((2, 20, 30), (64, 48)), ((1, 1, 200), (128, 64))]


def f32_bound(h_in, w_in, h_out, w_out, scale):
    return 4.0 * (max(RC.ksize(h_in, h_out), RC.ksize(w_in, w_out)) + 2) * RC.U * scale


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", U8_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resize_u8_is_pillow(shape, kind):
    a = RC.contents(kind, shape, seed=shape[1] * 7 + shape[2])
    if shape[0] > 1 and kind in ("random", "strokes"):
        assert not np.array_equal(a[0], a[1])
    x = torch.from_numpy(a).to(DEV)
    got = resize.resize_u8(x)
    want = RC.pillow_resize(a)
    assert got.shape == (shape[0], 64, 64) and got.dtype == torch.uint8
    differing = int((got.cpu().numpy() != want).sum())
    print(f"{shape} {kind}: {differing} differing bytes")
    assert differing == 0
    assert torch.equal(resize.resize_u8(x), got)                             # a second call: bit-equal
    four = resize.resize_u8(x[:, None])                                      # (N, 1, H, W) keeps its rank
    assert four.shape == (shape[0], 1, 64, 64) and torch.equal(four[:, 0], got)


@pytest.mark.parametrize("shape,size", OTHER_SIZES, ids=lambda v: "x".join(map(str, v)))
def test_resize_u8_is_pillow_where_the_kernel_takes_another_path(shape, size):
    a = RC.contents("random", shape, seed=11)
    x = torch.from_numpy(a).to(DEV)
    got = resize.resize_u8(x, size)
    assert tuple(got.shape) == (shape[0],) + size
    assert int((got.cpu().numpy() != RC.pillow_resize(a, size)).sum()) == 0
    out = torch.full_like(got, 7)
    assert resize.resize_u8(x, size, out=out) is out and torch.equal(out, got)


def test_device_refusals():
    x = torch.zeros(2, 128, 256, dtype=torch.uint8, device=DEV)
    for fn, t in ((resize.resize_u8, x[:, :, ::2]), (resize.resize_f32, x.float()[:, :, ::2])):
        with pytest.raises(ValueError, match="contiguous"):
            fn(t)
    with pytest.raises(ValueError, match="contiguous"):
        resize.resize_f32_adjoint(torch.zeros(2, 64, 128, device=DEV)[:, :, ::2], 128)
    with pytest.raises(ValueError, match="out must be"):
        resize.resize_u8(x, 64, out=torch.zeros(2, 64, 63, dtype=torch.uint8, device=DEV))
    assert resize.resize_u8(x[:0]).shape == (0, 64, 64)                      # an empty batch: nothing is launched


@pytest.mark.parametrize("e", [40, 128])
def test_embed_resized_is_embed_u8_of_pillows_bytes(e):
    from signature_gan_amd.signature_verifier_eval import SiameseNetwork
    m = SiameseNetwork(e, max_images=2)                                      # n = 5 crosses two chunk boundaries
    m.load_state_dict(VC.torch_state(e), strict=True)
    m = m.to(DEV).eval()
    a = RC.contents("strokes", (5, 128, 128), seed=3)
    want = m.embed_u8(torch.from_numpy(RC.pillow_resize(a)).to(DEV))
    got = m.embed_resized(torch.from_numpy(a).to(DEV))
    assert got.shape == (5, e) and torch.equal(got, want)
    assert not torch.equal(got[0], got[1])
    # 64x64 input: embed_u8 / forward_one themselves
    small = torch.from_numpy(RC.contents("strokes", (3, 64, 64), seed=4)).to(DEV)
    assert torch.equal(m.embed_resized(small), m.embed_u8(small))
    f = (small.float() / 127.5 - 1.0)[:, None].contiguous()
    assert torch.equal(m.embed_resized(f), m.forward_one(f))
    # fp32 at 128: resize_f32 then forward_one
    big = (torch.from_numpy(a).to(DEV).float() / 127.5 - 1.0)[:, None].contiguous()
    assert torch.equal(m.embed_resized(big), m.forward_one(resize.resize_f32(big)))


def f32_case(shape, size, seed):
    """x, dy on the device; the fp64 dense maps; y = R_h x R_w^T and dx = R_h^T dy R_w in fp64."""
    n, h, w = shape
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, size=shape).astype(np.float32)
    dy = rng.uniform(-1, 1, size=(n,) + size).astype(np.float32)
    rh, rw = RC.dense(h, size[0]), RC.dense(w, size[1])
    y_ref = np.einsum("oh,nhw,pw->nop", rh, x.astype(np.float64), rw)
    dx_ref = np.einsum("oh,nop,pw->nhw", rh, dy.astype(np.float64), rw)
    return x, dy, y_ref, dx_ref


def f32_margins(shape, size=(64, 64), seed=5):
    """Worst error / bound of the forward map, of the adjoint and of the inner-product identity, on the device."""
    n, h, w = shape
    x, dy, y_ref, dx_ref = f32_case(shape, size, seed)
    xd, dyd = torch.from_numpy(x).to(DEV), torch.from_numpy(dy).to(DEV)
    y, dx = resize.resize_f32(xd, size), resize.resize_f32_adjoint(dyd, (h, w))
    assert tuple(y.shape) == (n,) + size and tuple(dx.shape) == shape
    assert torch.equal(resize.resize_f32(xd, size), y) and torch.equal(resize.resize_f32_adjoint(dyd, (h, w)), dx)
    y, dx = y.cpu().double().numpy(), dx.cpu().double().numpy()
    b_fwd = f32_bound(h, w, size[0], size[1], float(np.abs(x).max()))
    b_adj = f32_bound(h, w, size[0], size[1], float(np.abs(dy).max()))
    lhs, rhs = float((y * dy).sum()), float((x.astype(np.float64) * dx).sum())
    b_dot = b_fwd * float(np.abs(dy).max()) * y.size + b_adj * float(np.abs(x).max()) * dx.size
    return {"shape": list(shape), "size": list(size), "forward_error_over_bound": float(np.abs(y - y_ref).max()) / b_fwd,
            "adjoint_error_over_bound": float(np.abs(dx - dx_ref).max()) / b_adj,
            "inner_product_difference_over_bound": abs(lhs - rhs) / b_dot, "bound_forward": b_fwd, "bound_adjoint": b_adj}


@pytest.mark.parametrize("shape", F32_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resize_f32_and_adjoint_against_fp64(shape):
    m = f32_margins(shape)
    print(json.dumps(m))
    assert m["forward_error_over_bound"] <= 1.0
    assert m["adjoint_error_over_bound"] <= 1.0
    assert m["inner_product_difference_over_bound"] <= 1.0


@pytest.mark.parametrize("shape,size", F32_OTHER, ids=lambda v: "x".join(map(str, v)))
def test_resize_f32_where_the_kernel_takes_another_path(shape, size):
    """The forward map (bound as above, max|x| <= 1) and the adjoint at the shapes where nothing is staged, the image is banded
    or an axis is upsampled.  The adjoint's weights there do not sum to 1: a pass sums at most ``terms`` products (ksize when
    the axis shrinks, at most n_out when it grows) whose weights sum to that axis' largest column sum c of R, so its error is
    at most (terms + 2) u c max|input|; the second pass adds its own and carries the first one's times its c:
    (terms_h + terms_w + 4) u c_h c_w max|dy| <= 2 (terms + 2) u c_h c_w, held here with the factor 4 of the forward bound."""
    n, h, w = shape
    x, dy, y_ref, dx_ref = f32_case(shape, size, seed=9)
    y = resize.resize_f32(torch.from_numpy(x).to(DEV), size).cpu().double().numpy()
    dx = resize.resize_f32_adjoint(torch.from_numpy(dy).to(DEV), (h, w)).cpu().double().numpy()
    assert float(np.abs(y - y_ref).max()) <= f32_bound(h, w, size[0], size[1], 1.0)
    colsum = RC.dense(h, size[0]).sum(axis=0).max() * RC.dense(w, size[1]).sum(axis=0).max()      # max of sum_o |R[o, i]|, both axes
    terms = max(size[0] if size[0] > h else RC.ksize(h, size[0]), size[1] if size[1] > w else RC.ksize(w, size[1]))
    assert float(np.abs(dx - dx_ref).max()) <= 4.0 * (terms + 2) * RC.U * max(colsum, 1.0)


def test_f32_path_against_the_byte_path():
    a = RC.contents("strokes", (3, 128, 128), seed=6)
    b = torch.from_numpy(a).to(DEV)
    f = resize.resize_f32(b.float() / 127.5 - 1.0)
    u = resize.resize_u8(b).float() / 127.5 - 1.0
    worst = float((f - u).abs().max())
    print(f"fp32 path vs byte path: worst {worst * 127.5:.4f} bytes")
    assert worst <= 1.01 / 127.5


@pytest.fixture(scope="module")
def verifier():
    from signature_gan_amd.signature_verifier_eval import SiameseNetwork
    v = SiameseNetwork(40, max_images=8)
    v.load_state_dict(IC.identity_state(40, dtype=torch.float32), strict=True)
    return v.to(DEV).eval()


def test_input_grad_resized_is_the_composition(verifier):
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.uniform(-1, 1, size=(3, 1, 128, 128)).astype(np.float32)).to(DEV)
    ref = verifier.embed_resized(torch.from_numpy(RC.contents("strokes", (3, 128, 128), seed=2)).to(DEV))
    dx, obj, terms, score, emb = verifier.input_grad_resized(x, ref, 0.5, 2.0, want_terms=True, want_score=True, want_emb=True)
    small = resize.resize_f32(x)
    dxs, obj2, terms2, score2, emb2 = verifier.input_grad(small, ref, 0.5, 2.0, want_terms=True, want_score=True, want_emb=True)
    assert dx.shape == x.shape and torch.equal(dx, resize.resize_f32_adjoint(dxs, (128, 128)))
    for a, b in ((obj, obj2), (terms, terms2), (score, score2), (emb, emb2)):
        assert torch.equal(a, b)
    assert torch.equal(emb, verifier.embed_resized(x))
    assert torch.equal(score, verifier.compare(verifier.embed_resized(x), ref).reshape(-1))
    assert float(dx.abs().max()) > 0 and bool(torch.isfinite(dx).all())
    out = torch.zeros_like(dx)
    assert torch.equal(verifier.input_grad_resized(x, ref, 0.5, 2.0, dx_out=out)[0], dx) and torch.equal(out, dx)
    x64 = small.clone()                                                      # 64x64: input_grad itself
    assert torch.equal(verifier.input_grad_resized(x64, ref, 0.5, 2.0)[0], dxs)


def generator(size):
    from signature_gan_amd.generator_vanilla_gan import Generator
    g = Generator(latent_dim=P_LATENT, output_size=size).to(DEV)
    g.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in I.gen_state(O.g_state_specs(P_LATENT, size), SEED["state_g"]).items()})
    return g.eval()


def same(a, b):
    return all(np.array_equal(*(t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in pair)) for pair in zip(a, b))


def test_projection_with_a_128_generator(verifier):
    from signature_gan_amd.utils.inference import generate_uint8, project_signatures
    g = generator(128)
    _, z_star, z0 = projection_case()
    t = generate_uint8(g, z_star[:2].to(DEV))
    assert t.shape == (2, 128, 128)
    kw = dict(steps=2, lr=P_LR, betas=P_BETAS, z0=z0[:2])
    with pytest.raises(ValueError, match="64x64"):
        project_signatures(g, t, verifier=verifier, identity_weight=0.5, **kw)
    z, recon, loss, hist = project_signatures(g, t, verifier=verifier, identity_weight=0.5, identity_score_weight=2.0,
                                              verifier_resize=True, **kw)
    assert z.shape == (2, P_LATENT) and recon.shape == (2, 128, 128) and hist.shape == (2, 2)
    assert all(bool(torch.isfinite(v).all()) for v in (z, loss, hist))
    plain = project_signatures(g, t, **kw)
    assert bool((hist[0] > plain[3][0]).all()) and not torch.equal(z, plain[0])     # the identity term is in the objective
    # with both identity weights 0: the call without a verifier, bit for bit
    assert same(project_signatures(g, t, verifier=verifier, identity_weight=0.0, identity_score_weight=0.0, verifier_resize=True, **kw), plain)


def test_projection_with_a_64_generator_does_not_change_a_bit(verifier):
    from signature_gan_amd.utils.inference import generate_uint8, project_signatures
    g = generator(P_SIZE)
    _, z_star, z0 = projection_case()
    t = generate_uint8(g, z_star[:2].to(DEV))
    kw = dict(steps=2, lr=P_LR, betas=P_BETAS, z0=z0[:2], verifier=verifier, identity_weight=0.5, identity_score_weight=2.0)
    assert same(project_signatures(g, t, verifier_resize=True, **kw), project_signatures(g, t, verifier_resize=False, **kw))


def test_projection_cli_records_identity_for_a_128_generator(verifier, tmp_path):
    from PIL import Image
    from signature_gan_amd import generate_signatures as cli
    from signature_gan_amd.utils.inference import generate_uint8
    g = generator(128)
    t = generate_uint8(g, projection_case()[1][:2].to(DEV))
    ck, vk = tmp_path / "g.pt", tmp_path / "v.pth"
    torch.save({"epoch": 1, "generator_state_dict": {k: v.detach().cpu().clone() for k, v in g.state_dict().items()},
                "config": {"latent_dim": P_LATENT, "image_size": 128}}, ck)
    torch.save({"model_state_dict": IC.identity_state(40, dtype=torch.float32), "embedding_dim": 40, "epoch": 1}, vk)
    src, out = tmp_path / "real", tmp_path / "out"
    src.mkdir()
    for i in range(2):
        Image.fromarray(t[i], mode="L").save(src / f"sig_{i}.png")
    cli.main(["--checkpoint", str(ck), "--output_dir", str(out), "--seed", "3", "--project", str(src), "--project_steps", "2",
              "--project_lr", "0.02", "--verifier_checkpoint", str(vk), "--project_identity_weight", "0.5", "--project_identity_resize"])
    rec = json.load(open(out / "signature_projection.json"))
    assert len(rec) == 2
    for r in rec:
        for key in ("identity", "identity_pixel_only"):
            assert 0 <= r[key]["embedding_distance"] <= 2 and 0 < r[key]["verifier_score"] < 1


def test_evaluate_cli_with_a_verifier_and_a_128_generator(tmp_path, capsys):
    """Modelled on test_verifier_frechet_gpu's CLI test: a random 128 checkpoint and 12 PNGs give a finite distance, the
    neighbour keys and ``verifier_input_resize``; the same call on a 64 checkpoint has it null beside the keys it always had."""
    from PIL import Image
    from signature_gan_amd import evaluate_vanilla_gan_signatures as cli
    vck = tmp_path / "verifier.pth"
    torch.save({"model_state_dict": VC.torch_state(128), "embedding_dim": 128, "val_accuracy": 0.9, "epoch": 1}, vck)
    real_dir = tmp_path / "real"
    real_dir.mkdir()
    rng = np.random.default_rng(0)
    for i in range(12):
        a = np.where(rng.uniform(size=(140, 152)) < 0.1, rng.integers(0, 128, (140, 152)), 255).astype(np.uint8)
        Image.fromarray(a, "L").save(real_dir / f"r{i:02d}.png")

    def run(size):
        g = generator(size)
        ck, out = tmp_path / f"ck{size}.pt", tmp_path / f"out{size}"
        torch.save({"epoch": 2, "generator_state_dict": {k: v.detach().cpu().clone() for k, v in g.state_dict().items()},
                    "config": {"latent_dim": P_LATENT, "image_size": size, "current_epoch": 2}}, ck)
        rc = cli.main(["--checkpoint", str(ck), "--n_samples", "40", "--batch_size", "16", "--n_grids", "0", "--seed", "3",
                       "--output_dir", str(out), "--real_dir", str(real_dir), "--verifier_checkpoint", str(vck),
                       "--verifier_neighbors", "3"])
        text = capsys.readouterr().out
        reports = glob.glob(str(out / "evaluation_report_*.json"))
        assert rc == 0 and len(reports) == 1, text
        with open(reports[0]) as f:
            return json.load(f)["metrics"]

    m128, m64 = run(128), run(64)
    for m in (m128, m64):
        assert "verifier_frechet_error" not in m and "verifier_neighbors_error" not in m
        assert math.isfinite(m["verifier_frechet_distance"]) and m["verifier_frechet_distance"] > 0
        assert all(m[k] is not None for k in cli.NEIGHBOR_KEYS) and m["verifier_neighbors_k"] == 3
        assert all(0 <= m[k] <= 1 for k in ("verifier_precision", "verifier_recall", "verifier_coverage"))
    assert m128["verifier_input_resize"] == "pillow_bilinear_128_to_64" and m64["verifier_input_resize"] is None
    assert m128["image_shape"] == [1, 128, 128] and set(m128) == set(m64)
    # the verifier saw the real FILES at 64x64, not a 128x128 copy shrunk again: the real set's spread is the 64 run's
    # (the 64 run normalises the bytes before the verifier, the 128 run inside it: the same images up to an fp32 rounding)
    assert math.isclose(m128["verifier_embedding_spread"]["real"], m64["verifier_embedding_spread"]["real"], rel_tol=1e-4)
