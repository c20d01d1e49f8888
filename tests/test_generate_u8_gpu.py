"""siggan_g_generate_u8: the eval-mode Generator forward whose last kernel writes the bytes callers of generation consume and
counts the stroke pixels per image (Engine.g_generate_u8).

Held, exactly, to what the parent path computes: the fp32 images to g_forward's, the bytes to tensor_to_uint8 (numpy on the
CPU) of those images, the counters to numpy float32 counts on them and to siggan_image_stats.  The cases: batch 5 at 64x64
(a ragged strip count per image, two 32-column blocks per row), 128x128 (four column blocks per row: packing across
blocks), a bf16 context (the epilogue acts on the fp32 tanh value of any element type); the final conv's weight and bias
are multiplied by a gain so that the bytes span the whole range, saturated ends included."""
import ctypes as C

import numpy as np
import pytest
import torch

from common import I, SEED
from strokecommon import numpy_counts

pytestmark = pytest.mark.gpu

CASES = [("f32", 64, 100, 5, 1.0), ("f32", 64, 100, 5, 64.0), ("f32", 128, 128, 3, 16.0), ("bf16", 64, 100, 4, 16.0)]
THRESHOLDS = (0.5, 0.6)


def _engine(dtype, size, latent, batch, gain):
    from hipcommon import make_engine
    eng = make_engine(size, latent, batch, dtype=dtype)
    v = eng.views("g")
    v["final_conv.0.weight"].mul_(gain); v["final_conv.0.bias"].mul_(gain)
    eng.params_changed()
    return eng


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-s{c[1]}-b{c[3]}-g{c[4]:g}")
def run(request):
    """One engine per case; everything the tests compare, computed once and brought to the CPU."""
    from signature_gan_amd.engine import Engine
    from signature_gan_amd.utils.inference import tensor_to_uint8
    dtype, size, latent, batch, gain = request.param
    eng = _engine(dtype, size, latent, batch, gain)
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"])).cuda()
    want_img = eng.g_forward(z, training=False)
    out = {"case": request.param, "want_img": want_img.cpu(), "want_u8": tensor_to_uint8(want_img), "stats": {}, "image_stats": {}}
    for thr in THRESHOLDS:
        u8, st, img = eng.g_generate_u8(z, threshold=thr, want_f32=True)
        out["u8"], out["img"] = u8.cpu().numpy(), img.cpu()
        out["stats"][thr] = st.cpu().numpy().astype(np.int64)
        out["image_stats"][thr] = Engine.image_stats(want_img, thr).cpu().numpy().astype(np.int64)
    out["u8_alone"] = eng.g_generate_u8(z).cpu().numpy()            # no counters, no fp32 images: the bytes alone
    # the same stats buffer twice, dirty before the first call: the call zeroes it itself
    st = torch.full((batch, 3), 12345, dtype=torch.int32, device="cuda")
    u8 = torch.empty(batch, size, size, dtype=torch.uint8, device="cuda")
    again = []
    for _ in range(2):
        rc = eng.lib.siggan_g_generate_u8(eng._h, C.c_void_p(z.data_ptr()), batch, C.c_void_p(u8.data_ptr()), None,
                                          C.c_void_p(st.data_ptr()), 0.6, eng._stream())
        assert rc == 0
        again.append(st.cpu().numpy().astype(np.int64))
    out["again"] = again
    eng.close()
    return out


def test_fp32_images_are_g_forwards(run):
    assert run["img"].shape == run["want_img"].shape
    assert torch.equal(run["img"], run["want_img"])


def test_bytes_follow_the_host_rule(run):
    _, size, _, batch, _ = run["case"]
    assert run["u8"].shape == (batch, size, size) and run["u8"].dtype == np.uint8
    assert np.array_equal(run["u8"], run["want_u8"])
    assert np.array_equal(run["u8_alone"], run["want_u8"])


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_counters_are_numpy_float32_counts(run, thr):
    want = numpy_counts(run["want_img"].numpy(), thr)
    assert np.array_equal(run["stats"][thr], want), (run["stats"][thr], want)


@pytest.mark.parametrize("thr", THRESHOLDS)
def test_counters_equal_image_stats(run, thr):
    assert np.array_equal(run["stats"][thr], run["image_stats"][thr])


def test_the_data_is_not_trivial(run):
    """What keeps the comparisons above from passing on flat data (expected figures: the oracle on the CPU, from which the
    HIP image differs by about 1e-6)."""
    dtype, size, _, _, gain = run["case"]
    u8, pixels = run["u8"], size * size
    if (dtype, size, gain) == ("f32", 128, 16.0):
        values = np.unique(u8)
        assert len(values) >= 250 and values[0] == 0 and values[-1] == 255          # oracle: all 256; 245 zeros, 102 x 255
        assert (run["stats"][0.5][:, 1] > 0).all()                                  # oracle: 4-10 % of the pixels
    if (dtype, size, gain) == ("f32", 64, 64.0):
        assert (u8 == 0).any() and (u8 == 255).any()                                # oracle: 5 zeros, 16 023 x 255
    if gain == 1.0:
        frac = run["stats"][0.6][:, 1] / pixels                                     # oracle: 0.62-0.66 at 64x64
        assert ((frac >= 0.05) & (frac <= 0.95)).all(), frac


def test_a_second_call_on_the_same_buffers_counts_the_same(run):
    first, second = run["again"]
    assert np.array_equal(first, run["stats"][0.6]) and np.array_equal(second, first)


def test_batch_growth_and_refusals():
    from signature_gan_amd.utils.inference import tensor_to_uint8
    eng = _engine("f32", 64, 100, 4, 1.0)
    assert eng.max_batch == 4
    z = torch.from_numpy(I.gen_z(5, 100, SEED["z"])).cuda()
    u8, st = eng.g_generate_u8(z, threshold=0.5)                                     # grows like g_forward
    assert eng.max_batch >= 5
    img = eng.g_forward(z, training=False)
    assert np.array_equal(u8.cpu().numpy(), tensor_to_uint8(img))
    assert np.array_equal(st.cpu().numpy(), numpy_counts(img.cpu().numpy(), 0.5))
    with pytest.raises(ValueError):
        eng.g_generate_u8(None)
    with pytest.raises(ValueError):
        eng.g_generate_u8(z, threshold=float("inf"))
    with pytest.raises(ValueError):
        eng.g_generate_u8(z[:, :50])
    eng.close()
