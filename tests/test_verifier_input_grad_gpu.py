"""siggan_verifier_input_grad (SiameseNetwork.input_grad): the verifier's eval-mode gradient with respect to its input images.

dx and the terms are held to the fp64 restatement identitycommon.input_grad_ref ON THE DEVICE'S OWN DECISIONS (pooling routes,
ReLU masks, signs of e - r, read through the debug hook) at the README parity contract's 1e-4 of max|dx_ref| per call; the
decisions to the fp64 run's own wherever that run is not borderline (the trainer tests' criterion); the bit contracts of
include/siggan_verifier_grad.h one by one.  Inputs: VI.gen_x1 against the embeddings of VI.gen_x2, verifiercommon's synthetic state
with a gamma < 0 and a gamma == 0 channel in bn2; N = 65 crosses the 64-row tile of the fc1 input gradient, 1 and 3 are ragged."""
import ctypes as C
import math

import pytest
import torch

import identitycommon as IC

pytestmark = pytest.mark.gpu
#        N   E   weights
CASES = [(1, 128, (0.5, 2.0)), (3, 128, (1.0, 0.0)), (3, 128, (0.0, 1.0)), (3, 128, (0.5, 2.0)), (65, 128, (0.5, 2.0)),
         (1, 40, (0.5, 2.0)), (3, 40, (0.5, 2.0)), (65, 40, (0.5, 2.0))]
MAX_IMAGES = 65


def make_model(e, max_images=MAX_IMAGES):
    from signature_gan_amd.signature_verifier_eval import SiameseNetwork
    m = SiameseNetwork(e, max_images=max_images)
    m.load_state_dict(IC.identity_state(e, dtype=torch.float32), strict=True)
    return m.cuda().eval()


_MODELS = {}


def model(e):
    if e not in _MODELS:
        _MODELS[e] = make_model(e)
    return _MODELS[e]


def device_decisions(m, n, e):
    dec = {k: m.input_grad_debug(k, (n,) + shape).cpu() for k, shape in IC.ROUTES.items()}
    dec["fc1_mask"] = m.input_grad_debug("fc1_mask", (n, 512)).cpu()
    dec["cls_mask"] = m.input_grad_debug("cls_mask", (n, 64)).cpu()
    dec["diff_sign"] = m.input_grad_debug("diff_sign", (n, e), torch.int8).cpu()
    return dec


def compute_case(case):
    """Everything the tests of one case compare (also what profiles/identity_parity_margins.py records)."""
    n, e, w = case
    m = model(e)
    x, t = IC.images(n)
    xc = x.cuda()
    r = m.forward_one(t.cuda())
    out = {"case": case}
    out["embed_before"] = m.forward_one(xc).cpu()
    res = m.input_grad(xc, r, *w, want_terms=True, want_score=True, want_emb=True)
    out["hip"] = tuple(v.cpu() for v in res)                              # dx, objective, terms, score, emb
    out["dec"] = device_decisions(m, n, e)
    out["again"] = tuple(v.cpu() for v in m.input_grad(xc, r, *w, want_terms=True, want_score=True, want_emb=True))
    out["embed_after"] = m.forward_one(xc).cpu()
    out["compare"] = m.compare(res[4], r).reshape(-1).cpu()
    if n == 3:                                                            # images do not interact
        out["single"] = [tuple(v.cpu() for v in m.input_grad(xc[i:i + 1], r[i:i + 1], *w, want_terms=True, want_score=True, want_emb=True))
                         for i in range(n)]
    sd64 = IC.identity_state(e)
    out["ref"] = IC.input_grad_ref(sd64, x, r.cpu(), *w, decisions=out["dec"])
    margins = {}
    out["own"] = IC.input_grad_ref(sd64, x, r.cpu(), *w, margins=margins)
    out["margins"] = margins
    return out


_RUNS = {}
case_id = lambda c: f"n{c[0]}-e{c[1]}-we{c[2][0]:g}-ws{c[2][1]:g}"


def run_of(case):
    if case not in _RUNS:
        _RUNS[case] = compute_case(case)
    return _RUNS[case]


@pytest.fixture(scope="module", params=CASES, ids=case_id)
def run(request):
    return run_of(request.param)


def grad_margins(run):
    """(max|dx - dx_ref| / max|dx_ref|, max|dx_ref|, worst relative term error)"""
    ref, (dx, obj, terms, score, emb) = run["ref"], run["hip"]
    scale = float(ref["dx"].abs().max())
    err = float((dx.double() - ref["dx"]).abs().max()) / scale
    tscale = float(ref["terms"].abs().max())
    terr = float((terms.double() - ref["terms"]).abs().max()) / tscale
    return err, scale, terr


def test_gradient_and_terms_are_the_restatements_on_the_devices_decisions(run):
    err, scale, terr = grad_margins(run)
    ref, (dx, obj, terms, score, emb) = run["ref"], run["hip"]
    dead = IC.dead_fraction(run["dec"])
    print(f"{run['case']}: max|dx - dx_ref| / max|dx_ref| = {err:.3e} (max|dx_ref| {scale:.3e}), terms {terr:.3e}, "
          f"max|logit| {float(ref['logit'].abs().max()):.3f}, dead {dead}")
    # not vacuous
    assert scale > 0
    p = score.double()
    assert float((torch.log(p) - torch.log1p(-p)).abs().max()) < 6 and float(ref["logit"].abs().max()) < 6
    assert all(v < 0.9 for v in dead.values()), dead
    assert err <= IC.BOUND, err
    assert terr <= IC.BOUND, terr
    w = run["case"][2]
    for k in range(2):                                                    # a term whose weight is 0 is reported as 0
        assert w[k] or not terms[k].any()
    want = w[0] * terms[0].double() + w[1] * terms[1].double()
    assert float((obj.double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())


def test_decisions_differ_only_where_fp64_is_borderline(run):
    counts = IC.differing(run["dec"], run["own"]["decisions"], run["margins"])
    print(f"{run['case']}: (differing, of those borderline) {counts}")
    for k, (diff, near) in counts.items():
        assert diff == near, (k, diff, near)


def test_embedding_and_score_are_the_inference_calls_bits(run):
    dx, obj, terms, score, emb = run["hip"]
    assert torch.equal(emb, run["embed_before"])
    assert torch.equal(score, run["compare"])
    assert torch.equal(run["embed_after"], run["embed_before"])          # embed is unchanged by an input_grad call in between


def test_two_calls_give_the_same_bits(run):
    for a, b in zip(run["hip"], run["again"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == 3], ids=case_id)
def test_images_do_not_interact(case):
    """The rows of an N = 3 call are the same images run as three N = 1 calls."""
    run = run_of(case)
    dx, obj, terms, score, emb = run["hip"]
    for i, (dx1, obj1, terms1, score1, emb1) in enumerate(run["single"]):
        assert torch.equal(dx[i:i + 1], dx1) and torch.equal(obj[i:i + 1], obj1) and torch.equal(terms[:, i:i + 1], terms1)
        assert torch.equal(score[i:i + 1], score1) and torch.equal(emb[i:i + 1], emb1)


def test_constant_images_route_to_the_first_element():
    """x = const: the four elements of every window away from the border are equal, so every route is 0 (or 4)."""
    e, n = 40, 2
    m = model(e)
    x = torch.stack([torch.full((1, 64, 64), 0.3), torch.full((1, 64, 64), -0.7)]).cuda()
    r = m.forward_one(IC.images(n)[1].cuda())
    m.input_grad(x, r, 1.0, 1.0)
    for k, (c, h, _) in IC.ROUTES.items():
        rt = m.input_grad_debug(k, (n, c, h, h)).cpu()
        b = {"route1": 1, "route2": 2, "route3": 3}[k]                    # (at least) the windows the zero padding reaches
        inner = rt[:, :, b:h - b, b:h - b]
        assert bool(((inner == 0) | (inner == 4)).all()), k
        assert bool((inner == 0).any()), k


def test_score_and_embed_results_are_unchanged_by_the_call():
    e, n = 128, 4
    m = model(e)
    x, t = IC.images(n)
    xc, tc = x.cuda(), t.cuda()
    before = tuple(v.cpu() for v in m(xc, tc))
    m.input_grad(xc, m.forward_one(tc), 0.5, 2.0)
    after = tuple(v.cpu() for v in m(xc, tc))
    for a, b in zip(before, after):
        assert torch.equal(a, b)


def test_out_tensors_are_written_in_place():
    e, n = 40, 3
    m = model(e)
    x, t = IC.images(n)
    r = m.forward_one(t.cuda())
    dx, obj = torch.empty(n, 1, 64, 64, device="cuda"), torch.empty(n, device="cuda")
    got = m.input_grad(x.cuda(), r, 0.5, 2.0, dx_out=dx, objective_out=obj)
    want = m.input_grad(x.cuda(), r, 0.5, 2.0)
    assert got[0] is dx and got[1] is obj
    assert torch.equal(dx, want[0]) and torch.equal(obj, want[1])


def test_refusals_enqueue_nothing():
    from signature_gan_amd import _lib
    e, n = 40, 2
    m = make_model(e, max_images=2)
    ctx = m._context()
    lib, h = ctx.lib, ctx._h
    pool = torch.zeros(n * 4096 + 4, device="cuda")
    x = pool[:n * 4096]
    r = torch.zeros(n, e, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    state = {}

    def call(x_=x, r_=r, n_=n, w=(1.0, 1.0), dx="own", obj="own", handle=h):
        state["dx"], state["obj"] = torch.full((n * 4096 + 4,), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
        dx_ = state["dx"][:n * 4096] if isinstance(dx, str) and dx == "own" else dx
        obj_ = state["obj"] if isinstance(obj, str) and obj == "own" else obj
        wp = C.byref(_lib.VerifierIdentity(*w)) if w is not None else None
        return lib.siggan_verifier_input_grad(handle, p(x_), p(r_), n_, wp, p(dx_), p(obj_), None, None, None, ctx._stream())

    def refused(**kw):
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc == _lib.E_ARG, (kw, rc)
        assert bool((state["dx"] == 7.0).all()) and bool((state["obj"] == 7.0).all())       # nothing ran

    refused()                                                              # before enable
    assert lib.siggan_verifier_input_grad_enable(h) == 0
    assert lib.siggan_verifier_input_grad_enable(h) == 0                   # twice: a no-op
    ctx._grad_enabled = True
    for w in ((-1.0, 1.0), (1.0, -0.5), (math.nan, 1.0), (1.0, math.inf), (0.0, 0.0), None):
        refused(w=w)
    refused(x_=None); refused(r_=None); refused(dx=None); refused(obj=None)
    refused(x_=pool[1:1 + n * 4096])                                       # misaligned x
    state["dx"] = torch.full((n * 4096 + 4,), 7.0, device="cuda")
    refused(n_=0); refused(n_=3)
    rc = lib.siggan_verifier_input_grad(h, p(x), p(r), n, C.byref(_lib.VerifierIdentity(1.0, 1.0)), p(pool[1:1 + n * 4096]),
                                        p(torch.empty(n, device="cuda")), None, None, None, ctx._stream())
    assert rc == _lib.E_ARG                                                # misaligned dx
    assert call() == 0                                                     # and the context works after refusals
    torch.cuda.synchronize()
    assert bool(torch.isfinite(state["dx"][:n * 4096]).all()) and not bool((state["dx"][:n * 4096] == 7.0).all())
    # before bind
    hh = C.c_void_p()
    assert lib.siggan_verifier_create(0, e, 2, C.byref(hh)) == 0
    assert lib.siggan_verifier_input_grad_enable(hh) == 0
    refused(handle=hh)
    lib.siggan_verifier_destroy(hh)
