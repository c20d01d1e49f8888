"""Host side of the latent objective and realism-guided refinement (no GPU): the new entry point is declared, listed and
exported and refuses a null context; the weights are validated before anything reaches the device; the refinement plan and the
rules by which a Discriminator comes into the Generator's context are what the documentation says; the CLI takes the new
flags, keeps the namespace of every older command line, and refuses the exclusive pairs with the stated messages."""
import math
import os
import re

import pytest

from common import ROOT

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd.engine import check_objective_weights
from signature_gan_amd.generate_signatures import LATER_DEFAULTS, opt, parse_args
from signature_gan_amd.utils.inference import discriminator_adoption, filter_plan, refine_plan


def test_entry_point_is_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "siggan.h")).read()
    decl = re.search(r"int siggan_g_latent_objective_grad\(([^)]*)\)", header)
    assert decl and len(decl.group(1).split(",")) == 12
    struct = re.search(r"typedef struct siggan_latent_objective \{(.*?)\} siggan_latent_objective;", header, re.S)
    assert struct and re.findall(r"float (\w+);", struct.group(1)) == ["recon_weight", "realism_weight", "prior_weight"]
    assert "#define SIGGAN_ABI_VERSION 4" in header                       # symbols are added, nothing existing changes
    assert "siggan_g_latent_objective_grad" in _lib.EXPORTS
    assert [f[0] for f in _lib.LatentObjective._fields_] == ["recon_weight", "realism_weight", "prior_weight"]
    lib = _lib.load()
    assert len(lib.siggan_g_latent_objective_grad.argtypes) == 12
    assert lib.siggan_g_latent_objective_grad(None, None, 1, None, None, None, None, None, None, None, None, None) == -1   # a null context
    assert len(lib.siggan_g_latent_grad.argtypes) == 9                    # the older entry point is as it was


def test_weights_are_validated_on_the_host():
    assert check_objective_weights(0, 1, 0, False) == (0.0, 1.0, 0.0)
    assert check_objective_weights(16, 1, 0.5, True, want_probs=True) == (16.0, 1.0, 0.5)
    assert check_objective_weights(0, 0, 2, False) == (0.0, 0.0, 2.0)       # the prior alone is an objective
    for bad in ((-1, 1, 0), (0, -1, 0), (0, 1, -0.5), (math.nan, 1, 0), (0, math.inf, 0), (0, 1, math.nan)):
        with pytest.raises(ValueError, match="finite and >= 0"):
            check_objective_weights(*bad, bad[0] > 0)
    with pytest.raises(ValueError, match="all three"):
        check_objective_weights(0, 0, 0, False)
    with pytest.raises(ValueError, match="needs a target"):
        check_objective_weights(1, 1, 0, False)
    with pytest.raises(ValueError, match="recon_weight is 0"):
        check_objective_weights(0, 1, 0, True)
    with pytest.raises(ValueError, match="want_probs"):
        check_objective_weights(1, 0, 0, True, want_probs=True)


def test_refine_plan_walks_chunks_of_max_batch():
    assert refine_plan(5, 2) == [(0, 2), (2, 2), (4, 1)]
    assert refine_plan(3, 64) == [(0, 3)] and refine_plan(64, 64) == [(0, 64)] and refine_plan(0, 4) == []
    for n, mb in ((7, 4), (65, 64), (1000, 64)):
        plan = refine_plan(n, mb)
        assert [t for t0, b in plan for t in range(t0, t0 + b)] == list(range(n)) and all(1 <= b <= mb for _, b in plan)
    for bad in ((-1, 4), (3, 0)):
        with pytest.raises(ValueError):
            refine_plan(*bad)
    # generation refines the batches the filter would draw first: ratio 1.0, the same sizes and seeds
    assert filter_plan(10, 1.0, 4, 7) == (10, [(4, 7), (4, 8), (2, 9)])


def test_adoption_rules_on_cpu_modules():
    from signature_gan_amd.discriminator_vanilla_gan import Discriminator
    from signature_gan_amd.generator_vanilla_gan import Generator
    g, d = Generator(latent_dim=100, output_size=64).eval(), Discriminator(input_size=64).eval()
    assert discriminator_adoption(g, d) == "copy"                         # engines of their own, plain Discriminator, same size
    marker = object()
    g._engine = d._engine = marker
    assert discriminator_adoption(g, d) == "shared"                       # one engine: nothing is copied
    g._engine = d._engine = None
    with pytest.raises(ValueError, match="_engine"):
        discriminator_adoption(g, Discriminator(input_size=64, use_spectral_norm=True).eval())
    with pytest.raises(ValueError, match="_engine"):
        discriminator_adoption(g, Discriminator(input_size=128).eval())
    g._shared_engine = True                                               # the Generator's engine is not its own to write into
    with pytest.raises(ValueError, match="_engine"):
        discriminator_adoption(g, d)
    g._shared_engine = False
    for mod in (g, d):
        mod.train()
        with pytest.raises(ValueError, match="eval"):
            discriminator_adoption(g, d)
        mod.eval()


def test_cli_takes_the_new_flags_and_keeps_older_namespaces():
    a = parse_args(["--checkpoint", "g.pt"])
    assert not set(vars(a)) & set(LATER_DEFAULTS)                         # an older command line parses to what it did
    assert {k: opt(a, k) for k in LATER_DEFAULTS} == dict(refine_by_realism=False, refine_steps=20, refine_lr=0.02, refine_prior=0.0,
                                                          project_realism_weight=0.0, project_prior_weight=0.0)
    a = parse_args(["--checkpoint", "g.pt", "--refine_by_realism", "--refine_steps", "7", "--refine_lr", "0.1", "--refine_prior", "0.3"])
    assert (opt(a, "refine_by_realism"), opt(a, "refine_steps"), opt(a, "refine_lr"), opt(a, "refine_prior")) == (True, 7, 0.1, 0.3)
    a = parse_args(["--checkpoint", "g.pt", "--project", "dir", "--project_realism_weight", "0.5", "--project_prior_weight", "0.2"])
    assert (opt(a, "project_realism_weight"), opt(a, "project_prior_weight")) == (0.5, 0.2)
    for bad in (["--refine_steps", "3"], ["--refine_lr", "0.1"], ["--refine_prior", "0.1"], ["--project_realism_weight", "0.5"],
                ["--project_prior_weight", "0.5"], ["--refine_by_realism", "--refine_steps", "0"], ["--refine_by_realism", "--refine_lr", "0"],
                ["--refine_by_realism", "--refine_prior", "-1"], ["--project", "d", "--project_realism_weight", "-1"]):
        with pytest.raises(SystemExit):
            parse_args(["--checkpoint", "g.pt"] + bad)


@pytest.mark.parametrize("other, name", [(["--filter_by_realism"], "filter_by_realism"), (["--project", "dir"], "project"),
                                         (["--morph"], "morph"), (["--morph", "a.png", "b.png"], "morph")])
def test_cli_refinement_excludes_the_other_modes(other, name, capsys):
    with pytest.raises(SystemExit):
        parse_args(["--checkpoint", "g.pt", "--refine_by_realism"] + other)
    assert f"--refine_by_realism and --{name} are mutually exclusive" in capsys.readouterr().err
