"""Host side of the parameter gradient and few-shot adaptation (no GPU): the new entry points are declared, listed and exported
and refuse a null context; adaptation_plan names the trainable and the frozen state_dict keys in parameters() order; the CLI takes
the new flags and keeps the namespace of every older command line; the argument checks raise before anything reaches a device."""
import os
import re

import numpy as np
import pytest
import torch

from common import O, ROOT

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib, layout
from signature_gan_amd.generate_signatures import ADAPT_DEFAULTS, LATER_DEFAULTS, adapt_opt, parse_args
from signature_gan_amd.utils.inference import adapt_generator, adaptation_plan, restore_generator


def test_entry_points_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "siggan.h")).read()
    decl = re.search(r"int siggan_g_param_grad\(([^)]*)\)", header)
    assert decl and len(decl.group(1).split(",")) == 13
    decl = re.search(r"int siggan_op_anchor\(([^)]*)\)", header)
    assert decl and len(decl.group(1).split(",")) == 7
    assert "#define SIGGAN_ABI_VERSION 4" in header                       # symbols are added, nothing existing changes
    assert "siggan_g_param_grad" in _lib.EXPORTS and "siggan_op_anchor" in _lib.EXPORTS
    lib = _lib.load()
    assert len(lib.siggan_g_param_grad.argtypes) == 13 and len(lib.siggan_op_anchor.argtypes) == 7
    assert lib.siggan_g_param_grad(None, None, 1, None, None, None, 0, None, None, None, None, None, None) == -1    # a null context
    assert lib.siggan_op_anchor(None, None, None, None, 1, 0.0, None) == -1
    assert len(lib.siggan_g_latent_objective_grad.argtypes) == 12        # the older entry point is as it was


@pytest.mark.parametrize("size, latent", [(64, 100), (128, 128)])
def test_adaptation_plan_follows_the_state_dict_order(size, latent):
    keys = O.param_names(O.g_state_specs(latent, size))
    lg = len(O.G_CHAIN[size]) - 1
    assert lg == {64: 4, 128: 5}[size]
    assert [k for layer in layout.generator_layer_keys(lg) for k in layer] == keys
    sizes = {k: int(np.prod(shape)) for k, (shape, kind) in O.g_state_specs(latent, size).items() if kind == "param"}
    for fl in range(lg + 2):
        train, frozen = adaptation_plan(fl, lg)
        assert frozen + train == keys                                     # a prefix and a suffix of parameters() order
        first = "fc.0.weight" if fl == 0 else ("final_conv.0.weight" if fl == lg + 1 else f"upsample_blocks.{fl - 1}.block.0.weight")
        assert train[0] == first and train[-1] == "final_conv.0.bias"
        spans = layout.spans(layout.generator_entries(latent, size))[0]
        assert spans[train[0]][0] == sum(sizes[k] for k in frozen)        # where Engine.layer_span puts the trainable suffix
    assert adaptation_plan(lg + 1, lg) == (["final_conv.0.weight", "final_conv.0.bias"], keys[:-2])
    for bad in (-1, lg + 2):
        with pytest.raises(ValueError, match="first_layer"):
            adaptation_plan(bad, lg)


def test_cli_takes_the_new_flags_and_keeps_older_namespaces():
    a = parse_args(["--checkpoint", "g.pt"])
    assert not set(vars(a)) & (set(ADAPT_DEFAULTS) | set(LATER_DEFAULTS))   # an older command line parses to what it did
    assert {k: adapt_opt(a, k) for k in ADAPT_DEFAULTS} == dict(adapt=None, adapt_steps=100, adapt_lr=1e-4, adapt_first_layer=0,
                                                                adapt_anchor=0.0, adapt_realism_weight=0.0, adapt_sigma=None,
                                                                adapt_save=None)
    b = parse_args(["--checkpoint", "g.pt", "--project", "dir", "--noise_scale", "0.5"])
    assert not set(vars(b)) & set(ADAPT_DEFAULTS)
    a = parse_args(["--checkpoint", "g.pt", "--adapt", "dir"])
    assert set(vars(a)) & set(ADAPT_DEFAULTS) == {"adapt"} and adapt_opt(a, "adapt") == "dir" and adapt_opt(a, "adapt_steps") == 100
    a = parse_args(["--checkpoint", "g.pt", "--adapt", "dir", "--adapt_steps", "7", "--adapt_lr", "0.001", "--adapt_first_layer", "3",
                    "--adapt_anchor", "0.5", "--adapt_realism_weight", "0.25", "--adapt_sigma", "0.1", "--adapt_save", "out.pt"])
    assert [adapt_opt(a, k) for k in ADAPT_DEFAULTS] == ["dir", 7, 0.001, 3, 0.5, 0.25, 0.1, "out.pt"]
    for bad in (["--adapt_steps", "3"], ["--adapt_lr", "0.1"], ["--adapt_save", "x.pt"], ["--adapt_sigma", "0.1"],
                ["--adapt", "d", "--adapt_steps", "0"], ["--adapt", "d", "--adapt_lr", "0"], ["--adapt", "d", "--adapt_anchor", "-1"],
                ["--adapt", "d", "--adapt_first_layer", "-1"], ["--adapt", "d", "--adapt_sigma", "-0.1"],
                ["--adapt", "d", "--project", "d"], ["--adapt", "d", "--morph"], ["--adapt", "d", "--filter_by_realism"],
                ["--adapt", "d", "--refine_by_realism"]):
        with pytest.raises(SystemExit):
            parse_args(["--checkpoint", "g.pt"] + bad)


def test_argument_checks_raise_before_a_device_is_needed():
    from signature_gan_amd.generator_vanilla_gan import Generator
    g = Generator(latent_dim=100, output_size=64)
    t = np.zeros((2, 64, 64), np.uint8)
    with pytest.raises(ValueError, match="eval"):
        adapt_generator(g, t, z=torch.zeros(2, 100))                      # a Generator in train() mode
    g.eval()
    with pytest.raises(RuntimeError, match="HIP engine"):
        adapt_generator(g, t, z=torch.zeros(2, 100))                      # there is no CPU path
    with pytest.raises(RuntimeError, match="HIP engine"):
        restore_generator(g, torch.zeros(1))
