"""The host side of the evaluation tool (evaluate_vanilla_gan_signatures.py, utils/metrics.py): everything that needs no GPU."""
import numpy as np
import pytest
import torch

import signature_gan_amd  # noqa: F401  (import shim for signature-gan_amd/)
from strokecommon import foreground_dict, numpy_counts, stroke_dict, torch_densities


def test_parser_flags_and_defaults():
    from signature_gan_amd.evaluate_vanilla_gan_signatures import parse_args
    a = vars(parse_args(["--checkpoint", "ck.pt"]))
    assert a == {"checkpoint": "ck.pt", "n_samples": 500, "real_dir": None, "output_dir": "figures/evaluation", "batch_size": 64,
                 "n_grids": 3, "grid_size": 64, "device": None, "seed": None}
    b = parse_args(["--checkpoint", "c", "--n_samples", "7", "--real_dir", "r", "--output_dir", "o", "--batch_size", "3",
                    "--n_grids", "2", "--grid_size", "4", "--device", "cuda:0", "--seed", "5"])
    assert (b.n_samples, b.real_dir, b.output_dir, b.batch_size, b.n_grids, b.grid_size, b.device, b.seed) == \
        (7, "r", "o", 3, 2, 4, "cuda:0", 5)
    with pytest.raises(SystemExit):
        parse_args([])                                   # --checkpoint is required


def test_missing_checkpoint_is_exit_code_1(tmp_path, capsys):
    from signature_gan_amd.evaluate_vanilla_gan_signatures import main
    assert main(["--checkpoint", str(tmp_path / "none.pt"), "--output_dir", str(tmp_path / "o")]) == 1
    assert "Error: Checkpoint not found" in capsys.readouterr().out


@pytest.mark.parametrize("signed", [True, False])
def test_counters_to_dictionaries(signed):
    """The pure-numpy half: counters in, the reference's dictionaries out -- both branches, picked from the summed NEG."""
    from signature_gan_amd.utils.metrics import (densities_from_counts, foreground_ratio_from_counts,
                                                 stroke_density_from_counts)
    gen = torch.Generator().manual_seed(4 + signed)
    x = torch.rand(9, 1, 64, 64, generator=gen)
    if signed:
        x = x * 2 - 1
    for thr in (0.5, 0.3):
        counts = numpy_counts(x.numpy(), thr)
        assert (counts[:, 0].sum() > 0) == signed
        want = torch_densities(x, thr)
        got = densities_from_counts(counts, 64 * 64)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert stroke_density_from_counts(counts, 64 * 64) == stroke_dict(want)
        assert foreground_ratio_from_counts(counts, 64 * 64) == foreground_dict(want)
    # the branch can be forced: the unit column of a signed batch
    forced = densities_from_counts(counts, 64 * 64, signed=False)
    assert np.array_equal(forced, counts[:, 2].astype(np.float32) / np.float32(4096))


def test_metrics_tracker():
    from signature_gan_amd.utils.metrics import MetricsTracker
    t = MetricsTracker()
    assert t.get_average("g") == 0.0 and t.get_history("g") == [] and t.get_last("g", 7.0) == 7.0
    t.add("g", 1.0); t.add("g", torch.tensor(3.0)); t.add("d", 0.5)
    assert t.get_average("g") == 2.0 and t.get_all_averages() == {"g": 2.0, "d": 0.5}
    t.reset()
    assert t.get_all_averages() == {} and t.get_history("g") == [2.0] and t.get_last("d") == 0.5
    t.add("g", 4.0)
    t.reset()
    assert t.get_history("g") == [2.0, 4.0] and t.get_history("d") == [0.5] and t.get_last("g") == 4.0


def test_no_cpu_path_and_absent_packages(monkeypatch):
    from signature_gan_amd.utils import metrics as M
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.calculate_stroke_density(torch.zeros(2, 1, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.calculate_foreground_ratio(torch.zeros(2, 1, 8, 8))
    if not M.INCEPTION_AVAILABLE:
        with pytest.raises(ImportError):
            M.calculate_fid(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
    if not M.LPIPS_AVAILABLE:
        with pytest.raises(ImportError):
            M.calculate_lpips_diversity([torch.zeros(1, 8, 8)] * 2)
