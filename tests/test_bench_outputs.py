"""bench.py --dump-outputs: what the last timed step returned to its caller, as float32 .npy files of bounded size, with the
parameter sample at the same positions from run to run (host logic; the timed step itself runs on the device)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _step_result():
    return {"loss": torch.tensor(0.25), "PF_L1": torch.tensor(0.2), "KL": torch.tensor(0.05), "grad_norm": torch.tensor(1.5),
            "Image_L1": None}


def _model(n_in, n_out):
    m = torch.nn.Linear(n_in, n_out)
    with torch.no_grad():                       # every value = its position in model.parameters() flattened in order
        m.weight.copy_(torch.arange(n_in * n_out, dtype=torch.float32).view(n_out, n_in))
        m.bias.copy_(torch.arange(n_in * n_out, n_in * n_out + n_out, dtype=torch.float32))
    return m


def test_outputs_are_the_step_result_and_the_updated_parameters():
    m = _model(8, 4)
    out = bench.step_outputs(_step_result(), m)
    assert sorted(out) == ["KL", "PF_L1", "grad_norm", "loss", "params"]
    assert all(a.dtype == np.float32 for a in out.values())
    assert out["loss"].shape == () and float(out["loss"]) == 0.25 and float(out["grad_norm"]) == 1.5
    assert np.array_equal(out["params"], np.arange(36, dtype=np.float32))


def test_parameter_sample_is_fixed_and_bounded(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_PARAM_SAMPLE", 100)
    m = _model(64, 32)
    a, b = bench.step_outputs(_step_result(), m)["params"], bench.step_outputs(_step_result(), m)["params"]
    assert a.shape == (100,) and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and a[-1] < 64 * 32 + 32       # distinct positions, ascending
    assert bench.DUMP_PARAM_SAMPLE < 64 * 32 + 32


def test_dump_fits_64_mb():
    assert bench.DUMP_PARAM_SAMPLE * 4 + 16 * 4 <= 64 << 20


def test_outputs_written_as_npy(tmp_path):
    out = bench.step_outputs(_step_result(), _model(8, 4))
    bench.write_outputs(out, str(tmp_path / "dump"))
    names = sorted(os.listdir(tmp_path / "dump"))
    assert names == sorted(f"{k}.npy" for k in out)
    for k, a in out.items():
        assert np.array_equal(np.load(tmp_path / "dump" / f"{k}.npy"), a)
