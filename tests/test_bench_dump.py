"""CPU: bench.py --dump-outputs writes float64 .npy files, within its size limit, with one fixed, seeded sample of envs
shared by every array of a batch when the outputs are larger (bench.dump_outputs, on host tensors here; the GPU twin is
tests/test_bench_contract.py::test_plain_line_and_dumped_outputs)."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _arrays(B):
    g = torch.Generator().manual_seed(0)
    return [("x", torch.rand((2, B), generator=g, dtype=torch.float64)),
            ("traj", torch.rand((3, 5, B), generator=g, dtype=torch.float64)),
            ("done", (torch.rand(B, generator=g) > 0.5).to(torch.uint8)),
            ("nsteps", torch.randint(0, 9, (2, B), generator=g, dtype=torch.int32))]


def test_small_outputs_are_written_whole_in_float64(tmp_path):
    b = _bench()
    arrays = _arrays(1000)
    assert b.dump_outputs(str(tmp_path), arrays) == ["x", "traj", "done", "nsteps"]
    for name, t in arrays:
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, t.double().numpy())
    assert not (tmp_path / "env_index.npy").exists()


def test_large_outputs_are_a_fixed_sample_within_the_limit(tmp_path):
    b = _bench()
    B, limit = 4000, 100_000
    arrays = _arrays(B)
    names = b.dump_outputs(str(tmp_path / "a"), arrays, limit_bytes=limit)
    assert names == ["x", "traj", "done", "nsteps", "env_index"]
    assert sum(np.load(tmp_path / "a" / f"{n}.npy").nbytes for n in names) <= limit
    ix = np.load(tmp_path / "a" / "env_index.npy")
    assert ix.dtype == np.float64 and 0 < ix.size < B and np.all(np.diff(ix) > 0)
    for name, t in arrays:  # every array keeps the same envs
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), t.double().numpy()[..., ix.astype(np.int64)])
    b.dump_outputs(str(tmp_path / "b"), arrays, limit_bytes=limit)  # the same sample from run to run
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy"))


def test_full_is_off_by_default_and_dump_outputs_takes_a_directory():
    ap = _bench().arg_parser()
    a = ap.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and a.dump_outputs is None and a.steps == 20 and a.warmup == 5
    a = ap.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"
