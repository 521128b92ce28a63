"""CPU: bench.py's output dump (float32 .npy, a seeded sample of an array above the cap) and its argument checks."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_outputs_writes_float32_and_samples_large_arrays_the_same_way(tmp_path):
    small = torch.randn(3, 4, 5, dtype=torch.float64)
    large = torch.arange(bench.DUMP_MAX_ELEMS + 1000, dtype=torch.float32).reshape(-1, 8)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), {'small': small, 'large': large, 'scalar': torch.tensor(2.5)})
    s = np.load(tmp_path / 'a' / 'small.npy')
    assert s.dtype == np.float32 and s.shape == (3, 4, 5) and np.array_equal(s, small.float().numpy())
    assert np.load(tmp_path / 'a' / 'scalar.npy') == np.float32(2.5)
    la, lb = np.load(tmp_path / 'a' / 'large.npy'), np.load(tmp_path / 'b' / 'large.npy')
    assert la.dtype == np.float32 and la.shape == (bench.DUMP_MAX_ELEMS,) and np.array_equal(la, lb)
    # distinct elements of the source, in their order
    assert (np.diff(la) > 0).all() and la[0] >= 0 and la[-1] < large.numel()


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2 and '--steps must be at least 1' in r.stderr
