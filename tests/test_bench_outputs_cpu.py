"""bench.py --dump-outputs: file types, the fixed sample of a large output, the size bound; --steps validation.  No GPU
needed."""
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import ROOT
from test_bench_launcher_cpu import _bench_module


def test_dump_outputs_types_and_fixed_sample(tmp_path):
    b = _bench_module()
    n = b.DUMP_MAX_ELEMS + 1000
    arrays = dict(half=torch.ones(3, 4, dtype=torch.float16), losses=np.array([1.0, 2.0]), scalar=torch.tensor(0.5),
                  big=torch.arange(n, dtype=torch.float32), big_np=np.arange(n, dtype=np.float64))
    total = b.dump_outputs(str(tmp_path / 'a'), arrays)
    got = {k: np.load(tmp_path / 'a' / f'{k}.npy') for k in arrays}
    assert got['half'].dtype == np.float32 and got['half'].shape == (3, 4)
    assert got['losses'].dtype == np.float64 and got['losses'].tolist() == [1.0, 2.0]
    assert got['scalar'].shape == () and float(got['scalar']) == 0.5
    assert got['big'].dtype == np.float32 and got['big_np'].dtype == np.float64
    # a large output becomes DUMP_MAX_ELEMS distinct elements in index order, the same ones for a tensor and an array
    assert got['big'].shape == (b.DUMP_MAX_ELEMS,) and np.all(np.diff(got['big']) > 0)
    assert np.array_equal(got['big'], got['big_np'])
    assert total == sum(a.nbytes for a in got.values()) <= 64 << 20
    b.dump_outputs(str(tmp_path / 'b'), dict(big=arrays['big']))
    assert np.array_equal(np.load(tmp_path / 'b' / 'big.npy'), got['big'])       # the sample is fixed from run to run


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and '--steps' in r.stderr and r.stdout == ''
