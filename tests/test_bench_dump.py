"""bench.py --dump-outputs: the arrays the timed paths returned in their last step, from inputs
that are the same on every run with the same arguments (so that two builds can be compared
output for output), within the size budget."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bench(monkeypatch):
    # (bench.py defaults OMP_NUM_THREADS on import: keep that out of the rest of the session)
    monkeypatch.setenv('OMP_NUM_THREADS', os.environ.get('OMP_NUM_THREADS', '1'))
    return importlib.import_module('bench')


def test_product_sample_and_budget(bench, tmp_path):
    Y = torch.randn(7, 1000, dtype=torch.float64)
    full, cols = bench.product_sample(Y)
    assert np.array_equal(cols, np.arange(1000)) and np.array_equal(full, Y.numpy())
    part, cols = bench.product_sample(Y, nbytes=7 * 8 * 100)
    assert part.shape == (7, 100) and np.all(np.diff(cols) > 0) and cols[-1] < 1000
    assert np.array_equal(part, Y.numpy()[:, cols])
    again, cols2 = bench.product_sample(torch.zeros(7, 1000, dtype=torch.float64), nbytes=7 * 8 * 100)
    assert np.array_equal(cols, cols2) and not again.any()

    shapes = bench.write_dumps(str(tmp_path / 'out'), {'a': part, 'b': np.float32(2.5)})
    assert shapes == {'a': [7, 100], 'b': []}
    a = np.load(tmp_path / 'out' / 'a.npy')
    assert a.dtype == np.float64 and np.array_equal(a, part)
    assert float(np.load(tmp_path / 'out' / 'b.npy')) == 2.5
    with pytest.raises(AssertionError):
        bench.write_dumps(str(tmp_path / 'big'), {'a': np.zeros(bench.DUMP_BYTES // 8 + 1)})


@pytest.mark.gpu
def test_dump_outputs_c2(tmp_path):
    """The dumped product is K_UU X for the X the run regenerates from its seed (checked
    against the oracle's product), the NLL step's outputs are finite, and all of it fits."""
    from oracle import operators as ops
    from runlmc_amd.util import synth
    out = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
                        '--config', 'c2', '--steps', '3', '--warmup', '1', '--no-cpu', '--no-sweep',
                        '--no-extra', '--no-families', '--no-full', '--dump-outputs', str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900,
                       env=dict(os.environ, OMP_NUM_THREADS='1'))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert line['steps'] == 3
    names = sorted(f[:-4] for f in os.listdir(out))
    assert names == sorted(line['dump_outputs']) == ['grid_mvm', 'grid_mvm_columns',
                                                     'nll_grad_gradient', 'nll_grad_nll_logdet']
    arrays = {k: np.load(out / (k + '.npy')) for k in names}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20

    D, Q, R, m, n_probes = synth.CONFIGS['c2']
    p = synth.make_problem(D, Q, R, m)
    gen = torch.Generator(device='cpu').manual_seed(1000)
    X = torch.randn(n_probes + 1, D * p.m, dtype=torch.float64, generator=gen).numpy()
    cols = arrays['grid_mvm_columns'].astype(np.int64)
    Bs = ops.coreg_mats(list(p.coreg_vecs), list(p.coreg_diags))
    toeps = [ops.BTTBOracle(t) for t in synth.tops(p)]
    ref = np.array([ops.grid_sum_matvec(Bs, toeps, x) for x in X])[:, cols]
    got = arrays['grid_mvm']
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-11 * np.abs(ref).max()

    n_params = Q * R * D + Q * D + Q + D
    assert arrays['nll_grad_gradient'].shape == (n_params,)
    assert np.all(np.isfinite(arrays['nll_grad_gradient']))
    assert np.all(np.isfinite(arrays['nll_grad_nll_logdet']))
    assert arrays['nll_grad_nll_logdet'][0] == pytest.approx(line['nll_grad']['nll'], rel=1e-6)
