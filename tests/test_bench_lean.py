"""bench.py without --full measures the headline product alone; everything else the benchmark
measures or checks is behind --full."""
import importlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what a --full line adds to the headline's
MOVED = ('transform_kernels', 'families', 'full_mvm', 'batch_sweep', 'nll_grad', 'nll_grad_eps1',
         'nll_grad_to_tolerance', 'nll_grad_krylov', 'nll_grad_to_stall',
         'nll_grad_krylov_to_tolerance', 'c2', 'cpu_baseline', 'speedup_vs_cpu_mvm')
SKIPS = ('no_families', 'no_cpu', 'no_sweep', 'no_full', 'no_extra', 'no_stall')


@pytest.fixture
def bench(monkeypatch):
    # (bench.py defaults OMP_NUM_THREADS on import: keep that out of the rest of the session)
    monkeypatch.setenv('OMP_NUM_THREADS', os.environ.get('OMP_NUM_THREADS', '1'))
    return importlib.import_module('bench')


def test_full_is_off_by_default(bench, monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '4', '--warmup', '2'])
    args = bench.parse()
    assert not args.full and (args.steps, args.warmup) == (4, 2)
    assert all(getattr(args, k) for k in SKIPS)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--full'])
    args = bench.parse()
    assert args.full and not any(getattr(args, k) for k in SKIPS) and not args.no_nll
    # the parts of a --full run can still be dropped one by one
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--no-full', '--no-cpu'])
    args = bench.parse()
    assert args.full and args.no_full and args.no_cpu and not args.no_sweep


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
                        '--config', 'c2', '--steps', '3', '--warmup', '1'],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                       env=dict(os.environ, OMP_NUM_THREADS='1'))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line['metric'] == 'kronecker_toeplitz_mvms_per_sec' and line['unit'] == 'MVM/s'
    assert line['higher_is_better'] is True and line['dtype'] == 'f64'
    assert line['steps'] == 3 and line['warmup'] == 1 and line['n_gpus'] == 1
    assert line['value'] > 0 and line['ms_per_step'] > 0
    # value and ms_per_step are one clock: 17 vectors per C2 step
    assert line['value'] == pytest.approx(line['config']['batch'] / (line['ms_per_step'] * 1e-3))
    assert not [k for k in MOVED if k in line]
    assert 'copy_same_vectors' not in line['roofline'] and 'dump_outputs' not in line
