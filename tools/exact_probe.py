"""Times of the exact dense likelihood on the device (include/runlmc_hip.h rl_exact_*), one JSON
line per size on stdout:

    python tools/exact_probe.py [--sizes 3054,15789,20000,40000] [--no-host]

Sizes: 3054 is the FX2007 fixture, 15789 the weather fixture, every other n a C2-style synthetic
problem (runlmc_amd/util/synth.py: D = 4, Q = 3 RBF kernels, rank 1, n / 4 points per output).
Each line: seconds of assembly, factorisation, K^-1, gradient sums and of the whole
ExactLMCLikelihood with gradients (constructor + functional_kernel.update_gradient); the
factorisation's TFLOP/s (n^3 / 3 flop); torch.linalg.cholesky of the same matrix (rocSOLVER, the
yardstick) and, for n <= 20 000, SciPy's cho_factor + cho_solve(I) on the host with the
OMP_NUM_THREADS of the environment; relative differences of log det against both.  Every device
call here ends in a device synchronisation (the rl_exact_* calls copy results back)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def problem(n):
    """(functional kernel, Xs, Ys, label) of size n."""
    from cases import Case
    import parity_suite as ps
    from runlmc_amd.util import synth
    for name in ('fx2007', 'weather'):
        c = Case(name)
        if c.n == n:
            return ps.functional_kernel_for(c), c.Xs, c.Ys, name
    D, Q, R = 4, 3, 1
    p = synth.make_problem(D, Q, R, n // D)
    return synth.functional_kernel(p), p.Xs, p.Ys, 'c2-style synthetic, %d per output' % (n // D)


def timed(f):
    t = time.perf_counter()
    out = f()
    return time.perf_counter() - t, out


def run(n, host):
    import torch
    from runlmc_amd._native import ExactOp
    from runlmc_amd.lmc import ExactLMCLikelihood
    fk, Xs, Ys, label = problem(n)
    X = np.vstack([np.asarray(x, dtype=float).reshape(len(x), -1) for x in Xs])
    y = np.hstack(Ys)
    lens = [len(v) for v in Ys]
    n = len(y)
    op = ExactOp(n, X.shape[1])
    op.set(X, lens, fk.kernels, fk.coreg_mats(), fk.noise)
    rec = dict(n=n, problem=label, D=fk.D, Q=fk.Q)
    rec['assemble_s'], _ = timed(op.assemble)
    rec['factor_s'], logdet = timed(op.factor)
    rec['factor_tflops'] = n ** 3 / 3 / rec['factor_s'] / 1e12
    ydev = torch.from_numpy(y).to(op.device)
    rec['solve_s'], alpha = timed(lambda: (op.solve(ydev), torch.cuda.synchronize())[0])
    rec['inverse_s'], _ = timed(op.invert)
    rec['grad_sums_s'], _ = timed(lambda: op.grad_sums(alpha))

    def whole():
        lik = ExactLMCLikelihood(fk, Xs, Ys)
        fk.update_gradient(lik)
        return lik
    rec['likelihood_with_gradients_s'], lik = timed(whole)
    rec['logdet'] = logdet
    del lik
    K = op.dense()
    Kd = torch.from_numpy(K).to(op.device)
    torch.linalg.cholesky(Kd[:64, :64])
    torch.cuda.synchronize()
    t = time.perf_counter()
    Lt = torch.linalg.cholesky(Kd)
    torch.cuda.synchronize()
    rec['torch_cholesky_s'] = time.perf_counter() - t
    ld_t = float(2.0 * torch.log(torch.diagonal(Lt)).sum())
    del Lt, Kd
    torch.cuda.empty_cache()
    rec['factor_over_torch'] = rec['factor_s'] / rec['torch_cholesky_s']
    rec['logdet_rel_diff_torch'] = abs(logdet - ld_t) / abs(ld_t)
    if host and n <= 20000:
        import scipy.linalg as la
        rec['omp_num_threads'] = os.environ.get('OMP_NUM_THREADS')
        t = time.perf_counter()
        cf = la.cho_factor(K, lower=True, overwrite_a=True)
        Kinv = la.cho_solve(cf, np.identity(n), overwrite_b=True)
        rec['scipy_factor_inverse_s'] = time.perf_counter() - t
        ld_s = 2.0 * np.log(np.diag(cf[0])).sum()
        rec['logdet_rel_diff_scipy'] = abs(logdet - ld_s) / abs(ld_s)
        dev_inv_s = rec['factor_s'] + rec['inverse_s']
        rec['device_factor_inverse_speedup_over_scipy'] = rec['scipy_factor_inverse_s'] / dev_inv_s
        del Kinv, cf
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='3054,15789,20000,40000')
    ap.add_argument('--no-host', action='store_true')
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'exact_probe.py measures the GPU: no GPU visible'
    from runlmc_amd import _lib
    assert _lib.get_library().is_hip
    run(3054, host=False)          # warm-up: code objects, allocator, rocSOLVER's first call
    for n in [int(v) for v in a.sizes.split(',')]:
        print(json.dumps(run(n, host=not a.no_host)), flush=True)


if __name__ == '__main__':
    main()
