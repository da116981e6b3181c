"""Measurements of the pivoted-Cholesky preconditioner (csrc/rl_pivchol.h) on the device; the
results and their reading are in profiles/pivchol/README.md.

    python tools/pivchol_probe.py --grid 512 512 --n 1000000 --D 4 --ranks 32 64 128
    python tools/pivchol_probe.py --grid 64 256 256 --n 1000000 --D 2 --ranks 32 64 128

Per rank: the build (host clock around rl_ski_factor, split by rl_ski_pivchol_build_ms into
diagonal / k products with their step kernels / Gram matrix and host maps), one application to
--nvec vectors (device events, median of --reps after two warm-up runs) with the share of the
measured copy bandwidth it reaches against the model 8 n (k + 2 nvec) bytes, and a solve of
--nrhs systems (y and +-1 rows) to the reference's rule ||b - K~ x|| < --tol with the
preconditioner and (--plain) without it: iterations, worst residual, seconds.  One JSON line per
measurement on stdout.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from runlmc_amd.kern import RBF, Matern32, Separable                      # noqa: E402
from runlmc_amd.lmc.functional_kernel import FunctionalKernel             # noqa: E402
from runlmc_amd.lmc.grid_kernel import gen_grid_kernel                    # noqa: E402
from runlmc_amd.approx.interpolation import multi_interpolant            # noqa: E402
from runlmc_amd.approx.iterative import Iterative                         # noqa: E402
from runlmc_amd.kern.stationary import Lags                               # noqa: E402


def kernels(ndim, scale):
    """Three latent kernels over all the input dimensions: an ARD RBF, an RBF x Matern-3/2
    separable product and an isotropic Matern-3/2, inverse length scales `scale` apart."""
    dims = list(range(ndim))
    sep = Separable(RBF(scale, active_dims=dims[:1]), Matern32(np.sqrt(scale), active_dims=dims[1:]))
    return [RBF.ard([scale * (1.0 + 0.5 * i) for i in dims], dims), sep, Matern32(2.0 * np.sqrt(scale), active_dims=dims)]


def build(args):
    rng = np.random.RandomState(args.seed)
    ndim, D = len(args.grid), args.D
    lens = [args.n // D + (1 if d < args.n % D else 0) for d in range(D)]
    Xs = [rng.rand(l, ndim) for l in lens]
    axes = [np.linspace(-2.0 / m, 1.0 + 2.0 / m, m) for m in args.grid]
    kerns = kernels(ndim, args.scale)
    fk = FunctionalKernel(D=D, lmc_kernels=kerns, lmc_ranks=[1] * len(kerns))
    fk.coreg_vecs = [rng.uniform(-1, 1, size=(1, D)) for _ in kerns]
    fk.coreg_diags = [0.2 + rng.rand(D) for _ in kerns]
    fk.noise = np.full(D, args.noise)
    fk.set_input_dim(ndim)
    W = multi_interpolant(Xs, *axes)
    mesh = np.meshgrid(*[a - a[0] for a in axes], indexing='ij')
    ad = tuple(range(ndim))
    lags = Lags(mesh, np.sqrt(sum(g ** 2 for g in mesh)))
    K, _ = gen_grid_kernel(fk, {ad: lags}, {ad: (W, W.T.tocsr())}, lens)
    y = np.concatenate([np.sin(4 * X[:, 0]) * np.cos(5 * X[:, -1]) + 0.1 * rng.randn(len(X)) for X in Xs])
    return K, y


def sync():
    torch.cuda.synchronize()


def timed(fn, reps):
    fn()
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        sync()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, nargs='+', default=[512, 512])
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--D', type=int, default=4)
    ap.add_argument('--ranks', type=int, nargs='+', default=[32, 64, 128])
    ap.add_argument('--nvec', type=int, default=129)
    ap.add_argument('--nrhs', type=int, default=17)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--tol', type=float, default=1e-4)
    ap.add_argument('--noise', type=float, default=1e-2)
    ap.add_argument('--scale', type=float, default=30.0)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--plain', action='store_true', help='also the solve without the preconditioner')
    ap.add_argument('--maxiter', type=int, default=2000)
    args = ap.parse_args()
    t0 = time.time()
    K, y = build(args)
    ski = K.device_operator()
    n, dev = ski.n, ski.device
    base = dict(grid=args.grid, n=n, D=args.D, noise=args.noise)
    print(json.dumps(dict(base, what='setup', seconds=time.time() - t0)), flush=True)
    rng = np.random.RandomState(2)
    B = torch.from_numpy(rng.randn(args.nvec, n)).to(dev)
    rhs = np.vstack([y] + [rng.randint(0, 2, n) * 2.0 - 1.0 for _ in range(args.nrhs - 1)])
    R = torch.from_numpy(rhs).to(dev)
    # copy bandwidth at the apply's size: one read and one write of the batch
    dst = torch.empty_like(B)
    ms = timed(lambda: dst.copy_(B), args.reps)
    copy_bw = 2.0 * B.numel() * 8 / (ms * 1e-3)
    print(json.dumps(dict(base, what='copy', ms=ms, GBps=copy_bw / 1e9)), flush=True)
    ms1 = timed(lambda: ski.mvm(B[:1]), args.reps)
    print(json.dumps(dict(base, what='product of one vector', ms=ms1)), flush=True)
    from runlmc_amd._native import solve_batch, CG
    if args.plain:
        sync()
        t = time.time()
        X, it, res, st = solve_batch(ski, R, CG, tol=args.tol, check_every=100, maxiter=args.maxiter)
        sync()
        print(json.dumps(dict(base, what='solve, no preconditioner (CG)', seconds=time.time() - t,
                              iterations=int(np.max(it)), worst_residual=float(np.max(res)),
                              met_rule=int(np.sum(np.asarray(res) < args.tol)), systems=len(res))), flush=True)
    split = (ctypes.c_double * 3)()
    for rank in args.ranks:
        ski.set_pivchol(rank)
        sync()
        t = time.time()
        ok, _, cond = ski.factor()
        sync()
        build_s = time.time() - t
        assert ok and ski.factor_mode == 4, ski.factor_reason
        ski.lib.call('rl_ski_pivchol_build_ms', ski.handle, split)
        used = ski.pivchol_info()[0]
        print(json.dumps(dict(base, what='build', rank=rank, rank_used=used, seconds=build_s, cond=cond,
                              diag_ms=split[0], products_and_steps_ms=split[1], gram_host_ms=split[2])), flush=True)
        ms = timed(lambda: ski.precond_apply(B), args.reps)
        model = 8.0 * n * (rank + 2 * args.nvec)
        print(json.dumps(dict(base, what='apply', rank=rank, nvec=args.nvec, ms=ms, model_GB=model / 1e9,
                              share_of_copy=model / (ms * 1e-3) / copy_bw)), flush=True)
        sync()
        t = time.time()
        X, it, res, st = Iterative.solve_device(K, R, tol=args.tol, maxiter=args.maxiter)
        sync()
        print(json.dumps(dict(base, what='solve, preconditioned', rank=rank, seconds=time.time() - t,
                              iterations=int(np.max(it)), worst_residual=float(np.max(res)),
                              met_rule=int(np.sum(np.asarray(res) < args.tol)), systems=len(res))), flush=True)
    ski.set_pivchol(0)


if __name__ == '__main__':
    main()
