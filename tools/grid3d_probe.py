"""Measurements behind profiles/grid3d/README.md (MI355X only; no CPU fallback).

    python tools/grid3d_probe.py products [--k 8] [--reps 7] [--inner 3]
        one product of --k vectors with D = 1 on the 3-D grids 16x64x64, 32x128x128 and
        64x256x256 through the 3-D handle (k_lead_fwd, one 2-D product per leading frequency,
        k_lead_inv).  2 warm-ups, then --reps samples of --inner products each; median and range
        per product, the workspace bytes per vector, and the seconds of one parameter update
        (rl_gridop_set_lmc: the F Q cosine rows on the host and F child updates).
    python tools/grid3d_probe.py bttb [--k 8] [--reps 3] [--shapes 16x64x64,32x128x128]
        the same product through linalg.BTTB (host vectors in and out, m0^2 slab products per
        vector), and the largest difference from the 3-D handle's result.
    python tools/grid3d_probe.py trace --shape 32x128x128 [--k 8] [--products 5]
        a few products of one shape and nothing else: the command to put behind
        rocprofv3 --kernel-trace --stats, whose per-kernel sums split a product into
        k_lead_fwd, the children's kernels and k_lead_inv.
    python tools/grid3d_probe.py step [--n1 33334] [--reps 3]
        one NLL + gradient step (InterpolatedLLGP.parameters_changed) of a D = 3 model with an
        RBF and a separable kernel over three input dimensions on a 16x64x64 grid, n = 3 n1.

One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

SHAPES = ((16, 64, 64), (32, 128, 128), (64, 256, 256))


def top_row(sizes):
    """An anisotropic, non-separable stationary row on the unit cube's grid."""
    ax = [np.linspace(0, 1, s) for s in sizes]
    d0, d1, d2 = np.meshgrid(*ax, indexing='ij')
    r2 = 9.0 * d0 ** 2 + 25.0 * d1 ** 2 + 49.0 * d2 ** 2 + 6.0 * d0 * d1
    return (np.exp(-r2) + 0.3 * np.exp(-np.sqrt(r2 + 1e-12))).reshape(1, -1)


def handle(sizes):
    from runlmc_amd._native import GridOp
    m = int(np.prod(sizes))
    g = GridOp(1, m, 1, sizes=sizes)
    top = top_row(sizes)
    g.set_lmc(top, [None], [np.ones(1)])
    return g, top


def vectors(g, k):
    gen = torch.Generator(device=g.device).manual_seed(1)
    return torch.randn((k, g.width), dtype=torch.float64, device=g.device, generator=gen)


def timed(g, X, Y, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        g.mvm(X, out=Y)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def parse_shapes(text):
    return [tuple(int(v) for v in s.split('x')) for s in text.split(',')]


def products(a):
    for sizes in parse_shapes(a.shapes):
        g, top = handle(sizes)
        X = vectors(g, a.k)
        Y = torch.empty_like(X)
        for _ in range(2):
            timed(g, X, Y, 1)
        ts = [timed(g, X, Y, a.inner) for _ in range(a.reps)]
        t0 = time.perf_counter()
        g.set_lmc(top, [None], [np.ones(1)])
        torch.cuda.synchronize()
        t_set = time.perf_counter() - t0
        inner_pts = sizes[1] * sizes[2]
        print(json.dumps(dict(what='product', shape=list(sizes), k=a.k, N0=g.N0, F=g.F,
                              inner=[g.L, g.N1, g.N2], seconds=float(np.median(ts)),
                              range=[min(ts), max(ts)], set_lmc_seconds=t_set,
                              workspace_bytes_per_vector=2 * g.F * 2 * g.D * inner_pts * 8,
                              vector_bytes=g.width * 8,
                              device=torch.cuda.get_device_name(0))), flush=True)
        del g, X, Y


def bttb(a):
    from runlmc_amd.linalg.bttb import BTTB
    for sizes in parse_shapes(a.shapes):
        g, top = handle(sizes)
        X = vectors(g, a.k)
        want = g.mvm(X).cpu().numpy()
        op = BTTB(top[0], sizes)
        Xh = np.ascontiguousarray(X.cpu().numpy().T)
        got = op.matmat(Xh)                                # warm-up: creates the 2-D handles
        err = float(np.abs(got.T - want).max() / np.abs(want).max())
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            op.matmat(Xh)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        print(json.dumps(dict(what='bttb', shape=list(sizes), k=a.k, seconds=float(np.median(ts)),
                              range=[min(ts), max(ts)], difference_from_3d_handle=err)), flush=True)
        del g, op


def trace(a):
    sizes = parse_shapes(a.shape)[0]
    g, _ = handle(sizes)
    X = vectors(g, a.k)
    Y = torch.empty_like(X)
    for _ in range(a.products):
        g.mvm(X, out=Y)
    torch.cuda.synchronize()
    print(json.dumps(dict(what='trace', shape=list(sizes), k=a.k, products=a.products, N0=g.N0, F=g.F)),
          flush=True)


def step(a):
    from runlmc_amd.kern import RBF, Matern32, Separable
    from runlmc_amd.lmc.functional_kernel import FunctionalKernel
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    D, n1 = 3, a.n1
    rng = np.random.RandomState(7)
    Xs = [rng.rand(n1, 3) for _ in range(D)]
    lat = lambda x: np.sin(5 * x[:, 0]) * np.cos(7 * x[:, 1]) + 0.5 * np.sin(11 * x[:, 2] + 1)
    Ys = [c * lat(x) + 0.3 * np.cos(9 * x[:, 1] + d) + 0.1 * rng.randn(n1)
          for d, (x, c) in enumerate(zip(Xs, (1.0, -0.7, 0.4)))]
    ks = [RBF(8.0, active_dims=[0, 1, 2]),
          Separable(RBF(4.0, active_dims=[0]), Matern32(6.0, active_dims=[1]), RBF(10.0, active_dims=[2]))]
    fk = FunctionalKernel(D=D, lmc_kernels=ks, lmc_ranks=[1, 1])
    # m counts the points inside the data's range; the grid adds two cells on either side
    lmc = InterpolatedLLGP(Xs, Ys, functional_kernel=fk, normalize=True, m=[12, 60, 60])

    def one():
        np.random.seed(11)                              # the same probes every step
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lmc.parameters_changed()
        g = lmc.gradient
        torch.cuda.synchronize()
        return time.perf_counter() - t0, g

    one()                                               # warm-up: creates the handles
    ts, g = [], None
    for _ in range(a.reps):
        t, g = one()
        ts.append(t)
    grid = [len(ax) for ax in lmc.grid_axes[(0, 1, 2)]]
    print(json.dumps(dict(what='step', n=D * n1, grid=grid, seconds=float(np.median(ts)),
                          range=[min(ts), max(ts)], nll=float(-lmc.log_likelihood()),
                          grad_max=float(np.abs(g).max()))), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('what', choices=('products', 'bttb', 'trace', 'step'))
    p.add_argument('--k', type=int, default=8)
    p.add_argument('--reps', type=int, default=None)
    p.add_argument('--inner', type=int, default=3)
    p.add_argument('--shapes', default=None)
    p.add_argument('--shape', default='32x128x128')
    p.add_argument('--products', type=int, default=5)
    p.add_argument('--n1', type=int, default=33334)
    a = p.parse_args()
    if a.reps is None:
        a.reps = 7 if a.what == 'products' else 3
    if a.shapes is None:
        a.shapes = ','.join('x'.join(str(v) for v in s) for s in (SHAPES if a.what == 'products' else SHAPES[:2]))
    if not torch.cuda.is_available():
        sys.exit('grid3d_probe needs the GPU')
    dict(products=products, bttb=bttb, trace=trace, step=step)[a.what](a)


if __name__ == '__main__':
    main()
