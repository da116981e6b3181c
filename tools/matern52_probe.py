"""Measurements behind profiles/matern52/README.md (MI355X only; no CPU fallback).

    python tools/matern52_probe.py products [--D 10] [--m 100000] [--k 129] [--reps 5] [--inner 4]
        single-top products of the d/dgamma rows of Matern-5/2 (four filter states) and of
        Matern-3/2 (three: the control) at gamma = 1 and 10, in the recursive-filter form and on
        the transform kernels (a second handle created under RUNLMC_NO_FILTER=1: what a build
        without degree-3 rows runs for the Matern-5/2 row).  2 warm-ups, then --reps samples of
        --inner products each, the two handles alternating; median and range per product, and
        the largest difference between the two handles' results.
    python tools/matern52_probe.py trace [--D 10] [--m 100000] [--k 129]
        a few filter-form products of both rows and nothing else: the command to put behind
        rocprofv3 --kernel-trace --stats.
    python tools/matern52_probe.py step [--n1 100000] [--reps 3]
        one NLL + gradient step (InterpolatedLLGP.parameters_changed) of a D = 3 model with two
        Matern-5/2 kernels, n = 3 n1, the gradient's handle with and without the filter form.

One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('RUNLMC_DEBUG', '1')          # the library reads RUNLMC_NO_FILTER only under it
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def dk52(x, g):
    s = np.sqrt(5.0) * g * x
    return -(5.0 * g * x * x / 3.0) * (1.0 + s) * np.exp(-s)


def dk32(x, g):
    return -3.0 * g * x * x * np.exp(-np.sqrt(3.0) * g * x)


ROWS = (('dk52 gamma 1', dk52, 1.0), ('dk52 gamma 10', dk52, 10.0),
        ('dk32 gamma 1', dk32, 1.0), ('dk32 gamma 10', dk32, 10.0))


def handles(D, m, filter_only=False):
    from runlmc_amd._native import GridOp
    x = np.linspace(0, 1, m)
    tops = np.array([f(x, g) for _, f, g in ROWS])
    out = []
    for no_filter in ((False,) if filter_only else (False, True)):
        if no_filter:
            os.environ['RUNLMC_NO_FILTER'] = '1'
        try:
            g = GridOp(D, m, len(ROWS))
            g.set_lmc(tops, [None] * len(ROWS), [np.zeros(D)] * len(ROWS))
        finally:
            os.environ.pop('RUNLMC_NO_FILTER', None)
        out.append(g)
    return out


def timed(g, top, X, Y, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        g.mvm(X, out=Y, top=top)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def products(a):
    gf, gt = handles(a.D, a.m)
    dev = gf.device
    gen = torch.Generator(device=dev).manual_seed(1)
    X = torch.randn((a.k, a.D * a.m), dtype=torch.float64, device=dev, generator=gen)
    Yf, Yt = torch.empty_like(X), torch.empty_like(X)
    for g, Y in ((gf, Yf), (gt, Yt)):
        for t in range(len(ROWS)):
            g.mvm(X, out=Y, top=t)                   # (runs the pending verification of the forms)
    print(json.dumps(dict(what='forms', filter=gf.top_forms()[0], no_filter=gt.top_forms()[0],
                          D=a.D, m=a.m, k=a.k, device=torch.cuda.get_device_name(0))), flush=True)
    for t, (name, _, _) in enumerate(ROWS):
        for _ in range(2):
            timed(gf, t, X, Yf, a.inner)
            timed(gt, t, X, Yt, a.inner)
        sf, st = [], []
        for _ in range(a.reps):
            sf.append(timed(gf, t, X, Yf, a.inner))
            st.append(timed(gt, t, X, Yt, a.inner))
        diff = float((Yf - Yt).abs().max() / Yt.abs().max())
        print(json.dumps(dict(
            what='product', row=name, filter_ms=1e3 * float(np.median(sf)),
            filter_range_ms=[1e3 * min(sf), 1e3 * max(sf)],
            transform_ms=1e3 * float(np.median(st)),
            transform_range_ms=[1e3 * min(st), 1e3 * max(st)],
            speedup=float(np.median(st) / np.median(sf)), rel_diff=diff)), flush=True)


def trace(a):
    (gf,) = handles(a.D, a.m, filter_only=True)
    X = torch.randn((a.k, a.D * a.m), dtype=torch.float64, device=gf.device)
    Y = torch.empty_like(X)
    for t in (0, 2):                                   # dk52 (NS = 4), dk32 (NS = 3) at gamma 1
        for _ in range(4):
            gf.mvm(X, out=Y, top=t)
    torch.cuda.synchronize()
    print(json.dumps(dict(what='trace', forms=gf.top_forms()[0])), flush=True)


def step(a):
    from runlmc_amd.kern.stationary import Matern52
    from runlmc_amd.lmc import likelihood
    from runlmc_amd.lmc.functional_kernel import FunctionalKernel
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    D, n1 = 3, a.n1
    rng = np.random.RandomState(7)
    xss = [np.sort(rng.rand(n1)) for _ in range(D)]
    lat = lambda x: np.sin(9 * x) + 0.5 * np.sin(31 * x + 1) + 0.2 * np.abs(np.sin(57 * x))
    yss = [c * lat(x) + 0.3 * np.cos(13 * x + d) + 0.1 * rng.randn(n1)
           for d, (x, c) in enumerate(zip(xss, (1.0, -0.7, 0.4)))]
    ks = [Matern52(inv_lengthscale=3.0, name='m0'), Matern52(inv_lengthscale=20.0, name='m1')]
    fk = FunctionalKernel(D=D, lmc_kernels=ks, lmc_ranks=[1, 1])
    lmc = InterpolatedLLGP(xss, yss, functional_kernel=fk, normalize=True, m=n1 // 5)

    def one():
        np.random.seed(11)                              # the same probes every step
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lmc.parameters_changed()
        g = lmc.gradient
        torch.cuda.synchronize()
        return time.perf_counter() - t0, g

    for no_filter in (False, True):
        likelihood._GRAD_OPS.clear()                    # the gradient's handle is created anew
        if no_filter:
            os.environ['RUNLMC_NO_FILTER'] = '1'
        try:
            one()                                       # warm-up: creates the handle
        finally:
            os.environ.pop('RUNLMC_NO_FILTER', None)
        ts, g = [], None
        for _ in range(a.reps):
            t, g = one()
            ts.append(t)
        forms = [op.top_forms()[0] for op in likelihood._GRAD_OPS.values()]
        print(json.dumps(dict(what='step', n=D * n1, grid=n1 // 5, gradient_no_filter=no_filter,
                              gradient_forms=forms, seconds=float(np.median(ts)),
                              range=[min(ts), max(ts)], grad_max=float(np.abs(g).max()))),
              flush=True)


if __name__ == '__main__':
    p = argparse.ArgumentParser()
    p.add_argument('mode', choices=('products', 'trace', 'step'))
    p.add_argument('--D', type=int, default=10)
    p.add_argument('--m', type=int, default=100000)
    p.add_argument('--k', type=int, default=129)
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--inner', type=int, default=4)
    p.add_argument('--n1', type=int, default=100000)
    a = p.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    from runlmc_amd import _lib
    assert _lib.get_library().is_hip
    {'products': products, 'trace': trace, 'step': step}[a.mode](a)
