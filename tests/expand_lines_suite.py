"""Checks of the polynomial form's expansion with whole-line stores (csrc/rl_lowrank.h:
k_lr_expand_lines), shared by the CPU run on the emulator build (tests/test_expand_lines_emu.py)
and the GPU run (tests/test_expand_lines_gpu.py).  Everything goes through GridOp: the batch gate
lifted (set_form_gate(0)), the product written into a caller's tensor (mvm(X, out=Y), top=).

What is held against what:
  * the product with the new store mapping against the product of a handle created under
    RUNLMC_LR_EXPAND_PLAIN=1 (k_lr_expand whatever the row length): BIT FOR BIT -- the arithmetic
    per element is the same, only the thread that stores an element differs.  The RBF handles
    take the library's default (k_lr_expand_lines at rank 24); ranks >= 36 and the accumulating
    expansion keep k_lr_expand by default, so their handles are created under
    RUNLMC_LR_EXPAND_PLAIN=3, which launches k_lr_expand_lines for them too;
  * the product against the transform kernels of the same handle (gate at 2^60) at the project's
    1e-12 of the result's largest entry, as parity_suite.check_polynomial_form does;
  * Y is a view at 0, 1, 5 and 12 doubles into a larger buffer filled with a sentinel: after the
    product every element outside the view still holds it (first / last block overruns).
Shapes: the smallest at which the mapping can go wrong -- row lengths with periods 1 (96), 4 (100,
500, 2500), 16 (odd lengths: a centre point), slots + phase crossing a multiple of 256 (513:
257 slots; 2047: 1024 slots; 4101), rows k D in {1, 3, 5, 17, 67} (empty classes, ragged last
blocks); an RBF pair (rank 24) and a periodic top of period 0.8 (rank 40 or
48 at every one of these lengths)."""
import contextlib
import os

import numpy as np
import torch

from runlmc_amd._native import GridOp

LENGTHS = (96, 97, 100, 257, 500, 513, 2047, 2500, 4101)
# (D, vectors): rows k D = 1, 17, 67 | 3 | 5
BATCHES = ((1, (1, 17, 67)), (3, (1,)), (5, (1,)))
OFFSETS = (0, 1, 5, 12)
SENTINEL = -7.25e77
PAD = 32


@contextlib.contextmanager
def _env(**kw):
    saved = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _tops(kern, m):
    x = np.linspace(0, 1, m)
    if kern == 'rbf':
        return np.array([np.exp(-0.5 * x ** 2), np.exp(-1.5 * x ** 2)])
    assert kern == 'periodic'
    return np.array([np.exp(-0.5 * x ** 2), np.exp(-0.5 * np.sin(np.pi * x / 0.8) ** 2)])


def _pair(D, m, Q, setter, force=False):
    """(handle with the library's default mapping -- `force`: with k_lr_expand_lines also for the
    instantiations that keep k_lr_expand by default, RUNLMC_LR_EXPAND_PLAIN=3 --, handle with
    k_lr_expand throughout)"""
    if force:
        with _env(RUNLMC_DEBUG='1', RUNLMC_LR_EXPAND_PLAIN='3'):
            g = GridOp(D, m, Q)
            setter(g)
    else:
        g = GridOp(D, m, Q)
        setter(g)
    with _env(RUNLMC_DEBUG='1', RUNLMC_LR_EXPAND_PLAIN='1'):
        gp = GridOp(D, m, Q)
        setter(gp)
    return g, gp


def _product_in_view(g, X, off, top=None):
    """the product above the gate, written into a view `off` doubles into a sentinel buffer"""
    k, w = X.shape
    buf = torch.full((k * w + PAD,), SENTINEL, dtype=torch.float64, device=X.device)
    Y = buf[off:off + k * w].view(k, w)
    g.set_form_gate(0)
    try:
        g.mvm(X, out=Y, top=top)
    finally:
        g.set_form_gate(-1)
    host = buf.cpu().numpy()
    assert np.all(host[:off] == SENTINEL), 'written before the view (offset %d)' % off
    assert np.all(host[off + k * w:] == SENTINEL), 'written past the view (offset %d)' % off
    return host[off:off + k * w].reshape(k, w).copy()


def _transforms(g, X, top=None):
    g.set_form_gate(1 << 60)
    try:
        return g.mvm(X, top=top).cpu().numpy()
    finally:
        g.set_form_gate(-1)


def _close(got, ref, rel):
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)
    assert err < rel, 'relative error %.3e >= %.1e' % (err, rel)


def _check(g, gp, X, top=None):
    ref = _transforms(g, X, top)
    for off in OFFSETS:
        new = _product_in_view(g, X, off, top)
        plain = _product_in_view(gp, X, off, top)
        assert np.array_equal(new, plain), \
            'offset %d: %d elements differ from the plain mapping' % (off, int((new != plain).sum()))
        _close(new, ref, 1e-12)
        assert not np.array_equal(new, ref)      # (it WAS the polynomial form)


def check_products(m, kern):
    """operator and single-top products of every batch shape, every base offset"""
    rng = np.random.RandomState(1000 + m)
    tops = _tops(kern, m)
    for D, counts in BATCHES:
        A = [rng.randn(1, D), rng.randn(2, D)]
        kap = [np.abs(rng.randn(D)) + 0.1 for _ in range(2)]
        g, gp = _pair(D, m, 2, lambda h: h.set_lmc(tops, A, kap), force=kern != 'rbf')
        rank = g.form()[0]
        assert (rank == 24 if kern == 'rbf' else rank >= 36), (kern, m, rank)
        assert gp.form()[0] == rank
        for k in counts:
            X = torch.from_numpy(rng.randn(k, D * m)).to(g.device)
            _check(g, gp, X)
            if k == counts[0]:
                _check(g, gp, X, top=1)


def check_accumulate():
    """the accumulating expansion: the smallest operator of parity_suite.check_filter_form that
    mixes filter and polynomial tops (rbf + periodic + Matern-3/2, D = 3, m = 2500: period 4)"""
    rng = np.random.RandomState(77)
    D, m, k = 3, 2500, 3
    x = np.linspace(0, 1, m)
    s = np.sqrt(3) * x
    mix = np.array([np.exp(-0.5 * x ** 2), np.exp(-0.5 * np.sin(np.pi * x / 3.0) ** 2),
                    (1 + s) * np.exp(-s)])
    A = [rng.randn(1, D) for _ in range(3)]
    kap = [np.abs(rng.randn(D)) + 0.1 for _ in range(3)]
    g, gp = _pair(D, m, 3, lambda h: h.set_lmc(mix, A, kap), force=True)
    assert g.top_forms() == ([1, 1, 2], True)
    X = torch.from_numpy(rng.randn(k, D * m)).to(g.device)
    _check(g, gp, X)
