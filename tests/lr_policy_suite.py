"""Checks of the polynomial form's cache policies and projection depth (csrc/rl_lowrank.h: LrPolicy,
RUNLMC_LR_POLICY), shared by the CPU run on the emulator build (tests/test_lr_policy_emu.py) and
the GPU run (tests/test_lr_policy_gpu.py).  Built like expand_lines_suite.py: everything goes
through GridOp with the batch gate lifted (set_form_gate(0)); the knob is explicit, which also
bypasses the size gate of the library's own choice, so small shapes reach the policy code.

What is held against what:
  * for each value of RUNLMC_LR_POLICY the product of a handle created under it against the product
    of a handle created under RUNLMC_LR_POLICY=0 (no hint, the default depth): BIT FOR BIT -- only
    cache hints and the assignment of rows to waves differ.  The reference product is computed
    ONCE per batch, from contiguous tensors, and every view of every value is held against it;
  * the product against the transform kernels of the same handle (gate at 2^60) at the project's
    1e-12 of the result's largest entry;
  * Y is a view at 0, 1, 5 and 12 doubles into a sentinel-filled buffer: nothing outside the view
    is written;  X is a view at 0 and 1 doubles into a larger buffer: rows that are only 8-byte
    aligned for the policy loads.
On the emulator the hints are no-ops; the projection with two rows per wave and a ring of four
(bit 3) is real code there.
Shapes: the smallest at which this can go wrong -- m = 96 and 97 (one short chunk; 97 has a centre
point), 500 (period 4 of the whole-line expansion), 4101 (2051 slots: two chunks, the second
nearly empty), 9000 (three chunks); rows k D in {1, 3, 5, 17, 67} (row blocks of 8 and of 16 both
ragged, clamped rows past the end).  Rank 24 (an RBF pair) under every policy and depth; a
periodic top (rank >= 36) and the accumulating expansion under the policies only (the depth bit
selects nothing above rank 24)."""
import numpy as np
import torch

import expand_lines_suite as es
from runlmc_amd._native import GridOp

LENGTHS = (96, 97, 500, 4101, 9000)
# (D, vectors): rows k D = 1, 17, 67 | 3 | 5
BATCHES = ((1, (1, 17, 67)), (3, (1,)), (5, (1,)))
# (x offset, y offset) of the two views: every offset of Y and both of X.  Not their cross: the
# offset of X reaches the projection only and the offset of Y the expansion only -- two launches
# with a coefficient buffer of the handle's own between them.
VIEWS = ((0, 0), (1, 1), (0, 5), (1, 12))
# bit 0 nt loads | bits 1-2 stores plain, nt, sc1 | bit 3 two rows per wave, ring of four
POLICIES = (1, 2, 3, 4, 5)
VALUES = POLICIES + tuple(8 + v for v in (0,) + POLICIES)
# the emulator's share.  Hints are no-ops there, so the one piece of new device code is the
# projection's other depth (8), which the offset of X reaches and the offset of Y does not: two
# views; every bit at once (13) checks the launchers' dispatch, at the shortest length only.
EMU_VALUES = (8,)
EMU_VALUES_SHORT = (8, 13)
EMU_POLICIES = (5,)
EMU_VIEWS = ((0, 0), (1, 12))


def _handle(D, m, Q, setter, value, plain=None):
    env = dict(RUNLMC_DEBUG='1', RUNLMC_LR_POLICY=str(value))
    if plain is not None:
        env['RUNLMC_LR_EXPAND_PLAIN'] = str(plain)
    with es._env(**env):
        g = GridOp(D, m, Q)
        setter(g)
    return g


def _product(g, X, xoff, yoff, top=None):
    """the product above the gate: X read from a view `xoff` doubles into a larger buffer, Y
    written into a view `yoff` doubles into a sentinel buffer"""
    k, w = X.shape
    xbuf = torch.full((k * w + es.PAD,), 3.5e66, dtype=torch.float64, device=X.device)
    xv = xbuf[xoff:xoff + k * w].view(k, w)
    xv.copy_(X)
    buf = torch.full((k * w + es.PAD,), es.SENTINEL, dtype=torch.float64, device=X.device)
    Y = buf[yoff:yoff + k * w].view(k, w)
    g.set_form_gate(0)
    try:
        g.mvm(xv, out=Y, top=top)
    finally:
        g.set_form_gate(-1)
    host = buf.cpu().numpy()
    assert np.all(host[:yoff] == es.SENTINEL), 'written before the view (offset %d)' % yoff
    assert np.all(host[yoff + k * w:] == es.SENTINEL), 'written past the view (offset %d)' % yoff
    return host[yoff:yoff + k * w].reshape(k, w).copy()


def _reference(g0, X, top=None, transforms=True):
    """(the product under RUNLMC_LR_POLICY=0, the transform kernels' product): once per batch.
    `transforms` False (the emulator's larger batches, where the transform kernels are most of
    the run): the second is the first -- every product is still held bit for bit against it"""
    plain = _product(g0, X, 0, 0, top)
    if not transforms:
        return plain, plain
    ref = es._transforms(g0, X, top)
    es._close(plain, ref, 1e-12)
    assert not np.array_equal(plain, ref)        # (it WAS the polynomial form)
    return plain, ref


def _check(g, value, X, plain, ref, top=None, views=VIEWS):
    for xoff, yoff in views:
        new = _product(g, X, xoff, yoff, top)
        assert np.array_equal(new, plain), \
            'policy %d, x offset %d, y offset %d: %d elements differ from policy 0' % (
                value, xoff, yoff, int((new != plain).sum()))
    es._close(new, ref, 1e-12)


def check_rbf(m, values=VALUES, views=VIEWS, transforms_all=True):
    """rank 24: operator and single-top products of every batch shape, every policy and depth"""
    rng = np.random.RandomState(2000 + m)
    tops = es._tops('rbf', m)
    for D, counts in BATCHES:
        A = [rng.randn(1, D), rng.randn(2, D)]
        kap = [np.abs(rng.randn(D)) + 0.1 for _ in range(2)]

        def setter(h):
            h.set_lmc(tops, A, kap)
        g0 = _handle(D, m, 2, setter, 0)
        assert g0.form()[0] == 24, (m, g0.form())
        gs = [(v, _handle(D, m, 2, setter, v)) for v in values]
        for k in counts:
            X = torch.from_numpy(rng.randn(k, D * m)).to(g0.device)
            for top in ((None, 1) if k == counts[0] else (None,)):
                plain, ref = _reference(g0, X, top, transforms_all or k == counts[0])
                for v, g in gs:
                    assert g.form()[0] == 24
                    _check(g, v, X, plain, ref, top, views)


def check_periodic(m=500, values=POLICIES):
    """a periodic top (rank >= 36: the plain-pointer loads of the projection, k_lr_expand by
    default and k_lr_expand_lines under RUNLMC_LR_EXPAND_PLAIN=3), the policies only"""
    rng = np.random.RandomState(3000 + m)
    tops = es._tops('periodic', m)
    D = 1
    A = [rng.randn(1, D), rng.randn(2, D)]
    kap = [np.abs(rng.randn(D)) + 0.1 for _ in range(2)]

    def setter(h):
        h.set_lmc(tops, A, kap)
    g0 = _handle(D, m, 2, setter, 0)
    rank = g0.form()[0]
    assert rank >= 36, rank
    Xs = [torch.from_numpy(rng.randn(k, D * m)).to(g0.device) for k in (1, 17)]
    refs = [_reference(g0, X) for X in Xs]
    top_ref = _reference(g0, Xs[0], 1)
    for plain_knob in (None, 3):
        for v in values:
            g = _handle(D, m, 2, setter, v, plain_knob)
            assert g.form()[0] == rank
            for X, (plain, ref) in zip(Xs, refs):
                _check(g, v, X, plain, ref)
            _check(g, v, Xs[0], top_ref[0], top_ref[1], top=1)


def check_accumulate(values=POLICIES):
    """the accumulating expansion: the operator of expand_lines_suite.check_accumulate (rbf +
    periodic + Matern-3/2, D = 3, m = 2500), the policies only; the read of Y stays plain"""
    rng = np.random.RandomState(77)
    D, m, k = 3, 2500, 3
    x = np.linspace(0, 1, m)
    s = np.sqrt(3) * x
    mix = np.array([np.exp(-0.5 * x ** 2), np.exp(-0.5 * np.sin(np.pi * x / 3.0) ** 2),
                    (1 + s) * np.exp(-s)])
    A = [rng.randn(1, D) for _ in range(3)]
    kap = [np.abs(rng.randn(D)) + 0.1 for _ in range(3)]

    def setter(h):
        h.set_lmc(mix, A, kap)
    g0 = _handle(D, m, 3, setter, 0)
    assert g0.top_forms() == ([1, 1, 2], True)
    X = torch.from_numpy(rng.randn(k, D * m)).to(g0.device)
    plain, ref = _reference(g0, X)
    for plain_knob in (None, 3):
        for v in values:
            g = _handle(D, m, 3, setter, v, plain_knob)
            assert g.top_forms() == ([1, 1, 2], True)
            _check(g, v, X, plain, ref)
