"""Device memory comes back: six create -> product -> solve -> destroy cycles of a small operator in
one process, free device memory read after the first and after the last.  The assertion is on
the growth between the two -- the runtime keeps memory of its own after first use, so the
absolute baseline says nothing.  The bound is what the commit before the handles owned their
buffers (DevBuf, csrc/rl_host.h) showed with this same file on one MI355X: no growth."""
import gc

import numpy as np
import pytest
import scipy.sparse as sp
import torch

# growth in bytes between cycle 1 and cycle 6 measured on the parent commit (profiles/devbuf/README.md)
PARENT_GROWTH = 0

D, N, NRHS = 2, 600, 17


def _interp(n, m):
    """Cubic-convolution W (n x D m): outputs one after another, rows sorted within an output."""
    per = n // D
    k = np.arange(n) % per
    d = np.arange(n) // per
    x = 1.0 + (k + 0.37) / per * (m - 3.0)
    b = np.minimum(x.astype(int) - 1, m - 4)
    s = x - (b + 1)
    w = np.stack([((-0.5 * s + 1.0) * s - 0.5) * s, (1.5 * s - 2.5) * s * s + 1.0,
                  ((-1.5 * s + 2.0) * s + 0.5) * s, (0.5 * s - 0.5) * s * s], axis=1)
    cols = (d * m + b)[:, None] + np.arange(4)[None, :]
    W = sp.csr_matrix((w.ravel(), cols.ravel(), 4 * np.arange(n + 1)), shape=(n, D * m))
    return W, W.T.tocsr()


def _tops(m, rough):
    t = np.linspace(0.0, 1.0, m)
    if rough:
        r = np.sqrt(3.0) * t / 0.004
        return np.array([(1.0 + r) * np.exp(-r)])
    return np.array([np.exp(-0.5 * (t / 0.8) ** 2), np.exp(-t / 0.3)])


def _cycle(k, X):
    from runlmc_amd._native import GridOp, SkiOp, solve_batch, solve_pcg
    m = 256
    tops = _tops(m, rough=k == 3)
    B = np.array([np.eye(D) * (1.0 + 0.1 * q) + 0.3 * (1 - np.eye(D)) for q in range(len(tops))])
    g = GridOp(D, m, 2)
    g.set_dense(tops, B)
    s = SkiOp(g, *_interp(N, m))
    s.set_noise(np.array([0.1, 0.2]), np.array([N // D, N // D]))
    if k == 2:                                  # a second term on a longer grid
        g2 = GridOp(D, 320, 1)
        g2.set_dense(_tops(320, rough=True), B[:1])
        s.add_term(g2, *_interp(N, 320))
    Y = s.mvm(X)
    if k == 3:                                  # the pivoted-Cholesky preconditioner
        s.set_pivchol(8)
        assert s.factor()[0] and s.factor_mode == 4
        Z = solve_pcg(s, X, tol=1e-6, maxiter=60)[0]
    else:
        Z = solve_batch(s, X, tol=1e-6, check_every=20, maxiter=60)[0]
    assert bool(torch.isfinite(Y).all()) and bool(torch.isfinite(Z).all())
    del s, g, Y, Z
    gc.collect()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


@pytest.mark.gpu
def test_device_memory_returns_after_destroy():
    rng = np.random.RandomState(5)
    X = torch.from_numpy(rng.randn(NRHS, N)).cuda()
    before = torch.cuda.mem_get_info()[0]
    free = [_cycle(k, X) for k in range(1, 7)]
    growth = free[0] - free[-1]
    print('free device memory before: %d, after each cycle: %s, growth cycle 1 -> 6: %d bytes'
          % (before, free, growth))
    assert growth <= PARENT_GROWTH
