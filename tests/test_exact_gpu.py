"""GPU run of the exact dense likelihood (tests/exact_suite.py on librunlmc_hip.so: the
matrix-core bodies of k_ex_gemm) and its checks at sizes of many panels: FX2007 (n = 3 054),
weather (n = 15 789) and C2 (n = 20 000) against SciPy / the oracle's dense twin."""
import numpy as np
import pytest
import scipy.linalg as la
import torch

import exact_suite as es
import parity_suite as ps
from cases import Case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_library():
    from runlmc_amd import _lib
    _lib.use_library(None)
    lib = _lib.get_library()
    assert lib.is_hip, 'GPU tests must run against librunlmc_hip.so'
    return lib


def test_golden_small():
    es.check_golden_small()


def test_deterministic():
    es.check_deterministic()


@pytest.mark.parametrize('n,D', [(1, 1), (17, 1), (17, 3), (64, 3), (65, 1), (129, 3), (200, 3),
                                 (1000, 3)])
def test_tile_edges(n, D):
    es.check_tile_edges(n, D)


def test_2d_inputs():
    es.check_2d()


def test_split_active_dims():
    es.check_split()


def test_not_positive_definite():
    es.check_not_positive_definite()


def test_errors():
    es.check_errors()


@pytest.mark.parametrize('name', ['lmc_small', 'lmc_2d'])
def test_model_exact_prediction(name):
    es.check_model_exact_prediction(name)


def test_model_metrics():
    es.check_model_metrics()


def test_model_metrics_declined():
    es.check_model_metrics_declined()


def _host_reference(spec, Xs, y, D):
    """log det, alpha and the four gradient families of the exact likelihood on the host
    (SciPy's Cholesky, K^-1 by cho_solve, the reference's identity dL/dt = 1/2 sum M dK with
    M = alpha alpha^T - K^-1), one n x n array at a time; also the 1-norm condition number."""
    from threadpoolctl import threadpool_limits
    lens = [len(x) for x in Xs]
    x = np.concatenate([np.ravel(v) for v in Xs])
    n = len(x)
    ends = np.cumsum(lens)
    begins = ends - np.asarray(lens)
    o = np.repeat(np.arange(D), lens)
    dist = np.abs(x[:, None] - x[None, :])
    K = np.zeros((n, n))
    for B, k in zip(spec.coreg_mats(), spec._kernels):
        K += B[np.ix_(o, o)] * k.from_dist(dist)
    K[np.diag_indices(n)] += np.repeat(spec.noise, lens)
    norm1 = np.abs(K).sum(axis=0).max()
    with threadpool_limits(limits=16):
        cf = la.cho_factor(K, lower=True, overwrite_a=True)
        logdet = 2.0 * np.log(np.diag(cf[0])).sum()
        alpha = la.cho_solve(cf, y)
        M = la.cho_solve(cf, np.identity(n), overwrite_b=True)
    del K, cf
    cond = norm1 * np.abs(M).sum(axis=0).max()
    M *= -1
    M += np.outer(alpha, alpha)

    def block_sums(Kq):
        P = M * Kq
        return np.array([[P[begins[a]:ends[a], begins[b]:ends[b]].sum() for b in range(D)]
                         for a in range(D)])

    g = dict(coreg_vec=[], coreg_diag=[], kernel=[], noise=None)
    for q, (a_q, B, k) in enumerate(zip(spec.coreg_vecs, spec.coreg_mats(), spec._kernels)):
        S = block_sums(k.from_dist(dist))
        g['coreg_vec'].append(0.5 * np.atleast_2d(a_q).dot(S + S.T))
        g['coreg_diag'].append(0.5 * np.diag(S).copy())
        g['kernel'].append([0.5 * np.sum(B * block_sums(dk)) for dk in k.kernel_gradient(dist)])
    g['noise'] = np.array([0.5 * np.trace(M[b:e, b:e]) for b, e in zip(begins, ends)])
    return logdet, alpha, g, cond


@pytest.mark.parametrize('name', ['fx2007', 'weather'])
def test_dataset_against_host(name):
    """Many panels (48 at FX2007, 247 at weather) against the host's dense Cholesky and the
    reference's gradient identity: alpha, log det and the four gradient families at 1e-9, loosened
    only by the fixture's own 1-norm condition number (printed): rounding of an O(n^3)
    factorisation grows with it on either side."""
    from runlmc_amd.lmc import ExactLMCLikelihood
    c = Case(name)
    fk = ps.functional_kernel_for(c)
    lik = ExactLMCLikelihood(fk, c.Xs, c.Ys)
    ld, alpha, g, cond = _host_reference(c.spec(), c.Xs, c.y, c.D)
    rtol = max(1e-9, 1e-16 * cond)
    print('%s: n = %d, 1-norm condition number %.3e, tolerance %.1e' % (name, c.n, cond, rtol))
    assert abs(lik.log_det_K() - ld) <= 1e-9 * abs(ld), (lik.log_det_K(), ld)
    es._close(lik.alpha(), alpha, rtol, 'alpha')
    vec, diag, kern, noise = es._grads_flat(lik, c.Q)
    for q in range(c.Q):
        es._close(vec[q], g['coreg_vec'][q], rtol, 'coreg_vec %d' % q)
        es._close(diag[q], g['coreg_diag'][q], rtol, 'coreg_diag %d' % q)
        es._close(kern[q], g['kernel'][q], rtol, 'kernel %d' % q)
    es._close(noise, g['noise'], rtol, 'noise')


def test_c2_against_host_cholesky():
    """C2 (n = 20 000, 313 panels): log det and alpha against SciPy's Cholesky of the same
    matrix, as test_gpu_full_size.py: test_c2_direct_solve_vs_dense_oracle does for K~."""
    from threadpoolctl import threadpool_limits
    from runlmc_amd._native import ExactOp
    from runlmc_amd.util import synth
    D, Q, R, m0, _ = synth.CONFIGS['c2']
    p = synth.make_problem(D, Q, R, m0)
    fk = synth.functional_kernel(p)
    op = ExactOp(p.n, 1)
    op.set(np.vstack(p.Xs), p.lens, fk.kernels, fk.coreg_mats(), p.noise)
    K = op.dense()
    logdet = op.factor()
    alpha = op.solve(torch.from_numpy(p.y).to(op.device)).cpu().numpy()
    with threadpool_limits(limits=16):
        cf = la.cho_factor(K, lower=True, overwrite_a=True)
        ld = 2.0 * np.log(np.diag(cf[0])).sum()
        aref = la.cho_solve(cf, p.y)
    assert abs(logdet - ld) <= 1e-10 * abs(ld), (logdet, ld)
    es._close(alpha, aref, 1e-8, 'alpha')
