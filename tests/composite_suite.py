"""Checks of composite kernels (runlmc_amd.kern: Cosine, Product) through every layer: the host
classes, the grid products of their rows, the exact dense likelihood's factor-list evaluator
(csrc/rl_exact.h: ex_eval_fact, rl_exact_set_factors), the model, leave-one-out and function
draws.  Shared by the CPU run on the emulator (tests/test_composite_emu.py) and the GPU run
(tests/test_composite_gpu.py); every function uses whichever native library is active.

The oracle has no composite kernels, so the yardsticks are written here from the closed forms
(CosineSpec, ProductSpec: the duck-typed surface oracle.kernels.KernelSpec consumes) on top of the
oracle's leaf specifications and matern52_suite.Matern52Spec:
    cos:      k(r) = cos(2 pi f r),             dk / df = -2 pi r sin(2 pi f r);
    product:  k(r) = prod_f k_f(r),             dk / dtheta_{f,p} = dk_f / dtheta_p prod_{g != f} k_g,
parameters in the order of the factors, each factor's in its own order; a scale outside, last.

Inputs of more than one dimension: exp(-g sin^2(pi |r| / T) / 2) and cos(2 pi f |r|) of a
EUCLIDEAN norm are positive definite functions on the line only (a product with them is indefinite
on scattered points of the plane, whatever the noise of this suite), so the 2-D case of the exact
likelihood puts every product that has such a factor on ONE input column (active_dims), alternating
between the two; the plain Matern-5/2 keeps both columns."""
import functools

import numpy as np
import scipy.linalg as la

from oracle import operators as ops
from oracle import likelihood as olik
from oracle.kernels import KernelSpec, RBFSpec, Matern32Spec, StdPeriodicSpec, ScaledSpec
from cases import Case

import exact_suite as es
import parity_suite as ps
import loo_suite
from parity_suite import _close, _poly_product
from matern52_suite import Matern52Spec, k52, dk52, _inputs, _oracle_top

from runlmc_amd.kern import RBF, Matern32, Matern52, StdPeriodic, Cosine, Product, Scaled
from runlmc_amd.lmc.functional_kernel import FunctionalKernel

TWO_PI = 2 * np.pi


class CosineSpec:
    n_params = 1

    def __init__(self, frequency=1.0, active_dims=None):
        self.frequency = float(frequency)
        self.active_dims = active_dims

    def from_dist(self, d):
        d = np.asarray(d, dtype=float)
        return np.cos(2 * np.pi * self.frequency * d)

    def kernel_gradient(self, d):
        d = np.asarray(d, dtype=float)
        return [-(2 * np.pi * d) * np.sin(2 * np.pi * self.frequency * d)]


class ProductSpec:
    def __init__(self, *factors, active_dims=None):
        self.factors = list(factors)
        self.active_dims = active_dims
        self.n_params = sum(f.n_params for f in factors)

    def from_dist(self, d):
        vals = [f.from_dist(d) for f in self.factors]
        if any(np.ndim(v) == 0 and np.isnan(v) for v in vals):
            return np.nan
        return np.prod(np.array(vals), axis=0)

    def kernel_gradient(self, d):
        vals = [f.from_dist(d) for f in self.factors]
        out = []
        for i, f in enumerate(self.factors):
            rest = np.prod(np.array([v for j, v in enumerate(vals) if j != i]), axis=0)
            out += [g * rest for g in f.kernel_gradient(d)]
        return out


_LEAF_SPEC = {RBF: RBFSpec, Matern32: Matern32Spec, Matern52: Matern52Spec,
              StdPeriodic: StdPeriodicSpec, Cosine: CosineSpec}


def _recipes(P=1):
    """The kernel set of the exact-likelihood checks as (class, parameters) recipes, with the
    active columns of the module docstring when P > 1."""
    one = (lambda i: None) if P == 1 else (lambda i: [i % P])
    return [((( RBF, (2.0,)), (StdPeriodic, (1.5, 0.4))), None, one(0)),
            (((Matern32, (3.0,)), (Cosine, (2.5,)), (RBF, (0.7,))), 1.7, one(1)),
            (((Matern52, (1.5,)),), None, None),
            (((StdPeriodic, (1.0, 0.3)), (StdPeriodic, (2.0, 0.5)), (StdPeriodic, (0.5, 0.9))), 0.8, one(0))]


def _build(recipe, spec):
    """A recipe as a package kernel (spec=False) or as its closed-form twin."""
    leaves, scale, ad = recipe
    if spec:
        fs = [_LEAF_SPEC[cls](*prm) for cls, prm in leaves]
        k = fs[0] if len(fs) == 1 else ProductSpec(*fs)
        k.active_dims = ad
        return k if scale is None else ScaledSpec(k, scale)
    fs = [cls(*prm) for cls, prm in leaves]
    if len(fs) == 1:
        k = type(fs[0])(*leaves[0][1], active_dims=ad)
    else:
        k = Product(*fs, active_dims=ad)
    return k if scale is None else Scaled(k, scale)


# --- 1. the classes (host) ----------------------------------------------------------------------
R4 = np.array([0.0, 1e-8, 0.3, 5.0])


def _with_params(recipe, theta):
    """The recipe with its leaf parameters (and the scale, last) replaced by theta."""
    leaves, scale, ad = recipe
    out, pos = [], 0
    for cls, prm in leaves:
        out.append((cls, tuple(theta[pos:pos + len(prm)])))
        pos += len(prm)
    return (tuple(out), None if scale is None else theta[pos], ad)


def _theta(recipe):
    leaves, scale, _ = recipe
    return [v for _, prm in leaves for v in prm] + ([] if scale is None else [scale])


def check_classes():
    # Cosine
    for f in (1.0, 2.5, 0.3):
        k = Cosine(f)
        assert k.name == 'cosine' and k.active_dims is None
        np.testing.assert_array_equal(k.param_array, [f])
        np.testing.assert_allclose(k.from_dist(R4), np.cos(TWO_PI * f * R4), rtol=1e-14, atol=0)
        (g,) = k.kernel_gradient(R4)
        assert k.from_dist(R4)[0] == 1.0 and g[0] == 0.0
        np.testing.assert_allclose(g, -(TWO_PI * R4) * np.sin(TWO_PI * f * R4), rtol=1e-14, atol=0)
    k = Cosine(1.0)
    k.set_params([2.0])
    assert k.frequency == 2.0
    k.update_gradient([0.5])
    np.testing.assert_array_equal(k.gradient, [0.5])
    assert Cosine(1.0, name='c', active_dims=[1]).active_dims == [1]

    # values and every gradient entry against the closed forms; every gradient against a central
    # difference in its parameter.  The difference's own truncation error is h^2 / 6 times the
    # third derivative in the parameter: for cos(2 pi f r) that is (1e-5 f)^2 (2 pi r)^2 / 6 of the
    # derivative's largest entry, 4e-8 at f = 2.5 on r <= 3 -- so the difference is taken on
    # r <= 3 (as check_kernel_class does for its scaled kernel), not at r = 5
    rr = np.linspace(0, 3, 50)
    singles = [((( Cosine, (f,)),), None, None) for f in (1.0, 2.5)]
    for recipe in _recipes() + singles:
        k, spec = _build(recipe, False), _build(recipe, True)
        np.testing.assert_allclose(k.from_dist(R4), spec.from_dist(R4), rtol=1e-14, atol=0)
        grads, want = k.kernel_gradient(R4), spec.kernel_gradient(R4)
        theta = _theta(recipe)
        assert len(grads) == len(want) == len(theta)
        for g, w in zip(grads, want):
            np.testing.assert_allclose(g, w, rtol=1e-14, atol=0)
        grads = k.kernel_gradient(rr)
        for p, t in enumerate(theta):
            h = 1e-5 * t
            up, dn = list(theta), list(theta)
            up[p], dn[p] = t + h, t - h
            fd = (_build(_with_params(recipe, up), False).from_dist(rr) -
                  _build(_with_params(recipe, dn), False).from_dist(rr)) / (2 * h)
            err = np.abs(grads[p] - fd).max()
            assert err <= 1e-7 * np.abs(fd).max(), (recipe, p, err, np.abs(fd).max())

    # order, set_params and update_gradient splitting
    p = Product(RBF(2.0), StdPeriodic(1.5, 0.4), Cosine(3.0))
    assert p.name == 'rbf_x_std_periodic_x_cosine' and p.active_dims is None
    assert Product(RBF(1), Cosine(1), name='sm').name == 'sm'
    np.testing.assert_array_equal(p.param_array, [2.0, 1.5, 0.4, 3.0])
    p.set_params([0.5, 0.6, 0.7, 0.8])
    f0, f1, f2 = p.factors
    assert (f0.inv_lengthscale, f1.inv_lengthscale, f1.period, f2.frequency) == (0.5, 0.6, 0.7, 0.8)
    np.testing.assert_array_equal(p.param_array, [0.5, 0.6, 0.7, 0.8])
    p.update_gradient([1.0, 2.0, 3.0, 4.0])
    np.testing.assert_array_equal(p.gradient, [1.0, 2.0, 3.0, 4.0])
    np.testing.assert_array_equal(f0.gradient, [1.0])
    np.testing.assert_array_equal(f1.gradient, [2.0, 3.0])
    np.testing.assert_array_equal(f2.gradient, [4.0])
    # StdPeriodic's NaN convention
    assert np.isnan(Product(RBF(1.0), StdPeriodic(1.0, 1e-100)).from_dist(R4))

    # Scaled(Product): the inner parameters, the scale's derivative last
    sk = Scaled(Product(Matern32(3.0), Cosine(2.5)), 1.7)
    assert sk.name == 'scaled_matern32_x_cosine'
    np.testing.assert_array_equal(sk.param_array, [3.0, 2.5])
    grads = sk.kernel_gradient(rr)
    assert len(grads) == 3
    np.testing.assert_allclose(grads[2], Matern32Spec(3.0).from_dist(rr) * CosineSpec(2.5).from_dist(rr),
                               rtol=1e-14)
    sk.update_gradient([0.25, 0.5, 4.0])
    np.testing.assert_array_equal(sk.k.gradient, [0.25, 0.5])
    np.testing.assert_array_equal(sk.k.factors[1].gradient, [0.5])
    assert sk.scale_gradient == 4.0
    sk.set_params([0.9, 1.1])
    assert sk.k.factors[0].inv_lengthscale == 0.9 and sk.k.factors[1].frequency == 1.1 and sk.scale == 1.7

    # nested products are flattened
    a, b, c = RBF(1.0), Cosine(2.0), Matern52(3.0)
    nested = Product(Product(a, b), c)
    assert nested.factors == [a, b, c] and nested.name == 'rbf_x_cosine_x_matern52'
    np.testing.assert_array_equal(nested.param_array, [1.0, 2.0, 3.0])

    # the three ValueErrors
    for bad in (lambda: Product(Product(RBF(1), RBF(2)), Product(RBF(3), RBF(4))),
                lambda: Product(Scaled(RBF(1.0), 2.0), RBF(1.0)),
                lambda: Product(RBF(1.0, active_dims=[1]), Cosine(1.0), active_dims=[0])):
        try:
            bad()
        except ValueError:
            pass
        else:
            raise AssertionError('accepted')
    assert Product(RBF(1.0, active_dims=[0]), Cosine(1.0), active_dims=[0]).active_dims == [0]

    # active dimensions reach the factors through FunctionalKernel.set_input_dim
    p2, p3 = Product(RBF(1.0), Cosine(1.0)), Product(RBF(1.0), Matern32(1.0), active_dims=[1])
    fk = FunctionalKernel(D=2, lmc_kernels=[p2, p3], lmc_ranks=[1, 1])
    fk.set_input_dim(2)
    assert p2.active_dims == (0, 1) and all(f.active_dims == (0, 1) for f in p2.factors)
    assert p3.active_dims == (1,) and all(f.active_dims == (1,) for f in p3.factors)


# --- 2. grid products -----------------------------------------------------------------------------
def _rows(x):
    """name -> (top row, the form measured for it or None)."""
    m32, m52 = Matern32Spec, Matern52Spec
    pp = ProductSpec(m32(3.0), m32(7.0))
    p54 = ProductSpec(m52(3.0), m32(7.0))
    return {
        'm32 x m32': (pp.from_dist(x), 2),
        'd/dgamma_1 of m32 x m32': (pp.kernel_gradient(x)[0], 2),
        'm52 x m32': (p54.from_dist(x), 2),
        'rbf x cos': (ProductSpec(RBFSpec(20.0), CosineSpec(3.0)).from_dist(x), 1),
        'rbf x periodic': (ProductSpec(RBFSpec(4.0), StdPeriodicSpec(2.0, 0.3)).from_dist(x), None),
        'm32 x cos': (ProductSpec(m32(3.0), CosineSpec(3.0)).from_dist(x), None),
        'rbf x fast cos': (ProductSpec(RBFSpec(200.0), CosineSpec(12.0)).from_dist(x), None),
        'd/dgamma of m52 x m32': (p54.kernel_gradient(x)[0], None),
    }


def check_grid_products(m, k):
    """Every composite row and gradient row as the single top of an operator (D = 2) and all of
    them as the tops of one: products against the oracle's BTTB products at _close's default and
    against the same handle's transform kernels at 1e-12; the measured forms where they are
    part of the contract."""
    from runlmc_amd._native import GridOp
    D = 2
    x = np.linspace(0, 1, m)
    rng = np.random.RandomState(60 + m + k)
    Xs = _inputs(rng, D, m, k, x)
    rows = _rows(x)
    g = GridOp(D, m, 1)
    for name, (row, form) in rows.items():
        g.set_lmc(row[None], [None], [np.ones(D)])
        forms, _ = g.top_forms()
        if form is not None:
            assert forms == [form], (name, m, forms)
        for X in Xs:
            want = _oracle_top(row, X, D, m)
            fft = g.matmat_host(X)
            got = _poly_product(g, X)
            _close(fft, want)
            _close(got, want)
            _close(got, fft, 1e-12)
    # all rows in one LMC operator
    tops = np.array([row for row, _ in rows.values()])
    Q = len(tops)
    A = [rng.randn(1 + q % 2, D) for q in range(Q)]
    kap = [np.abs(rng.randn(D)) + 0.1 for _ in range(Q)]
    Bs = ops.coreg_mats(A, kap)
    toeps = [ops.BTTBOracle(t) for t in tops]
    gq = GridOp(D, m, Q)
    gq.set_lmc(tops, A, kap)
    forms, _ = gq.top_forms()
    for (name, (_, form)), got in zip(rows.items(), forms):
        assert form is None or got == form, (name, m, forms)
    for X in Xs:
        want = np.array([ops.grid_sum_matvec(Bs, toeps, r) for r in X])
        fft = gq.matmat_host(X)
        got = _poly_product(gq, X)
        _close(fft, want)
        _close(got, want)
        _close(got, fft, 1e-12)


# --- 3. the exact likelihood ------------------------------------------------------------------------
def _exact_model(n, D, P, seed):
    """matern52_suite._exact_model's data, coregionalisation and noise (>= 0.05) for the four
    kernels of _recipes."""
    rng = np.random.RandomState(seed)
    lens = np.full(D, n // D)
    lens[:n - lens.sum()] += 1
    if P == 1:
        Xs = [np.sort(rng.rand(int(l)))[:, None] for l in lens]
    else:
        Xs = [rng.rand(int(l), P) for l in lens]
    rec = _recipes(P)
    Q = len(rec)
    A = [rng.randn(1 + q % 2, D) * 0.6 for q in range(Q)]
    kappa = [np.abs(rng.randn(D)) * 0.3 + 0.05 for _ in range(Q)]
    noise = 0.05 + 0.1 * rng.rand(D)
    y = rng.randn(n)
    fk = es._fk(D, [_build(r, False) for r in rec], A, kappa, noise, P=P)
    spec = KernelSpec(D, [_build(r, True) for r in rec], A, kappa, noise)
    spec.set_input_dim(P)
    return fk, spec, Xs, y, [int(l) for l in lens]


def _host_reference(spec, Xs, y, D):
    """matern52_suite._host_reference's recipe (SciPy's Cholesky, K^-1 by cho_solve,
    dL/dt = 1/2 sum M dK with M = alpha alpha^T - K^-1), every kernel on the distance over ITS
    active columns."""
    lens = [len(x) for x in Xs]
    X = np.vstack([np.asarray(x, dtype=float).reshape(len(x), -1) for x in Xs])
    n = len(X)
    ends = np.cumsum(lens)
    begins = ends - np.asarray(lens)
    o = np.repeat(np.arange(D), lens)

    def dist_of(k):
        cols = list(k.active_dims)
        return np.sqrt(np.square(X[:, None, cols] - X[None, :, cols]).sum(axis=-1))
    K = np.zeros((n, n))
    for B, k in zip(spec.coreg_mats(), spec._kernels):
        K += B[np.ix_(o, o)] * k.from_dist(dist_of(k))
    K[np.diag_indices(n)] += np.repeat(spec.noise, lens)
    cf = la.cho_factor(K, lower=True)
    logdet = 2.0 * np.log(np.diag(cf[0])).sum()
    alpha = la.cho_solve(cf, y)
    M = np.outer(alpha, alpha) - la.cho_solve(cf, np.identity(n))

    def block_sums(Kq):
        Pm = M * Kq
        return np.array([[Pm[begins[a]:ends[a], begins[b]:ends[b]].sum() for b in range(D)]
                         for a in range(D)])

    g = dict(coreg_vec=[], coreg_diag=[], kernel=[], noise=None)
    for a_q, B, k in zip(spec.coreg_vecs, spec.coreg_mats(), spec._kernels):
        dist = dist_of(k)
        S = block_sums(k.from_dist(dist))
        g['coreg_vec'].append(0.5 * np.atleast_2d(a_q).dot(S + S.T))
        g['coreg_diag'].append(0.5 * np.diag(S).copy())
        g['kernel'].append([0.5 * np.sum(B * block_sums(dk)) for dk in k.kernel_gradient(dist)])
    g['noise'] = np.array([0.5 * np.trace(M[b:e, b:e]) for b, e in zip(begins, ends)])
    return logdet, alpha, g, K


def check_exact(n, D, P=1):
    from runlmc_amd._native import ExactOp, exact_factor_descriptors, exact_is_composite
    from runlmc_amd.lmc import ExactLMCLikelihood
    fk, spec, Xs, y, lens = _exact_model(n, D, P, seed=n * 7 + D + P)
    assert exact_is_composite(fk.kernels)
    nfact, leaves, _, scaled, scales, _, nder = exact_factor_descriptors(fk.kernels)
    assert list(nfact) == [2, 3, 1, 3] and nder == [3, 4, 1, 7]
    assert leaves.tolist() == [[0, 2, 0], [1, 4, 0], [3, 0, 0], [2, 2, 2]]
    assert list(scaled) == [0, 1, 0, 1] and list(scales) == [0.0, 1.7, 0.0, 0.8]
    logdet, alpha, ref, K = _host_reference(spec, Xs, y, D)
    op = ExactOp(n, P)
    op.set(np.vstack(Xs), lens, fk.kernels, fk.coreg_mats(), fk.noise)
    es._close(op.dense(), K, 1e-12, 'dense')
    rng = np.random.RandomState(1)
    Xt = [rng.rand(3 + d, P) for d in range(D)]
    ads = [k.active_dims for k in spec._kernels]
    Kx = es._cross_dense(spec, Xt, Xs, D, ads)
    es._close(op.cross(np.vstack(Xt), [len(v) for v in Xt]), Kx, 1e-12, 'cross')
    Ys = np.split(y, np.cumsum(lens)[:-1])
    lik = ExactLMCLikelihood(fk, Xs, Ys)
    assert abs(lik.log_det_K() - logdet) <= 1e-9 * abs(logdet), (lik.log_det_K(), logdet)
    assert [len(g) for g in lik.kernel_gradients()] == [3, 4, 1, 7]
    es._compare_to_oracle(lik, ref, alpha, K, 4, rtol=1e-9)
    # two calls, two handles: the same bits
    lik2 = ExactLMCLikelihood(fk, Xs, Ys)
    S1, n1 = lik._op.grad_sums(lik._alpha_dev)
    S2, n2 = lik._op.grad_sums(lik._alpha_dev)
    assert np.array_equal(S1, S2) and np.array_equal(n1, n2)
    for u, v in zip(es._grads_flat(lik, 4), es._grads_flat(lik2, 4)):
        for a, b in zip(u, v):
            assert np.array_equal(a, b)
    assert lik.log_det_K() == lik2.log_det_K() and np.array_equal(lik.alpha(), lik2.alpha())


def check_exact_cosine_alone():
    """A set with no Product: Cosine alone (one factor, which ex_eval has no formula for) and
    under Scaled, beside a plain RBF; K, cross rows and every gradient against the host."""
    from runlmc_amd._native import ExactOp, exact_is_composite
    from runlmc_amd.lmc import ExactLMCLikelihood
    n, D = 65, 3
    rng = np.random.RandomState(77)
    lens = [22, 22, 21]
    Xs = [np.sort(rng.rand(l))[:, None] for l in lens]
    A = [rng.randn(1, D) * 0.6 for _ in range(3)]
    kappa = [np.abs(rng.randn(D)) * 0.3 + 0.05 for _ in range(3)]
    noise = 0.05 + 0.1 * rng.rand(D)
    y = rng.randn(n)
    fk = es._fk(D, [Cosine(2.5), Scaled(Cosine(1.2), 0.7), RBF(2.0)], A, kappa, noise)
    spec = KernelSpec(D, [CosineSpec(2.5), ScaledSpec(CosineSpec(1.2), 0.7), RBFSpec(2.0)], A, kappa, noise)
    spec.set_input_dim(1)
    assert exact_is_composite(fk.kernels)
    logdet, alpha, ref, K = _host_reference(spec, Xs, y, D)
    op = ExactOp(n, 1)
    op.set(np.vstack(Xs), lens, fk.kernels, fk.coreg_mats(), fk.noise)
    assert op.nder == [1, 2, 1]
    es._close(op.dense(), K, 1e-12, 'dense')
    Xt = [rng.rand(3 + d, 1) for d in range(D)]
    es._close(op.cross(np.vstack(Xt), [len(v) for v in Xt]), es._cross_dense(spec, Xt, Xs, D), 1e-12, 'cross')
    lik = ExactLMCLikelihood(fk, Xs, np.split(y, np.cumsum(lens)[:-1]))
    assert abs(lik.log_det_K() - logdet) <= 1e-9 * abs(logdet)
    es._compare_to_oracle(lik, ref, alpha, K, 3, rtol=1e-9)


def _simple(n=17, D=1, seed=3):
    rng = np.random.RandomState(seed)
    X = np.sort(rng.rand(n))[:, None]
    return X, [n], 0.05 + 0.1 * rng.rand(D)


def check_exact_limits():
    """Q + sum p = 32 is accepted (four 7-derivative kernels: 4 + 28), one RBF more (34) is not,
    and the message names the count."""
    from runlmc_amd._native import ExactOp
    X, lens, noise = _simple()
    seven = lambda: Scaled(Product(StdPeriodic(1, .3), StdPeriodic(2, .5), StdPeriodic(.5, .9)), 0.8)
    kerns = [seven() for _ in range(4)]
    for k in kerns:
        k.active_dims = (0,)
    op = ExactOp(17, 1)
    B = np.array([[[0.5]]] * 4)
    op.set(X, lens, kerns, B, noise)
    assert op.Q + sum(op.nder) == 32
    op.factor()
    S, _ = op.grad_sums(np.ones(17))
    assert S.shape == (32, 1, 1) and np.all(np.isfinite(S))
    more = kerns + [RBF(1.0, active_dims=(0,))]
    try:
        op.set(X, lens, more, np.array([[[0.5]]] * 5), noise)
    except NotImplementedError as e:
        assert '34' in str(e), str(e)
    else:
        raise AssertionError('Q + sum p = 34 accepted')
    # more kernels than the handle has slots for: refused with the count before anything indexed
    # by the kernel is written (33 two-factor products: 33 + 66; 70 plain kernels: 70 + 70)
    many = [Product(RBF(1.0 + 0.01 * q), Matern32(2.0), active_dims=(0,)) for q in range(33)]
    plain = [RBF(1.0 + 0.01 * q, active_dims=(0,)) for q in range(70)]
    for ks, count in ((many, '99'), (plain, '140')):
        try:
            op.set(X, lens, ks, np.array([[[0.5]]] * len(ks)), noise)
        except NotImplementedError as e:
            assert count in str(e), str(e)
        else:
            raise AssertionError('%d kernels accepted' % len(ks))
    op.set(X, lens, kerns, B, noise)        # the handle is still usable
    op.factor()


def check_exact_old_path():
    """Plain kernels through rl_exact_set_factors (one factor each): the same bits as rl_exact_set,
    in K and in the gradient sums; unknown leaf kinds are rejected."""
    from runlmc_amd import _native
    from runlmc_amd._lib import host_ptr
    rng = np.random.RandomState(4)
    n, D = 65, 3
    lens = [22, 22, 21]
    X = rng.rand(n, 1)
    kerns = [RBF(2.0), Matern32(1.5), Scaled(StdPeriodic(1.0, 0.7), 1.7), Scaled(Matern52(3.0), 0.6)]
    for k in kerns:
        k.active_dims = (0,)
    A = [rng.randn(1, D) * 0.6 for _ in kerns]
    B = np.array([a.T @ a + np.diag(np.abs(rng.randn(D)) * 0.3 + 0.05) for a in A])
    noise = 0.05 + 0.1 * rng.rand(D)
    alpha = rng.randn(n)
    assert not _native.exact_is_composite(kerns)
    old = _native.ExactOp(n, 1)
    old.set(X, lens, kerns, B, noise)
    new = _native.ExactOp(n, 1)
    saved = _native.exact_is_composite
    _native.exact_is_composite = lambda kernels: True
    try:
        new.set(X, lens, kerns, B, noise)
    finally:
        _native.exact_is_composite = saved
    assert new.nder == old.nder == [1, 1, 3, 2]
    assert np.array_equal(new.dense(), old.dense())
    Xt = rng.rand(7, 1)
    assert np.array_equal(new.cross(Xt, [3, 2, 2]), old.cross(Xt, [3, 2, 2]))
    assert old.factor() == new.factor()
    for u, v in zip(old.grad_sums(alpha), new.grad_sums(alpha)):
        assert np.array_equal(u, v)
    # unknown leaf kinds
    nfact, leaves, lparams, scaled, scales, cols, _ = _native.exact_factor_descriptors(kerns)
    L = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    for bad in (5, 15):
        lv = leaves.copy()
        lv[1, 0] = bad
        try:
            new.lib.call('rl_exact_set_factors', new._h, host_ptr(X), host_ptr(L), D, len(kerns),
                         host_ptr(nfact), host_ptr(lv), host_ptr(lparams), host_ptr(scaled),
                         host_ptr(scales), host_ptr(cols), host_ptr(B), host_ptr(noise))
        except ValueError as e:
            assert 'unknown kernel kind %d' % bad in str(e), str(e)
        else:
            raise AssertionError('leaf kind %d accepted' % bad)
    # a plain kernel inside a composite set runs ex_eval_fact<3> with one factor: the same bits as
    # ex_eval.  A Product with B = 0 joins the plain kernels (it adds exact zeros to K), LAST, so
    # that the plain kernels keep their order in every sum; K, cross rows and the plain kernels'
    # value and derivative block sums against the plain handle's
    mixed = _native.ExactOp(n, 1)
    prod = Scaled(Product(Matern32(3.0), Cosine(2.5), StdPeriodic(0.5, 0.9)), 1.7)
    prod.active_dims = (0,)
    mixed.set(X, lens, kerns + [prod], np.concatenate([B, np.zeros((1, D, D))]), noise)
    assert mixed.nder == [1, 1, 3, 2, 5]
    assert np.array_equal(mixed.dense(), old.dense())
    assert np.array_equal(mixed.cross(Xt, [3, 2, 2]), old.cross(Xt, [3, 2, 2]))
    assert mixed.factor() == old.factor()
    (So, no), (Sm, nm) = old.grad_sums(alpha), mixed.grad_sums(alpha)
    Q = len(kerns)
    assert So.shape == (Q + 7, D, D) and Sm.shape == (Q + 1 + 12, D, D)
    assert np.array_equal(Sm[:Q], So[:Q])                       # k_q
    assert np.array_equal(Sm[Q + 1:Q + 1 + 7], So[Q:])          # dk_q / dtheta_p, scales included
    assert np.array_equal(nm, no)
    assert np.all(np.isfinite(Sm))
    # exact_descriptors still names the class it has no formula for
    try:
        _native.exact_descriptors([Cosine(1.0, active_dims=(0,))])
    except NotImplementedError as e:
        assert 'Cosine' in str(e)
    else:
        raise AssertionError('exact_descriptors took a Cosine')


# --- 4. the model ---------------------------------------------------------------------------------
GRID = 640


def _kernels(spec):
    if spec:
        return [ProductSpec(RBFSpec(2.0), StdPeriodicSpec(1.5, 0.4)), Matern32Spec(1.5)]
    return [Product(RBF(2.0), StdPeriodic(1.5, 0.4)), Matern32(1.5)]


@functools.lru_cache(maxsize=None)
def _model_case():
    c = Case('lmc_small')
    A, kap = list(c.coreg_vecs[:2]), list(c.coreg_diags[:2])
    spec = KernelSpec(c.D, _kernels(True), A, kap, c.noise)
    spec.set_input_dim(1)
    Xtr = [np.asarray(v).reshape(len(v), 1) for v in c.Xs]
    rng = np.random.RandomState(9)
    Xt = [np.sort(rng.rand(4 + d, 1), axis=0) * 0.9 + 0.05 for d in range(c.D)]
    return c, A, kap, spec, Xtr, Xt


def _model(prediction='on-the-fly', metrics=False, variance_batch=None, tolerance=1e-4, kernels=None):
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    c, A, kap, _, Xtr, _ = _model_case()
    fk = FunctionalKernel(D=c.D, lmc_kernels=kernels or _kernels(False),
                          lmc_ranks=[len(a) for a in A])
    fk.coreg_vecs = A
    fk.coreg_diags = kap
    fk.noise = c.noise
    np.random.seed(5)
    return InterpolatedLLGP(Xtr, c.Ys, normalize=False, m=[GRID], functional_kernel=fk,
                            prediction=prediction, metrics=metrics, trace_iterations=len(c.rs),
                            tolerance=tolerance, variance_batch=variance_batch)


def check_model_params():
    """param_array: the expected length, a round trip at 1e-12, and the values landing in the
    factors."""
    from runlmc_amd.models.interpolated_llgp import _softplus
    c, A, kap, _, _, _ = _model_case()
    model = _model()
    x = model.param_array.copy()
    want = sum(a.size for a in A) + 2 * c.D + (3 + 1) + c.D
    assert x.shape == (want,), (x.shape, want)
    rng = np.random.RandomState(3)
    x1 = x + 0.05 * rng.randn(len(x))
    model.param_array = x1
    np.testing.assert_allclose(model.param_array, x1, rtol=0, atol=1e-12)
    i = sum(a.size for a in A) + 2 * c.D
    prod = model._functional_kernel.kernels[0]
    got = [prod.factors[0].inv_lengthscale, prod.factors[1].inv_lengthscale, prod.factors[1].period]
    np.testing.assert_allclose(got, _softplus(x1[i:i + 3]), rtol=1e-12)
    assert model.gradient.shape == x.shape and np.all(np.isfinite(model.gradient))
    assert len(prod.gradient) == 3 and len(prod.factors[1].gradient) == 2


def check_model_metrics():
    model = _model(metrics=True)
    model.parameters_changed()
    got = model.metrics.grad_error
    assert len(got) == 1 and np.isfinite(got[0]), got
    assert np.all(np.isfinite(model.gradient))
    (W, _), = model.interpolants.values()
    assert W.shape[1] >= 600 * model.output_dim


def _native_variance():
    c, A, kap, spec, _, Xt = _model_case()
    coreg = np.column_stack([np.square(a).sum(axis=0) for a in A]) + np.column_stack(kap)
    k0 = np.array([float(k.from_dist(0.0)) for k in spec._kernels])
    return np.repeat(coreg @ k0 + c.noise, [len(v) for v in Xt])


def check_model_exact_prediction():
    c, _, _, spec, Xtr, Xt = _model_case()
    model = _model(prediction='exact')
    _, var = model.predict(Xt)
    Kx = es._cross_dense(spec, Xt, Xtr, c.D)
    Kd = es._cross_dense(spec, Xtr, Xtr, c.D) + np.diag(np.repeat(c.noise, c.lens))
    native = _native_variance()
    ref = np.clip(native - np.einsum('ij,ji->i', Kx, la.solve(Kd, Kx.T)), 0, None)
    np.testing.assert_allclose(np.concatenate(var), ref, rtol=0, atol=1e-8 * native.max())
    es._close(model.K(), Kd, 1e-12, 'K()')


def check_model_tiled_variances():
    _, _, _, _, _, Xt = _model_case()
    mu0, var0 = _model().predict(Xt)
    mu1, var1 = _model(variance_batch=16).predict(Xt)
    native = _native_variance()
    atol = 1e-5 * max(native.max(), 1.0)
    err = np.abs(np.concatenate(var1) - np.concatenate(var0)).max()
    print('tiled against host-assembled variances: max difference %.3e (atol %.3e)' % (err, atol))
    np.testing.assert_allclose(np.concatenate(var1), np.concatenate(var0), rtol=0, atol=atol)
    np.testing.assert_array_equal(np.concatenate(mu1), np.concatenate(mu0))


def check_model_solve():
    """matern52_suite.check_model_solve on the composite model."""
    from runlmc_amd.approx.iterative import Iterative
    c, _, _, spec, _, _ = _model_case()
    model = _model()
    model._ensure()
    K = model._K
    (ad, (W, WT)), = model.interpolants.items()
    assert W.shape[1] >= 600 * c.D
    op = olik.LMCOperatorOracle(spec, model.dists[ad], W, WT, c.lens)
    Kd = ps._dense_spd(op, c.n)
    xref = la.solve(Kd, c.y, assume_a='pos')
    x, _, res = Iterative.solve(K, c.y, verbose=True)
    assert res < 1e-4 and np.linalg.norm(c.y - Kd @ x) < 1e-4, (res, np.linalg.norm(c.y - Kd @ x))
    M = K.preconditioner
    if M is None:
        bound = np.linalg.norm(c.y - Kd @ x) / c.noise.min()
        assert np.abs(x - xref).max() <= bound
        return 'krylov'
    bar = 1e-9 if M.exact else 1e-8
    x, _, res = Iterative.solve(K, c.y, verbose=True, tol=bar)
    assert res < bar, res
    _close(x, xref, rel=bar)
    return 'exact' if M.exact else 'preconditioner'


def check_model_update():
    """A model moved to other parameters through param_array (GridKernel.update on the live
    handles) against a model built at those parameters: alpha and the predictive means at the
    product tolerance (_close's default).  Both solve to 1e-12 with MINRES ended by the residual
    rule alone, so that what is compared is the operator and not where a 1e-4 solve stopped."""
    _, _, _, _, _, Xt = _model_case()
    with loo_suite._tight_krylov():
        walked = _model(tolerance=1e-12)
        x0 = walked.param_array.copy()
        rng = np.random.RandomState(8)
        x1 = x0 + 0.1 * rng.randn(len(x0))
        np.random.seed(5)
        walked.param_array = x1
        fresh = _model(tolerance=1e-12)
        fk, src = fresh._functional_kernel, walked._functional_kernel
        fk.coreg_vecs, fk.coreg_diags, fk.noise = src.coreg_vecs, src.coreg_diags, src.noise
        for k, s in zip(fk.kernels, src.kernels):
            k.set_params(s.param_array)
        np.random.seed(5)
        fresh._ensure()
        np.testing.assert_allclose(fresh.param_array, x1, rtol=0, atol=1e-12)
        a, b = walked.kernel.alpha(), fresh.kernel.alpha()
        _close(a, b)
        mu_a, mu_b = walked.predict(Xt)[0], fresh.predict(Xt)[0]
    _close(np.concatenate(mu_a), np.concatenate(mu_b))


# --- 5. downstream features --------------------------------------------------------------------------
def check_model_loo():
    """loo_predict against the dense leave-one-out formulas on the oracle operator's dense K~, at
    loo_suite.check_model_loo's bars (means 1e-8 max|y|, variances delta_d / d^2 with
    delta_d = 1e-9 max(1 / eps)) -- the same for the 'direct' and the 'solve' method; 'solve'
    (one solve per row) is asked for a selection of rows, as there."""
    c, _, _, spec, _, _ = _model_case()
    with loo_suite._tight_krylov():
        model = _model(tolerance=1e-12)
        model._ensure()
        (ad, (W, WT)), = model.interpolants.items()
        op = olik.LMCOperatorOracle(spec, model.dists[ad], W, WT, c.lens)
        Kd = ps._dense_spd(op, c.n)
        Kinv = la.inv(Kd)
        alpha, d = Kinv @ c.y, np.diag(Kinv)
        mean_ref, var_ref = c.y - alpha / d, 1.0 / d
        mean_tol = 1e-8 * np.abs(c.y).max()
        var_tol = loo_suite.DIAG_REL * np.max(1.0 / c.noise) / d ** 2
        ends = np.cumsum(c.lens)[:-1]
        sel = np.concatenate([[0, c.n - 1], ends - 1, ends, [7, 23]])
        means, vars_ = model.loo_predict(indices=sel, tol=1e-12)
    used = model.loo_stats['method']
    assert used in ('direct', 'solve'), used
    assert model.loo_stats['nonpositive'] == 0
    em, ev = np.abs(means - mean_ref[sel]).max(), (np.abs(vars_ - var_ref[sel]) / var_tol[sel]).max()
    print('composite loo (%s): mean error %.3e (tol %.3e), variance error / tol %.3e' % (used, em, mean_tol, ev))
    assert em <= mean_tol and ev <= 1.0, (em, mean_tol, ev)
    assert np.all(vars_ > np.repeat(c.noise, c.lens)[sel])


def check_model_draws():
    """64 seeded posterior draws at 8 test points per output: the sample mean within
    5 sqrt(var / 64) of predict's mean, var = predict's variance less the noise."""
    c, _, _, _, _, _ = _model_case()
    model = _model()
    rng = np.random.RandomState(12)
    Xt = [np.sort(rng.rand(8, 1), axis=0) * 0.9 + 0.05 for _ in range(c.D)]
    mu, var = model.predict(Xt)
    f = model.posterior_draws(64, seed=2024)(Xt)
    for d in range(c.D):
        assert f[d].shape == (64, 8)
        latent = var[d] - c.noise[d]
        assert np.all(latent > 0)
        z = np.abs(f[d].mean(axis=0) - mu[d]) / np.sqrt(latent / 64)
        print('output %d: mean z-scores up to %.2f' % (d, z.max()))
        assert z.max() <= 5.0, (d, z)
