"""Checks of separable kernels (runlmc_amd.kern: Separable, RBF.ard, Lags) through every layer: the
host classes, the 2-D grid products of their rows, the exact dense likelihood on per-leaf
distances (csrc/rl_exact.h: ex_eval_sep, rl_exact_set_separable), the model, leave-one-out and
function draws.  Shared by the CPU run on the emulator (tests/test_separable_emu.py) and the GPU
run (tests/test_separable_gpu.py); every function uses whichever native library is active.

The oracle has no separable kernels, so the yardsticks are NumPy written here.  A kernel is
described by _Sep: a list of (leaf closed form, positions of its axes among the kernel's sorted
active dimensions) and a scale,
    k(lags) = c prod_g k_g(sqrt(sum_{i in g} lags_i^2)),
    dk / dtheta_{g,p} = c dk_g / dtheta_p prod_{h != g} k_h,   dk / dc = prod_g k_g  (last),
with the leaf closed forms of the oracle (RBF, Matern-3/2, periodic), matern52_suite (Matern-5/2)
and composite_suite (cosine, one-distance product).  An isotropic kernel is the _Sep of one factor
over all its axes.  Dense matrices are built from these entry by entry; Toeplitz blocks of a
separable row are np.kron of two scipy.linalg.toeplitz."""
import functools

import numpy as np
import scipy.linalg as la

from oracle import interp as ointerp
from oracle.kernels import RBFSpec, Matern32Spec, StdPeriodicSpec

import exact_suite as es
import grid2d_suite as g2
import loo_suite
from matern52_suite import Matern52Spec
from composite_suite import CosineSpec, ProductSpec

from runlmc_amd.kern import (RBF, Matern32, Matern52, StdPeriodic, Cosine, Product, Scaled,
                             Separable, Lags)
from runlmc_amd.lmc.functional_kernel import FunctionalKernel


class _Sep:
    """The closed form of the module docstring: factors = [(leaf form, axis positions)]."""

    def __init__(self, factors, scale=None, active_dims=None):
        self.factors, self.scale, self.active_dims = list(factors), scale, active_dims

    def _dists(self, lags):
        return [np.sqrt(sum(np.square(np.asarray(lags[i], dtype=float)) for i in pos))
                for _, pos in self.factors]

    def value(self, lags):
        out = None
        for (f, _), r in zip(self.factors, self._dists(lags)):
            v = f.from_dist(r)
            out = v if out is None else out * v
        return out if self.scale is None else self.scale * out

    def grads(self, lags):
        rs = self._dists(lags)
        vals = [f.from_dist(r) for (f, _), r in zip(self.factors, rs)]
        out = []
        for i, ((f, _), r) in enumerate(zip(self.factors, rs)):
            others = 1.0
            for j, v in enumerate(vals):
                if j != i:
                    others = others * v
            out += [g * others for g in f.kernel_gradient(r)]
        if self.scale is None:
            return out
        plain = vals[0]
        for v in vals[1:]:
            plain = plain * v
        return [self.scale * g for g in out] + [plain]


def _raises(exc, fn, *needles):
    try:
        fn()
    except exc as e:
        for s in needles:
            assert s in str(e), (s, str(e))
    else:
        raise AssertionError('%s not raised' % exc.__name__)


# --- 1. the classes (host) ----------------------------------------------------------------------
R4 = np.array([0.0, 1e-8, 0.3, 5.0])


def _class_cases(theta=None):
    """(package kernel, closed form, parameters) of the three kernels of check_classes at the
    parameters theta[i] (default: the list's own)."""
    t = theta or [[2.0, 1.5, 0.4], [3.0, 0.6, 0.7], [6.0, 40.0, 1.3]]
    a, b, c = t
    return [
        (Separable(RBF(a[0], active_dims=[0]), StdPeriodic(a[1], a[2], active_dims=[1])),
         _Sep([(RBFSpec(a[0]), [0]), (StdPeriodicSpec(a[1], a[2]), [1])]), a),
        (Separable(Product(Matern32(b[0]), Cosine(b[1]), active_dims=[0]), RBF(b[2], active_dims=[1])),
         _Sep([(ProductSpec(Matern32Spec(b[0]), CosineSpec(b[1])), [0]), (RBFSpec(b[2]), [1])]), b),
        (RBF.ard(c, [0, 1, 2]), _Sep([(RBFSpec(g), [i]) for i, g in enumerate(c)]), c),
    ]


def check_classes():
    l0, l1, l2 = np.meshgrid(R4, R4, R4[:2], indexing='ij')
    # central differences on lags <= 3 (composite_suite.check_classes: the difference's own
    # truncation error in a cosine's frequency passes 1e-7 at r = 5)
    rr = np.linspace(0, 3, 13)
    d0, d1, d2 = np.meshgrid(rr, rr, rr[:3], indexing='ij')
    for i, (k, ref, theta) in enumerate(_class_cases()):
        lags = (l0, l1, l2)[:len(k.active_dims)]
        assert k.separable and k.active_dims == tuple(range(len(lags)))
        np.testing.assert_allclose(k.from_lags(lags), ref.value(lags), rtol=1e-14, atol=0)
        grads, want = k.kernel_gradient_lags(lags), ref.grads(lags)
        assert len(grads) == len(want) == len(theta) == len(k.param_array)
        np.testing.assert_array_equal(k.param_array, theta)
        for g, w in zip(grads, want):
            np.testing.assert_allclose(g, w, rtol=1e-14, atol=0)
        assert k.from_lags(tuple(np.zeros(1) for _ in lags))[0] == 1.0
        lags = (d0, d1, d2)[:len(k.active_dims)]
        grads = k.kernel_gradient_lags(lags)
        for p, t in enumerate(theta):
            h = 1e-5 * t
            up, dn = [list(x) for x in (theta, theta)]
            up[p], dn[p] = t + h, t - h
            tu, td = [None] * 3, [None] * 3
            tu[i], td[i] = up, dn
            fd = (_class_cases([x or [1.0, 1.0, 1.0] for x in tu])[i][0].from_lags(lags) -
                  _class_cases([x or [1.0, 1.0, 1.0] for x in td])[i][0].from_lags(lags)) / (2 * h)
            err = np.abs(grads[p] - fd).max()
            assert err <= 1e-7 * np.abs(fd).max(), (i, p, err, np.abs(fd).max())

    # lags broadcast against each other
    k = _class_cases()[0][0]
    np.testing.assert_array_equal(k.from_lags((R4[:, None], R4[None, :])),
                                  k.from_lags(np.meshgrid(R4, R4, indexing='ij')))

    # the base class: every kernel of one distance answers at lags with its from_dist of the norm
    plain = [RBF(2.0), Matern32(3.0), Matern52(1.5), StdPeriodic(1.5, 0.4), Cosine(2.5),
             Product(RBF(2.0), StdPeriodic(1.5, 0.4), Cosine(3.0)), Scaled(Matern32(3.0), 1.7)]
    a, b = np.meshgrid(R4, R4, indexing='ij')
    for k in plain:
        assert not k.separable
        for lags in ((R4,), (a, b)):
            r = np.sqrt(sum(np.square(g) for g in lags))
            assert np.array_equal(k.from_lags(lags), k.from_dist(r))
            for g, w in zip(k.kernel_gradient_lags(lags), k.kernel_gradient(r)):
                assert np.array_equal(g, w)

    # names, order, set_params and the update_gradient split
    s = Separable(RBF(2.0, active_dims=[2]), Product(Matern32(3.0), Cosine(2.5), active_dims=[0]))
    assert s.name == 'rbf_x_matern32_x_cosine' and s.active_dims == (0, 2)
    assert Separable(RBF(1, active_dims=[0]), RBF(1, active_dims=[1]), name='st').name == 'st'
    assert [f.active_dims for f in s.factors] == [(2,), (0,)]
    np.testing.assert_array_equal(s.param_array, [2.0, 3.0, 2.5])
    # lags come in the order of the sorted union: axis 0 is the product's, axis 2 the RBF's
    lags = (np.array([0.3]), np.array([0.1]))
    want = (RBFSpec(2.0).from_dist(0.1) * Matern32Spec(3.0).from_dist(0.3) * CosineSpec(2.5).from_dist(0.3))
    np.testing.assert_allclose(s.from_lags(lags), [want], rtol=1e-14)
    s.set_params([0.5, 0.6, 0.7])
    assert (s.factors[0].inv_lengthscale, s.factors[1].factors[0].inv_lengthscale,
            s.factors[1].factors[1].frequency) == (0.5, 0.6, 0.7)
    s.update_gradient([1.0, 2.0, 3.0])
    np.testing.assert_array_equal(s.gradient, [1.0, 2.0, 3.0])
    np.testing.assert_array_equal(s.factors[0].gradient, [1.0])
    np.testing.assert_array_equal(s.factors[1].gradient, [2.0, 3.0])
    np.testing.assert_array_equal(s.factors[1].factors[1].gradient, [3.0])
    ard = RBF.ard([6.0, 40.0], [0, 1])
    assert type(ard) is Separable and ard.name == 'rbf_ard' and ard.active_dims == (0, 1)
    np.testing.assert_array_equal(ard.param_array, [6.0, 40.0])
    np.testing.assert_allclose(ard.from_lags((R4, R4[::-1])),
                               np.exp(-0.5 * (6.0 * R4 ** 2 + 40.0 * R4[::-1] ** 2)), rtol=1e-14)

    # Scaled(Separable): the inner parameters, the scale's derivative last
    sk = Scaled(_class_cases()[1][0], 1.7)
    ref = _class_cases()[1][1]
    ref.scale = 1.7
    assert sk.separable and sk.name == 'scaled_matern32_x_cosine_x_rbf' and sk.active_dims == (0, 1)
    np.testing.assert_array_equal(sk.param_array, [3.0, 0.6, 0.7])
    np.testing.assert_allclose(sk.from_lags((a, b)), ref.value((a, b)), rtol=1e-14)
    grads = sk.kernel_gradient_lags((a, b))
    assert len(grads) == 4
    for g, w in zip(grads, ref.grads((a, b))):
        np.testing.assert_allclose(g, w, rtol=1e-14, atol=0)
    sk.update_gradient([0.25, 0.5, 0.75, 4.0])
    np.testing.assert_array_equal(sk.k.gradient, [0.25, 0.5, 0.75])
    assert sk.scale_gradient == 4.0

    # no single distance: a plain array never passes for one, through any door
    k = _class_cases()[0][0]
    _raises(ValueError, lambda: k.from_dist(R4), k.name)
    _raises(ValueError, lambda: k.kernel_gradient(R4), k.name)
    _raises(ValueError, lambda: sk.from_dist(R4), sk.k.name)
    fk = FunctionalKernel(D=1, lmc_kernels=[_class_cases()[0][0]], lmc_ranks=[1])
    fk.set_input_dim(2)
    _raises(ValueError, lambda: fk.eval_kernels({(0, 1): a}), k.name)
    _raises(ValueError, lambda: fk.eval_kernels_fixed_dim(a, (0, 1)), k.name)
    _raises(ValueError, lambda: fk.eval_kernel_gradients({(0, 1): a}), k.name)
    at = Lags((a, b))
    assert np.array_equal(at.dist, np.sqrt(a ** 2 + b ** 2)) and at.shape == a.shape
    np.testing.assert_array_equal(fk.eval_kernels({(0, 1): at})[0], k.from_lags((a, b)))

    # the ValueErrors, each naming the offender
    r0, r1 = (lambda: RBF(1.0, name='r0', active_dims=[0])), (lambda: RBF(1.0, name='r1', active_dims=[1]))
    _raises(ValueError, lambda: Separable(Scaled(r0(), 2.0), r1()), 'scaled_r0', 'outside')
    _raises(ValueError, lambda: Separable(r0(), RBF(1.0, name='free')), 'free', 'active_dims')
    _raises(ValueError, lambda: Separable(r0(), RBF(1.0, name='none', active_dims=[])), 'none')
    _raises(ValueError, lambda: Separable(r0(), RBF(1.0, name='twin', active_dims=[1, 0])), 'r0', 'twin')
    _raises(ValueError, lambda: Separable(Product(RBF(1), RBF(2), active_dims=[0]),
                                          Product(RBF(3), RBF(4), active_dims=[1])), '3', '4')
    _raises(ValueError, lambda: Separable(r0()), '1')
    _raises(ValueError, lambda: Separable(r0(), Separable(r1(), RBF(1, active_dims=[2]))), 'Separable')
    _raises(ValueError, lambda: RBF.ard([1.0], [0]))
    _raises(ValueError, lambda: RBF.ard([1.0, 2.0], [0]))
    _raises(ValueError, lambda: RBF.ard([1.0] * 4, range(4)))
    # Product is as it was: factors on other dimensions are refused
    _raises(ValueError, lambda: Product(RBF(1.0, active_dims=[1]), Cosine(1.0), active_dims=[0]))

    # StdPeriodic's NaN convention
    nan = Separable(RBF(1.0, active_dims=[0]), StdPeriodic(1.0, 1e-100, active_dims=[1]))
    assert np.isnan(nan.from_lags((R4, R4)))
    assert np.isnan(Scaled(nan, 2.0).from_lags((R4, R4)))

    # FunctionalKernel: the union is the kernel's active set, next to an isotropic kernel's
    fk = FunctionalKernel(D=2, lmc_kernels=[RBF.ard([1.0, 2.0], [1, 0]), Matern32(1.0)], lmc_ranks=[1, 1])
    fk.set_input_dim(2)
    assert fk.active_dims == {(0, 1): [0, 1]}


# --- 2. grid products -----------------------------------------------------------------------------
def _bttb(top):
    """Dense block-Toeplitz matrix of a top row laid out (m1, m2), row-major."""
    m1, m2 = top.shape
    i1, i2 = np.abs(np.subtract.outer(np.arange(m1), np.arange(m1))), \
        np.abs(np.subtract.outer(np.arange(m2), np.arange(m2)))
    return top[i1[:, None, :, None], i2[None, :, None, :]].reshape(m1 * m2, m1 * m2)


def check_grid_products(m1, m2):
    """The device's 2-D grid product of one separable and one isotropic row, as the host layers lay
    them out (FunctionalKernel.eval_kernels_fixed_dim at the grid's Lags), against
    sum_q B_q (x) T_q with T of the separable row np.kron of its two Toeplitz factors: axis 0 of
    the row is the first sorted active dimension.  A transposed layout fails (m1 != m2, the two
    axes on other parameters)."""
    assert m1 != m2
    D, nvec = 3, 3
    rng = np.random.RandomState(100 * m1 + m2)
    ax = [np.linspace(0, 1.0, m1), np.linspace(0, 1.3, m2)]
    mesh = np.meshgrid(*ax, indexing='ij')
    at = Lags(mesh)
    kerns = [Separable(StdPeriodic(1.5, 0.45, active_dims=[0]), Matern32(4.0, active_dims=[1])),
             Matern52(2.5)]
    fk = FunctionalKernel(D=D, lmc_kernels=kerns, lmc_ranks=[1, 2])
    fk.set_input_dim(2)
    tops = np.asarray(fk.eval_kernels_fixed_dim(at, (0, 1)), dtype=float)
    assert tops.shape == (2, m1, m2)
    T = [np.kron(la.toeplitz(StdPeriodicSpec(1.5, 0.45).from_dist(ax[0])),
                 la.toeplitz(Matern32Spec(4.0).from_dist(ax[1]))),
         _bttb(Matern52Spec(2.5).from_dist(np.sqrt(mesh[0] ** 2 + mesh[1] ** 2)))]
    A, kap = [rng.randn(1, D), rng.randn(2, D)], [np.abs(rng.randn(D)) + 0.1 for _ in range(2)]
    Bs = [a.T @ a + np.diag(k) for a, k in zip(A, kap)]
    g = g2._new_grid(m1, m2, D, 2)
    g.set_lmc(tops.reshape(2, -1), A, kap)
    X = rng.randn(nvec, D * m1 * m2)
    got = g.matmat_host(X)
    Xm = X.reshape(nvec, D, m1 * m2)
    want = sum(np.einsum('ab,vbm->vam', B, Xm @ Tq) for B, Tq in zip(Bs, T)).reshape(nvec, -1)
    err = g2._vs_oracle(got, want)
    print('separable grid product %dx%d: error %.2e of max|y| (bar %.0e)' % (m1, m2, err, g2.REL))
    assert err < g2.REL, err
    # the derivative rows are laid out the same way
    grads = fk.eval_kernel_gradients({(0, 1): at})[0]
    want = np.multiply.outer(StdPeriodicSpec(1.5, 0.45).kernel_gradient(ax[0])[1],
                             Matern32Spec(4.0).from_dist(ax[1]))
    assert len(grads) == 3 and grads[1].shape == (m1, m2)
    np.testing.assert_allclose(grads[1], want, rtol=1e-13, atol=1e-300)


# --- 3. the exact likelihood ------------------------------------------------------------------------
def _exact_kernels(P, third=False):
    """(package kernels, closed forms over the P input columns) of check_exact."""
    cols = list(range(P))
    if third:
        k0 = Separable(RBF(2.0, active_dims=[0, 1]), Matern52(1.2, active_dims=[2]))
        r0 = _Sep([(RBFSpec(2.0), [0, 1]), (Matern52Spec(1.2), [2])])
    else:
        k0 = Separable(RBF(2.0, active_dims=[0]), StdPeriodic(1.5, 0.4, active_dims=[1]))
        r0 = _Sep([(RBFSpec(2.0), [0]), (StdPeriodicSpec(1.5, 0.4), [1])])
    k1 = Scaled(Separable(Product(Matern32(3.0), Cosine(2.5), active_dims=[0]),
                          RBF(0.7, active_dims=[1])), 1.7)
    r1 = _Sep([(ProductSpec(Matern32Spec(3.0), CosineSpec(2.5)), [0]), (RBFSpec(0.7), [1])], scale=1.7)
    k2, r2 = Matern52(1.5), _Sep([(Matern52Spec(1.5), cols)])
    return [k0, k1, k2], [r0, r1, r2]


def _pair_lags(Xa, Xb):
    return [np.abs(Xa[:, None, c] - Xb[None, :, c]) for c in range(Xa.shape[1])]


def _dense_cross(refs, Bs, Xa, la_, Xb, lb):
    ro, co = np.repeat(np.arange(len(la_)), la_), np.repeat(np.arange(len(lb)), lb)
    lags = _pair_lags(Xa, Xb)
    return sum(B[np.ix_(ro, co)] * r.value(lags) for B, r in zip(Bs, refs))


def _host_reference(refs, A, Bs, noise, X, lens, y):
    """SciPy's Cholesky, K^-1 by cho_solve and dL/dt = 1/2 sum M dK, M = alpha alpha^T - K^-1, in
    the reference's four families (composite_suite._host_reference's recipe at per-axis lags)."""
    n, D = len(X), len(lens)
    ends = np.cumsum(lens)
    begins = ends - np.asarray(lens)
    lags = _pair_lags(X, X)
    K = _dense_cross(refs, Bs, X, lens, X, lens) + np.diag(np.repeat(noise, lens))
    cf = la.cho_factor(K, lower=True)
    logdet = 2.0 * np.log(np.diag(cf[0])).sum()
    alpha = la.cho_solve(cf, y)
    M = np.outer(alpha, alpha) - la.cho_solve(cf, np.identity(n))

    def block_sums(Kq):
        Pm = M * Kq
        return np.array([[Pm[begins[a]:ends[a], begins[b]:ends[b]].sum() for b in range(D)]
                         for a in range(D)])
    g = dict(coreg_vec=[], coreg_diag=[], kernel=[], noise=None)
    for a_q, B, r in zip(A, Bs, refs):
        S = block_sums(r.value(lags))
        g['coreg_vec'].append(0.5 * np.atleast_2d(a_q).dot(S + S.T))
        g['coreg_diag'].append(0.5 * np.diag(S).copy())
        g['kernel'].append([0.5 * np.sum(B * block_sums(dk)) for dk in r.grads(lags)])
    g['noise'] = np.array([0.5 * np.trace(M[b:e, b:e]) for b, e in zip(begins, ends)])
    return logdet, alpha, g, K


def _exact_problem(n, D, P, third=False):
    rng = np.random.RandomState(n * 7 + D + 31 * P + (5 if third else 0))
    lens = np.full(D, n // D)
    lens[:n - lens.sum()] += 1
    lens = [int(l) for l in lens]
    X = rng.rand(n, P)
    kerns, refs = _exact_kernels(P, third)
    A = [rng.randn(1 + q % 2, D) * 0.6 for q in range(3)]
    kappa = [np.abs(rng.randn(D)) * 0.3 + 0.05 for _ in range(3)]
    noise = 0.05 + 0.1 * rng.rand(D)
    y = rng.randn(n)
    fk = es._fk(D, kerns, A, kappa, noise, P=P)
    return fk, refs, A, fk.coreg_mats(), noise, X, lens, y


def check_exact(n, D, P=2, third=False):
    from runlmc_amd._native import ExactOp, exact_is_separable, exact_separable_descriptors
    from runlmc_amd.lmc import ExactLMCLikelihood
    fk, refs, A, Bs, noise, X, lens, y = _exact_problem(n, D, P, third)
    assert exact_is_separable(fk.kernels)
    nfact, leaves, _, lcols, scaled, scales, nder = exact_separable_descriptors(fk.kernels)
    assert list(nfact) == [2, 3, 1] and nder == [2 if third else 3, 4, 1]
    assert leaves.tolist() == [[0, 3, 0] if third else [0, 2, 0], [1, 4, 0], [3, 0, 0]]
    assert lcols[0].tolist() == ([[0, 1, -1, -1], [2, -1, -1, -1], [-1] * 4] if third else
                                 [[0, -1, -1, -1], [1, -1, -1, -1], [-1] * 4])
    assert lcols[1].tolist() == [[0, -1, -1, -1], [0, -1, -1, -1], [1, -1, -1, -1]]
    assert lcols[2].tolist() == [list(range(P)) + [-1] * (4 - P), [-1] * 4, [-1] * 4]
    assert list(scaled) == [0, 1, 0] and list(scales) == [0.0, 1.7, 0.0]
    logdet, alpha, ref, K = _host_reference(refs, A, Bs, noise, X, lens, y)
    op = ExactOp(n, P)
    op.set(X, lens, fk.kernels, Bs, noise)
    assert op.nder == nder
    es._close(op.dense(), K, 1e-12, 'dense')
    rng = np.random.RandomState(1)
    tl = [3 + d for d in range(D)]
    Xt = rng.rand(sum(tl), P)
    es._close(op.cross(Xt, tl), _dense_cross(refs, Bs, Xt, tl, X, lens), 1e-12, 'cross')
    cuts = np.cumsum(lens)[:-1]
    lik = ExactLMCLikelihood(fk, np.split(X, cuts), np.split(y, cuts))
    assert abs(lik.log_det_K() - logdet) <= 1e-9 * abs(logdet), (lik.log_det_K(), logdet)
    assert [len(g) for g in lik.kernel_gradients()] == nder
    es._compare_to_oracle(lik, ref, alpha, K, 3, rtol=1e-9)
    # the static cross-covariance takes the same door
    Kx = ExactLMCLikelihood.kernel_from_indices(np.split(Xt, np.cumsum(tl)[:-1]), np.split(X, cuts), fk)
    es._close(Kx, _dense_cross(refs, Bs, Xt, tl, X, lens), 1e-12, 'kernel_from_indices')


def _one_distance_sets(P):
    """Kernel sets rl_exact_set_factors takes, positive definite on P input columns (periodic and
    cosine factors of a Euclidean norm are so on the line only: composite_suite's docstring)."""
    if P == 1:
        return [Product(RBF(2.0), StdPeriodic(1.5, 0.4)),
                Scaled(Product(Matern32(3.0), Cosine(2.5), RBF(0.7)), 1.7), Matern52(1.5)]
    return [Product(RBF(2.0), Matern32(1.5)),
            Scaled(Product(Matern52(3.0), RBF(2.5), Matern32(0.7)), 1.7), Matern52(1.5)]


def check_exact_same_columns_bits(P):
    """Every leaf on its kernel's full column list through rl_exact_set_separable: the bits of
    rl_exact_set_factors in K, the cross rows and the gradient sums; then a plain rl_exact_set on
    the same handle gives the plain path's bits."""
    from runlmc_amd import _native
    from runlmc_amd._lib import host_ptr
    n, D = 65, 3
    rng = np.random.RandomState(4 + P)
    lens = [22, 22, 21]
    X = rng.rand(n, P)
    kerns = _one_distance_sets(P)
    for k in kerns:
        k.active_dims = tuple(range(P))
    A = [rng.randn(1, D) * 0.6 for _ in kerns]
    B = np.array([a.T @ a + np.diag(np.abs(rng.randn(D)) * 0.3 + 0.05) for a in A])
    noise = 0.05 + 0.1 * rng.rand(D)
    alpha = rng.randn(n)
    Xt = rng.rand(7, P)
    old = _native.ExactOp(n, P)
    old.set(X, lens, kerns, B, noise)
    nfact, leaves, lparams, scaled, scales, cols, nder = _native.exact_factor_descriptors(kerns)
    lcols = np.full((len(kerns), 3, 4), -1, dtype=np.int32)
    for q in range(len(kerns)):
        lcols[q, :nfact[q]] = cols[q]
    new = _native.ExactOp(n, P)
    L = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    new.lib.call('rl_exact_set_separable', new._h, host_ptr(X), host_ptr(L), D, len(kerns),
                 host_ptr(nfact), host_ptr(leaves), host_ptr(lparams), host_ptr(lcols),
                 host_ptr(scaled), host_ptr(scales), host_ptr(B), host_ptr(noise))
    new.D, new.Q, new.nder = D, len(kerns), nder
    # (the binding builds the same table for such a set)
    assert np.array_equal(_native.exact_separable_descriptors(kerns)[3], lcols)

    def same(a, b):
        assert np.array_equal(a.dense(), b.dense())
        assert np.array_equal(a.cross(Xt, [3, 2, 2]), b.cross(Xt, [3, 2, 2]))
        da = a.cross_device(Xt, [3, 2, 2], 2, 5).cpu().numpy()
        assert np.array_equal(da, b.cross_device(Xt, [3, 2, 2], 2, 5).cpu().numpy())
        assert a.factor() == b.factor()
        for u, v in zip(a.grad_sums(alpha), b.grad_sums(alpha)):
            assert np.array_equal(u, v)
    same(new, old)
    # back to the plain path on the handle that ran the separable one
    plain = [RBF(2.0), Matern32(1.5), Scaled(Matern52(3.0), 0.6)]
    for k in plain:
        k.active_dims = tuple(range(P))
    fresh = _native.ExactOp(n, P)
    fresh.set(X, lens, plain, B, noise)
    new.set(X, lens, plain, B, noise)
    same(new, fresh)
    # ... and through the one-distance factor lists
    new.set(X, lens, kerns, B, noise)
    same(new, old)


class _Recorder:
    """Records the names an ExactOp's library is called with."""

    def __init__(self, lib):
        self.lib, self.names = lib, []

    def __enter__(self):
        real = self.lib.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        self.lib.call = call
        return self

    def __exit__(self, *exc):
        del self.lib.call


def check_exact_limits():
    from runlmc_amd import _native
    from runlmc_amd._lib import host_ptr
    r = lambda d, g=1.0: RBF(g, name='r%d' % d, active_dims=[d])
    # the classes refuse what the device has no place for
    _raises(ValueError, lambda: Separable(Product(RBF(1), RBF(2), active_dims=[0]),
                                          Product(RBF(3), RBF(4), active_dims=[1])), '4')
    _raises(ValueError, lambda: Separable(r(0), RBF(1.0, name='both', active_dims=[0, 1])), 'r0', 'both')
    _raises(ValueError, lambda: Separable(Scaled(r(0), 2.0), r(1)), 'scaled_r0')
    rng = np.random.RandomState(3)
    n, P, D = 17, 2, 1
    X, lens, noise = rng.rand(n, P), [n], np.array([0.1])
    kerns = [Separable(r(0, 2.0), StdPeriodic(1.5, 0.4, active_dims=[1])), Matern52(1.5, active_dims=(0, 1))]
    B = np.array([[[0.5]]] * 2)
    op = _native.ExactOp(n, P)
    with _Recorder(op.lib) as rec:
        op.set(X, lens, kerns, B, noise)
    assert rec.names == ['rl_exact_set_separable'], rec.names
    op.factor()
    # bad column tables: RL_EINVAL as ValueError
    nfact, leaves, lparams, lcols, scaled, scales, _ = _native.exact_separable_descriptors(kerns)
    L = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))

    def call(table):
        op.lib.call('rl_exact_set_separable', op._h, host_ptr(X), host_ptr(L), D, len(kerns),
                    host_ptr(nfact), host_ptr(leaves), host_ptr(lparams), host_ptr(table),
                    host_ptr(scaled), host_ptr(scales), host_ptr(B), host_ptr(noise))
    for q, f, c, col in ((0, 1, 0, P), (1, 0, 1, P + 3), (0, 0, 1, 2 ** 30)):
        bad = lcols.copy()
        bad[q, f, c] = col
        _raises(ValueError, lambda: call(bad), 'beyond P')
    bad = lcols.copy()
    bad[0, 1, :] = -1
    _raises(ValueError, lambda: call(bad), 'without active columns', 'leaf 1 of kernel 0')
    for nf in (0, 4):
        badn = nfact.copy()
        badn[1] = nf
        _raises(ValueError, lambda: op.lib.call(
            'rl_exact_set_separable', op._h, host_ptr(X), host_ptr(L), D, len(kerns), host_ptr(badn),
            host_ptr(leaves), host_ptr(lparams), host_ptr(lcols), host_ptr(scaled), host_ptr(scales),
            host_ptr(B), host_ptr(noise)), '%d factors' % nf)
    lv = leaves.copy()
    lv[0, 1] = 5
    _raises(ValueError, lambda: op.lib.call(
        'rl_exact_set_separable', op._h, host_ptr(X), host_ptr(L), D, len(kerns), host_ptr(nfact),
        host_ptr(lv), host_ptr(lparams), host_ptr(lcols), host_ptr(scaled), host_ptr(scales),
        host_ptr(B), host_ptr(noise)), 'unknown kernel kind 5')
    call(lcols)                     # the handle is still usable
    op.factor()
    # 33 slots: 11 kernels of 2 derivatives each
    many = [Separable(r(0, 1.0 + 0.01 * q), r(1, 2.0)) for q in range(11)]
    _raises(NotImplementedError, lambda: op.set(X, lens, many, np.array([[[0.5]]] * 11), noise), '33')
    op.set(X, lens, many[:10] + [r(0)], np.array([[[0.05]]] * 11), noise)       # 32: accepted
    assert op.Q + sum(op.nder) == 32
    op.factor()
    # a Separable the device cannot take is named, nothing falls back to the host
    wide = Separable(RBF(1.0, name='wide', active_dims=[0, 1, 2, 3, 4]), r(5))
    _raises(NotImplementedError, lambda: _native.exact_separable_descriptors([wide]), 'wide')
    # sets without a Separable keep their calls
    for ks, want in (([RBF(1.0, active_dims=(0, 1)), Matern52(1.5, active_dims=(0,))], 'rl_exact_set'),
                     ([Product(RBF(1.0), Matern32(2.0), active_dims=(0, 1)), RBF(1.0, active_dims=(1,))],
                      'rl_exact_set_factors')):
        assert not _native.exact_is_separable(ks)
        with _Recorder(op.lib) as rec:
            op.set(X, lens, ks, B, noise)
        assert rec.names == [want], rec.names
    assert _native.exact_is_separable([Scaled(RBF.ard([1, 2], [0, 1]), 2.0)])


def check_cross_tiles():
    """rl_exact_cross_dev (k_ex_cross_rows) in tiles of 16 rows, the last one short."""
    from runlmc_amd._native import ExactOp
    n, D, P = 200, 3, 2
    fk, refs, A, Bs, noise, X, lens, y = _exact_problem(n, D, P)
    op = ExactOp(n, P)
    op.set(X, lens, fk.kernels, Bs, noise)
    rng = np.random.RandomState(2)
    tl = [13, 12, 12]
    Xt = rng.rand(37, P)
    whole = op.cross(Xt, tl)
    es._close(whole, _dense_cross(refs, Bs, Xt, tl, X, lens), 1e-12, 'cross')
    for row0 in (0, 16, 32):
        nrows = min(16, 37 - row0)
        got = op.cross_device(Xt, tl, row0, nrows).cpu().numpy()
        assert got.shape == (nrows, n)
        es._close(got, whole[row0:row0 + nrows], 1e-12, 'tile at %d' % row0)


# --- 4. the model ---------------------------------------------------------------------------------
GAMMAS, NU = (6.0, 40.0), 2.0


class _ModelCase:
    pass


@functools.lru_cache(maxsize=None)
def _model_case():
    """The seeded two-input problem and its dense references (computed once, left unchanged)."""
    from runlmc_amd.approx.interpolation import autogrid
    rng = np.random.RandomState(77)
    c = _ModelCase()
    c.D, c.lens = 2, [150, 147]
    c.n = sum(c.lens)
    c.Xs = [rng.rand(l, 2) for l in c.lens]
    c.Ys = [np.sin(5 * X[:, 0] + d) * np.cos(9 * X[:, 1]) + 0.1 * rng.randn(len(X))
            for d, X in enumerate(c.Xs)]
    c.y = np.hstack(c.Ys)
    c.A = [rng.uniform(-1, 1, size=(1, c.D)) for _ in range(2)]
    c.kappa = [0.2 + rng.rand(c.D) for _ in range(2)]
    c.noise = 0.05 + 0.1 * rng.rand(c.D)
    c.Bs = [a.T @ a + np.diag(k) for a, k in zip(c.A, c.kappa)]
    c.refs = [_Sep([(RBFSpec(GAMMAS[0]), [0]), (RBFSpec(GAMMAS[1]), [1])]),
              _Sep([(Matern32Spec(NU), [0, 1])])]
    c.axes = autogrid(c.Xs, None, None, np.array([20, 16]))
    c.shape = tuple(len(a) for a in c.axes)
    assert c.shape == (24, 20)
    m = c.shape[0] * c.shape[1]
    W = np.zeros((c.n, c.D * m))
    start = 0
    for d, X in enumerate(c.Xs):
        W[start:start + len(X), d * m:(d + 1) * m] = ointerp.bicubic_rows(c.axes[0], c.axes[1], X)
        start += len(X)
    c.W = W
    c.Kd = _ski_dense(c, c.refs)
    c.Xt = [rng.rand(5 + d, 2) * 0.9 + 0.05 for d in range(c.D)]
    c.rs = rng.randint(0, 2, (4, c.n)) * 2 - 1
    return c


def _grid_tops(c, refs, grads=False):
    """Dense Toeplitz blocks on the grid, per kernel: of k (grads=False) or of every dk / dtheta."""
    a0, a1 = c.axes[0] - c.axes[0][0], c.axes[1] - c.axes[1][0]
    mesh = np.meshgrid(a0, a1, indexing='ij')
    out = []
    for r in refs:
        if grads:
            out.append([_bttb(g) for g in r.grads(mesh)])
        elif len(r.factors) == 2:
            (f0, _), (f1, _) = r.factors
            out.append(np.kron(la.toeplitz(f0.from_dist(a0)), la.toeplitz(f1.from_dist(a1))))
        else:
            out.append(_bttb(r.value(mesh)))
    return out


def _ski_dense(c, refs, Bs=None, noise=None):
    """W (sum_q B_q (x) T_q) W^T + diag eps."""
    Bs = c.Bs if Bs is None else Bs
    noise = c.noise if noise is None else noise
    Kuu = sum(np.kron(B, T) for B, T in zip(Bs, _grid_tops(c, refs)))
    K = c.W @ Kuu @ c.W.T + np.diag(np.repeat(noise, c.lens))
    return 0.5 * (K + K.T)


def _kernels():
    return [RBF.ard(GAMMAS, [0, 1]), Matern32(NU)]


def _model(prediction='on-the-fly', metrics=False, variance_batch=None, tolerance=1e-4):
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    c = _model_case()
    fk = FunctionalKernel(D=c.D, lmc_kernels=_kernels(), lmc_ranks=[1, 1])
    fk.coreg_vecs, fk.coreg_diags, fk.noise = c.A, c.kappa, c.noise
    np.random.seed(5)
    return InterpolatedLLGP(c.Xs, c.Ys, normalize=False, m=[20, 16], functional_kernel=fk,
                            prediction=prediction, metrics=metrics, trace_iterations=4,
                            tolerance=tolerance, variance_batch=variance_batch)


def check_model_params():
    from runlmc_amd.models.interpolated_llgp import _softplus
    c = _model_case()
    model = _model()
    x = model.param_array.copy()
    want = sum(a.size for a in c.A) + 2 * c.D + (2 + 1) + c.D
    assert x.shape == (want,), (x.shape, want)
    # dists stays the array it was; the mesh is beside it
    (ad,) = model.dists
    assert ad == (0, 1) and type(model.dists[ad]) is np.ndarray and model.dists[ad].shape == c.shape
    assert model.lags[ad].dist is model.dists[ad] and len(model.lags[ad].lags) == 2
    np.testing.assert_array_equal(model.lags[ad].lags[0][:, 0], c.axes[0] - c.axes[0][0])
    np.testing.assert_array_equal(model.lags[ad].lags[1][0, :], c.axes[1] - c.axes[1][0])
    rng = np.random.RandomState(3)
    x1 = x + 0.05 * rng.randn(len(x))
    model.param_array = x1
    np.testing.assert_allclose(model.param_array, x1, rtol=0, atol=1e-12)
    i = sum(a.size for a in c.A) + 2 * c.D
    ard = model._functional_kernel.kernels[0]
    np.testing.assert_allclose([f.inv_lengthscale for f in ard.factors], _softplus(x1[i:i + 2]), rtol=1e-12)
    assert model.gradient.shape == x.shape and np.all(np.isfinite(model.gradient))
    assert len(ard.gradient) == 2 and len(ard.factors[1].gradient) == 1
    # three dimensions per kernel: the model says where such a kernel is usable
    fk = FunctionalKernel(D=c.D, lmc_kernels=[RBF.ard([1, 2, 3], [0, 1, 2])], lmc_ranks=[1])
    X3 = [np.random.RandomState(0).rand(5, 3) for _ in range(c.D)]
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    _raises(NotImplementedError, lambda: InterpolatedLLGP(X3, [x[:, 0] for x in X3], functional_kernel=fk),
            'ExactLMCLikelihood')


def check_model_operator():
    """K~ applied to the identity against W (sum B (x) T) W^T + diag eps."""
    c = _model_case()
    model = _model()
    model._ensure()
    got = model._K.matmat(np.identity(c.n))
    err = np.abs(got - c.Kd).max() / np.abs(c.Kd).max()
    print('separable model operator: error %.2e of the largest entry (bar 1e-11)' % err)
    assert err <= 1e-11, err
    # the rows the likelihood keeps are laid out like dists
    assert model.kernel.materialized_kernels[0].shape == c.shape
    np.testing.assert_allclose(model.kernel.materialized_kernels[0],
                               c.refs[0].value(model.lags[(0, 1)].lags), rtol=1e-14)
    assert all(g.shape == c.shape for g in model.kernel.materialized_grads[0])


def check_model_solve():
    """composite_suite.check_model_solve's rule on the dense K~ of this suite, and the model's own
    alpha at tolerance 1e-12."""
    from runlmc_amd.approx.iterative import Iterative
    c = _model_case()
    xref = la.solve(c.Kd, c.y, assume_a='pos')
    with loo_suite._tight_krylov():
        model = _model(tolerance=1e-12)
        model._ensure()
        alpha = model.kernel.alpha()
    K = model._K
    r = np.linalg.norm(c.y - c.Kd @ alpha)
    print('separable model alpha: residual %.2e, error %.2e' % (r, np.abs(alpha - xref).max()))
    assert r < 1e-8 * np.linalg.norm(c.y), r
    assert np.abs(alpha - xref).max() <= r / c.noise.min() + 1e-12 * np.abs(xref).max()
    x, _, res = Iterative.solve(K, c.y, verbose=True)
    assert res < 1e-4 and np.linalg.norm(c.y - c.Kd @ x) < 1e-4, (res, np.linalg.norm(c.y - c.Kd @ x))
    M = K.preconditioner
    if M is None:
        bound = np.linalg.norm(c.y - c.Kd @ x) / c.noise.min()
        assert np.abs(x - xref).max() <= bound
        return 'krylov'
    bar = 1e-9 if M.exact else 1e-8
    x, _, res = Iterative.solve(K, c.y, verbose=True, tol=bar)
    assert res < bar, res
    es._close(x, xref, bar, 'solve')
    return 'exact' if M.exact else 'preconditioner'


def check_model_gradients():
    """Gradient assembly on the streaming path with fixed probes and dense solves against the
    reference's loops, one dense dK = W (dB (x) T) W^T per parameter:
    dL/dt = (alpha^T dK alpha - mean_i (K^-1 r_i)^T dK r_i) / 2."""
    from parity_suite import _FixedDeriv
    from runlmc_amd.lmc.likelihood import ApproxLMCLikelihood
    c = _model_case()
    model = _model()
    model._ensure()
    fk, K = model._functional_kernel, model._K
    cf = la.cho_factor(c.Kd)
    alpha = la.cho_solve(cf, c.y)
    inv_rs = la.cho_solve(cf, c.rs.T.astype(float)).T
    lik = ApproxLMCLikelihood(fk, K, model.lags, model.interpolants, c.Ys,
                              _FixedDeriv(alpha, c.rs, inv_rs, K.device))
    m = c.shape[0] * c.shape[1]
    Wd = [c.W[:, d * m:(d + 1) * m] for d in range(c.D)]

    def loop(dB, T):
        WT = [w @ T for w in Wd]
        dK = sum(dB[a, b] * WT[a] @ Wd[b].T for a in range(c.D) for b in range(c.D) if dB[a, b] != 0.0)
        tr = np.mean([s @ dK @ r for s, r in zip(inv_rs, c.rs)])
        return 0.5 * (alpha @ dK @ alpha - tr)
    tops, dtops = _grid_tops(c, c.refs), _grid_tops(c, c.refs, grads=True)
    want = dict(coreg_vec=[], coreg_diag=[], kernel=[])
    eye = np.identity(c.D)
    for q in range(2):
        gA = np.zeros_like(c.A[q])
        for i in range(gA.shape[0]):
            for j in range(c.D):
                dB = np.outer(eye[j], c.A[q][i])
                gA[i, j] = loop(dB + dB.T, tops[q])
        want['coreg_vec'].append(gA)
        want['coreg_diag'].append(np.array([loop(np.outer(eye[d], eye[d]), tops[q]) for d in range(c.D)]))
        want['kernel'].append([loop(c.Bs[q], dT) for dT in dtops[q]])
    ends = np.cumsum(c.lens)
    begins = ends - np.asarray(c.lens)
    want['noise'] = np.array([0.5 * (alpha[b:e] @ alpha[b:e] - np.mean([s[b:e] @ r[b:e] for s, r in zip(inv_rs, c.rs)]))
                              for b, e in zip(begins, ends)])
    gv, gd = lik.coreg_vec_gradients(), lik.coreg_diags_gradients()
    gkk, gn = lik.kernel_gradients(), lik.noise_gradient()
    assert [len(g) for g in gkk] == [2, 1]
    scale = max(max(np.abs(a).max() for a in want['coreg_vec']), 1.0)
    err = float(np.abs(gn - want['noise']).max())
    for q in range(2):
        err = max(err, float(np.abs(gv[q] - want['coreg_vec'][q]).max()),
                  float(np.abs(gd[q] - want['coreg_diag'][q]).max()),
                  float(np.abs(np.array(gkk[q]) - np.array(want['kernel'][q])).max()))
    print('separable model gradients: error %.2e of the scale (bar 1e-9)' % (err / scale))
    assert err < 1e-9 * scale, err / scale


def _native_variance(c):
    coreg = np.column_stack([np.square(a).sum(axis=0) for a in c.A]) + np.column_stack(c.kappa)
    return np.repeat(coreg @ np.ones(2) + c.noise, [len(v) for v in c.Xt])


def _exact_dense(c, Xa, la_):
    X = np.vstack(c.Xs)
    return _dense_cross(c.refs, c.Bs, np.vstack(Xa), la_, X, c.lens)


def check_model_exact_prediction():
    c = _model_case()
    model = _model(prediction='exact', metrics=True)
    _, var = model.predict(c.Xt)
    tl = [len(v) for v in c.Xt]
    Kx = _exact_dense(c, c.Xt, tl)
    Kd = _exact_dense(c, c.Xs, c.lens) + np.diag(np.repeat(c.noise, c.lens))
    native = _native_variance(c)
    ref = np.clip(native - np.einsum('ij,ji->i', Kx, la.solve(Kd, Kx.T)), 0, None)
    err = np.abs(np.concatenate(var) - ref).max()
    print('separable exact variances: error %.2e (atol %.2e)' % (err, 1e-8 * native.max()))
    np.testing.assert_allclose(np.concatenate(var), ref, rtol=0, atol=1e-8 * native.max())
    es._close(model.K(), Kd, 1e-12, 'K()')
    got = model.metrics.grad_error
    assert len(got) == 1 and np.isfinite(got[0]), got
    # the host-assembled cross kernel of 'on-the-fly'
    es._close(model._exact_cross_kernel(c.Xt), Kx, 1e-13, '_exact_cross_kernel')


def check_model_tiled_variances():
    c = _model_case()
    mu0, var0 = _model().predict(c.Xt)
    mu1, var1 = _model(variance_batch=5).predict(c.Xt)
    native = _native_variance(c)
    atol = 1e-5 * max(native.max(), 1.0)
    err = np.abs(np.concatenate(var1) - np.concatenate(var0)).max()
    print('separable tiled against host-assembled variances: max difference %.3e (atol %.3e)' % (err, atol))
    np.testing.assert_allclose(np.concatenate(var1), np.concatenate(var0), rtol=0, atol=atol)
    np.testing.assert_array_equal(np.concatenate(mu1), np.concatenate(mu0))
    assert np.all(np.concatenate(var0) > 0) and np.all(np.concatenate(var0) < native)


def check_model_loo():
    """composite_suite.check_model_loo's bars on the dense K~ of this suite."""
    c = _model_case()
    with loo_suite._tight_krylov():
        model = _model(tolerance=1e-12)
        model._ensure()
        Kinv = la.inv(c.Kd)
        alpha, d = Kinv @ c.y, np.diag(Kinv)
        mean_ref, var_ref = c.y - alpha / d, 1.0 / d
        mean_tol = 1e-8 * np.abs(c.y).max()
        var_tol = loo_suite.DIAG_REL * np.max(1.0 / c.noise) / d ** 2
        ends = np.cumsum(c.lens)[:-1]
        sel = np.concatenate([[0, c.n - 1], ends - 1, ends, [7, 23]])
        means, vars_ = model.loo_predict(indices=sel, method='solve', tol=1e-12)
    assert model.loo_stats['method'] == 'solve' and model.loo_stats['nonpositive'] == 0
    em, ev = np.abs(means - mean_ref[sel]).max(), (np.abs(vars_ - var_ref[sel]) / var_tol[sel]).max()
    print('separable loo: mean error %.3e (tol %.3e), variance error / tol %.3e' % (em, mean_tol, ev))
    assert em <= mean_tol and ev <= 1.0, (em, mean_tol, ev)
    assert np.all(vars_ > np.repeat(c.noise, c.lens)[sel])


def check_model_update():
    """A model walked through three parameter updates (GridKernel.update on the live handles)
    against a model built at the last parameters: alpha and the predictive means at
    parity_suite._close's default, both solved to 1e-12 (composite_suite.check_model_update)."""
    from parity_suite import _close
    c = _model_case()
    with loo_suite._tight_krylov():
        walked = _model(tolerance=1e-12)
        x = walked.param_array.copy()
        rng = np.random.RandomState(8)
        for _ in range(3):
            x = x + 0.1 * rng.randn(len(x))
            np.random.seed(5)
            walked.param_array = x
        fresh = _model(tolerance=1e-12)
        fk, src = fresh._functional_kernel, walked._functional_kernel
        fk.coreg_vecs, fk.coreg_diags, fk.noise = src.coreg_vecs, src.coreg_diags, src.noise
        for k, s in zip(fk.kernels, src.kernels):
            k.set_params(s.param_array)
        np.random.seed(5)
        fresh._ensure()
        np.testing.assert_allclose(fresh.param_array, x, rtol=0, atol=1e-12)
        _close(walked.kernel.alpha(), fresh.kernel.alpha())
        mu_a, mu_b = walked.predict(c.Xt)[0], fresh.predict(c.Xt)[0]
    _close(np.concatenate(mu_a), np.concatenate(mu_b))
    # the walked operator is the dense one at the walked parameters
    ard, m32 = src.kernels
    refs = [_Sep([(RBFSpec(f.inv_lengthscale), [i]) for i, f in enumerate(ard.factors)]),
            _Sep([(Matern32Spec(m32.inv_lengthscale), [0, 1])])]
    Kd = _ski_dense(c, refs, src.coreg_mats(), src.noise)
    got = walked._K.matmat(np.identity(c.n))
    assert np.abs(got - Kd).max() <= 1e-11 * np.abs(Kd).max()


def check_model_optimize():
    """Two optimiser steps run through param_array and leave finite parameters and gradients."""
    model = _model()
    x0 = model.param_array.copy()
    model.optimize(max_it=2)
    assert np.all(np.isfinite(model.param_array)) and np.all(np.isfinite(model.gradient))
    assert not np.array_equal(model.param_array, x0)


def check_model_draws():
    """64 seeded posterior draws at 8 test points per output: the sample mean within
    5 sqrt(var / 64) of predict's mean (composite_suite.check_model_draws)."""
    c = _model_case()
    model = _model()
    rng = np.random.RandomState(12)
    Xt = [rng.rand(8, 2) * 0.9 + 0.05 for _ in range(c.D)]
    mu, var = model.predict(Xt)
    f = model.posterior_draws(64, seed=2024)(Xt)
    for d in range(c.D):
        assert f[d].shape == (64, 8)
        latent = var[d] - c.noise[d]
        assert np.all(latent > 0)
        z = np.abs(f[d].mean(axis=0) - mu[d]) / np.sqrt(latent / 64)
        print('output %d: mean z-scores up to %.2f' % (d, z.max()))
        assert z.max() <= 5.0, (d, z)


def check_anisotropy():
    """4096 prior draws of a one-output RBF.ard model on its grid: the empirical correlation
    between two grid points h apart along axis 0 is exp(-gamma_1 h^2 / 2), along axis 1
    exp(-gamma_2 h^2 / 2), each within 5 standard errors sqrt((1 + rho^2) / S) (the variance of a
    Gaussian sample covariance with known zero mean and unit variances); the two targets are
    more than 10 standard errors apart, so an isotropic sampler cannot pass."""
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    from runlmc_amd.approx.pathwise import CLIP_TOL
    S, steps = 4096, 3
    rng = np.random.RandomState(21)
    X = rng.rand(150, 2)
    fk = FunctionalKernel(D=1, lmc_kernels=[RBF.ard(GAMMAS, [0, 1])], lmc_ranks=[1])
    fk.coreg_vecs, fk.coreg_diags, fk.noise = [np.array([[0.8]])], [np.array([0.3])], np.array([0.1])
    np.random.seed(5)
    model = InterpolatedLLGP([X], [np.sin(4 * X[:, 0])], normalize=False, lo=[0.0, 0.0], hi=[1.0, 1.0],
                             m=[16, 16], functional_kernel=fk)
    a0, a1 = model.grid_axes[(0, 1)]
    h = steps * (a0[1] - a0[0])
    assert len(a0) == len(a1) == 20 and abs(steps * (a1[1] - a1[0]) - h) < 1e-15
    rho = [np.exp(-0.5 * g * h * h) for g in GAMMAS]
    se = [np.sqrt((1 + r * r) / S) for r in rho]
    assert abs(rho[0] - rho[1]) > 10 * max(se), (rho, se)
    draws = model.prior_draws(S, seed=11, batch=256)
    (sampler,) = model._pathwise_samplers(16)
    assert all(s.clipped < CLIP_TOL for s in sampler.stats), sampler.stats
    U = draws.grid_draws[(0, 1)].reshape(S, 20, 20)
    k0 = 0.8 ** 2 + 0.3
    i, j = 8, 9
    got = [np.mean(U[:, i, j] * U[:, i + steps, j]) / k0, np.mean(U[:, i, j] * U[:, i, j + steps]) / k0]
    var0 = np.mean(U[:, i, j] ** 2) / k0
    print('anisotropy: h = %.4f, correlations %.4f / %.4f against %.4f / %.4f (se %.4f / %.4f), '
          'variance / k(0) %.4f' % (h, got[0], got[1], rho[0], rho[1], se[0], se[1], var0))
    assert abs(var0 - 1.0) <= 5 * np.sqrt(2.0 / S)
    for g, r, s in zip(got, rho, se):
        assert abs(g - r) <= 5 * s, (g, r, s)
