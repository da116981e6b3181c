"""Long-lived handles walked through parameter updates against fresh ones (shared by the CPU run on
the emulator, tests/test_update_walk_emu.py, and the GPU run, tests/test_update_walk_gpu.py; every
function uses whichever native library is active).

A fit creates its operator once and then only calls GridKernel.update() (rl_gridop_set_lmc) and
LMCOperator.update_noise() (rl_ski_set_noise).  Both handles carry state from step to step --
parameter and noise versions, deferred set-time work, the accepted rank, the table F = W Phi, the
factorisation with its mode and its cached failure, two back-offs, the solver's workspace and
captured graph -- and every other check of the suite uses a handle once.  Here ONE operator takes a
sequence of states and is compared after each with an operator built at that state:

  * same reported state (forms, rank, factor mode) -> the same BITS in every observation;
  * different reported state (only while a back-off sits out) -> the form-to-form and solve bars of
    check_polynomial_form / check_direct_solve / check_precond_hi, and the walked handle never
    more permissive than the fresh one;
  * the back-offs rejoin when the comments of rl_host.h / rl_gridop.hip / rl_solve.hip say;
  * once per distinct reported state, and at the end, the dense oracle.

"Update" in those comments counts parameter sets whose set-time work RAN: rl_gridop_set_lmc defers
the verification of the forms to the first product, factorisation or query that needs it
(lr_dirty), so a set that is overwritten before anything asked for the operator neither counts as a
rejection nor uses up a sat-out update.  The walks contain such sets ('silent' states)."""
import time

import numpy as np
import scipy.linalg as la
import torch

from oracle import likelihood as olik
from oracle.kernels import KernelSpec, RBFSpec, Matern32Spec, StdPeriodicSpec
from parity_suite import (_synth_problem_and_oracle, _dense_spd, functional_kernel_for_synth,
                          _env_set, _close)
from matern52_suite import Matern52Spec
import loo_suite

from runlmc_amd._lib import NativeError
from runlmc_amd._native import GridOp
from runlmc_amd.approx.iterative import Iterative
from runlmc_amd.kern.stationary import RBF, Matern32, Matern52, StdPeriodic
from runlmc_amd.lmc.functional_kernel import FunctionalKernel
from runlmc_amd.lmc.grid_kernel import gen_grid_kernel
from runlmc_amd.lmc.likelihood import ApproxLMCLikelihood
from runlmc_amd.lmc.stochastic_deriv import StochasticDerivService

TOL = 1e-8                 # the solves' residual rule (check_direct_solve / check_precond_hi: 1e-8 / 1e-9)
FORM_REL = 1e-12           # one form of a product against another (check_polynomial_form)
SOLVE_REL = 1e-8           # solutions through different factorisations (check_precond_hi)
TRUE_RES = 2e-8            # explicit residual through the oracle's operator (check_direct_solve)
ORACLE_PRODUCT = 1e-11     # a product against the oracle's (check_row_polynomial_form)
ORACLE_LOGDET = 1e-11      # relative (check_direct_solve)
CAP = 10                   # iterations of a solve that has no preconditioner (it never converges here: n
                           # iterations; iterates, counts and residuals are compared as they stand)
AD = (0,)

PKG = {'rbf': RBF, 'matern': Matern32, 'matern52': Matern52, 'periodic': StdPeriodic}
ORA = {'rbf': RBFSpec, 'matern': Matern32Spec, 'matern52': Matern52Spec, 'periodic': StdPeriodicSpec}

# what the walks saw, for the record (printed by the tests)
REPORT = {}


# --- the problems ----------------------------------------------------------------------------------
def _main_problem():
    """synth.make_problem(2, 2, 1, 300): n = 600 on a grid of 304 points -- the smallest size at
    which the polynomial form (>= 96 points), the rank-48 table with D r = 96 and the filter's
    32-point segments are all in play."""
    from runlmc_amd.util import synth
    return synth.make_problem(2, 2, 1, 300, eps=0.1, kern='rbf')


def _ragged_problem(lens=(37, 64, 129)):
    """check_inverse_diag_borders' instance: outputs that end inside a wave, next to a wave's edge
    and inside a workgroup, every output with its own noise."""
    from runlmc_amd.util import synth
    from runlmc_amd.approx.interpolation import autogrid, multi_interpolant
    rng = np.random.RandomState(23)
    p = synth.SynthProblem()
    p.D, p.Q, p.R = len(lens), 2, 1
    p.Xs = [np.sort(rng.rand(n)).reshape(-1, 1) for n in lens]
    p.Ys = [rng.randn(n) for n in lens]
    p.lens, p.n = list(lens), sum(lens)
    p.grid = autogrid(p.Xs, None, None, [150])[0]
    p.grid_dists = p.grid - p.grid[0]
    p.m = len(p.grid)
    p.W = multi_interpolant(p.Xs, p.grid).tocsr()
    p.WT = p.W.transpose().tocsr()
    p.WT.sort_indices()
    p.WT.indices = p.WT.indices.astype(np.int32)
    p.WT.indptr = p.WT.indptr.astype(np.int32)
    p.coreg_vecs = np.array([rng.randn(1, p.D) for _ in range(p.Q)])
    p.coreg_diags = np.array([np.abs(rng.randn(p.D)) + 0.1 for _ in range(p.Q)])
    p.noise = np.array([0.05, 0.2, 0.11, 0.4, 0.07][:p.D])
    p.y = np.hstack(p.Ys)
    return p


def _functional_kernel(p, desc, scale, noise):
    """A new FunctionalKernel, same Q, as check_row_polynomial_form builds its update."""
    fk = FunctionalKernel(D=p.D, lmc_kernels=[PKG[d[0]](*d[1:]) for d in desc], lmc_ranks=[1] * p.Q)
    fk.coreg_vecs = [np.sqrt(scale) * a for a in p.coreg_vecs]
    fk.coreg_diags = [scale * k for k in p.coreg_diags]
    fk.noise = np.array(noise, dtype=float)
    fk.set_input_dim(1)
    return fk


def _oracle(p, desc, scale, noise):
    spec = KernelSpec(p.D, [ORA[d[0]](*d[1:]) for d in desc], [np.sqrt(scale) * a for a in p.coreg_vecs],
                      [scale * k for k in p.coreg_diags], np.array(noise, dtype=float))
    spec.set_input_dim(1)
    return olik.LMCOperatorOracle(spec, p.grid_dists, p.W, p.WT, p.lens)


# --- a state and what is observed in it ---------------------------------------------------------------
class State:
    """kerns: ('rbf', g) / ('matern', g) / ('matern52', g) / ('periodic', g, period) per top row.
    noise: factors on the problem's noise, per output.  silent: applied to the walked operator and
    overwritten by the next state with no product, solve or factorisation in between.
    order: what the walked operator is asked first --
      'product'  the below-gate product, the gate-0 product, factor(), the solve;
      'factor'   factor() as the first call after the update;
      'small'    only the below-gate product (5 vectors at the default gate) before the solve.
    gate: 'set' leaves the walked handle's gate at 0 after the state; 'kept' does not touch the
    gate before the first product (it must still be 0 from the state before: the fresh handle sets
    0 there) -- set_form_gate persists across updates.
    only: 'noise' -- K.update_noise() alone, no gk.update(); 'kernel' -- gk.update() alone (the noise
    is the state before's): each version counter then has to do its work without the other's help.
    batch: systems in the solve (y and fixed +-1 rows).  loud: the noise is large enough for MINRES
    to converge without a preconditioner.  reject: a setter with bad arguments after the state."""

    def __init__(self, name, kerns, scale=1.0, noise=1.0, silent=False, order='product', gate=None,
                 batch=3, loud=False, reject=False, only=None):
        self.only = only
        self.name, self.kerns, self.scale, self.noise = name, kerns, scale, noise
        self.silent, self.order, self.gate, self.batch = silent, order, gate, batch
        self.loud, self.reject = loud, reject


def _host(t):
    return t.cpu().numpy()


def _observe(K, fixed, state, walked):
    """Everything the issue lists, of one operator in one state.  The fresh operator is always asked
    in the plain order."""
    V, Bfull, Wpm = fixed
    ski = K.device_operator()
    g = ski.grid
    o = {}
    order = state.order if walked else 'product'

    def factor():
        ok, ld, cond = ski.factor()
        o['mode'] = ski.factor_mode if ok else 0
        o['reason'] = ski.factor_reason
        o['ld'] = ld if o['mode'] == 1 else None

    def product_default():
        if not (walked and state.gate == 'kept'):
            g.set_form_gate(0 if state.gate == 'kept' else -1)
        o['Y'] = ski.matmat_host(V)

    def product_gate0():
        g.set_form_gate(0)
        o['Y0'] = ski.matmat_host(V)
        g.set_form_gate(0 if state.gate == 'set' else -1)
        o['WT'] = _host(ski.apply_wt(torch.from_numpy(V).to(ski.device)))

    def solve():
        if 'mode' not in o:
            factor()                     # (K.preconditioner asks the same first)
        B = Bfull[:state.batch]
        if o['mode'] != 0 or state.loud:
            # (loud states may run MINRES: ended by the residual rule alone, looked at every 10
            # iterations -- SciPy's own exits stop at 1e-7 here)
            with loo_suite._tight_krylov():
                X, it, res = Iterative.solve(K, B, verbose=True, tol=TOL)
            o['X'], o['it'], o['res'], o['istop'] = np.asarray(X), np.asarray(it), np.asarray(res), None
            o['converged'] = True
        else:
            X, it, res, st = Iterative.solve_device(K, torch.from_numpy(B).to(ski.device), tol=TOL,
                                                    maxiter=CAP)
            o['X'], o['it'], o['res'], o['istop'] = _host(X), np.asarray(it), np.asarray(res), np.asarray(st)
            o['converged'] = False

    steps = dict(product=(product_default, product_gate0, factor, solve),
                 factor=(factor, product_default, product_gate0, solve),
                 small=(product_default, solve, product_gate0))[order]
    for step in steps:
        step()
    o['forms'] = list(g.top_forms()[0])
    o['rank'] = g.form()[0]
    if o['mode'] == 1:
        d, exact = ski.inverse_diag()
        assert exact is True
        o['extra'] = _host(d)
    elif o['mode'] in (2, 3):
        R, ldp = ski.precond_sample(torch.from_numpy(Wpm).to(ski.device))
        o['extra'] = np.concatenate([_host(R).ravel(), [ldp]])
    else:
        o['extra'] = None
    return o


def _same_bits(a, b, key):
    x, y = a[key], b[key]
    if x is None or y is None:
        return x is None and y is None
    return np.array_equal(np.asarray(x), np.asarray(y))


# --- the documented back-offs, restated ---------------------------------------------------------------
class _Backoff:
    """rl_host.h:168-170 / rl_gridop.hip forms_setup: after k rejections in a row the verification
    sits out 0, 1, 3, ... 31 updates.  rl_solve.hip dz_ensure: after k failed factorisations in a
    row the next attempt (of an operator that is not wholly in the polynomial form) comes after
    1, 3, 7 ... 31 updates.  The counts are those comments'."""

    def __init__(self):
        self.rejects = self.lr_skip = 0
        self.streak = self.dz_skip = 0

    def forms(self, any_row_to_verify, fresh_all_pass):
        """True when the walked handle's verification runs in this state."""
        if not any_row_to_verify:
            return True
        if self.lr_skip > 0:
            self.lr_skip -= 1
            return False
        if fresh_all_pass:
            self.rejects = 0
        else:
            self.rejects = min(self.rejects + 1, 6)
            self.lr_skip = (0, 0, 1, 3, 7, 15, 31)[self.rejects]
        return True

    def factor(self, exact, succeeded_if_tried):
        """True when the walked handle attempts its factorisation in this state;
        succeeded_if_tried is a callable (asked only when it does)."""
        if not exact and self.streak > 0 and self.dz_skip > 0:
            self.dz_skip -= 1
            return False
        if succeeded_if_tried():
            self.streak = self.dz_skip = 0
        else:
            self.streak = min(self.streak + 1, 5)
            self.dz_skip = (0, 1, 3, 7, 15, 31)[self.streak]
        return True


# --- 1. the operator walk -----------------------------------------------------------------------------
SMOOTH = [('rbf', 1.0), ('rbf', 10.0)]
SHORT = [('rbf', 4e4), ('rbf', 3e4)]


def main_states():
    n2 = [0.5, 2.0]
    loud = [40.0, 40.0]
    return [
        State('rbf 1,10', SMOOTH),
        State('rbf 55,70: rank up', [('rbf', 55.0), ('rbf', 70.0)], order='factor'),
        State('noise only', [('rbf', 55.0), ('rbf', 70.0)], noise=n2, order='small', batch=39, only='noise'),
        State('couplings only', [('rbf', 55.0), ('rbf', 70.0)], scale=1.7, noise=n2, reject=True, only='kernel'),
        State('one row at 4e4: rejected', [('rbf', 4e4), ('rbf', 10.0)], gate='set'),
        State('smooth at once', SMOOTH, gate='kept', order='product'),
        # two rejections in a row, the second after a set that nothing looked at
        State('short', SHORT),
        State('short, silent', [('rbf', 2e4), ('rbf', 1e4)], silent=True),
        State('short again', [('rbf', 3e4), ('rbf', 2e4)], order='factor'),
        State('smooth after two', SMOOTH, order='small'),
        State('smooth + 1', [('rbf', 1.1), ('rbf', 10.0)], batch=39),
        # filter rows
        State('matern32 + rbf', [('matern', 3.0), ('rbf', 2.0)], order='factor', batch=21),
        State('matern32 + rbf, couplings', [('matern', 3.0), ('rbf', 2.0)], scale=1.7, only='kernel'),
        State('matern32 only', [('matern', 3.0), ('matern', 8.0)], noise=n2),
        State('matern52 + rbf', [('matern52', 3.0), ('rbf', 2.0)], order='small'),
        State('periodic + rbf', [('periodic', 1.0, 1.0), ('rbf', 2.0)], scale=1.7),
        # three rejections in a row (the third after a sat-out update), then smooth for four
        State('short 1', SHORT),
        State('short 2', [('rbf', 3e4), ('rbf', 2e4)], order='factor'),
        State('short 3 (sat out)', SHORT),
        State('short 4', [('rbf', 3e4), ('rbf', 2e4)]),
        State('smooth, sits out 1', SMOOTH, noise=loud, loud=True),
        State('smooth, sits out 2', [('rbf', 1.1), ('rbf', 10.0)], noise=loud, loud=True, order='small'),
        State('smooth, sits out 3', [('rbf', 1.2), ('rbf', 10.0)], order='factor'),
        State('smooth, rejoined', [('rbf', 1.3), ('rbf', 10.0)], scale=1.7),
        State('rbf 1,10 again', SMOOTH),
    ]


def ragged_states():
    per = [0.5, 1.0, 2.0]
    return [
        State('rbf 1,10', SMOOTH),
        State('noise per output', SMOOTH, noise=per, order='factor', only='noise'),
        State('couplings only', SMOOTH, scale=1.7, noise=per, only='kernel'),
        State('rbf 55,70', [('rbf', 55.0), ('rbf', 70.0)], noise=per, order='small', batch=21),
        State('short', SHORT, silent=True),
        State('short', SHORT),
        State('matern32 + rbf', [('matern', 3.0), ('rbf', 2.0)], noise=per),
        State('rbf 1,10 again', SMOOTH),
    ]


def batch_states():
    """Solve batches of 3, 39, 3, 21 systems on one handle (the workspace kept between calls is
    sized by the largest so far), on a direct and on a preconditioned operator."""
    out = []
    for i, b in enumerate((3, 39, 3, 21)):
        out.append(State('rbf batch %d' % b, [('rbf', 1.0 + 0.1 * i), ('rbf', 10.0)], batch=b))
    for i, b in enumerate((3, 39, 3, 21)):
        out.append(State('matern batch %d' % b, [('matern', 3.0 + 0.1 * i), ('rbf', 2.0)], batch=b))
    return out


def check_operator_walk(which='main', env=None):
    """One LMCOperator through `which` list of states (main_states / ragged_states / batch_states)
    against a fresh gen_grid_kernel at every state and the dense oracle.

    Finding (parent commit; fixed with this check): rl_solve_pcg kept its (rho, rho_prev) pairs,
    dz_scal, under the capacity dz_rhs_cap that it shares with rl_solve_direct, which grows dz_part
    and dz_go -- and that capacity -- without dz_scal.  A handle that ran PCG on 3 systems (dz_scal:
    48 bytes), then the direct solver on 39 (capacity 39), then PCG on 21 cleared and wrote 21 pairs
    into room for 3: the main walk's states 'smooth after two' (still sitting out: a preconditioner),
    'smooth + 1' (39 systems, direct) and 'matern32 + rbf' (21 systems).  On the emulator the heap
    was corrupted (glibc: "corrupted double-linked list" two states later); an emulator build with
    guard zones around every device allocation named the buffer.  A fresh handle can never show
    it.  dz_scal has a capacity of its own now (rl_host.h: dz_scal_cap).

    With one refresh removed at a time the walk fails: without ++noise_ver in rl_ski_set_noise, and
    with the dz_eps_ver comparison gone, at 'noise only' (the solve's bits); without ++param_ver in
    set_commit at 'couplings only' (the solve's bits) -- the latter only because that state calls
    gk.update() ALONE: a walk that always calls update_noise() as well, as the model does, cannot
    see a parameter version that stands still, the noise version covers for it."""
    with _env_set(**(env or {})):
        return _operator_walk(which)


def _operator_walk(which):
    p = _ragged_problem() if which == 'ragged' else _main_problem()
    states = dict(main=main_states, ragged=ragged_states, batch=batch_states)[which]()
    rng = np.random.RandomState(0)
    V = rng.randn(5, p.n)
    Bfull = np.vstack([p.y, rng.randint(0, 2, (38, p.n)) * 2.0 - 1])
    Wpm = rng.randint(0, 2, (5, p.n)) * 2.0 - 1
    fixed = (V, Bfull, Wpm)
    interp = {AD: (p.W, p.WT)}
    K = gk = None
    model = _Backoff()
    seen, rep = {}, dict(states=[], bitwise=0, tolerance=0, worst_product=0.0, worst_solve=0.0,
                         worst_residual=0.0, combos=set())
    observed = [s for s in states if not s.silent]
    waiting_forms = waiting_mode = False
    for s in states:
        t0 = time.time()
        noise = p.noise * np.asarray(s.noise, dtype=float)
        fk = _functional_kernel(p, s.kerns, s.scale, noise)
        if K is None:
            K, gks = gen_grid_kernel(fk, {AD: p.grid_dists}, interp, p.lens)
            gk = gks[AD]
        else:
            if s.only != 'noise':
                gk.update(fk, p.grid_dists)
            if s.only != 'kernel':
                K.update_noise(noise, p.lens)
        if s.silent:
            continue
        a = _observe(K, fixed, s, walked=True)
        Kf, _ = gen_grid_kernel(_functional_kernel(p, s.kerns, s.scale, noise), {AD: p.grid_dists},
                                interp, p.lens)
        b = _observe(Kf, fixed, s, walked=False)
        del Kf
        tag = '%s[%s]' % (which, s.name)
        same = a['forms'] == b['forms'] and a['rank'] == b['rank'] and a['mode'] == b['mode']
        scaleY = np.abs(b['Y0']).max()
        dY = max(np.abs(a[k] - b[k]).max() for k in ('Y', 'Y0')) / scaleY
        dX = np.abs(a['X'] - b['X']).max() / np.abs(b['X']).max()
        print('%-38s walked %s r%d mode %d | fresh %s r%d mode %d | dY %.1e dX %.1e it %s/%s  %.1fs'
              % (tag, a['forms'], a['rank'], a['mode'], b['forms'], b['rank'], b['mode'], dY, dX,
                 a['it'][:3].tolist(), b['it'][:3].tolist(), time.time() - t0), flush=True)
        # never more permissive than a fresh handle
        for fa, fb in zip(a['forms'], b['forms']):
            assert not (fa in (1, 2) and fb == 0), (tag, a['forms'], b['forms'])
        assert not (a['mode'] == 1 and b['mode'] != 1), (tag, a['mode'], b['mode'], b['reason'])
        # the back-offs, as documented
        to_verify = any(f != 2 for f in b['forms'])
        verified = model.forms(to_verify, all(f != 0 for f in b['forms']))
        if verified:
            assert a['forms'] == b['forms'] and a['rank'] == b['rank'], \
                (tag, 'the verification was due in this state', a['forms'], b['forms'], a['rank'], b['rank'])
        exact = all(f == 1 for f in a['forms'])
        tried = model.factor(exact, lambda: a['mode'] != 0)
        if tried and a['forms'] == b['forms']:
            assert a['mode'] == b['mode'], (tag, 'the factorisation was due in this state', a['mode'],
                                            b['mode'], a['reason'], b['reason'])
        if same:
            rep['bitwise'] += 1
            for key in ('Y', 'Y0', 'WT', 'X', 'it', 'res', 'istop', 'ld', 'extra'):
                assert _same_bits(a, b, key), (tag, key, 'differs in its bits from a fresh handle')
            # (a handle that sits out its factorisation back-off repeats its LAST reason)
            assert a['reason'] == b['reason'] or not tried, (tag, a['reason'], b['reason'])
        else:
            rep['tolerance'] += 1
            assert not verified or not tried, tag          # (only while a back-off sits out)
            assert dY <= FORM_REL, (tag, dY)
            assert np.array_equal(a['WT'], b['WT']), tag   # (the interpolation knows no forms)
            assert a['converged'] and b['converged'], (tag, 'a state of the walk that differs must converge')
            assert np.all(a['res'] < TOL) and np.all(b['res'] < TOL), (tag, a['res'], b['res'])
            assert dX <= SOLVE_REL, (tag, dX)
            op = _oracle(p, s.kerns, s.scale, noise)
            worst = 0.0
            for o in (a, b):
                for i in range(len(o['X'])):
                    worst = max(worst, np.linalg.norm(Bfull[i] - op.matvec(o['X'][i])))
            assert worst < TRUE_RES, (tag, worst)
            rep['worst_product'] = max(rep['worst_product'], dY)
            rep['worst_solve'] = max(rep['worst_solve'], dX)
            rep['worst_residual'] = max(rep['worst_residual'], worst)
        combo = (tuple(a['forms']), a['rank'], a['mode'])
        rep['combos'].add(combo)
        rep['states'].append((s.name, combo, (tuple(b['forms']), b['rank'], b['mode']), same))
        # the dense oracle: equality with a fresh handle cannot see what both share
        if combo not in seen or s is observed[-1]:
            seen[combo] = s.name
            _against_oracle(p, s, noise, a, fixed, tag)
        if s.reject:
            # a setter that rejects its arguments in the middle of the walk: the operator stays
            # (check_failed_setter_leaves_operator), its versions and deferred work with it
            tops = np.ones((p.Q, p.m))
            bad = np.array([np.eye(p.D), np.triu(np.ones((p.D, p.D)))][:p.Q])
            try:
                gk._op.set_dense(2.0 * tops, bad)
            except (ValueError, NativeError):
                pass
            else:
                raise AssertionError('a coupling matrix that is not symmetric was accepted')
            gk._op.set_form_gate(-1)
            assert np.array_equal(K.device_operator().matmat_host(V), a['Y']), tag
            ok = K.device_operator().factor()[0]
            assert (K.device_operator().factor_mode if ok else 0) == a['mode'], tag
    # the walk ends where a fresh handle is
    last = rep['states'][-1]
    assert last[3], ('the walked handle has not rejoined a fresh one at the end', last)
    rep['combos'] = sorted(rep['combos'])
    print('%s: %d bitwise states, %d tolerance states; worst product %.2e, solve %.2e, residual %.2e'
          % (which, rep['bitwise'], rep['tolerance'], rep['worst_product'], rep['worst_solve'],
             rep['worst_residual']))
    print('%s: (forms, rank, mode) visited: %s' % (which, rep['combos']))
    REPORT[which] = rep
    return rep


def _against_oracle(p, s, noise, a, fixed, tag):
    V, Bfull, Wpm = fixed
    op = _oracle(p, s.kerns, s.scale, noise)
    Kd = _dense_spd(op, p.n)
    for key in ('Y', 'Y0'):
        _close(a[key], V @ Kd, ORACLE_PRODUCT)
    if a['converged']:
        cf = la.cho_factor(Kd)
        _close(a['X'], la.cho_solve(cf, Bfull[:len(a['X'])].T).T, SOLVE_REL)
        if a['mode'] == 1:
            ld_ref = 2.0 * np.log(np.diag(cf[0])).sum()
            assert abs(a['ld'] - ld_ref) <= ORACLE_LOGDET * abs(ld_ref), (tag, a['ld'], ld_ref)
            ref = np.diag(la.inv(Kd))
            bound = loo_suite.DIAG_REL * np.max(1.0 / noise)
            err = np.abs(a['extra'] - ref).max()
            assert err <= bound, (tag, err, bound)


# --- 1b. a bare grid operator between its two setters --------------------------------------------------
def check_gridop_setter_walk():
    """rl_gridop_set_dense and rl_gridop_set_lmc alternating on ONE bare GridOp, smooth and short
    rows, against a fresh GridOp given the same set: the same forms and the same bits (the dense
    setter factors B = sum w a a^T on the host and shares set_commit with the other), and the
    oracle's grid product at 1e-11 of the largest entry."""
    from oracle import operators as ops
    rng = np.random.RandomState(4)
    D, Q, m = 3, 2, 160
    dists = np.linspace(0.0, 1.0, m)
    X = rng.randn(7, D * m)
    g = GridOp(D, m, Q)
    seq = [('lmc', (1.0, 10.0)), ('dense', (2.0, 5.0)), ('lmc', (4e4, 3e4)), ('dense', (1.0, 10.0)),
           ('dense', (4e4, 10.0)), ('lmc', (55.0, 70.0)), ('dense', (55.0, 70.0)), ('lmc', (1.0, 10.0))]
    for i, (setter, gam) in enumerate(seq):
        tops = np.array([RBF(v).from_dist(dists) for v in gam])
        A = [rng.randn(1, D) for _ in range(Q)]
        kap = [np.abs(rng.randn(D)) + 0.1 for _ in range(Q)]
        Bs = ops.coreg_mats(A, kap)
        f = GridOp(D, m, Q)
        for h in (g, f):
            if setter == 'lmc':
                h.set_lmc(tops, A, kap)
            else:
                h.set_dense(tops, np.array(Bs))
            h.set_form_gate(0)
        Yg, Yf = g.matmat_host(X), f.matmat_host(X)
        fg, ff = g.top_forms()[0], f.top_forms()[0]
        print('gridop %d %s %s: walked %s r%d, fresh %s r%d' % (i, setter, gam, fg, g.form()[0], ff, f.form()[0]))
        for a_, b_ in zip(fg, ff):
            assert not (a_ != 0 and b_ == 0), (i, fg, ff)
        if fg == ff and g.form()[0] == f.form()[0]:
            assert np.array_equal(Yg, Yf), (i, setter, np.abs(Yg - Yf).max())
        else:
            assert np.abs(Yg - Yf).max() <= FORM_REL * np.abs(Yf).max(), (i, setter)
        toeps = [ops.BTTBOracle(t) for t in tops]
        _close(Yg[:3], np.array([ops.grid_sum_matvec(Bs, toeps, x) for x in X[:3]]), ORACLE_PRODUCT)
    assert fg == ff


# --- 3. objects that outlive an update ---------------------------------------------------------------
def check_stale_objects():
    """Objects built on an operator and kept across gk.update() / K.update_noise().

    Finding (finding 2; fixed with this check): on the preconditioned-CG path
    StochasticDeriv's log det is deferred -- a closure over the LIVE operator run at the first
    log_det_K().  A likelihood kept across gk.update(couplings x 1.7) answered with the NEW
    operator's estimate next to the old alpha (n = 600, Matern-3/2 rows: -0.5 (log det + ...)
    moved by the 600 log 1.7 / 2-sized difference of the two log dets without any sign of it).
    Now: a deferred value that was never evaluated raises RuntimeError once the operator has
    moved on; one evaluated before the update is kept and returned.  The likelihood's gradients
    (Gram terms read from the operator's handle on first use) follow the same rule, and a
    FactoredInverse reads its kind (K~^-1 / preconditioner) from the handle again after an update."""
    p, fk, K, gk, spec, op = _synth_problem_and_oracle(2, 2, 300, 'matern')
    rs = np.random.RandomState(3).randint(0, 2, (4, p.n)) * 2 - 1
    svc = StochasticDerivService(None, None, len(rs), TOL)

    def lik():
        return ApproxLMCLikelihood(fk, K, {AD: p.grid_dists}, {AD: (p.W, p.WT)}, p.Ys, svc, probes=rs)
    asked, unasked = lik(), lik()
    assert asked.deriv.lanczos is None and asked.deriv.logdet_exact is None     # (deferred)
    ld_old = asked.log_det_K()
    ll_old = asked.log_likelihood()
    Kd = _dense_spd(op, p.n)
    ld_dense = 2.0 * np.log(np.diag(la.cholesky(Kd, lower=True))).sum()
    sem = asked.deriv.logdet_precond[1]
    assert abs(ld_old - ld_dense) <= 4.0 * sem + 1e-9 * abs(ld_dense), (ld_old, ld_dense, sem)
    M_old = K.preconditioner
    assert M_old is not None and not M_old.exact
    gk.update(functional_kernel_for_synth(p, scale=1.7), p.grid_dists)
    # evaluated before the update: kept
    assert asked.log_det_K() == ld_old and asked.log_likelihood() == ll_old
    # never evaluated: no longer answerable for the parameters it was built for
    for call in (unasked.log_det_K, unasked.log_likelihood, unasked.kernel_gradients,
                 unasked.noise_gradient):
        try:
            got = call()
        except RuntimeError as e:
            assert 'update' in str(e), str(e)
        else:
            raise AssertionError('%s answered %r for an operator that has moved on (the kept '
                                 'likelihood said %r before the update)' % (call.__name__, got, ld_old))
    assert unasked.normal_quadratic() == asked.normal_quadratic()       # (alpha is the object's own)
    # a likelihood of the new state is whole again, and differs as the dense log det does
    spec.coreg_vecs = [np.sqrt(1.7) * a for a in spec.coreg_vecs]
    spec.coreg_diags = [1.7 * k for k in spec.coreg_diags]
    op2 = olik.LMCOperatorOracle(spec, p.grid_dists, p.W, p.WT, p.lens)
    Kd2 = _dense_spd(op2, p.n)
    ld2 = 2.0 * np.log(np.diag(la.cholesky(Kd2, lower=True))).sum()
    new = lik()
    got2 = new.log_det_K()
    sem2 = new.deriv.logdet_precond[1]
    assert abs(got2 - ld2) <= 4.0 * sem2 + 1e-9 * abs(ld2), (got2, ld2, sem2)
    print('stale objects: log det %.6f (sem %.2e) before, %.6f (sem %.2e) after the update; dense %.6f / %.6f'
          % (ld_old, sem, got2, sem2, ld_dense, ld2))
    assert abs(ld2 - ld_dense) > 10.0 * (sem + sem2)            # (the two are far apart: the check can see)
    # the same for a noise update
    kept = lik()
    K.update_noise(p.noise * np.array([0.5, 2.0]), p.lens)
    try:
        kept.log_det_K()
    except RuntimeError:
        pass
    else:
        raise AssertionError('a deferred log det answered after update_noise')
    K.update_noise(p.noise, p.lens)

    # FactoredInverse across an update that changes the factor mode: Matern rows (mode 2) -> smooth
    # rows (mode 1) -> short rows (no factorisation)
    assert K.device_operator().factor()[0] and K.device_operator().factor_mode == 2
    M = K.preconditioner
    assert M.exact is False
    smooth = _functional_kernel(p, SMOOTH, 1.0, p.noise)
    gk.update(smooth, p.grid_dists)
    Kd3 = _dense_spd(_oracle(p, SMOOTH, 1.0, p.noise), p.n)
    cf3 = la.cho_factor(Kd3)
    ld3 = 2.0 * np.log(np.diag(cf3[0])).sum()
    B = torch.from_numpy(np.vstack([p.y, rs[0].astype(float)])).to(K.device)
    assert M.exact is True, 'the kept FactoredInverse still calls K~^-1 a preconditioner'
    assert abs(M.logdet() - ld3) <= ORACLE_LOGDET * abs(ld3)
    est = M.logdet_estimate(tol=TOL)
    assert est[0] == M.logdet() and est[1] == 0.0
    X, it, res, st = M.solve(B, tol=TOL)
    Mf = K.preconditioner
    Xf, itf, resf, stf = Mf.solve(B, tol=TOL)
    assert np.array_equal(_host(X), _host(Xf)) and np.array_equal(it, itf) and np.array_equal(st, stf)
    _close(_host(X), la.cho_solve(cf3, _host(B).T).T, SOLVE_REL)
    # ... and back: exact -> preconditioner
    gk.update(functional_kernel_for_synth(p), p.grid_dists)
    assert Mf.exact is False
    X, it, res, st = Mf.solve(B, tol=TOL)
    assert np.all(st == 10) and np.all(res < TOL), (st, res)       # (rl_solve_pcg's exit, not rl_solve_direct's)
    _close(_host(X), la.solve(Kd, _host(B).T, assume_a='pos').T, SOLVE_REL)
    try:
        Mf.logdet()
    except ValueError as e:
        assert 'preconditioner' in str(e) or 'polynomial' in str(e), str(e)
    else:
        raise AssertionError('an exact log det from a preconditioner')
    # ... and to an operator without any factorisation
    gk.update(_functional_kernel(p, SHORT, 1.0, p.noise), p.grid_dists)
    for call in (lambda: Mf.exact, lambda: Mf.solve(B, tol=TOL), lambda: Mf.logdet_estimate(tol=TOL)):
        try:
            call()
        except RuntimeError as e:
            assert 'K.preconditioner' in str(e), str(e)
        else:
            raise AssertionError('a kept FactoredInverse answered for an operator without a factorisation')
    assert K.preconditioner is None

    # K.preconditioner taken before and after a noise-only update: the log dets differ by the
    # dense oracle's difference
    gk.update(smooth, p.grid_dists)
    before = K.preconditioner
    ld_b = before.logdet()
    noise2 = p.noise * np.array([0.5, 2.0])
    K.update_noise(noise2, p.lens)
    after = K.preconditioner
    ld_a = after.logdet()
    Kd4 = Kd3 + np.diag(np.repeat(noise2 - p.noise, p.lens))
    ld4 = 2.0 * np.log(np.diag(la.cholesky(Kd4, lower=True))).sum()
    assert abs(ld_b - ld3) <= ORACLE_LOGDET * abs(ld3) and abs(ld_a - ld4) <= ORACLE_LOGDET * abs(ld4)
    assert abs((ld_a - ld_b) - (ld4 - ld3)) <= ORACLE_LOGDET * (abs(ld3) + abs(ld4)), (ld_a - ld_b, ld4 - ld3)
    assert before.logdet() == ld_a               # (the kept one works on the live handle: the new noise)


# --- 2. the model walk -------------------------------------------------------------------------------
MODEL_TOL = 1e-8


def _new_model(kind):
    """'smooth': Case('lmc_smooth') (three outputs, RBF / periodic / RBF rows, n = 540: the direct
    solver).  'matern': the synthetic Matern-3/2 problem of check_precond_diag (n = 600:
    preconditioned CG, the log det deferred).  Both as parity_suite._model_for wraps them, with
    solves at 1e-8 and four probes."""
    import copy
    from cases import Case
    from parity_suite import functional_kernel_for
    from runlmc_amd.models.interpolated_llgp import InterpolatedLLGP
    from runlmc_amd.util import synth
    if kind == 'smooth':
        c = Case('lmc_smooth')
        fk = copy.deepcopy(functional_kernel_for(c))
        Xs = [np.asarray(x).reshape(len(x), c.P) for x in c.Xs]
        Ys, m = [np.array(y) for y in c.Ys], [len(a) - 4 for a in c.grid_axes]
    else:
        p = synth.make_problem(2, 2, 1, 300, kern='matern')
        fk = copy.deepcopy(synth.functional_kernel(p))
        Xs, Ys, m = [x.copy() for x in p.Xs], [y.copy() for y in p.Ys], [p.m - 4]
    return InterpolatedLLGP(Xs, Ys, normalize=False, m=m, functional_kernel=fk, trace_iterations=4,
                            tolerance=MODEL_TOL)


def _kernel_index(model, q):
    pos = 0
    for name, holder, _, _ in model._param_blocks():
        size = len(holder.param_array) if hasattr(holder, 'set_params') else holder.size
        if name == 'kern%d' % q:
            return pos
        pos += size
    raise KeyError(q)


def _scaled(model, x, q, factor):
    """x with kernel q's first parameter (an inverse length scale: 1 / l^2 for the RBF, so 30 x in
    l is 900 x here; 1 / l for the Matern rows) multiplied by `factor`, in the optimiser's space."""
    from runlmc_amd.models.interpolated_llgp import _softplus, _softplus_inv
    out = x.copy()
    i = _kernel_index(model, q)
    out[i] = _softplus_inv(_softplus(x[i]) * factor)
    return out


def _model_state(model):
    ski = model._K.device_operator()
    ok = ski.factor()[0]
    return list(ski.grid.top_forms()[0]), ski.grid.form()[0], ski.factor_mode if ok else 0


def _model_observe(model, kind, Xt, what, k):
    """The observations named in `what`, in that order.  'pre' is the precompute mode (one solve per
    grid point: the smooth model only, its solver is the direct one), with variance_batch None in
    even states and 100 in odd ones (the cached nu is one per parameter set)."""
    o = {}
    for w in what:
        if w == 'lik':
            o['ll'], o['ld'], o['nq'] = model.log_likelihood(), model.log_det_K(), model.normal_quadratic()
            pre = getattr(model.kernel.deriv, 'logdet_precond', None)
            o['sem'] = pre[1] if pre is not None else 0.0
        elif w == 'nq':
            o['nq'] = model.normal_quadratic()
        elif w == 'grad':
            o['grad'] = model.gradient.copy()
        elif w in ('fly', 'flyb', 'pre'):
            model.prediction = 'precompute' if w == 'pre' else 'on-the-fly'
            model.variance_batch = {'fly': None, 'flyb': 3, 'pre': None if k % 2 == 0 else 100}[w]
            mu, var = model.predict(Xt)
            o[w] = np.concatenate(mu + var)
            model.prediction, model.variance_batch = 'on-the-fly', None
        elif w == 'loo':
            idx = None if kind == 'smooth' else np.array([0, 299, 300, 599, 17, 411])
            with loo_suite._tight_krylov():
                mu, var = model.loo_predict(indices=idx, tol=MODEL_TOL)
                o['looll'] = model.loo_log_likelihood(indices=idx, tol=MODEL_TOL)
            o['loo'] = np.concatenate([np.ravel(np.concatenate(mu)) if idx is None else mu,
                                       np.ravel(np.concatenate(var)) if idx is None else var])
            o['loo_method'] = model.loo_stats['method']
        elif w == 'draws':
            o['draws'] = np.concatenate(model.posterior_draws(size=4, seed=11)(Xt), axis=1)
    return o


def check_model_walk(kind):
    """One InterpolatedLLGP through param_array settings against a model built at each setting:
    the vectors of a short AdaDelta run on the walked model itself, then hand-made jumps.  Smooth
    model: one RBF length scale 30 x shorter (that row is rejected; factor mode 1 -> 2), a second
    row's after it (two rejections in a row) and back -- the
    state in which the walked model still sits out its back-off, on the transform kernels with a
    preconditioner where a fresh model solves directly -- and the first vector again.  Matern
    model: both length scales 30 x and 40 x shorter (no factorisation; the second sits out the
    factorisation's back-off) and back.  np.random.seed before both models, so that the probes
    agree.  The walked model is asked for another subset in another order from state to state
    (predict before the gradient, no predict at all, ...), the fresh one for the same things in one
    fixed order.  In the jump states the solves are capped (no preconditioner: n iterations) and
    only y^T alpha and the gradient are compared.

    Same forms, rank and factor mode: the same bits.  Else: y^T alpha at 1e-7 (alpha at 1e-8), the
    log det at 4 standard errors of the estimate + 1e-9 (check_logdet_preconditioned), gradients
    and predictions at 1e-5 of the largest entry (check_model_prediction / predict_suite),
    leave-one-out at 1e-7."""
    from runlmc_amd.models.optimization import AdaDelta
    walked = _new_model(kind)
    rng = np.random.RandomState(9)
    Xt = [np.sort(rng.rand(4 + d, 1), axis=0) * 0.9 + 0.05 for d in range(walked.output_dim)]
    x0 = walked.param_array.copy()
    trail = []

    def neg_grad(xx):
        trail.append(xx.copy())
        walked.param_array = xx
        return -walked.gradient
    np.random.seed(1)
    AdaDelta(max_it=3).opt(x0.copy(), neg_grad)
    x3 = trail[-1]
    light = ['nq', 'grad']       # (no log det: sixteen more solves on the transform kernels)
    if kind == 'smooth':
        # (30 x in l is 900 x in the RBF's 1 / l^2; rows 0 and 2 are the RBF rows)
        j1 = _scaled(walked, x3, 0, 900.0)
        j2 = _scaled(walked, j1, 2, 900.0)
        everything = ['lik', 'grad', 'fly', 'flyb', 'pre', 'loo', 'draws']
        xs = [('adadelta 1', trail[0], everything), ('adadelta 2', trail[1], ['fly', 'draws', 'grad', 'lik']),
              ('adadelta 3', x3, ['loo', 'lik', 'grad']),
              ('jump', j1, light), ('second jump', j2, light),
              ('back, sitting out', x3, ['fly', 'grad', 'lik']),
              ('first again', trail[0], ['pre', 'lik', 'grad', 'loo', 'draws'])]
    else:
        # (Matern rows stay in the filter form whatever their length scale; 30 x shorter, the
        # polynomial subspace holds too little of them and the operator has no preconditioner.
        # The handle then sits out one update before it tries again: the second jump)
        j1 = _scaled(walked, _scaled(walked, x3, 0, 30.0), 1, 30.0)
        j2 = _scaled(walked, _scaled(walked, x3, 0, 40.0), 1, 40.0)
        everything = ['lik', 'grad', 'fly', 'flyb', 'loo', 'draws']
        xs = [('adadelta 1', trail[0], everything), ('adadelta 3', x3, ['fly', 'draws', 'grad', 'lik']),
              ('jump', j1, light), ('second jump', j2, light),
              ('back', x3, ['loo', 'lik', 'grad']), ('first again', trail[0], everything)]
    rep = dict(bitwise=0, tolerance=0, states=[], worst={})
    for k, (name, x, what) in enumerate(xs):
        t0 = time.time()
        fresh = _new_model(kind)
        capped = 'jump' in name
        for model in (walked, fresh):
            model._deriv_service._maxiter = CAP if capped else 0
            np.random.seed(100 + k)
            model.param_array = x
        sa, sb = _model_state(walked), _model_state(fresh)
        if sa[2] == 0 or sb[2] == 0:
            # no preconditioner: MINRES would run its n iterations in every prediction solve
            assert capped and what == light, (name, sa, sb)
        a = _model_observe(walked, kind, Xt, what, k)
        fixed_order = ['lik', 'nq', 'grad', 'fly', 'flyb', 'pre', 'loo', 'draws']
        b = _model_observe(fresh, kind, Xt, [w for w in fixed_order if w in what], k)
        same = sa == sb
        print('model %s[%s] walked %s | fresh %s | %s  %.1fs' % (kind, name, sa, sb, what, time.time() - t0),
              flush=True)
        for fa, fb in zip(sa[0], sb[0]):
            assert not (fa in (1, 2) and fb == 0), (name, sa, sb)
        assert not (sa[2] == 1 and sb[2] != 1), (name, sa, sb)
        rep['states'].append((name, sa, sb, same))
        if same:
            rep['bitwise'] += 1
            for key in a:
                assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), \
                    (kind, name, key, 'differs in its bits from a fresh model', a[key], b[key])
            continue
        rep['tolerance'] += 1

        def rel(key):
            d = np.abs(np.asarray(a[key]) - np.asarray(b[key])).max() / max(np.abs(np.asarray(b[key])).max(), 1e-300)
            rep['worst'][key] = max(rep['worst'].get(key, 0.0), d)
            return d
        if 'nq' in a:
            assert rel('nq') <= 1e-7, (name, a['nq'], b['nq'])         # (y . alpha, alpha at 1e-8)
        if 'ld' in a:
            slack = 4.0 * (a['sem'] + b['sem']) + 1e-9 * abs(b['ld'])
            assert abs(a['ld'] - b['ld']) <= slack, (name, a['ld'], b['ld'], slack)
            assert abs(a['ll'] - b['ll']) <= 0.5 * slack + 1e-7 * abs(b['nq']), (name, a['ll'], b['ll'])
            rep['worst']['ld'] = max(rep['worst'].get('ld', 0.0), abs(a['ld'] - b['ld']) / abs(b['ld']))
        for key in ('grad', 'fly', 'flyb', 'pre'):
            if key in a:
                assert rel(key) <= 1e-5, (name, key, rel(key))
        if 'loo' in a:
            assert a['loo_method'] == b['loo_method'] or kind == 'smooth', (a['loo_method'], b['loo_method'])
            assert rel('loo') <= 1e-7, (name, rel('loo'))
        # (no draws here: a row in another form maps the same normal variates to another function
        # of the same distribution -- pathwise_suite compares covariances, not draws)
        assert 'draws' not in a, name
    assert rep['states'][-1][3], ('the walked model has not rejoined a fresh one', rep['states'][-1])
    print('model %s: %d bitwise states, %d tolerance states, worst relative differences %s'
          % (kind, rep['bitwise'], rep['tolerance'], rep['worst']))
    REPORT['model ' + kind] = rep
    return rep
