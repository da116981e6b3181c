"""CPU run of the three-dimensional grid checks (tests/grid3d_suite.py) on the thread-level
emulator build of the same kernel source (tests/emu): the tricubic interpolant, k_lead_fwd /
k_lead_inv around the children's 2-D products, the refusals, the SKI operator, solves, gradients
and the model, update walk and variances included (on the suite's small problem, a 5 x 6 x 7 grid:
the emulator walks every thread).  The gfx950 bodies run in tests/test_grid3d_gpu.py on the
9 x 10 x 11 problem, which also holds the checks that are minutes of emulator time and add no
kernel path here: the other two kernel sets of the operator and gradient checks, the 'precompute'
variance mode (one solve per grid point) and the optimiser steps."""
import pytest

import grid3d_suite as g3


@pytest.fixture(scope='module', autouse=True)
def emu_library():
    from runlmc_amd import _lib, build
    lib = _lib.use_library(build.build_emu())
    assert not lib.is_hip
    g3.use_problem('small')
    yield lib
    g3.use_problem('full')
    _lib.use_library(None)


def test_tricubic():
    g3.check_tricubic()


@pytest.mark.parametrize('row', g3.LATTICE, ids=g3.lattice_id)
def test_plan_lattice3(row):
    g3.check_plan_lattice3(row)


@pytest.mark.parametrize('row', [g3.LATTICE[5], g3.LATTICE[10]], ids=g3.lattice_id)
def test_top_products(row):
    g3.check_top_products(row)


def test_unit_columns():
    g3.check_unit_columns3()


def test_update_bits():
    g3.check_update_bits()


def test_refusals():
    g3.check_refusals()


def test_ski_operator():
    g3.check_ski_operator('mix')


def test_ski_solve():
    g3.check_ski_solve()


def test_two_terms():
    g3.check_two_terms()


def test_model_params():
    g3.check_model_params()


def test_model_solve():
    g3.check_model_solve()


def test_model_gradients():
    g3.check_model_gradients('mix')


def test_model_exact_prediction():
    g3.check_model_exact_prediction()


def test_model_variances():
    g3.check_model_variances(precompute=False)


def test_model_loo():
    g3.check_model_loo()


def test_model_update():
    g3.check_model_update()


def test_model_draws_refuse():
    g3.check_model_draws_refuse()
