"""GPU run of the three-dimensional grid checks (tests/grid3d_suite.py) on librunlmc_hip.so:
k_lead_fwd / k_lead_inv for every N0 around the children's 2-D products, the refusals, the SKI
operator, solves, gradients and the model on the device."""
import pytest

import grid3d_suite as g3

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_library():
    from runlmc_amd import _lib
    _lib.use_library(None)
    lib = _lib.get_library()
    assert lib.is_hip, 'GPU tests must run against librunlmc_hip.so'
    return lib


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


@pytest.mark.parametrize('kind', ['iso', 'mix', 'ard'])
def test_ski_operator(kind):
    g3.check_ski_operator(kind)


def test_ski_solve():
    g3.check_ski_solve()


def test_two_terms():
    g3.check_two_terms()


def test_model_params():
    g3.check_model_params()


def test_model_solve():
    g3.check_model_solve()


@pytest.mark.parametrize('kind', ['mix', 'ard'])
def test_model_gradients(kind):
    g3.check_model_gradients(kind)


def test_model_exact_prediction():
    g3.check_model_exact_prediction()


def test_model_variances():
    g3.check_model_variances()


def test_model_loo():
    g3.check_model_loo()


def test_model_update():
    g3.check_model_update()


def test_model_optimize():
    g3.check_model_optimize()


def test_model_draws_refuse():
    g3.check_model_draws_refuse()
