"""GPU run of the separable-kernel checks (tests/separable_suite.py) on librunlmc_hip.so: the 2-D
grid products of separable rows, k_ex_assemble / k_ex_cross_rows / k_ex_grad_tiles on per-leaf
distances (rl_exact_set_separable; against rl_exact_set_factors bit for bit where the leaves share
their kernel's columns), the model, leave-one-out and function draws on the device."""
import pytest

import separable_suite as ss

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_library():
    from runlmc_amd import _lib
    _lib.use_library(None)
    lib = _lib.get_library()
    assert lib.is_hip, 'GPU tests must run against librunlmc_hip.so'
    return lib


def test_classes():
    ss.check_classes()


@pytest.mark.parametrize('m1,m2', [(5, 7), (33, 20), (64, 65)])
def test_grid_products(m1, m2):
    ss.check_grid_products(m1, m2)


@pytest.mark.parametrize('n,D', [(n, D) for n in (17, 65, 200) for D in (1, 3)])
def test_exact(n, D):
    ss.check_exact(n, D, P=2)


def test_exact_three_inputs():
    ss.check_exact(65, 3, P=3, third=True)


@pytest.mark.parametrize('P', [1, 2])
def test_exact_same_columns_bits(P):
    ss.check_exact_same_columns_bits(P)


def test_exact_limits():
    ss.check_exact_limits()


def test_cross_tiles():
    ss.check_cross_tiles()


def test_model_params():
    ss.check_model_params()


def test_model_operator():
    ss.check_model_operator()


def test_model_solve():
    ss.check_model_solve()


def test_model_gradients():
    ss.check_model_gradients()


def test_model_exact_prediction():
    ss.check_model_exact_prediction()


def test_model_tiled_variances():
    ss.check_model_tiled_variances()


def test_model_loo():
    ss.check_model_loo()


def test_model_update():
    ss.check_model_update()


def test_model_optimize():
    ss.check_model_optimize()


def test_model_draws():
    ss.check_model_draws()


def test_anisotropy():
    ss.check_anisotropy()
