"""GPU run of the composite-kernel checks (tests/composite_suite.py) on librunlmc_hip.so: the grid
products of composite rows, k_ex_assemble / k_ex_cross_rows / k_ex_grad_tiles at three factors
(and at one, against rl_exact_set), the model, leave-one-out and function draws on the device."""
import pytest

import composite_suite as cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_library():
    from runlmc_amd import _lib
    _lib.use_library(None)
    lib = _lib.get_library()
    assert lib.is_hip, 'GPU tests must run against librunlmc_hip.so'
    return lib


def test_classes():
    cs.check_classes()


@pytest.mark.parametrize('m', [601, 2500])
@pytest.mark.parametrize('k', [1, 3])
def test_grid_products(m, k):
    cs.check_grid_products(m, k)


@pytest.mark.parametrize('n,D', [(n, D) for n in (17, 65, 200) for D in (1, 3)])
def test_exact(n, D):
    cs.check_exact(n, D)


def test_exact_2d_inputs():
    cs.check_exact(65, 3, P=2)


def test_exact_cosine_alone():
    cs.check_exact_cosine_alone()


def test_exact_limits():
    cs.check_exact_limits()


def test_exact_old_path():
    cs.check_exact_old_path()


def test_model_params():
    cs.check_model_params()


def test_model_metrics():
    cs.check_model_metrics()


def test_model_exact_prediction():
    cs.check_model_exact_prediction()


def test_model_tiled_variances():
    cs.check_model_tiled_variances()


def test_model_solve():
    cs.check_model_solve()


def test_model_update():
    cs.check_model_update()


def test_model_loo():
    cs.check_model_loo()


def test_model_draws():
    cs.check_model_draws()
