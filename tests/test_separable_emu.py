"""CPU run of the separable-kernel checks (tests/separable_suite.py) on the thread-level emulator
build of the same kernel source (tests/emu): the Separable / RBF.ard classes and the lag entry
points, the 2-D grid products of separable rows, the exact likelihood on per-leaf distances
(rl_exact_set_separable), the model, leave-one-out and function draws.  The gfx950 bodies run in
tests/test_separable_gpu.py."""
import pytest

import separable_suite as ss


@pytest.fixture(scope='module', autouse=True)
def emu_library():
    from runlmc_amd import _lib, build
    lib = _lib.use_library(build.build_emu())
    assert not lib.is_hip
    yield lib
    _lib.use_library(None)


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
