"""GPU run of the function-draw checks (tests/pathwise_suite.py) on librunlmc_hip.so: k_smp_embed1,
k_smp_cols / k_smp_rows, k_smp_poly_coef with k_lr_expand, k_smp_normal, k_smp_residual and the
model on the device."""
import pytest

import pathwise_suite as pws

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_library():
    from runlmc_amd import _lib
    _lib.use_library(None)
    lib = _lib.get_library()
    assert lib.is_hip, 'GPU tests must run against librunlmc_hip.so'
    return lib


def test_embedding_1d():
    pws.check_embedding_1d()


@pytest.mark.parametrize('case', ['A', 'B'])
def test_ladder(case):
    pws.check_ladder(case)


def test_ladder_exhausted():
    pws.check_ladder_exhausted()


def test_polynomial():
    pws.check_polynomial()


def test_mixed_forms():
    pws.check_mixed_forms()


@pytest.mark.parametrize('D', [1, 3])
@pytest.mark.parametrize('m,kind', pws.TWO_PASS)
def test_transform_paths(m, kind, D):
    pws.check_transform_paths(m, kind, D)


def test_grid_2d():
    pws.check_grid_2d()


def test_grid_2d_limit():
    pws.check_grid_2d_limit()


# ('2d2': two outputs with couplings on a 2-D grid, 1 754 Krylov solves -- minutes on the emulator
# build, which is why tests/test_pathwise_emu.py leaves it out)
@pytest.mark.parametrize('kind', ['1d', '2d', '2d2', 'split'])
def test_posterior_map(kind):
    pws.check_posterior_map(kind)


@pytest.mark.parametrize('name', ['lmc_2d', 'lmc_split'])
def test_zero_noise_mean_golden(name):
    pws.check_zero_noise_mean_golden(name)


def test_noise_moments():
    pws.check_noise_moments()


def test_stream_invariance():
    pws.check_stream_invariance()


def test_model_interface():
    pws.check_model_interface()


def test_model_statistics():
    pws.check_model_statistics()
