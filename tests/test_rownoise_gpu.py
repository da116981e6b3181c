"""GPU run of the per-observation noise checks (tests/rownoise_suite.py) on librunlmc_hip.so: the
kernels of csrc/rl_rownoise.h around the gfx950 bodies of k_rp_project / k_dz_mix / k_rp_expand /
k_dz_diag on the scaled table, the exact handle's diagonal, and the Python layers."""
import pytest

import rownoise_suite as rn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_library():
    from runlmc_amd import _lib
    _lib.use_library(None)
    lib = _lib.get_library()
    assert lib.is_hip, 'GPU tests must run against librunlmc_hip.so'
    yield lib


@pytest.mark.parametrize('permuted', [False, True])
def test_product(permuted):
    rn.check_product(permuted)


@pytest.mark.parametrize('kern,rank', [('rbf', 24), ('periodic', 36)])
def test_factor_exact(kern, rank):
    rn.check_factor_exact(kern, rank)


def test_interleaved():
    rn.check_interleaved()


def test_fold_handle():
    rn.check_fold_handle()


def test_fold_model():
    rn.check_fold_model()


def test_precond():
    rn.check_precond()


@pytest.mark.parametrize('kern', ['rbf', 'periodic'])
def test_inverse_diag(kern):
    rn.check_inverse_diag(kern)


def test_exact():
    rn.check_exact()


@pytest.mark.parametrize('which', ['1d', '2d', 'exact'])
def test_model(which):
    rn.check_model(which)


def test_validation():
    rn.check_validation()
