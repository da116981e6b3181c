"""CPU run of the per-observation noise checks (tests/rownoise_suite.py) on the thread-level
emulator build of the same kernel source (tests/emu): rl_ski_set_noise_rows, the scaled
factorisation of csrc/rl_rownoise.h in modes 1 and 2, rl_exact_set_row_noise and the Python
layers.  The gfx950 bodies run in tests/test_rownoise_gpu.py."""
import pytest

import rownoise_suite as rn


@pytest.fixture(scope='module', autouse=True)
def emu_library():
    from runlmc_amd import _lib, build
    lib = _lib.use_library(build.build_emu())
    assert not lib.is_hip
    yield lib
    _lib.use_library(None)


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
