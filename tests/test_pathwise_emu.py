"""CPU run of the function-draw checks (tests/pathwise_suite.py) on the thread-level emulator build
of the same kernel source (tests/emu): the embedding kernels of both transform paths, the
polynomial rows, the noise generator, Matheron's rule and the model."""
import pytest

import pathwise_suite as pws


@pytest.fixture(scope='module', autouse=True)
def emu_library():
    from runlmc_amd import _lib, build
    lib = _lib.use_library(build.build_emu())
    assert not lib.is_hip
    yield lib
    _lib.use_library(None)


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


@pytest.mark.parametrize('kind', ['1d', '2d', 'split'])
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
