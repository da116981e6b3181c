"""CPU run of the exact dense likelihood's checks (tests/exact_suite.py) on the thread-level
emulator build of the same kernel source (tests/emu): index arithmetic, tile edges, split-k
reductions and the host logic.  The matrix-core bodies of k_ex_gemm run only in the GPU run
(tests/test_exact_gpu.py)."""
import pytest

import exact_suite as es


@pytest.fixture(scope='module', autouse=True)
def emu_library():
    from runlmc_amd import _lib, build
    lib = _lib.use_library(build.build_emu())
    assert not lib.is_hip
    yield lib
    _lib.use_library(None)


def test_golden_small():
    es.check_golden_small()


def test_deterministic():
    es.check_deterministic()


@pytest.mark.parametrize('n,D', [(n, D) for n in (1, 17, 64, 65, 129, 200) for D in (1, 3)
                                 if n >= D])
def test_tile_edges(n, D):
    es.check_tile_edges(n, D)


def test_2d_inputs():
    es.check_2d()


def test_split_active_dims():
    es.check_split()


def test_not_positive_definite():
    es.check_not_positive_definite()


def test_errors():
    es.check_errors()


@pytest.mark.parametrize('name', ['lmc_small', 'lmc_2d'])
def test_model_exact_prediction(name):
    es.check_model_exact_prediction(name)


def test_model_metrics():
    es.check_model_metrics()


def test_model_metrics_declined():
    es.check_model_metrics_declined()
