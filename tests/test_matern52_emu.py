"""CPU run of the Matern-5/2 checks (tests/matern52_suite.py) on the thread-level emulator build
of the same kernel source (tests/emu): the kernel class, the detection of degree-3 rows, the
four-state recurrences and carries of the recursive filter, the exact likelihood's device
formula and the model.  The DPP bodies of the filter kernels run only in the GPU run
(tests/test_matern52_gpu.py)."""
import pytest

import matern52_suite as ms


@pytest.fixture(scope='module', autouse=True)
def emu_library():
    from runlmc_amd import _lib, build
    lib = _lib.use_library(build.build_emu())
    assert not lib.is_hip
    yield lib
    _lib.use_library(None)


def test_kernel_class():
    ms.check_kernel_class()


@pytest.mark.parametrize('m', [601, 700, 2500])
@pytest.mark.parametrize('gamma', [1.0, 3.0, 10.0])
def test_detection(m, gamma):
    ms.check_detection(m, gamma)


@pytest.mark.parametrize('D,Q,m,k', ms.SHAPES)
def test_four_state_products(D, Q, m, k):
    ms.check_four_state(D, Q, m, k)


def test_four_state_products_scan2():
    ms.check_four_state(2, 2, 20011, 2, scan2=True)


@pytest.mark.parametrize('n,D', [(n, D) for n in (17, 65, 200) for D in (1, 3)])
def test_exact(n, D):
    ms.check_exact(n, D)


def test_exact_2d_inputs():
    ms.check_exact(65, 3, P=2)


def test_exact_unknown_kind():
    ms.check_exact_unknown_kind()


def test_model_metrics():
    ms.check_model_metrics()


def test_model_exact_prediction():
    ms.check_model_exact_prediction()


def test_model_tiled_variances():
    ms.check_model_tiled_variances()


def test_model_solve():
    ms.check_model_solve()
