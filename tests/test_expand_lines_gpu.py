"""GPU run of the whole-line expansion's checks (tests/expand_lines_suite.py) on librunlmc_hip.so:
k_lr_expand_lines against k_lr_expand bit for bit, against the transform kernels, and the
sentinels around a view at every base offset."""
import pytest

import expand_lines_suite as es

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_library():
    from runlmc_amd import _lib
    _lib.use_library(None)
    lib = _lib.get_library()
    assert lib.is_hip, 'GPU tests must run against librunlmc_hip.so'
    return lib


@pytest.mark.parametrize('kern', ['rbf', 'periodic'])
@pytest.mark.parametrize('m', es.LENGTHS)
def test_products(m, kern):
    es.check_products(m, kern)


def test_accumulate():
    es.check_accumulate()
