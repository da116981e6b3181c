"""GPU run of the polynomial form's policy and depth checks (tests/lr_policy_suite.py) on
librunlmc_hip.so: every value of RUNLMC_LR_POLICY (nt loads, nt / sc1 stores, the projection with
two rows per wave and a ring of four) against RUNLMC_LR_POLICY=0 bit for bit, against the transform
kernels, and the sentinels around a view of Y at every base offset, X a view too."""
import pytest

import lr_policy_suite as ps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_library():
    from runlmc_amd import _lib
    _lib.use_library(None)
    lib = _lib.get_library()
    assert lib.is_hip, 'GPU tests must run against librunlmc_hip.so'
    return lib


@pytest.mark.parametrize('m', ps.LENGTHS)
def test_rbf(m):
    ps.check_rbf(m)


def test_periodic():
    ps.check_periodic()


def test_accumulate():
    ps.check_accumulate()
