"""GPU run of the update walks (tests/update_walk_suite.py) on librunlmc_hip.so: one operator / one
model through many parameter states against fresh ones -- captured graphs, the solver's kept
workspace and the matrix-core kernels are the device's own here."""
import pytest

import update_walk_suite as uw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_library():
    from runlmc_amd import _lib
    _lib.use_library(None)
    lib = _lib.get_library()
    assert lib.is_hip, 'GPU tests must run against librunlmc_hip.so'
    return lib


@pytest.mark.parametrize('which', ['main', 'ragged', 'batch'])
def test_operator_walk(which):
    uw.check_operator_walk(which)


def test_operator_walk_no_workspace_cache():
    uw.check_operator_walk('batch', env=dict(RUNLMC_WS_CACHE_MB=0))


def test_gridop_setter_walk():
    uw.check_gridop_setter_walk()


@pytest.mark.parametrize('kind', ['smooth', 'matern'])
def test_model_walk(kind):
    uw.check_model_walk(kind)


def test_stale_objects():
    uw.check_stale_objects()
