"""GPU run of the pivoted-Cholesky preconditioner's checks (tests/pivchol_suite.py) on
librunlmc_hip.so: the build kernels, k_pc_project / k_pc_expand on the fp64 matrix cores for
every rank and batch size of the suite, solves, the model, updates and refusals."""
import pytest

import pivchol_suite as pc

pytestmark = pytest.mark.gpu

OPS = ['sep2d', 'grid3d', 'terms', 'wide']


@pytest.fixture(scope='module', autouse=True)
def hip_library():
    from runlmc_amd import _lib
    _lib.use_library(None)
    lib = _lib.get_library()
    assert lib.is_hip, 'GPU tests must run against librunlmc_hip.so'
    pc.operator.cache_clear()
    yield lib
    pc.operator.cache_clear()


@pytest.mark.parametrize('name', OPS)
def test_diagonal(name):
    pc.check_diagonal(name)


@pytest.mark.parametrize('rank', pc.RANKS)
@pytest.mark.parametrize('name', OPS)
def test_factor(name, rank):
    pc.check_factor(name, rank)


def test_rank_clip():
    pc.check_rank_clip()


def test_early_stop():
    pc.check_early_stop()


@pytest.mark.parametrize('rank', pc.RANKS)
@pytest.mark.parametrize('name', OPS)
def test_apply(name, rank):
    pc.check_apply(name, rank)


@pytest.mark.parametrize('name,rank', [('sep2d', 64), ('grid3d', 37), ('terms', 16), ('wide', 64)])
def test_solves(name, rank):
    pc.check_solves(name, rank)


def test_iteration_gain():
    pc.check_iteration_gain()


@pytest.mark.parametrize('which', ['sep2d', 'grid3d'])
def test_model(which):
    pc.check_model(which)


def test_updates():
    pc.check_updates()


def test_refusals():
    assert pc.check_refusals() == 1
