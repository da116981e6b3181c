"""CPU run of the pivoted-Cholesky preconditioner's checks (tests/pivchol_suite.py) on the
thread-level emulator build of the same kernel source (tests/emu): the scalar bodies of
k_pc_project / k_pc_expand, every build kernel, the host maps and the Python layers, on the small
problems and low ranks (the emulator walks every thread).  The gfx950 bodies, the larger ranks
and the iteration comparison run in tests/test_pivchol_gpu.py."""
import pytest

import grid3d_suite as g3
import pivchol_suite as pc


@pytest.fixture(scope='module', autouse=True)
def emu_library():
    from runlmc_amd import _lib, build
    lib = _lib.use_library(build.build_emu())
    assert not lib.is_hip
    g3.use_problem('small')
    pc.operator.cache_clear()
    yield lib
    pc.operator.cache_clear()
    g3.use_problem('full')
    _lib.use_library(None)


@pytest.mark.parametrize('name', ['grid3d', 'wide'])
def test_diagonal(name):
    pc.check_diagonal(name)


@pytest.mark.parametrize('name,rank', [('grid3d', 5), ('grid3d', 16), ('terms', 5), ('wide', 37)])
def test_factor(name, rank):
    pc.check_factor(name, rank)


def test_rank_clip():
    pc.check_rank_clip()


@pytest.mark.parametrize('name,rank', [('grid3d', 5), ('wide', 16)])
def test_apply(name, rank):
    pc.check_apply(name, rank, nvecs=(1, 3, 17))


def test_solves():
    pc.check_solves('grid3d', 16)


def test_early_stop():
    pc.check_early_stop()


def test_refusals():
    assert pc.check_refusals() in (0, 1)
