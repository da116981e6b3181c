"""CPU run of the update walks (tests/update_walk_suite.py) on the thread-level emulator build of
the same kernel source (tests/emu): one operator / one model through many parameter states against
fresh ones.  Left to the GPU run (tests/test_update_walk_gpu.py): the batch walk with the solver's
kept workspace (here it runs without, RUNLMC_WS_CACHE_MB=0; the main walk has the same batch
sizes with the workspace kept).  The emulator has no streams and replays a captured graph as a
list of launches, so what the walks say about those is the GPU run's.  Measured on this build:
about 200 s in all -- the main walk 60 s, the smooth model 45 s, the Matern model 26 s, the ragged
walk 25 s, the grid operator's setters up to 25 s, the batch walk 12 s, the stale objects 7 s
(eight rejected states of the main walk run 2 x 10 capped MINRES iterations on the emulated
transform kernels, 6 s each; the models' jump states the same)."""
import pytest

import update_walk_suite as uw


@pytest.fixture(scope='module', autouse=True)
def emu_library():
    from runlmc_amd import _lib, build
    lib = _lib.use_library(build.build_emu())
    assert not lib.is_hip
    yield lib
    _lib.use_library(None)


@pytest.mark.parametrize('which', ['main', 'ragged'])
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
