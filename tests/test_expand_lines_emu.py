"""CPU run of the whole-line expansion's checks (tests/expand_lines_suite.py) on the thread-level
emulator build of the same kernel source (tests/emu): which thread owns which slot, the rows of
a class, liveness of the first and the last column block."""
import pytest

import expand_lines_suite as es


@pytest.fixture(scope='module', autouse=True)
def emu_library():
    from runlmc_amd import _lib, build
    lib = _lib.use_library(build.build_emu())
    assert not lib.is_hip
    yield lib
    _lib.use_library(None)


@pytest.mark.parametrize('kern', ['rbf', 'periodic'])
@pytest.mark.parametrize('m', es.LENGTHS)
def test_products(m, kern):
    es.check_products(m, kern)


def test_accumulate():
    es.check_accumulate()
