"""CPU run of the polynomial form's policy and depth checks (tests/lr_policy_suite.py) on the
thread-level emulator build of the same kernel source (tests/emu).  The cache hints are no-ops
there; what this run checks is the launcher's dispatch (lr_policy_suite.EMU_VALUES_SHORT) and the
projection with two rows per wave and a ring of four lane-steps (which rows a wave owns, clamped
rows past the end, the ring's first and last requests), bit for bit against the default depth."""
import pytest

import lr_policy_suite as ps


@pytest.fixture(scope='module', autouse=True)
def emu_library():
    from runlmc_amd import _lib, build
    lib = _lib.use_library(build.build_emu())
    assert not lib.is_hip
    yield lib
    _lib.use_library(None)


@pytest.mark.parametrize('m', ps.LENGTHS)
def test_rbf(m):
    ps.check_rbf(m, ps.EMU_VALUES_SHORT if m == ps.LENGTHS[0] else ps.EMU_VALUES, ps.EMU_VIEWS,
                 transforms_all=False)


def test_periodic():
    ps.check_periodic(values=ps.EMU_POLICIES)


def test_accumulate():
    ps.check_accumulate(ps.EMU_POLICIES)
