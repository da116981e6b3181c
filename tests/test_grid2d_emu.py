"""CPU run of the 2-D grid checks (tests/grid2d_suite.py) on the thread-level emulator build of
the same kernel source (tests/emu): the plan lattice, the planner's limits and the wide route,
the chunked two-stream product, the N-D reduction and the smallest of the 2-D models."""
import pytest

import grid2d_suite as gs

# Emulator cut-off: rows of the lattice with L * D <= EMU_MAX_LD run here (L = N1 * N2; a wide
# row counts its one-output child).  Timed on the emulator build: the largest rows of the table
# (L * D = 2^20: 130 x 300, 300 x 130 and 300 x 300) take about 2 s each, oracle and direct
# sum included, so a cut-off of "about 20 s" keeps every row of the table; a row added above 2^20 is left to the GPU run.
EMU_MAX_LD = 1 << 20
EMU_LATTICE = [r for r in gs.LATTICE if r[5] * r[6] * (r[2] if r[2] <= 16 else 1) <= EMU_MAX_LD]


@pytest.fixture(scope='module', autouse=True)
def emu_library():
    from runlmc_amd import _lib, build
    lib = _lib.use_library(build.build_emu())
    assert not lib.is_hip
    yield lib
    _lib.use_library(None)


def test_emulator_set():
    """The emulator keeps at least these rows of the lattice: 2 x 600, 600 x 2, 33 x 65, a
    third-generation row and a wide one."""
    shapes = {r[:3] for r in EMU_LATTICE}
    for need in ((2, 600, 1), (600, 2, 2), (33, 65, 2), (20, 40, 3)):
        assert need in shapes, need
    assert any(r[2] > 16 for r in EMU_LATTICE)


@pytest.mark.parametrize('row', EMU_LATTICE, ids=gs.lattice_id)
def test_plan_lattice(row):
    gs.check_plan_lattice(*row)


@pytest.mark.parametrize('m1,m2,D', gs.ADMITTED)
def test_limits_admitted(m1, m2, D):
    gs.check_limit_shape(m1, m2, D)


@pytest.mark.parametrize('m1,m2,D', gs.WIDE_ROUTE)
def test_limits_wide_route(m1, m2, D):
    gs.check_limit_shape(m1, m2, D)


def test_limits_refused():
    gs.check_refusals()


def test_wide_consumers():
    gs.check_wide_consumers()


def test_chunked_product_2d():
    gs.check_chunked_product_2d()


def test_nd_reduction():
    gs.check_nd_reduction()


# (the 2-D models A and B run their solves on the GPU only: tens of seconds each here)
def test_ski_2d_operator():
    gs.check_ski_2d_operator('C')


def test_ski_2d_solve():
    gs.check_ski_2d_solve('C')


def test_ski_2d_gradients():
    gs.check_ski_2d_gradients('C')
