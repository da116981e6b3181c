"""GPU run of the 2-D grid checks (tests/grid2d_suite.py) on librunlmc_hip.so: every plan of
the transform kernels a two-dimensional grid can take, the limits of the planner, the 2-D
model on the fused kernels, and seeded random shapes."""
import pytest

import grid2d_suite as gs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_library():
    from runlmc_amd import _lib
    _lib.use_library(None)
    lib = _lib.get_library()
    assert lib.is_hip, 'GPU tests must run against librunlmc_hip.so'
    return lib


@pytest.mark.parametrize('row', gs.LATTICE, ids=gs.lattice_id)
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


@pytest.mark.parametrize('case', sorted(gs.SKI_CASES))
def test_ski_2d_operator(case):
    gs.check_ski_2d_operator(case)


@pytest.mark.parametrize('case,minres', [('A', True), ('B', True), ('C', True), ('A', False)])
def test_ski_2d_solve(case, minres):
    gs.check_ski_2d_solve(case, minres)


@pytest.mark.parametrize('case', sorted(gs.SKI_CASES))
def test_ski_2d_gradients(case):
    gs.check_ski_2d_gradients(case)


def test_chunked_product_2d():
    gs.check_chunked_product_2d()


def test_nd_reduction():
    gs.check_nd_reduction()


@pytest.mark.parametrize('it', range(len(gs.RANDOM_DRAWS)),
                         ids=[gs.lattice_id(d) for d in gs.RANDOM_DRAWS])
def test_random_2d_shapes_vs_oracle(it):
    gs.check_random_2d_shape(it)


def test_random_2d_shapes_cover_embeddings():
    gs.check_random_coverage()
