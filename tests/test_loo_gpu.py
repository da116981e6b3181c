"""GPU run of the leave-one-out checks (tests/loo_suite.py) on librunlmc_hip.so: k_dz_diag,
k_loo_accumulate, k_loo_reduce, rl_ski_precond_apply and the model on the device."""
import pytest

import loo_suite as ls

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def hip_library():
    from runlmc_amd import _lib
    _lib.use_library(None)
    lib = _lib.get_library()
    assert lib.is_hip, 'GPU tests must run against librunlmc_hip.so'
    return lib


@pytest.mark.parametrize('D,m_data', [(1, 100), (3, 400), (16, 70)])
@pytest.mark.parametrize('kern', ['rbf', 'periodic'])
def test_inverse_diag(kern, D, m_data):
    ls.check_inverse_diag(kern, D, m_data)


@pytest.mark.parametrize('lens', [(37, 64, 129), (64, 192, 70)])
def test_inverse_diag_borders(lens):
    ls.check_inverse_diag_borders(lens)


def test_precond_diag():
    ls.check_precond_diag()


def test_diag_accumulate():
    ls.check_diag_accumulate()


@pytest.mark.parametrize('which', ['direct', 'precond', 'grid2d'])
def test_probes_estimator(which):
    ls.check_probes_estimator(which)


@pytest.mark.parametrize('which', ['precond', 'grid2d'])
def test_solve_subset(which):
    ls.check_solve_subset(which)


@pytest.mark.parametrize('name,normalize', [('lmc_smooth', False), ('lmc_small', False),
                                            ('lmc_smooth', True)])
def test_model_loo(name, normalize):
    ls.check_model_loo(name, normalize)


def test_loo_reduce():
    ls.check_loo_reduce()


def test_abi_errors():
    ls.check_abi_errors()
