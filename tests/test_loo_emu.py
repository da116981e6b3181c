"""CPU run of the leave-one-out checks (tests/loo_suite.py) on the thread-level emulator build of
the same kernel source (tests/emu): k_dz_diag with its border waves, k_loo_accumulate,
k_loo_reduce, rl_ski_precond_apply and the model.  Left to the GPU run (tests/test_loo_gpu.py): the
2-D grid operator of check_probes_estimator (45 s on this build) and of check_solve_subset (57 s) --
MINRES to 1e-10 on the emulated 2-D transform kernels; neither runs a kernel of csrc/rl_loo.h that
the other cases here do not.  The rest takes about 100 s, the longest case 22 s."""
import pytest

import loo_suite as ls


@pytest.fixture(scope='module', autouse=True)
def emu_library():
    from runlmc_amd import _lib, build
    lib = _lib.use_library(build.build_emu())
    assert not lib.is_hip
    yield lib
    _lib.use_library(None)


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


@pytest.mark.parametrize('which', ['direct', 'precond'])
def test_probes_estimator(which):
    ls.check_probes_estimator(which)


@pytest.mark.parametrize('which', ['precond'])
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
