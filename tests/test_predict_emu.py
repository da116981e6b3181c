"""CPU run of the tiled predictive variances' checks (tests/predict_suite.py) on the thread-level
emulator build of the same kernel source (tests/emu): row groups and windows of
k_ex_cross_rows, the two-stage reduction, the engine and the model's variance_batch keyword."""
import pytest

import predict_suite as pr


@pytest.fixture(scope='module', autouse=True)
def emu_library():
    from runlmc_amd import _lib, build
    lib = _lib.use_library(build.build_emu())
    assert not lib.is_hip
    yield lib
    _lib.use_library(None)


@pytest.mark.parametrize('n,nt,D', [(n, nt, D) for n in pr.CROSS_N for nt in pr.CROSS_NT
                                    for D in (1, 3)])
def test_cross_rows(n, nt, D):
    pr.check_cross_rows(n, nt, D)


def test_cross_rows_2d_inputs():
    pr.check_cross_2d()


def test_cross_rows_split_active_dims():
    pr.check_cross_split()


def test_row_dots():
    pr.check_row_dots()


@pytest.mark.parametrize('batch', pr.BATCHES)
@pytest.mark.parametrize('mode', ['on-the-fly', 'precompute'])
@pytest.mark.parametrize('name', ['lmc_small', 'lmc_2d'])
def test_model(name, mode, batch):
    pr.check_model(name, mode, batch)


@pytest.mark.parametrize('batch', pr.BATCHES)
def test_model_split_active_dims(batch):
    pr.check_model_split(batch)


def test_host_path_not_taken(monkeypatch):
    pr.check_host_path_not_taken(monkeypatch)


def test_errors():
    pr.check_errors()


def test_engine_index_list_and_log():
    pr.check_engine_subset()
