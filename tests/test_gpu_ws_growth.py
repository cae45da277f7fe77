"""Workspace buffers that grow and are then reused by a smaller call, in one process: the direct 1-D solve's planes and
overflow words, the pinned control-block mirror of the 1-D sweeps, and the activity map and tile lists of masked-tile
skipping.  Small call, larger call (every buffer is freed and allocated again), the small call once more -- each bit for
bit against its model."""
import numpy as np
import pytest

import std1d_model as M1
import tridiag_model as MT
import util
from util import rand2d, run_hip_batched, run_oracle
from xinvert_amd import _lib

pytestmark = pytest.mark.gpu
UNDEF = util.U
COLOUR_2 = 2                                                # (oracle.COLOUR_2)


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb])


def members_1d(nb, xc, seed):
    """nb members of the 1-D form: A shared, B, F and the first guess per member, some masks at the ends."""
    rng = np.random.default_rng(seed)
    A, B = rng.uniform(0.5, 1.5, xc), rng.uniform(-0.5, -0.1, (nb, xc))
    F, S0 = rng.standard_normal((nb, xc)), rng.standard_normal((nb, xc)) * 0.1
    F[1::4, 0] = UNDEF
    F[2::4, xc - 1] = UNDEF
    return S0, A, B, F


def solve_1d(S0, A, B, F, BCx, mxLoop, tol, **opt):
    """xinv_standard_1d_f64_batched on host arrays -> (S [nbatch, xc], flags [nbatch, 3])"""
    L = _lib.require_gpu()
    S = np.array(S0, dtype=np.float64)
    nb, xc = S.shape
    fl = np.tile([0.0, 1.0, 0.0], (nb, 1))
    rc = L.xinv_standard_1d_f64_batched(*[_lib.hptr(np.ascontiguousarray(v)) for v in (S, A, B, F)], nb,
                                        _lib.strides_arg([xc, 0, xc, xc]), xc, 1.0, _lib.bc(BCx), 0.49, 1.5, UNDEF,
                                        _lib.hptr(fl), mxLoop, tol, _lib.options(**opt))
    _lib.check(rc)
    return S, fl


def test_direct_1d_planes_and_overflow_words_grow_and_are_reused():
    xc = 5
    # (3 systems, one plane; 70: across the 64-system chunk, periodic: three planes; 3 again in the grown buffers)
    for nb, BCx in ((3, 'fixed'), (70, 'periodic'), (3, 'fixed')):
        S0, A, B, F = members_1d(nb, xc, 100 + nb)
        Sm, flm = MT.direct_solve(S0, A, B, F, BCx, 0.49, UNDEF)
        S, fl = solve_1d(S0, A, B, F, BCx, 7, 1e-3, path=_lib.PATH_DIRECT1D)
        assert _lib.last_stats()['path'] == _lib.PATH_DIRECT1D
        assert bits_equal(S, Sm) and bits_equal(fl, flm), (nb, BCx)


def test_sweeps_1d_control_block_mirror_grows_and_is_reused():
    xc = 9
    for nb in (2, 130, 2):
        S0, A, B, F = members_1d(nb, xc, 200 + nb)
        S, fl = solve_1d(S0, A, B, F, 'extend', 12, 1e-3, sweeps_per_launch=5)      # (three launches, polls between them)
        assert _lib.last_stats()['path'] == _lib.PATH_WAVE1D
        for m in range(nb):
            Sm, flm = M1.rb_solve(S0[m], A, B[m], F[m], 'extend', 0.49, 1.5, UNDEF, 12, 1e-3)
            assert bits_equal(S[m], Sm) and bits_equal(fl[m], flm), (nb, m)


def test_tile_skip_activity_map_and_lists_grow_and_are_reused():
    def member(yc, xc, seed):
        p = rand2d('std2d', yc, xc, 'fixed', 'periodic', 0, 0, seed=seed)
        p['coefs'][-1][:yc // 2] = UNDEF                    # half of the forcing: whole row blocks of tiles never change
        p['S0'][:yc // 2] = 0.25
        return p

    got = []
    for p in (member(24, 40, 1), member(72, 200, 2), member(24, 40, 1)):
        S, fl, st = run_hip_batched([p], 30, 1e-5, path=_lib.PATH_FUSED, rows_per_tile=-4, force_tile_skip=1)
        assert st['path'] == _lib.PATH_FUSED and st['masked_tile_pct'] > 0, st
        So, flo = run_oracle(p, 30, 1e-5, COLOUR_2)
        # (as tests/test_gpu_parity.py's skip tests: S, the overflow flag and the loop count exactly, the norm to rounding)
        assert np.array_equal(S[0], So) and fl[0][0] == flo[0] and fl[0][2] == flo[2], (p['S0'].shape, fl, flo)
        assert abs(fl[0][1] - flo[1]) <= 1e-12 + 1e-9 * abs(flo[1]), (fl, flo)
        got.append((S, fl))
    assert np.array_equal(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1])
