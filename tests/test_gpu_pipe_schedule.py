"""GPU: the wave-pipelined pass with its wavefronts' marches padded in front (xinv_tiles.h: xinv_pipe_*) against the
coloured-ordering oracle and the single-wavefront kernel, bit for bit.

Tile heights of 10, 12, 14 and 16 rows are 2, 4, 6 and 0 (mod 8): every padding of the marches -- none, in front only,
in front with the ring slots flipped -- with top and bottom tiles whose rows are clamped to the slice and a short last
block; rows_per_tile = -3 splits the rows evenly (12 / 14 / 14 and 18 / 20 / 20 rows).

Against the single-wavefront kernel (no_pipe = 1): S, flags[0] and flags[2] bit for bit; flags[1], the relative change of
the norm, to the bar of test_gpu_parity.assert_same (1e-12 absolute + 1e-9 relative) -- the two kernels cut the slice into
different tiles and add the norm's partial sums in a different order, a few ulp of each norm."""
import functools

import numpy as np
import pytest

from util import rand2d, run_oracle, run_hip_batched
from test_gpu_parity import COLOUR_2, PATH_FUSED, _seed, _uniform2d, _uniform2d_all, assert_same

pytestmark = pytest.mark.gpu

NSW = 26                                              # six four-sweep passes and a two-sweep tail


@functools.lru_cache(maxsize=None)
def _case(kind, BCy, BCx, shape):
    """Three members with their own coefficients and their own masks, the oracle's results and the
    single-wavefront kernel's: computed once per (form, boundaries, shape), read-only afterwards."""
    yc, xc = shape
    uni = {'std2d': _uniform2d, 'gen2d': _uniform2d_all}[kind]          # per-row A, C / A, C, D, E, F
    ps = [uni(rand2d(kind, yc, xc, BCy, BCx, 0, 1, seed=_seed(('pipesched', kind, BCy, BCx, shape, m))))
          for m in range(3)]
    ref = [run_oracle(p, NSW, 1e-9, COLOUR_2) for p in ps]
    S0, f0, st0 = run_hip_batched(ps, NSW, 1e-9, path=PATH_FUSED, sweeps_per_launch=4, no_pipe=1)
    assert st0['pipelined'] == 0, st0
    return ps, ref, S0, f0


@pytest.mark.parametrize('BCy,BCx', [('fixed', 'periodic'), ('extend', 'periodic'), ('extend', 'fixed')])
@pytest.mark.parametrize('shape', [(40, 300), (58, 257)])              # (257 columns, periodic: the seam variants)
@pytest.mark.parametrize('kind', ['std2d', 'gen2d'])
@pytest.mark.parametrize('rows', [10, 12, 14, 16, -3])
def test_front_padded_marches_equal_the_oracle_and_the_single_wavefront_pass(rows, kind, shape, BCy, BCx):
    ps, ref, S0, f0 = _case(kind, BCy, BCx, shape)
    for fr in (-1, 1):                                # the forcing re-read from memory / riding the LDS ring
        for skip in (0, 1):
            kw = dict(path=PATH_FUSED, pipe_fr=fr, rows_per_tile=rows)
            if skip:
                kw['force_tile_skip'] = 1
            S, fl, st = run_hip_batched(ps, NSW, 1e-9, **kw)
            assert st['pipelined'] == 1 and st['sweeps_per_launch'] == 4, st
            what = 'front-padded %s %r rows %d fr %d skip %d' % (kind, shape, rows, fr, skip)
            for m in range(3):
                assert_same(S[m], fl[m], ref[m][0], ref[m][1], '%s member %d' % (what, m))
            assert np.array_equal(S, S0), what
            assert np.array_equal(fl[:, 2], f0[:, 2]) and np.array_equal(fl[:, 0], f0[:, 0]), what
            assert np.all(np.abs(fl[:, 1] - f0[:, 1]) <= 1e-12 + 1e-9 * np.abs(f0[:, 1])), what


def test_front_padded_marches_stop_inside_a_pass():
    """The tolerance is met in sweep 10, the second of the third pass (tiles of 14 rows: padding in front, slots
    flipped): the oracle's stopping sweep and its bits, and the single-wavefront kernel's."""
    p = _uniform2d(rand2d('std2d', 40, 300, 'fixed', 'periodic', 0, 1, seed=7))
    So, flo = run_oracle(p, 500, 2e-4, COLOUR_2)
    assert 2 < flo[2] < 499 and (flo[2] + 1) % 4 != 0
    S0, f0, st0 = run_hip_batched([p], 500, 2e-4, path=PATH_FUSED, sweeps_per_launch=4, no_pipe=1)
    assert st0['pipelined'] == 0, st0
    for fr in (-1, 1):
        S, fl, st = run_hip_batched([p], 500, 2e-4, path=PATH_FUSED, rows_per_tile=14, pipe_fr=fr)
        assert st['pipelined'] == 1 and st['sweeps_per_launch'] == 4, st
        assert_same(S[0], fl[0], So, flo, 'front-padded, early stop, fr %d' % fr)
        assert st['sweeps_max'] == flo[2] + 1
        assert np.array_equal(S, S0) and fl[0][2] == f0[0][2] and fl[0][0] == f0[0][0]
        assert abs(fl[0][1] - f0[0][1]) <= 1e-12 + 1e-9 * abs(f0[0][1])
