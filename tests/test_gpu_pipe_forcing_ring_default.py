"""k_pipe2d just above the planner's switch to the forcing through the LDS ring (xinv_tiles.h: xinv_pipe_forcing_ring,
80 MB of streams per launch): one 2800 x 1200 lat-lon Poisson slice with the land mask, 80.6 MB -- a size the planner
gave the other path until the switch moved.  The default choice, the path forced either way and the single-wavefront
kernel return the coloured oracle's field bit for bit, for a whole number of passes with a tail and for a tolerance that
stops inside a pass."""
import numpy as np
import pytest

import util
from util import run_oracle

pytestmark = pytest.mark.gpu

COLOUR_2 = 2
NY, NX, SWEEPS = 1200, 2800, 10                           # two four-sweep passes and a two-sweep tail


@pytest.fixture(scope='module')
def case():
    from xinvert_amd import synthetic
    q = synthetic.member(synthetic.poisson_latlon(NY, NX, mask=True), 0)
    assert NY * NX * 24.0 > 8.0e7 > 900 * 1800 * 24.0
    So, flo = run_oracle(q, SWEEPS - 1, 0.0, COLOUR_2)
    hist = [run_oracle(q, n, 0.0, COLOUR_2)[1][1] for n in (5, 6)]
    return q, So, flo, hist


@pytest.mark.parametrize('fr', [0, -1, 1])
def test_default_and_forced_forcing_paths_equal_the_oracle(case, fr):
    q, So, flo, _ = case
    S, fl, st = util.run_hip_dev([q], SWEEPS - 1, 0.0, pipe_fr=fr)
    assert st['path'] == 2 and st['pipelined'] == 1 and st['sweeps_per_launch'] == 4, st
    nbad = int((S[0] != So).sum())
    assert nbad == 0, '%d points differ from the oracle' % nbad
    assert fl[0][2] == flo[2] == SWEEPS - 1 and fl[0][0] == flo[0] == 0
    assert abs(fl[0][1] - flo[1]) <= 1e-12, (fl[0][1], flo[1])      # (the project's bound: summation order of the norm)


def test_default_path_stops_inside_a_pass_where_the_oracle_stops(case):
    q, _, _, hist = case
    tol = 0.5 * (hist[0] + hist[1])                       # first sweep whose change is below: loop index 6, sweep 3 of pass 2
    So, fo = run_oracle(q, 40, tol, COLOUR_2)
    assert fo[2] == 6, (fo, hist)
    S, fl, st = util.run_hip_dev([q], 40, tol)
    assert st['pipelined'] == 1, st
    assert fl[0][2] == fo[2] and np.array_equal(S[0], So), (fl, fo)
