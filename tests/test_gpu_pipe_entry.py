"""GPU: the entry of the wave-pipelined pass takes a tile's geometry from a record built with the plan (xinv_tiles.h:
PipeTileRec -- strip, owned rows, steps of the march, origin of the lane map) instead of deriving it in every workgroup
of every launch.  Every case forces k_pipe2d with the existing options and compares S bit for bit, and the loop index, with
the oracle's coloured ordering; flags[1] to 1e-12.

The smallest shapes at which each field of a record can go wrong:
  6 x 16 periodic            one strip wider than the grid (the lane map wraps the row several times), one tile;
  14 x 240, 46 x 240         three strips, the last owning 16 columns; tile heights 14 and 46, whose marches pad in front by
                             counts that differ in the ring-slot flip; fixed and periodic x; 'extend' on the taller one;
  90 x 128, 12 / 44 rows     top, inner and bottom tiles, rows clamped to the slice;
  96 x 352 with a land block a tile list with idle entries and a non-empty skip list -- and without: one record per tile,
                             the same for every member; two members with different masks: the records differ per member;
  37 x 241 periodic          the seam variant (the ring layout's strips, the heavy-first dispatch order);
  46 x 240 general form      per-row A, C, D, E, F;
  a stop on sweep 2 of a     S is the oracle's stopping sweep: the launches queued behind the one that stopped return at
  four-sweep pass            the entry, before they touch anything -- for a member of a batch whose other member runs on
                             for many more passes as well;
  a resident plan            solved twice, and again after xinv_plan_refresh with another mask: the records are rebuilt."""
import functools

import numpy as np
import pytest

from util import rand2d, run_oracle, run_hip_batched
from test_gpu_parity import COLOUR_2, PATH_FUSED, _seed, _uniform2d, _uniform2d_all

pytestmark = pytest.mark.gpu

NSW = 10                                              # two four-sweep passes and a tail of two or three sweeps


def same(S, fl, So, flo, what):
    assert np.array_equal(S, So), '%s: S differs at %d points' % (what, int((S != So).sum()))
    assert fl[2] == flo[2] and fl[0] == flo[0], (what, fl, flo)
    assert abs(fl[1] - flo[1]) <= 1e-12, (what, fl, flo)


@functools.lru_cache(maxsize=None)
def _problem(kind, yc, xc, BCy, BCx, land=None, seed=0):
    """Per-row coefficients (the pipelined forms), a random mask, optionally a block of land; with the oracle's result."""
    uni = {'std2d': _uniform2d, 'gen2d': _uniform2d_all}[kind]
    p = uni(rand2d(kind, yc, xc, BCy, BCx, 0, 1, seed=_seed(('pipeentry', kind, yc, xc, BCy, BCx, seed))))
    if land:
        y0, y1, x0, x1 = land
        p['coefs'][-1][y0:y1, x0:x1] = p['undef']
    return p, run_oracle(p, NSW, 0.0, COLOUR_2)


def _run(ps, mx, tol, **kw):
    S, fl, st = run_hip_batched(list(ps), mx, tol, path=PATH_FUSED, **kw)
    assert st['pipelined'] == 1 and st['sweeps_per_launch'] == 4, st
    return S, fl, st


@pytest.mark.parametrize('kind,yc,xc,BCy,BCx,rows', [
    ('std2d', 6, 16, 'fixed', 'periodic', 0),
    ('std2d', 14, 240, 'fixed', 'fixed', 14), ('std2d', 14, 240, 'fixed', 'periodic', 14),
    ('std2d', 46, 240, 'fixed', 'fixed', 46), ('std2d', 46, 240, 'fixed', 'periodic', 46),
    ('std2d', 46, 240, 'extend', 'periodic', 46), ('std2d', 46, 240, 'extend', 'fixed', 46),
    ('std2d', 90, 128, 'fixed', 'periodic', 12), ('std2d', 90, 128, 'fixed', 'fixed', 44),
    ('std2d', 37, 241, 'fixed', 'periodic', 0), ('std2d', 37, 241, 'fixed', 'periodic', 12),
    ('gen2d', 46, 240, 'fixed', 'periodic', 46), ('gen2d', 46, 240, 'extend', 'fixed', 14),
])
def test_record_fields_on_their_smallest_shapes(kind, yc, xc, BCy, BCx, rows):
    p, (So, flo) = _problem(kind, yc, xc, BCy, BCx)
    for fr in (-1, 1):                                # the forcing re-read from memory / riding the LDS ring
        S, fl, st = _run([p], NSW, 0.0, rows_per_tile=rows, pipe_fr=fr)
        same(S[0], fl[0], So, flo, '%s %dx%d %s/%s rows %d fr %d' % (kind, yc, xc, BCy, BCx, rows, fr))


LAND = (24, 72, 112, 224)                             # rows 24..71 of strip 1: two whole tiles of four 24-row blocks


@pytest.mark.parametrize('kind', ['std2d', 'gen2d'])
def test_tile_list_with_skipped_tiles_and_identity_records(kind):
    pl, (Sl, fll) = _problem(kind, 96, 352, 'fixed', 'periodic', land=LAND)
    pn, (Sn, fln) = _problem(kind, 96, 352, 'fixed', 'periodic')
    S, fl, st = _run([pl], NSW, 0.0, rows_per_tile=-4, force_tile_skip=1)
    assert st['masked_tile_pct'] > 0, st              # (tile list present, skip list non-empty)
    same(S[0], fl[0], Sl, fll, kind + ' land block')
    S, fl, st = _run([pn], NSW, 0.0, rows_per_tile=-4, force_tile_skip=1)
    assert st['masked_tile_pct'] == 0, st             # (nothing to skip: one set of records for every member)
    same(S[0], fl[0], Sn, fln, kind + ' no land')
    # two members with different masks: their lists, and so their records, differ
    po, (Soo, floo) = _problem(kind, 96, 352, 'fixed', 'periodic', land=(0, 48, 224, 352), seed=1)
    S, fl, st = _run([pl, po, pn], NSW, 0.0, rows_per_tile=-4, force_tile_skip=1)
    assert st['masked_tile_pct'] > 0, st
    for m, (So, flo) in enumerate([(Sl, fll), (Soo, floo), (Sn, fln)]):
        same(S[m], fl[m], So, flo, '%s member %d of three' % (kind, m))


def test_extend_with_a_tile_list():
    p, (So, flo) = _problem('std2d', 96, 352, 'extend', 'fixed', land=LAND)
    S, fl, st = _run([p], NSW, 0.0, rows_per_tile=-4, force_tile_skip=1)
    assert st['masked_tile_pct'] > 0, st
    same(S[0], fl[0], So, flo, 'extend, land block')


def _stop_tolerance(p, loop):
    """A tolerance the stop rule first meets at loop index `loop`: between the relative changes of that sweep and of
    every sweep before it (the oracle's, sweep by sweep)."""
    ch = [run_oracle(p, k, 0.0, COLOUR_2)[1][1] for k in range(loop + 1)]
    assert all(c > ch[loop] for c in ch[:loop]), ch
    return float(np.sqrt(ch[loop] * min(ch[:loop])))


def test_stop_on_the_second_sweep_of_a_pass_and_the_launches_behind_it():
    p, _ = _problem('std2d', 46, 240, 'fixed', 'periodic')
    tol = _stop_tolerance(p, 5)                       # sweep 6: the second of the second four-sweep pass
    So, flo = run_oracle(p, 400, tol, COLOUR_2)
    assert flo[2] == 5 and (flo[2] + 1) % 4 == 2, flo
    S, fl, st = _run([p], 400, tol, rows_per_tile=46)
    assert st['sweeps_max'] == 6, st
    same(S[0], fl[0], So, flo, 'stop inside a pass')
    # ... as a member of a batch whose other member runs on for more than two further passes: every
    # later launch of the batch finds the first member finished and returns at the entry, leaving its S and flags alone
    q = _uniform2d(rand2d('std2d', 46, 240, 'fixed', 'periodic', 0, 0, seed=2))        # (no mask: its norm settles later)
    Sq, flq = run_oracle(q, 41, tol, COLOUR_2)
    assert flq[2] > flo[2] + 8, (flq, flo)
    So2, flo2 = run_oracle(p, 41, tol, COLOUR_2)
    assert flo2[2] == 5
    S, fl, st = _run([p, q], 41, tol, rows_per_tile=46)
    same(S[0], fl[0], So2, flo2, 'finished member of a batch')
    same(S[1], fl[1], Sq, flq, 'the member that ran on')


def test_resident_plan_twice_and_after_a_refresh_with_another_mask():
    import torch
    from xinvert_amd.resident import ResidentProblem
    from test_gpu_plan import _as_problem
    p, (So, flo) = _problem('std2d', 96, 352, 'fixed', 'periodic', land=LAND)
    rp = ResidentProblem(_as_problem([dict(p)], ()))
    opts = dict(path=PATH_FUSED, rows_per_tile=-4, force_tile_skip=1)
    for rep in range(2):
        rp.reset()
        fl, st = rp.solve(NSW, 0.0, **opts)
        assert st['planned'] == 1 and st['pipelined'] == 1 and st['masked_tile_pct'] > 0, st
        same(rp.result()[0], fl[0], So, flo, 'plan, solve %d' % rep)
    # another mask (land elsewhere): lists and records are stale until the plan is refreshed
    q, (Sq, flq) = _problem('std2d', 96, 352, 'fixed', 'periodic', land=(48, 96, 0, 112), seed=3)
    for k in (0, 2, 3):
        rp.coefs[k].copy_(torch.from_numpy(np.ascontiguousarray(q['coefs'][k])[None]).to(rp.dev))
    rp.S0.copy_(torch.from_numpy(q['S0'][None]).to(rp.dev)); rp.reset()
    rp.refresh()
    fl, st = rp.solve(NSW, 0.0, **opts)
    assert st['planned'] == 1 and st['pipelined'] == 1 and st['masked_tile_pct'] > 0, st
    same(rp.result()[0], fl[0], Sq, flq, 'plan after refresh')
    rp.close()
