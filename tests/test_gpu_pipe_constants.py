"""GPU: the per-plan constants of the wave-pipelined pass -- the update masks it reads out of the plan's table
(k_pipe_masks: column, row and `forcing defined` as two lane words per row and strip) and the norm's sample count it keeps
on the scalar unit -- against the coloured-ordering oracle and the single-wavefront kernel (no_pipe = 1).

S, flags[0] and flags[2] bit for bit; flags[1] to the bar of test_gpu_parity.assert_same (the two kernels add the norm's
partial sums in a different order).

On top of the random masks every member's forcing is undefined at columns 0, 1 and xc-1 (lane 0 and the last lanes of a
word), on both sides of every strip border of the launch (a halo column two strips see; 112 owned columns, 110 in the
seam layout of 257 periodic columns), along one interior row, along rows 1 and yc-2 and at a single point."""
import functools

import numpy as np
import pytest

from util import rand2d, run_oracle, run_hip_batched
from test_gpu_parity import COLOUR_2, PATH_FUSED, _seed, _uniform2d, _uniform2d_all, assert_same

pytestmark = pytest.mark.gpu

NSW = 26                                              # six four-sweep passes and a tail
FMA = 0x100                                           # the oracle's contracted restatement (tests/test_gpu_fma.py)
UNI = {'std2d': _uniform2d, 'gen2d': _uniform2d_all}  # per-row A, C / A, C, D, E, F: the hoisted marches


def _strip_width(xc, BCx):
    """owned columns of a strip of the pipelined pass (xinv_tiles.h: the seam's ring layout, xinv_ring_uw with H = 8)"""
    if BCx == 'periodic' and xc % 2:
        return 128 - 16 - (2 if xc >= 128 - 16 - 2 + 8 else 4)
    return 112


def _mask_forcing(p, k=0):
    """the deterministic masks (in place, on the problem's own forcing)"""
    F = p['coefs'][-1]
    yc, xc = F.shape
    U = p['undef']
    F[:, [0, 1, xc - 1]] = U
    uw = _strip_width(xc, p['BCx'])
    for b in range(uw, xc, uw):
        F[:, [c for c in (b - 1, b, b + 1) if c < xc]] = U
    F[yc // 2 + k, :] = U
    F[[1, yc - 2], :] = U
    F[yc // 3, (xc // 2 + 7 * k) | 1] = U
    return p


def _same_as_single_wavefront(S, fl, S0, f0, what):
    assert np.array_equal(S, S0, equal_nan=True), what
    assert np.array_equal(fl[:, 2], f0[:, 2]) and np.array_equal(fl[:, 0], f0[:, 0]), what
    assert np.all(np.abs(fl[:, 1] - f0[:, 1]) <= 1e-12 + 1e-9 * np.abs(f0[:, 1])), what


@functools.lru_cache(maxsize=None)
def _case(kind, BCy, BCx, shape, fma):
    """Three members with their own coefficients and masks, the oracle's results and the single-wavefront kernel's:
    computed once per (form, boundaries, shape, arithmetic), read-only afterwards."""
    yc, xc = shape
    ps = [_mask_forcing(UNI[kind](rand2d(kind, yc, xc, BCy, BCx, 0, 1, seed=_seed(('pipeconst', kind, BCy, BCx, shape, m)))), m)
          for m in range(3)]
    ref = [run_oracle(p, NSW, 1e-9, COLOUR_2 | (FMA if fma else 0)) for p in ps]
    S0, f0, st0 = run_hip_batched(ps, NSW, 1e-9, path=PATH_FUSED, sweeps_per_launch=4, no_pipe=1, fma=fma)
    assert st0['pipelined'] == 0, st0
    return ps, ref, S0, f0


def _check_case(rows, kind, shape, BCy, BCx, fma):
    ps, ref, S0, f0 = _case(kind, BCy, BCx, shape, fma)
    for fr in (-1, 1):                                # the forcing re-read from memory / riding the LDS ring
        for skip in (0, 1):
            kw = dict(path=PATH_FUSED, pipe_fr=fr, rows_per_tile=rows, fma=fma)
            if skip:
                kw['force_tile_skip'] = 1
            S, fl, st = run_hip_batched(ps, NSW, 1e-9, **kw)
            assert st['pipelined'] == 1 and st['sweeps_per_launch'] == 4, st
            what = 'masks from the table: %s %r rows %d fr %d skip %d fma %d' % (kind, shape, rows, fr, skip, fma)
            for m in range(3):
                assert_same(S[m], fl[m], ref[m][0], ref[m][1], '%s member %d' % (what, m))
            _same_as_single_wavefront(S, fl, S0, f0, what)


@pytest.mark.parametrize('BCy,BCx', [('fixed', 'periodic'), ('extend', 'periodic'), ('extend', 'fixed')])
@pytest.mark.parametrize('shape', [(40, 300), (58, 257)])              # (257 columns, periodic: the seam tiles)
@pytest.mark.parametrize('kind', ['std2d', 'gen2d'])
@pytest.mark.parametrize('rows', [10, 12, 14, 16, -3])
def test_table_masks_equal_the_oracle_and_the_single_wavefront_pass(rows, kind, shape, BCy, BCx):
    _check_case(rows, kind, shape, BCy, BCx, 0)


@pytest.mark.parametrize('BCy,BCx', [('fixed', 'periodic'), ('extend', 'periodic'), ('extend', 'fixed')])
@pytest.mark.parametrize('kind', ['std2d', 'gen2d'])
@pytest.mark.parametrize('rows', [10, 12, 14, 16, -3])
def test_table_masks_with_contracted_arithmetic(rows, kind, BCy, BCx):
    """(no contracted variant runs the odd-xc periodic seam: 300 columns only)"""
    _check_case(rows, kind, (40, 300), BCy, BCx, 1)


def test_a_forcing_whose_scaled_value_equals_undef_is_updated():
    """delxSqr = 4 and one defined forcing value undef / 4: F * delxSqr is undef exactly, F is not -- the point is updated
    as the oracle updates it."""
    p = rand2d('std2d', 40, 300, 'fixed', 'periodic', 0, 1, seed=31, delx=2.0)
    assert p['delxSqr'] == 4.0
    p = _mask_forcing(_uniform2d(p))
    j, i = 17, 150
    p['coefs'][-1][j - 1:j + 2, i - 1:i + 2] = 0.25             # (defined neighbours: the point's value spreads)
    p['coefs'][-1][j, i] = p['undef'] / 4.0
    assert p['coefs'][-1][j, i] * p['delxSqr'] == p['undef'] and p['coefs'][-1][j, i] != p['undef']
    p['S0'][j - 1:j + 2, i - 1:i + 2] = 0.0
    So, flo = run_oracle(p, NSW, 0.0, COLOUR_2)
    assert So[j, i] != p['S0'][j, i]
    for rows in (12, -3):
        S, fl, st = run_hip_batched([p], NSW, 0.0, path=PATH_FUSED, rows_per_tile=rows)
        assert st['pipelined'] == 1, st
        assert_same(S[0], fl[0], So, flo, 'F * delxSqr == undef, rows %d' % rows)


def test_a_nan_forcing_value_counts_as_defined():
    """NaN != undef: the point is updated, S is poisoned and the overflow exit trips in the oracle's sweep.  (How far the
    NaN has spread when the run stops is the one thing the streaming kernels do not share with the oracle, DESIGN.md 2:
    the exit sweep and the flags are the same.)"""
    p = _mask_forcing(_uniform2d(rand2d('std2d', 40, 300, 'fixed', 'periodic', 0, 1, seed=32)))
    p['coefs'][-1][20, 151] = np.nan
    p['S0'][20, 151] = 0.0
    So, flo = run_oracle(p, NSW, 1e-9, COLOUR_2)
    assert np.isnan(So[20, 151]) and flo[0] == 1.0
    for fr in (-1, 1):
        S, fl, st = run_hip_batched([p], NSW, 1e-9, path=PATH_FUSED, rows_per_tile=12, pipe_fr=fr)
        assert st['pipelined'] == 1, st
        assert np.isnan(S[0][20, 151]), fr
        assert fl[0][0] == flo[0] == 1.0 and fl[0][2] == flo[2], (fl, flo)


def _resident(p):
    from xinvert_amd.resident import ResidentProblem
    q = dict(p)
    q['S0'] = p['S0'][None]
    q['coefs'] = [c[None] for c in p['coefs']]
    return ResidentProblem(q, plan=True, null_zero_B=True)


@pytest.mark.parametrize('kind', ['std2d', 'gen2d'])
def test_two_solves_on_one_plan_with_other_forcing_values(kind):
    """The forcing's values change between two solves on a plan, its mask does not: the second solve is a fresh solve of
    the new values, bit for bit."""
    import torch
    p = _mask_forcing(UNI[kind](rand2d(kind, 58, 257, 'fixed', 'periodic', 0, 1, seed=41)))
    rp = _resident(p)
    fl, st = rp.solve(NSW, 0.0, rows_per_tile=14)
    assert st['pipelined'] == 1 and st['planned'] == 1, st
    So, flo = run_oracle(p, NSW, 0.0, COLOUR_2)
    assert_same(rp.result()[0], fl[0], So, flo, 'first solve on the plan')
    q = dict(p); q['coefs'] = list(p['coefs'])
    F = np.array(p['coefs'][-1], copy=True)
    defined = F != p['undef']
    F[defined] = np.random.default_rng(42).standard_normal(int(defined.sum()))
    q['coefs'][-1] = F
    rp.coefs[-1].copy_(torch.from_numpy(F[None]).to(rp.dev))
    rp.reset()
    fl, st = rp.solve(NSW, 0.0, rows_per_tile=14)
    assert st['planned'] == 1 and st['plan_ms'] == 0.0, st
    So, flo = run_oracle(q, NSW, 0.0, COLOUR_2)
    assert_same(rp.result()[0], fl[0], So, flo, 'second solve on the plan, other forcing values')
    Sf, ff, _ = run_hip_batched([q], NSW, 0.0, path=PATH_FUSED, rows_per_tile=14)
    assert np.array_equal(rp.result()[0], Sf[0]) and np.array_equal(fl[0], ff[0])
    rp.close()


@pytest.mark.parametrize('shape,BCx', [((40, 300), 'periodic'), ((58, 257), 'periodic'), ((40, 300), 'fixed')])
def test_plan_refresh_rebuilds_the_table_of_masks(shape, BCx):
    """After xinv_plan_refresh with another mask in the forcing the solve equals a fresh plan's (a stale table would keep
    the old mask's points fixed and update the new mask's)."""
    import torch
    yc, xc = shape
    p = _mask_forcing(_uniform2d(rand2d('std2d', yc, xc, 'fixed', BCx, 0, 1, seed=51)))
    rp = _resident(p)
    fl, st = rp.solve(NSW, 0.0, rows_per_tile=12)
    assert st['pipelined'] == 1, st
    q = _mask_forcing(_uniform2d(rand2d('std2d', yc, xc, 'fixed', BCx, 0, 1, seed=52)), 3)
    q['coefs'][0] = p['coefs'][0]; q['coefs'][2] = p['coefs'][2]; q['S0'] = p['S0']
    assert not np.array_equal(q['coefs'][-1] == q['undef'], p['coefs'][-1] == p['undef'])
    rp.coefs[-1].copy_(torch.from_numpy(np.ascontiguousarray(q['coefs'][-1])[None]).to(rp.dev))
    rp.reset()
    rp.refresh()
    fl, st = rp.solve(NSW, 0.0, rows_per_tile=12)
    assert st['pipelined'] == 1 and st['planned'] == 1, st
    So, flo = run_oracle(q, NSW, 0.0, COLOUR_2)
    assert_same(rp.result()[0], fl[0], So, flo, 'after the refresh')
    fresh = _resident(q)
    ff, _ = fresh.solve(NSW, 0.0, rows_per_tile=12)
    assert np.array_equal(rp.result(), fresh.result()) and np.array_equal(fl, ff)
    fresh.close(); rp.close()


def test_table_masks_stop_inside_a_pass():
    """The tolerance is met in the second sweep of a pass: the oracle's stopping sweep and its bits."""
    p = _mask_forcing(_uniform2d(rand2d('std2d', 40, 300, 'fixed', 'periodic', 0, 1, seed=7)))
    tol = 8e-4
    So, flo = run_oracle(p, 500, tol, COLOUR_2)
    assert 2 < flo[2] < 499 and (flo[2] + 1) % 4 == 2
    S0, f0, st0 = run_hip_batched([p], 500, tol, path=PATH_FUSED, sweeps_per_launch=4, no_pipe=1)
    assert st0['pipelined'] == 0, st0
    for fr in (-1, 1):
        S, fl, st = run_hip_batched([p], 500, tol, path=PATH_FUSED, rows_per_tile=14, pipe_fr=fr)
        assert st['pipelined'] == 1 and st['sweeps_per_launch'] == 4, st
        assert_same(S[0], fl[0], So, flo, 'early stop, fr %d' % fr)
        assert st['sweeps_max'] == flo[2] + 1
        _same_as_single_wavefront(S, fl, S0, f0, 'early stop, fr %d' % fr)


@pytest.mark.parametrize('shape,BCx', [((40, 300), 'periodic'), ((58, 257), 'periodic')])
def test_the_sample_count_follows_s_from_sweep_to_sweep(shape, BCx):
    """The first guess holds undef where the first sweep updates (the point is a sample from then on) and where the forcing
    is undefined too (never a sample): the count differs between the sweeps of one pass.  Every sweep budget 1..8."""
    yc, xc = shape
    p = _mask_forcing(_uniform2d(rand2d('std2d', yc, xc, 'fixed', BCx, 0, 0, seed=61)))
    U = p['undef']
    p['S0'][5:9, 20:140] = U                              # forcing defined but for the masked border columns: updated
    p['coefs'][-1][22:27, 100:130] = U
    p['S0'][21:28, 90:135] = U                            # partly over the undefined forcing: those stay undef
    p['S0'][3, :] = U; p['S0'][:, xc - 2] = U
    for n in range(1, 9):
        So, flo = run_oracle(p, n - 1, 0.0, COLOUR_2)
        S0, f0, st0 = run_hip_batched([p], n - 1, 0.0, path=PATH_FUSED, sweeps_per_launch=4, no_pipe=1)
        for rows in (12, -3):
            S, fl, st = run_hip_batched([p], n - 1, 0.0, path=PATH_FUSED, rows_per_tile=rows)
            if n >= 4:
                assert st['pipelined'] == 1, st
            assert_same(S[0], fl[0], So, flo, 'sample count, %d sweeps, rows %d' % (n, rows))
            _same_as_single_wavefront(S, fl, S0, f0, 'sample count, %d sweeps, rows %d' % (n, rows))


def test_rolling_host_batch_builds_each_chunks_masks_behind_its_upload():
    """The rolling host-pointer batch plans before the later chunks' forcing has arrived: every chunk's share of the table
    is built when the chunk joins, behind its upload.  Two batches of one geometry, the second with other masks in every
    member (a table built from whatever the device buffers held before -- the first batch's forcing -- would freeze defined
    points and update undefined ones); one member per chunk, two lanes."""
    nb, yc, xc = 6, 300, 920
    base = rand2d('std2d', yc, xc, 'fixed', 'periodic', 0, 0, seed=970)
    for q in range(3):
        base['coefs'][q][:] = base['coefs'][q][:, :1]
    for batch in range(2):
        ps = []
        for m in range(nb):
            r = rand2d('std2d', yc, xc, 'fixed', 'periodic', 0, 1, seed=971 + 10 * batch + m)
            q = dict(base)
            F = np.array(r['coefs'][-1], copy=True)
            F[(17 * m + 40 * batch) % (yc - 40) + 5:][:3, 100 * m + 50 * batch:][:, :400] = base['undef']   # (thin: no whole tile,
            F[20:220, 31 * m + 13 * batch + 7:][:, :3] = base['undef']                                     #  or the batch would not roll)
            q['coefs'] = list(base['coefs'][:3]) + [F]
            q['S0'] = np.where(r['S0'] == base['undef'], 0.0, r['S0'])
            ps.append(q)
        S, fl, st = run_hip_batched(ps, 11, 0.0, shared=(0, 1, 2), host_inflight=-1, force_tile_skip=1, host_chunk=1)
        assert st['rolling'] == 1 and st['pipelined'] == 1 and st['host_chunks'] == nb, st
        for m, q in enumerate(ps):
            So, flo = run_oracle(q, 11, 0.0, COLOUR_2)
            assert_same(S[m], fl[m], So, flo, 'rolling batch %d, member %d' % (batch, m))
