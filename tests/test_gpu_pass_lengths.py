"""Every pass length of every sweep-kernel family runs the right kernel.  A plan resolves one kernel per pass length
k = 1 .. K (Plan::kern, xinv_plan.h: plan_kernels): the full pass, every shorter tail, and the one-sweep redo of a
pass the stop rule fired inside.  For each family and its planned K, budgets of K + r sweeps, r = 1 .. K - 1, run one
full pass and a tail of r; a tolerance that stops inside the first pass runs the one-sweep redo.  A wrong kernel in any
slot (another K, another model, another mask of per-row streams) sweeps other points or in another order: everything is
BIT FOR BIT the coloured oracle.  Shapes: the smallest with two strips and an odd row count."""
import functools

import numpy as np
import pytest

from util import rand2d, rand2dt, rand3d, rand3dg, randbih, run_hip_batched, run_oracle

pytestmark = pytest.mark.gpu
COLOUR_AUTO, COLOUR_2, FMA, PATH_FUSED = 1, 2, 0x100, 2
STOP_AT_ONCE = 1e30          # |norm - normPrev| / normPrev is below it at the first sweep that tests it


def _uniform(p, which):
    """coefficient arrays `which` constant along x (a lat-lon grid's): the per-row-coefficient variants"""
    q = dict(p)
    q['coefs'] = [np.ascontiguousarray(np.broadcast_to(c[..., :1], c.shape)) if k in which else c
                  for k, c in enumerate(p['coefs'])]
    return q


@functools.lru_cache(maxsize=None)
def _problem(name):
    """The problems, built once; name = form[+x-uniform][+9-point] @ shape, periodic x on the odd widths."""
    form, shape = name.split('@')
    shape = tuple(int(s) for s in shape.split('x'))
    BCx = 'periodic' if shape[-1] % 2 else 'fixed'
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(name))
    if form == 'std2d':   return rand2d('std2d', *shape, 'fixed', BCx, 0, 1, seed=seed)
    if form == 'std2d_u': return _uniform(rand2d('std2d', *shape, 'fixed', BCx, 0, 1, seed=seed), (0, 2))
    if form == 'gen2d':   return rand2d('gen2d', *shape, 'fixed', BCx, 0, 1, seed=seed)
    if form == 'gen2d_u': return _uniform(rand2d('gen2d', *shape, 'fixed', BCx, 0, 1, seed=seed), (0, 2, 3, 4, 5))
    if form == 'std2dt':  return rand2dt(*shape, 'fixed', BCx, 0, 1, seed=seed)
    if form == 'std2d_9': return rand2d('std2d', *shape, 'extend', BCx, 1, 1, seed=seed)
    if form == 'gen2d_9': return rand2d('gen2d', *shape, 'fixed', BCx, 1, 1, seed=seed)
    if form == 'bih':     return randbih(*shape, 'extend', BCx, 1, 1, seed=seed)
    if form == 'bih_z':   return randbih(*shape, 'fixed', BCx, 0, 1, seed=seed)     # (no mixed derivatives: B == E == 0)
    if form == 'bih_u':   return _uniform(randbih(*shape, 'fixed', BCx, 1, 1, seed=seed), range(9))
    if form == 'std3d':   return rand3d(*shape, 'fixed', BCx, 1, seed=seed)
    if form == 'std3d_u': return _uniform(rand3d(*shape, 'fixed', BCx, 1, seed=seed), (0, 1, 2))
    if form == 'std3d_ue': return _uniform(rand3d(*shape, 'extend', BCx, 1, seed=seed), (0, 1, 2))
    if form == 'gen3d_u': return _uniform(rand3dg(*shape, 'fixed', BCx, 1, seed=seed), range(7))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(name, mxLoop, tol, order):
    """The oracle's result, computed once per (problem, budget, tolerance, ordering) and shared by the variants."""
    S, fl = run_oracle(_problem(name), mxLoop, tol, order)
    S.setflags(write=False); fl.setflags(write=False)
    return S, fl


S2, S9, S2P, T3, T3P = '33x130', '33x130', '33x131', '7x17x24', '8x39x65'
# (problem, planned sweeps per pass, pipelined, oracle ordering, options)
CASES = [
    # 2-D 5-point forms: the wave-pipelined pass (k_pipe2d at k = 4, k_fused2d with the same per-row mask below) ...
    ('std2d_u@' + S2, 4, 1, COLOUR_2, {}),
    ('gen2d_u@' + S2, 4, 1, COLOUR_2, {}),
    ('std2d_u@' + S2, 4, 1, COLOUR_2 | FMA, dict(fma=1)),
    ('gen2d_u@' + S2, 4, 1, COLOUR_2 | FMA, dict(fma=1)),
    # ... and k_fused2d alone at the deepest pass each model is instantiated for
    ('std2d_u@' + S2, 4, 0, COLOUR_2, dict(no_pipe=1, sweeps_per_launch=4)),
    ('gen2d_u@' + S2, 3, 0, COLOUR_2, dict(no_pipe=1, sweeps_per_launch=3)),
    ('std2d_u@' + S2, 4, 0, COLOUR_2 | FMA, dict(no_pipe=1, sweeps_per_launch=4, fma=1)),
    ('gen2d_u@' + S2, 3, 0, COLOUR_2 | FMA, dict(no_pipe=1, sweeps_per_launch=3, fma=1)),
    ('std2d@' + S2, 4, 0, COLOUR_2, dict(no_pipe=1, sweeps_per_launch=4)),        # every stream a vector
    ('gen2d@' + S2, 3, 0, COLOUR_2, dict(no_pipe=1, sweeps_per_launch=3)),        # the point-factor model
    ('std2dt@' + S2, 3, 0, COLOUR_2, dict(no_pipe=1, sweeps_per_launch=3)),
    # the odd-xc periodic seam variants
    ('std2d_u@' + S2P, 4, 1, COLOUR_2, {}),
    ('gen2d_u@' + S2P, 4, 1, COLOUR_2, {}),
    ('std2d_u@' + S2P, 4, 0, COLOUR_2, dict(no_pipe=1, sweeps_per_launch=4)),
    ('gen2d_u@' + S2P, 3, 0, COLOUR_2, dict(no_pipe=1, sweeps_per_launch=3)),
    ('std2dt@' + S2P, 3, 0, COLOUR_2, dict(no_pipe=1, sweeps_per_launch=3)),
    # 9-point forms (k_fused9), with and without the seam
    ('std2d_9@' + S9, 3, 0, COLOUR_AUTO, dict(sweeps_per_launch=3)),
    ('gen2d_9@' + S9, 2, 0, COLOUR_AUTO, {}),
    ('std2d_9@' + S2P, 3, 0, COLOUR_AUTO, dict(sweeps_per_launch=3)),
    ('gen2d_9@' + S2P, 2, 0, COLOUR_AUTO, {}),
    # biharmonic form (k_fusedbih: one sweep per pass): per-row records, nine vector streams, four
    ('bih_u@' + S2, 1, 0, COLOUR_AUTO, {}),
    ('bih@' + S2, 1, 0, COLOUR_AUTO, {}),
    ('bih_z@' + S2, 1, 0, COLOUR_AUTO, {}),
    # 3-D forms: k_pipe3d at k = 2 over k_fused3d; k_fused3d alone; k_fused3dg
    ('std3d_u@' + T3, 2, 0, COLOUR_2, {}),
    ('std3d_u@' + T3P, 2, 0, COLOUR_2, {}),
    ('std3d_ue@' + T3, 2, 0, COLOUR_2, {}),
    ('std3d_u@' + T3, 2, 0, COLOUR_2 | FMA, dict(fma=1)),
    ('std3d_u@' + T3P, 1, 0, COLOUR_2, dict(sweeps_per_launch=1)),
    ('std3d@' + T3, 1, 0, COLOUR_2, {}),
    ('std3d@' + T3P, 1, 0, COLOUR_2, {}),
    ('gen3d_u@' + T3, 1, 0, COLOUR_2, {}),
    ('gen3d_u@' + T3P, 1, 0, COLOUR_2, {}),
]


def _same(S, fl, ref, what):
    So, flo = ref
    assert np.array_equal(S, So), '%s: %d points differ' % (what, int((S != So).sum()))
    assert fl[2] == flo[2] and fl[0] == flo[0], (what, fl, flo)
    assert abs(fl[1] - flo[1]) <= 1e-12 + 1e-9 * abs(flo[1]), (what, fl, flo)


def _one_case(name, K, pipelined, order, opt):
    p = _problem(name)
    # a full pass and every shorter tail; three passes for the families with one sweep per pass
    for sweeps in ([K + r for r in range(1, K)] or [3]):
        S, fl, st = run_hip_batched([p], sweeps - 1, 0.0, path=PATH_FUSED, **opt)
        assert st['path'] == PATH_FUSED and st['sweeps_per_launch'] == K and st['pipelined'] == pipelined, st
        assert st['sweeps_max'] == sweeps, st
        _same(S[0], fl[0], _reference(name, sweeps - 1, 0.0, order), '%d sweeps' % sweeps)
    # the stop rule fires inside the first pass: the one-sweep redo from the pass's source
    ref = _reference(name, 4 * K, STOP_AT_ONCE, order)
    assert K == 1 or ref[1][2] + 1 < K, ref[1]
    S, fl, st = run_hip_batched([p], 4 * K, STOP_AT_ONCE, path=PATH_FUSED, **opt)
    assert st['sweeps_per_launch'] == K and st['sweeps_max'] == ref[1][2] + 1, st
    _same(S[0], fl[0], ref, 'stop inside the first pass')


def test_every_pass_length_runs_its_own_kernel():
    """One test over all the cases (a few milliseconds each): every case runs, and every one that fails is named."""
    bad = []
    for case in CASES:
        try:
            _one_case(*case)
        except AssertionError as e:
            bad.append('%s %r: %s' % (case[0], case[4], str(e)[:300]))
    assert not bad, '%d of %d cases fail:\n%s' % (len(bad), len(CASES), '\n'.join(bad))
