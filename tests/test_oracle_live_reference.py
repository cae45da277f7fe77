"""The C oracle against the reference's own numbas.py on seeded random inputs: every cell of
kernel x BCy x BCx x mask x (B == 0 | B != 0), bit-exact S and flags.

The inputs are regenerated here from the seed (cases()); what the reference computed on them is
stored in tests/golden/live_reference.npz, written by tests/golden/gen_golden.py (`live`), which
runs the reference's kernels on the same cases()."""
import numpy as np

from util import U, golden

# oracle function -> the reference kernel it restates (xinvert/numbas.py)
REF_NAMES = {'standard_2d': 'invert_standard_2D', 'general_2d': 'invert_general_2D',
             'standard_3d': 'invert_standard_3D', 'standard_2d_test': 'invert_standard_2D_test',
             'general_bih_2d': 'invert_general_bih_2D'}


def cases():
    """-> (oracle function name, S0, coefficient arrays, scalar arguments, mxLoop, tolerance), in a fixed order."""
    rng = np.random.default_rng(424242)
    mk = lambda sh: rng.uniform(0.5, 1.5, sh)
    for (yc, xc) in [(11, 14), (9, 9), (8, 21)]:
        for BCy in ('fixed', 'extend'):
            for BCx in ('fixed', 'periodic', 'extend'):
                for bnz in (0, 1):
                    for msk in (0, 1):
                        sh = (yc, xc)
                        A, C = mk(sh), mk(sh)
                        B = rng.uniform(-.2, .2, sh) if bnz else np.zeros(sh)
                        F = rng.standard_normal(sh)
                        if msk:
                            F[rng.random(sh) < 0.15] = U
                            A[rng.random(sh) < 0.03] = U
                            if bnz:
                                B[rng.random(sh) < 0.03] = U
                        S0 = rng.standard_normal(sh) * 0.1
                        if msk:
                            S0[rng.random(sh) < 0.05] = U
                        a2 = (yc, xc, 1.3, 1.1, BCy, BCx, 1.21, 1.1 / 1.3 / 4, (1.1 / 1.3)**2, 1.3, U)
                        yield 'standard_2d', S0, (A, B, C, F), a2, 12, 1e-9
                        D, E, Fc = mk(sh) * 0.1, mk(sh) * 0.1, -mk(sh) * 0.01
                        ag = (yc, xc, 1.3, 1.1, BCy, BCx, 1.21, 1.1 / 1.3, 1.1 / 1.3 / 4, (1.1 / 1.3)**2, 1.3, U)
                        yield 'general_2d', S0, (A, B, C, D, E, Fc, F), ag, 12, 1e-9
    for sh in [(5, 7, 9), (4, 6, 8)]:
        for BCy in ('fixed', 'extend'):
            for BCx in ('fixed', 'periodic'):
                for msk in (0, 1):
                    A, B, C, F = mk(sh), mk(sh), mk(sh), rng.standard_normal(sh)
                    if msk:
                        F[rng.random(sh) < 0.15] = U
                        B[rng.random(sh) < 0.03] = U
                    S0 = rng.standard_normal(sh) * 0.1
                    a3 = (*sh, 2., 1.3, 1.1, 'fixed', BCy, BCx, 1.21, (1.1 / 2)**2, (1.1 / 1.3)**2, 1.2, U)
                    yield 'standard_3d', S0, (A, B, C, F), a3, 8, 1e-9
    for (yc, xc) in [(8, 10), (7, 9)]:
        for BCy in ('fixed', 'extend'):
            for BCx in ('fixed', 'periodic'):
                for bnz in (0, 1):
                    sh = (yc, xc)
                    mkt = lambda s=1.0: rng.uniform(0.5, 1.5, sh) * s
                    A, D = mkt(), mkt()
                    B = rng.uniform(-.2, .2, sh) if bnz else np.zeros(sh)
                    C = rng.uniform(-.2, .2, sh) if bnz else np.zeros(sh)
                    E = -mkt(0.05); F = rng.standard_normal(sh); F[rng.random(sh) < 0.1] = U
                    S0 = rng.standard_normal(sh) * 0.1
                    r = 1.1 / 1.3
                    at = (yc, xc, 1.3, 1.1, BCy, BCx, 1.21, r / 4, r**2, 1.3, U)
                    yield 'standard_2d_test', S0, (A, B, C, D, E, F), at, 8, 1e-9
    for (yc, xc) in [(8, 10), (7, 8)]:
        for BCy in ('fixed', 'extend'):
            for BCx in ('fixed', 'periodic'):
                for bnz in (0, 1):
                    sh = (yc, xc)
                    mkb = lambda s=1.0: rng.uniform(0.5, 1.5, sh) * s
                    A, C = mkb(), mkb()
                    B = mkb(0.3) if bnz else np.zeros(sh)
                    D, E, F = -mkb(0.5), (mkb(0.1) if bnz else np.zeros(sh)), -mkb(0.5)
                    G, H, I = mkb(0.05), mkb(0.05), mkb(0.01)
                    J = rng.standard_normal(sh); J[rng.random(sh) < 0.1] = U
                    S0 = rng.standard_normal(sh) * 0.1
                    r = 1.1 / 1.3
                    ab = (yc, xc, 1.3, 1.1, BCy, BCx, 1.1**4, 1.1**3, 1.1**2, r, r**4, r / 4, r**2, 0.9, U)
                    yield 'general_bih_2d', S0, (A, B, C, D, E, F, G, H, I, J), ab, 8, 1e-9


def test_lexicographic_oracle_equals_reference_live(oracle):
    want = golden('live_reference.npz')
    n = {}
    for i, (kernel, S0, arrays, args, mxLoop, tol) in enumerate(cases()):
        S = S0.copy(); fl = np.array([0., 1., 0.])
        getattr(oracle, kernel)(S, *arrays, *args, fl, mxLoop, tol)
        assert np.array_equal(S, want['S%03d' % i]) and np.array_equal(fl, want['f%03d' % i]), (i, kernel)
        n[kernel] = n.get(kernel, 0) + 1
    assert n == {'standard_2d': 72, 'general_2d': 72, 'standard_3d': 16, 'standard_2d_test': 16, 'general_bih_2d': 16}
    assert len(want.files) == 2 * sum(n.values())
