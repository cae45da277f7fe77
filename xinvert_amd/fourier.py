"""The direct Fourier solve of the 2-D standard form for periodic x (iParams['method'] = 'fourier'; include/xinv.h,
"fourier") and of the 2-D general form (iParams['method'] = 'cfourier': B == 0, complex systems): the row transform for
callers who want the spectrum, FourierPlan for callers who solve one operator again and again (the factors are kept; a
solve only queues), the table of what differs between the two methods (METHODS) and the one ordered statement of their
conditions (_conditions) behind the eligibility tests of the front end (eligible, eligible_general, resident_eligible).

rfft_rows / irfft_rows are numpy.fft.rfft / irfft along the last axis of a CUDA float64 tensor, on the HIP kernel k_rowdft
(queued on the current stream).  Row lengths are products of 2, 3 and 5 up to MAX_N.  There is no CPU fallback.
"""
import numpy as np

from . import _lib

MAX_N = 4096                     # XINV_DFT_MAX_N of xinvert_amd/csrc/xinv_fourier.h


def length_error(n):
    """None when the transform takes rows of n points, otherwise what is wrong with n (the library's own words)."""
    n = int(n)
    if n < 2:
        return 'a row needs at least 2 points, got %d' % n
    r = n
    for q in (2, 3, 5):
        while r % q == 0:
            r //= q
    if r != 1:
        f = next((p for p in range(7, int(r ** 0.5) + 1, 2) if r % p == 0), r)
        return 'the row length %d has the prime factor %d (the transform takes products of 2, 3 and 5)' % (n, f)
    if n > MAX_N:
        return "the row length %d is beyond the transform's LDS budget (at most %d points)" % (n, MAX_N)
    return None


def _rows(x, what):
    import torch
    if not isinstance(x, torch.Tensor) or x.device.type != 'cuda' or x.dtype != what or x.ndim < 1:
        raise _lib.XinvError('rfft_rows takes a CUDA float64 tensor, irfft_rows a CUDA complex128 one')
    return x.contiguous()


def rfft_rows(x):
    """Real [..., n] -> half spectrum [..., n // 2 + 1] (complex128)."""
    import torch
    x = _rows(x, torch.float64)
    n = x.shape[-1]
    err = length_error(n)
    if err:
        raise _lib.XinvError(err)
    out = torch.empty(x.shape[:-1] + (n // 2 + 1,), dtype=torch.complex128, device=x.device)
    nrows = x.numel() // n
    if nrows:
        L = _lib.require_gpu()
        with torch.cuda.device(x.device):
            _lib.check(L.xinv_rowdft_f64_dev(_lib.dptr(out), _lib.dptr(x), nrows, n, 0, _lib.stream_arg(x.device)))
    return out


def irfft_rows(X, n=None):
    """Half spectrum [..., K] -> real [..., n]; n defaults to 2 (K - 1), as numpy.fft.irfft."""
    import torch
    X = _rows(X, torch.complex128)
    K = X.shape[-1]
    n = 2 * (K - 1) if n is None else int(n)
    err = length_error(n)
    if err:
        raise _lib.XinvError(err)
    if n // 2 + 1 != K:
        raise _lib.XinvError('a row of %d points has %d wavenumbers, got %d' % (n, n // 2 + 1, K))
    out = torch.empty(X.shape[:-1] + (n,), dtype=torch.float64, device=X.device)
    nrows = X.numel() // K
    if nrows:
        L = _lib.require_gpu()
        with torch.cuda.device(X.device):
            _lib.check(L.xinv_rowdft_f64_dev(_lib.dptr(out), _lib.dptr(X), nrows, n, 1, _lib.stream_arg(X.device)))
    return out


class FourierPlan:
    """One operator, many forcings (include/xinv.h, "fourier": xinv_fourier_plan_*).  The per-wavenumber factors are computed
    once, here; every `solve` then only queues a check pass, three transforms and a substitution without a division.

    A, C: numpy arrays or CUDA float64 tensors, one value per row: [yc] (shared by the batch) or [nbatch, yc].  The plan
    keeps its own copies.  `undef` at a point of A or C the solve reads raises XinvError."""

    def __init__(self, A, C, nbatch, yc, xc, delxSqr, ratioSqr, undef=-9.99e8, device=0):
        import ctypes
        import torch
        self._h = None
        self.L = _lib.require_gpu()
        self.nbatch, self.yc, self.xc = int(nbatch), int(yc), int(xc)
        self.dev = torch.device('cuda', device)
        self.K = self.xc // 2 + 1

        def rows(a, name):
            if not isinstance(a, torch.Tensor):
                a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
            a = a.to(device=self.dev, dtype=torch.float64).contiguous()
            if tuple(a.shape) not in ((self.yc,), (self.nbatch, self.yc)):
                raise _lib.XinvError('%s must be one value per row, [yc] or [nbatch, yc] = [%d] or [%d, %d], got %s'
                                     % (name, self.yc, self.nbatch, self.yc, list(a.shape)))
            return a

        A, C = rows(A, 'A'), rows(C, 'C')
        self.nset = self.nbatch if (A.ndim == 2 or C.ndim == 2) and self.nbatch > 1 else 1
        # what the plan holds in HBM: factors, spectrum, its copies of A and C, the status words
        self.nbytes = (16 * self.nset + 16 * self.nbatch) * self.yc * self.K + 8 * (A.numel() + C.numel()) + 8 * self.nbatch
        h = ctypes.c_void_p()
        with torch.cuda.device(self.dev):
            st = torch.cuda.current_stream(self.dev)
            rc = self.L.xinv_fourier_plan_create_standard_2d_f64_dev(
                ctypes.byref(h), _lib.dptr(A), _lib.dptr(C), self.nbatch,
                _lib.strides_arg([self.yc if A.ndim == 2 else 0, self.yc if C.ndim == 2 else 0]), self.yc, self.xc,
                float(delxSqr), float(ratioSqr), float(undef), ctypes.c_void_p(st.cuda_stream))
        _lib.check(rc)                                       # (create returns with the copies made: A and C may go)
        self._h = h

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def close(self):
        """Wait for the last solve and free what the plan owns."""
        h, self._h = getattr(self, '_h', None), None
        if h is not None:
            self.L.xinv_fourier_plan_destroy(h)

    def _live(self):
        if self._h is None:
            raise _lib.XinvError('the Fourier plan has been closed')
        return self._h

    def solve(self, S, F, stream=None):
        """Queue one solve on `stream` (default: torch's current stream): S [nbatch, yc, xc] CUDA float64, rows contiguous,
        the members at least one slice apart; rows 0 and yc-1 are the boundary values, rows 1 .. yc-2 are overwritten.
        F [nbatch, yc, xc], or [yc, xc]: one forcing for every member.  Nothing is waited for: `status()` has the flags."""
        import ctypes
        import torch
        h = self._live()
        nb, yc, xc = self.nbatch, self.yc, self.xc
        for t, name in ((S, 'S'), (F, 'F')):
            if not isinstance(t, torch.Tensor) or t.device != self.dev or t.dtype != torch.float64:
                raise _lib.XinvError('%s must be a float64 tensor on %s' % (name, self.dev))
        if S.ndim == 2 and nb == 1:
            S = S.unsqueeze(0)
        if tuple(S.shape) != (nb, yc, xc) or S.stride(2) != 1 or S.stride(1) != xc or (nb > 1 and S.stride(0) < yc * xc):
            raise _lib.XinvError('S must be [%d, %d, %d] with contiguous slices at least one slice apart, got shape %s strides %s'
                                 % (nb, yc, xc, list(S.shape), list(S.stride())))
        if tuple(F.shape) == (yc, xc):
            ok, sF = F.is_contiguous(), 0
        else:
            ok = tuple(F.shape) == (nb, yc, xc) and F.stride(2) == 1 and F.stride(1) == xc and (nb == 1 or F.stride(0) >= yc * xc)
            sF = F.stride(0) if ok and nb > 1 else 0
        if not ok:
            raise _lib.XinvError('F must be [%d, %d, %d] or [%d, %d] with contiguous slices, got shape %s strides %s'
                                 % (nb, yc, xc, yc, xc, list(F.shape), list(F.stride())))
        st = stream if stream is not None else torch.cuda.current_stream(self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(self.L.xinv_fourier_plan_solve_f64_dev(h, _lib.dptr(S), _lib.dptr(F), S.stride(0) if nb > 1 else 0, sF,
                                                             ctypes.c_void_p(st.cuda_stream)))

    def status(self):
        """Wait for the last solve -> (flags [nbatch, 3] = [overflow, 0, 0], bad [nbatch] = undef counts).  Raises XinvError
        naming the first member that held `undef` at a point the solve reads (its S was left alone; the others are solved);
        `self.flags` and `self.bad` are filled either way."""
        import ctypes
        h = self._live()
        self.flags = np.zeros((self.nbatch, 3))
        self.bad = np.zeros(self.nbatch, dtype=np.int32)
        rc = self.L.xinv_fourier_plan_status(h, _lib.hptr(self.flags), self.bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        _lib.check(rc)
        return self.flags, self.bad


# What differs between the two one-shot methods (core._method, core._solve_fourier and the eligibility tests read the rest
# off this): the one form that has the method, the host-pointer entry, the coefficients that travel as one value per row (B, identically zero, does not), the
# last row each is read on counted from the end (rows 1 .. yc-last), the forcing's letter, the scalars in the entry's order.
METHODS = {
    'fourier': dict(kind='std2d', entry='xinv_fourier_standard_2d_f64_batched', coefs='AC', last=dict(A=1, C=2), forcing='F',
                    scalars=('del1Sqr', 'ratioSqr')),
    'cfourier': dict(kind='gen2d', entry='xinv_fourier_general_2d_f64_batched', coefs='ACDEF', last=dict.fromkeys('ACDEF', 2),
                     forcing='G', scalars=('del1', 'del1Sqr', 'ratio', 'ratioSqr')),
}


def _conditions(method, B_nonzero, BCy, BCx, varies, undef_at, yc, xc):
    """The conditions of a Fourier path in the order of DESIGN.md 4.16; the first that fails raises an Exception naming it.
    varies(name): whether that coefficient varies along x; undef_at(): None, or (array, rows) of the first array -- forcing,
    coefficients, S -- with an undefined value at a point the solve reads."""
    def no(why):
        raise Exception("iParams['method'] = '%s': %s; 'sor' solves this case" % (method, why))
    if B_nonzero:
        no('B must be identically zero (the array B is not)')
    if BCy != 'fixed':
        no("BCs must be ['fixed', 'periodic'] (the boundary code along y is %r)" % (BCy,))
    if BCx != 'periodic':
        no("BCs must be ['fixed', 'periodic'] (the boundary code along x is %r)" % (BCx,))
    for name in METHODS[method]['coefs']:
        if varies(name):
            no('%s must be constant along x (the array %s varies along it)' % (name, name))
    at = undef_at()
    if at:
        no('no undefined value may sit at a point the solve reads (the array %s holds one on rows %s)' % at)
    if yc < 3:
        no('yc must be at least 3, got %d' % yc)
    err = length_error(xc) if xc >= 3 else 'xc must be at least 3, got %d' % xc
    if err:
        no(err)


def resident_eligible(kind, B_nonzero, BCy, BCx, varies, yc, xc):
    """The conditions of the Fourier path on a batch that is resident in HBM (ResidentProblem.solve_fourier), in the order and
    words of `eligible`; `varies`: the names of the coefficient arrays among A, C that vary along x.  The undef test is the
    device's (FourierPlan: at creation for A and C, in every solve for F and the boundary rows of S)."""
    if kind != 'std2d':
        raise _lib.XinvError("solve_fourier is available for the 2-D standard form only (kind 'std2d'), not for kind %r" % (kind,))
    _conditions('fourier', B_nonzero, BCy, BCx, lambda name: name in varies, lambda: None, yc, xc)


def eligible_for(method, coefs, B, Fv, Sv, BCs, undef):
    """The conditions of `method` on the host arrays of one call.  coefs: {letter: (array, rowconst)} as core._prep_coef
    returns them, and B likewise (None = identically zero); Fv (the forcing), Sv [nbatch, yc, xc].  -> the coefficients of
    METHODS[method]['coefs'], each as one float64 value per row ([yc] or [nbatch, yc])."""
    m = METHODS[method]
    yc, xc = Fv.shape[-2:]
    full = {k: np.asarray(coefs[k][0], dtype=np.float64) for k in m['coefs']}
    # (rowconst: a stride-0 view along x, of which only the first column travelled)
    rows = {k: np.ascontiguousarray(a if coefs[k][1] else a[..., 0]) for k, a in full.items()}

    def varies(name):
        if coefs[name][1]:
            return False
        a, first = full[name], full[name][..., :1]
        return not ((a == first) | (np.isnan(a) & np.isnan(first))).all()   # (a NaN row -- cos beyond the pole -- is constant too)

    def undef_at():
        pts = [(m['forcing'], Fv[:, 1:-1], '1 .. yc-2')]
        pts += [(k, rows[k][..., 1:yc + 1 - m['last'][k]], '1 .. yc-%d' % m['last'][k]) for k in m['coefs']]
        pts += [('S', Sv[:, [0, -1]], '0 and yc-1')]
        return next(((name, where) for name, p, where in pts if (p == undef).any()), None)

    BCs = list(BCs)
    _conditions(method, B[0] is not None and np.any(np.asarray(B[0]) != 0), BCs[0], BCs[1], varies, undef_at, yc, xc)
    return [rows[k] for k in m['coefs']]


def eligible_general(A, B, C, D, E, Fc, Gv, Sv, BCs, undef):
    """`eligible_for` the 2-D general form ('cfourier') -> [A, C, D, E, Fc] as one value per row.  Diagonal dominance is NOT
    a condition: the overflow flag and the residual are the safety net."""
    return eligible_for('cfourier', dict(zip('ACDEF', (A, C, D, E, Fc))), B, Gv, Sv, BCs, undef)


def eligible(A, B, C, Fv, Sv, BCs, undef):
    """`eligible_for` the 2-D standard form ('fourier') -> (A, C) as one value per row."""
    return tuple(eligible_for('fourier', dict(A=A, C=C), B, Fv, Sv, BCs, undef))
