"""The direct Fourier solve of the 2-D standard form for periodic x (iParams['method'] = 'fourier'; include/xinv.h,
"fourier"): the row transform for callers who want the spectrum, and the eligibility test of the front end.

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


def _refuse(why):
    raise Exception("iParams['method'] = 'fourier': %s; 'sor' solves this case" % why)


def _per_row(name, a, rowconst):
    """A coefficient as _prep_coef hands it over -> one float64 value per row ([yc] or [nbatch, yc])."""
    a = np.asarray(a, dtype=np.float64)
    if rowconst:                                         # (a stride-0 view along x: only its first column travelled)
        return np.ascontiguousarray(a)
    first = a[..., :1]
    if not ((a == first) | (np.isnan(a) & np.isnan(first))).all():     # (a NaN row -- cos beyond the pole -- is constant too)
        _refuse('%s must be constant along x (the array %s varies along it)' % (name, name))
    return np.ascontiguousarray(a[..., 0])


def eligible(A, B, C, Fv, Sv, BCs, undef):
    """The conditions of the Fourier path on the host arrays of one call, in the order of DESIGN.md 4.16; the first that
    fails raises an Exception naming it.  A, B, C: (array, rowconst) as core._prep_coef returns them (B: None = identically
    zero); Fv, Sv [nbatch, yc, xc].  -> (A, C) as one value per row."""
    if B[0] is not None and np.any(np.asarray(B[0]) != 0):
        _refuse('B must be identically zero (the array B is not)')
    BCs = list(BCs)
    if BCs[0] != 'fixed':
        _refuse("BCs must be ['fixed', 'periodic'] (the boundary code along y is %r)" % (BCs[0],))
    if BCs[1] != 'periodic':
        _refuse("BCs must be ['fixed', 'periodic'] (the boundary code along x is %r)" % (BCs[1],))
    Ar, Cr = _per_row('A', *A), _per_row('C', *C)
    for name, pts, rows in (('F', Fv[:, 1:-1], '1 .. yc-2'), ('A', Ar[..., 1:], '1 .. yc-1'), ('C', Cr[..., 1:-1], '1 .. yc-2'),
                            ('S', Sv[:, [0, -1]], '0 and yc-1')):
        if (pts == undef).any():
            _refuse('no undefined value may sit at a point the solve reads (the array %s holds one on rows %s)' % (name, rows))
    yc, xc = Fv.shape[-2:]
    if yc < 3:
        _refuse('yc must be at least 3, got %d' % yc)
    err = length_error(xc) if xc >= 3 else 'xc must be at least 3, got %d' % xc
    if err:
        _refuse(err)
    return Ar, Cr
