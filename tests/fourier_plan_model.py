"""A Fourier plan restated in numpy ("Plans"): the arithmetic of k_fourier_factor and k_fourier_subst of
xinvert_amd/csrc/xinv_fourier.h, operation by operation in float64, around the transforms of tests/fourier_model.py.

    factor(A, C, ratioSqr, lam)         -> (inv, gam) [nset, yc, K]: inv_j = 1 / (di_jk - lo_j gam_{j-1}), gam_j = up_j inv_j on rows
                                           1 .. yc-2 (zeros elsewhere); nset = 1 when A and C are both one row of values
    substitute(spec2, A, ratioSqr, inv, gam) -> (spec2, overflow [nbatch]): spec2 [nbatch, yc, 2K] float64, re and im interleaved
                                           along the last axis; lane q of a member works with the factors of wavenumber q >> 1
    solve(S0, F, delxSqr, ratioSqr, factors, A, C, undef) -> (S, flags [nbatch, 3], bad [nbatch]): a member with bad != 0 keeps its S0
All leave their inputs alone.
"""
import numpy as np

import fourier_model as M


def factor(A, C, ratioSqr, lam):
    A, C = np.asarray(A, dtype=np.float64), np.asarray(C, dtype=np.float64)
    nset = max(A.shape[0] if A.ndim == 2 else 1, C.shape[0] if C.ndim == 2 else 1)
    yc = A.shape[-1]
    A, C = np.broadcast_to(A, (nset, yc)), np.broadcast_to(C, (nset, yc))
    inv, gam = np.zeros((nset, yc, lam.size)), np.zeros((nset, yc, lam.size))
    gp = np.zeros((nset, lam.size))
    with np.errstate(all='ignore'):
        for j in range(1, yc - 1):
            Aj, Ap, Cj = A[:, j, None], A[:, j + 1, None], C[:, j, None]
            lo, up, di = Aj * ratioSqr, Ap * ratioSqr, -((Ap + Aj) * ratioSqr + Cj * lam)
            inv[:, j] = 1.0 / (di if j == 1 else di - lo * gp)
            gp = up * inv[:, j]
            gam[:, j] = gp
    return inv, gam


def substitute(spec2, A, ratioSqr, inv, gam):
    x = np.array(spec2, dtype=np.float64, copy=True)
    nb, yc, K2 = x.shape
    A = np.broadcast_to(np.asarray(A, dtype=np.float64), (nb, yc))
    k = np.arange(K2) >> 1
    inv, gam = np.broadcast_to(inv, (nb,) + inv.shape[1:])[:, :, k], np.broadcast_to(gam, (nb,) + gam.shape[1:])[:, :, k]
    with np.errstate(all='ignore'):
        p = x[:, 0].copy()
        for j in range(1, yc - 1):
            r = x[:, j]
            if j == yc - 2:
                r = r - (A[:, yc - 1, None] * ratioSqr) * x[:, yc - 1]
            p = (r - (A[:, j, None] * ratioSqr) * p) * inv[:, j]
            x[:, j] = p
        for j in range(yc - 3, 0, -1):
            p = x[:, j] - gam[:, j] * p
            x[:, j] = p
    return x, (~np.isfinite(x[:, 1:-1])).any(axis=(1, 2))


def _split(X):
    """complex [..., K] -> float64 [..., 2K], re and im interleaved (the device's layout)."""
    out = np.empty(X.shape[:-1] + (2 * X.shape[-1],))
    out[..., 0::2], out[..., 1::2] = X.real, X.imag
    return out


def solve(S0, F, delxSqr, ratioSqr, factors, A, C, undef=-9.99e8):
    S = np.array(S0, dtype=np.float64, copy=True)
    nb, yc, xc = S.shape
    F = np.broadcast_to(np.asarray(F, dtype=np.float64), S.shape)
    bad = M.undef_count(S, A, C, F, undef)
    spec = np.zeros((nb, yc, xc // 2 + 1), dtype=np.complex128)
    spec[:, 1:-1] = M.rfft_rows(F[:, 1:-1], delxSqr)
    spec[:, [0, yc - 1]] = M.rfft_rows(S[:, [0, yc - 1]])
    x, ovf = substitute(_split(spec), A, ratioSqr, *factors)
    with np.errstate(all='ignore'):
        out = M.irfft_rows(x[:, 1:-1, 0::2] + 1j * x[:, 1:-1, 1::2], xc)
    keep = bad != 0
    S[~keep, 1:-1] = out[~keep]
    fl = np.zeros((nb, 3))
    fl[:, 0] = ovf
    return S, fl, bad
