"""A long-double truth for the direct Fourier solve of the 2-D general form for periodic x ("General form"),
without a GPU and without tests/fourier_general_model.py: only the equation in the header of
xinvert_amd/csrc/xinv_cfourier.h is shared.

    ld_solve(S0, c, G, sc) -> S      the full xc x xc DFT matrix (fourier_ld._dft_matrix), one complex Thomas recurrence
                                     per wavenumber k = 0 .. xc-1
    ld_backward(S, c, G, sc) -> [nbatch]   max|R| / max|G| of the reference stencil's fixed-point equation (numbas.py:1092-1184
                                     with B == 0), evaluated directly on the grid, the columns wrapping along x
c = (A, C, D, E, Fc), one value per row, [yc] or [nbatch, yc]; sc = (delx, delxSqr, ratio, ratioSqr); S0, G [nbatch, yc, xc]
or [yc, xc].  Everything is numpy.longdouble.  Inputs are left alone.
"""
import numpy as np

from fourier_ld import CLD, LD, PI, _dft_matrix


def _batched(S0, c, G):
    S = np.asarray(S0)
    one = S.ndim == 2
    S = S.astype(LD).reshape((-1,) + S.shape[-2:])
    G = np.asarray(G).astype(LD).reshape(S.shape)
    nb, yc, _ = S.shape
    c = [np.broadcast_to(np.asarray(x).astype(LD), (nb, yc)) for x in c]
    return one, S, c, G


def ld_solve(S0, c, G, sc):
    one, S, (A, C, D, E, Fc), G = _batched(S0, c, G)
    nb, yc, xc = S.shape
    delx, dx2, ratio, rs = (LD(v) for v in sc)
    W = _dft_matrix(xc)
    k = np.arange(xc, dtype=LD)
    s = np.sin(PI * k / LD(xc))
    lam = LD(4) * s * s                                                      # [xc]
    sig = np.sin(LD(2) * PI * k / LD(xc))
    Wr, Wi = W.real, W.imag

    rows = lambda x: x.reshape(-1, xc).T

    def dft(x):                                              # real rows: two real products (W is symmetric: W x^T walks its rows)
        out = np.empty(x.shape, dtype=CLD)
        out.real, out.imag = (Wr @ rows(x)).T.reshape(x.shape), (Wi @ rows(x)).T.reshape(x.shape)
        return out

    rhs = np.zeros((nb, yc, xc), dtype=CLD)                                  # rows 0 and yc-1 are not used
    rhs[:, 1:-1] = dft(G[:, 1:-1] * dx2)
    bottom, top = dft(S[:, 0]), dft(S[:, yc - 1])
    half = D * ratio * delx / LD(2)
    sub, sup = A * rs - half, A * rs + half                                  # the coefficients of X[j-1], X[j+1] in row j
    dia = np.empty((nb, yc, xc), dtype=CLD)
    dia.real = -(LD(2) * (A * rs)[:, :, None] + C[:, :, None] * lam) + (Fc * dx2)[:, :, None]
    dia.imag = (E * delx)[:, :, None] * sig
    rhs[:, 1] = rhs[:, 1] - sub[:, 1, None] * bottom
    rhs[:, yc - 2] = rhs[:, yc - 2] - sup[:, yc - 2, None] * top
    cp = np.zeros((nb, yc, xc), dtype=CLD)
    dp = np.zeros((nb, yc, xc), dtype=CLD)
    cp[:, 1] = sup[:, 1, None] / dia[:, 1]
    dp[:, 1] = rhs[:, 1] / dia[:, 1]
    for j in range(2, yc - 1):
        den = dia[:, j] - sub[:, j, None] * cp[:, j - 1]
        cp[:, j] = sup[:, j, None] / den
        dp[:, j] = (rhs[:, j] - sub[:, j, None] * dp[:, j - 1]) / den
    X = np.zeros((nb, yc, xc), dtype=CLD)
    X[:, yc - 2] = dp[:, yc - 2]
    for j in range(yc - 3, 0, -1):
        X[:, j] = dp[:, j] - cp[:, j] * X[:, j + 1]
    out = S.copy()
    Xi = X[:, 1:-1]
    out[:, 1:-1] = ((Wr @ rows(Xi.real) + Wi @ rows(Xi.imag)) / LD(xc)).T.reshape(Xi.shape)      # Re(X conj(W)) / xc
    return out[0] if one else out


def ld_backward(S, c, G, sc):
    """[nbatch] max|R| / max|G| over rows 1 .. yc-2; R is the sweep's `temp` before optArg, over delxSqr."""
    _, S, (A, C, D, E, Fc), G = _batched(S, c, G)
    delx, dx2, ratio, rs = (LD(v) for v in sc)
    mid, lo, up = S[:, 1:-1], S[:, :-2], S[:, 2:]
    east, west = np.roll(mid, -1, axis=2), np.roll(mid, 1, axis=2)
    a, cc, d, e, f = (x[:, 1:-1, None] for x in (A, C, D, E, Fc))
    R = (a * ((up - mid) - (mid - lo)) * rs + cc * ((east - mid) - (mid - west)) +
         (d * (up - lo) * ratio + e * (east - west)) * delx / LD(2) + (f * mid - G[:, 1:-1]) * dx2)
    return np.abs(R).max(axis=(1, 2)) / (np.abs(G[:, 1:-1]).max(axis=(1, 2)) * dx2)
