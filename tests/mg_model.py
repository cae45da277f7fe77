"""numpy restatement of the multigrid grid transfers k_mg_restrict / k_mg_prolong (xinvert_amd/csrc/xinv_mg.h), in the
kernels' order of operations, so that the GPU tests can compare them bit for bit.  Arrays are [nbatch, *core] with 1 to
3 core dims."""
import numpy as np


def restrict(fine, ratios, undef):
    """Coarse point = block sum over the points that are not `undef` (NaN undef: the NaN points), ((0.0 + v0) + v1) + ...
    in lexicographic offset order (slowest axis first), divided once by the count; `undef` for an empty block."""
    fine = np.asarray(fine, dtype=np.float64)
    nd = fine.ndim - 1
    m = [n // r for n, r in zip(fine.shape[1:], ratios)]
    acc = np.zeros((fine.shape[0],) + tuple(m))
    cnt = np.zeros_like(acc)
    for offs in np.ndindex(*ratios):
        sl = (slice(None),) + tuple(slice(o, o + k * r, r) for o, k, r in zip(offs, m, ratios))
        v = fine[sl]
        ok = (v == v) if np.isnan(undef) else (v != undef)
        acc = np.where(ok, acc + v, acc)
        cnt = np.where(ok, cnt + 1.0, cnt)
    assert nd == len(ratios)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(cnt > 0.0, acc / cnt, undef)


def prolong(coarse, fine0, tables, keep_edges=0, force=None, undef=-9.99e8):
    """fine0 with every point replaced by the d-linear blend of `coarse`, nested from the slowest core axis to the
    fastest, except where force == undef, on the edges of the axes in keep_edges, and where the blend is not finite."""
    coarse = np.asarray(coarse, dtype=np.float64)
    out = np.array(fine0, dtype=np.float64, copy=True)
    nd = out.ndim - 1
    fshape = out.shape[1:]

    def blend(c, a):
        # c: coarse values with axes < a already fixed to fine indices ([nb, f0, .., f_{a-1}, c_a, ...])
        if a == nd:
            return c
        lo, hi, w = (np.asarray(x) for x in tables[a])
        shp = [1] * (1 + nd)
        shp[1 + a] = fshape[a]
        w = w.reshape(shp)
        cl, ch = np.take(c, lo, axis=1 + a), np.take(c, hi, axis=1 + a)
        return (1.0 - w) * blend(cl, a + 1) + w * blend(ch, a + 1)

    with np.errstate(invalid='ignore', over='ignore'):
        v = blend(coarse, 0)
    write = np.isfinite(v)
    if force is not None:
        write &= np.asarray(force) != undef
    for a in range(nd):
        if keep_edges >> a & 1:
            idx = np.arange(fshape[a])
            edge = (idx == 0) | (idx == fshape[a] - 1)
            shp = [1] * (1 + nd)
            shp[1 + a] = fshape[a]
            write &= ~edge.reshape(shp)
    out[write] = v[write]
    return out
