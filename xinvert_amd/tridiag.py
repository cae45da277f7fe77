"""trace / traceCyclic: the reference's tridiagonal direct solver (xinvert/numbas.py:1589-1685) on the GPU.

Same names and argument order as the reference.  Any leading axes form the batch: every system is solved by one lane
of the HIP kernel k_tridiag with the reference's recurrence, bit for bit (include/xinv.h, "tridiagonal systems").  A
coefficient array without the batch axes is shared by every system (batch stride 0).  numpy arrays in give a numpy array
out (host-pointer entry: upload, one solve, download); CUDA torch float64 tensors in give a tensor out, the solve
queued on the current stream (device-pointer entry).  Solves queued from several streams take turns on the device's one
scratch buffer: the library orders them.  There is no CPU fallback.
"""
import numpy as np

from . import _lib


def trace(a, b, c, d):
    """Solve a[i-1] x[i-1] + b[i] x[i] + c[i] x[i+1] = d[i]: a, c [..., N-1], b, d [..., N] -> x [..., N]."""
    return _solve(a, b, c, d, None, None)


def traceCyclic(a, b, c, d, a0, cn):
    """... with periodic corners: row 0 also holds a0 x[N-1], row N-1 also cn x[0] (scalars, or one value per system)."""
    return _solve(a, b, c, d, a0, cn)


def _is_tensor(v):
    return type(v).__module__.split('.')[0] == 'torch' and hasattr(v, 'data_ptr')


def _layout(arrs, corners):
    """-> (batch shape, nbatch, N, strides of a, b, c, d (+ a0, cn)) after the reference's length check."""
    N = arrs[1].shape[-1] if arrs[1].ndim else 0
    lens = [N - 1, N, N - 1, N]
    if any(v.ndim < 1 or v.shape[-1] != n for v, n in zip(arrs, lens)):
        raise Exception('lengths of given arrays are not satisfied')
    leads = {tuple(v.shape[:-1]) for v in arrs if v.ndim > 1} | {tuple(v.shape) for v in corners if v.ndim > 0}
    if len(leads) > 1:
        raise Exception('batch axes of the given arrays differ: %s' % sorted(leads))
    lead = leads.pop() if leads else ()
    nbatch = int(np.prod(lead)) if lead else 1
    strides = [n if v.ndim > 1 else 0 for v, n in zip(arrs, lens)] + [1 if v.ndim > 0 else 0 for v in corners]
    return lead, nbatch, N, strides


def _solve(a, b, c, d, a0, cn):
    cyclic = a0 is not None
    if any(_is_tensor(v) for v in (a, b, c, d)):
        return _solve_torch(a, b, c, d, a0, cn)
    if cyclic and any(_is_tensor(v) for v in (a0, cn)):
        raise _lib.XinvError('trace / traceCyclic take numpy arrays, or CUDA float64 tensors on one device')
    arrs = [np.ascontiguousarray(v, dtype=np.float64) for v in (a, b, c, d)]
    corners = [np.require(v, dtype=np.float64, requirements='C') for v in (a0, cn)] if cyclic else []     # (a scalar stays 0-d)
    lead, nbatch, N, strides = _layout(arrs, corners)
    if nbatch == 0:
        return np.zeros(lead + (N,))
    L = _lib.require_gpu()
    x = np.empty(lead + (N,))
    ptrs = [_lib.hptr(v) for v in arrs] + ([_lib.hptr(v.reshape(-1)) for v in corners] if cyclic else [None, None])
    _lib.check(L.xinv_tridiag_f64(_lib.hptr(x), *ptrs, nbatch, _lib.strides_arg([N] + strides), N))
    return x


def _solve_torch(a, b, c, d, a0, cn):
    import torch
    cyclic = a0 is not None
    arrs = [a, b, c, d]
    dev = next(v.device for v in arrs if _is_tensor(v))
    corners = [v if _is_tensor(v) else torch.tensor(float(v), dtype=torch.float64, device=dev) for v in (a0, cn)] \
        if cyclic else []
    for v in arrs + corners:
        if not _is_tensor(v) or v.dtype != torch.float64 or v.device != dev or dev.type != 'cuda':
            raise _lib.XinvError('trace / traceCyclic take numpy arrays, or CUDA float64 tensors on one device')
    arrs = [v.contiguous() for v in arrs]
    corners = [v.contiguous() for v in corners]
    lead, nbatch, N, strides = _layout(arrs, corners)
    x = torch.empty(lead + (N,), dtype=torch.float64, device=dev)
    if nbatch == 0:
        return x
    L = _lib.require_gpu()
    ptrs = [_lib.dptr(v) for v in [x] + arrs + (corners if cyclic else [None, None])]
    with torch.cuda.device(dev):
        _lib.check(L.xinv_tridiag_f64_dev(*ptrs, nbatch, _lib.strides_arg([N] + strides), N, _lib.stream_arg(dev)))
    return x
