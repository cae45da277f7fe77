"""xinv_tridiag_f64_dev only queues its kernel, and the kernel keeps buf1 (cyclic: and the two auxiliary solves) in the
device's one scratch buffer between its forward and its backward pass.  Solves queued from two streams would run side by
side and overwrite each other's buf1; the library orders every user of the buffer behind the one before it
(Workspace::tri_user, xinv_host.h).  Here two streams queue solves on different data back to back -- 64 systems
are ONE workgroup, so two such kernels fit on the device together many times over, and 4000 points keep each running for
milliseconds while the next call is queued in microseconds -- and every result must be the model's bits."""
import numpy as np
import pytest

import tridiag_model as M
import xinvert_amd as xa
from xinvert_amd import _lib

pytestmark = pytest.mark.gpu
UNDEF = -9.99e8
NB, N = 64, 4000


def bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb])


def systems(seed):
    rng = np.random.default_rng(seed)
    a, c = rng.uniform(-1, 1, (NB, N - 1)), rng.uniform(-1, 1, (NB, N - 1))
    b = rng.uniform(2.5, 4.0, (NB, N)) * rng.choice([-1.0, 1.0], (NB, N))
    return a, b, c, rng.standard_normal((NB, N))


def test_solves_queued_on_two_streams_do_not_share_buf1():
    import torch
    dev = torch.device('cuda', 0)
    up = lambda arrs: [torch.tensor(v, dtype=torch.float64, device=dev) for v in arrs]
    host = [systems(k) for k in range(4)]
    want = [M.trace(*h) for h in host]
    wantc = M.traceCyclic(*host[0], 0.3, -0.2)
    # a member batch of the 1-D form, for the direct path: the third user of the buffer
    rng = np.random.default_rng(9)
    A, B = rng.uniform(0.5, 1.5, N), rng.uniform(-0.5, -0.1, (NB, N))
    F, S0 = rng.standard_normal((NB, N)), np.zeros((NB, N))
    Sm, flm = M.direct_solve(S0, A, B, F, 'fixed', 0.49, UNDEF)
    onc = [up(h) for h in host]
    S, Ad, Bd, Fd = up((S0, A, B, F))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    got = [None] * 4
    for rnd in range(2):                                      # the same buffer size again: no regrowth the second time
        for k in range(4):
            with torch.cuda.stream((s1, s2)[k % 2]):
                got[k] = xa.trace(*onc[k])
    with torch.cuda.stream(s1):
        gotc = xa.traceCyclic(*onc[0], 0.3, -0.2)             # (three arrays: the buffer grows under a queued solve)
    with torch.cuda.stream(s2):
        got3 = xa.trace(*onc[3])
        L = _lib.require_gpu()
        fl = np.tile([0.0, 1.0, 0.0], (NB, 1))
        rc = L.xinv_standard_1d_f64_dev(S.data_ptr(), Ad.data_ptr(), Bd.data_ptr(), Fd.data_ptr(), NB,
                                        _lib.strides_arg([N, 0, N, N]), N, 1.0, _lib.bc('fixed'), 0.49, 1.5, UNDEF,
                                        _lib.hptr(fl), 5, 1e-8, _lib.options(path=_lib.PATH_DIRECT1D), s2.cuda_stream)
    torch.cuda.synchronize()
    bad = [k for k in range(4) if not bits_equal(got[k].cpu().numpy(), want[k])]
    assert not bad, bad
    assert bits_equal(gotc.cpu().numpy(), wantc)
    assert bits_equal(got3.cpu().numpy(), want[3])
    assert rc == 0 and bits_equal(S.cpu().numpy(), Sm) and bits_equal(fl, flm)
