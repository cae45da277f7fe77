"""A batch of slices kept resident in HBM across solves (the `*_dev` entry points of include/xinv.h).

The host-pointer entry points upload the coefficient stack on every call.  Callers that solve the
same operator repeatedly -- `apps.animate_iteration` (reference apps.py:1031-1044: one
`invt_func(...)` per frame on the same coefficients), restarts, the benchmark -- upload once with
this class and then call `solve()` as often as they like: only the flags cross PCIe.  torch is used
for device memory and streams only; every solve goes through the C-ABI.

A problem is the dict the parity tests and `xinvert_amd.synthetic` use: kind, S0 [nb, ...core],
coefs (list, last one = forcing), shared (indices of coefficient arrays given once for the whole
batch), the grid counts and the derived scalars under the reference's argument names.
"""
import ctypes

import numpy as np

from . import _lib, forms

# the forms a batch can be resident for (xinvert_amd/forms.py): C symbol stems, plan constructors, positional scalars
FN = {k: forms.symbol(k, 'single') for k, f in forms.FORMS.items() if f.resident}
PLAN_FN = {k: forms.symbol(k, 'plan') for k in FN}
scalars = forms.scalars


class ResidentProblem:
    """Upload once, solve many times.  `members`: optional (lo, hi) block of the batch axis this
    process owns (batch-axis sharding, xinvert_amd.dist).

    plan=True (default): every `solve()` runs on a resident PLAN (include/xinv.h, xinv_plan_*): what the engine derives
    from the coefficient stack -- is B zero, which arrays are constant along x, per-row records, the forcing's activity
    map, row split and tile lists -- is built once per set of engine options, on the first solve with them, and kept in
    HBM next to the stack.  Coefficients that are stride-0 views along x (the lat-lon builders of apps.py) are uploaded
    as ONE value per row (rowconst_mask): the plan expands them on the device and never has to test them.
    The coefficient arrays (and the forcing's set of undefined points) must not change while the object lives; after
    writing into `coefs[k]` call `refresh()`.  plan=False: every solve goes through xinv_<form>_f64_dev and re-derives
    all of it (what rounds 1-4 did)."""

    def __init__(self, p, device=0, members=None, null_zero_B=True, plan=True):
        import torch
        self.L = _lib.require_gpu()
        self.kind = p['kind']
        self.p = {k: v for k, v in p.items() if k not in ('S0', 'coefs')}
        self.dev = torch.device('cuda', device)
        self.device = device
        self.use_plan = bool(plan)
        self._plans = {}
        self._fplan = None                                   # the Fourier plan (solve_fourier), made on first use
        S0 = np.asarray(p['S0'])
        form = forms.FORMS[self.kind]
        core_nd = form.rank
        if S0.ndim == core_nd:
            S0 = S0[None]
        lo, hi = members if members is not None else (0, S0.shape[0])
        self.lo, self.hi = lo, hi
        self.nb = hi - lo
        self.core = S0.shape[1:]
        self.n = int(np.prod(self.core))
        self.rows = self.n // self.core[-1]
        shared = tuple(p.get('shared', ()))
        def up(a):
            a = np.ascontiguousarray(a, dtype=np.float64)
            return torch.from_numpy(a if a.flags.writeable else a.copy()).to(self.dev)    # (a view of a broadcast array is read-only)
        self.S0 = up(S0[lo:hi])
        self.S = self.S0.clone()
        self.coefs, strides = [], [self.n]
        self.rowconst = 0                                    # bit k: coefs[k] holds one value per row
        ncoef = len(p['coefs'])
        for k, c in enumerate(p['coefs']):
            c = np.asarray(c)
            is_shared = k in shared or c.ndim == core_nd
            # a stride-0 view along x (lat-lon coefficients: functions of latitude): only the rows travel
            rc = self.use_plan and k < ncoef - 1 and c.strides[-1] == 0 and c.shape[-1] > 1
            if is_shared:
                # the cross coefficient B of the 2-D standard / general forms travels as NULL when it
                # is identically zero, exactly as the front end hands it over (core._prep_coef)
                if null_zero_B and k == 1 and form.null_B and not c.any():
                    self.coefs.append(None)
                elif rc:
                    self.coefs.append(up(c[..., 0])); self.rowconst |= 1 << k
                else:
                    self.coefs.append(up(c))
                strides.append(0)
            elif rc:
                self.coefs.append(up(c[lo:hi][..., 0])); self.rowconst |= 1 << k
                strides.append(self.rows)
            else:
                self.coefs.append(up(c[lo:hi]))
                strides.append(self.n)
        self._strides = list(strides)
        self._last_stream = None                             # a non-current stream a solve left S completing on (_join)
        self.strides = _lib.strides_arg(strides)
        self.flags = np.tile(np.array([0., 1., 0.]), (self.nb, 1))
        torch.cuda.synchronize(self.dev)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def close(self):
        """Destroy the plans (their HBM: per-row records, tile lists, expanded row-constant coefficients)."""
        plans, self._plans = getattr(self, '_plans', {}), {}
        for h in plans.values():
            self.L.xinv_plan_destroy(h)
        self._drop_fourier_plan()

    def _drop_fourier_plan(self):
        fp, self._fplan = getattr(self, '_fplan', None), None
        if fp is not None:
            fp.close()

    def _join(self):
        """A plan solve returns with S completing in stream order on ITS stream.  Everything that reads or overwrites S
        afterwards runs on torch's current stream: when the solve was given another stream, make the current one wait
        for it first (no host synchronisation)."""
        import torch
        last, self._last_stream = self._last_stream, None
        if last is not None:
            cur = torch.cuda.current_stream(self.dev)
            if cur.cuda_stream != last.cuda_stream:
                cur.wait_stream(last)

    def reset(self):
        self._join()
        self.S.copy_(self.S0)

    def refresh(self):
        """The coefficient arrays (or the forcing's mask) were changed in place: re-derive every plan."""
        import torch
        self._join()
        st = _lib.stream_arg(self.dev)
        for h in self._plans.values():
            _lib.check(self.L.xinv_plan_refresh(h, st))
        self._drop_fourier_plan()                            # (its factors are the old A and C: remade on the next solve_fourier)

    def _plan(self, opt, st):
        key = tuple(sorted(opt.items()))
        h = self._plans.get(key)
        if h is None:
            o = _lib.options(device=self.device, rowconst_mask=self.rowconst, **opt)
            h = ctypes.c_void_p()
            rc = getattr(self.L, PLAN_FN[self.kind])(
                ctypes.byref(h), *[_lib.dptr(c) for c in self.coefs], self.nb, self.strides, *scalars(self.p),
                ctypes.byref(o), ctypes.c_void_p(st.cuda_stream))
            _lib.check(rc)
            self._plans[key] = h
        return h

    def solve(self, mxLoop, tolerance, stream=None, **opt):
        """One call of the hot path on the resident batch: S is updated in place (restartable, as
        the reference's kernels).  Returns (flags [nb, 3], stats)."""
        import torch
        cur = torch.cuda.current_stream(self.dev)
        st = stream if stream is not None else cur
        if st.cuda_stream != cur.cuda_stream:                # (what the current stream queued on S -- a reset -- comes first)
            self._join()
            st.wait_stream(cur)
            self._last_stream = st
        else:
            self._join()
        self.flags[:] = np.array([0., 1., 0.])
        if self.use_plan:
            h = self._plan(opt, st)
            rc = self.L.xinv_plan_solve_f64_dev(h, _lib.dptr(self.S), _lib.hptr(self.flags),
                                                int(mxLoop), float(tolerance), ctypes.c_void_p(st.cuda_stream))
            _lib.check(rc)
            return self.flags, _lib.last_stats()
        o = _lib.options(device=self.device, **opt)
        rc = getattr(self.L, FN[self.kind] + '_dev')(
            _lib.dptr(self.S), *[_lib.dptr(c) for c in self.coefs], self.nb, self.strides, *scalars(self.p),
            _lib.hptr(self.flags), int(mxLoop), float(tolerance), ctypes.byref(o),
            ctypes.c_void_p(st.cuda_stream))
        _lib.check(rc)
        return self.flags, _lib.last_stats()

    def solve_frames(self, frames, mxLoop, tolerance, stream=None, **opt):
        """`frames.shape[0]` restarts of the solve queued behind each other (include/xinv.h: xinv_plan_solve_frames_f64_dev):
        frame f continues from frame f-1's S, which is copied into `frames[f]` (a torch tensor [nframes, *S.shape] on this
        device).  -> flags [nframes, nb, 3].  No host round trip between the frames while every frame runs its whole budget."""
        import torch
        assert self.use_plan, 'solve_frames runs on a resident plan'
        assert frames.is_cuda and frames.dtype == self.S.dtype and tuple(frames.shape[1:]) == tuple(self.S.shape) and frames.is_contiguous()
        cur = torch.cuda.current_stream(self.dev)
        st = stream if stream is not None else cur
        self._join()
        if st.cuda_stream != cur.cuda_stream:
            st.wait_stream(cur)
        nf = int(frames.shape[0])
        fl = np.tile(np.array([0., 1., 0.]), (nf, self.nb, 1))
        h = self._plan(opt, st)
        rc = self.L.xinv_plan_solve_frames_f64_dev(h, _lib.dptr(self.S), _lib.dptr(frames), nf,
                                                   int(self.S.numel()), _lib.hptr(fl), int(mxLoop), float(tolerance),
                                                   ctypes.c_void_p(st.cuda_stream))
        _lib.check(rc)
        self.flags[:] = fl[-1]
        return fl, _lib.last_stats()

    # ---- the direct Fourier solve on the resident batch (xinvert_amd/fourier.py: FourierPlan) ------------------------
    def _fourier_plan(self):
        """The batch's FourierPlan, made on first use: the eligibility test of the front end on the resident data (B zero,
        BCs, A and C one value per row or constant along x -- one comparison on the device --, the row length), then the
        factors.  `refresh()` drops it."""
        from . import fourier
        import torch
        if self._fplan is not None:
            return self._fplan
        if self.kind != 'std2d':
            fourier.resident_eligible(self.kind, False, None, None, (), 0, 0)
        yc, xc = self.core
        B = self.coefs[1]
        rows, varies = {}, []
        for name, k in (('A', 0), ('C', 2)):
            c = self.coefs[k]
            if not (self.rowconst >> k) & 1:
                first = c[..., :1]
                if not bool(((c == first) | (torch.isnan(c) & torch.isnan(first))).all()):
                    varies.append(name)
                c = c[..., 0].contiguous()
            rows[name] = c
        fourier.resident_eligible(self.kind, B is not None and bool((B != 0).any()), self.p['BCy'], self.p['BCx'], varies, yc, xc)
        self._fplan = fourier.FourierPlan(rows['A'], rows['C'], self.nb, yc, xc, self.p['delxSqr'], self.p['ratioSqr'],
                                          undef=self.p['undef'], device=self.device)
        return self._fplan

    def solve_fourier(self, stream=None, wait=True):
        """The direct Fourier solve of the resident batch (2-D standard form, B zero, BCs fixed / periodic, A and C constant
        along x: DESIGN.md 4.16) on a plan that is made on first use and kept: S rows 1 .. yc-2 are overwritten with the
        solution of the forcing `coefs[-1]` as it stands now (writing a new forcing into it needs no `refresh()`).
        wait=True -> flags [nb, 3] = [overflow, 0, 0]; wait=False queues only and returns None: `fourier_status()` has the
        flags.  A member that holds `undef` where the solve reads keeps its S; the status raises XinvError naming it."""
        import torch
        with torch.cuda.device(self.dev):
            plan = self._fourier_plan()
        cur = torch.cuda.current_stream(self.dev)
        st = stream if stream is not None else cur
        if st.cuda_stream != cur.cuda_stream:
            self._join()
            st.wait_stream(cur)
            self._last_stream = st
        else:
            self._join()
        plan.solve(self.S, self.coefs[-1], stream=st)
        return self.fourier_status() if wait else None

    def fourier_status(self):
        """Wait for the last `solve_fourier` -> flags [nb, 3] (also `self.flags`)."""
        if self._fplan is None:
            raise _lib.XinvError('fourier_status: no solve_fourier has been queued')
        try:
            self._fplan.status()
        finally:
            self.flags[:] = self._fplan.flags
        return self.flags

    def full_arrays(self):
        """The coefficient stack as the entries that take full arrays want it -> (arrays, strides of S and the arrays):
        a coefficient kept as one value per row is expanded along x (a fresh tensor on the current stream)."""
        cs, strides = [], [self.n]
        for k, c in enumerate(self.coefs):
            if c is not None and (self.rowconst >> k) & 1:
                c = c.unsqueeze(-1).expand(*c.shape, self.core[-1]).contiguous()
                strides.append(self.n if self._strides[1 + k] else 0)
            else:
                strides.append(self._strides[1 + k])
            cs.append(c)
        return cs, strides

    def residual(self, stream=None):
        """R = L(S) - F of the resident state, on the device (include/xinv_resid.h; S is not modified) -> (R as a torch
        tensor shaped like S, norms [nb, 4] = {n_live, mean|R|, max|R|, max|F|}).  Coefficients kept as one value per row
        are expanded for the call."""
        import torch
        if self.kind not in forms.RESIDUAL:
            raise _lib.XinvError('the %s form has no residual entry' % self.kind)
        cur = torch.cuda.current_stream(self.dev)
        st = stream if stream is not None else cur
        self._join()
        # R and the expanded coefficients belong to the current stream, which is where the caller goes on using R; the
        # call's stream waits for them, and the call returns only after its launch has run (it brings the norms back)
        R = torch.empty_like(self.S)
        cs, strides = self.full_arrays()
        if st.cuda_stream != cur.cuda_stream:
            st.wait_stream(cur)
        norms = np.zeros((self.nb, 4))
        rc = getattr(self.L, forms.symbol(self.kind, 'resid_dev'))(
            _lib.dptr(R), _lib.dptr(self.S), *[_lib.dptr(c) for c in cs], self.nb, _lib.strides_arg([self.n] + strides),
            *scalars(self.p), _lib.hptr(norms), ctypes.c_void_p(st.cuda_stream))
        _lib.check(rc)
        if st.cuda_stream != cur.cuda_stream:
            cur.wait_stream(st)
        return R, norms

    def result(self):
        self._join()
        return self.S.cpu().numpy()
