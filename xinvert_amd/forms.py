"""The operator forms of include/xinv.h as ONE table: what the binding, the front end, the resident batch and the test
helpers need to know about a form's positional argument list (taken from the reference's numba kernels).

Every form has up to four entry points: 'single' (one slice, host pointers), 'batched' (host pointers), 'dev' (device
pointers) and 'plan' (xinv_plan_create_*_dev).  Their parameters are, in order: S (plan: the handle's address), the
coefficient arrays with the forcing last, `nbatch, strides` (not single), the form's scalars, `flags, mxLoop, tolerance`
(not plan), `opt` (not single, except the 1-D form), `stream` (dev, plan).  tests/test_host.py holds the table to the header.

The five second-order forms (RESIDUAL) also have 'resid_dev' and 'resid_batched' (include/xinv_resid.h): `R, S`, the arrays,
`nbatch, strides`, the same scalars, `norms`, then `stream` / `opt`.
"""
import ctypes
from collections import namedtuple

from . import _lib

# name: 'standard_2d' -> the C symbols xinv_standard_2d_f64[...], and the oracle's function of that name (a string only)
# inv: the core.inv_* front-end call; arrays: the letters after S; null_B: array 1 (B) may travel as NULL (identically 0)
# scalars: the names between the arrays and `flags`; resident: has a plan entry (and so runs as a ResidentProblem)
# single_opt: the single-slice entry takes `opt`
Form = namedtuple('Form', 'kind name inv rank arrays null_B scalars resident single_opt')

_GRID2 = 'yc xc dely delx BCy BCx '
_GRID3 = 'zc yc xc delz dely delx BCz BCy BCx '


def _form(kind, name, inv, rank, arrays, scalars, null_B=False, resident=True, single_opt=False):
    return Form(kind, name, inv, rank, arrays, null_B, tuple((scalars + ' optArg undef').split()), resident, single_opt)


FORMS = {f.kind: f for f in (
    _form('std2d', 'standard_2d', 'inv_standard2D', 2, 'ABCF', _GRID2 + 'delxSqr ratioQtr ratioSqr', null_B=True),
    _form('gen2d', 'general_2d', 'inv_general2D', 2, 'ABCDEFG', _GRID2 + 'delxSqr ratio ratioQtr ratioSqr', null_B=True),
    _form('std3d', 'standard_3d', 'inv_standard3D', 3, 'ABCF', _GRID3 + 'delxSqr ratio2Sqr ratio1Sqr'),
    _form('bih2d', 'general_bih_2d', 'inv_general2D_bih', 2, 'ABCDEFGHIJ',
          _GRID2 + 'delxSSr delxTr delxSqr ratio ratioSSr ratioQtr ratioSqr'),
    _form('std2dt', 'standard_2d_test', 'inv_standard2D_test', 2, 'ABCDEF', _GRID2 + 'delxSqr ratioQtr ratioSqr'),
    _form('gen3d', 'general_3d', 'inv_general3D', 3, 'ABCDEFGH', _GRID3 + 'delxSqr ratio2 ratio1 ratio2Sqr ratio1Sqr'),
    _form('std1d', 'standard_1d', 'inv_standard1D', 1, 'ABF', 'xc delx BCx delxSqr', resident=False, single_opt=True),
)}

# the forms xinv_residual_* exists for, in the order of include/xinv_resid.h
RESIDUAL = ('std2d', 'gen2d', 'std2dt', 'std3d', 'gen3d')

# a scalar's iParams key where it is not the scalar's own name (BC codes: iParams['BCs'] by position; undef: the caller's)
IPARAM = {'xc': 'gc1', 'yc': 'gc2', 'zc': 'gc3', 'delx': 'del1', 'dely': 'del2', 'delz': 'del3',
          'delxSqr': 'del1Sqr', 'delxSSr': 'del1SSr', 'delxTr': 'del1Tr'}

_i64, _f64, _int, _vp = ctypes.c_int64, ctypes.c_double, ctypes.c_int, ctypes.c_void_p
_dp, _ip, _opt = ctypes.POINTER(_f64), ctypes.POINTER(_i64), ctypes.POINTER(_lib.XinvOptions)


def _ctype(scalar):
    """Grid counts are int64_t, boundary codes int, everything else double."""
    return _i64 if scalar in ('xc', 'yc', 'zc') else _int if scalar.startswith('BC') else _f64


def symbol(kind, entry):
    f = FORMS[kind]
    if entry == 'plan' and not f.resident:
        raise KeyError('the %s form has no plan entry' % kind)
    if entry.startswith('resid_') and kind not in RESIDUAL:
        raise KeyError('the %s form has no residual entry' % kind)
    return {'resid_dev': 'xinv_residual_%s_f64_dev', 'resid_batched': 'xinv_residual_%s_f64_batched',
            'single': 'xinv_%s_f64', 'batched': 'xinv_%s_f64_batched', 'dev': 'xinv_%s_f64_dev',
            'plan': 'xinv_plan_create_%s_f64_dev'}[entry] % f.name


def params(kind, entry):
    """[(name, ctypes type)] of the entry point's prototype.  Host entries take the arrays as double *; the device
    entries as addresses (integers); `flags` is a host array everywhere."""
    f = FORMS[kind]
    symbol(kind, entry)                                  # (raises for an entry the form does not have)
    arr =_dp if entry in ('single', 'batched', 'resid_batched') else _vp
    ps = [('plan', ctypes.POINTER(_vp))] if entry == 'plan' else [('S', arr)]
    if entry.startswith('resid_'):
        ps.insert(0, ('R', arr))
    ps += [(a, arr) for a in f.arrays]
    if entry != 'single':
        ps += [('nbatch', _i64), ('strides', _ip)]
    ps += [(s, _ctype(s)) for s in f.scalars]
    if entry.startswith('resid_'):
        return ps + [('norms', _dp), ('stream', _vp) if entry == 'resid_dev' else ('opt', _opt)]
    if entry != 'plan':
        ps += [('flags', _dp), ('mxLoop', _i64), ('tolerance', _f64)]
    if entry != 'single' or f.single_opt:
        ps.append(('opt', _opt))
    if arr is _vp:
        ps.append(('stream', _vp))
    return ps


def argtypes(kind, entry):
    return [t for _, t in params(kind, entry)]


def scalars(p):
    """Problem dict -> the positional scalar arguments between the arrays and `flags` (BC names coded)."""
    return [_lib.bc(p[s]) if s.startswith('BC') else p[s] for s in FORMS[p['kind']].scalars]


def from_iparams(kind, iParams, undef):
    """The scalar part of a problem dict out of the front end's iParams."""
    p = dict(kind=kind, undef=undef)
    BCs = iter(iParams['BCs'])
    for s in FORMS[kind].scalars:
        if s.startswith('BC'):
            p[s] = next(BCs)
        elif s != 'undef':
            p[s] = (int if _ctype(s) is _i64 else float)(iParams[IPARAM.get(s, s)])
    return p
