"""xinvert_amd -- MI355X-native SOR inversion engine behind the xinvert call boundary.

Layout (only what the hot path needs):
  csrc/          hand-written HIP kernels for gfx950 + the C-ABI (include/xinv.h)
  _lib.py        ctypes binding of libxinv_hip.so (no CPU fallback)
  forms.py       the operator forms as one table: symbols, arrays, scalar order (what _lib, core and resident share)
  core.py        inv_standard1D / inv_standard2D / inv_general2D / inv_standard3D / inv_general3D ...   (reference xinvert/core.py)
  apps.py        invert_Poisson / invert_Stommel / invert_GillMatsuno / invert_omega, cal_flow
                 (reference xinvert/apps.py)
  dist.py        batch-axis sharding across ranks (one process per GPU) + flags gather
  field.py       minimal labelled array standing in for xarray.DataArray
  finitediffs.py FiniteDiff / deriv / deriv2 / padBCs: one HIP launch per operator (reference xinvert/finitediffs.py)
  utils.py       loop_noncore (reference xinvert/utils.py)
  tridiag.py     trace / traceCyclic: batched tridiagonal direct solves, one system per lane (reference xinvert/numbas.py)
  fourier.py     rfft_rows / irfft_rows, the eligibility tests of iParams['method'] = 'fourier' / 'cfourier' (the direct 2-D
                 solves of the standard and the general form), and FourierPlan: the factors of one operator kept across solves
  multigrid.py   invert_MultiGrid: coarse-to-fine SOR solves, HIP restriction / prolongation (reference xinvert/apps.py)
"""
from .field import Field                                           # noqa: F401
from .core import (inv_standard1D, inv_standard2D, inv_standard2D_test, inv_general2D, inv_general2D_bih,    # noqa: F401
                   inv_standard3D, inv_general3D)
from .apps import (invert_Poisson, invert_Stommel, invert_StommelMunk, invert_GillMatsuno,  # noqa: F401
                   invert_Fofonoff, invert_BrethertonHaidvogel, invert_omega, invert_3DOcean,
                   invert_RefState, invert_PV2D, invert_Eliassen, invert_GillMatsuno_test,
                   invert_Stommel_test, invert_StommelArons, invert_geostrophic,
                   invert_GeoAdjustment, invert_RefStateSWM,
                   animate_iteration, cal_flow, default_iParams, default_mParams)
from .utils import loop_noncore                                    # noqa: F401
from .finitediffs import FiniteDiff, deriv, deriv2, padBCs, DeviceField   # noqa: F401
from .multigrid import invert_MultiGrid                             # noqa: F401
from .tridiag import trace, traceCyclic                             # noqa: F401
from .fourier import rfft_rows, irfft_rows, FourierPlan             # noqa: F401

__version__ = '0.1.0'
