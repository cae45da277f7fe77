"""Small helpers of the reference's xinvert/utils.py."""
import itertools

import numpy as np


def loop_noncore(data, dims=None):
    """Yield one {dim: coordinate value} per combination of the non-core dims of `data` (reference utils.py:10-51).

    The core dims are `dims`; every other dim of data, in data's order, is looped over.  With no non-core dim the
    single yield is {}.  Deviation: the reference yields inside its inner loop, so with two or more non-core dims it
    also yields partial dicts; here each combination is yielded once, complete, which is what the reference's own
    caller (core.py:59, `data.loc[selDict]`) needs."""
    dims = [] if dims is None else ([dims] if isinstance(dims, str) else list(dims))
    nonc = [d for d in data.dims if d not in dims]
    if not nonc:
        yield {}
        return
    values = [np.asarray(data.coords[d].values if hasattr(data.coords[d], 'values') else data.coords[d])
              if d in data.coords else np.arange(data.shape[data.dims.index(d)]) for d in nonc]
    for idx in itertools.product(*values):
        yield dict(zip(nonc, idx))
