#!/usr/bin/env python3
"""Throughput of the finite-difference kernel (k_fd, xinvert_amd/csrc/xinv_fd.h) on one GPU.

Times curl, divg, Laplacian and two-dim grad on device-resident 8 x 1800 x 3600 float64 fields (DeviceField ->
xinv_fd_f64_dev) with HIP events after warm-up, and reports algorithmic bytes over the event time: every input read
once plus every output written once.  `--host` adds the end-to-end time of FiniteDiff.curl on host arrays (PCIe
transfers included) against the numpy restatement tests/fd_model.py at the same size.

  python tools/bench_fd.py [--reps N] [--host]
Kernel times without launch gaps: run it under  rocprofv3 --kernel-trace --stats -d DIR -o fd -- python tools/bench_fd.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from xinvert_amd import FiniteDiff, Field          # noqa: E402
from xinvert_amd.finitediffs import DeviceField    # noqa: E402

SHAPE = (8, 1800, 3600)
COPY_TBS = 6.29                                     # measured float4 copy rate of the MI355X (TB/s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host', action='store_true')
    args = ap.parse_args()
    import torch
    dev = torch.device('cuda', 0)
    lat = np.linspace(-90, 90, SHAPE[1])
    lon = np.arange(SHAPE[2]) * 0.1
    dims = ('time', 'lat', 'lon')
    crd = {'time': np.arange(float(SHAPE[0])), 'lat': lat, 'lon': lon}
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    u, v = (DeviceField(torch.randn(SHAPE, dtype=torch.float64, device=dev, generator=g), dims, crd) for _ in range(2))
    fd = FiniteDiff({'T': 'time', 'Y': 'lat', 'X': 'lon'}, BCs={'Y': 'reflect', 'X': 'periodic'})
    cases = [('curl', lambda: fd.curl(u, v), 2, 1),
             ('divg', lambda: fd.divg([u, v], ['X', 'Y']), 2, 1),
             ('Laplacian', lambda: fd.Laplacian(u, ['X', 'Y']), 1, 1),
             ('grad2', lambda: fd.grad(u, ['X', 'Y']), 1, 2)]
    n = int(np.prod(SHAPE))
    for name, fn, nin, nout in cases:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(args.reps):
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        byts = (nin + nout) * 8 * n
        best = min(ms)
        print(json.dumps({'op': name, 'shape': SHAPE, 'bytes': byts, 'event_ms_min': round(best, 4),
                          'event_ms_median': round(float(np.median(ms)), 4),
                          'TBps_event_min': round(byts / best / 1e9, 3),
                          'frac_of_copy_rate': round(byts / best / 1e9 / COPY_TBS, 3)}), flush=True)
    if args.host:
        import fd_model as M
        rng = np.random.default_rng(0)
        hu, hv = (Field(rng.standard_normal(SHAPE), dims, crd) for _ in range(2))
        fd.curl(hu, hv)
        t0 = time.perf_counter()
        fd.curl(hu, hv)
        t1 = time.perf_counter()
        md = M.FiniteDiff(fd.dmap, fd.BCs, fd.fill)
        md.curl(hu, hv)
        t2 = time.perf_counter()
        print(json.dumps({'op': 'curl_host_end_to_end', 'shape': SHAPE, 'hip_s_incl_pcie': round(t1 - t0, 3),
                          'numpy_model_s': round(t2 - t1, 3)}), flush=True)


if __name__ == '__main__':
    main()
