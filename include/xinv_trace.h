/*
 * xinv_trace.h -- the tridiagonal direct solver of libxinv_hip.so: numbas.trace / numbas.traceCyclic
 * (reference numbas.py:1589-1685).  Included by xinv.h, which describes the arguments ("tridiagonal systems"); it may
 * also be included alone.  Implemented in xinvert_amd/csrc/xinv_hip.hip over the kernel k_tridiag (xinv_tridiag.h).
 */
#ifndef XINV_TRACE_H
#define XINV_TRACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* host pointers: upload (a shared array once), one solve, download x */
int xinv_tridiag_f64(double *x, const double *a, const double *b, const double *c, const double *d, const double *a0,
                     const double *cn, int64_t nbatch, const int64_t *strides, int64_t n);

/* device pointers; the solve is queued on `stream` */
int xinv_tridiag_f64_dev(double *x, const double *a, const double *b, const double *c, const double *d, const double *a0,
                         const double *cn, int64_t nbatch, const int64_t *strides, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* XINV_TRACE_H */
