/*
 * xinv_fourier.h -- the direct Fourier solve of the 2-D standard form for periodic x, and the row transform under it.
 * Included by xinv.h, which describes the arguments ("fourier"); it may also be included after xinv.h alone
 * (xinv_options is declared there).  Implemented in xinvert_amd/csrc/xinv_hip.hip over the kernels k_rowdft,
 * k_fourier_tri and k_fourier_check (xinv_fourier.h of csrc).
 */
#ifndef XINV_FOURIER_H
#define XINV_FOURIER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* device pointers, the current device, on `stream`; returns with S and flags complete */
int xinv_fourier_standard_2d_f64_dev(double *S, const double *A, const double *C, const double *F, int64_t nbatch,
                                     const int64_t *strides, int64_t yc, int64_t xc, double delxSqr, double ratioSqr,
                                     double undef, double *flags, void *stream);

/* host pointers: upload (a shared array once), the solve, download S */
int xinv_fourier_standard_2d_f64_batched(double *S, const double *A, const double *C, const double *F, int64_t nbatch,
                                         const int64_t *strides, int64_t yc, int64_t xc, double delxSqr, double ratioSqr,
                                         double undef, double *flags, const xinv_options *opt);

/* device pointers; the transform is queued on `stream` */
int xinv_rowdft_f64_dev(double *out, const double *in, int64_t nrows, int64_t n, int inverse, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* XINV_FOURIER_H */
