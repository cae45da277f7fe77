/*
 * xinv_resid.h -- the residual R = L(S) - F of the five second-order operator forms of libxinv_hip.so, with its norms.
 * Included by xinv.h, which describes the arguments ("residual"); it may also be included after xinv.h alone
 * (xinv_options is declared there).  Implemented in xinvert_amd/csrc/xinv_hip.hip over the kernels k_resid2d / k_resid3d
 * (xinv_resid.h of csrc).  One pair per form, in the order of the forms' table: device pointers (queued on `stream`),
 * then host pointers.
 */
#ifndef XINV_RESID_H
#define XINV_RESID_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int xinv_residual_standard_2d_f64_dev(double *R, const double *S, const double *A, const double *B, const double *C,
                                      const double *F, int64_t nbatch, const int64_t *strides, int64_t yc, int64_t xc,
                                      double dely, double delx, int BCy, int BCx, double delxSqr, double ratioQtr,
                                      double ratioSqr, double optArg, double undef, double *norms, void *stream);

int xinv_residual_standard_2d_f64_batched(double *R, const double *S, const double *A, const double *B,
                                          const double *C, const double *F, int64_t nbatch, const int64_t *strides,
                                          int64_t yc, int64_t xc, double dely, double delx, int BCy, int BCx,
                                          double delxSqr, double ratioQtr, double ratioSqr, double optArg,
                                          double undef, double *norms, const xinv_options *opt);

int xinv_residual_general_2d_f64_dev(double *R, const double *S, const double *A, const double *B, const double *C,
                                     const double *D, const double *E, const double *F, const double *G,
                                     int64_t nbatch, const int64_t *strides, int64_t yc, int64_t xc, double dely,
                                     double delx, int BCy, int BCx, double delxSqr, double ratio, double ratioQtr,
                                     double ratioSqr, double optArg, double undef, double *norms, void *stream);

int xinv_residual_general_2d_f64_batched(double *R, const double *S, const double *A, const double *B,
                                         const double *C, const double *D, const double *E, const double *F,
                                         const double *G, int64_t nbatch, const int64_t *strides, int64_t yc,
                                         int64_t xc, double dely, double delx, int BCy, int BCx, double delxSqr,
                                         double ratio, double ratioQtr, double ratioSqr, double optArg, double undef,
                                         double *norms, const xinv_options *opt);

int xinv_residual_standard_2d_test_f64_dev(double *R, const double *S, const double *A, const double *B,
                                           const double *C, const double *D, const double *E, const double *F,
                                           int64_t nbatch, const int64_t *strides, int64_t yc, int64_t xc,
                                           double dely, double delx, int BCy, int BCx, double delxSqr,
                                           double ratioQtr, double ratioSqr, double optArg, double undef,
                                           double *norms, void *stream);

int xinv_residual_standard_2d_test_f64_batched(double *R, const double *S, const double *A, const double *B,
                                               const double *C, const double *D, const double *E, const double *F,
                                               int64_t nbatch, const int64_t *strides, int64_t yc, int64_t xc,
                                               double dely, double delx, int BCy, int BCx, double delxSqr,
                                               double ratioQtr, double ratioSqr, double optArg, double undef,
                                               double *norms, const xinv_options *opt);

int xinv_residual_standard_3d_f64_dev(double *R, const double *S, const double *A, const double *B, const double *C,
                                      const double *F, int64_t nbatch, const int64_t *strides, int64_t zc, int64_t yc,
                                      int64_t xc, double delz, double dely, double delx, int BCz, int BCy, int BCx,
                                      double delxSqr, double ratio2Sqr, double ratio1Sqr, double optArg, double undef,
                                      double *norms, void *stream);

int xinv_residual_standard_3d_f64_batched(double *R, const double *S, const double *A, const double *B,
                                          const double *C, const double *F, int64_t nbatch, const int64_t *strides,
                                          int64_t zc, int64_t yc, int64_t xc, double delz, double dely, double delx,
                                          int BCz, int BCy, int BCx, double delxSqr, double ratio2Sqr,
                                          double ratio1Sqr, double optArg, double undef, double *norms,
                                          const xinv_options *opt);

int xinv_residual_general_3d_f64_dev(double *R, const double *S, const double *A, const double *B, const double *C,
                                     const double *D, const double *E, const double *F, const double *G,
                                     const double *H, int64_t nbatch, const int64_t *strides, int64_t zc, int64_t yc,
                                     int64_t xc, double delz, double dely, double delx, int BCz, int BCy, int BCx,
                                     double delxSqr, double ratio2, double ratio1, double ratio2Sqr, double ratio1Sqr,
                                     double optArg, double undef, double *norms, void *stream);

int xinv_residual_general_3d_f64_batched(double *R, const double *S, const double *A, const double *B,
                                         const double *C, const double *D, const double *E, const double *F,
                                         const double *G, const double *H, int64_t nbatch, const int64_t *strides,
                                         int64_t zc, int64_t yc, int64_t xc, double delz, double dely, double delx,
                                         int BCz, int BCy, int BCx, double delxSqr, double ratio2, double ratio1,
                                         double ratio2Sqr, double ratio1Sqr, double optArg, double undef,
                                         double *norms, const xinv_options *opt);

#ifdef __cplusplus
}
#endif

#endif /* XINV_RESID_H */
