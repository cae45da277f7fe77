/*
 * xinv_fourier.h -- the direct Fourier solve of the 2-D standard form for periodic x, and the row transform under it.
 * Included by xinv.h, which describes the arguments ("fourier"); it may also be included after xinv.h alone
 * (xinv_options is declared there).  Implemented in xinvert_amd/csrc/xinv_hip.hip over the kernels k_rowdft,
 * k_fourier_tri and k_fourier_check (xinv_fourier.h of csrc); the plans add k_fourier_factor and k_fourier_subst.
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

/* The 2-D GENERAL form, B == 0 (xinv.h, "fourier": the general form): one complex tridiagonal system per wavenumber
 * (k_fourier_gcheck, k_fourier_cfactor, k_fourier_csubst of csrc/xinv_cfourier.h around k_rowdft).  A, C, D, E, F: one
 * value per row; strides[7]: of S, A, C, D, E, F, G between two members, 0 = shared (not S), else >= yc (S, G: yc * xc).
 * The contract of the standard-form pair: flags = [overflow, 0, 0] per member, rows 0 and yc-1 of S are not written, a
 * member that holds `undef` at a point that is read makes the call return XINV_ERR_ARG with every S untouched. */
int xinv_fourier_general_2d_f64_dev(double *S, const double *A, const double *C, const double *D, const double *E,
                                    const double *F, const double *G, int64_t nbatch, const int64_t *strides, int64_t yc,
                                    int64_t xc, double delx, double delxSqr, double ratio, double ratioSqr, double undef,
                                    double *flags, void *stream);

int xinv_fourier_general_2d_f64_batched(double *S, const double *A, const double *C, const double *D, const double *E,
                                        const double *F, const double *G, int64_t nbatch, const int64_t *strides,
                                        int64_t yc, int64_t xc, double delx, double delxSqr, double ratio, double ratioSqr,
                                        double undef, double *flags, const xinv_options *opt);

/* device pointers; the transform is queued on `stream` */
int xinv_rowdft_f64_dev(double *out, const double *in, int64_t nrows, int64_t n, int inverse, void *stream);

/* Plans: one operator, many forcings.  Device pointers, the current device.  create factors the per-wavenumber systems once
 * and returns with the plan ready; a solve only queues on `stream`; status waits for the plan's last solve.  UNLIKE the
 * one-shot entry, a member that holds `undef` at a point the solve reads keeps its S while the other members ARE solved;
 * status names the first such member (XINV_ERR_ARG) after filling flags and bad. */
typedef struct xinv_fourier_plan xinv_fourier_plan;

/* strides[2]: of A and C between two members, 0 = shared, else >= yc */
int xinv_fourier_plan_create_standard_2d_f64_dev(xinv_fourier_plan **plan, const double *A, const double *C, int64_t nbatch,
                                                 const int64_t *strides, int64_t yc, int64_t xc, double delxSqr,
                                                 double ratioSqr, double undef, void *stream);

/* sS, sF: member strides of S and F in elements; sF = 0: one forcing for all members */
int xinv_fourier_plan_solve_f64_dev(xinv_fourier_plan *plan, double *S, const double *F, int64_t sS, int64_t sF, void *stream);

/* flags: host double[nbatch][3] = {overflow, 0, 0}; bad: host int[nbatch] (undef counts) or NULL */
int xinv_fourier_plan_status(xinv_fourier_plan *plan, double *flags, int *bad);

/* waits for the plan's last solve, frees everything the plan owns; NULL is accepted */
int xinv_fourier_plan_destroy(xinv_fourier_plan *plan);

#ifdef __cplusplus
}
#endif

#endif /* XINV_FOURIER_H */
