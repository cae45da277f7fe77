// xinv_hip.hip -- host driver and C-ABI of the MI355X SOR inversion engine (include/xinv.h).
//
// Replaces the reference's numba kernels behind the call boundary of xinvert/core.py
// (core.py:60-69, 130-139, 419-428).  Built for gfx950 only:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared
//
// Control flow of one solve (all batch members together, one stream):
//   k_solve_init -> [ sweep launches ... ] x check_every -> async read-back of the per-member
//   control blocks -> repeat until every member has stopped.  The stopping rule runs on the
//   device after every sweep (reducing workgroup / k_norm_final); once a member is done
//   every later launch is a no-op for it, so S holds exactly the sweep the reference stops at.
//
// Threading: solves on one device are serialised by a per-device lock (they share the cached
// workspace); different devices may be driven concurrently from different host threads.
// Statistics and the last error text are thread-local.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <ctype.h>
#include <algorithm>
#include <exception>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <thread>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../../include/xinv.h"
#include "xinv_device.h"
#include "xinv_colour.h"
#define XINV_AUX_KERNELS            /* the detection / skip-norm helper kernels live in this unit */
#include "xinv_dispatch.h"          /* argument structs + launchers of the sweep kernels (xinv_tu_*.hip) */

#define XINV_VERSION 900
#define XINV_MEMBER_CHUNK 32768     /* members per launch: grid.y / grid.z are limited to 65535 */

// The shipped library reads NO environment variable: the planner's choices are overridden through xinv_options
// (lanes, norm_lag, pipe_fr, graph, sweeps_per_launch, flags).  The test-hooks build (build/libxinv_hooks.so) and A/B
// variant builds (-DXINV_EXPERIMENTS=1) additionally honour the XINV_* switches of rounds 2-4 where the option is 0.
#if XINV_TEST_HOOKS || XINV_EXPERIMENTS
#define XINV_ENV_INT(name, dflt) ([&] { const char *e_ = getenv(name); return e_ ? atoi(e_) : (dflt); }())
#else
#define XINV_ENV_INT(name, dflt) (dflt)
#endif

// The control-block mirror and the mailbox word the host SPINS on (k_ctl_mail) must be fine-grained, coherent host
// memory whatever HIP_HOST_COHERENT says: the device's stores of the blocks have to be visible before its store of the
// sequence word.
#define XINV_HOST_COHERENT (hipHostMallocCoherent | hipHostMallocMapped)
static inline void xinv_cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
}

#include "xinv_host.h"
#include "xinv_launch.h"

#include "xinv_plan.h"        /* planner */
#include "xinv_sweep.h"       /* sweep loop, finalise, device-pointer solve, resident plans */
#include "xinv_hostptr.h"     /* host-pointer pipeline, in-call multi-GPU split */
#include "xinv_std1d_host.h"   /* 1-D standard form: register-resident solve (k_std1d) */
#include "xinv_tridiag_host.h" /* trace / traceCyclic and the direct 1-D solve (k_tridiag) */
#include "xinv_fd_host.h"      /* finite-difference operators (k_fd) */
#include "xinv_mg.h"           /* multigrid grid transfers (k_mg_restrict, k_mg_prolong) */
#include "xinv_resid_host.h"   /* the residual L(S) - F of the second-order forms (k_resid2d, k_resid3d) */
#include "xinv_fourier_host.h" /* the direct Fourier solve of the 2-D standard form for periodic x (k_rowdft, k_fourier_tri) */
#include "xinv_cfourier_host.h" /* ... and of the 2-D general form (k_fourier_cfactor, k_fourier_csubst) */

// ------------------------------------------------------------------ C-ABI
extern "C" {

void xinv_default_options(xinv_options *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->device = -1;
    o->path = XINV_PATH_AUTO;
}

int xinv_last_stats(xinv_stats *out)
{
    if (!out) return XINV_ERR_ARG;
    *out = t_stats;
    return XINV_OK;
}

const char *xinv_last_error(void) { return t_err.c_str(); }

int xinv_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int xinv_version(void) { return XINV_VERSION; }
void xinv_abi_sizes(int32_t *options_bytes, int32_t *stats_bytes)
{
    if (options_bytes) *options_bytes = (int32_t)sizeof(xinv_options);
    if (stats_bytes) *stats_bytes = (int32_t)sizeof(xinv_stats);
}

#define GUARD(expr) try { return (expr); } catch (const std::exception &e) { t_err = e.what(); return XINV_ERR_HIP; } catch (...) { t_err = "unknown C++ exception"; return XINV_ERR_HIP; }

// ---- the operator forms: one problem builder, one way through an entry point ---------------------------------------
// `c`: the FORM[kind].ncoef coefficient arrays, the forcing last; `st`: batch strides of S and of every array (NULL: one
// slice); the 2-D forms pass zc = 1 and BCz = 0; `sc`: the fields of XinvScal the form's kernels read, the rest 0.
static Problem mk_problem(int kind, double *S, const double *const *c, int64_t nbatch, const int64_t *st, int64_t zc,
                          int64_t yc, int64_t xc, int BCz, int BCy, int BCx, const XinvScal &sc, int64_t mxLoop, double tol)
{
    Problem p;
    memset(&p, 0, sizeof p);
    p.kind = kind; p.nbatch = nbatch; p.zc = zc; p.yc = yc; p.xc = xc;
    p.S = S; p.ncoef = FORM[kind].ncoef;
    const int64_t n = zc * yc * xc;
    p.sS = st ? st[0] : n;
    for (int q = 0; q < p.ncoef; q++) { p.c[q] = c[q]; p.sc[q] = st ? st[1 + q] : n; }
    p.BCz = BCz; p.BCy = BCy; p.BCx = BCx;
    p.sc_ = sc;
    p.stop.mxLoop = mxLoop; p.stop.tolerance = tol; p.stop.stop_on_zero_norm = FORM[kind].stop_on_zero_norm;
    return p;
}

// What every entry point of a form does with its arguments.  RUN_SINGLE: one slice, no strides, default options;
// RUN_PLAN: `plan` instead of S, flags, mxLoop and tolerance (the callers pass nullptr, nullptr, 0, 0.0).
enum { RUN_SINGLE, RUN_BATCHED, RUN_DEV, RUN_PLAN };
static int run_form(int how, int kind, xinv_plan **plan, double *S, const double *const *c, int64_t nbatch,
                    const int64_t *strides, int64_t zc, int64_t yc, int64_t xc, int BCz, int BCy, int BCx,
                    const XinvScal &sc, double *flags, int64_t mxLoop, double tolerance, const xinv_options *opt,
                    void *stream)
{
    if (how != RUN_SINGLE && !strides) return fail_arg("null strides");
    if (opt && opt->path == XINV_PATH_DIRECT1D)
        return fail_arg("XINV_PATH_DIRECT1D: the direct solve exists for the 1-D standard form only");
    Problem p = mk_problem(kind, S, c, nbatch, strides, zc, yc, xc, BCz, BCy, BCx, sc, mxLoop, tolerance);
    GUARD(how == RUN_PLAN ? plan_create(plan, p, opt, (hipStream_t)stream)
          : how == RUN_DEV ? solve_dev(p, flags, opt, (hipStream_t)stream) : solve_host(p, flags, opt))
}

int xinv_standard_2d_f64(double *S, const double *A, const double *B, const double *C,
                         const double *F, int64_t yc, int64_t xc, double dely, double delx,
                         int BCy, int BCx, double delxSqr, double ratioQtr, double ratioSqr,
                         double optArg, double undef, double *flags, int64_t mxLoop,
                         double tolerance)
{
    (void)dely;
    const double *c[] = { A, B, C, F };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.optArg = optArg;
    sc.undef = undef;
    return run_form(RUN_SINGLE, KIND_STD2D, nullptr, S, c, 1, nullptr, 1, yc, xc, 0, BCy, BCx, sc, flags, mxLoop,
                    tolerance, nullptr, nullptr);
}

int xinv_general_2d_f64(double *S, const double *A, const double *B, const double *C,
                        const double *D, const double *E, const double *F, const double *G,
                        int64_t yc, int64_t xc, double dely, double delx, int BCy, int BCx,
                        double delxSqr, double ratio, double ratioQtr, double ratioSqr,
                        double optArg, double undef, double *flags, int64_t mxLoop,
                        double tolerance)
{
    (void)dely;
    const double *c[] = { A, B, C, D, E, F, G };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratio = ratio; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr;
    sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_SINGLE, KIND_GEN2D, nullptr, S, c, 1, nullptr, 1, yc, xc, 0, BCy, BCx, sc, flags, mxLoop,
                    tolerance, nullptr, nullptr);
}

int xinv_standard_3d_f64(double *S, const double *A, const double *B, const double *C,
                         const double *F, int64_t zc, int64_t yc, int64_t xc, double delz,
                         double dely, double delx, int BCz, int BCy, int BCx, double delxSqr,
                         double ratio2Sqr, double ratio1Sqr, double optArg, double undef,
                         double *flags, int64_t mxLoop, double tolerance)
{
    (void)delz; (void)dely; (void)delx;
    const double *c[] = { A, B, C, F };
    XinvScal sc = {};
    sc.delxSqr = delxSqr; sc.ratio2Sqr = ratio2Sqr; sc.ratio1Sqr = ratio1Sqr; sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_SINGLE, KIND_STD3D, nullptr, S, c, 1, nullptr, zc, yc, xc, BCz, BCy, BCx, sc, flags, mxLoop,
                    tolerance, nullptr, nullptr);
}

int xinv_standard_2d_f64_batched(double *S, const double *A, const double *B, const double *C,
                                 const double *F, int64_t nbatch, const int64_t *strides,
                                 int64_t yc, int64_t xc, double dely, double delx, int BCy,
                                 int BCx, double delxSqr, double ratioQtr, double ratioSqr,
                                 double optArg, double undef, double *flags, int64_t mxLoop,
                                 double tolerance, const xinv_options *opt)
{
    (void)dely;
    const double *c[] = { A, B, C, F };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.optArg = optArg;
    sc.undef = undef;
    return run_form(RUN_BATCHED, KIND_STD2D, nullptr, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc, flags,
                    mxLoop, tolerance, opt, nullptr);
}

int xinv_general_2d_f64_batched(double *S, const double *A, const double *B, const double *C,
                                const double *D, const double *E, const double *F,
                                const double *G, int64_t nbatch, const int64_t *strides,
                                int64_t yc, int64_t xc, double dely, double delx, int BCy,
                                int BCx, double delxSqr, double ratio, double ratioQtr,
                                double ratioSqr, double optArg, double undef, double *flags,
                                int64_t mxLoop, double tolerance, const xinv_options *opt)
{
    (void)dely;
    const double *c[] = { A, B, C, D, E, F, G };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratio = ratio; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr;
    sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_BATCHED, KIND_GEN2D, nullptr, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc, flags,
                    mxLoop, tolerance, opt, nullptr);
}

int xinv_standard_3d_f64_batched(double *S, const double *A, const double *B, const double *C,
                                 const double *F, int64_t nbatch, const int64_t *strides,
                                 int64_t zc, int64_t yc, int64_t xc, double delz, double dely,
                                 double delx, int BCz, int BCy, int BCx, double delxSqr,
                                 double ratio2Sqr, double ratio1Sqr, double optArg,
                                 double undef, double *flags, int64_t mxLoop, double tolerance,
                                 const xinv_options *opt)
{
    (void)delz; (void)dely; (void)delx;
    const double *c[] = { A, B, C, F };
    XinvScal sc = {};
    sc.delxSqr = delxSqr; sc.ratio2Sqr = ratio2Sqr; sc.ratio1Sqr = ratio1Sqr; sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_BATCHED, KIND_STD3D, nullptr, S, c, nbatch, strides, zc, yc, xc, BCz, BCy, BCx, sc, flags,
                    mxLoop, tolerance, opt, nullptr);
}

int xinv_standard_2d_f64_dev(double *S, const double *A, const double *B, const double *C,
                             const double *F, int64_t nbatch, const int64_t *strides,
                             int64_t yc, int64_t xc, double dely, double delx, int BCy,
                             int BCx, double delxSqr, double ratioQtr, double ratioSqr,
                             double optArg, double undef, double *flags, int64_t mxLoop,
                             double tolerance, const xinv_options *opt, void *stream)
{
    (void)dely;
    const double *c[] = { A, B, C, F };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.optArg = optArg;
    sc.undef = undef;
    return run_form(RUN_DEV, KIND_STD2D, nullptr, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc, flags, mxLoop,
                    tolerance, opt, stream);
}

int xinv_general_2d_f64_dev(double *S, const double *A, const double *B, const double *C,
                            const double *D, const double *E, const double *F, const double *G,
                            int64_t nbatch, const int64_t *strides, int64_t yc, int64_t xc,
                            double dely, double delx, int BCy, int BCx, double delxSqr,
                            double ratio, double ratioQtr, double ratioSqr, double optArg,
                            double undef, double *flags, int64_t mxLoop, double tolerance,
                            const xinv_options *opt, void *stream)
{
    (void)dely;
    const double *c[] = { A, B, C, D, E, F, G };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratio = ratio; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr;
    sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_DEV, KIND_GEN2D, nullptr, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc, flags, mxLoop,
                    tolerance, opt, stream);
}

int xinv_standard_3d_f64_dev(double *S, const double *A, const double *B, const double *C,
                             const double *F, int64_t nbatch, const int64_t *strides,
                             int64_t zc, int64_t yc, int64_t xc, double delz, double dely,
                             double delx, int BCz, int BCy, int BCx, double delxSqr,
                             double ratio2Sqr, double ratio1Sqr, double optArg, double undef,
                             double *flags, int64_t mxLoop, double tolerance,
                             const xinv_options *opt, void *stream)
{
    (void)delz; (void)dely; (void)delx;
    const double *c[] = { A, B, C, F };
    XinvScal sc = {};
    sc.delxSqr = delxSqr; sc.ratio2Sqr = ratio2Sqr; sc.ratio1Sqr = ratio1Sqr; sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_DEV, KIND_STD3D, nullptr, S, c, nbatch, strides, zc, yc, xc, BCz, BCy, BCx, sc, flags,
                    mxLoop, tolerance, opt, stream);
}

int xinv_general_3d_f64(double *S, const double *A, const double *B, const double *C,
                        const double *D, const double *E, const double *F, const double *G,
                        const double *H, int64_t zc, int64_t yc, int64_t xc, double delz,
                        double dely, double delx, int BCz, int BCy, int BCx, double delxSqr,
                        double ratio2, double ratio1, double ratio2Sqr, double ratio1Sqr,
                        double optArg, double undef, double *flags, int64_t mxLoop,
                        double tolerance)
{
    (void)delz; (void)dely;
    const double *c[] = { A, B, C, D, E, F, G, H };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratio2 = ratio2; sc.ratio1 = ratio1; sc.ratio2Sqr = ratio2Sqr;
    sc.ratio1Sqr = ratio1Sqr; sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_SINGLE, KIND_GEN3D, nullptr, S, c, 1, nullptr, zc, yc, xc, BCz, BCy, BCx, sc, flags, mxLoop,
                    tolerance, nullptr, nullptr);
}

int xinv_general_3d_f64_batched(double *S, const double *A, const double *B, const double *C,
                                const double *D, const double *E, const double *F,
                                const double *G, const double *H, int64_t nbatch,
                                const int64_t *strides, int64_t zc, int64_t yc, int64_t xc,
                                double delz, double dely, double delx, int BCz, int BCy, int BCx,
                                double delxSqr, double ratio2, double ratio1, double ratio2Sqr,
                                double ratio1Sqr, double optArg, double undef, double *flags,
                                int64_t mxLoop, double tolerance, const xinv_options *opt)
{
    (void)delz; (void)dely;
    const double *c[] = { A, B, C, D, E, F, G, H };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratio2 = ratio2; sc.ratio1 = ratio1; sc.ratio2Sqr = ratio2Sqr;
    sc.ratio1Sqr = ratio1Sqr; sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_BATCHED, KIND_GEN3D, nullptr, S, c, nbatch, strides, zc, yc, xc, BCz, BCy, BCx, sc, flags,
                    mxLoop, tolerance, opt, nullptr);
}

int xinv_general_3d_f64_dev(double *S, const double *A, const double *B, const double *C,
                            const double *D, const double *E, const double *F, const double *G,
                            const double *H, int64_t nbatch, const int64_t *strides, int64_t zc,
                            int64_t yc, int64_t xc, double delz, double dely, double delx, int BCz,
                            int BCy, int BCx, double delxSqr, double ratio2, double ratio1,
                            double ratio2Sqr, double ratio1Sqr, double optArg, double undef,
                            double *flags, int64_t mxLoop, double tolerance,
                            const xinv_options *opt, void *stream)
{
    (void)delz; (void)dely;
    const double *c[] = { A, B, C, D, E, F, G, H };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratio2 = ratio2; sc.ratio1 = ratio1; sc.ratio2Sqr = ratio2Sqr;
    sc.ratio1Sqr = ratio1Sqr; sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_DEV, KIND_GEN3D, nullptr, S, c, nbatch, strides, zc, yc, xc, BCz, BCy, BCx, sc, flags,
                    mxLoop, tolerance, opt, stream);
}

int xinv_general_bih_2d_f64(double *S, const double *A, const double *B, const double *C,
                            const double *D, const double *E, const double *F, const double *G,
                            const double *H, const double *I, const double *J, int64_t yc,
                            int64_t xc, double dely, double delx, int BCy, int BCx,
                            double delxSSr, double delxTr, double delxSqr, double ratio,
                            double ratioSSr, double ratioQtr, double ratioSqr, double optArg,
                            double undef, double *flags, int64_t mxLoop, double tolerance)
{
    (void)dely; (void)delx;
    const double *c[] = { A, B, C, D, E, F, G, H, I, J };
    XinvScal sc = {};
    sc.delxSSr = delxSSr; sc.delxTr = delxTr; sc.delxSqr = delxSqr; sc.ratio = ratio; sc.ratioSSr = ratioSSr;
    sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_SINGLE, KIND_BIH2D, nullptr, S, c, 1, nullptr, 1, yc, xc, 0, BCy, BCx, sc, flags, mxLoop,
                    tolerance, nullptr, nullptr);
}

int xinv_general_bih_2d_f64_batched(double *S, const double *A, const double *B, const double *C,
                                    const double *D, const double *E, const double *F,
                                    const double *G, const double *H, const double *I,
                                    const double *J, int64_t nbatch, const int64_t *strides,
                                    int64_t yc, int64_t xc, double dely, double delx, int BCy,
                                    int BCx, double delxSSr, double delxTr, double delxSqr,
                                    double ratio, double ratioSSr, double ratioQtr,
                                    double ratioSqr, double optArg, double undef, double *flags,
                                    int64_t mxLoop, double tolerance, const xinv_options *opt)
{
    (void)dely; (void)delx;
    const double *c[] = { A, B, C, D, E, F, G, H, I, J };
    XinvScal sc = {};
    sc.delxSSr = delxSSr; sc.delxTr = delxTr; sc.delxSqr = delxSqr; sc.ratio = ratio; sc.ratioSSr = ratioSSr;
    sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_BATCHED, KIND_BIH2D, nullptr, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc, flags,
                    mxLoop, tolerance, opt, nullptr);
}

int xinv_general_bih_2d_f64_dev(double *S, const double *A, const double *B, const double *C,
                                const double *D, const double *E, const double *F,
                                const double *G, const double *H, const double *I,
                                const double *J, int64_t nbatch, const int64_t *strides,
                                int64_t yc, int64_t xc, double dely, double delx, int BCy,
                                int BCx, double delxSSr, double delxTr, double delxSqr,
                                double ratio, double ratioSSr, double ratioQtr, double ratioSqr,
                                double optArg, double undef, double *flags, int64_t mxLoop,
                                double tolerance, const xinv_options *opt, void *stream)
{
    (void)dely; (void)delx;
    const double *c[] = { A, B, C, D, E, F, G, H, I, J };
    XinvScal sc = {};
    sc.delxSSr = delxSSr; sc.delxTr = delxTr; sc.delxSqr = delxSqr; sc.ratio = ratio; sc.ratioSSr = ratioSSr;
    sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_DEV, KIND_BIH2D, nullptr, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc, flags, mxLoop,
                    tolerance, opt, stream);
}

int xinv_standard_2d_test_f64(double *S, const double *A, const double *B, const double *C,
                              const double *D, const double *E, const double *F, int64_t yc,
                              int64_t xc, double dely, double delx, int BCy, int BCx,
                              double delxSqr, double ratioQtr, double ratioSqr, double optArg,
                              double undef, double *flags, int64_t mxLoop, double tolerance)
{
    (void)dely;
    const double *c[] = { A, B, C, D, E, F };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.optArg = optArg;
    sc.undef = undef;
    return run_form(RUN_SINGLE, KIND_STD2DT, nullptr, S, c, 1, nullptr, 1, yc, xc, 0, BCy, BCx, sc, flags, mxLoop,
                    tolerance, nullptr, nullptr);
}

int xinv_standard_2d_test_f64_batched(double *S, const double *A, const double *B, const double *C,
                                      const double *D, const double *E, const double *F,
                                      int64_t nbatch, const int64_t *strides, int64_t yc,
                                      int64_t xc, double dely, double delx, int BCy, int BCx,
                                      double delxSqr, double ratioQtr, double ratioSqr,
                                      double optArg, double undef, double *flags, int64_t mxLoop,
                                      double tolerance, const xinv_options *opt)
{
    (void)dely;
    const double *c[] = { A, B, C, D, E, F };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.optArg = optArg;
    sc.undef = undef;
    return run_form(RUN_BATCHED, KIND_STD2DT, nullptr, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc, flags,
                    mxLoop, tolerance, opt, nullptr);
}

int xinv_standard_2d_test_f64_dev(double *S, const double *A, const double *B, const double *C,
                                  const double *D, const double *E, const double *F,
                                  int64_t nbatch, const int64_t *strides, int64_t yc, int64_t xc,
                                  double dely, double delx, int BCy, int BCx, double delxSqr,
                                  double ratioQtr, double ratioSqr, double optArg, double undef,
                                  double *flags, int64_t mxLoop, double tolerance,
                                  const xinv_options *opt, void *stream)
{
    (void)dely;
    const double *c[] = { A, B, C, D, E, F };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.optArg = optArg;
    sc.undef = undef;
    return run_form(RUN_DEV, KIND_STD2DT, nullptr, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc, flags, mxLoop,
                    tolerance, opt, stream);
}

// ---- standard 1-D form (k_std1d) --------------------------------------------------------------------------------
static Std1dProblem mk_std1d(double *S, const double *A, const double *B, const double *F, int64_t nbatch,
                             const int64_t *st, int64_t xc, int BCx, double delxSqr, double optArg, double undef,
                             int64_t mxLoop, double tol)
{
    Std1dProblem p;
    memset(&p, 0, sizeof p);
    p.S = S; p.A = A; p.B = B; p.F = F; p.nbatch = nbatch; p.xc = xc;
    p.sS = st ? st[0] : xc; p.sA = st ? st[1] : xc; p.sB = st ? st[2] : xc; p.sF = st ? st[3] : xc;
    p.BCx = BCx; p.delxSqr = delxSqr; p.optArg = optArg; p.undef = undef;
    p.mxLoop = mxLoop; p.tolerance = tol;
    return p;
}

int xinv_standard_1d_f64(double *S, const double *A, const double *B, const double *F, int64_t xc, double delx,
                         int BCx, double delxSqr, double optArg, double undef, double *flags, int64_t mxLoop,
                         double tolerance, const xinv_options *opt)
{
    (void)delx;
    Std1dProblem p = mk_std1d(S, A, B, F, 1, nullptr, xc, BCx, delxSqr, optArg, undef, mxLoop, tolerance);
    GUARD(std1d_solve_host(p, flags, opt))
}

int xinv_standard_1d_f64_batched(double *S, const double *A, const double *B, const double *F, int64_t nbatch,
                                 const int64_t *strides, int64_t xc, double delx, int BCx, double delxSqr,
                                 double optArg, double undef, double *flags, int64_t mxLoop, double tolerance,
                                 const xinv_options *opt)
{
    (void)delx;
    if (!strides) return fail_arg("null strides");
    Std1dProblem p = mk_std1d(S, A, B, F, nbatch, strides, xc, BCx, delxSqr, optArg, undef, mxLoop, tolerance);
    GUARD(std1d_solve_host(p, flags, opt))
}

int xinv_standard_1d_f64_dev(double *S, const double *A, const double *B, const double *F, int64_t nbatch,
                             const int64_t *strides, int64_t xc, double delx, int BCx, double delxSqr,
                             double optArg, double undef, double *flags, int64_t mxLoop, double tolerance,
                             const xinv_options *opt, void *stream)
{
    (void)delx;
    if (!strides) return fail_arg("null strides");
    Std1dProblem p = mk_std1d(S, A, B, F, nbatch, strides, xc, BCx, delxSqr, optArg, undef, mxLoop, tolerance);
    GUARD(std1d_solve_dev(p, flags, opt, (hipStream_t)stream))
}

// ---- tridiagonal systems (k_tridiag: numbas.trace / traceCyclic) --------------------------------------------------
static TridiagCall mk_tridiag(double *x, const double *a, const double *b, const double *c, const double *d,
                              const double *a0, const double *cn, int64_t nbatch, const int64_t *strides, int64_t n)
{
    TridiagCall t;
    memset(&t, 0, sizeof t);
    t.x = x; t.a = a; t.b = b; t.c = c; t.d = d; t.a0 = a0; t.cn = cn; t.nbatch = nbatch; t.n = n;
    if (strides)
        for (int q = 0; q < (a0 && cn ? 7 : 5); q++) t.s[q] = strides[q];
    return t;
}

int xinv_tridiag_f64(double *x, const double *a, const double *b, const double *c, const double *d, const double *a0,
                     const double *cn, int64_t nbatch, const int64_t *strides, int64_t n)
{
    GUARD(tridiag_solve_host(mk_tridiag(x, a, b, c, d, a0, cn, nbatch, strides, n), strides))
}

int xinv_tridiag_f64_dev(double *x, const double *a, const double *b, const double *c, const double *d, const double *a0,
                         const double *cn, int64_t nbatch, const int64_t *strides, int64_t n, void *stream)
{
    GUARD(tridiag_solve_dev(mk_tridiag(x, a, b, c, d, a0, cn, nbatch, strides, n), strides, (hipStream_t)stream))
}

// ---- the direct Fourier solve of the 2-D standard and general forms for periodic x (include/xinv_fourier.h) --------
// `coef`, `letters`, `letters_and`: the form's per-row coefficient arrays in the ABI's order and how the messages name them
static FourierCall mk_fourier(double *S, std::initializer_list<const double *> coef, const double *F, const char *letters,
                              const char *letters_and, int64_t nbatch, const int64_t *strides, int64_t yc, int64_t xc,
                              double delx, double delxSqr, double ratio, double ratioSqr, double undef)
{
    FourierCall c;
    memset(&c, 0, sizeof c);
    c.a[c.na++] = { S, yc * xc, 0 };
    for (const double *p : coef) c.a[c.na++] = { const_cast<double *>(p), yc, 0 };
    c.a[c.na++] = { const_cast<double *>(F), yc * xc, 0 };
    if (strides)
        for (int q = 0; q < c.na; q++) c.a[q].stride = strides[q];
    c.letters = letters; c.letters_and = letters_and;
    c.nbatch = nbatch; c.yc = yc; c.xc = xc;
    c.delx = delx; c.delxSqr = delxSqr; c.ratio = ratio; c.ratioSqr = ratioSqr; c.undef = undef;
    return c;
}

static FourierCall mk_fourier_std(double *S, const double *A, const double *C, const double *F, int64_t nbatch,
                                  const int64_t *strides, int64_t yc, int64_t xc, double delxSqr, double ratioSqr, double undef)
{
    return mk_fourier(S, { A, C }, F, "A, C", "A and C", nbatch, strides, yc, xc, 0.0, delxSqr, 0.0, ratioSqr, undef);
}

static FourierCall mk_fourier_gen(double *S, const double *A, const double *C, const double *D, const double *E, const double *F,
                                  const double *G, int64_t nbatch, const int64_t *strides, int64_t yc, int64_t xc, double delx,
                                  double delxSqr, double ratio, double ratioSqr, double undef)
{
    return mk_fourier(S, { A, C, D, E, F }, G, "A, C, D, E, F", "A, C, D, E and F", nbatch, strides, yc, xc, delx, delxSqr, ratio,
                      ratioSqr, undef);
}

int xinv_fourier_standard_2d_f64_dev(double *S, const double *A, const double *C, const double *F, int64_t nbatch,
                                     const int64_t *strides, int64_t yc, int64_t xc, double delxSqr, double ratioSqr,
                                     double undef, double *flags, void *stream)
{
    GUARD(fourier_dev(mk_fourier_std(S, A, C, F, nbatch, strides, yc, xc, delxSqr, ratioSqr, undef), strides, flags,
                      fourier_run_dev, (hipStream_t)stream))
}

int xinv_fourier_standard_2d_f64_batched(double *S, const double *A, const double *C, const double *F, int64_t nbatch,
                                         const int64_t *strides, int64_t yc, int64_t xc, double delxSqr, double ratioSqr,
                                         double undef, double *flags, const xinv_options *opt)
{
    GUARD(fourier_host(mk_fourier_std(S, A, C, F, nbatch, strides, yc, xc, delxSqr, ratioSqr, undef), strides, flags,
                       fourier_run_dev, opt))
}

int xinv_fourier_general_2d_f64_dev(double *S, const double *A, const double *C, const double *D, const double *E,
                                    const double *F, const double *G, int64_t nbatch, const int64_t *strides, int64_t yc,
                                    int64_t xc, double delx, double delxSqr, double ratio, double ratioSqr, double undef,
                                    double *flags, void *stream)
{
    GUARD(fourier_dev(mk_fourier_gen(S, A, C, D, E, F, G, nbatch, strides, yc, xc, delx, delxSqr, ratio, ratioSqr, undef), strides,
                      flags, cfourier_run_dev, (hipStream_t)stream))
}

int xinv_fourier_general_2d_f64_batched(double *S, const double *A, const double *C, const double *D, const double *E,
                                        const double *F, const double *G, int64_t nbatch, const int64_t *strides,
                                        int64_t yc, int64_t xc, double delx, double delxSqr, double ratio, double ratioSqr,
                                        double undef, double *flags, const xinv_options *opt)
{
    GUARD(fourier_host(mk_fourier_gen(S, A, C, D, E, F, G, nbatch, strides, yc, xc, delx, delxSqr, ratio, ratioSqr, undef), strides,
                       flags, cfourier_run_dev, opt))
}

int xinv_rowdft_f64_dev(double *out, const double *in, int64_t nrows, int64_t n, int inverse, void *stream)
{
    GUARD(rowdft_dev(out, in, nrows, n, inverse, (hipStream_t)stream))
}

// ... and its plans: the per-wavenumber factors once, a solve per forcing (fplan_* of xinv_fourier_host.h)
int xinv_fourier_plan_create_standard_2d_f64_dev(xinv_fourier_plan **plan, const double *A, const double *C, int64_t nbatch,
                                                 const int64_t *strides, int64_t yc, int64_t xc, double delxSqr,
                                                 double ratioSqr, double undef, void *stream)
{
    GUARD(fplan_create(plan, A, C, nbatch, strides, yc, xc, delxSqr, ratioSqr, undef, (hipStream_t)stream))
}

int xinv_fourier_plan_solve_f64_dev(xinv_fourier_plan *plan, double *S, const double *F, int64_t sS, int64_t sF, void *stream)
{
    GUARD(fplan_solve(plan, S, F, sS, sF, (hipStream_t)stream))
}

int xinv_fourier_plan_status(xinv_fourier_plan *plan, double *flags, int *bad)
{
    GUARD(fplan_status(plan, flags, bad))
}

int xinv_fourier_plan_destroy(xinv_fourier_plan *plan)
{
    GUARD(fplan_destroy(plan))
}

// ---- the residual L(S) - F of the five second-order forms (k_resid2d / k_resid3d; include/xinv_resid.h) ------------
// The solve entries' arrays and scalars behind R and S; optArg is accepted and ignored.
int xinv_residual_standard_2d_f64_dev(double *R, const double *S, const double *A, const double *B, const double *C,
                                      const double *F, int64_t nbatch, const int64_t *strides, int64_t yc, int64_t xc,
                                      double dely, double delx, int BCy, int BCx, double delxSqr, double ratioQtr,
                                      double ratioSqr, double optArg, double undef, double *norms, void *stream)
{
    (void)dely; (void)optArg;
    const double *c[] = { A, B, C, F };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.undef = undef;
    const ResidCall rc_ = mk_resid(KIND_STD2D, R, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc);
    GUARD(resid_dev(rc_, strides, norms, (hipStream_t)stream))
}

int xinv_residual_standard_2d_f64_batched(double *R, const double *S, const double *A, const double *B,
                                          const double *C, const double *F, int64_t nbatch, const int64_t *strides,
                                          int64_t yc, int64_t xc, double dely, double delx, int BCy, int BCx,
                                          double delxSqr, double ratioQtr, double ratioSqr, double optArg,
                                          double undef, double *norms, const xinv_options *opt)
{
    (void)dely; (void)optArg;
    const double *c[] = { A, B, C, F };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.undef = undef;
    const ResidCall rc_ = mk_resid(KIND_STD2D, R, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc);
    GUARD(resid_host(rc_, strides, norms, opt))
}

int xinv_residual_general_2d_f64_dev(double *R, const double *S, const double *A, const double *B, const double *C,
                                     const double *D, const double *E, const double *F, const double *G,
                                     int64_t nbatch, const int64_t *strides, int64_t yc, int64_t xc, double dely,
                                     double delx, int BCy, int BCx, double delxSqr, double ratio, double ratioQtr,
                                     double ratioSqr, double optArg, double undef, double *norms, void *stream)
{
    (void)dely; (void)optArg;
    const double *c[] = { A, B, C, D, E, F, G };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratio = ratio; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.undef = undef;
    const ResidCall rc_ = mk_resid(KIND_GEN2D, R, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc);
    GUARD(resid_dev(rc_, strides, norms, (hipStream_t)stream))
}

int xinv_residual_general_2d_f64_batched(double *R, const double *S, const double *A, const double *B,
                                         const double *C, const double *D, const double *E, const double *F,
                                         const double *G, int64_t nbatch, const int64_t *strides, int64_t yc,
                                         int64_t xc, double dely, double delx, int BCy, int BCx, double delxSqr,
                                         double ratio, double ratioQtr, double ratioSqr, double optArg, double undef,
                                         double *norms, const xinv_options *opt)
{
    (void)dely; (void)optArg;
    const double *c[] = { A, B, C, D, E, F, G };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratio = ratio; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.undef = undef;
    const ResidCall rc_ = mk_resid(KIND_GEN2D, R, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc);
    GUARD(resid_host(rc_, strides, norms, opt))
}

int xinv_residual_standard_2d_test_f64_dev(double *R, const double *S, const double *A, const double *B,
                                           const double *C, const double *D, const double *E, const double *F,
                                           int64_t nbatch, const int64_t *strides, int64_t yc, int64_t xc,
                                           double dely, double delx, int BCy, int BCx, double delxSqr,
                                           double ratioQtr, double ratioSqr, double optArg, double undef,
                                           double *norms, void *stream)
{
    (void)dely; (void)optArg;
    const double *c[] = { A, B, C, D, E, F };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.undef = undef;
    const ResidCall rc_ = mk_resid(KIND_STD2DT, R, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc);
    GUARD(resid_dev(rc_, strides, norms, (hipStream_t)stream))
}

int xinv_residual_standard_2d_test_f64_batched(double *R, const double *S, const double *A, const double *B,
                                               const double *C, const double *D, const double *E, const double *F,
                                               int64_t nbatch, const int64_t *strides, int64_t yc, int64_t xc,
                                               double dely, double delx, int BCy, int BCx, double delxSqr,
                                               double ratioQtr, double ratioSqr, double optArg, double undef,
                                               double *norms, const xinv_options *opt)
{
    (void)dely; (void)optArg;
    const double *c[] = { A, B, C, D, E, F };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.undef = undef;
    const ResidCall rc_ = mk_resid(KIND_STD2DT, R, S, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc);
    GUARD(resid_host(rc_, strides, norms, opt))
}

int xinv_residual_standard_3d_f64_dev(double *R, const double *S, const double *A, const double *B, const double *C,
                                      const double *F, int64_t nbatch, const int64_t *strides, int64_t zc, int64_t yc,
                                      int64_t xc, double delz, double dely, double delx, int BCz, int BCy, int BCx,
                                      double delxSqr, double ratio2Sqr, double ratio1Sqr, double optArg, double undef,
                                      double *norms, void *stream)
{
    (void)delz; (void)dely; (void)delx; (void)optArg;
    const double *c[] = { A, B, C, F };
    XinvScal sc = {};
    sc.delxSqr = delxSqr; sc.ratio2Sqr = ratio2Sqr; sc.ratio1Sqr = ratio1Sqr; sc.undef = undef;
    const ResidCall rc_ = mk_resid(KIND_STD3D, R, S, c, nbatch, strides, zc, yc, xc, BCz, BCy, BCx, sc);
    GUARD(resid_dev(rc_, strides, norms, (hipStream_t)stream))
}

int xinv_residual_standard_3d_f64_batched(double *R, const double *S, const double *A, const double *B,
                                          const double *C, const double *F, int64_t nbatch, const int64_t *strides,
                                          int64_t zc, int64_t yc, int64_t xc, double delz, double dely, double delx,
                                          int BCz, int BCy, int BCx, double delxSqr, double ratio2Sqr,
                                          double ratio1Sqr, double optArg, double undef, double *norms,
                                          const xinv_options *opt)
{
    (void)delz; (void)dely; (void)delx; (void)optArg;
    const double *c[] = { A, B, C, F };
    XinvScal sc = {};
    sc.delxSqr = delxSqr; sc.ratio2Sqr = ratio2Sqr; sc.ratio1Sqr = ratio1Sqr; sc.undef = undef;
    const ResidCall rc_ = mk_resid(KIND_STD3D, R, S, c, nbatch, strides, zc, yc, xc, BCz, BCy, BCx, sc);
    GUARD(resid_host(rc_, strides, norms, opt))
}

int xinv_residual_general_3d_f64_dev(double *R, const double *S, const double *A, const double *B, const double *C,
                                     const double *D, const double *E, const double *F, const double *G,
                                     const double *H, int64_t nbatch, const int64_t *strides, int64_t zc, int64_t yc,
                                     int64_t xc, double delz, double dely, double delx, int BCz, int BCy, int BCx,
                                     double delxSqr, double ratio2, double ratio1, double ratio2Sqr, double ratio1Sqr,
                                     double optArg, double undef, double *norms, void *stream)
{
    (void)delz; (void)dely; (void)optArg;
    const double *c[] = { A, B, C, D, E, F, G, H };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratio2 = ratio2; sc.ratio1 = ratio1; sc.ratio2Sqr = ratio2Sqr; sc.ratio1Sqr = ratio1Sqr; sc.undef = undef;
    const ResidCall rc_ = mk_resid(KIND_GEN3D, R, S, c, nbatch, strides, zc, yc, xc, BCz, BCy, BCx, sc);
    GUARD(resid_dev(rc_, strides, norms, (hipStream_t)stream))
}

int xinv_residual_general_3d_f64_batched(double *R, const double *S, const double *A, const double *B,
                                         const double *C, const double *D, const double *E, const double *F,
                                         const double *G, const double *H, int64_t nbatch, const int64_t *strides,
                                         int64_t zc, int64_t yc, int64_t xc, double delz, double dely, double delx,
                                         int BCz, int BCy, int BCx, double delxSqr, double ratio2, double ratio1,
                                         double ratio2Sqr, double ratio1Sqr, double optArg, double undef,
                                         double *norms, const xinv_options *opt)
{
    (void)delz; (void)dely; (void)optArg;
    const double *c[] = { A, B, C, D, E, F, G, H };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratio2 = ratio2; sc.ratio1 = ratio1; sc.ratio2Sqr = ratio2Sqr; sc.ratio1Sqr = ratio1Sqr; sc.undef = undef;
    const ResidCall rc_ = mk_resid(KIND_GEN3D, R, S, c, nbatch, strides, zc, yc, xc, BCz, BCy, BCx, sc);
    GUARD(resid_host(rc_, strides, norms, opt))
}

// ---- finite differences (k_fd) ----------------------------------------------------------------------------------
static FdCall mk_fd(const double *const *in, int nin, double *const *out, int nout, int ndim, const int64_t *shape,
                    int mode, int nterms, const int64_t *iterm, const double *dterm, const double *tab, int64_t ntab,
                    int mask_axis, int64_t mask_off)
{
    FdCall c;
    c.in = in; c.nin = nin; c.out = out; c.nout = nout; c.ndim = ndim; c.shape = shape;
    c.mode = mode; c.nterms = nterms; c.iterm = iterm; c.dterm = dterm; c.tab = tab; c.ntab = ntab;
    c.mask_axis = mask_axis; c.mask_off = mask_off;
    return c;
}

int xinv_fd_f64(const double *const *in, int nin, double *const *out, int nout, int ndim, const int64_t *shape,
                int mode, int nterms, const int64_t *iterm, const double *dterm, const double *tab, int64_t ntab,
                int mask_axis, int64_t mask_off)
{
    GUARD(fd_run_host(mk_fd(in, nin, out, nout, ndim, shape, mode, nterms, iterm, dterm, tab, ntab, mask_axis,
                            mask_off)))
}

int xinv_fd_f64_dev(const double *const *in, int nin, double *const *out, int nout, int ndim, const int64_t *shape,
                    int mode, int nterms, const int64_t *iterm, const double *dterm, const double *tab, int64_t ntab,
                    int mask_axis, int64_t mask_off, void *stream)
{
    GUARD(fd_run_dev(mk_fd(in, nin, out, nout, ndim, shape, mode, nterms, iterm, dterm, tab, ntab, mask_axis,
                           mask_off), (hipStream_t)stream))
}

// ---- resident plans (include/xinv.h: "resident plans") ---------------------------------------------------------
int xinv_plan_create_standard_2d_f64_dev(xinv_plan **plan, const double *A, const double *B, const double *C,
                                         const double *F, int64_t nbatch, const int64_t *strides, int64_t yc,
                                         int64_t xc, double dely, double delx, int BCy, int BCx, double delxSqr,
                                         double ratioQtr, double ratioSqr, double optArg, double undef,
                                         const xinv_options *opt, void *stream)
{
    (void)dely;
    const double *c[] = { A, B, C, F };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.optArg = optArg;
    sc.undef = undef;
    return run_form(RUN_PLAN, KIND_STD2D, plan, nullptr, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc, nullptr, 0,
                    0.0, opt, stream);
}

int xinv_plan_create_general_2d_f64_dev(xinv_plan **plan, const double *A, const double *B, const double *C,
                                        const double *D, const double *E, const double *F, const double *G,
                                        int64_t nbatch, const int64_t *strides, int64_t yc, int64_t xc, double dely,
                                        double delx, int BCy, int BCx, double delxSqr, double ratio, double ratioQtr,
                                        double ratioSqr, double optArg, double undef, const xinv_options *opt,
                                        void *stream)
{
    (void)dely;
    const double *c[] = { A, B, C, D, E, F, G };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratio = ratio; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr;
    sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_PLAN, KIND_GEN2D, plan, nullptr, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc, nullptr, 0,
                    0.0, opt, stream);
}

int xinv_plan_create_standard_3d_f64_dev(xinv_plan **plan, const double *A, const double *B, const double *C,
                                         const double *F, int64_t nbatch, const int64_t *strides, int64_t zc,
                                         int64_t yc, int64_t xc, double delz, double dely, double delx, int BCz,
                                         int BCy, int BCx, double delxSqr, double ratio2Sqr, double ratio1Sqr,
                                         double optArg, double undef, const xinv_options *opt, void *stream)
{
    (void)delz; (void)dely; (void)delx;
    const double *c[] = { A, B, C, F };
    XinvScal sc = {};
    sc.delxSqr = delxSqr; sc.ratio2Sqr = ratio2Sqr; sc.ratio1Sqr = ratio1Sqr; sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_PLAN, KIND_STD3D, plan, nullptr, c, nbatch, strides, zc, yc, xc, BCz, BCy, BCx, sc, nullptr,
                    0, 0.0, opt, stream);
}

int xinv_plan_create_general_3d_f64_dev(xinv_plan **plan, const double *A, const double *B, const double *C,
                                        const double *D, const double *E, const double *F, const double *G,
                                        const double *H, int64_t nbatch, const int64_t *strides, int64_t zc,
                                        int64_t yc, int64_t xc, double delz, double dely, double delx, int BCz,
                                        int BCy, int BCx, double delxSqr, double ratio2, double ratio1,
                                        double ratio2Sqr, double ratio1Sqr, double optArg, double undef,
                                        const xinv_options *opt, void *stream)
{
    (void)delz; (void)dely;
    const double *c[] = { A, B, C, D, E, F, G, H };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratio2 = ratio2; sc.ratio1 = ratio1; sc.ratio2Sqr = ratio2Sqr;
    sc.ratio1Sqr = ratio1Sqr; sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_PLAN, KIND_GEN3D, plan, nullptr, c, nbatch, strides, zc, yc, xc, BCz, BCy, BCx, sc, nullptr,
                    0, 0.0, opt, stream);
}

int xinv_plan_create_general_bih_2d_f64_dev(xinv_plan **plan, const double *A, const double *B, const double *C,
                                            const double *D, const double *E, const double *F, const double *G,
                                            const double *H, const double *I, const double *J, int64_t nbatch,
                                            const int64_t *strides, int64_t yc, int64_t xc, double dely, double delx,
                                            int BCy, int BCx, double delxSSr, double delxTr, double delxSqr,
                                            double ratio, double ratioSSr, double ratioQtr, double ratioSqr,
                                            double optArg, double undef, const xinv_options *opt, void *stream)
{
    (void)dely; (void)delx;
    const double *c[] = { A, B, C, D, E, F, G, H, I, J };
    XinvScal sc = {};
    sc.delxSSr = delxSSr; sc.delxTr = delxTr; sc.delxSqr = delxSqr; sc.ratio = ratio; sc.ratioSSr = ratioSSr;
    sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.optArg = optArg; sc.undef = undef;
    return run_form(RUN_PLAN, KIND_BIH2D, plan, nullptr, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc, nullptr, 0,
                    0.0, opt, stream);
}

int xinv_plan_create_standard_2d_test_f64_dev(xinv_plan **plan, const double *A, const double *B, const double *C,
                                              const double *D, const double *E, const double *F, int64_t nbatch,
                                              const int64_t *strides, int64_t yc, int64_t xc, double dely,
                                              double delx, int BCy, int BCx, double delxSqr, double ratioQtr,
                                              double ratioSqr, double optArg, double undef, const xinv_options *opt,
                                              void *stream)
{
    (void)dely;
    const double *c[] = { A, B, C, D, E, F };
    XinvScal sc = {};
    sc.delx = delx; sc.delxSqr = delxSqr; sc.ratioQtr = ratioQtr; sc.ratioSqr = ratioSqr; sc.optArg = optArg;
    sc.undef = undef;
    return run_form(RUN_PLAN, KIND_STD2DT, plan, nullptr, c, nbatch, strides, 1, yc, xc, 0, BCy, BCx, sc, nullptr, 0,
                    0.0, opt, stream);
}

int xinv_plan_solve_f64_dev(xinv_plan *plan, double *S, double *flags, int64_t mxLoop, double tolerance, void *stream)
{
    GUARD(plan_solve(plan, S, flags, mxLoop, tolerance, (hipStream_t)stream))
}

int xinv_plan_solve_frames_f64_dev(xinv_plan *plan, double *S, double *frames, int64_t nframes, int64_t frame_stride,
                                   double *flags, int64_t mxLoop, double tolerance, void *stream)
{
    GUARD(plan_solve_frames(plan, S, frames, nframes, frame_stride, flags, mxLoop, tolerance, (hipStream_t)stream))
}

int xinv_plan_refresh(xinv_plan *plan, void *stream)
{
    if (!plan || plan->magic != XINV_PLAN_MAGIC) return fail_arg("xinv_plan_refresh: not a live plan");
    GUARD(plan_build(plan, (hipStream_t)stream))
}

int xinv_plan_destroy(xinv_plan *plan)
{
    if (!plan) return XINV_OK;
    if (plan->magic != XINV_PLAN_MAGIC) return fail_arg("xinv_plan_destroy: not a live plan");
    {   // (not while a solve on this device is using the plan's buffers)
        Workspace *ws = get_ws(plan->device);
        std::lock_guard<std::recursive_mutex> lock(ws->busy);
        plan_free(plan);
    }
    return XINV_OK;
}

// Gill-Matsuno (u, v) from the mass field; every array argument is a DEVICE pointer.
static int gm_flow_dev(const double *S, double *u, double *v, int64_t nbatch, int64_t yc, int64_t xc,
                       const double *ytab, const double *xtab, int yuniform, int xuniform,
                       const double *rowtab, double deg2m, int latlon, hipStream_t st)
{
    if (!S || !u || !v || !ytab || !xtab || !rowtab || nbatch < 1 || yc < 2 || xc < 2)
        return fail_arg("bad arguments to xinv_gm_flow_f64_dev");
    FlowArgs a;
    memset(&a, 0, sizeof a);
    a.S = S; a.u = u; a.v = v; a.nbatch = nbatch; a.yc = yc; a.xc = xc;
    // ytab / xtab: [3][n] interior weights a, b, c followed by {dx, dx0, dxn}
    a.gy.a = ytab; a.gy.b = ytab + yc; a.gy.c = ytab + 2 * yc; a.gy.uniform = yuniform;
    a.gx.a = xtab; a.gx.b = xtab + xc; a.gx.c = xtab + 2 * xc; a.gx.uniform = xuniform;
    double hy[3], hx[3];
    HIPCHK(hipMemcpyAsync(hy, ytab + 3 * yc, sizeof hy, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hx, xtab + 3 * xc, sizeof hx, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    a.gy.dx = hy[0]; a.gy.dx0 = hy[1]; a.gy.dxn = hy[2];
    a.gx.dx = hx[0]; a.gx.dx0 = hx[1]; a.gx.dxn = hx[2];
    a.coef1 = rowtab; a.coef2 = rowtab + yc; a.cosl = rowtab + 2 * yc;
    a.deg2m = deg2m; a.latlon = latlon;
    for (int64_t m0 = 0; m0 < nbatch; m0 += XINV_MEMBER_CHUNK) {
        const int64_t nm = std::min<int64_t>(XINV_MEMBER_CHUNK, nbatch - m0);
        FlowArgs b = a;
        b.S = S + m0 * yc * xc; b.u = u + m0 * yc * xc; b.v = v + m0 * yc * xc;
        if (yc > 65535) return fail_arg("xinv_gm_flow_f64_dev: yc > 65535 not supported");
        hipLaunchKernelGGL(k_gm_flow, dim3(cdiv(xc, 256), (unsigned)yc, (unsigned)nm), dim3(256), 0, st, b);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return XINV_OK;
}

int xinv_gm_flow_f64_dev(const double *S, double *u, double *v, int64_t nbatch, int64_t yc,
                         int64_t xc, const double *ytab, const double *xtab, int yuniform,
                         int xuniform, const double *rowtab, double deg2m, int latlon, void *stream)
{
    GUARD(gm_flow_dev(S, u, v, nbatch, yc, xc, ytab, xtab, yuniform, xuniform, rowtab, deg2m, latlon,
                      (hipStream_t)stream))
}

static int abs_norm_dev(const double *S, int64_t n, double undef, double *out, hipStream_t st)
{
    if (!S || !out || n < 1) return fail_arg("bad arguments to xinv_abs_norm_f64_dev");
    int device;
    HIPCHK(hipGetDevice(&device));
    Workspace *ws = get_ws(device);
    // shares the solver's partials / ctl buffers: one user of a device's workspace at a time
    std::lock_guard<std::recursive_mutex> ws_lock(ws->busy);
    int rc = ensure_dev(&ws->partials, &ws->partials_cap,
                        (size_t)XINV_NORM_BLOCKS * (sizeof(double) + sizeof(long long)) + 64);
    if (rc) return rc;
    rc = ensure_dev(&ws->ctl, &ws->ctl_cap, sizeof(XinvCtl));
    if (rc) return rc;
    NormArgs a;
    memset(&a, 0, sizeof a);
    a.S = S; a.sS = 0; a.n = n; a.undef = undef;
    a.psum = (double *)ws->partials;
    a.pcnt = (long long *)((char *)ws->partials + XINV_NORM_BLOCKS * sizeof(double));
    a.ctl = ws->ctl; a.force = 1; a.member0 = 0;
    int nblk = (int)std::min<int64_t>(XINV_NORM_BLOCKS, std::max<int64_t>(1, n / 2048));
    double *dout = (double *)((char *)ws->partials + XINV_NORM_BLOCKS * (sizeof(double) + sizeof(long long)));
    hipLaunchKernelGGL(k_norm_partial, dim3(nblk, 1, 1), dim3(256, 1, 1), 0, st, a);
    hipLaunchKernelGGL(k_norm_out, dim3(1), dim3(64), 0, st, a.psum, a.pcnt, nblk, dout);
    HIPCHK(hipMemcpyAsync(out, dout, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return XINV_OK;
}

int xinv_abs_norm_f64_dev(const double *S, int64_t n, double undef, double *out, void *stream)
{
    GUARD(abs_norm_dev(S, n, undef, out, (hipStream_t)stream))
}

// ---- multigrid grid transfers (k_mg_restrict, k_mg_prolong: xinv_mg.h) -------------------------------------------
// The core is padded to three dims with leading length-1 dims; blocks of XINV_MG_WG lanes cover one row of the last axis.
static int mg_shape(int64_t nbatch, int ndim, const int64_t *shape, int64_t n3[3])
{
    if (nbatch < 1 || ndim < 1 || ndim > 3 || !shape) return fail_arg("multigrid: need nbatch >= 1 and 1 to 3 core dims");
    for (int a = 0; a < 3; ++a) n3[a] = a < 3 - ndim ? 1 : shape[a - (3 - ndim)];
    for (int a = 0; a < 3; ++a)
        if (n3[a] < 1) return fail_arg("multigrid: a core dim is empty");
    return XINV_OK;
}

static int mg_restrict_dev(const double *fine, double *coarse, int64_t nbatch, int ndim, const int64_t *fshape,
                           const int64_t *ratio, double undef, hipStream_t st)
{
    MgRestrictArgs a;
    memset(&a, 0, sizeof a);
    if (!fine || !coarse || !ratio) return fail_arg("multigrid restrict: null argument");
    int rc = mg_shape(nbatch, ndim, fshape, a.fn);
    if (rc) return rc;
    for (int a3 = 0; a3 < 3; ++a3) {
        a.r[a3] = a3 < 3 - ndim ? 1 : ratio[a3 - (3 - ndim)];
        if (a.r[a3] < 1 || a.fn[a3] / a.r[a3] < 1) return fail_arg("multigrid restrict: need 1 <= ratio <= length");
        a.cn[a3] = a.fn[a3] / a.r[a3];
    }
    a.fine = fine; a.coarse = coarse;
    a.fslice = a.fn[0] * a.fn[1] * a.fn[2];
    a.cslice = a.cn[0] * a.cn[1] * a.cn[2];
    a.rows = nbatch * a.cn[0] * a.cn[1];
    a.nbx = (a.cn[2] + XINV_MG_WG - 1) / XINV_MG_WG;
    a.undef = undef; a.nan = undef != undef;
    xinv_launch_mg_restrict(a, a.rows * a.nbx, st);
    HIPCHK(hipGetLastError());
    return XINV_OK;
}

static int mg_prolong_dev(const double *coarse, double *fine, const double *force, int64_t nbatch, int ndim,
                          const int64_t *cshape, const int64_t *fshape, const int64_t *idx, const double *w,
                          int keep_edges, double undef, hipStream_t st)
{
    MgProlongArgs a;
    memset(&a, 0, sizeof a);
    if (!coarse || !fine || !idx || !w) return fail_arg("multigrid prolong: null argument");
    int rc = mg_shape(nbatch, ndim, fshape, a.fn);
    if (!rc) rc = mg_shape(nbatch, ndim, cshape, a.cn);
    if (rc) return rc;
    if (keep_edges < 0 || keep_edges >= (1 << ndim)) return fail_arg("multigrid prolong: keep_edges names no core dim");
    const int pad = 3 - ndim;
    int64_t off = 0, woff = 0;
    for (int d = 0; d < ndim; ++d) {               // per core dim: lo[n], hi[n] in idx; w[n] in w
        const int64_t n = a.fn[pad + d];
        a.lo[pad + d] = idx + off; a.hi[pad + d] = idx + off + n; a.w[pad + d] = w + woff;
        off += 2 * n; woff += n;
        if (keep_edges & (1 << d)) a.keep |= 1 << (pad + d);
    }
    a.coarse = coarse; a.fine = fine; a.force = force;
    a.fslice = a.fn[0] * a.fn[1] * a.fn[2];
    a.cslice = a.cn[0] * a.cn[1] * a.cn[2];
    a.rows = nbatch * a.fn[0] * a.fn[1];
    a.nbx = (a.fn[2] + XINV_MG_WG - 1) / XINV_MG_WG;
    a.undef = undef; a.nd = ndim;
    if (xinv_launch_mg_prolong(a, a.rows * a.nbx, st)) return fail_arg("multigrid prolong: no kernel for this rank");
    HIPCHK(hipGetLastError());
    return XINV_OK;
}

int xinv_mg_restrict_f64_dev(const double *fine, double *coarse, int64_t nbatch, int ndim, const int64_t *fshape,
                             const int64_t *ratio, double undef, void *stream)
{
    GUARD(mg_restrict_dev(fine, coarse, nbatch, ndim, fshape, ratio, undef, (hipStream_t)stream))
}

int xinv_mg_prolong_f64_dev(const double *coarse, double *fine, const double *force, int64_t nbatch, int ndim,
                            const int64_t *cshape, const int64_t *fshape, const int64_t *idx, const double *w,
                            int keep_edges, double undef, void *stream)
{
    GUARD(mg_prolong_dev(coarse, fine, force, nbatch, ndim, cshape, fshape, idx, w, keep_edges, undef,
                         (hipStream_t)stream))
}

} // extern "C"
