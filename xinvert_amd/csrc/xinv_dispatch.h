// xinv_dispatch.h -- which instantiation of a sweep kernel a plan runs, stated as a value.  Each kernel family is
// instantiated in its own translation unit (xinv_tu_*.hip) so that the library builds in parallel and a change to one
// family recompiles one file.  A unit exports ONE function, its resolver: SweepVariant -> KernelRef, the unit's one
// ladder over the template parameters.  The host driver (xinv_hip.hip) picks the resolver (xinv_kernel, xinv_launch.h),
// keeps the reference in the plan and launches / asks the occupancy through it (kernel_launch, kernel_occupancy).
#pragma once
#include <hip/hip_runtime.h>
#include "xinv_fused.h"
#include "xinv_pipe2d.h"
#include "xinv_fused3d.h"
#include "xinv_fused3dg.h"
#include "xinv_pipe3d.h"
#include "xinv_fusedbih.h"

#define XINV_HIDDEN __attribute__((visibility("hidden")))

// the operator forms (Problem::kind)
enum { KIND_STD2D = 0, KIND_GEN2D = 1, KIND_STD3D = 2, KIND_BIH2D = 3, KIND_STD2DT = 4, KIND_GEN3D = 5 };

// A kernel instantiation: its host-side address (what hipLaunchKernel takes) and its workgroup size.  fn == nullptr:
// the variant is not instantiated.  Addresses live as long as the process.
struct KernelRef { const void *fn; unsigned threads; };

enum SweepFamily {
    FAM_FUSED2D,             // k_fused2d: 2-D 5-point forms, K sweeps per pass
    FAM_PIPE2D,              // k_pipe2d: ... the wave-pipelined pass of XINV_PIPE_P sweeps
    FAM_FUSED9,              // k_fused9: 2-D 9-point forms
    FAM_FUSED3D,             // k_fused3d: standard 3-D form, one sweep per pass
    FAM_PIPE3D,              // k_pipe3d: ... two sweeps per pass
    FAM_FUSED3DG,            // k_fused3dg: general 3-D form
    FAM_BIH,                 // k_fusedbih: biharmonic form
};

// Everything that selects an instantiation.  A family reads the fields it has a template parameter for.
struct SweepVariant {
    int family, kind;
    int K;                   // sweeps per pass (k_fused2d, k_fused9)
    unsigned um;             // k_fused2d / k_pipe2d: streams read as one scalar per row (| 2 on the point-factor model: C read out of A)
    bool al, ext, seam, fma; // aligned vector loads; BCy = 'extend'; odd-xc periodic seam; contracted arithmetic
    bool pq;                 // k_fused2d: the point-factor stream (FusedGen2DQ / FusedGen2DQA)
    bool pipe_fr;            // k_pipe2d: the forcing rides the LDS ring
    int NW;                  // 3-D: wavefronts per workgroup
    bool uni;                // k_fused3d: coefficients constant along x
    bool per, zbe;           // k_fusedbih: periodic x; B == E == 0
    int vm;                  // k_fusedbih: where the coefficients come from (xinv_fusedbih.h: 0 per-row records, 1 A C D F as
                             // vector streams, 2 all nine, 3 as 1 with C read out of A and F out of D)
};

// xinv_tu_fused2d.hip and xinv_tu_pipe2d.hip are compiled once per model, -DXINV_TU_MODEL=<value below>, and once more per
// seam variant (-DXINV_TU_SEAM=1: odd-xc periodic seam, unaligned strips only); each unit defines its own specialisation.
enum { FUSED2D_STD = 0, FUSED2D_GEN = 1, FUSED2D_STD2DT = 2, FUSED2D_STDF = 3, FUSED2D_GENF = 4, FUSED2D_GENQ = 5 };
enum { PIPE2D_STD = 0, PIPE2D_GEN = 1, PIPE2D_FMA = 2 };
template <int MODEL, bool SEAM> XINV_HIDDEN KernelRef xinv_kernel_fused2d(const SweepVariant &v);
template <int MODEL, bool SEAM> XINV_HIDDEN KernelRef xinv_kernel_pipe2d(const SweepVariant &v);
XINV_HIDDEN KernelRef xinv_kernel_fused9(const SweepVariant &v);
XINV_HIDDEN KernelRef xinv_kernel_fused3d(const SweepVariant &v);        // FAM_FUSED3D and FAM_FUSED3DG
XINV_HIDDEN KernelRef xinv_kernel_fused3d_fma(const SweepVariant &v);    // FAM_FUSED3D, contracted arithmetic
XINV_HIDDEN KernelRef xinv_kernel_fused3d_seam(const SweepVariant &v);   // FAM_FUSED3D and FAM_FUSED3DG, odd-xc periodic seam
XINV_HIDDEN KernelRef xinv_kernel_pipe3d(const SweepVariant &v);
XINV_HIDDEN KernelRef xinv_kernel_bih(const SweepVariant &v);

// what a resolver's ladder ends in
template <class A>
static inline KernelRef kernel_ref(void (*k)(A), unsigned threads) { return KernelRef{(const void *)k, threads}; }
