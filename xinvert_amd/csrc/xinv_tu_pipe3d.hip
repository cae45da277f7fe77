// xinv_tu_pipe3d.hip -- instantiations of k_pipe3d (two sweeps per pass, pipelined across two groups of eight wavefronts:
// xinv_pipe3d.h; x-uniform coefficients), plain and contracted (XINV_FLAG_FMA).  Compiled with
// -amdgpu-sched-strategy=iterative-minreg (xinvert_amd/build.py): sixteen wavefronts leave 128 VGPRs, and with the default
// scheduler the variant that carries the forcing through the LDS ring spilled 11-30 of them.
#include "xinv_dispatch.h"

KernelRef xinv_kernel_pipe3d(const SweepVariant &v)
{
    constexpr int G = XINV_P3_G, RR = XINV_P3_RR;
    constexpr unsigned T = 2 * G * 64;
    if (v.fma) return v.al ? kernel_ref(k_pipe3d<G, RR, true, true>, T) : kernel_ref(k_pipe3d<G, RR, false, true>, T);
    if (v.ext)                                           // BCy = 'extend' (never with the seam: the planner keeps the one-sweep kernel)
        return v.al ? kernel_ref(k_pipe3d<G, RR, true, false, false, true>, T) : kernel_ref(k_pipe3d<G, RR, false, false, false, true>, T);
    if (v.seam) return kernel_ref(k_pipe3d<G, RR, false, false, true>, T);       // (periodic x, odd xc)
    return v.al ? kernel_ref(k_pipe3d<G, RR, true>, T) : kernel_ref(k_pipe3d<G, RR, false>, T);
}
