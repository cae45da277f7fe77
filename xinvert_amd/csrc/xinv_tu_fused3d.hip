// xinv_tu_fused3d.hip -- instantiations of k_fused3d (standard 3-D form) and k_fused3dg (general 3-D form with x-uniform
// coefficients).  k_pipe3d (two sweeps per pass) has its own unit, xinv_tu_pipe3d.hip.
#include "xinv_dispatch.h"

template <int NW, bool AL>
static KernelRef fused3d_uni_ext(bool uni, bool ext)
{
    if (uni) return ext ? kernel_ref(k_fused3d<NW, AL, true, true>, NW * 64) : kernel_ref(k_fused3d<NW, AL, true, false>, NW * 64);
    return ext ? kernel_ref(k_fused3d<NW, AL, false, true>, NW * 64) : kernel_ref(k_fused3d<NW, AL, false, false>, NW * 64);
}

static KernelRef fused3d(const SweepVariant &v)
{
    if (v.NW == 8) return v.al ? fused3d_uni_ext<8, true>(v.uni, v.ext) : fused3d_uni_ext<8, false>(v.uni, v.ext);
    if (v.NW == 12) return v.al ? fused3d_uni_ext<12, true>(v.uni, v.ext) : fused3d_uni_ext<12, false>(v.uni, v.ext);
    // sixteen wavefronts leave 128 VGPRs per lane: enough for the x-uniform variant without 'extend' only (the other
    // sixteen-wavefront variants spilled 76-203 bytes per lane and are not instantiated: the planner gives them twelve)
    if (v.NW == 16 && v.uni && !v.ext)
        return v.al ? kernel_ref(k_fused3d<16, true, true, false>, 16 * 64) : kernel_ref(k_fused3d<16, false, true, false>, 16 * 64);
    return KernelRef{};
}

// general 3-D form (every coefficient array x-uniform; sixteen wavefronts: 128 VGPRs, spills -- not instantiated)
template <int NW>
static KernelRef fused3dg_nw(bool al, bool ext)
{
    if (al) return ext ? kernel_ref(k_fused3dg<NW, true, true>, NW * 64) : kernel_ref(k_fused3dg<NW, true, false>, NW * 64);
    return ext ? kernel_ref(k_fused3dg<NW, false, true>, NW * 64) : kernel_ref(k_fused3dg<NW, false, false>, NW * 64);
}

KernelRef xinv_kernel_fused3d(const SweepVariant &v)
{
    if (v.family == FAM_FUSED3D) return fused3d(v);
    if (v.NW == 8) return fused3dg_nw<8>(v.al, v.ext);
    if (v.NW == 12) return fused3dg_nw<12>(v.al, v.ext);
    return KernelRef{};
}
