// xinv_tu_fused3d_fma.hip -- the contracted-arithmetic variants (XINV_FLAG_FMA) of the 3-D standard-form kernels:
// k_fused3d with x-uniform coefficients (k_pipe3d's: xinv_tu_pipe3d.hip).
#include "xinv_dispatch.h"

template <int NW>
static KernelRef fused3d_fma_nw(bool al, bool ext)
{
    if (al) return ext ? kernel_ref(k_fused3d<NW, true, true, true, true>, NW * 64) : kernel_ref(k_fused3d<NW, true, true, false, true>, NW * 64);
    return ext ? kernel_ref(k_fused3d<NW, false, true, true, true>, NW * 64) : kernel_ref(k_fused3d<NW, false, true, false, true>, NW * 64);
}

KernelRef xinv_kernel_fused3d_fma(const SweepVariant &v)
{
    if (v.NW == 8) return fused3d_fma_nw<8>(v.al, v.ext);
    if (v.NW == 12) return fused3d_fma_nw<12>(v.al, v.ext);
    if (v.NW == 16 && !v.ext)                            // (as the plain kernel: sixteen wavefronts without 'extend' only)
        return v.al ? kernel_ref(k_fused3d<16, true, true, false, true>, 16 * 64) : kernel_ref(k_fused3d<16, false, true, false, true>, 16 * 64);
    return KernelRef{};
}
