// xinv_tu_fused3d_seam.hip -- k_fused3d / k_fused3dg with the odd-xc periodic seam inside the kernel (SEAM variants: unaligned strips,
// the even-ring layout; xinv_fused3d.h), eight or twelve wavefronts.
#include "xinv_dispatch.h"

template <int NW>
static KernelRef seam_nw(const SweepVariant &v)
{
    if (v.family == FAM_FUSED3DG)                        // general 3-D form (x-uniform coefficients)
        return v.ext ? kernel_ref(k_fused3dg<NW, false, true, true>, NW * 64) : kernel_ref(k_fused3dg<NW, false, false, true>, NW * 64);
    if (v.uni) return v.ext ? kernel_ref(k_fused3d<NW, false, true, true, false, true>, NW * 64) : kernel_ref(k_fused3d<NW, false, true, false, false, true>, NW * 64);
    return v.ext ? kernel_ref(k_fused3d<NW, false, false, true, false, true>, NW * 64) : kernel_ref(k_fused3d<NW, false, false, false, false, true>, NW * 64);
}

KernelRef xinv_kernel_fused3d_seam(const SweepVariant &v)
{
    if (v.NW == 8) return seam_nw<8>(v);
    if (v.NW == 12) return seam_nw<12>(v);
    return KernelRef{};
}
