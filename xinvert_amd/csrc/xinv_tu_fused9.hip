// xinv_tu_fused9.hip -- instantiations of k_fused9 (the 9-point forms, B != 0).
#include "xinv_dispatch.h"
#include "xinv_fused9.h"

template <class M, int K>
static KernelRef fused9_k(const SweepVariant &v)
{
    if (v.seam)                                          // (odd xc: unaligned strips)
        return v.ext ? kernel_ref(k_fused9<M, K, false, true, true>, 256) : kernel_ref(k_fused9<M, K, false, false, true>, 256);
    if (v.al) return v.ext ? kernel_ref(k_fused9<M, K, true, true, false>, 256) : kernel_ref(k_fused9<M, K, true, false, false>, 256);
    return v.ext ? kernel_ref(k_fused9<M, K, false, true, false>, 256) : kernel_ref(k_fused9<M, K, false, false, false>, 256);
}

KernelRef xinv_kernel_fused9(const SweepVariant &v)
{
    if (v.kind == KIND_GEN2D) {
        if (v.K == 1) return fused9_k<Fused9Gen, 1>(v);
        if (v.K == 2) return fused9_k<Fused9Gen, 2>(v);
    } else {
        if (v.K == 1) return fused9_k<Fused9Std, 1>(v);
        if (v.K == 2) return fused9_k<Fused9Std, 2>(v);
        if (v.K == 3) return fused9_k<Fused9Std, 3>(v);
    }
    return KernelRef{};
}
