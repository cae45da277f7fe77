// xinv_tu_bih.hip -- instantiations of k_fusedbih (one-pass biharmonic kernel).
#include "xinv_dispatch.h"

// vm: 0 = A..I per row (records); 1 = A, C, D, F vector streams (B == E == 0: zbe); 3 = ... with C read out of A, F out of D;
//     2 = all nine vector streams
template <int VM>
static KernelRef bih_vm(bool per, bool zbe)
{
    if constexpr (VM != 1 && VM != 3)
        if (!zbe) return per ? kernel_ref(k_fusedbih<true, false, VM>, 256) : kernel_ref(k_fusedbih<false, false, VM>, 256);
    return per ? kernel_ref(k_fusedbih<true, true, VM>, 256) : kernel_ref(k_fusedbih<false, true, VM>, 256);
}

KernelRef xinv_kernel_bih(const SweepVariant &v)
{
    if (v.vm == 1) return bih_vm<1>(v.per, v.zbe);
    if (v.vm == 3) return bih_vm<3>(v.per, v.zbe);
    if (v.vm == 2) return bih_vm<2>(v.per, v.zbe);
    return bih_vm<0>(v.per, v.zbe);
}
