// xinv_tu_tridiag.hip -- instantiations of k_tridiag (trace / traceCyclic and the direct 1-D solve: xinv_tridiag.h).
#include "xinv_tridiag.h"

void xinv_launch_tridiag(const TridiagArgs &a, bool fused, bool cyclic, hipStream_t st)
{
    const dim3 grid((unsigned)((a.nbatch + XINV_TRI_SYS - 1) / XINV_TRI_SYS)), block(XINV_TRI_SYS);
    if (fused) {
        if (cyclic) hipLaunchKernelGGL((k_tridiag<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_tridiag<true, false>), grid, block, 0, st, a);
    } else {
        if (cyclic) hipLaunchKernelGGL((k_tridiag<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_tridiag<false, false>), grid, block, 0, st, a);
    }
}
