// xinv_tu_fd.hip -- instantiations of k_fd (finite-difference operators: xinv_fd.h), one per term count.
#define XINV_FD_DEVICE
#include "xinv_fd.h"

int xinv_launch_fd(const FdArgs &a, int64_t nblocks, hipStream_t st)
{
    const dim3 grid((unsigned)nblocks), block(XINV_FD_WG);
    switch (a.nt) {
    case 1: hipLaunchKernelGGL(k_fd<1>, grid, block, 0, st, a); return 0;
    case 2: hipLaunchKernelGGL(k_fd<2>, grid, block, 0, st, a); return 0;
    case 3: hipLaunchKernelGGL(k_fd<3>, grid, block, 0, st, a); return 0;
    case 4: hipLaunchKernelGGL(k_fd<4>, grid, block, 0, st, a); return 0;
    }
    return 1;
}
