// xinv_tu_std1d.hip -- instantiations of k_std1d (1-D standard form, register-resident: xinv_std1d.h).
#include "xinv_std1d.h"

int xinv_launch_std1d(const Std1dArgs &a, hipStream_t st)
{
    int ppl = 0, nw = 0;
    xinv_std1d_shape(a.xc, &ppl, &nw);
    if (nw > 1) {
        hipLaunchKernelGGL((k_std1d<8, true>), dim3((unsigned)a.nbatch), dim3(64 * nw), 0, st, a);
        return 0;
    }
    const dim3 grid((unsigned)((a.nbatch + XINV_STD1D_MEMBERS_PER_WG - 1) / XINV_STD1D_MEMBERS_PER_WG));
    const dim3 block(64 * XINV_STD1D_MEMBERS_PER_WG);
    switch (ppl) {
    case 2:  hipLaunchKernelGGL((k_std1d<2, false>), grid, block, 0, st, a); return 0;
    case 4:  hipLaunchKernelGGL((k_std1d<4, false>), grid, block, 0, st, a); return 0;
    case 8:  hipLaunchKernelGGL((k_std1d<8, false>), grid, block, 0, st, a); return 0;
    }
    return 1;
}
