// xinv_tu_mg.hip -- the multigrid grid transfers (xinv_mg.h): k_mg_restrict and k_mg_prolong per core rank.
#define XINV_MG_DEVICE
#include "xinv_mg.h"

static dim3 mg_grid(int64_t nblocks)
{
    return dim3((unsigned)(nblocks < XINV_MG_MAXBLOCKS ? nblocks : XINV_MG_MAXBLOCKS));
}

int xinv_launch_mg_restrict(const MgRestrictArgs &a, int64_t nblocks, hipStream_t st)
{
    hipLaunchKernelGGL(k_mg_restrict, mg_grid(nblocks), dim3(XINV_MG_WG), 0, st, a);
    return 0;
}

int xinv_launch_mg_prolong(const MgProlongArgs &a, int64_t nblocks, hipStream_t st)
{
    const dim3 grid = mg_grid(nblocks), block(XINV_MG_WG);
    switch (a.nd) {
    case 1: hipLaunchKernelGGL(k_mg_prolong<1>, grid, block, 0, st, a); return 0;
    case 2: hipLaunchKernelGGL(k_mg_prolong<2>, grid, block, 0, st, a); return 0;
    case 3: hipLaunchKernelGGL(k_mg_prolong<3>, grid, block, 0, st, a); return 0;
    }
    return 1;
}
