// xinv_tu_resid.hip -- instantiations of k_resid2d / k_resid3d / k_resid_final (the residual L(S) - F: xinv_resid.h).
#define XINV_RESID_KERNELS
#include "xinv_resid.h"

#define RESID_MEMBER_CHUNK 32768    /* members per launch, as the colour kernels chunk them (grid.z <= 65535) */

template <int FORM, bool NINE>
static void launch2d(const ResidArgs &a, dim3 grid, hipStream_t st)
{
    hipLaunchKernelGGL((k_resid2d<FORM, NINE>), grid, dim3(XINV_RESID_WG), 0, st, a);
}

int xinv_launch_resid(int form, bool nine, ResidArgs a, int64_t nbatch, double *norms, hipStream_t st)
{
    const bool threed = form == RESID_STD3D || form == RESID_GEN3D;
    if (!threed) {
        const int64_t gx = (a.xc + XINV_RESID_WG - 1) / XINV_RESID_WG, gy = (a.yc + XINV_RESID_ROWS - 1) / XINV_RESID_ROWS;
        if (gx > 0x7fffffff || gy > 65535) return 1;
        for (int64_t m0 = 0; m0 < nbatch; m0 += RESID_MEMBER_CHUNK) {
            const int64_t nm = nbatch - m0 < RESID_MEMBER_CHUNK ? nbatch - m0 : RESID_MEMBER_CHUNK;
            const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)nm);
            a.member0 = m0;
            if (form == RESID_STD2D) { if (nine) launch2d<RESID_STD2D, true>(a, grid, st); else launch2d<RESID_STD2D, false>(a, grid, st); }
            else if (form == RESID_GEN2D) { if (nine) launch2d<RESID_GEN2D, true>(a, grid, st); else launch2d<RESID_GEN2D, false>(a, grid, st); }
            else launch2d<RESID_STD2DT, true>(a, grid, st);
        }
    } else {
        const int64_t gx = (a.xc + XINV_RESID_TX - 1) / XINV_RESID_TX, gy = (a.yc + XINV_RESID_TY - 1) / XINV_RESID_TY;
        const int64_t ns = (a.zc + XINV_RESID_PLANES - 1) / XINV_RESID_PLANES;
        if (gx > 0x7fffffff || gy > 65535 || ns > 65535) return 1;
        a.nstrip = (int)ns;
        const int64_t chunk = 65535 / ns < RESID_MEMBER_CHUNK ? 65535 / ns : RESID_MEMBER_CHUNK;
        for (int64_t m0 = 0; m0 < nbatch; m0 += chunk) {
            const int64_t nm = nbatch - m0 < chunk ? nbatch - m0 : chunk;
            const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)(nm * ns)), block(XINV_RESID_TX, XINV_RESID_TY);
            a.member0 = m0;
            if (form == RESID_STD3D) hipLaunchKernelGGL((k_resid3d<RESID_STD3D>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((k_resid3d<RESID_GEN3D>), grid, block, 0, st, a);
        }
    }
    if (a.part && norms)
        for (int64_t m0 = 0; m0 < nbatch; m0 += RESID_MEMBER_CHUNK) {
            const int64_t nm = nbatch - m0 < RESID_MEMBER_CHUNK ? nbatch - m0 : RESID_MEMBER_CHUNK;
            hipLaunchKernelGGL(k_resid_final, dim3((unsigned)nm), dim3(64), 0, st, (const double *)a.part, a.nslot, norms, m0);
        }
    return 0;
}
