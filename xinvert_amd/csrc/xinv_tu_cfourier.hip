// xinv_tu_cfourier.hip -- instantiations of k_fourier_cfactor / k_fourier_csubst / k_fourier_gcheck (the direct Fourier solve
// of the 2-D general form: xinv_cfourier.h).  A unit of its own: the device code of xinv_tu_fourier.hip stays as it is.
#define XINV_CFOURIER_KERNELS
#include "xinv_cfourier.h"

#define CFOURIER_MEMBER_CHUNK 32768   /* members per launch (grid.y <= 65535) */

void xinv_launch_fourier_cfactor(CFourierFactorArgs a, int64_t nset, hipStream_t st)
{
    const unsigned gx = (unsigned)((a.K + XINV_CFAC_WG - 1) / XINV_CFAC_WG);
    for (int64_t s0 = 0; s0 < nset; s0 += CFOURIER_MEMBER_CHUNK) {
        const int64_t ns = nset - s0 < CFOURIER_MEMBER_CHUNK ? nset - s0 : CFOURIER_MEMBER_CHUNK;
        a.set0 = s0;
        hipLaunchKernelGGL(k_fourier_cfactor, dim3(gx, (unsigned)ns), dim3(XINV_CFAC_WG), 0, st, a);
    }
}

void xinv_launch_fourier_csubst(CFourierSubstArgs a, int64_t nbatch, hipStream_t st)
{
    const unsigned gx = (unsigned)((a.K + XINV_CSUB_WG - 1) / XINV_CSUB_WG);
    for (int64_t m0 = 0; m0 < nbatch; m0 += CFOURIER_MEMBER_CHUNK) {
        const int64_t nm = nbatch - m0 < CFOURIER_MEMBER_CHUNK ? nbatch - m0 : CFOURIER_MEMBER_CHUNK;
        a.member0 = m0;
        hipLaunchKernelGGL(k_fourier_csubst, dim3(gx, (unsigned)nm), dim3(XINV_CSUB_WG), 0, st, a);
    }
}

void xinv_launch_fourier_gcheck(CFourierCheckArgs a, int64_t nbatch, hipStream_t st)
{
    for (int64_t m0 = 0; m0 < nbatch; m0 += CFOURIER_MEMBER_CHUNK) {
        const int64_t nm = nbatch - m0 < CFOURIER_MEMBER_CHUNK ? nbatch - m0 : CFOURIER_MEMBER_CHUNK;
        a.member0 = m0;
        hipLaunchKernelGGL(k_fourier_gcheck, dim3((unsigned)a.yc, (unsigned)nm), dim3(XINV_GCHK_WG), 0, st, a);
    }
}
