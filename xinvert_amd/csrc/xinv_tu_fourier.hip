// xinv_tu_fourier.hip -- instantiations of k_rowdft / k_fourier_tri / k_fourier_check (the direct Fourier solve: xinv_fourier.h)
// and of a plan's k_fourier_factor / k_fourier_subst.
#define XINV_FOURIER_KERNELS
#include "xinv_fourier.h"

// 0, or the HIP error of raising the kernel's dynamic-LDS limit (a pair of n complex doubles passes 64 KiB at n = 2048)
int xinv_launch_rowdft(const RowDftArgs &a, bool inverse, hipStream_t st)
{
    const size_t lds = (size_t)a.n * 32;
    const void *fn = inverse ? (const void *)k_rowdft<true> : (const void *)k_rowdft<false>;
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const dim3 grid((unsigned)((a.nrows / a.rpm) * ((a.rpm + 1) / 2))), block(XINV_DFT_WG);
    if (inverse) hipLaunchKernelGGL(k_rowdft<true>, grid, block, lds, st, a);
    else hipLaunchKernelGGL(k_rowdft<false>, grid, block, lds, st, a);
    return 0;
}

void xinv_launch_fourier_tri(FourierTriArgs a, int64_t nbatch, hipStream_t st)
{
    const unsigned gx = (unsigned)((a.K + XINV_FTRI_WG - 1) / XINV_FTRI_WG);
    xinv_launch_chunks(k_fourier_tri, a, &FourierTriArgs::member0, nbatch, gx, XINV_FTRI_WG, st);
}

void xinv_launch_fourier_factor(FourierFactorArgs a, int64_t nset, hipStream_t st)
{
    const unsigned gx = (unsigned)((a.K + XINV_FFAC_WG - 1) / XINV_FFAC_WG);
    xinv_launch_chunks(k_fourier_factor, a, &FourierFactorArgs::set0, nset, gx, XINV_FFAC_WG, st);
}

void xinv_launch_fourier_subst(FourierSubstArgs a, int64_t nbatch, hipStream_t st)
{
    const unsigned gx = (unsigned)((2 * a.K + XINV_FSUB_WG - 1) / XINV_FSUB_WG);
    xinv_launch_chunks(k_fourier_subst, a, &FourierSubstArgs::member0, nbatch, gx, XINV_FSUB_WG, st);
}

void xinv_launch_fourier_check(FourierCheckArgs a, int64_t nbatch, hipStream_t st)
{
    xinv_launch_chunks(k_fourier_check, a, &FourierCheckArgs::member0, nbatch, (unsigned)a.yc, XINV_FCHK_WG, st);
}
