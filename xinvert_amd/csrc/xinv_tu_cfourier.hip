// xinv_tu_cfourier.hip -- instantiations of k_fourier_cfactor / k_fourier_csubst / k_fourier_gcheck (the direct Fourier solve
// of the 2-D general form: xinv_cfourier.h).  A unit of its own: the device code of xinv_tu_fourier.hip stays as it is.
#define XINV_CFOURIER_KERNELS
#include "xinv_cfourier.h"
#include "xinv_fourier.h"             /* xinv_launch_chunks (no kernel of its own is instantiated here) */

void xinv_launch_fourier_cfactor(CFourierFactorArgs a, int64_t nset, hipStream_t st)
{
    const unsigned gx = (unsigned)((a.K + XINV_CFAC_WG - 1) / XINV_CFAC_WG);
    xinv_launch_chunks(k_fourier_cfactor, a, &CFourierFactorArgs::set0, nset, gx, XINV_CFAC_WG, st);
}

void xinv_launch_fourier_csubst(CFourierSubstArgs a, int64_t nbatch, hipStream_t st)
{
    const unsigned gx = (unsigned)((a.K + XINV_CSUB_WG - 1) / XINV_CSUB_WG);
    xinv_launch_chunks(k_fourier_csubst, a, &CFourierSubstArgs::member0, nbatch, gx, XINV_CSUB_WG, st);
}

void xinv_launch_fourier_gcheck(CFourierCheckArgs a, int64_t nbatch, hipStream_t st)
{
    xinv_launch_chunks(k_fourier_gcheck, a, &CFourierCheckArgs::member0, nbatch, (unsigned)a.yc, XINV_GCHK_WG, st);
}
