// xinv_tu_pipe2d.hip -- instantiations of k_pipe2d (wave-pipelined four-sweep pass, one tile per 256-thread workgroup:
// xinv_pipe2d.h) for ONE model (-DXINV_TU_MODEL=0 standard form, um = 3: A and C per row; 1 general form, um = 0x1f: A C D
// E F per row; each once more with -DXINV_TU_SEAM=1: the odd-xc periodic seam variants -- unaligned strips; 2: both forms
// in contracted arithmetic, XINV_FLAG_FMA).  No variant for coefficient arrays that vary along x: measured slower than
// k_fused2d (plan5_sweeps).
#include "xinv_dispatch.h"

#ifndef XINV_TU_SEAM
#define XINV_TU_SEAM 0
#endif
constexpr bool SEAM = XINV_TU_SEAM != 0;

template <class M, unsigned UM, bool FR>
static KernelRef pipe_al_ext(bool al, bool ext)
{
    constexpr unsigned T = 64 * XINV_PIPE_P;
    if constexpr (!SEAM) {
        if (al) return ext ? kernel_ref(k_pipe2d<M, UM, FR, true, true, SEAM>, T) : kernel_ref(k_pipe2d<M, UM, FR, true, false, SEAM>, T);
    } else if (al) return KernelRef{};
    return ext ? kernel_ref(k_pipe2d<M, UM, FR, false, true, SEAM>, T) : kernel_ref(k_pipe2d<M, UM, FR, false, false, SEAM>, T);
}

// pipe_fr: the forcing row rides the LDS ring with S
template <class M, unsigned UM>
static KernelRef pipe_m(const SweepVariant &v)
{
    if (v.um != UM) return KernelRef{};
    return v.pipe_fr ? pipe_al_ext<M, UM, true>(v.al, v.ext) : pipe_al_ext<M, UM, false>(v.al, v.ext);
}

template <> XINV_HIDDEN KernelRef xinv_kernel_pipe2d<XINV_TU_MODEL, SEAM>(const SweepVariant &v)
{
#if XINV_TU_MODEL == 2       /* PIPE2D_FMA */
    return v.kind == KIND_GEN2D ? pipe_m<FusedGen2DF, 0x1fu>(v) : pipe_m<FusedStd2DF, 3u>(v);
#elif XINV_TU_MODEL == 0     /* PIPE2D_STD */
    return pipe_m<FusedStd2D, 3u>(v);
#else                        /* PIPE2D_GEN */
    return pipe_m<FusedGen2D, 0x1fu>(v);
#endif
}
