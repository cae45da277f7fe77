// xinv_tu_fused2d.hip -- instantiations of k_fused2d for ONE model (compiled three times:
// -DXINV_TU_MODEL=0 standard form, 1 general form, 2 standard "test" form; and each once more with -DXINV_TU_SEAM=1:
// the odd-xc periodic seam variants, unaligned strips only; 3 / 4: the contracted-arithmetic models of XINV_FLAG_FMA,
// per-row-coefficient variants only; 5: the general form with the point-factor stream).
#include <type_traits>
#include "xinv_dispatch.h"

#ifndef XINV_TU_SEAM
#define XINV_TU_SEAM 0
#endif
constexpr bool SEAM = XINV_TU_SEAM != 0;

// sweeps per pass
template <class M, bool AL, unsigned UM, bool EXT>
static KernelRef fused_k(int K)
{
    switch (K) {
    case 1: return kernel_ref(k_fused2d<M, 1, AL, UM, EXT, 0, SEAM>, 256);
    case 2: return kernel_ref(k_fused2d<M, 2, AL, UM, EXT, 0, SEAM>, 256);
    case 3: return kernel_ref(k_fused2d<M, 3, AL, UM, EXT, 0, SEAM>, 256);
    // four sweeps per pass: only the standard form with per-row A and C keeps two wavefronts per SIMD at that window
    // depth (249 VGPRs; the general form does not gain)
    case 4:
        if constexpr (std::is_base_of<FusedStd2D, M>::value) return kernel_ref(k_fused2d<M, 4, AL, UM, EXT, 0, SEAM>, 256);
        break;
    default: break;
    }
    return KernelRef{};
}

// the masks of per-row streams a model is instantiated for
template <class M, bool AL, bool EXT>
static KernelRef fused_um(unsigned um, int K)
{
    if constexpr (ModelFma<M>::value) {                  // contracted arithmetic: the per-row-coefficient variants only
        constexpr unsigned UMF = std::is_base_of<FusedStd2D, M>::value ? 3u : 0x1fu;
        return um == UMF ? fused_k<M, AL, UMF, EXT>(K) : KernelRef{};
    } else if constexpr (std::is_same<M, FusedGen2DQA>::value) {   // (C read out of A: bit 1 set, nothing of C loaded)
        if (um == 0x1eu) return fused_k<M, AL, 0x1eu, EXT>(K);
        if (um == 0x02u) return fused_k<M, AL, 0x02u, EXT>(K);
        return KernelRef{};
    } else {
        if constexpr (std::is_same<M, FusedStd2D>::value) {
            if (um == 3u) return fused_k<M, AL, 3u, EXT>(K);
        } else if constexpr (std::is_same<M, FusedStd2DT>::value) {
            if (um == 7u) return fused_k<M, AL, 7u, EXT>(K);
        } else if constexpr (ModelPQ<M>::value) {        // (A, C varying along x: D, E, F per row, or nothing)
            if (um == 0x1cu) return fused_k<M, AL, 0x1cu, EXT>(K);
            if (um != 0u) return KernelRef{};
        } else {
            if (um == 0x1fu) return fused_k<M, AL, 0x1fu, EXT>(K);
            if (um == 0x1cu) return fused_k<M, AL, 0x1cu, EXT>(K);
        }
        return fused_k<M, AL, 0u, EXT>(K);               // (every stream a vector)
    }
}

template <class M>
static KernelRef fused_m(const SweepVariant &v)
{
    if constexpr (!SEAM) {
        if (v.al) return v.ext ? fused_um<M, true, true>(v.um, v.K) : fused_um<M, true, false>(v.um, v.K);
    } else if (v.al) return KernelRef{};
    return v.ext ? fused_um<M, false, true>(v.um, v.K) : fused_um<M, false, false>(v.um, v.K);
}

template <> XINV_HIDDEN KernelRef xinv_kernel_fused2d<XINV_TU_MODEL, SEAM>(const SweepVariant &v)
{
#if XINV_TU_MODEL == 0       /* FUSED2D_STD */
    return fused_m<FusedStd2D>(v);
#elif XINV_TU_MODEL == 1     /* FUSED2D_GEN */
    return fused_m<FusedGen2D>(v);
#elif XINV_TU_MODEL == 2     /* FUSED2D_STD2DT */
    return fused_m<FusedStd2DT>(v);
#elif XINV_TU_MODEL == 3     /* FUSED2D_STDF */
    return fused_m<FusedStd2DF>(v);
#elif XINV_TU_MODEL == 4     /* FUSED2D_GENF */
    return fused_m<FusedGen2DF>(v);
#else                        /* FUSED2D_GENQ */
    return (v.um & 2u) ? fused_m<FusedGen2DQA>(v) : fused_m<FusedGen2DQ>(v);
#endif
}
