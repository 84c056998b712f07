// k_shape_curvature<HBM>: one translation unit (launch.hpp), built without contraction like the shape kernels' (Makefile)
#include "kernels_curvature.hpp"
#include "launch.hpp"

namespace vxh {

static_assert(VXH_SHAPE_LARGE_MAX_VERT <= 0xFFFF && VXH_CURV_CHUNK == 64 && VXH_CURV_THREADS % VXH_CURV_CHUNK == 0, "16-bit vertex ids; a chunk is a wavefront");
static_assert((size_t)24 * VXH_CURV_LDS_MAX_VERT + VXH_CURV_STATIC_LDS <= VXH_SHAPE_CU_LDS, "the points of the largest LDS robot fit the CU");

void launch_shape_curvature(const DBatch& B, const DCurv& C, int count, size_t lds, hipStream_t s)
{
    static size_t granted[64] = {};
    if (lds + VXH_CURV_STATIC_LDS > VXH_SHAPE_CU_LDS) throw std::logic_error("k_shape_curvature: LDS request above the CU's");
    grant_dynamic_lds((const void*)k_shape_curvature<false>, granted, lds);
    hipLaunchKernelGGL(k_shape_curvature<false>, dim3(count), dim3(VXH_CURV_THREADS), lds, s, B, C);
}

void launch_shape_curvature_hbm(const DBatch& B, const DCurv& C, int count, hipStream_t s)
{
    hipLaunchKernelGGL(k_shape_curvature<true>, dim3(count), dim3(VXH_CURV_THREADS), 0, s, B, C);
}

}  // namespace vxh
