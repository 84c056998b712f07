// k_shape_results, k_shape_results_large: one translation unit (launch.hpp)
#include "kernels_shape_large.hpp"
#include "launch.hpp"

namespace vxh {

void launch_shape_results(const DBatch& B, const DShape& Q, int count, size_t lds, hipStream_t s)
{
    static size_t granted[64] = {};
    grant_dynamic_lds((const void*)k_shape_results, granted, lds);
    hipLaunchKernelGGL(k_shape_results, dim3(count), dim3(VXH_SHAPE_THREADS), lds, s, B, Q);
}

static_assert(sizeof(ShapeLargeShared) + sizeof(unsigned long long) * SHAPE_LARGE_NW <= VXH_SHAPE_LARGE_STATIC_LDS, "static LDS of k_shape_results_large");
static_assert(VXH_SHAPE_LARGE_MAX_VERT < SHAPE_NONE && VXH_SHAPE_CU_LDS / 46 < SHAPE_NONE, "vertex and face ids are 16 bits");

void launch_shape_results_large(const DBatch& B, const DShape& Q, int count, size_t lds, hipStream_t s)
{
    static size_t granted[64] = {};
    if (lds + VXH_SHAPE_LARGE_STATIC_LDS > VXH_SHAPE_CU_LDS) throw std::logic_error("k_shape_results_large: LDS request above the CU's");
    grant_dynamic_lds((const void*)k_shape_results_large, granted, lds);
    hipLaunchKernelGGL(k_shape_results_large, dim3(count), dim3(VXH_SHAPE_LARGE_THREADS), lds, s, B, Q);
}

}  // namespace vxh
