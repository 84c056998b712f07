// k_shape_results: one translation unit (launch.hpp)
#include "kernels_shape.hpp"
#include "launch.hpp"

namespace vxh {

void launch_shape_results(const DBatch& B, const DShape& Q, int count, size_t lds, hipStream_t s)
{
    static size_t granted[64] = {};
    grant_dynamic_lds((const void*)k_shape_results, granted, lds);
    hipLaunchKernelGGL(k_shape_results, dim3(count), dim3(VXH_SHAPE_THREADS), lds, s, B, Q);
}

}  // namespace vxh
