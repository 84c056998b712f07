// The streaming kernels, k_results and k_dispatch_order: one translation unit (launch.hpp)
#include "kernels_stream.hpp"
#include "kernels_order.hpp"
#include "launch.hpp"

namespace vxh {

// one time step of the streamed robots: five kernels when a robot is in a fluid, else three
void launch_stream_round(const DBatch& B, bool any_fluid, int reb_blocks, const int* reb_robot, const int* reb_i0, hipStream_t s, long long cap)
{
    const int nb_b = (3 * B.nv + 255) / 256, nb_v = (B.nv + 255) / 256;
    hipLaunchKernelGGL(k_step_begin, dim3(B.n_robots), dim3(256), 0, s, B, cap, 1);
    if (any_fluid) {
        hipLaunchKernelGGL(k_mesh_vertices, dim3((B.n_mv + 255) / 256), dim3(256), 0, s, B);
        hipLaunchKernelGGL(k_facets, dim3((B.n_facet + 255) / 256), dim3(256), 0, s, B);
    }
    hipLaunchKernelGGL(k_bonds, dim3(nb_b + reb_blocks), dim3(256), 0, s, B, nb_b, reb_robot, reb_i0);
    hipLaunchKernelGGL(k_voxels, dim3(nb_v), dim3(256), 0, s, B);
}

void launch_stream_finish(const DBatch& B, hipStream_t s, long long cap)
{
    hipLaunchKernelGGL(k_step_begin, dim3(B.n_robots), dim3(256), 0, s, B, cap, 0);   // finish the last step
}

void launch_results(const DBatch& B, int n_robots, DResult* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_results, dim3(n_robots), dim3(256), 0, s, B, out);
}

void launch_dispatch_order(const DispatchCost* cost, int count, int len, int* perm, hipStream_t s)
{
    hipLaunchKernelGGL(k_dispatch_order, dim3((count + VXH_ORDER_BLOCK - 1) / VXH_ORDER_BLOCK), dim3(VXH_ORDER_BLOCK), 0, s, cost, count, len, perm);
}

}  // namespace vxh
