// Host-side launch entry points of every kernel.  Each kernel family is its own translation unit (launch_fused_*.hip,
// launch_wide.hip, launch_tiled.hip, launch_stream.hip, launch_shape.hip, launch_curvature.hip) so that the Makefile compiles them side by side and a change to one family
// recompiles that family only; engine.hip (device memory, the call loop, graph capture) compiles no kernel and sees these declarations.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <stdexcept>
#include <string>
#include "device_types.hpp"
#include "dispatch_order.hpp"

namespace vxh {

inline void hip_check(hipError_t e, const char* what)
{
    if (e != hipSuccess) throw std::runtime_error(std::string("HIP: ") + what + ": " + hipGetErrorString(e));
}

// The opt-in to more than 64 KB of dynamic LDS is per function AND per device (engines on several devices and threads may live in
// one process): the largest size granted on each device is remembered per kernel, under a lock.
inline void grant_dynamic_lds(const void* kernel, size_t (&granted)[64], size_t lds)
{
    static std::mutex lock;
    int dev = 0;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    std::lock_guard<std::mutex> hold(lock);
    if (dev < 0 || dev >= 64 || lds > granted[dev]) {
        hip_check(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), "hipFuncSetAttribute(dynamic LDS)");
        if (dev >= 0 && dev < 64) granted[dev] = lds;
    }
}

// k_robot_steps<block, nacc, FLUID, TABG, COST> (kernels_fused.hpp): block in {256, 512, 768, 1024}; land robots / land_water robots;
// cost: the instances that measure what their robots cost (order_in: the launch's permutation with the cost words behind it, never null)
void launch_fused_land(const DBatch& B, int block, bool tabg, const int* list, int count, size_t lds, hipStream_t s, long long cap, int iters,
                       const unsigned long long* order_in, unsigned long long* order_out, bool cost, bool stats = false);
void launch_fused_mesh(const DBatch& B, int block, bool tabg, const int* list, int count, size_t lds, hipStream_t s, long long cap, int iters,
                       const unsigned long long* order_in, unsigned long long* order_out, bool cost);
// k_robot_wide<block, MESH, TABG, STATS> (kernels_wide.hpp); block: 512, or VXH_WIDE_SMALL_BLOCK for a group of small robots (option wide_small);
// stats (with launch_fused_land too): the STATS instances, for groups of robots under StopConditionType 4-7 (512 only)
void launch_wide_group(const DBatch& B, int block, bool mesh, bool tabg, bool stats, const int* list, int count, size_t lds, hipStream_t s, long long cap, int iters, int two_tiles);
// k_tile_steps<TABG, MESH, FLUID, CLS> (kernels_tiled.hpp); mesh_kind: 0 = _voxcad, 1 = land_water robot on land, 2 = in a fluid
// cls: VXH_TILE_CLASS_* (device_types.hpp) -- SMALL / MEDIUM: every tile of the launch within VXH_TILE_S_* / VXH_TILE_M_*: the instances with
// compile-time LDS strides
void launch_tile_group(const DBatch& B, bool tabg, int mesh_kind, int cls, const int* list, int count, size_t lds, hipStream_t s, long long cap, int iters, unsigned gen);
// threads of a tile's workgroup (the host sizes launches and LDS with the kernel's own constants)
int tile_threads();
// the streaming kernels (kernels_stream.hpp).  One time step of the streamed robots: k_step_begin, k_mesh_vertices and k_facets when any robot is
// in a fluid, k_bonds (its blocks + reb_blocks broad-phase blocks: reb_robot / reb_i0), k_voxels; stats: a streamed robot is under
// StopConditionType 4-7 -- k_step_begin_stats and k_bonds_stats in their places, k_stream_stats behind k_voxels ...
void launch_stream_round(const DBatch& B, bool any_fluid, int reb_blocks, const int* reb_robot, const int* reb_i0, hipStream_t s, long long cap, bool stats);
// ... and the k_step_begin that finishes the last step of a call
void launch_stream_finish(const DBatch& B, hipStream_t s, long long cap, bool stats);
// k_results: one DResult per robot
void launch_results(const DBatch& B, int n_robots, DResult* out, hipStream_t s);
// k_shape_results (kernels_shape.hpp): one workgroup per robot of Q.list (count of them); lds: shape_lds_bytes of the largest
void launch_shape_results(const DBatch& B, const DShape& Q, int count, size_t lds, hipStream_t s);
// k_shape_results_large (kernels_shape_large.hpp): one workgroup per robot of Q.large_list; lds: the most shape_large_lds_bytes of them
void launch_shape_results_large(const DBatch& B, const DShape& Q, int count, size_t lds, hipStream_t s);
// k_shape_curvature<false> (kernels_curvature.hpp): one workgroup per robot of C.list; lds: curv_lds_bytes of the largest.  <true>: the robots
// of C.hbm_list, points in C.pts
void launch_shape_curvature(const DBatch& B, const DCurv& C, int count, size_t lds, hipStream_t s);
void launch_shape_curvature_hbm(const DBatch& B, const DCurv& C, int count, hipStream_t s);
// k_dispatch_order (kernels_order.hpp): perm = the `count` list entries by descending expected cost of a launch of `len` steps (0: the list order)
void launch_dispatch_order(const DispatchCost* cost, int count, int len, int* perm, hipStream_t s);

}  // namespace vxh
