// k_robot_wide: one translation unit (launch.hpp)
#include <cstdio>
#include <cstdlib>

#include "kernels_wide.hpp"
#include "launch.hpp"

namespace vxh {

template <int BLOCK, bool MESH, bool TABG, bool STATS = false>
static void launch_wide(const DBatch& B, const int* list, int count, size_t lds, hipStream_t s, long long cap, int iters, int two_tiles)
{
    static size_t granted[64] = {};
    grant_dynamic_lds((const void*)k_robot_wide<BLOCK, MESH, TABG, STATS>, granted, lds);
    // VXH_PROF_WIDE: the launch as the device will place it -- workgroups of this instance a CU holds at this LDS size (what the small
    // instances exist for), as the runtime's occupancy query answers it, one line per launch on stderr
    if (std::getenv("VXH_PROF_WIDE")) {
        int per_cu = 0;
        hip_check(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_robot_wide<BLOCK, MESH, TABG, STATS>, BLOCK, lds), "hipOccupancyMaxActiveBlocksPerMultiprocessor(k_robot_wide)");
        std::fprintf(stderr, "vxhip: wide launch block=%d mesh=%d tabg=%d stats=%d two_tiles=%d: %d robots, %zu B of LDS, %d workgroups per CU\n", BLOCK, (int)MESH, (int)TABG,
                     (int)STATS, two_tiles, count, lds, per_cu);
    }
    hipLaunchKernelGGL((k_robot_wide<BLOCK, MESH, TABG, STATS>), dim3(count), dim3(BLOCK), lds, s, B, B.robot, list, cap, iters, (int)(lds / 8), two_tiles);
}

template <int BLOCK>
static void launch_wide_plain(const DBatch& B, bool mesh, bool tabg, const int* list, int count, size_t lds, hipStream_t s, long long cap, int iters, int two_tiles)
{
    if (mesh) { if (tabg) launch_wide<BLOCK, true, true>(B, list, count, lds, s, cap, iters, two_tiles); else launch_wide<BLOCK, true, false>(B, list, count, lds, s, cap, iters, two_tiles); }
    else { if (tabg) launch_wide<BLOCK, false, true>(B, list, count, lds, s, cap, iters, two_tiles); else launch_wide<BLOCK, false, false>(B, list, count, lds, s, cap, iters, two_tiles); }
}

// block: 512, or VXH_WIDE_SMALL_BLOCK for a group of small robots (option wide_small; no STATS instances)
// stats: the group's robots are under StopConditionType 4-7 (_voxcad only; lds includes the VXH_STAT_LDS doubles of the pass)
void launch_wide_group(const DBatch& B, int block, bool mesh, bool tabg, bool stats, const int* list, int count, size_t lds, hipStream_t s, long long cap, int iters, int two_tiles)
{
    if (block != 512 && block != VXH_WIDE_SMALL_BLOCK) throw std::runtime_error("k_robot_wide: no instance of " + std::to_string(block) + " threads");
    if (stats) {
        if (mesh || (B.stat_lo == 0 && B.stat_hi == 0)) throw std::runtime_error("k_robot_wide: a STATS group without history rings or with a surface mesh");
        if (block != 512) throw std::runtime_error("k_robot_wide: no STATS instance of the small block");
        if (tabg) launch_wide<512, false, true, true>(B, list, count, lds, s, cap, iters, two_tiles); else launch_wide<512, false, false, true>(B, list, count, lds, s, cap, iters, two_tiles);
    }
    else if (block == VXH_WIDE_SMALL_BLOCK) launch_wide_plain<VXH_WIDE_SMALL_BLOCK>(B, mesh, tabg, list, count, lds, s, cap, iters, two_tiles);
    else launch_wide_plain<512>(B, mesh, tabg, list, count, lds, s, cap, iters, two_tiles);
}

}  // namespace vxh
