// Host side of a batch, plain C++ (no HIP): which kernel steps which robot, the host tables of a batch (assemble_batch) and how its
// robots are tiled, packed into launches and grouped (plan_launches).  Engine::prepare() (engine.hip) uploads what these return.
#pragma once
#include <cstddef>
#include <vector>

#include "device_types.hpp"
#include "engine.hpp"      // Options
#include "model.hpp"

namespace vxh {

// Which kernel steps which robot: functions of the robot alone (and of the engine's options), never of the batch.
// Wide kernel (kernels_wide.hpp; robots of up to WIDE_BLOCK voxels and 1023 bonds): its bond records share their LDS region with
// the scratch of the whole-robot passes (12 * BLOCK doubles, then the mesh vertices of a robot in a fluid); the record that stays
// zero lies behind both.
constexpr int WIDE_BLOCK = 512;
struct WideLayout { int zidx = 0, region = 0; };
WideLayout wide_layout(const RobotModel& M, int variant);
bool wide_listed(const RobotModel& M, int variant, const Options& opt);
// workgroup size of the resident kernel for a robot of n voxels: its size class
int resident_block(int n);
// Resident kernel (kernels_fused.hpp) or wide kernel, one workgroup per robot: the variant follows from the robot's size, fluid, and the
// LDS need of its own tables.  block == 0: neither takes the robot.
struct FusedVariant { int block = 0, nacc = 0, fluid = 0, tabg = 0, wide = 0, two_tiles = 0; size_t lds = 0; };
FusedVariant fused_variant(const RobotModel& M, int variant, const Options& opt);

// Every host table of a batch, in the layout the kernels read (DBatch, device_types.hpp, describes each), and the scalars that go with them.
struct HostBatch {
    int nv = 0, ns = 0;                        // padded voxel slots (a multiple of 64 per robot) / surface voxels of colliding robots
    std::vector<DRobot> robot;
    std::vector<DRobotState> rstate;
    std::vector<int> vox_begin, surf_begin;    // per robot, global slot of voxel 0 / of its first surface voxel
    std::vector<int> trace_begin, trace_cap;   // per robot, entries of DBatch::trace
    int total_trace = 0;
    // robots with <NormDistByVol>: volumes of those points (DBatch::trace_vol), after-life [0] and frozen [1] traces (DBatch::xtrace); every
    // other robot has empty ranges
    std::vector<int> vol_begin, xt_begin[2], xt_cap[2];
    int total_vol = 0, total_xtrace = 0;
    long long max_planned = 0;
    int max_nvox = 0;                          // largest robot of the batch
    std::vector<DVoxClass> vtab;
    std::vector<DBondClass> btab;
    std::vector<int> wave_robot, nbr, surf, surf_code, surf_ord;
    std::vector<unsigned long long> excl;
    std::vector<unsigned short> vclass;
    std::vector<short> bclass;
    std::vector<int> sched_off, bsched;        // bond schedules of the resident kernel: [3][block] per robot, block = the workgroup size of the robot's size class
    std::vector<int> wl_off, wlist, wgather;
    std::vector<float> amp_damp, dev;
    std::vector<double> act_sb, act_cb;
    std::vector<double> px, py, pz, sc, qw;
    std::vector<unsigned char> small;
    bool any_dev = false, any_mesh = false, any_fluid = false;
    // land_water robots: deformable surface mesh (fluid drag, RobotVolume tags)
    int total_mv = 0, total_facet = 0;
    std::vector<int> mv_begin, facet_begin;
    std::vector<int> vert_pack;
    // robots in a fluid: the same mesh with global indices for the streaming kernels (robots that do not fit the resident one)
    std::vector<int> vert_vox, vert_robot;
    std::vector<double> vert_v0;
    std::vector<int> facet_vox, facet_vert, facet_first, facet_robot;
    std::vector<unsigned char> facet_count;
    // offsets of the per-robot pieces of the shared tables
    std::vector<int> vtab_off, btab_off;
    std::vector<long long> excl_off, col_off;
    std::vector<int> col_cap;
    std::vector<int> img_idx;                  // slot of the robot's saved contact-row image (DBatch::rimg_*), colliding robots of up to 1024 voxels
    long long col_total = 0;
};
// device_mem: the device's total memory in bytes (the contact-row budget is a third of it); 0 = unknown, rows are not cut
HostBatch assemble_batch(const std::vector<RobotModel>& robots, int variant, const Options& opt, size_t device_mem);

// A launch group of the resident / wide kernels: the robots of one kernel variant
struct GroupPlan {
    int block = 0, nacc = 0, fluid = 0, tabg = 0;   // template arguments of k_robot_steps
    int wide = 0;                     // 1: k_robot_wide<block, fluid, tabg> (kernels_wide.hpp)
    int two_tiles = 0;                // wide kernel: a second pose tile in LDS (two barriers per step instead of three)
    int count = 0;
    bool order_use = false;           // short launches are dispatched "robots due for a broad-phase run first" (kernels_fused.hpp fused_dispatch_slot),
                                      // long ones by measured cost, longest first (dispatch_order.hpp): k_robot_steps groups with colliding robots
    size_t lds = 0;                   // dynamic LDS bytes
    std::vector<int> robots;
};
// A launch of the tiled kernel: all tiles of its robots, no more than the chip keeps resident
struct TileLaunchPlan {
    int tabg = 0, mesh = 0, count = 0;   // template arguments of k_tile_steps (mesh: land_water robots, whose strains are part of the state)
    int small = 0;                    // ... and SMALL: every tile of the launch within VXH_TILE_S_* (compile-time LDS strides)
    size_t lds = 0;
    std::vector<int> tile_ids, robots;
};
struct LaunchPlan {
    // tiled path: the robots cut into tiles, packed into launches that fit the chip (all tiles of a robot in one launch)
    std::vector<DTile> tiles;
    std::vector<int> tile_vox, tile_bond, tile_bcls, tile_bslot, xslot;
    std::vector<int> tile_of, tile_lidx;
    int nx_total = 0;
    bool any_fluid_tiles = false;
    // fluid tiles: their parts of the drag mesh (DBatch::tile_mvert [8][n_tmv], tile_mv0 [3][n_tmv], tile_facet [4][n_tf], ...)
    int n_tmv = 0, n_tf = 0;
    std::vector<int> tile_mvert, tile_facet, tile_ffirst, tile_mvox;
    std::vector<double> tile_mv0;
    std::vector<unsigned char> tile_fcount;
    std::vector<TileLaunchPlan> tile_launches;
    std::vector<unsigned char> robot_tiled;   // per robot
    std::vector<int> robot_tiles;             // per robot: number of tiles (0 = not tiled)
    // fused path: launch groups by kernel variant; inside a group the longest-running robots first
    std::vector<GroupPlan> groups;
    // masks for DBatch::streamed: every robot / the robots outside the launch groups (tiled robots in neither)
    std::vector<unsigned char> streamed_all, streamed_rest;
    int n_rest = 0, n_all = 0;            // robots (with voxels) that only the streaming kernels can step / that they step with fused = 0
    std::vector<int> reb_robot, reb_i0;   // streaming path: one rebuild block per 256 surface voxels of every colliding robot
};
LaunchPlan plan_launches(const std::vector<RobotModel>& robots, const HostBatch& H, int variant, const Options& opt, bool tiling_allowed, int n_cu);

// The dominant kernel of one call (vxh_counters::dominant_*): the unit -- the tiled launches, one launch group, the streaming kernels
// next to the groups (REST), or the streaming kernels alone (STREAMED: a call without launch groups) -- that processed most voxel-steps.
struct DominantKernel {
    enum Unit { TILES, GROUP, REST, STREAMED } unit = STREAMED;
    int group = -1;                   // GROUP: which
    int block = 0, robots = 0;        // block: 1 = k_tile_steps, 0 = the streaming kernels; a group: its workgroup size, + 1 for the wide kernel
    long long launches = 0;
    double alg_bytes = 0, voxel_steps = 0;
};
// steps: what each robot took in this call; fused, tiled, streaming: the paths the call used; todo: its step rounds
DominantKernel dominant_kernel(const std::vector<RobotModel>& robots, const std::vector<int>& steps, const std::vector<const GroupPlan*>& groups,
                               const std::vector<unsigned char>& robot_tiled, bool fused, bool tiled, bool streaming, int n_rest, long long todo,
                               const std::vector<long long>& group_launches, long long tile_launch_count);

}  // namespace vxh
