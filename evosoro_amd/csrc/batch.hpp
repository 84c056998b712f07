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
// Option wide_small: a wide-listed robot of up to VXH_WIDE_SMALL_VOX voxels that is not under StopConditionType 4-7 and whose LDS, laid out with
// voxel planes of that many slots and INCLUDING its contact rows, fits the share of a CU's LDS that VXH_WIDE_SMALL_PER_CU workgroups leave
// each other takes the VXH_WIDE_SMALL_BLOCK-thread instances (wide_small: taken, and then its TABG choice, second pose tile and LDS bytes);
// its record region follows from the smaller scratch (wide_layout).  Every other robot keeps the 512-thread instances and their layout.
constexpr int WIDE_BLOCK = 512;
struct WideLayout { int zidx = 0, region = 0; };
struct WideSmall { int taken = 0, tabg = 0, two_tiles = 0; size_t lds = 0; };
WideLayout wide_layout(const RobotModel& M, int variant, const Options& opt);
bool wide_listed(const RobotModel& M, int variant, const Options& opt);
WideSmall wide_small(const RobotModel& M, int variant, const Options& opt);
// workgroup size of the resident kernel for a robot of n voxels: its size class
int resident_block(int n);
// Resident kernel (kernels_fused.hpp) or wide kernel, one workgroup per robot: the variant follows from the robot's size, fluid, and the
// LDS need of its own tables.  block == 0: neither takes the robot.
// stats: the robot is under StopConditionType 4-7 and takes the STATS instance of its kernel (stat_rules below) -- the same kernel choice as
// under any other rule, with VXH_STAT_LDS doubles more of dynamic LDS (the contact rows give them up where the layout is full).
struct FusedVariant { int block = 0, nacc = 0, fluid = 0, tabg = 0, wide = 0, two_tiles = 0, stats = 0; size_t lds = 0; };
// the energy and motion stop rules (CVX_Sim::StopConditionMet, VX_Sim.cpp:1427-1460), which need whole-robot statistics after every step
inline bool stat_rules(const RobotModel& M) { return M.vxa.stop_type >= 4 && M.vxa.stop_type <= 7; }
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
    // engine option device_shape, land_water robots of up to VXH_SHAPE_MAX_VERT mesh vertices: what k_shape_results reads beside the tables above
    // (DShape, device_types.hpp) -- per mesh vertex its voxels in the host's order, and the robots it is launched for.  Empty without the option.
    std::vector<int> shape_vert, shape_list;
    int shape_max_nmv = 0;                     // most mesh vertices of a robot of shape_list (sizes the launch's LDS)
    // ... and option device_shape_large: the robots above that cap, up to VXH_SHAPE_LARGE_MAX_VERT vertices, that k_shape_results_large takes
    // (shape_vert is filled for them too), per list entry the first double of its 6 nmv of the point table, the table's size in
    // doubles, and the most LDS a robot of the list needs (shape_large_lds_bytes is not monotonic in nmv: the launch takes the maximum)
    std::vector<int> shape_large_list;
    std::vector<long long> shape_large_off;
    long long shape_large_points = 0;
    size_t shape_large_lds = 0;
    // option device_curvature (with device_shape): what k_shape_curvature reads beside shape_vert (DCurv, device_types.hpp).  Its lists are its own:
    // every land_water robot that has a corner table, by nmv alone into the LDS instance's list or the HBM instance's.  Per robot the
    // first record and the chunks of its table (0: not listed) and, for the HBM instance, the first double of its points.
    std::vector<unsigned long long> curv_rec;
    std::vector<long long> curv_rec_begin, curv_pts_begin;
    std::vector<int> curv_n_chunk, curv_list, curv_hbm_list;
    long long curv_points = 0;                 // doubles of the HBM instance's point table
    int curv_max_nmv = 0;                      // most mesh vertices of a robot of curv_list (sizes the launch's LDS)
    // offsets of the per-robot pieces of the shared tables
    std::vector<int> vtab_off, btab_off;
    std::vector<long long> excl_off, col_off;
    std::vector<int> col_cap;
    std::vector<int> img_idx;                  // slot of the robot's saved contact-row image (DBatch::rimg_*), colliding robots of up to 1024 voxels
    long long col_total = 0;
    // robots under StopConditionType 4-7: per robot its number among them or -1 (DStat::stat_slot; the history rings are sized by n_stat),
    // and per row of btab the three strain-energy factors (DStat::bond_energy).  Both empty when the batch holds no such robot.
    std::vector<int> stat_slot;
    std::vector<double> bond_energy;
    int n_stat = 0;
};
// The corner table of a robot's surface mesh for k_shape_curvature (device_types.hpp describes the records): walk the facets in order, emit
// (at, p, q) for corner a, for b if b != a, for c if c != a && c != b (mesh_angle_excess: a vertex a facet lists twice counts once, in its
// first role); group by `at`, facet order kept; lay the groups out in chunks of VXH_CURV_CHUNK records, padded so that none straddles a
// chunk.  Appends to `rec` and returns the number of chunks; 0 (nothing appended): the robot has no table -- no mesh, more than
// VXH_SHAPE_LARGE_MAX_VERT vertices, a vertex of no corner or of more than VXH_CURV_CHUNK.
int curvature_corner_table(const RobotModel& M, std::vector<unsigned long long>& rec);
// device_mem: the device's total memory in bytes (the contact-row budget is a third of it); 0 = unknown, rows are not cut
HostBatch assemble_batch(const std::vector<RobotModel>& robots, int variant, const Options& opt, size_t device_mem);

// A launch group of the resident / wide kernels: the robots of one kernel variant
struct GroupPlan {
    int block = 0, nacc = 0, fluid = 0, tabg = 0;   // template arguments of k_robot_steps
    int wide = 0;                     // 1: k_robot_wide<block, fluid, tabg> (kernels_wide.hpp)
    int two_tiles = 0;                // wide kernel: a second pose tile in LDS (two barriers per step instead of three)
    int stats = 0;                    // the STATS instances: robots under StopConditionType 4-7 (never measured for the dispatch order)
    int count = 0;
    bool order_use = false;           // short launches are dispatched "robots due for a broad-phase run first" (kernels_fused.hpp fused_dispatch_slot),
                                      // long ones by measured cost, longest first (dispatch_order.hpp): k_robot_steps groups with colliding robots
    size_t lds = 0;                   // dynamic LDS bytes
    std::vector<int> robots;
};
// A launch of the tiled kernel: all tiles of its robots, no more than the chip keeps resident
struct TileLaunchPlan {
    int tabg = 0, mesh = 0, count = 0;   // template arguments of k_tile_steps (mesh: land_water robots, whose strains are part of the state)
    int cls = 0;                      // ... and its size class, VXH_TILE_CLASS_*: SMALL / MEDIUM = every tile of the launch within VXH_TILE_S_* /
                                      // VXH_TILE_M_* (compile-time LDS strides; MEDIUM only with the option tile_medium)
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
