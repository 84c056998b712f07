// Host-only check of the import pipeline (import.hpp), batch assembly, launch planning and the dominant-kernel choice (batch.hpp): no HIP,
// built with the plain C++ compiler (make batch_check), so it also runs under the host sanitizers.  Exit status 0 = all consistent.
//   batch_check <variant 0|1> <CUs> robot.vxa...    all robots form ONE batch, assembled and planned under several option sets; every table
//                                                  is then unpacked and compared with the robots' models
//   batch_check --arrays <variant 0|1> robot.vxa... every file's lattice and layers handed over as arrays (models_from_arrays) must give the
//                                                  batch the file gives, value for value; and what that route must refuse
//   batch_check --dominant                         dominant_kernel on a table of hand-made calls, one per branch of its rule
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <type_traits>
#include <vector>

#include "batch.hpp"
#include "import.hpp"

using namespace vxh;

namespace {

const char* g_set = "";
[[noreturn]] void fail(const char* fmt, ...)
{
    std::fprintf(stderr, "batch_check [%s]: ", g_set);
    va_list ap; va_start(ap, fmt); std::vfprintf(stderr, fmt, ap); va_end(ap);
    std::fprintf(stderr, "\n");
    std::exit(1);
}
#define CHECK(cond, ...) do { if (!(cond)) fail(__VA_ARGS__); } while (0)

typedef std::vector<RobotModel> Robots;

// every robot in exactly one of: a launch group, a tile launch, the `rest` mask, empty; the masks' counts; LDS and CU bounds
void check_partition(const Robots& robots, const LaunchPlan& P, int n_cu)
{
    const int nr = (int)robots.size();
    std::vector<int> in_group(nr, 0), in_tiles(nr, 0);
    for (const GroupPlan& g : P.groups) {
        CHECK(g.count == (int)g.robots.size() && g.count > 0, "group count %d against %zu robots", g.count, g.robots.size());
        CHECK(g.lds <= (size_t)160 * 1024 - (size_t)(g.wide ? (int)VXH_WIDE_STATIC_LDS : (int)VXH_FUSED_STATIC_LDS), "group (block %d) asks for %zu B of LDS", g.block, g.lds);
        for (int r : g.robots) { CHECK(r >= 0 && r < nr, "group lists robot %d", r); ++in_group[r]; }
    }
    for (const TileLaunchPlan& L : P.tile_launches) {
        CHECK(L.count == (int)L.tile_ids.size() && L.count > 0 && L.count <= n_cu, "tile launch of %d tiles (%zu ids) on %d CUs", L.count, L.tile_ids.size(), n_cu);
        size_t at = 0;
        for (int r : L.robots) {               // the tiles of a robot: contiguous, in order, all in this launch
            CHECK(r >= 0 && r < nr, "tile launch lists robot %d", r);
            ++in_tiles[r];
            CHECK(at < L.tile_ids.size(), "robot %d: no tiles in its launch", r);
            const DTile& first = P.tiles[L.tile_ids[at]];
            CHECK(first.robot == r && first.tile0 == L.tile_ids[at] && first.ntiles == P.robot_tiles[r], "robot %d: first tile %d is (robot %d, tile0 %d, ntiles %d)", r, L.tile_ids[at], first.robot, first.tile0, first.ntiles);
            for (int t = 0; t < first.ntiles; ++t, ++at) {
                CHECK(at < L.tile_ids.size() && L.tile_ids[at] == first.tile0 + t, "robot %d: its tiles are not contiguous in the launch", r);
                const DTile& d = P.tiles[L.tile_ids[at]];
                CHECK(d.robot == r && d.tile0 == first.tile0 && d.ntiles == first.ntiles, "robot %d: tile %d belongs to (robot %d, tile0 %d)", r, L.tile_ids[at], d.robot, d.tile0);
            }
        }
        CHECK(at == L.tile_ids.size(), "tile launch: %zu tile ids, %zu of them of its robots", L.tile_ids.size(), at);
    }
    int n_rest = 0, n_all = 0;
    for (int r = 0; r < nr; ++r) {
        const bool work = robots[r].nvox > 0, rest = P.streamed_rest[r] && work, all = P.streamed_all[r] && work;
        CHECK(in_group[r] + in_tiles[r] + (rest ? 1 : 0) + (work ? 0 : 1) == 1, "robot %d: in %d groups, %d tile launches, rest mask %d, %d voxels", r, in_group[r], in_tiles[r], (int)rest, robots[r].nvox);
        CHECK((P.robot_tiled[r] != 0) == (in_tiles[r] == 1) && (P.robot_tiles[r] > 0) == (in_tiles[r] == 1), "robot %d: robot_tiled %d, robot_tiles %d, in %d tile launches", r, P.robot_tiled[r], P.robot_tiles[r], in_tiles[r]);
        CHECK((P.streamed_all[r] != 0) == (in_tiles[r] == 0), "robot %d: mask `all` %d, tiled %d", r, P.streamed_all[r], in_tiles[r]);
        n_rest += rest; n_all += all;
    }
    CHECK(n_rest == P.n_rest && n_all == P.n_all, "n_rest %d (mask: %d), n_all %d (mask: %d)", P.n_rest, n_rest, P.n_all, n_all);
}

// resident schedule: every bond of an axis exactly once in the axis' [block] slice, unpacking to the model's (v, neighbour, class); the rest -1
void check_schedule(const RobotModel& M, int r, const HostBatch& H)
{
    if (!(M.nvox > 0 && M.nvox <= 1024 && M.bond_classes.size() <= 4095)) return;
    const int block = resident_block(M.nvox);
    CHECK(H.robot[r].sched_begin == H.sched_off[r] && H.sched_off[r + 1] - H.sched_off[r] == 3 * block, "robot %d: schedule of %d entries for block %d", r, H.sched_off[r + 1] - H.sched_off[r], block);
    for (int a = 0; a < 3; ++a) {
        std::vector<char> seen(M.nvox, 0);
        int listed = 0, bonds = 0;
        for (int v = 0; v < M.nvox; ++v) bonds += M.bond_class[(size_t)v * 3 + a] >= 0;
        for (int j = 0; j < block; ++j) {
            const int e = H.bsched[H.sched_off[r] + a * block + j];
            if (e == -1) continue;
            const int v = e & 1023, n = (e >> 10) & 1023, c = (int)((unsigned)e >> 20);
            CHECK(v < M.nvox && !seen[v], "robot %d axis %d: schedule entry %d names voxel %d (out of range or twice)", r, a, j, v);
            CHECK(M.bond_class[(size_t)v * 3 + a] == c && M.nbr[(size_t)v * 6 + 2 * a] == n, "robot %d axis %d: entry %d = (v %d, n %d, class %d), model (n %d, class %d)", r, a, j, v, n, c, M.nbr[(size_t)v * 6 + 2 * a], M.bond_class[(size_t)v * 3 + a]);
            seen[v] = 1; ++listed;
        }
        CHECK(listed == bonds, "robot %d axis %d: %d bonds scheduled, the model has %d", r, a, listed, bonds);
    }
}

// wide lists: every bond once, axis-major, with the right fields; the six gather fields of a voxel: the record of that direction's bond or wzidx
void check_wide(const RobotModel& M, int r, int variant, const Options& opt, const HostBatch& H)
{
    const DRobot& R = H.robot[r];
    CHECK(R.wl_begin == H.wl_off[r], "robot %d: wl_begin %d against offset %d", r, R.wl_begin, H.wl_off[r]);
    if (!wide_listed(M, variant, opt)) { CHECK(R.wnbond == 0 && H.wl_off[r + 1] == H.wl_off[r], "robot %d: not wide-listed, but %d list entries", r, R.wnbond); return; }
    CHECK(R.wnbond == M.nbond && H.wl_off[r + 1] - H.wl_off[r] == M.nbond && R.wzidx <= 1023 && R.wzidx >= M.nbond, "robot %d: wnbond %d (model %d), wzidx %d", r, R.wnbond, M.nbond, R.wzidx);
    std::vector<int> rec((size_t)M.nvox * 3, -1);
    int t = 0;
    for (int a = 0; a < 3; ++a)
        for (int v = 0; v < M.nvox; ++v) {
            const int c = M.bond_class[(size_t)v * 3 + a];
            if (c < 0) continue;
            CHECK(t < M.nbond, "robot %d: more bonds with a class than nbond = %d", r, M.nbond);
            const unsigned e = (unsigned)H.wlist[R.wl_begin + t];
            const int ev = e & 511, en = (e >> 9) & 511, ea = (e >> 18) & 3, ec = e >> 20;
            CHECK(ev == v && en == M.nbr[(size_t)v * 6 + 2 * a] && ea == a && ec == c, "robot %d: wlist[%d] = (v %d, n %d, axis %d, class %d), expected (%d, %d, %d, %d)", r, t, ev, en, ea, ec, v, M.nbr[(size_t)v * 6 + 2 * a], a, c);
            rec[(size_t)v * 3 + a] = t++;
        }
    CHECK(t == M.nbond, "robot %d: %d bonds listed, nbond %d", r, t, M.nbond);
    for (int v = 0; v < M.nvox; ++v) {
        const unsigned w[2] = {(unsigned)H.wgather[H.vox_begin[r] + v], (unsigned)H.wgather[(size_t)H.nv + H.vox_begin[r] + v]};
        for (int d = 0; d < 6; ++d) {
            const int a = d / 2, from = (d & 1) ? M.nbr[(size_t)v * 6 + d] : v;      // +A: the voxel's own bond; -A: that of its -A neighbour
            const int want = from >= 0 && rec[(size_t)from * 3 + a] >= 0 ? rec[(size_t)from * 3 + a] : R.wzidx;
            const int got = (w[d / 3] >> (10 * (d % 3))) & 1023;
            CHECK(got == want, "robot %d voxel %d direction %d: gather field %d, expected %d (wzidx %d)", r, v, d, got, want, R.wzidx);
        }
    }
}

// DRobot ranges and the exclusion bit rows
void check_robot_ranges(const Robots& robots, const HostBatch& H)
{
    const int nr = (int)robots.size();
    for (int r = 0; r < nr; ++r) {
        const RobotModel& M = robots[r];
        const DRobot& R = H.robot[r];
        CHECK(R.vox_begin == H.vox_begin[r] && R.vox_begin % 64 == 0 && R.nvox == M.nvox, "robot %d: vox_begin %d, nvox %d", r, R.vox_begin, R.nvox);
        const int vox_end = R.vox_begin + (M.nvox + 63) / 64 * 64;
        CHECK(vox_end <= (r + 1 < nr ? H.robot[r + 1].vox_begin : H.nv), "robot %d: voxel range ends at %d, beyond the next robot's", r, vox_end);
        CHECK(R.nsurf == (M.vxa.self_col_enabled ? M.nsurf : 0), "robot %d: nsurf %d", r, R.nsurf);
        CHECK(R.col_begin + (long long)R.col_cap * R.nsurf <= (r + 1 < nr ? H.robot[r + 1].col_begin : H.col_total), "robot %d: contact rows [%lld + %d x %d) overlap the next robot's", r, R.col_begin, R.col_cap, R.nsurf);
        if (!M.vxa.self_col_enabled) continue;
        CHECK(R.excl_wpr == (M.nsurf + 63) / 64 && R.excl_begin + (long long)R.excl_wpr * M.nsurf <= (long long)H.excl.size(), "robot %d: exclusion rows out of range", r);
        std::vector<char> near(M.nvox, 0);
        for (int i = 0; i < M.nsurf; ++i) {
            const int vi = M.surf[i];
            CHECK(H.surf[R.surf_begin + i] == R.vox_begin + vi && H.surf_ord[R.vox_begin + vi] == i, "robot %d: surface ordinal %d", r, i);
            for (int k = M.near_off[vi]; k < M.near_off[vi + 1]; ++k) near[M.near_idx[k]] = 1;
            for (int j = 0; j < R.excl_wpr * 64; ++j) {
                const bool bit = (H.excl[(size_t)R.excl_begin + (size_t)i * R.excl_wpr + (j >> 6)] >> (j & 63)) & 1;
                CHECK(bit == (j < M.nsurf && near[M.surf[j]]), "robot %d: exclusion bit (%d, %d) is %d", r, i, j, (int)bit);
            }
            for (int k = M.near_off[vi]; k < M.near_off[vi + 1]; ++k) near[M.near_idx[k]] = 0;
        }
    }
}

// the tiles of one tiled robot: ownership, halo, bonds, its part of the drag mesh
void check_tiles(const RobotModel& M, int r, const HostBatch& H, const LaunchPlan& P)
{
    const int base = H.vox_begin[r], nv = H.nv, k = P.robot_tiles[r];
    int tile0 = -1;
    for (size_t t = 0; t < P.tiles.size() && tile0 < 0; ++t) if (P.tiles[t].robot == r) tile0 = P.tiles[t].tile0;
    CHECK(tile0 >= 0 && k > 0, "robot %d: tiled, but no tiles", r);
    std::map<int, int> vox_of_slot;            // exchange slot -> voxel of this robot
    int owned = 0;
    for (int v = 0; v < M.nvox; ++v) {
        const int g = base + v, t = P.tile_of[g];
        CHECK(t >= tile0 && t < tile0 + k, "robot %d voxel %d: owner tile %d outside [%d, %d)", r, v, t, tile0, tile0 + k);
        const DTile& d = P.tiles[t];
        CHECK(P.tile_lidx[g] >= 0 && P.tile_lidx[g] < d.n_own && P.tile_vox[d.vox_off + P.tile_lidx[g]] == g, "robot %d voxel %d: tile_lidx %d is not its place in tile %d", r, v, P.tile_lidx[g], t);
        CHECK(P.xslot[g] == d.xoff + P.tile_lidx[g] && d.xoff % 64 == 0, "robot %d voxel %d: exchange slot %d, tile xoff %d", r, v, P.xslot[g], d.xoff);
        CHECK(vox_of_slot.emplace(P.xslot[g], v).second, "robot %d voxel %d: exchange slot %d used twice", r, v, P.xslot[g]);
    }
    long long sum_nb = 0, expect_nb = 0;
    std::map<std::pair<int, int>, int> listed;  // (bond slot, tile) -> times
    for (int t = tile0; t < tile0 + k; ++t) {
        const DTile& d = P.tiles[t];
        owned += d.n_own;
        std::vector<int> local(d.n_own + d.n_halo);         // local index -> voxel of the robot
        for (int i = 0; i < d.n_own; ++i) {
            const int g = P.tile_vox[d.vox_off + i];
            CHECK(g >= base && g < base + M.nvox && P.tile_of[g] == t, "tile %d: owned entry %d is global slot %d", t, i, g);
            local[i] = g - base;
        }
        for (int i = 0; i < d.n_halo; ++i) {
            const auto it = vox_of_slot.find(P.tile_vox[d.vox_off + d.n_own + i]);
            CHECK(it != vox_of_slot.end() && P.tile_of[base + it->second] != t, "tile %d: halo entry %d = %d is no exchange slot of another tile of robot %d", t, i, P.tile_vox[d.vox_off + d.n_own + i], r);
            local[d.n_own + i] = it->second;
        }
        sum_nb += d.nb;
        for (int b = 0; b < d.nb; ++b) {
            const unsigned e = (unsigned)P.tile_bond[d.bond_off + b];
            const int l1 = e & 1023, l2 = (e >> 10) & 1023, a = e >> 20, slot = P.tile_bslot[d.bond_off + b];
            CHECK(a < 3 && l1 < (int)local.size() && l2 < (int)local.size(), "tile %d bond %d: entry (%d, %d, axis %d)", t, b, l1, l2, a);
            const int v1 = slot - a * nv - base;
            CHECK(v1 >= 0 && v1 < M.nvox && local[l1] == v1 && M.bond_class[(size_t)v1 * 3 + a] >= 0, "tile %d bond %d: slot %d is no bond of robot %d (axis %d, voxel %d)", t, b, slot, r, a, v1);
            CHECK(local[l2] == M.nbr[(size_t)v1 * 6 + 2 * a] && P.tile_bcls[d.bond_off + b] == M.bond_class[(size_t)v1 * 3 + a], "tile %d bond %d: positive end %d / class %d differ from the model", t, b, local[l2], P.tile_bcls[d.bond_off + b]);
            CHECK(P.tile_of[base + v1] == t || P.tile_of[base + local[l2]] == t, "tile %d bond %d: owns neither end", t, b);
            CHECK(++listed[std::make_pair(slot, t)] == 1, "tile %d: bond slot %d listed twice", t, slot);
        }
        if (d.n_mv > 0 || d.n_f > 0) {
            for (int i = 0; i < d.n_mv; ++i)
                for (int c = 0; c < 8; ++c) { const int s = P.tile_mvert[(size_t)c * P.n_tmv + d.mv_off + i]; CHECK(s >= -1 && s < d.n_mx, "tile %d: mesh vertex %d corner %d names voxel %d of %d", t, i, c, s, d.n_mx); }
            for (int f = 0; f < d.n_f; ++f) {
                CHECK(P.tile_facet[d.f_off + f] >= 0 && P.tile_facet[d.f_off + f] < d.n_own, "tile %d: facet %d owned by %d", t, f, P.tile_facet[d.f_off + f]);
                for (int c = 1; c < 4; ++c) { const int i = P.tile_facet[(size_t)c * P.n_tf + d.f_off + f]; CHECK(i >= 0 && i < d.n_mv, "tile %d: facet %d names vertex %d of %d", t, f, i, d.n_mv); }
            }
            for (int i = 0; i < d.n_mx; ++i) CHECK(vox_of_slot.count(P.tile_mvox[d.mx_off + i]), "tile %d: mesh voxel %d is no exchange slot of robot %d", t, i, r);
        }
    }
    CHECK(owned == M.nvox, "robot %d: its tiles own %d voxels of %d", r, owned, M.nvox);
    // every bond by the tile owning either end: once, or twice across a tile boundary -- what vxh_tiling_info::total_bonds counts
    for (int v = 0; v < M.nvox; ++v)
        for (int a = 0; a < 3; ++a) {
            if (M.bond_class[(size_t)v * 3 + a] < 0) continue;
            const int t1 = P.tile_of[base + v], t2 = P.tile_of[base + M.nbr[(size_t)v * 6 + 2 * a]], slot = a * nv + base + v;
            CHECK(listed.count(std::make_pair(slot, t1)) && listed.count(std::make_pair(slot, t2)), "robot %d: bond (%d, axis %d) is missing in tile %d or %d", r, v, a, t1, t2);
            expect_nb += t1 == t2 ? 1 : 2;
        }
    CHECK(sum_nb == expect_nb, "robot %d: its tiles list %lld bonds, expected %lld", r, sum_nb, expect_nb);
    const TilePlan again = plan_tiles(M, k);
    if (again.k == k) {
        long long total = 0;
        for (const auto& t : again.tiles) total += (long long)t.bond_v1.size();
        CHECK(total == sum_nb, "robot %d: plan_tiles(%d) lists %lld bonds, the batch %lld", r, k, total, sum_nb);
    }
}

void check_batch(const Robots& robots, int variant, int n_cu, const char* name, const Options& opt)
{
    g_set = name;
    const HostBatch H = assemble_batch(robots, variant, opt, 0);
    const LaunchPlan P = plan_launches(robots, H, variant, opt, true, n_cu);
    const int nr = (int)robots.size();
    check_partition(robots, P, n_cu);
    check_robot_ranges(robots, H);
    int n_tiled = 0;
    for (int r = 0; r < nr; ++r) {
        check_schedule(robots[r], r, H);
        check_wide(robots[r], r, variant, opt, H);
        if (P.robot_tiled[r]) { check_tiles(robots[r], r, H, P); ++n_tiled; }
        else if (!P.tiles.empty()) for (int v = 0; v < robots[r].nvox; ++v) CHECK(P.tile_of[H.vox_begin[r] + v] == -1, "robot %d: not tiled, but voxel %d has an owner tile", r, v);
    }
    std::printf("batch_check [%s]: %d robots, %d voxel slots; %zu groups, %zu tile launches (%d robots, %zu tiles), %d left to the streaming kernels: ok\n",
                name, nr, H.nv, P.groups.size(), P.tile_launches.size(), n_tiled, P.tiles.size(), P.n_rest);
}

// ---- --arrays: the in-memory route (models_from_arrays, what vxh_add_robots takes) against the file route ----
struct FileLayer { const char* tag; bool VxaModel::*has; std::vector<double> VxaModel::*values; };
const FileLayer file_layers[] = {
    {"PhaseOffset", &VxaModel::has_phase_offset, &VxaModel::phase_offset}, {"TempAmpDamp", &VxaModel::has_temp_amp_damp, &VxaModel::temp_amp_damp},
    {"Stiffness", &VxaModel::has_stiffness, &VxaModel::stiffness}, {"FinalPhaseOffset", &VxaModel::has_final_phase_offset, &VxaModel::final_phase_offset},
    {"FinalTempAmpDamp", &VxaModel::has_final_temp_amp_damp, &VxaModel::final_temp_amp_damp}, {"InitialVoxelSize", &VxaModel::has_initial_voxel_size, &VxaModel::initial_voxel_size},
    {"FinalVoxelSize", &VxaModel::has_final_voxel_size, &VxaModel::final_voxel_size}, {"GrowthTime", &VxaModel::has_growth_time, &VxaModel::growth_time},
    {"StartGrowthTime", &VxaModel::has_start_growth_time, &VxaModel::start_growth_time},
};

// a file's own lattice and layers handed back as arrays: material = structure, every present layer expanded from per-occupied-voxel values to the full lattice
struct ArraysOfFile {
    std::vector<std::vector<double>> full;
    std::vector<const char*> tags;
    std::vector<const double*> ptrs;
    vxh_robot_arrays A{};
    explicit ArraysOfFile(const VxaModel& vxa)
    {
        for (const FileLayer& l : file_layers) {
            if (!(vxa.*(l.has))) continue;
            std::vector<double> f(vxa.structure.size(), 0.0);
            size_t occupied = 0;
            for (size_t k = 0; k < f.size(); ++k) if (vxa.structure[k]) f[k] = (vxa.*(l.values)).at(occupied++);
            full.push_back(std::move(f)); tags.push_back(l.tag);
        }
        for (const auto& f : full) ptrs.push_back(f.data());
        A.nx = vxa.nx; A.ny = vxa.ny; A.nz = vxa.nz; A.material = vxa.structure.data();
        A.n_layers = (int)full.size(); A.layer_tags = tags.data(); A.layers = ptrs.data();
    }
    ArraysOfFile(const ArraysOfFile&) = delete;
};

template <class T>
void same_values(const char* what, const std::vector<T>& a, const std::vector<T>& b)
{
    static_assert(std::is_arithmetic<T>::value, "element-wise comparison of numbers");
    CHECK(a.size() == b.size(), "%s: %zu against %zu elements", what, a.size(), b.size());
    for (size_t i = 0; i < a.size(); ++i) CHECK(a[i] == b[i], "%s[%zu] differs", what, i);
}
// (bytewise: only for structs without padding)
static_assert(sizeof(DVoxClass) == 12 * sizeof(double) + 2 * sizeof(int), "DVoxClass has padding");
static_assert(sizeof(DBondClass) == 20 * sizeof(double) + 2 * sizeof(int), "DBondClass has padding");
static_assert(sizeof(DRobot) == 30 * sizeof(int) + 2 * sizeof(long long) + 17 * sizeof(double) + 2 * sizeof(float), "DRobot has padding");
static_assert(sizeof(DRobotState) == 13 * sizeof(double) + sizeof(unsigned long long) + 14 * sizeof(int), "DRobotState has padding");
template <class T>
void same_bytes(const char* what, const std::vector<T>& a, const std::vector<T>& b)
{
    CHECK(a.size() == b.size(), "%s: %zu against %zu elements", what, a.size(), b.size());
    for (size_t i = 0; i < a.size(); ++i) CHECK(std::memcmp(&a[i], &b[i], sizeof(T)) == 0, "%s[%zu] differs", what, i);
}

void same_batch(const HostBatch& a, const HostBatch& b)
{
#define SCALAR(f) CHECK(a.f == b.f, #f " differs")
#define VALUES(f) same_values(#f, a.f, b.f)
#define BYTES(f) same_bytes(#f, a.f, b.f)
    SCALAR(nv); SCALAR(ns); SCALAR(total_trace); SCALAR(total_vol); SCALAR(total_xtrace); SCALAR(max_planned); SCALAR(max_nvox); SCALAR(any_dev); SCALAR(any_mesh); SCALAR(any_fluid);
    SCALAR(total_mv); SCALAR(total_facet); SCALAR(col_total);
    BYTES(robot); BYTES(rstate); BYTES(vtab); BYTES(btab);
    VALUES(vox_begin); VALUES(surf_begin); VALUES(trace_begin); VALUES(trace_cap); VALUES(vol_begin); VALUES(xt_begin[0]); VALUES(xt_begin[1]); VALUES(xt_cap[0]); VALUES(xt_cap[1]); VALUES(wave_robot); VALUES(nbr); VALUES(surf); VALUES(surf_code);
    VALUES(surf_ord); VALUES(excl); VALUES(vclass); VALUES(bclass); VALUES(sched_off); VALUES(bsched); VALUES(wl_off); VALUES(wlist); VALUES(wgather);
    VALUES(amp_damp); VALUES(dev); VALUES(act_sb); VALUES(act_cb); VALUES(px); VALUES(py); VALUES(pz); VALUES(sc); VALUES(qw); VALUES(small);
    VALUES(mv_begin); VALUES(facet_begin); VALUES(vert_pack); VALUES(vert_vox); VALUES(vert_robot); VALUES(vert_v0); VALUES(facet_vox); VALUES(facet_vert);
    VALUES(facet_first); VALUES(facet_robot); VALUES(facet_count); VALUES(vtab_off); VALUES(btab_off); VALUES(excl_off); VALUES(col_off); VALUES(col_cap);
    VALUES(img_idx);
#undef SCALAR
#undef VALUES
#undef BYTES
}

void expect_refusal(const char* what, const std::string& text, const vxh_robot_arrays* in, int n, int variant, const char* message)
{
    g_set = what;
    try {
        models_from_arrays(text.data(), text.size(), in, n, false, variant, false);
    } catch (const std::invalid_argument& ex) {
        CHECK(std::strstr(ex.what(), message), "refused with \"%s\", expected \"%s\"", ex.what(), message);
        return;
    }
    fail("accepted, expected the refusal \"%s\"", message);
}

// what models_from_arrays must refuse, on variations of one good robot
void check_refusals(const std::string& text, const vxh_robot_arrays& good, int variant)
{
    const size_t cells = (size_t)good.nx * good.ny * good.nz;
    vxh_robot_arrays A = good;
    A.nx = 0; expect_refusal("nx = 0", text, &A, 1, variant, "bad lattice");
    A = good; A.material = nullptr; expect_refusal("no material", text, &A, 1, variant, "bad lattice");
    const std::vector<unsigned char> wrong(cells, 200);
    A = good; A.material = wrong.data(); expect_refusal("material 200", text, &A, 1, variant, "material index outside the palette");
    const std::vector<double> layer(cells, 0.5);
    const char* tag = "Bogus"; const double* values = layer.data();
    A = good; A.n_layers = 1; A.layer_tags = &tag; A.layers = &values;
    expect_refusal("unknown layer", text, &A, 1, variant, "unsupported per-voxel layer <Bogus>");
    tag = "GrowthTime";
    if (variant == 1) expect_refusal("land-only layer", text, &A, 1, variant, "unsupported <GrowthTime> development layer (land_water)");
    A.layer_tags = nullptr; expect_refusal("no tag array", text, &A, 1, variant, "bad layer arrays");
    A.layer_tags = &tag; A.layers = nullptr; expect_refusal("no layer array", text, &A, 1, variant, "bad layer arrays");
    A.n_layers = -1; expect_refusal("n_layers = -1", text, &A, 1, variant, "bad layer arrays");
    A.n_layers = 1; A.layers = &values; tag = nullptr; expect_refusal("null tag", text, &A, 1, variant, "null layer tag or layer");
    tag = "PhaseOffset"; values = nullptr; expect_refusal("null layer", text, &A, 1, variant, "null layer tag or layer");
    // of several bad robots the first IN INDEX ORDER is reported, whichever thread met which
    std::vector<vxh_robot_arrays> many(40, good);
    many[17].material = wrong.data(); many[30].nx = 0;
    expect_refusal("40 robots, 17 and 30 bad", text, many.data(), 40, variant, "material index outside the palette");
}

void check_arrays(int variant, const std::vector<std::string>& paths)
{
    const Robots by_file = build_vxa_files(paths, variant, false);
    for (size_t i = 0; i < paths.size(); ++i) {
        g_set = paths[i].c_str();
        std::ifstream in(paths[i], std::ios::binary);
        std::stringstream ss;
        ss << in.rdbuf();
        const std::string text = ss.str();
        const VxaModel vxa = read_vxa(text.data(), text.size(), variant);
        const ArraysOfFile arrays(vxa);
        const Robots by_arrays = build_models(models_from_arrays(text.data(), text.size(), &arrays.A, 1, false, variant, false));
        CHECK(by_arrays.size() == 1 && by_arrays[0].nvox == by_file[i].nvox && by_arrays[0].nbond == by_file[i].nbond, "the robot built from arrays has other dimensions");
        same_batch(assemble_batch(by_arrays, variant, Options(), 0), assemble_batch(Robots(1, by_file[i]), variant, Options(), 0));
        if (i == 0) check_refusals(text, arrays.A, variant);
        std::printf("batch_check --arrays [%s]: %d voxels, %d layers: the same batch as from the file: ok\n", paths[i].c_str(), by_file[i].nvox, arrays.A.n_layers);
    }
}

// ---- --dominant: dominant_kernel on hand-made calls; the expected values were worked out from the rule by hand ----
struct DomRobot { int nvox, nbond, steps, tiled; };
struct DomCase {
    const char* name;
    std::vector<DomRobot> robots;
    std::vector<std::vector<int>> groups;      // group k: block 256 * (k + 1), wide when k is odd
    bool fused, tiled, streaming;
    int n_rest; long long todo; std::vector<long long> group_launches; long long tile_launch_count;
    DominantKernel want;                       // {unit, group, block, robots, launches, alg_bytes, voxel_steps}
};

void check_dominant()
{
    typedef DominantKernel D;
    const std::vector<DomCase> cases = {
        // all 21500, tiles 20000, group 1000, rest 500
        {"the tiles win", {{2000, 5000, 10, 1}, {100, 200, 10, 0}, {50, 80, 10, 0}}, {{1}}, true, true, true, 1, 10, {1}, 2,
         {D::TILES, -1, 1, 1, 2, 10 * (224.0 * 2000 + 144.0 * 5000), 20000}},
        {"the tiles tie with the best group: the tiles, by >=", {{100, 150, 10, 1}, {100, 0, 10, 0}}, {{1}}, true, true, false, 0, 10, {1}, 3,
         {D::TILES, -1, 1, 1, 3, 10 * (224.0 * 100 + 144.0 * 150), 1000}},
        // groups 1500 and 2000 (a robot that took 5 steps while the others took 10)
        {"the best of two groups", {{100, 0, 10, 0}, {400, 30, 5, 0}, {50, 0, 10, 0}}, {{0, 2}, {1}}, true, false, false, 0, 10, {4, 7}, 0,
         {D::GROUP, 1, 513, 1, 7, 5 * (224.0 * 400 + 144.0 * 30), 2000}},
        {"two groups tie: the first", {{100, 10, 10, 0}, {100, 0, 10, 0}}, {{0}, {1}}, true, false, false, 0, 10, {4, 7}, 0,
         {D::GROUP, 0, 256, 1, 4, 10 * (224.0 * 100 + 144.0 * 10), 1000}},
        {"the streamed rest beats the best group", {{100, 0, 10, 0}, {300, 20, 10, 0}}, {{0}}, true, false, true, 1, 10, {1}, 0,
         {D::REST, -1, 0, 1, 10, 10 * (224.0 * 300 + 144.0 * 20), 3000}},
        {"the rest ties with the best group: the group, by >", {{100, 0, 10, 0}, {100, 0, 10, 0}}, {{0}}, true, false, true, 1, 10, {5}, 0,
         {D::GROUP, 0, 256, 1, 5, 10 * 224.0 * 100, 1000}},
        // the option fused = 0: the plan still has its group, the call did not use it; the small tiled robot (500 of 3500) does not win
        {"fused = 0: everything streamed", {{100, 0, 10, 0}, {200, 10, 10, 0}, {50, 0, 10, 1}}, {{0, 1}}, false, true, true, 0, 10, {0}, 1,
         {D::STREAMED, -1, 0, 2, 10, 10 * (224.0 * 300 + 144.0 * 10), 3000}},
        // tiles 1000 against groups of 900, 800 and 700: more than every single unit, less than all - tiles - best group = 1500
        {"the other groups together outweigh the tiles", {{100, 0, 10, 1}, {90, 0, 10, 0}, {80, 0, 10, 0}, {70, 0, 10, 0}}, {{1}, {2}, {3}}, true, true, false, 0, 10, {2, 2, 2}, 1,
         {D::GROUP, 0, 256, 1, 2, 10 * 224.0 * 90, 900}},
    };
    for (const DomCase& c : cases) {
        g_set = c.name;
        Robots robots(c.robots.size());
        std::vector<int> steps;
        std::vector<unsigned char> robot_tiled;
        for (size_t r = 0; r < c.robots.size(); ++r) {
            robots[r].nvox = c.robots[r].nvox; robots[r].nbond = c.robots[r].nbond;
            steps.push_back(c.robots[r].steps); robot_tiled.push_back((unsigned char)c.robots[r].tiled);
        }
        std::vector<GroupPlan> plans(c.groups.size());
        std::vector<const GroupPlan*> groups;
        for (size_t k = 0; k < plans.size(); ++k) {
            plans[k].block = 256 * ((int)k + 1); plans[k].wide = (int)(k & 1); plans[k].robots = c.groups[k]; plans[k].count = (int)c.groups[k].size();
            groups.push_back(&plans[k]);
        }
        const D got = dominant_kernel(robots, steps, groups, robot_tiled, c.fused, c.tiled, c.streaming, c.n_rest, c.todo, c.group_launches, c.tile_launch_count);
        CHECK(got.unit == c.want.unit && got.group == c.want.group, "unit %d group %d, expected unit %d group %d", (int)got.unit, got.group, (int)c.want.unit, c.want.group);
        CHECK(got.block == c.want.block && got.robots == c.want.robots && got.launches == c.want.launches, "block %d, %d robots, %lld launches; expected %d, %d, %lld",
              got.block, got.robots, got.launches, c.want.block, c.want.robots, c.want.launches);
        CHECK(got.alg_bytes == c.want.alg_bytes && got.voxel_steps == c.want.voxel_steps, "%.17g bytes, %.17g voxel-steps; expected %.17g, %.17g",
              got.alg_bytes, got.voxel_steps, c.want.alg_bytes, c.want.voxel_steps);
        std::printf("batch_check --dominant [%s]: ok\n", c.name);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    try {
        if (mode == "--dominant") { check_dominant(); return 0; }
        if (mode == "--arrays" && argc >= 4) { check_arrays(std::atoi(argv[2]), std::vector<std::string>(argv + 3, argv + argc)); return 0; }
        if (argc < 4 || mode[0] == '-') { std::fprintf(stderr, "usage: batch_check <variant 0|1> <CUs> robot.vxa... | --arrays <variant 0|1> robot.vxa... | --dominant\n"); return 2; }
        const int variant = std::atoi(argv[1]), n_cu = std::atoi(argv[2]);
        const Robots robots = build_vxa_files(std::vector<std::string>(argv + 3, argv + argc), variant, false);
        Options o;
        check_batch(robots, variant, n_cu, "defaults", o);
        o = Options(); o.wide = 0;
        check_batch(robots, variant, n_cu, "wide=0", o);
        o = Options(); o.tiled = 2;
        check_batch(robots, variant, n_cu, "tiled=2", o);
        o.tiles_per_robot = 3;
        check_batch(robots, variant, n_cu, "tiled=2,tiles_per_robot=3", o);
        o = Options(); o.tile_small = 1;
        check_batch(robots, variant, std::max(n_cu, 4 * (int)robots.size()), "tile_small=1", o);
        o = Options(); o.fused = 0;
        check_batch(robots, variant, n_cu, "fused=0", o);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "batch_check: %s\n", ex.what());
        return 1;
    }
    return 0;
}
