// Host-only check of batch assembly and launch planning (batch.hpp): no HIP, built with the plain C++ compiler (make batch_check), so it
// also runs under the host sanitizers.  usage: batch_check <variant 0|1> <CUs> robot.vxa...   All robots form ONE batch, assembled and
// planned under several option sets; every table is then unpacked and compared with the robots' models.  Exit status 0 = all consistent.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "batch.hpp"

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

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: batch_check <variant 0|1> <CUs> robot.vxa...\n"); return 2; }
    const int variant = std::atoi(argv[1]), n_cu = std::atoi(argv[2]);
    Robots robots;
    try {
        for (int i = 3; i < argc; ++i) {
            std::ifstream in(argv[i], std::ios::binary);
            if (!in) throw std::runtime_error(std::string("io: cannot open ") + argv[i]);
            std::stringstream ss;
            ss << in.rdbuf();
            const std::string text = ss.str();
            const VxaModel vxa = read_vxa(text.data(), text.size(), variant);
            if (!vxa.unsupported.empty()) throw std::runtime_error(std::string(argv[i]) + ": unsupported " + vxa.unsupported.front());
            robots.push_back(build_robot(vxa));
        }
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
