// The developer switches' reports (dev_report.hpp)
#include "dev_report.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "device_types.hpp"

namespace vxh {

// The spread of the robots' cost in the last LONG launch of a colliding k_robot_steps group, as the workgroups
// measured it (constant-rate clock, whole launch incl. broad-phase runs), and what the dispatch order made of it: the CUs take the
// workgroups in order as they get free, so the launch ends with the largest sum of a CU -- set against the mean sum (no idle CU at
// all) and against the same hand-out with the true costs known beforehand (what two robots per CU allow at best).
void report_dispatch_cost(size_t group, const std::vector<DispatchCost>& c, const std::vector<int>& perm, int block, size_t lds, long long last_len,
                          bool last_ordered, int n_cu, double us_per_tick)
{
    const int count = (int)c.size();
    const double steps = (double)std::max<long long>(1, last_len);
    std::vector<double> t(count);
    double sum = 0, sq = 0, mx = 0, mn = DBL_MAX, reb = 0; int n_reb = 0;
    for (int k = 0; k < count; ++k) {
        t[k] = us_per_tick * (double)c[k].launch_ticks / steps;
        sum += t[k]; sq += t[k] * t[k]; mx = std::max(mx, t[k]); mn = std::min(mn, t[k]);
        if (c[k].reb_ticks > 0) { reb += us_per_tick * c[k].reb_ticks; ++n_reb; }
    }
    const double mean = sum / count, sigma = std::sqrt(std::max(0.0, sq / count - mean * mean));
    // workgroups per CU: what the LDS leaves room for (threads: 2048 per CU)
    const int per_cu = std::max(1, std::min((int)(160 * 1024 / (lds + VXH_FUSED_STATIC_LDS)), 2048 / std::max(1, block)));
    const int slots = std::max(1, n_cu * per_cu);
    auto hand_out = [&](const std::vector<int>& order) {
        std::vector<double> load(std::min(slots, count), 0.0);
        for (int k : order) { auto it = std::min_element(load.begin(), load.end()); *it += t[k]; }
        return *std::max_element(load.begin(), load.end());
    };
    std::vector<int> best(perm);
    std::stable_sort(best.begin(), best.end(), [&](int a, int b) { return t[a] > t[b]; });
    const double mean_sum = sum / (double)std::min(slots, count);
    std::fprintf(stderr, "dispatch cost: group %zu, k_robot_steps<%d>, %d robots on %d workgroup slots, last long launch %lld steps, order %s\n"
                 "  us per step per robot: mean %.3f  sigma %.3f (%.1f %%)  min %.3f  max %.3f; broad-phase run %.1f us (mean of %d robots)\n"
                 "  us per step per slot: largest sum under this order %.3f | mean sum %.3f | largest sum with the true costs known %.3f  -> idle at the end %.1f %% (%.1f %% at best)\n",
                 group, block, count, slots, last_len, last_ordered ? "by measured cost" : "of the list", mean, sigma, 100 * sigma / mean, mn, mx,
                 n_reb ? reb / n_reb : 0.0, n_reb, hand_out(perm), mean_sum, hand_out(best), 100 * (hand_out(perm) / mean_sum - 1), 100 * (hand_out(best) / mean_sum - 1));
}

void report_contact_rows(const std::vector<int>& cnt, const std::vector<int>& surf_begin, const std::vector<int>& nsurf)
{
    long long hist[9] = {0}, total = 0; int mx = 0;
    for (int c : cnt) { total += c; mx = std::max(mx, c); ++hist[c == 0 ? 0 : std::min(8, 1 + (c - 1) / 8)]; }
    fprintf(stderr, "contact rows: %zu surface voxels, %.1f partners on average, longest %d; rows by length 0 | 1-8 | 9-16 | ... | 57-64:", cnt.size(), (double)total / cnt.size(), mx);
    for (long long v : hist) fprintf(stderr, " %lld", v);
    long long per_robot_max = 0;
    for (size_t r = 0; r < nsurf.size(); ++r) {
        long long sum = 0;
        const int b = surf_begin[r], n = nsurf[r];
        for (int i = 0; i < n; ++i) sum += cnt[b + i];
        per_robot_max = std::max(per_robot_max, sum);
    }
    fprintf(stderr, "\n  most partners in one robot: %lld\n", per_robot_max);
}

void report_phase_counters(const unsigned long long* h, int n_tiles, bool tiled)
{
    if (std::getenv("VXH_PROF_TILES")) {    // the first tiles at one step of the last launch: real-time counter (10 ns ticks) at the step's boundaries
        const int nt = std::min((int)VXH_PROF_TILE_COUNT, n_tiles);
        auto mark = [&](int t, int k) { return h[VXH_PROF_TILE + t * VXH_PROF_TILE_WORDS + k]; };
        unsigned long long t0 = ~0ull;
        for (int t = 0; t < nt; ++t) if (mark(t, 0)) t0 = std::min(t0, mark(t, 0));
        fprintf(stderr, "tile: top  halo-done  bond-done  voxel-done  C-passed | svc: barrier-resolved | next top | mv-published   (us after the first tile's top)\n");
        for (int t = 0; t < nt; ++t) {
            fprintf(stderr, "tile %3d:", t);
            for (int k : {0, 1, 2, 3, 4, 5, 6, 7}) fprintf(stderr, " %7.2f", 0.01 * (double)(long long)(mark(t, k) - t0));
            fprintf(stderr, "\n");
        }
    }
    if (h[VXH_PROF_XROW_LANES]) fprintf(stderr, "contact rows in LDS: cross-check (dbg 8): %llu lanes, %llu with different bits, %llu whose LDS row differs from memory; of the differing lanes: %llu with fewer mask bits than pairs in reach, %llu with more, %llu with as many\n",
                        h[VXH_PROF_XROW_LANES], h[VXH_PROF_XROW_DIFFER], h[VXH_PROF_XROW_LDS_DIFFERS], h[VXH_PROF_XROW_FEWER], h[VXH_PROF_XROW_MORE], h[VXH_PROF_XROW_AS_MANY]);
    const unsigned long long runs = h[VXH_PROF_REB_RUNS];
    if (runs) fprintf(stderr, "broad-phase runs (resident kernel, with the copy of the rows): %llu, %.0f cycles each on average; workgroup-launches with at least one: %llu; "
                        "most cycles one workgroup spent in them in one launch (maximum over ALL launches): %llu\n", runs, (double)h[VXH_PROF_REB_CYCLES] / (double)runs, h[VXH_PROF_REB_LAUNCHES], h[VXH_PROF_REB_MAX_CYCLES]);
    if (runs && h[VXH_PROF_REB_STAGE]) fprintf(stderr, "   of a broad-phase run, cycles on average (first wavefront): staging the surface list %.0f | its own scan / block pairs %.0f | wait for the "
                                  "slowest wavefront %.0f | bit matrix -> rows %.0f | the rest (copy of the rows to LDS) %.0f\n", (double)h[VXH_PROF_REB_STAGE] / runs, (double)h[VXH_PROF_REB_SCAN] / runs, (double)h[VXH_PROF_REB_WAIT] / runs,
                                  (double)h[VXH_PROF_REB_ROWS] / runs, ((double)h[VXH_PROF_REB_CYCLES] - (double)h[VXH_PROF_REB_STAGE] - (double)h[VXH_PROF_REB_SCAN] - (double)h[VXH_PROF_REB_WAIT] - (double)h[VXH_PROF_REB_ROWS]) / runs);
    if (h[VXH_PROF_XREB_ROWS]) fprintf(stderr, "   broad-phase cross-check (dbg 16): %llu rows built by both scans, %llu differ (%llu longer, %llu shorter than the plain scan's; longest row %llu against %llu; partners in all %llu against %llu)\n",
                         h[VXH_PROF_XREB_ROWS], h[VXH_PROF_XREB_DIFFER], h[VXH_PROF_XREB_LONGER], h[VXH_PROF_XREB_SHORTER], h[VXH_PROF_XREB_MAX_NEW], h[VXH_PROF_XREB_MAX_OLD], h[VXH_PROF_XREB_SUM_NEW], h[VXH_PROF_XREB_SUM_OLD]);
    if (h[VXH_PROF_PRO_TABLES]) fprintf(stderr, "   prologue of the resident kernel, cycle sums of the first thread over all workgroup-launches: tables + first barrier %.3e | state load, zeroing, "
                         "first control %.3e | rows_to_lds %.3e  = (its parts, incl. the calls after broad-phase runs) ordinal -> count loads + barrier %.3e | scan + allotment %.3e | copy + barrier %.3e\n",
                         (double)h[VXH_PROF_PRO_TABLES], (double)h[VXH_PROF_PRO_STATE], (double)h[VXH_PROF_PRO_R2L], (double)h[VXH_PROF_R2L_COUNT], (double)h[VXH_PROF_R2L_SCAN], (double)h[VXH_PROF_R2L_COPY]);
    const unsigned long long* tv = h + VXH_PROF_TILE_VOXEL;
    if (tv[2]) fprintf(stderr, "   tiled kernel, voxel phase of the first thread of every tile, cycle sums: six-direction sums %.3e | contacts %.3e | voxel update %.3e | pose granules out %.3e\n",
                         (double)tv[0], (double)tv[1], (double)tv[2], (double)tv[3]);
    const unsigned long long* dr = h + VXH_PROF_DRAG;
    if (dr[1]) fprintf(stderr, "   drag, facet pass (first thread, cycle sums): barrier behind the vertices %.3e | facet loop %.3e | barrier %.3e | per-voxel sums %.3e | barrier %.3e\n",
                         (double)dr[0], (double)dr[1], (double)dr[2], (double)dr[3], (double)dr[4]);
    static const char* names[6] = {"ctl+barA", "aux", "bond", "barB", "voxel", "barC+pub"};
    static const char* tnames[8] = {"halo-wait", "bond", "svc:poll", "barB", "latch/rebuild", "voxel", "barC+mv", "svc:reduce+horizon"};
    if (tiled && h[VXH_PROF_BARRIERS]) fprintf(stderr, "robot barrier: %.2f poll rounds per barrier, %.0f cycles per barrier\n", (double)h[VXH_PROF_BARRIER_POLLS] / h[VXH_PROF_BARRIERS], (double)h[VXH_PROF_BARRIER_CYCLES] / h[VXH_PROF_BARRIERS]);
    for (int w = 0; w < 15; ++w) {
        const unsigned long long* hw = h + VXH_PROF_WAVE + w * VXH_PROF_WAVE_WORDS;
        double tot = 0; for (int k = 0; k < (tiled ? 8 : 6); ++k) tot += (double)hw[k];
        if (tot == 0) continue;
        fprintf(stderr, "wave %2d:", w);
        if (tiled) for (int k = 0; k < 8; ++k) fprintf(stderr, " %s %5.1f%%", tnames[k], 100.0 * hw[k] / tot);
        else for (int k = 0; k < 6; ++k) fprintf(stderr, " %s %5.1f%%", names[k], 100.0 * hw[k] / tot);
        fprintf(stderr, "  total %.3e cycles", tot);
        if (!tiled && hw[6] + hw[7]) fprintf(stderr, "  (MESH: mesh vertices / facets inside aux; else: before the step loop / after it, cycles)  %.3e  %.3e", (double)hw[6], (double)hw[7]);
        fprintf(stderr, "\n");
    }
}

}  // namespace vxh
