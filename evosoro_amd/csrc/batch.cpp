// Batch assembly and launch planning (batch.hpp): everything Engine::prepare() works out on the host before it uploads.
#include "batch.hpp"
#include "import.hpp"      // for_each_index

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

namespace vxh {

WideLayout wide_layout(const RobotModel& M, int variant)
{
    WideLayout W;
    const bool in_fluid = variant == 1 && M.vxa.fluid_env;
    const int scratch = 12 * WIDE_BLOCK + (in_fluid ? 3 * ((M.nvox + 63) / 64 * 64) + 3 * M.nmv : 0);
    W.zidx = std::max(M.nbond, (scratch + VXH_WIDE_REC - 1) / VXH_WIDE_REC);
    W.region = (VXH_WIDE_REC * (W.zidx + 1) + 1) & ~1;
    return W;
}
bool wide_listed(const RobotModel& M, int variant, const Options& opt)
{
    return opt.wide && M.nvox > 0 && M.nvox <= WIDE_BLOCK && M.nbond <= 1023 && M.bond_classes.size() <= 4095 && wide_layout(M, variant).zidx <= 1023;
}
int resident_block(int n) { return n <= 256 ? 256 : (n <= 512 ? 512 : (n <= 768 ? 768 : 1024)); }

FusedVariant fused_variant(const RobotModel& M, int variant, const Options& opt)
{
    FusedVariant fv;
    const size_t lds_max = 160 * 1024 - VXH_FUSED_STATIC_LDS;
    const int n = M.nvox;
    if (n == 0 || n > 1024 || M.bond_classes.size() > 4095) return fv;   // (12 class bits in a bond entry; a robot of 1024 voxels has at most 3072 bonds)
    if (wide_listed(M, variant, opt)) {
        // the wide kernel when its LDS layout fits (mirrors the top of k_robot_wide): pose tile, record region, class tables,
        // the strain tile of a land_water robot, the mask + pool of the contact rows
        const WideLayout W = wide_layout(M, variant);
        const int mesh = M.nmv > 0 ? 1 : 0;
        auto wneed = [&](bool tables_in_lds) {
            return (size_t)(8 * WIDE_BLOCK + W.region) * 8 +
                   (tables_in_lds ? M.bond_classes.size() * sizeof(DBondClass) + M.vox_classes.size() * sizeof(DVoxClass) : 0) +
                   (mesh ? (size_t)48 * WIDE_BLOCK : 0) + (M.vxa.self_col_enabled ? (size_t)8 * WIDE_BLOCK : 0);
        };
        const int wtabg = wneed(true) > lds_max ? 1 : 0;
        if (wneed(!wtabg) <= lds_max) {
            fv.block = WIDE_BLOCK; fv.nacc = 0; fv.fluid = mesh; fv.tabg = wtabg; fv.wide = 1; fv.lds = wneed(!wtabg);
            // a second pose tile (64 B per thread) where the layout leaves room for it and, for a colliding robot, for at least
            // 8 KB of contact rows: the step then has two workgroup barriers instead of three (kernels_wide.hpp)
            const size_t tile = (size_t)64 * WIDE_BLOCK, rows_min = M.vxa.self_col_enabled ? (size_t)8 * 1024 : 0;
            if (opt.wide_two_tiles && fv.lds + tile + rows_min <= lds_max) fv.two_tiles = 1;
            const size_t room = lds_max - (fv.two_tiles ? tile : 0);
            if (M.vxa.self_col_enabled && room > fv.lds) fv.lds += std::min<size_t>(room - fv.lds, (size_t)24 * 1024);
            fv.lds &= ~(size_t)7;
            if (fv.two_tiles) fv.lds += tile;
            return fv;
        }
    }
    const int block = resident_block(n);
    const int fluid = M.nmv > 0 ? 1 : 0;      // (the MESH variants: every land_water robot carries the surface mesh)
    const bool in_fluid = variant == 1 && M.vxa.fluid_env;
    // LDS need: pose tile, accumulator tiles, actuation phases; class tables; the mesh vertices of a robot in a
    // fluid; with two accumulator tiles the MESH variants also hold the strain tile (with one it stays in HBM)
    // (mirrors the layout at the top of k_robot_steps; SLIM = the 768-thread MESH variant, phases and strains in HBM)
    const bool slim = fluid && block == 768;
    auto need = [&](int nacc, bool tables_in_lds) {
        return (size_t)(8 + 6 * nacc + (slim ? 0 : 2)) * block * 8 +
               (tables_in_lds ? M.bond_classes.size() * sizeof(DBondClass) + M.vox_classes.size() * sizeof(DVoxClass) : 0) +
               (in_fluid ? (size_t)24 * M.nmv : 0) + ((fluid && nacc == 2 && !slim) ? (size_t)48 * block : 0);
    };
    // accumulator tiles: two up to 768 voxels, one for 1024; class tables in LDS unless they do not fit (per-voxel
    // evolved stiffness makes nearly every bond a class of its own), then the TABG variant reads them from HBM
    const int nacc = block == 1024 ? 1 : 2;
    const int tabg = need(nacc, true) > lds_max ? 1 : 0;
    if (need(nacc, !tabg) > lds_max) return fv;                   // (e.g. a mesh with thousands of vertices)
    fv.block = block; fv.nacc = nacc; fv.fluid = fluid; fv.tabg = tabg; fv.lds = need(nacc, !tabg);
    // colliding robots: what the workgroup can spare without lowering the number of workgroups a CU holds (two of the 256-thread
    // variant, by its registers; one of the others) takes the contact rows, 12 bytes per listed pair
    if (M.vxa.self_col_enabled) {
        const size_t room = (block == 256 ? (size_t)80 * 1024 - VXH_FUSED_STATIC_LDS : lds_max);
        if (room > fv.lds) fv.lds += std::min<size_t>(room - fv.lds, (size_t)24 * 1024);
    }
    fv.lds &= ~(size_t)7;
    return fv;
}

// ---- assemble_batch: the per-robot offsets into every shared table, then each robot's part of the tables ----
namespace {

// voxel, surface and trace ranges of the robots, and the tables that are sized by them
void lay_out_voxels(const std::vector<RobotModel>& robots, int variant, HostBatch& H)
{
    const int nr = (int)robots.size();
    H.robot.assign(nr, DRobot{});
    H.vox_begin.assign(nr, 0);
    H.surf_begin.assign(nr, 0);
    int nv = 0, ns = 0;
    for (int r = 0; r < nr; ++r) {
        H.vox_begin[r] = nv;
        H.surf_begin[r] = ns;
        nv += (robots[r].nvox + 63) / 64 * 64;
        ns += robots[r].vxa.self_col_enabled ? robots[r].nsurf : 0;
        if (robots[r].nvox > 0) H.max_planned = std::max(H.max_planned, robots[r].planned_steps);
        H.max_nvox = std::max(H.max_nvox, robots[r].nvox);
    }
    if (nv == 0) nv = 64;
    // the kernels address a component plane as 32-bit `plane * nv + slot` (up to 36 planes of bond slots)
    if ((long long)nv * 36 >= (1LL << 32))
        throw std::invalid_argument("batch too large for one engine (" + std::to_string(nv) + " voxel slots; limit 119 million): split the population");
    H.nv = nv; H.ns = ns;
    // centre-of-mass traces (<TimeBetweenTraces>): one entry at most every trace_dt of simulated time after InitCmTime
    H.trace_begin.assign(nr, 0); H.trace_cap.assign(nr, 0); H.total_trace = 0;
    for (int r = 0; r < nr; ++r) {
        const RobotModel& M = robots[r];
        H.trace_begin[r] = H.total_trace;
        if (variant == 0 && M.vxa.time_between_traces > 0 && M.nvox > 0) {
            const double span = std::max(0.0, (double)M.planned_steps * M.dt - M.vxa.init_cm_time);
            const double n = span / M.vxa.time_between_traces + 8;
            if (!(n < 4e6)) throw std::invalid_argument("TimeBetweenTraces asks for more than 4 million trace points");
            H.trace_cap[r] = (int)n;
            H.total_trace += H.trace_cap[r];
        }
    }
    // <NormDistByVol>: a volume per point of that trace, and the after-life / frozen traces (DBatch::trace_vol, xtrace), sized the same way
    // from the spans in which UpdateStats can record them (VX_Sim.cpp:1549-1565): AfterlifeTime, MidLifeFreezeTime
    H.vol_begin.assign(nr, 0);
    H.total_vol = 0; H.total_xtrace = 0;
    for (int k = 0; k < 2; ++k) { H.xt_begin[k].assign(nr, 0); H.xt_cap[k].assign(nr, 0); }
    for (int r = 0; r < nr; ++r) {
        const RobotModel& M = robots[r];
        H.vol_begin[r] = H.total_vol;
        for (int k = 0; k < 2; ++k) H.xt_begin[k][r] = H.total_xtrace;
        if (!(variant == 0 && M.vxa.norm_dist_by_vol && H.trace_cap[r] > 0)) continue;
        H.total_vol += H.trace_cap[r];
        const double span[2] = { std::max(0.0, M.vxa.afterlife_time), std::max(0.0, M.vxa.midlife_freeze_time) };
        for (int k = 0; k < 2; ++k) {
            H.xt_begin[k][r] = H.total_xtrace;
            if (!(span[k] > 0)) continue;
            const double n = span[k] / M.vxa.time_between_traces + 8;
            if (!(n < 4e6)) throw std::invalid_argument("TimeBetweenTraces asks for more than 4 million trace points");
            H.xt_cap[k][r] = (int)n;
            H.total_xtrace += H.xt_cap[k][r];
        }
    }

    H.wave_robot.assign(nv / 64, -1); H.nbr.assign((size_t)6 * nv, -1);
    H.surf.assign(std::max(ns, 1), 0); H.surf_code.assign(std::max(ns, 1), 0); H.surf_ord.assign(nv, -1);
    H.vclass.assign(nv, 0);
    H.bclass.assign((size_t)3 * nv, -1);
    H.sched_off.assign(nr + 1, 0);
    for (int r = 0; r < nr; ++r)
        H.sched_off[r + 1] = H.sched_off[r] + ((robots[r].nvox > 0 && robots[r].nvox <= 1024) ? 3 * resident_block(robots[r].nvox) : 0);
    H.bsched.assign(std::max(H.sched_off[nr], 1), -1);
    H.wgather.assign((size_t)2 * nv, 0);
    H.amp_damp.assign(nv, 1.f);
    H.act_sb.assign(nv, 0.0); H.act_cb.assign(nv, 1.0);
    for (int r = 0; r < nr; ++r) H.any_dev = H.any_dev || robots[r].development;
    H.dev.assign(H.any_dev ? (size_t)7 * nv : 7, 0.f);
    H.px.assign(nv, 0); H.py.assign(nv, 0); H.pz.assign(nv, 0); H.sc.assign(nv, 0); H.qw.assign(nv, 1.0);
    H.small.assign((size_t)3 * nv, 1);
    H.rstate.resize(nr);
}

// ... the surface meshes of land_water robots
void lay_out_meshes(const std::vector<RobotModel>& robots, int variant, HostBatch& H)
{
    const int nr = (int)robots.size(), nv = H.nv;
    H.mv_begin.assign(nr, 0);
    for (int r = 0; r < nr; ++r) { H.mv_begin[r] = H.total_mv; H.total_mv += robots[r].nmv; H.any_mesh = H.any_mesh || robots[r].nmv > 0; }
    const int total_mv = H.total_mv;
    H.vert_pack.assign((size_t)3 * std::max(total_mv, 1), 0);
    for (int r = 0; r < nr; ++r) H.any_fluid = H.any_fluid || (variant == 1 && robots[r].vxa.fluid_env && robots[r].nmv > 0);
    const bool any_fluid = H.any_fluid;
    H.vert_vox.assign(any_fluid ? (size_t)8 * std::max(total_mv, 1) : 8, -1); H.vert_robot.assign(any_fluid ? std::max(total_mv, 1) : 1, 0);
    H.vert_v0.assign((size_t)3 * std::max(total_mv, 1), 0.0);
    H.facet_begin.assign(nr, 0);
    for (int r = 0; r < nr; ++r) { H.facet_begin[r] = H.total_facet; H.total_facet += (int)robots[r].facet_vox.size(); }
    const int total_facet = H.total_facet;
    H.facet_vox.assign(std::max(total_facet, 1), 0); H.facet_vert.assign((size_t)3 * std::max(total_facet, 1), 0); H.facet_first.assign(H.any_mesh ? nv : 1, 0);
    H.facet_count.assign(H.any_mesh ? nv : 1, 0);
    H.facet_robot.assign(any_fluid ? std::max(total_facet, 1) : 1, 0);
}

// ... and the class tables, exclusion rows, contact rows and wide-kernel lists
void lay_out_tables(const std::vector<RobotModel>& robots, int variant, const Options& opt, size_t device_mem, HostBatch& H)
{
    const int nr = (int)robots.size();
    H.vtab_off.assign(nr + 1, 0); H.btab_off.assign(nr + 1, 0); H.wl_off.assign(nr + 1, 0);
    H.excl_off.assign(nr + 1, 0); H.col_off.assign(nr + 1, 0);
    H.col_cap.assign(nr, 0);
    H.img_idx.assign(nr, -1);
    { int n_img = 0; for (int r = 0; r < nr; ++r) if (robots[r].vxa.self_col_enabled && robots[r].nvox > 0 && robots[r].nvox <= 1024) H.img_idx[r] = n_img++; }
    // contact rows: as long as the physics makes them -- a surface voxel can list every other one (CreateColBond, VX_Sim.cpp:753-769,
    // has no cap) -- unless the option col_cap bounds them; 12-16 bytes per entry, untouched beyond the partners a row really has.
    // That is nsurf^2 entries of address space per robot (75 MB for a 20^3 lattice, 1.5 GB for 512 robots of 10^3: nothing on this
    // device), but it grows with the FOURTH power of a lattice's edge: when the uncapped rows of a batch would take more than a third of
    // the device's free memory (a lattice of 100^3 and beyond) every robot's rows are cut to an equal share of that third, never
    // below 64, and the engine says so -- a row that then overflows gives its robot VXH_ROBOT_COL_OVERFLOW, as with a col_cap of the
    // user's.  (Round 3 allocated nsurf^2 whatever the size and ran out of memory in this function for lattices it used to step.)
    long long row_limit = 0x7fffffff;
    if (opt.col_cap <= 0) {
        double want = 0, rows = 0;
        for (int r = 0; r < nr; ++r) if (robots[r].vxa.self_col_enabled) { want += 16.0 * (double)robots[r].nsurf * (double)std::max(1, robots[r].nsurf - 1); rows += robots[r].nsurf; }
        // (the budget is a third of the device's TOTAL memory, not of what happens to be free: how long a row can grow -- and with it whether a
        // robot ends FINISHED or COL_OVERFLOW -- must not depend on what other processes hold on the GPU at this moment; if the rows then do
        // not fit what IS free, the allocation fails with an error instead of changing outcomes silently.  ADVICE round 4)
        if (want > 0 && device_mem > 0 && want > (double)device_mem / 3.0) {
            row_limit = std::max<long long>(64, (long long)((double)device_mem / 3.0 / 16.0 / std::max(1.0, rows)));
            std::fprintf(stderr, "vxhip: the contact rows of this batch would take %.1f GB uncapped (device memory: %.1f GB); rows are cut to %lld partners "
                                 "(option col_cap sets the length; a robot whose row overflows ends with status COL_OVERFLOW)\n", want / 1e9, (double)device_mem / 1e9, row_limit);
        }
    }
    for (int r = 0; r < nr; ++r) {
        const RobotModel& M = robots[r];
        if (M.vox_classes.size() > 32767 || M.bond_classes.size() > 32767) throw std::runtime_error("too many distinct voxel/bond classes in one robot");
        H.vtab_off[r + 1] = H.vtab_off[r] + (int)M.vox_classes.size();
        H.btab_off[r + 1] = H.btab_off[r] + (int)M.bond_classes.size();
        H.excl_off[r + 1] = H.excl_off[r] + (M.vxa.self_col_enabled ? (long long)M.nsurf * ((M.nsurf + 63) / 64) : 0);
        H.col_cap[r] = M.vxa.self_col_enabled ? std::max(1, opt.col_cap > 0 ? std::min(opt.col_cap, M.nsurf - 1) : (int)std::min<long long>(row_limit, M.nsurf - 1)) : 0;
        H.col_off[r + 1] = H.col_off[r] + (long long)H.col_cap[r] * (M.vxa.self_col_enabled ? M.nsurf : 0);
        H.wl_off[r + 1] = H.wl_off[r] + (wide_listed(M, variant, opt) ? M.nbond : 0);
    }
    H.wlist.assign(std::max(H.wl_off[nr], 1), -1);
    H.col_total = H.col_off[nr];
    H.vtab.resize(H.vtab_off[nr]);
    H.btab.resize(H.btab_off[nr]);
    H.excl.assign((size_t)H.excl_off[nr], 0ull);
}

void class_tables(const RobotModel& M, int r, HostBatch& H)
{
    const int vtab_begin = H.vtab_off[r], btab_begin = H.btab_off[r];
    for (size_t i = 0; i < M.vox_classes.size(); ++i) {
        const VoxClass& c = M.vox_classes[i];
        DVoxClass d;
        std::memset(&d, 0, sizeof(d));
        d.mass = c.mass; d.mass_inv = c.mass_inv; d.inertia_inv = c.inertia_inv; d.c_lin = c.c_lin; d.c_ang = c.c_ang;
        d.E = c.E; d.k_floor = c.k_floor; d.u_static = c.u_static; d.u_dynamic = c.u_dynamic; d.cte = c.cte;
        d.nom_size = c.nom_size; d.mat = c.mat;
        d.prenatal_k = ((double)(float)c.nom_size / c.nom_size) - 1;
        H.vtab[vtab_begin + i] = d;
    }
    for (size_t i = 0; i < M.bond_classes.size(); ++i) {
        const BondClass& c = M.bond_classes[i];
        DBondClass d;
        std::memset(&d, 0, sizeof(d));
        const double zi = (0.5 * M.vxa.bond_damping_z) * (1.0 / M.dt), zh = 0.5 * zi;   // BondDampingZ/2 (moments: /4) over dt
        d.L100 = 100.0 * c.L; d.a2 = c.a2; d.b1 = c.b1; d.b2 = c.b2; d.b3 = c.b3;
        d.kf_L = c.stress_k * c.area_sum / 2 / c.L; d.strain_a1_L = c.strain_a1 / c.L; d.strain_a2_L = c.strain_a2 / c.L;
        d.dA1 = c.sq_a1m1 * zi; d.dB1 = c.sq_b1m1 * zi; d.dF1 = c.sq_b2fm1 * zi;
        d.dA2 = c.sq_a1m2 * zi; d.dB2 = c.sq_b1m2 * zi; d.dF2 = c.sq_b2fm2 * zi;
        d.dT1 = c.sq_a2i1 * zh; d.dG1 = c.sq_b2fm1 * zh; d.dH1 = c.sq_b3i1 * zh;
        d.dT2 = c.sq_a2i2 * zh; d.dG2 = c.sq_b2fm2 * zh; d.dH2 = c.sq_b3i2 * zh;
        d.homogeneous = c.homogeneous;
        H.btab[btab_begin + i] = d;
    }
    DRobot& R = H.robot[r];
    R.vtab_begin = vtab_begin; R.n_vclass = (int)M.vox_classes.size(); R.btab_begin = btab_begin; R.n_bclass = (int)M.bond_classes.size();
}

void voxel_planes(const RobotModel& M, int r, HostBatch& H)
{
    const int base = H.vox_begin[r], nv = H.nv;
    for (int w = base / 64; w < (base + (M.nvox + 63) / 64 * 64) / 64; ++w) H.wave_robot[w] = r;
    for (int v = 0; v < M.nvox; ++v) {
        const int g = base + v;
        H.vclass[g] = (unsigned short)M.vox_class[v];
        { const double b = (double)(2 * 3.1415926f) * (double)M.phase_offset[v]; H.act_sb[g] = std::sin(b); H.act_cb[g] = std::cos(b); }
        H.amp_damp[g] = M.temp_amp_damp[v];
        if (M.development) {
            const float vals[7] = {M.initial_voxel_size[v], M.final_voxel_size[v], M.start_growth_time[v], M.growth_time[v],
                                   M.phase_offset[v], M.final_phase_offset[v], M.final_temp_amp_damp[v]};
            for (int k = 0; k < 7; ++k) H.dev[(size_t)k * nv + g] = vals[k];
        }
        H.px[g] = M.nom_pos[3 * v]; H.py[g] = M.nom_pos[3 * v + 1]; H.pz[g] = M.nom_pos[3 * v + 2];
        H.sc[g] = M.vox_classes[M.vox_class[v]].nom_size;
        for (int d = 0; d < 6; ++d) { int o = M.nbr[(size_t)v * 6 + d]; H.nbr[(size_t)d * nv + g] = o < 0 ? -1 : base + o; }
        for (int a = 0; a < 3; ++a) { int c = M.bond_class[(size_t)v * 3 + a]; H.bclass[(size_t)a * nv + g] = c < 0 ? (short)-1 : (short)c; }
    }
}

void resident_schedule(const RobotModel& M, int r, HostBatch& H)
{
    H.robot[r].sched_begin = H.sched_off[r];
    if (!(M.nvox > 0 && M.nvox <= 1024 && M.bond_classes.size() <= 4095)) return;
    // The resident kernel's bond schedule.  X and Z: bond j of the axis' compacted list to thread j.  Y: the kernel variants
    // with two accumulator tiles (up to 768 threads) evaluate X and Y without a barrier between them -- an accumulator entry
    // gets at most one X and one Y contribution per tile, both added to zero with LDS atomics, and a + b == b + a, so the sums
    // are those of the barrier-separated rounds bit for bit -- and a wavefront's bond is a latency-bound chain (a lone
    // wavefront issues a dependent FP64 instruction every ~7 cycles, three that share a SIMD one every ~4): the 64-bond
    // chunks of Y are dealt to the wavefronts that X leaves idle, least-loaded SIMD first (wavefront w runs on SIMD w mod 4),
    // so that X + Y occupy every SIMD with three to four chunk executions spread over its three wavefronts instead of
    // two rounds of two.  The 1024-thread variant (one tile, two barrier-separated sub-steps per round) keeps Y in list order.
    const int block = resident_block(M.nvox), nw = block / 64;
    int* sx = &H.bsched[H.sched_off[r]], *sy = sx + block, *sz = sy + block;
    std::vector<int> list[3];
    for (int a = 0; a < 3; ++a)
        for (int v = 0; v < M.nvox; ++v) {
            const int c = M.bond_class[(size_t)v * 3 + a];
            if (c >= 0) list[a].push_back((int)((unsigned)v | ((unsigned)M.nbr[(size_t)v * 6 + 2 * a] << 10) | ((unsigned)c << 20)));
        }
    for (size_t j = 0; j < list[0].size(); ++j) sx[j] = list[0][j];
    for (size_t j = 0; j < list[2].size(); ++j) sz[j] = list[2][j];
    if (block == 1024) { for (size_t j = 0; j < list[1].size(); ++j) sy[j] = list[1][j]; }
    else {
        const int nchx = ((int)list[0].size() + 63) / 64, nchy = ((int)list[1].size() + 63) / 64;
        std::vector<int> simd_load(4, 0), wave_load(nw, 0), has_y(nw, 0);
        for (int w = 0; w < nchx; ++w) { ++simd_load[w % 4]; ++wave_load[w]; }
        for (int c = 0; c < nchy; ++c) {
            int best = -1;
            for (int w = 0; w < nw; ++w) {
                if (has_y[w]) continue;
                if (best < 0 || simd_load[w % 4] < simd_load[best % 4] ||
                    (simd_load[w % 4] == simd_load[best % 4] && wave_load[w] < wave_load[best])) best = w;
            }
            has_y[best] = 1; ++simd_load[best % 4]; ++wave_load[best];
            for (int k = 0; k < 64 && (size_t)(64 * c + k) < list[1].size(); ++k) sy[64 * best + k] = list[1][(size_t)64 * c + k];
        }
    }
}

void wide_lists(const RobotModel& M, int r, int variant, const Options& opt, HostBatch& H)
{
    DRobot& R = H.robot[r];
    const int base = H.vox_begin[r];
    R.wl_begin = H.wl_off[r]; R.wnbond = 0; R.wzidx = 0; R.wregion = 0;
    if (!wide_listed(M, variant, opt)) return;
    // wide kernel: all bonds in one list, axis after axis; a bond's place in it is the number of its record, and every voxel
    // learns the records of its six directions (+A: the bond it is the negative end of; -A: that of its -A neighbour)
    const WideLayout W = wide_layout(M, variant);
    std::vector<int> slot_of((size_t)M.nvox * 3, -1);
    int t = 0;
    for (int a = 0; a < 3; ++a)
        for (int v = 0; v < M.nvox; ++v) {
            const int c = M.bond_class[(size_t)v * 3 + a];
            if (c < 0) continue;
            slot_of[(size_t)v * 3 + a] = t;
            H.wlist[H.wl_off[r] + t++] = (int)((unsigned)v | ((unsigned)M.nbr[(size_t)v * 6 + 2 * a] << 9) | ((unsigned)a << 18) | ((unsigned)c << 20));
        }
    for (int v = 0; v < M.nvox; ++v) {
        int idx[6];
        for (int a = 0; a < 3; ++a) {
            idx[2 * a] = slot_of[(size_t)v * 3 + a];
            const int n = M.nbr[(size_t)v * 6 + 2 * a + 1];
            idx[2 * a + 1] = n >= 0 ? slot_of[(size_t)n * 3 + a] : -1;
        }
        for (int d = 0; d < 6; ++d) if (idx[d] < 0) idx[d] = W.zidx;
        H.wgather[base + v] = idx[0] | (idx[1] << 10) | (idx[2] << 20);
        H.wgather[(size_t)H.nv + base + v] = idx[3] | (idx[4] << 10) | (idx[5] << 20);
    }
    R.wnbond = M.nbond; R.wzidx = W.zidx; R.wregion = W.region;
}

void surface_rows(const RobotModel& M, int r, HostBatch& H)
{
    DRobot& R = H.robot[r];
    const int base = H.vox_begin[r];
    if (M.vxa.self_col_enabled)
        for (int i = 0; i < M.nsurf; ++i) {
            H.surf[H.surf_begin[r] + i] = base + M.surf[i]; H.surf_ord[base + M.surf[i]] = i;
            H.surf_code[H.surf_begin[r] + i] = (int)((unsigned)M.surf[i] | ((unsigned)M.vox_class[M.surf[i]] << 10));     // (robots the resident kernels take: < 1024 voxels)
        }
    // CalcNearby exclusion lists as bit rows over surface ordinals
    const long long excl_begin = H.excl_off[r];
    int wpr = 0;
    if (M.vxa.self_col_enabled) {
        wpr = (M.nsurf + 63) / 64;
        std::vector<int> ord(M.nvox, -1);
        for (int i = 0; i < M.nsurf; ++i) ord[M.surf[i]] = i;
        for (int i = 0; i < M.nsurf; ++i) {
            const int vi = M.surf[i];
            for (int k = M.near_off[vi]; k < M.near_off[vi + 1]; ++k) {
                const int j = ord[M.near_idx[k]];
                if (j >= 0) H.excl[(size_t)excl_begin + (size_t)i * wpr + (j >> 6)] |= 1ull << (j & 63);
            }
        }
    }
    R.excl_wpr = wpr; R.excl_begin = excl_begin;
    R.col_begin = H.col_off[r]; R.col_cap = H.col_cap[r];
    R.surf_begin = H.surf_begin[r]; R.nsurf = M.vxa.self_col_enabled ? M.nsurf : 0;
}

void mesh_tables(const RobotModel& M, int r, HostBatch& H)
{
    DRobot& R = H.robot[r];
    const int base = H.vox_begin[r], mv_begin = H.mv_begin[r], facet_begin = H.facet_begin[r];
    R.vert_begin = mv_begin; R.nmv = M.nmv;
    R.facet_begin = facet_begin; R.nfacet = (int)M.facet_vox.size();
    for (size_t f = 0; f < M.facet_vox.size(); ++f) {
        H.facet_vox[facet_begin + f] = M.facet_vox[f];
        if (H.any_fluid) H.facet_robot[facet_begin + f] = r;
        for (int k = 0; k < 3; ++k) H.facet_vert[(size_t)k * std::max(H.total_facet, 1) + facet_begin + f] = M.facet_vert[f * 3 + k];
    }
    if (M.nmv == 0) return;
    const size_t tm = (size_t)std::max(H.total_mv, 1);
    for (int i = 0; i < M.nmv; ++i) {
        unsigned w[3] = {0, 0, 0};
        for (int q = 0; q < 8; ++q) {
            const int c = M.vert_comp[(size_t)i * 8 + q];
            if (c < 0 || M.nvox > 1024) continue;       // (only the fused path, robots <= 1024 voxels, reads it)
            const unsigned corner = (unsigned)c & 7u, l = (unsigned)c >> 3;
            w[corner / 3] |= l << (10 * (corner % 3));
            w[2] |= 1u << (20 + corner);
        }
        for (int k = 0; k < 3; ++k) H.vert_pack[k * tm + mv_begin + i] = (int)w[k];
        if (H.any_fluid) {
            H.vert_robot[mv_begin + i] = r;
            for (int q = 0; q < 8; ++q) {
                const int c = M.vert_comp[(size_t)i * 8 + q];
                if (c >= 0) H.vert_vox[(size_t)(c & 7) * tm + mv_begin + i] = base + (c >> 3);
            }
        }
        for (int k = 0; k < 3; ++k) H.vert_v0[k * tm + mv_begin + i] = M.vert_v0[(size_t)i * 3 + k];
    }
    for (int v = 0; v < M.nvox; ++v) {
        H.facet_first[base + v] = M.facet_first[v]; H.facet_count[base + v] = M.facet_count[v];
    }
}

void robot_scalars(const RobotModel& M, int r, int variant, HostBatch& H)
{
    const VxaModel& X = M.vxa;
    DRobot& R = H.robot[r];
    R.img_index = H.img_idx[r];
    R.vox_begin = H.vox_begin[r]; R.nvox = M.nvox;
    R.flags = (X.self_col_enabled ? RF_SELF_COL : 0) | (X.grav_enabled ? RF_GRAV : 0) | (X.floor_enabled ? RF_FLOOR : 0) |
              (X.temp_enabled ? RF_TEMP : 0) | ((X.sticky_floor && variant == 0) ? RF_STICKY : 0) |
              ((variant == 1 && X.fluid_env) ? RF_FLUID : 0) | (variant == 1 ? RF_LW : 0) |
              ((X.col_system == 2 || X.col_system == 3) ? RF_HORIZON_COL : 0) |
              (M.development ? RF_DEV : 0) | ((X.has_initial_voxel_size || X.has_final_voxel_size) ? RF_DEV_SIZE : 0) |
              (X.has_final_voxel_size ? RF_DEV_FSIZE : 0) | (X.has_final_phase_offset ? RF_DEV_FPHASE : 0) |
              (X.has_final_temp_amp_damp ? RF_DEV_FTAD : 0) |
              ((variant == 0 && X.norm_dist_by_vol && H.trace_cap[r] > 0) ? RF_NORM_VOL : 0);
    R.stop_type = X.stop_type;
    R.dt = M.dt; R.lat = X.lattice_dim; R.bond_z_half = 0.5 * X.bond_damping_z; R.slow_z = X.slow_damping_z; R.col_z = X.col_damping_z;
    R.grav_acc = X.grav_acc; R.init_cm_time = X.init_cm_time; R.stop_value = X.stop_value;
    R.afterlife = variant == 0 ? X.afterlife_time : 0.0;
    R.temp_period_d = X.temp_period; R.min_temp_fact = X.min_temp_fact; R.growth_amplitude = X.growth_amplitude;
    R.col_horizon = X.collision_horizon;
    { double fd = X.collision_horizon * 1.5 * X.lattice_dim; R.filter_dist2 = fd * fd; }
    R.drag_coef = X.aggregate_drag_coef;
    R.midlife_freeze_time = X.midlife_freeze_time;
    R.trace_dt = H.trace_cap[r] > 0 ? X.time_between_traces : 0.0; R.trace_begin = H.trace_begin[r]; R.trace_cap = H.trace_cap[r];
    R.vol_begin = H.vol_begin[r];
    for (int k = 0; k < 2; ++k) { R.xt_begin[k] = H.xt_begin[k][r]; R.xt_cap[k] = H.xt_cap[k][r]; }
    R.temp_amplitude = (float)X.temp_amplitude; R.temp_period = (float)X.temp_period;
    DRobotState& S = H.rstate[r];
    std::memset(&S, 0, sizeof(S));
    S.max_disp = (double)FLT_MAX;      // ClearAll, VX_Sim.cpp:369: forces a collision-list build on the first step
    S.act_time = -1.0;
    S.status = M.nvox == 0 ? 3 : 0;
}

void assemble_robot(const RobotModel& M, int r, int variant, const Options& opt, HostBatch& H)
{
    class_tables(M, r, H);
    voxel_planes(M, r, H);
    resident_schedule(M, r, H);
    wide_lists(M, r, variant, opt, H);
    surface_rows(M, r, H);
    mesh_tables(M, r, H);
    robot_scalars(M, r, variant, H);
}

}  // namespace

HostBatch assemble_batch(const std::vector<RobotModel>& robots, int variant, const Options& opt, size_t device_mem)
{
    HostBatch H;
    lay_out_voxels(robots, variant, H);
    lay_out_meshes(robots, variant, H);
    lay_out_tables(robots, variant, opt, device_mem, H);
    // the robots are assembled on the host cores (disjoint ranges)
    const int nr = (int)robots.size();
    for_each_index(nr, std::min(nr / 8, 32), [&](int r) { assemble_robot(robots[r], r, variant, opt, H); });
    return H;
}

// ---- plan_launches: which robots are tiled and how, the tile launches, the launch groups, what is left to the streaming kernels ----
namespace {

bool in_fluid(const RobotModel& M, int variant) { return variant == 1 && M.vxa.fluid_env && M.nmv > 0; }

// Which robots are tiled.  By default only those the resident kernel cannot take (more than 1024 voxels, oversized tables): the
// kernel that steps a robot is then a function of the robot ALONE, and so is its trajectory, bit for bit, whatever the batch --
// a robot re-evaluated alone gives the bits it gave inside a generation of 512 (tests/test_gpu_parity.py
// test_full_size_batch_properties; the tiled and the resident kernel agree to 1e-12 voxel, not to the bit).
// Option tile_small = 1 gives that up for speed where it was measured to pay (scripts/dev_gpu_diag.py tilepolicy, one box, us per
// population step, resident | tiled): 64 robots of 6^3 10.2 | 11.1, 7^3 11.0 | 11.3, 8^3 11.1 | 11.7, 9^3 13.7 | 14.2, 10^3 15.6 |
// 14.7; 16 of 10^3 15.1 | 13.2; 128 of 8^3 11.3 | 14.0; 128 of 10^3 16.0 | 32.9 (their tiles no longer fit one co-resident
// launch) -- i.e. large robots (the 768- and 1024-thread variants) in populations of at most a quarter of the CUs.  (Until late in
// round 2 the default was "any robot, up to three quarters of the CUs": slower for every size below 10^3, 2x slower at 128 robots,
// and population-dependent in the last bits.)
std::vector<int> tile_candidates(const std::vector<RobotModel>& robots, int variant, const Options& opt, int tiled_now, int n_cu)
{
    const int nr = (int)robots.size();
    int n_work = 0;
    for (int r = 0; r < nr; ++r) if (robots[r].nvox > 0) ++n_work;
    const bool small_population = opt.tile_small && n_work * 4 <= n_cu;
    std::vector<int> cand;
    for (int r = 0; r < nr; ++r) {
        const RobotModel& M = robots[r];
        // land_water robots are tiled on land (round 4: the tiles keep the directional strains the RobotVolume tags need) and, since
        // round 5, in a FLUID: the tile then carries its part of the drag mesh, and the voxels a mesh vertex averages over -- up to
        // seven, across tile boundaries, diagonal neighbours included -- come through the exchange buffer with their strains
        if (M.nvox == 0) continue;
        const int block = fused_variant(M, variant, opt).block;
        if (tiled_now == 2 || !opt.fused || block == 0 || (small_population && block >= 768)) cand.push_back(r);
    }
    return cand;
}

// a robot in a fluid: per tile the mesh vertices its owned voxels' facets use and those facets (counts, for the LDS layout; the tables
// themselves are filled when the exchange slots of the robot's voxels are known)
void tile_mesh_counts(const RobotModel& M, int variant, const TilePlan::Tile& t, int& n_mv, int& n_f, int& n_mx)
{
    n_mv = n_f = n_mx = 0;
    if (!in_fluid(M, variant)) return;
    std::vector<char> seen(M.nmv, 0), vseen(M.nvox, 0);
    for (int v : t.own)
        for (int f = M.facet_first[v]; f < M.facet_first[v] + (int)M.facet_count[v]; ++f) {
            ++n_f;
            for (int k = 0; k < 3; ++k) {
                const int i = M.facet_vert[(size_t)f * 3 + k];
                if (seen[i]) continue;
                seen[i] = 1; ++n_mv;
                for (int e = 0; e < 8; ++e) { const int c = M.vert_comp[(size_t)i * 8 + e]; if (c >= 0 && !vseen[c >> 3]) { vseen[c >> 3] = 1; ++n_mx; } }
            }
        }
}

struct Planned { int r; TilePlan plan; int tabg; size_t lds; int mesh; int small; };

// one robot, starting from k tiles: more of them until every tile fits the workgroup and its LDS; false: cannot be tiled, left to the other kernels
bool plan_robot_tiles(const RobotModel& M, int r, int variant, int k, Planned& out)
{
    const size_t lds_cap = 160 * 1024 - VXH_TILE_STATIC_LDS;
    const int tab_doubles = (int)(M.bond_classes.size() * sizeof(DBondClass) / 8 + M.vox_classes.size() * sizeof(DVoxClass) / 8);
    const int tabg = (size_t)tab_doubles * 8 > 32 * 1024 ? 1 : 0;
    k = std::max(1, std::min(k, M.nvox / 8));
    for (;;) {
        TilePlan P = plan_tiles(M, k);
        size_t lds = 0;
        bool small = true;                                    // every tile within the SMALL size class: its kernel instances, its (fixed) layout
        for (const auto& t : P.tiles) small = small && (int)t.own.size() <= VXH_TILE_S_OWN && (int)t.halo.size() <= VXH_TILE_S_HALO && (int)t.bond_v1.size() <= VXH_TILE_S_BONDS;
        for (const auto& t : P.tiles) {
            int n_mv = 0, n_f = 0, n_mx = 0;
            tile_mesh_counts(M, variant, t, n_mv, n_f, n_mx);
            const TileLayout TL = small ? tile_layout(VXH_TILE_S_OWN, VXH_TILE_S_HALO, VXH_TILE_S_BONDS, tabg ? 0 : tab_doubles, M.nmv > 0, n_mv, n_f, n_mx)
                                        : tile_layout((int)t.own.size(), (int)t.halo.size(), (int)t.bond_v1.size(), tabg ? 0 : tab_doubles, M.nmv > 0, n_mv, n_f, n_mx);
            lds = std::max(lds, (size_t)TL.total * 8);
        }
        if (P.k > VXH_TILE_MAX_TILES) return false;           // (left to the other kernels)
        if (P.max_own <= VXH_TILE_BLOCK && P.max_local <= 1024 && lds <= lds_cap) { out = Planned{r, std::move(P), tabg, lds, M.nmv > 0 ? (in_fluid(M, variant) ? 2 : 1) : 0, small ? 1 : 0}; return true; }
        if (k >= M.nvox / 8) return false;                    // cannot be tiled: left to the other kernels
        k = std::min(std::max(k + 1, k * 5 / 4 + 1), std::max(1, M.nvox / 8));
    }
}

// tiles per robot: one bond per lane and one WAVEFRONT of owned voxels per tile if the CUs allow it (a step then costs one bond
// evaluation + one voxel update on one wavefront + the barrier), fewer when the candidates outnumber the CUs.  (Until late in
// round 3 only the bonds counted: 112 tiles of 71-72 voxels for the 20^3 lattice -- a second, nearly empty wavefront in every
// voxel phase -- where 125 tiles of 64 step it in 8.7 instead of 10.3 us; scripts/dev_gpu_diag.py cfg4tiles: 64 tiles 11.2,
// 216 tiles 9.1, 250 tiles 8.8.)
std::vector<Planned> plan_candidates(const std::vector<RobotModel>& robots, const std::vector<int>& cand, int variant, const Options& opt, int n_cu)
{
    auto k_bonds = [&](const RobotModel& M) { return std::max(1, (int)((M.nbond * 5LL / 4 + VXH_TILE_BLOCK - 1) / VXH_TILE_BLOCK)); };
    auto k_wave = [&](const RobotModel& M) { return std::max(k_bonds(M), (M.nvox + 63) / 64); };
    long long sum_wave = 0;
    for (int r : cand) sum_wave += k_wave(robots[r]);
    const bool by_wave = sum_wave <= n_cu;       // (else the round-2 rule: by bonds, scaled down to the CUs -- 64 robots of 10^3 with tile_small: 14.3 us, against 16.4 with the wavefront rule scaled down)
    auto k_latency = [&](const RobotModel& M) { return by_wave ? k_wave(M) : k_bonds(M); };
    long long sum_lat = 0;
    for (int r : cand) sum_lat += k_latency(robots[r]);
    std::vector<Planned> planned;
    for (int r : cand) {
        const RobotModel& M = robots[r];
        const int k = opt.tiles_per_robot > 0 ? opt.tiles_per_robot
                                              : (sum_lat <= n_cu ? k_latency(M) : std::max(1, (int)(k_latency(M) * (long long)n_cu / sum_lat)));
        Planned q;
        if (plan_robot_tiles(M, r, variant, k, q)) planned.push_back(std::move(q));
    }
    return planned;
}

// the fluid tiles' mesh tables as they grow tile by tile (fluid_tile_mesh), one vector per plane; upload_form() transposes them into the plan
struct FluidTileTables {
    std::vector<int> tmv_slot[8], tf_owner, tf_vert[3];      // mesh vertices (per corner code), facets
    std::vector<double> tmv_v0[3];
};

// the drag mesh, tile by tile: the vertices the facets of the tile's owned voxels use (every voxel touching such a vertex named
// by its EXCHANGE slot: the vertex pass reads pose and strains of all of them from the exchange buffer, whoever owns them)
// and those facets, per owned voxel in the reference's order
void fluid_tile_mesh(const RobotModel& M, const TilePlan& plan, int tile0, int base, FluidTileTables& F, LaunchPlan& P)
{
    P.any_fluid_tiles = true;
    for (int t = 0; t < plan.k; ++t) {
        DTile& d = P.tiles[tile0 + t];
        const TilePlan::Tile& T = plan.tiles[t];
        std::vector<int> local(M.nmv, -1), verts;
        d.f_off = (int)F.tf_owner.size();
        for (size_t o = 0; o < T.own.size(); ++o) {
            const int v = T.own[o];
            P.tile_ffirst[d.vox_off + o] = (int)F.tf_owner.size() - d.f_off;
            P.tile_fcount[d.vox_off + o] = M.facet_count[v];
            for (int f = M.facet_first[v]; f < M.facet_first[v] + (int)M.facet_count[v]; ++f) {
                F.tf_owner.push_back((int)o);
                for (int c = 0; c < 3; ++c) {
                    const int i = M.facet_vert[(size_t)f * 3 + c];
                    if (local[i] < 0) { local[i] = (int)verts.size(); verts.push_back(i); }
                    F.tf_vert[c].push_back(local[i]);
                }
            }
        }
        d.n_f = (int)F.tf_owner.size() - d.f_off;
        d.mv_off = (int)F.tmv_v0[0].size(); d.n_mv = (int)verts.size();
        d.mx_off = (int)P.tile_mvox.size();
        std::vector<int> vlocal(M.nvox, -1);
        for (int i : verts) {
            int slot[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
            for (int e = 0; e < 8; ++e) {
                const int c = M.vert_comp[(size_t)i * 8 + e];
                if (c < 0) continue;
                const int v = c >> 3;
                if (vlocal[v] < 0) { vlocal[v] = (int)P.tile_mvox.size() - d.mx_off; P.tile_mvox.push_back(P.xslot[base + v]); }
                slot[c & 7] = vlocal[v];
            }
            for (int c = 0; c < 8; ++c) F.tmv_slot[c].push_back(slot[c]);
            for (int c = 0; c < 3; ++c) F.tmv_v0[c].push_back(M.vert_v0[(size_t)i * 3 + c]);
        }
        d.n_mx = (int)P.tile_mvox.size() - d.mx_off;
    }
}

void upload_form(const FluidTileTables& F, LaunchPlan& P)
{
    const size_t nm = F.tmv_v0[0].size(), nf = F.tf_owner.size();
    P.tile_mvert.assign(std::max<size_t>(1, 8 * nm), -1); P.tile_facet.assign(std::max<size_t>(1, 4 * nf), 0);
    P.tile_mv0.assign(std::max<size_t>(1, 3 * nm), 0.0);
    for (int c = 0; c < 8; ++c) for (size_t i = 0; i < nm; ++i) P.tile_mvert[(size_t)c * nm + i] = F.tmv_slot[c][i];
    for (int c = 0; c < 3; ++c) for (size_t i = 0; i < nm; ++i) P.tile_mv0[(size_t)c * nm + i] = F.tmv_v0[c][i];
    for (size_t f = 0; f < nf; ++f) { P.tile_facet[f] = F.tf_owner[f]; for (int c = 0; c < 3; ++c) P.tile_facet[(size_t)(c + 1) * nf + f] = F.tf_vert[c][f]; }
    P.tile_ffirst.resize(std::max<size_t>(1, P.tile_vox.size()), 0); P.tile_fcount.resize(std::max<size_t>(1, P.tile_vox.size()), 0);
    P.n_tmv = (int)nm; P.n_tf = (int)nf;
    if (P.tile_mvox.empty()) P.tile_mvox.push_back(0);
}

// the tiles of one planned robot appended to the tile tables and to the launch `cur`
void append_robot_tiles(const RobotModel& M, const Planned& q, const HostBatch& H, int variant, TileLaunchPlan& cur, FluidTileTables& F, LaunchPlan& P)
{
    const int k = q.plan.k, nv = H.nv;
    const int tile0 = (int)P.tiles.size(), base = H.vox_begin[q.r];
    for (int t = 0; t < k; ++t) {
        const TilePlan::Tile& T = q.plan.tiles[t];
        DTile d;
        d.robot = q.r; d.tile0 = tile0; d.ntiles = k;
        d.n_own = (int)T.own.size(); d.n_halo = (int)T.halo.size(); d.nb = (int)T.bond_v1.size();
        d.vox_off = (int)P.tile_vox.size(); d.bond_off = (int)P.tile_bond.size();
        d.xoff = P.nx_total; d.pad = 0; d.mv_off = d.n_mv = d.f_off = d.n_f = d.mx_off = d.n_mx = 0;
        for (size_t i = 0; i < T.own.size(); ++i) { P.tile_vox.push_back(base + T.own[i]); P.xslot[base + T.own[i]] = P.nx_total + (int)i; }
        P.nx_total += ((int)T.own.size() + 63) / 64 * 64;
        for (int v : T.halo) P.tile_vox.push_back(-(base + v) - 1);      // (exchange slots once every tile of the robot has its range)
        for (size_t b = 0; b < T.bond_v1.size(); ++b) {
            P.tile_bond.push_back(T.bond_entry[b]);
            P.tile_bcls.push_back(M.bond_class[(size_t)T.bond_v1[b] * 3 + T.bond_axis[b]]);
            P.tile_bslot.push_back(T.bond_axis[b] * nv + base + T.bond_v1[b]);
        }
        cur.tile_ids.push_back((int)P.tiles.size());
        P.tiles.push_back(d);
    }
    for (int t = 0; t < k; ++t) {                          // halo voxels: global slot -> exchange slot
        const DTile& d = P.tiles[tile0 + t];
        for (int i = 0; i < d.n_halo; ++i) { int& e = P.tile_vox[d.vox_off + d.n_own + i]; e = P.xslot[-(e + 1)]; }
    }
    P.tile_ffirst.resize(P.tile_vox.size(), 0); P.tile_fcount.resize(P.tile_vox.size(), 0);
    if (in_fluid(M, variant)) fluid_tile_mesh(M, q.plan, tile0, base, F, P);
    cur.count += k;
    cur.robots.push_back(q.r);
    P.robot_tiled[q.r] = 1;
    P.robot_tiles[q.r] = k;
}

// launches: all tiles of a robot in one launch, a launch no larger than what the chip keeps resident (the tiles of a
// robot wait for each other): ONE workgroup per CU -- four wavefronts of up to 512 registers each fill the register files of a CU
// whatever the LDS says, and an over-estimate ends in VXH_ROBOT_SYNC_TIMEOUT replays, an under-estimate only in smaller launches
void pack_tile_launches(const std::vector<RobotModel>& robots, const HostBatch& H, const std::vector<Planned>& planned, int variant, int n_cu,
                        FluidTileTables& F, LaunchPlan& P)
{
    const long long capacity = n_cu;
    for (int kind = 0; kind < 12; ++kind) {
        const int tabg = kind & 1, mesh = (kind >> 1) % 3, small = kind / 6;      // mesh: 0 _voxcad, 1 land_water on land, 2 land_water in a fluid
        TileLaunchPlan cur;
        cur.tabg = tabg; cur.mesh = mesh; cur.small = small;
        for (const auto& q : planned) {
            if (q.tabg != tabg || q.mesh != mesh || q.small != small) continue;
            const int k = q.plan.k;
            if (k > capacity) continue;                    // more tiles than the chip holds: not tiled
            if (cur.count > 0 && cur.count + k > capacity) { P.tile_launches.push_back(cur); cur = TileLaunchPlan(); cur.tabg = tabg; cur.mesh = mesh; cur.small = small; }
            cur.lds = std::max(cur.lds, q.lds);
            append_robot_tiles(robots[q.r], q, H, variant, cur, F, P);
        }
        if (cur.count > 0) P.tile_launches.push_back(cur);
    }
    for (auto& L : P.tile_launches) {
        // a launch with no more tiles than CUs: a CU to every tile.  Two tiles that share a CU share its SIMDs, run at half
        // speed, and the whole robot waits for them at every barrier; asking for more than half of the LDS keeps them apart.
        if (L.count <= n_cu) L.lds = std::max(L.lds, (size_t)(81 * 1024));
        if (std::getenv("VXH_PROF_TILES"))
            std::fprintf(stderr, "vxhip: tile launch kind tabg=%d mesh=%d: %d tiles of %zu robots, %zu B of LDS, 1 workgroups per CU\n", L.tabg, L.mesh, L.count,
                         L.robots.size(), L.lds);
    }
}

// fused path: launch groups by kernel variant; inside a group the longest-running robots first
void form_groups(const std::vector<RobotModel>& robots, int variant, const Options& opt, LaunchPlan& P)
{
    const int nr = (int)robots.size();
    for (int r = 0; r < nr; ++r) {
        if (P.robot_tiled[r]) continue;
        const FusedVariant fv = fused_variant(robots[r], variant, opt);
        if (fv.block == 0) continue;                              // streaming kernels
        GroupPlan* g = nullptr;
        for (auto& q : P.groups) if (q.block == fv.block && q.nacc == fv.nacc && q.fluid == fv.fluid && q.tabg == fv.tabg && q.wide == fv.wide && q.two_tiles == fv.two_tiles) g = &q;
        if (!g) { P.groups.emplace_back(); g = &P.groups.back(); g->block = fv.block; g->nacc = fv.nacc; g->fluid = fv.fluid; g->tabg = fv.tabg; g->wide = fv.wide; g->two_tiles = fv.two_tiles; }
        g->robots.push_back(r);
        g->lds = std::max(g->lds, fv.lds);
    }
    // masks of the robots the streaming kernels step: everything the other kernels do not take / (option fused = 0)
    // everything but the tiled robots
    std::vector<unsigned char>& all = P.streamed_all, & rest = P.streamed_rest;
    all.assign(std::max(nr, 1), 1); rest.assign(std::max(nr, 1), 1);
    for (auto& g : P.groups) for (int r : g.robots) rest[r] = 0;
    for (int r = 0; r < nr; ++r) if (P.robot_tiled[r]) all[r] = rest[r] = 0;
    P.n_rest = P.n_all = 0;
    for (int r = 0; r < nr; ++r) { if (rest[r] && robots[r].nvox > 0) ++P.n_rest; if (all[r] && robots[r].nvox > 0) ++P.n_all; }
    for (auto& g : P.groups) {
        std::stable_sort(g.robots.begin(), g.robots.end(), [&](int a, int b) {
            return (double)robots[a].planned_steps * robots[a].nvox > (double)robots[b].planned_steps * robots[b].nvox; });
        g.count = (int)g.robots.size();
        if (!g.wide)                    // (k_robot_steps; colliding robots only: what differs between robots is contact work and broad-phase runs)
            for (int r : g.robots) if (robots[r].vxa.self_col_enabled) g.order_use = true;
    }
}

}  // namespace

LaunchPlan plan_launches(const std::vector<RobotModel>& robots, const HostBatch& H, int variant, const Options& opt, bool tiling_allowed, int n_cu)
{
    const int nr = (int)robots.size(), nv = H.nv;
    LaunchPlan P;
    // Tiled kernel (kernels_tiled.hpp), several workgroups per robot: for robots the resident kernel cannot take, and for
    // populations too small to give every CU a robot.  The number of tiles depends on the population (the results do not:
    // the tiled kernel's arithmetic per bond and per voxel, and its summation orders, are those of the resident kernel).
    P.robot_tiled.assign(nr, 0);
    P.robot_tiles.assign(nr, 0);
    P.xslot.assign(nv, 0);
    FluidTileTables F;
    const int tiled_now = tiling_allowed ? opt.tiled : 0;
    if (tiled_now > 0) {
        const std::vector<int> cand = tile_candidates(robots, variant, opt, tiled_now, n_cu);
        const std::vector<Planned> planned = plan_candidates(robots, cand, variant, opt, n_cu);
        pack_tile_launches(robots, H, planned, variant, n_cu, F, P);
    }
    P.tile_of.assign(P.tiles.empty() ? 1 : nv, -1); P.tile_lidx.assign(P.tiles.empty() ? 1 : nv, 0);
    for (size_t t = 0; t < P.tiles.size(); ++t)
        for (int k = 0; k < P.tiles[t].n_own; ++k) { const int g = P.tile_vox[P.tiles[t].vox_off + k]; P.tile_of[g] = (int)t; P.tile_lidx[g] = k; }
    upload_form(F, P);
    form_groups(robots, variant, opt, P);
    // streaming path: one rebuild block per 256 surface voxels of every colliding robot
    for (int r = 0; r < nr; ++r)
        if (robots[r].vxa.self_col_enabled)
            for (int i0 = 0; i0 < robots[r].nsurf; i0 += 256) { P.reb_robot.push_back(r); P.reb_i0.push_back(i0); }
    return P;
}

// ---- dominant_kernel: which unit of a call did most of its work ----
DominantKernel dominant_kernel(const std::vector<RobotModel>& robots, const std::vector<int>& steps, const std::vector<const GroupPlan*>& groups,
                               const std::vector<unsigned char>& robot_tiled, bool fused, bool tiled, bool streaming, int n_rest, long long todo,
                               const std::vector<long long>& group_launches, long long tile_launch_count)
{
    struct Work { double vs = 0, ab = 0; };      // voxel-steps, algorithmic bytes
    auto add = [&](Work& w, int r) {
        const double ds = steps[r];
        w.vs += ds * robots[r].nvox; w.ab += ds * (224.0 * robots[r].nvox + 144.0 * robots[r].nbond);
    };
    Work all, tiles;
    int n_tiled = 0;
    for (size_t r = 0; r < robots.size(); ++r) {
        if (robots[r].nvox) add(all, (int)r);
        if (robot_tiled[r]) { add(tiles, (int)r); ++n_tiled; }
    }
    std::vector<Work> grp(fused ? groups.size() : 0);
    size_t best = 0;
    double grp_best = 0;
    for (size_t k = 0; k < grp.size(); ++k) {
        for (int r : groups[k]->robots) add(grp[k], r);
        if (grp[k].vs > grp[best].vs) best = k;
        grp_best = std::max(grp_best, grp[k].vs);
    }
    // The rule, and it is not symmetric.  The tiles win when they did at least as much (>=) as the best group AND as everything else
    // without that group: all - tiles - best group, i.e. the streamed rest TOGETHER WITH every other group -- so they can lose although
    // they beat every single unit.  The best group (the first of equals) is then compared with the streamed rest alone, all - tiles -
    // EVERY group, and keeps the call unless the rest did strictly more (>).  Without launch groups: whatever was not tiled.
    typedef DominantKernel D;
    auto unit = [](D::Unit u, int group, int block, int n, long long launches, const Work& w) { return D{u, group, block, n, launches, w.ab, w.vs}; };
    if (tiled && tiles.vs >= grp_best && tiles.vs >= all.vs - tiles.vs - grp_best) return unit(D::TILES, -1, 1, n_tiled, tile_launch_count, tiles);
    Work rest = {all.vs - tiles.vs, all.ab - tiles.ab};
    if (grp.empty()) return unit(D::STREAMED, -1, 0, (int)robots.size() - n_tiled, todo, rest);
    for (const Work& g : grp) { rest.vs -= g.vs; rest.ab -= g.ab; }
    if (streaming && rest.vs > grp[best].vs) return unit(D::REST, -1, 0, n_rest, todo, rest);
    const GroupPlan& g = *groups[best];
    return unit(D::GROUP, (int)best, g.block + (g.wide ? 1 : 0), g.count, group_launches[best], grp[best]);
}

}  // namespace vxh
