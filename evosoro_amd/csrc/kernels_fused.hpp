// Fused path of the batched Voxelyze stepper: k_robot_steps<BLOCK, NACC, MESH, TABG>, one workgroup per robot, the robot
// resident in the CU for a whole launch of many time steps (its workgroup-level parts: kernels_group.hpp).  MESH = land_water
// robots, which carry the deformable surface mesh (fluid drag, RobotVolume tags); TABG = the robot's class tables are read
// from HBM instead of being copied into LDS (robots with per-voxel evolved stiffness, whose tables outgrow it).
//
// A step has two kinds of work items mapped onto the same threads:
//   voxels  thread t owns voxel t: its momenta stay in registers for the whole launch, its pose is published in LDS;
//   bonds   three slots per thread, one per axis (the axis is a compile-time constant per slot): the robot's per-axis COMPACTED bond
//           lists dealt to the threads by DBatch::bsched, so a sparse robot keeps ceil(bonds_A / 64) wavefronts busy per axis instead
//           of one lane per voxel whether it has that bond or not.  Up to 768 threads the X and Y slots are evaluated back to back
//           WITHOUT a barrier between them (their sums commute: below), the Y chunks dealt to the wavefronts X leaves idle; Z follows
//           behind a barrier.  The history of a bond is one 48-byte record in DBatch::hist_aos.
//   contact pairs  (self-colliding robots) the reach test of every listed pair -- pass 1 of fused_contact_forces -- is run for the whole
//           workgroup by the wavefronts that hold no bond of the Z slot, while the others evaluate theirs (fused_contact_reach_all): it needs
//           the poses only, and at the head of the voxel phase it was a latency chain on every wavefront at once.
// Dynamic LDS layout (doubles):
//   ps   [8][BLOCK]        pose tile: pos x y z, scale, quaternion w x y z of every voxel (read by bonds, contact forces,
//                          the broad-phase, the drag mesh)
//   acc  [NACC][6][BLOCK]  force / minus-moment accumulators of every voxel.  NACC = 2: tile 0 collects the bonds in
//                          which the voxel is the negative end (Force1/Moment1), tile 1 those in which it is the
//                          positive end; an entry gets at most one contribution per axis, added with an LDS atomic: X and Y
//                          in either order (a + b == b + a from the zero the voxel phase left), Z behind a barrier.  NACC = 1 (BLOCK 1024, where two tiles do not fit next to the pose tile): one
//                          tile, the two ends of a round are added in two barrier-separated sub-steps, which gives
//                          the reference's summation order +X -X +Y -Y +Z -Z.
//                          Also scratch of latch / broad-phase between steps (re-zeroed by the voxel phase).
//   pht  [2][BLOCK]        sin / cos of 2 pi' * PhaseOffset of every voxel (constants of the launch; kept out of registers
//                          and out of the step's load queue; read from HBM by the 768-thread MESH variant)
//   tabs                   this robot's DBondClass and DVoxClass rows (not TABG)
//   st   [6][BLOCK]        MESH, BLOCK <= 512: directional strains of the previous step (DBatch::strain otherwise)
//   mesh [3][nmv]          MESH only: vertices of the drag mesh (robots in a fluid)
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "device_types.hpp"
#include "dispatch_order.hpp"
#include "kernels_group.hpp"
#ifdef VXH_PHASE_TIMING
#include "kernels_dev.hpp"      // the developer library's cross-checks (dev_check_*)
#endif

namespace vxh {

// Dispatch order of LONG launches (more than VXH_ORDER_MAX_STEPS steps; dispatch_order.hpp): a launch ends with its slowest CU, and a CU steps its
// robots one after the other, so the workgroups are handed out by descending expected cost -- the permutation k_dispatch_order (kernels_order.hpp,
// queued in front of the launch) leaves in the group's workspace.  The cost is measured by the COST instances of k_robot_steps, which step the
// long launches of colliding groups: one lane reads the constant-rate clock in front of and behind the step loop and brackets the broad-phase
// runs, and the workgroup leaves the result for its robot in the workspace (by list entry).  The start values live in static LDS: a scalar
// register held across the step loop costs the loop a spill.  Short launches, and groups without collisions, run the instances without any of
// it (DESIGN.md "The cost of a launch": the numbers).
//
// Dispatch order of SHORT launches (a call of a few dozen steps: one launch, two robots per CU one after the other).  A broad-phase run
// is ~42 us, a sixth of a 20-step launch, and the launch ends with its slowest CU: with the robots in their fixed list order the last
// workgroups to be dispatched -- which land on the CUs that a run has already delayed -- bring runs of their own four times out of five
// (scripts/dev_gpu_diag.py launchcost: 69 us of fixed cost per launch against 20 without collisions).  So every workgroup leaves a bit at
// the end of EVERY launch: "my robot is due for a run within a launch like this one, or within VXH_ORDER_HORIZON steps if this one was
// longer" (its displacement since the last run, extrapolated at the average rate since then), and a SHORT launch takes the flagged robots FIRST: workgroup i steps the i-th flagged robot of the list,
// or the (i - flagged)-th unflagged one.  Every workgroup reads the same words (written by the PREVIOUS launch, two buffers), so the
// assignment is a permutation whatever the bits are; the robots do not interact, so the order changes no result.
__device__ __forceinline__ int fused_dispatch_slot(const unsigned long long* __restrict__ bits, int count, int i)
{
    const int nw = (count + 63) >> 6;
    int flagged = 0;
    for (int w = 0; w < nw; ++w) flagged += __builtin_popcountll(bits[w]);
    const bool set = i < flagged;
    int k = set ? i : i - flagged;
    for (int w = 0; w < nw; ++w) {
        unsigned long long x = set ? bits[w] : ~bits[w];
        if (!set && w == nw - 1 && (count & 63)) x &= (1ull << (count & 63)) - 1;
        const int c = __builtin_popcountll(x);
        if (k < c) { for (int j = 0; j < k; ++j) x &= x - 1; return (w << 6) + __builtin_ctzll(x); }
        k -= c;
    }
    return i;      // (not reached: flagged + unflagged == count)
}

// static LDS of the COST instances: the constant-rate clock in front of the step loop / at the start of the broad-phase run in progress, ticks
// in broad-phase runs during this launch / in the last one
struct FusedCostLds { unsigned long long t0, treb; unsigned reb_sum, reb_last; };
struct FusedNoLds {};

// order_in / order_out.  Not COST: the flag words a short launch reads (null: the list order) / those every launch leaves for the next.
// COST: order_in is the launch's permutation (never null) with the cost words behind it (dispatch_order.hpp order_ws_cost).
template <int BLOCK, int NACC, bool MESH, bool TABG, bool COST>
__global__ __launch_bounds__(BLOCK, (BLOCK + 255) / 256) void k_robot_steps(DBatch B, const DRobot* __restrict__ robots,
                                                                            const int* __restrict__ robot_list, long long step_cap, int iters,
                                                                            int lds_doubles, const unsigned long long* __restrict__ order_in,
                                                                            unsigned long long* order_out)
{
    extern __shared__ __align__(16) double lds[];
    double* const ps = lds;
    double* const acc = lds + 8 * BLOCK;
    // the 768-thread MESH variant is SLIM: actuation phases and strains stay in HBM, so that two accumulator tiles and the
    // mesh vertices fit into the 160 KB
    constexpr bool SLIM = MESH && BLOCK == 768;
    double* const pht = acc + NACC * 6 * BLOCK;    // sin / cos of every voxel's actuation phase, [2][BLOCK] (not SLIM)
    double* const tabs = pht + (SLIM ? 0 : 2 * BLOCK);
    // the robot's mutable control block lives in LDS for the whole launch: the per-step control is a serial chain
    // of ~20 dependent accesses executed by one thread while the workgroup waits, so it must not touch HBM
    __shared__ DRobotState rs;
    // per-step control words, double-buffered by step parity: thread 0 prepares step n+1 while the slower waves are
    // still in the voxel phase of step n (it idles at the barrier otherwise); only the collision-horizon decision,
    // which needs every voxel's new velocity, stays between the barriers
    __shared__ FusedCtl s_ctl[2];
    __shared__ int s_div, s_na[3], s_seg[2 * (BLOCK / 64)];
    __shared__ std::conditional_t<COST, FusedCostLds, FusedNoLds> s_cost;
    static_assert(sizeof(DRobotState) + 2 * sizeof(FusedCtl) + 4 * sizeof(int) /* s_div, s_na */ + 2 * 16 * sizeof(int) + sizeof(FusedCostLds) + 16 <= VXH_FUSED_STATIC_LDS, "static LDS bound");

    const int tid = threadIdx.x;
    VXH_T_PRO_BEGIN
    int slot;
    if constexpr (COST) slot = __builtin_amdgcn_readfirstlane(((const int*)order_in)[blockIdx.x]);
    else slot = order_in ? __builtin_amdgcn_readfirstlane(fused_dispatch_slot(order_in, (int)gridDim.x, (int)blockIdx.x)) : (int)blockIdx.x;
    const int r = __builtin_amdgcn_readfirstlane(robot_list[slot]);   // robots of one launch group, longest-running first; uniform -> scalar loads of R
    const DRobot& R = robots[r];            // separate noalias argument: its loads stay scalar although the kernel stores to HBM
    const unsigned nv = B.nv;
    const int base = R.vox_begin;
    const bool valid = tid < R.nvox;
    const int v = base + tid;
    if (tid == 0) { rs = B.rstate[r]; s_na[0] = s_na[1] = s_na[2] = 0; if constexpr (COST) s_cost.reb_sum = s_cost.reb_last = 0u; }
    // the robot's class tables: copied into LDS, or (TABG: robots with per-voxel evolved stiffness, where nearly every
    // bond and voxel is a class of its own and the tables outgrow the LDS) read from HBM / L2 where they lie
    const int nbd = TABG ? 0 : R.n_bclass * (int)(sizeof(DBondClass) / 8), nvd = TABG ? 0 : R.n_vclass * (int)(sizeof(DVoxClass) / 8);
    const DBondClass* bct;
    const DVoxClass* vct;
    if constexpr (TABG) {
        bct = B.bclass_tab + R.btab_begin;
        vct = B.vclass_tab + R.vtab_begin;
    } else {
        for (int k = tid; k < nbd; k += BLOCK) tabs[k] = ((const double*)(B.bclass_tab + R.btab_begin))[k];
        for (int k = tid; k < nvd; k += BLOCK) tabs[nbd + k] = ((const double*)(B.vclass_tab + R.vtab_begin))[k];
        bct = (const DBondClass*)tabs;
        vct = (const DVoxClass*)(tabs + nbd);
    }
    // MESH (land_water robots): directional strains of the previous step (inputs of the surface mesh: fluid drag, and the
    // RobotVolumeEnd tag on the host) in LDS next to the tables, then the mesh vertices; the 1024-thread variant has no
    // room for the strains and keeps them in HBM
    constexpr bool STRAIN_LDS = MESH && NACC == 2 && !SLIM;
    double* const st = STRAIN_LDS ? tabs + nbd + nvd : B.strain + R.vox_begin;
    const unsigned st_stride = STRAIN_LDS ? (unsigned)BLOCK : nv;
    double* const mesh = tabs + nbd + nvd + (STRAIN_LDS ? 6 * BLOCK : 0);
    // what is left of the dynamic LDS (lds_doubles in all) holds the contact rows of colliding robots: a mask per voxel (fused_contacts),
    // then the pairs: stiffnesses, codes
    unsigned long long* const cmask = (unsigned long long*)(mesh + ((MESH && (R.flags & RF_FLUID)) ? 3 * R.nmv : 0));
    double* const rc_a1 = (double*)cmask + BLOCK;
    const int pool_cap = ((R.flags & RF_SELF_COL) && !VXH_DBG(4)) ? max(0, (int)((lds_doubles - (int)(rc_a1 - lds)) * 2 / 3) - 1) : 0;
    int* const rc_code = (int*)(rc_a1 + pool_cap);
    if constexpr (STRAIN_LDS) {
#pragma unroll
        for (int k = 0; k < 6; ++k) st[k * BLOCK + tid] = tid < R.nvox ? B.strain[(unsigned)k * nv + (unsigned)(R.vox_begin + tid)] : 0.0;
    }
    __syncthreads();

    VXH_T_PRO(VXH_PROF_PRO_TABLES)             // tables -> LDS, first barrier
    // ---- this thread's voxel (momenta -> registers, pose -> LDS, accumulators zeroed) and its three bonds
    const DVoxClass& C = vct[valid ? B.vclass[v] : 0];
    int entry[3];                             // my bond of the X, Y and Z slot of a step (DBatch::bsched), -1 = none
    unsigned modebits = 0;                    // 2 bits per bond: SmallAngle, history layout (DBatch::hist)
    float amp_damp = 1.f;
    d3 lm = mk3(0, 0, 0), am = mk3(0, 0, 0);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        entry[a] = B.bsched[R.sched_begin + a * BLOCK + tid];      // (also threads without a voxel: the Y chunks are dealt to the idle wavefronts)
        if (entry[a] != -1) modebits |= (unsigned)(B.small_angle[(unsigned)a * nv + (base + (entry[a] & 1023))] & 3) << (2 * a);
    }
    // wavefronts that hold bonds of a slot (two tiles: that matters for Z, whose list goes to the threads in order -- the first s_na[2]
    // wavefronts; one tile: X, Y and Z all do); the others run the contact reach test of the whole workgroup there (fused_contact_reach_all)
    if ((tid & 63) == 0) {
#pragma unroll
        for (int a = (NACC == 2 ? 2 : 0); a < 3; ++a) if (entry[a] != -1) atomicAdd(&s_na[a], 1);
    }
    if (valid) {
        const int b0 = rs.steps & 1;
        amp_damp = B.amp_damp[v];
        if constexpr (!SLIM) { pht[tid] = B.act_sb[v]; pht[BLOCK + tid] = B.act_cb[v]; }
        lm = mk3(LINMOM(0, v), LINMOM(1, v), LINMOM(2, v));
        am = mk3(ANGMOM(0, v), ANGMOM(1, v), ANGMOM(2, v));
        ps[tid] = POS(b0, 0, v); ps[BLOCK + tid] = POS(b0, 1, v); ps[2 * BLOCK + tid] = POS(b0, 2, v); ps[3 * BLOCK + tid] = SCALE(b0, v);
        ps[4 * BLOCK + tid] = QUAT(0, v); ps[5 * BLOCK + tid] = QUAT(1, v); ps[6 * BLOCK + tid] = QUAT(2, v); ps[7 * BLOCK + tid] = QUAT(3, v);
    }
#pragma unroll
    for (int k = 0; k < NACC * 6; ++k) acc[k * BLOCK + tid] = 0.0;
    const FetchLds<BLOCK> fetch{ps, base};
    DragCache<BLOCK> dcache;
    if constexpr (MESH && DragCache<BLOCK>::KEEP) { if ((R.flags & RF_FLUID) && R.nmv > 0 && R.nfacet > 0) { dcache.load(B, R, tid); if (valid) { dcache.my_first = B.facet_first[v]; dcache.my_count = (int)B.facet_count[v]; } } }
    // my contact row: partner count | (start of the workgroup's LDS copy of it + 1) << VXH_ROWD_BITS; s_seg: where the rows of each wavefront's
    // lanes start in the copy and how many pairs they hold (-1: they did not fit, that wavefront reads its rows from memory).
    // Refreshed after every broad-phase run.  (every thread calls: barriers inside)
    int rowd = 0;
    auto rows_to_lds = [&](bool at_launch) {
        rowd = 0;
        if (!(R.flags & RF_SELF_COL)) return;
        // (see opaque_tid.  The 1024-thread variant uses the kernel's own index: with a local `tid` re-read from threadIdx.x here -- the
        // same value -- dense 10^3 robots ran 4-5 % slower, 56.1-56.7 against 53.3-54.5 us per step, same box, interleaved; without it
        // they run as before, 52.9-53.6 against 53.2-53.5.  Why is not known: the ISA of the two differs by register numbering.)
        int tid_r = tid;
        if constexpr (BLOCK != 1024) tid_r = opaque_tid<BLOCK>();
#ifdef VXH_PHASE_TIMING
        unsigned long long t_r2l = __builtin_readcyclecounter();
#define VXH_R2L_MARK(slot) { const unsigned long long t_now = __builtin_readcyclecounter(); if (B.prof && tid == 0) atomicAdd(&B.prof[slot], t_now - t_r2l); t_r2l = t_now; }
#else
#define VXH_R2L_MARK(slot)
#endif
        const int img = R.img_index;
        constexpr int NW = BLOCK / 64;
        if (at_launch && img >= 0 && rs.rows_img != 0 && !VXH_DBG(1)) {
            // the copy as the previous launch left it (DBatch::rimg_*): one round trip of coalesced loads.  The rows only change in a
            // broad-phase run, and every run ends in the save below.
            const int* const seg = B.rimg_seg + (size_t)img * 64;
            const int used = __builtin_amdgcn_readfirstlane(seg[2 * NW]);
            if (valid) rowd = B.rimg_rowd[v];
            if (tid_r < 2 * NW) s_seg[tid_r] = seg[tid_r];
            for (int k = tid_r; k < used; k += BLOCK) { rc_code[k] = B.rimg_code[(size_t)img * VXH_RIMG_CAP + k]; rc_a1[k] = B.rimg_a1[(size_t)img * VXH_RIMG_CAP + k]; }
            if (pool_cap > 0) cmask[tid_r] = 0;
            __syncthreads();
            VXH_R2L_MARK(VXH_PROF_R2L_COPY)
            return;
        }
        int row = -1;
        if (valid) { const int so = B.surf_ord[v]; if (so >= 0) row = R.surf_begin + so; }
        const int ccnt = (row >= 0 && !VXH_DBG(1)) ? B.col_cnt[row] : 0;
        if (pool_cap > 0) cmask[tid_r] = 0;
        __syncthreads();
        VXH_R2L_MARK(VXH_PROF_R2L_COUNT)     // surface ordinal -> row count (two dependent loads), first barrier
        const int ccnt_l = ccnt <= 64 ? ccnt : 0;     // (a longer row stays in memory: 64 mask bits per voxel)
        int incl = ccnt_l;                    // places in the copy: prefix sum within the wavefront, one atomic per wavefront
        const int lane = tid_r & 63;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
        const int wave_total = __shfl(incl, 63);
        // the wavefronts' segments follow each other in wavefront order: which rows fit (and which are read from memory) must not
        // depend on who got there first, the two paths need not round alike
        if (lane == 0) s_seg[2 * (tid_r >> 6) + 1] = wave_total;
        __syncthreads();
        int wave_base = 0, all_total = 0;
        for (int w = 0; w < NW; ++w) { const int t = s_seg[2 * w + 1]; if (w < (tid_r >> 6)) wave_base += t; all_total += t; }
        __syncthreads();                      // (s_seg is rewritten below)
        VXH_R2L_MARK(VXH_PROF_R2L_SCAN)     // scan, totals, two barriers, prefix over the wavefronts
        const bool fits = wave_base + wave_total <= pool_cap;
        if (lane == 0) { s_seg[2 * (tid_r >> 6)] = wave_base; s_seg[2 * (tid_r >> 6) + 1] = fits ? wave_total : -1; }
        // (the developer build used to count wavefront copies and overflows here with global atomics from every wavefront: contended, and the
        // barrier below waits for them -- this function took 52 k cycles per call with them and takes 13.5 k without, and the difference
        // was for a while mistaken for a cost of copying the rows; removed)
        const int off = wave_base + incl - ccnt_l;
        rowd = ccnt;
        if (fits && ccnt_l > 0) {
            rowd = ccnt | ((off + 1) << VXH_ROWD_BITS);
            for (int k0 = 0; k0 < ccnt; k0 += 4) {           // (four entries' loads in flight: a row of 16 costs four round trips, not sixteen)
                int pj[4]; double aj[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { const size_t at = col_at(R, min(k0 + j, ccnt - 1), row); pj[j] = B.col_partner[at]; aj[j] = B.col_a1[at]; }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k0 + j < ccnt) { rc_code[off + k0 + j] = (pj[j] - base) | (tid_r << 10) | ((k0 + j) << 20); rc_a1[off + k0 + j] = aj[j]; }
            }
        }
        __syncthreads();
        VXH_R2L_MARK(VXH_PROF_R2L_COPY)     // the copy itself, last barrier
        if (img >= 0 && !VXH_DBG(1)) {
            // save the copy for the next launches (stores only: nothing waits for them)
            const int used = min(min(all_total, pool_cap), (int)VXH_RIMG_CAP);
            int* const seg = B.rimg_seg + (size_t)img * 64;
            if (valid) B.rimg_rowd[v] = rowd;
            if (tid_r < 2 * NW) seg[tid_r] = s_seg[tid_r];
            if (tid_r == 0) { seg[2 * NW] = used; rs.rows_img = (all_total <= VXH_RIMG_CAP || pool_cap <= VXH_RIMG_CAP) ? 1 : 0; }
            for (int k = tid_r; k < used; k += BLOCK) { B.rimg_code[(size_t)img * VXH_RIMG_CAP + k] = rc_code[k]; B.rimg_a1[(size_t)img * VXH_RIMG_CAP + k] = rc_a1[k]; }
        }
    };

    // the control thread sits in the LAST wave: the one with the fewest (often no) voxels, so its serial work hides
    // behind the other waves' voxel phase
    const bool ctl_thread = tid == BLOCK - 64;
    if (ctl_thread) { fused_control_begin(R, rs, step_cap, iters > 0, s_ctl[0]); fused_control_horizon(R, rs, s_ctl[0]); s_div = 0; }
    VXH_T_PRO(VXH_PROF_PRO_STATE)              // state load, zeroing, control
    rows_to_lds(true);
    VXH_T_PRO(VXH_PROF_PRO_R2L)                // rows_to_lds as a whole
    __syncthreads();                           // control of the first step + every voxel's pose visible
    constexpr int NWAVES = BLOCK / 64;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // (one tile, 1024 threads: a third of the pairs in each of the three rounds -- a dense lattice leaves ONE wavefront idle per round)
    const int nz = __builtin_amdgcn_readfirstlane(s_na[2]);
    const int nx = NACC == 1 ? __builtin_amdgcn_readfirstlane(s_na[0]) : 0, ny = NACC == 1 ? __builtin_amdgcn_readfirstlane(s_na[1]) : 0;
    const bool reach_early = (R.flags & RF_SELF_COL) && nz < NWAVES && nx < NWAVES && ny < NWAVES && !VXH_DBG(32);     // (uniform)
    // pairs of the LDS copy that are really there: the wavefronts whose rows fit are a prefix (a wavefront's place is the sum of ALL
    // earlier totals), so the sum of their totals is the end of the valid stretch
    auto pairs_in_copy = [&]() { int n = 0; for (int w = 0; w < NWAVES; ++w) n += max(s_seg[2 * w + 1], 0); return __builtin_amdgcn_readfirstlane(n); };
    int npairs = reach_early ? pairs_in_copy() : 0;
    VXH_T_DECL
    VXH_T_REB_DECL
    VXH_T_PRO_END
    // (the clock is read here, behind the prologue's loads: the instruction waits for every scalar load and LDS access in flight)
    if constexpr (COST) { if (tid == 0) s_cost.t0 = __builtin_amdgcn_s_memrealtime(); }
    int it = 0;
    for (;; ++it) {
        const FusedCtl& K = s_ctl[it & 1];
        FusedCtl& Knext = s_ctl[(it + 1) & 1];
        const int kf = __builtin_amdgcn_readfirstlane(K.flags);
        const bool k_go = kf & 1, k_latch = kf & 2, k_eol = kf & 4, k_rebuild = kf & 8, k_trace = kf & VXH_CTL_TRACE_BITS;
        if (!k_go && !k_trace) break;
        // opaque per-step copies: keeps the compiler from hoisting every address of the step out of the loop (dozens of
        // loop-invariant 64-bit pointers, which it then spills)
        int vv = v;
        asm volatile("" : "+v"(vv));
        bool scratch_used = false;            // latch / broad-phase borrow the accumulator tile
        if (k_latch || k_eol || k_trace) {
            fused_latch_cm<BLOCK>(B, R, rs, ps, acc, valid, C, k_latch, k_eol, fused_trace_mask(kf), K.trace_index);
            scratch_used = true;
        }
        if (!k_go) break;                      // (the robot has stopped; the last step's trace point, if one was due, is in)
        VXH_T_REB_BEGIN
        if (__builtin_expect(k_rebuild, 0)) {
            if constexpr (COST) { if (tid == 0) s_cost.treb = __builtin_amdgcn_s_memrealtime(); }
            fused_rebuild<BLOCK>(B, R, rs, ps, acc, NACC * 6 * BLOCK, (double*)cmask, max(0, lds_doubles - (int)((double*)cmask - lds)), vct);
#ifdef VXH_PHASE_TIMING
            if (VXH_DBG(16) && B.prof) dev_check_rebuild<BLOCK>(B, R, rs, ps, (int*)acc, vct, tid);
#endif
            rows_to_lds(false);
            if (reach_early) npairs = pairs_in_copy();
#pragma unroll
            for (int k = 1; k < NACC * 6; ++k) acc[k * BLOCK + tid] = 0.0;      // the scratch of the broad-phase (plane 0: below)
            scratch_used = true;
            if constexpr (COST) { if (tid == 0) { const unsigned dtr = (unsigned)(__builtin_amdgcn_s_memrealtime() - s_cost.treb); s_cost.reb_last = dtr; s_cost.reb_sum += dtr; } }
        }
        VXH_T_REB_END(k_rebuild)
        if (scratch_used) { acc[tid] = 0.0; __syncthreads(); }
        d3 drag = mk3(0, 0, 0);
        const bool fluid = MESH && (R.flags & RF_FLUID) != 0;
        if constexpr (MESH) { if (fluid) drag = fused_drag<BLOCK, NACC * 6 * BLOCK>(B, R, ps, st, st_stride, mesh, acc, valid, vv, lm, C.mass_inv, dcache); }
        const bool damp_on = (kf & 32) != 0;
        VXH_T_MARK(1)

        // ---- bond phase.  Two accumulator tiles: the X and Y slots back to back, no barrier between them (every accumulator entry
        // gets at most one X and one Y contribution, both ADDED to the zero the voxel phase left: a + b == b + a, the sums are those of
        // barrier-separated rounds bit for bit; the Y chunks sit on the wavefronts X leaves idle: DBatch::bsched), barrier, the Z slot
        // on top.  One tile (1024 threads): three rounds, each in two barrier-separated sub-steps.
        // (Measured and not kept, round 4: Z EVALUATED in the same barrier-free stretch, its chunks dealt like Y's -- 21 chunks on 12
        // wavefronts, 6 / 5 / 5 / 5 per SIMD -- and its twelve outputs held in registers across the barrier that orders them behind
        // X + Y: the held outputs raise the peak of the bond's register need, 28 -> 124 B of scratch, 25.5 -> 25.9 us per step.)
        bool div = false;
        fused_round<0, BLOCK, NACC, MESH>(B, R, bct, ps, acc, entry[0], modebits, damp_on, div, st, st_stride);
        if constexpr (NACC == 1) {
            if (reach_early && wave >= nx) fused_contact_reach_all<BLOCK>(ps, 0, npairs / 3, wave - nx, NWAVES - nx, cmask, rc_code);
            __syncthreads();
        }
        fused_round<1, BLOCK, NACC, MESH>(B, R, bct, ps, acc, entry[1], modebits, damp_on, div, st, st_stride);
        if constexpr (NACC == 1) { if (reach_early && wave >= ny) fused_contact_reach_all<BLOCK>(ps, npairs / 3, 2 * (npairs / 3), wave - ny, NWAVES - ny, cmask, rc_code); }
        __syncthreads();
        fused_round<2, BLOCK, NACC, MESH>(B, R, bct, ps, acc, entry[2], modebits, damp_on, div, st, st_stride);
        if (reach_early && wave >= nz) fused_contact_reach_all<BLOCK>(ps, NACC == 1 ? 2 * (npairs / 3) : 0, npairs, wave - nz, NWAVES - nz, cmask, rc_code);
        if (div) s_div = 1;
        VXH_T_MARK(2)
        __syncthreads();                       // (B)
        VXH_T_MARK(3)
        if (s_div) {                           // Integrate() returns before the voxel loop (VX_Sim.cpp:1777)
            __syncthreads();                   // everyone has read s_div
            if (ctl_thread) { rs.diverged = 1; fused_control_begin(R, rs, step_cap, 0, Knext); s_div = 0; }   // -> status diverged, go = 0
            __syncthreads();
            continue;
        }
        // ---- voxel phase: sums from the accumulators (zeroed again for the next step), pose from the tile, momenta in
        // registers; contact partners from the pose tile
        double vel2 = 0;
        VoxState S;
        if (R.flags & RF_SELF_COL) {
            if (!reach_early) {                             // (else: done in the Z slot by the wavefronts without a Z bond)
                const int nseg = s_seg[2 * (tid >> 6) + 1];     // pairs in the LDS copy of my wavefront's contact rows (-1: the rows are read from memory)
                if (nseg > 0) fused_contact_reach<BLOCK>(ps, s_seg[2 * (tid >> 6)], nseg, cmask, rc_code);   // every lane: the wavefront shares the pairs
            }
        }
        if (valid) {
            d3 F = mk3(acc[tid], acc[BLOCK + tid], acc[2 * BLOCK + tid]), M = mk3(acc[3 * BLOCK + tid], acc[4 * BLOCK + tid], acc[5 * BLOCK + tid]);
            if constexpr (NACC == 2) {
                F = F + mk3(acc[6 * BLOCK + tid], acc[7 * BLOCK + tid], acc[8 * BLOCK + tid]);
                M = M + mk3(acc[9 * BLOCK + tid], acc[10 * BLOCK + tid], acc[11 * BLOCK + tid]);
            }
            S.pos = mk3(ps[tid], ps[BLOCK + tid], ps[2 * BLOCK + tid]); S.scale = ps[3 * BLOCK + tid];
            S.ang = mkq(ps[4 * BLOCK + tid], ps[5 * BLOCK + tid], ps[6 * BLOCK + tid], ps[7 * BLOCK + tid]);
            S.lm = lm; S.am = am;
            // (measured and not kept: the class constants copied by value here, so that their LDS reads go out with the sums and the pose
            // instead of one by one inside the update -- 23.45 -> 23.68 us per step, and other contraction choices, i.e. other last bits)
            const d3 vel = S.lm * C.mass_inv;
            F = F + (vel * (-R.slow_z)) * C.c_lin;
#ifdef VXH_PHASE_TIMING
            const d3 F_before = F;
            const unsigned long long mask_seen = ((rowd >> VXH_ROWD_BITS) != 0) ? cmask[tid] : 0ull;     // what pass 2 is about to consume
#endif
            if (rowd != 0) F = fused_contact_forces<BLOCK>(B, R, ps, F, S.pos, S.scale, tid, vv, rowd, cmask, rc_code, rc_a1);
#ifdef VXH_PHASE_TIMING
            if (VXH_DBG(8) && B.prof && (rowd >> VXH_ROWD_BITS) != 0) dev_check_contact_rows<BLOCK>(B, R, ps, F_before, F, S, tid, vv, rowd, mask_seen, cmask, rc_code, rc_a1);
#endif
            vel2 = voxel_update(B, R, C, vv, fetch, K.time, K.act_sin, K.act_cos, K.prenatal_c, F, M, vel, S, -1, 0, fluid, drag,
                                SLIM ? B.act_sb[vv] : pht[tid], SLIM ? B.act_cb[vv] : pht[BLOCK + tid], amp_damp);
            lm = S.lm; am = S.am;
            // the accumulators zeroed for the next step -- HERE, behind the update: stores into the LDS between the reads above and the
            // update's own (class table, contact rows) kept the compiler from issuing those reads together (23.75 -> 23.43 us per step)
#pragma unroll
            for (int k = 0; k < NACC * 6; ++k) acc[k * BLOCK + tid] = 0.0;
        }
        // next step's control, off the critical path.  (Round 4, measured and taken out again: the same call issued earlier -- next to the
        // X / Y chunks with one Y chunk fewer on this wavefront, 25.2 -> 26.0 us per step: that slot is issue-bound on every SIMD; or
        // during the Z slot, which leaves this wavefront idle, 25.3 -> 25.45: the developer timers show this wavefront last at barrier
        // (C), but the voxel wavefronts sharing its SIMD finish at the same time with or without it.)
        HorizonInputs hz = {0.0, 0.0, 0, 0, 0, 0};
        if (ctl_thread) { fused_control_begin(R, rs, step_cap, it + 1 < iters, Knext); hz = fused_horizon_prefetch(rs, Knext); }
        if ((R.flags & RF_SELF_COL) && !VXH_DBG(2)) {            // SS.MaxVoxVel for the collision horizon (VX_Sim.cpp:1625-1649)
            vel2 = wave_max_nonneg(vel2);       // (DPP: VALU speed)
            if ((tid & 63) == 0) atomicMax(&rs.maxvel2_bits, (unsigned long long)__double_as_longlong(vel2));
        }
        VXH_T_MARK(4)
        __syncthreads();                       // (C) every read of the old poses is done
        if (valid) {
            ps[tid] = S.pos.x; ps[BLOCK + tid] = S.pos.y; ps[2 * BLOCK + tid] = S.pos.z; ps[3 * BLOCK + tid] = S.scale;
            ps[4 * BLOCK + tid] = S.ang.w; ps[5 * BLOCK + tid] = S.ang.x; ps[6 * BLOCK + tid] = S.ang.y; ps[7 * BLOCK + tid] = S.ang.z;
        }
        VXH_T_MARK(5)
        if (ctl_thread) { fused_horizon_decide(R, rs, Knext, hz); s_div = 0; }
        __syncthreads();                       // (A) control + every voxel's published pose visible
        VXH_T_MARK(0)
    }
    VXH_T_FLUSH
    VXH_T_EPI_BEGIN
    VXH_T_REB_FLUSH
    // ---- back to HBM: state into the buffer the step count selects, flag bits, control block
    if (valid) {
        const int b1 = rs.steps & 1;
        POS(b1, 0, v) = ps[tid]; POS(b1, 1, v) = ps[BLOCK + tid]; POS(b1, 2, v) = ps[2 * BLOCK + tid];
        SCALE(b1, v) = ps[3 * BLOCK + tid];
        QUAT(0, v) = ps[4 * BLOCK + tid]; QUAT(1, v) = ps[5 * BLOCK + tid]; QUAT(2, v) = ps[6 * BLOCK + tid]; QUAT(3, v) = ps[7 * BLOCK + tid];
        LINMOM(0, v) = lm.x; LINMOM(1, v) = lm.y; LINMOM(2, v) = lm.z;
        ANGMOM(0, v) = am.x; ANGMOM(1, v) = am.y; ANGMOM(2, v) = am.z;
    }
    if constexpr (STRAIN_LDS) {
        if (valid) {
#pragma unroll
            for (int k = 0; k < 6; ++k) B.strain[(unsigned)k * nv + (unsigned)v] = st[k * BLOCK + tid];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (entry[a] != -1) B.small_angle[(unsigned)a * nv + (base + (entry[a] & 1023))] = (unsigned char)((modebits >> (2 * a)) & 3u);
    if (tid == 0) {
        B.rstate[r] = rs; if (B.rstate_mirror) B.rstate_mirror[r] = rs;
        // (the list entry is worked out again rather than kept: a scalar register held across the step loop costs the loop a spill)
        if constexpr (COST) {      // what this launch cost, and what the next long one's order needs of the robot's state (dispatch_order.hpp)
            const bool horizon = (R.flags & RF_SELF_COL) && (R.flags & RF_HORIZON_COL);
            DispatchCost& mine = order_ws_cost((const int*)order_in, (int)gridDim.x)[((const int*)order_in)[blockIdx.x]];
            DispatchCost c = {0.f, 0.f, 0.f, 0.f, 0, 0};
            const unsigned in_runs = horizon ? s_cost.reb_sum : 0u;      // (a robot that runs the broad-phase every step: the runs are part of its step)
            const long long ticks = (long long)(__builtin_amdgcn_s_memrealtime() - s_cost.t0);
            c.launch_ticks = (int)ticks;
            c.step_ticks = it > 0 ? (float)(ticks - (long long)in_runs) / (float)it : mine.step_ticks;      // (a launch without a step measures nothing)
            c.reb_ticks = !horizon ? 0.f : (s_cost.reb_last ? (float)s_cost.reb_last : mine.reb_ticks);      // (no run in this launch: what an earlier one took)
            if (rs.status == 0) {
                // steps until the robot's own stop condition (step_control_begin); none: as good as unbounded
                double left = 1e9;
                if (R.stop_type == 1) left = (double)((int)(R.stop_value + 0.5) + 1 - rs.steps);
                else if (R.stop_type == 2) left = (R.stop_value + R.afterlife - rs.cur_time) / R.dt + 1.0;
                else if (R.stop_type == 3) left = (R.temp_period_d * R.stop_value - rs.cur_time) / R.dt + 1.0;
                c.left = (int)fmin(fmax(left, 1.0), 1e9);
                if (horizon) {     // the next run: the displacement since the last one, growing at the average rate since then
                    const double thr = (R.col_horizon - 1.0) / 2;
                    if (thr > 0) { c.disp_frac = (float)(rs.max_disp / thr); c.rate_frac = (float)(rs.max_disp / (double)max(1, rs.steps - rs.reb_step) / thr); }
                }
            }
            mine = c;
        }
        if (order_out) {       // due for a broad-phase run within a launch like this one?  (see fused_dispatch_slot)
            bool soon = false;
            if (rs.status == 0 && (R.flags & RF_SELF_COL) && (R.flags & RF_HORIZON_COL)) {
                const double rate = rs.max_disp / (double)max(1, rs.steps - rs.reb_step);
                // (`it`: the steps of this launch; a long launch -- whose own order is by cost -- leaves the flags for a short one behind it.
                // Generous: a robot flagged for nothing costs nothing, a run in the second round of a late CU costs the launch 42 us; 2.5 against
                // 1.25 launch lengths: the driver's command 1.383-1.405e10 against 1.380-1.403e10, same box, alternating)
                soon = rs.max_disp + rate * (2.5 * (double)min(max(1, it), (int)VXH_ORDER_HORIZON)) > (R.col_horizon - 1.0) / 2;
            }
            int my;
            if constexpr (COST) my = ((const int*)order_in)[blockIdx.x];
            else my = order_in ? fused_dispatch_slot(order_in, (int)gridDim.x, (int)blockIdx.x) : (int)blockIdx.x;
            const unsigned long long bit = 1ull << (my & 63);
            if (soon) atomicOr(&order_out[my >> 6], bit); else atomicAnd(&order_out[my >> 6], ~bit);
        }
    }
    VXH_T_EPI_END
}

}  // namespace vxh
