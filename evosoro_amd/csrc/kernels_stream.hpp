// The streaming kernels, for lattices of any size: k_step_begin / k_mesh_vertices / k_facets / k_bonds / k_voxels, one thread per bond
// slot / voxel, state and bond outputs through HBM; and k_results, the reduction behind the result file.  Launched by launch_stream.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.hpp"
#include "kernels_physics.hpp"

namespace vxh {

// ================================================================================================ streaming path
// where the whole-robot passes (IniCM latch, broad-phase) read position + scale of an arbitrary voxel of the robot
struct PoseFromState {     // streaming path: the state planes, buffer `cur`
    const DBatch& B; int cur;
    __device__ __forceinline__ void operator()(int slot, double& x, double& y, double& z, double& s) const
    { x = POS(cur, 0, slot); y = POS(cur, 1, slot); z = POS(cur, 2, slot); s = SCALE(cur, slot); }
};

// The reductions behind the result file, from the state the stepping kernels left in HBM: one workgroup per robot.  The centre of
// mass keeps the reference's summation order (thread 0 adds voxel after voxel; the products come from all threads); the extrema
// and counts are order-free.  Every expression that the host used to evaluate is written with explicit roundings (no contraction),
// so the numbers are those of the host path bit for bit (option host_results = 1 keeps that path for cross-checks).
static __global__ __launch_bounds__(256) void k_results(DBatch B, DResult* __restrict__ out)
{
#pragma clang fp contract(off)      // every product and sum below is rounded on its own, like on the host (HIP's *_rn arithmetic helpers would not
                                    // do: they are plain operators compiled where they are DEFINED, with contraction on)
    const int r = blockIdx.x, tid = threadIdx.x;
    const DRobot& R = B.robot[r];
    const DRobotState& rs = B.rstate[r];
    __shared__ double sh[4 * 256];
    __shared__ double red[4][4];
    __shared__ int cnt[2][4];
    const int cur = rs.steps & 1, base = R.vox_begin;
    double sx = 0, sy = 0, sz = 0, sm = 0;
    double d2max = 0.0, d2min = 1.0e300, ymax = -1.0e300, ymin = 1.0e300;
    int touching = 0, feet = 0;
    const double ix = rs.ini_cm[0], iy = rs.ini_cm[1];
    for (int c0 = 0; c0 < R.nvox; c0 += 256) {
        const int k = c0 + tid;
        if (k < R.nvox) {
            const int g = base + k;
            const DVoxClass& C = B.vclass_tab[R.vtab_begin + B.vclass[g]];
            const double x = POS(cur, 0, g), y = POS(cur, 1, g), z = POS(cur, 2, g), s = SCALE(cur, g);
            sh[tid] = x * C.mass; sh[256 + tid] = y * C.mass; sh[512 + tid] = z * C.mass; sh[768 + tid] = C.mass;
            const double dx = x - ix, dy = y - iy;
            const double dxx = dx * dx, dyy = dy * dy;
            const double d2 = dxx + dyy;
            d2max = d2 > d2max ? d2 : d2max; d2min = d2 < d2min ? d2 : d2min;
            if (C.mat != 5) { ymax = y > ymax ? y : ymax; ymin = y < ymin ? y : ymin; }
            const double half = 0.5 * s;
            if (half - z > 0) { ++touching; if (C.mat == 6) ++feet; }
        }
        __syncthreads();
        if (tid == 0) {
            const int n = min(256, R.nvox - c0);
            for (int j = 0; j < n; ++j) { sx = sx + sh[j]; sy = sy + sh[256 + j]; sz = sz + sh[512 + j]; sm = sm + sh[768 + j]; }
        }
        __syncthreads();
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double a = __shfl_xor(d2max, off), b = __shfl_xor(d2min, off), c = __shfl_xor(ymax, off), d = __shfl_xor(ymin, off);
        d2max = a > d2max ? a : d2max; d2min = b < d2min ? b : d2min; ymax = c > ymax ? c : ymax; ymin = d < ymin ? d : ymin;
        touching += __shfl_xor(touching, off); feet += __shfl_xor(feet, off);
    }
    if ((tid & 63) == 0) { const int w = tid >> 6; red[0][w] = d2max; red[1][w] = d2min; red[2][w] = ymax; red[3][w] = ymin; cnt[0][w] = touching; cnt[1][w] = feet; }
    __syncthreads();
    if (tid == 0) {
        DResult o;
        const double inv = R.nvox > 0 ? 1.0 / sm : 0.0;
        o.cm[0] = inv * sx; o.cm[1] = inv * sy; o.cm[2] = inv * sz;
        o.d2max = fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
        o.d2min = fmin(fmin(red[1][0], red[1][1]), fmin(red[1][2], red[1][3]));
        o.ymax = fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));
        o.ymin = fmin(fmin(red[3][0], red[3][1]), fmin(red[3][2], red[3][3]));
        o.touching = cnt[0][0] + cnt[0][1] + cnt[0][2] + cnt[0][3];
        o.feet = cnt[1][0] + cnt[1][1] + cnt[1][2] + cnt[1][3];
        out[r] = o;
    }
}

static __global__ __launch_bounds__(256) void k_step_begin(DBatch B, long long step_cap, int begin_new_step)
{
    const int r = blockIdx.x;
    if (!B.streamed[r]) return;             // (stepped by the resident kernel)
    const DRobot& R = B.robot[r];
    DRobotState& rs = B.rstate[r];
    __shared__ double sh[5 * 256];
    __shared__ int s_latch, s_eol, s_trace, s_tidx;
    if (threadIdx.x == 0) {
        StepCtl c = step_control(R, rs, step_cap, begin_new_step);
        s_latch = c.latch; s_eol = c.eol; s_trace = c.trace; s_tidx = c.trace_index;
        if (c.go) actuation_sincos(R, rs.cur_time, rs.act_sin, rs.act_cos);
    }
    __syncthreads();
    if (s_latch || s_eol || s_trace) latch_cm(B, R, rs, PoseFromState{B, rs.steps & 1}, s_latch != 0, s_eol != 0, sh, 256, s_trace, s_tidx);
}

template <int A>
__device__ __forceinline__ void stream_bond(const DBatch& B, const DRobot& R, const DRobotState& rs, int r, int slot, int v1, int bc)
{
    const int v2 = B.nbr[(2 * A) * B.nv + v1];
    const int cur = rs.steps & 1;
    d3 p1 = mk3(POS(cur, 0, v1), POS(cur, 1, v1), POS(cur, 2, v1));
    d3 p2 = mk3(POS(cur, 0, v2), POS(cur, 1, v2), POS(cur, 2, v2));
    dq q1 = mkq(QUAT(0, v1), QUAT(1, v1), QUAT(2, v1), QUAT(3, v1));
    dq q2 = mkq(QUAT(0, v2), QUAT(1, v2), QUAT(2, v2), QUAT(3, v2));
    const double sc1 = SCALE(cur, v1), sc2 = SCALE(cur, v2);
    BondHist H = load_bond_hist(B, slot);
    const unsigned old_flags = H.flags;
    BondOut o = bond_compute<A>(B, B.bclass_tab[R.btab_begin + bc], H, p1, q1, sc1, p2, q2, sc2, rs.dt_prev != 0);
    store_bond_hist(B, slot, H, old_flags);
    if (o.diverged) atomicOr(&B.rstate[r].diverged, 1);
    if (R.nmv > 0) {      // land_water: CurStrainV1 / CurStrainV2 (SetStrainDir), inputs of the surface mesh in the next step
        B.strain[(unsigned)A * B.nv + v1] = o.strain1;
        B.strain[(unsigned)(3 + A) * B.nv + v2] = o.strain2;
    }
    BOUT(0, slot) = o.f1.x; BOUT(1, slot) = o.f1.y; BOUT(2, slot) = o.f1.z;
    BOUT(3, slot) = o.m1.x; BOUT(4, slot) = o.m1.y; BOUT(5, slot) = o.m1.z;
    BOUT(6, slot) = o.f2.x; BOUT(7, slot) = o.f2.y; BOUT(8, slot) = o.f2.z;
    BOUT(9, slot) = o.m2.x; BOUT(10, slot) = o.m2.y; BOUT(11, slot) = o.m2.z;
}

// Fluid drag of the streaming path (robots in a fluid that do not fit the resident kernel): the surface mesh of the step,
// one thread per vertex, then one thread per facet; k_voxels adds up each voxel's facets.  Launched between k_step_begin
// and k_bonds: the strains read here are those of the previous step, the poses and momenta those at the start of this one.
static __global__ __launch_bounds__(256) void k_mesh_vertices(DBatch B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B.n_mv) return;
    const int r = B.vert_robot[i];
    const DRobot& R = B.robot[r];
    const DRobotState& rs = B.rstate[r];
    if (!B.streamed[r] || !(R.flags & RF_FLUID) || !rs.active) return;
    const int cur = rs.steps & 1;
    const unsigned tm = B.total_mv, nv = B.nv;
    const double nom = R.lat;
    d3 part = mk3(0, 0, 0);
    int count = 0;
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {              // corner-code order, as in fused_drag
        const int g = B.vert_vox[(unsigned)corner * tm + i];
        if (g < 0) continue;
        const double hx = (1 + B.strain[((corner & 4) ? 0u : 3u) * nv + g]) * nom * 0.5;     // CornerPosCur / CornerNegCur
        const double hy = (1 + B.strain[((corner & 2) ? 1u : 4u) * nv + g]) * nom * 0.5;
        const double hz = (1 + B.strain[((corner & 1) ? 2u : 5u) * nv + g]) * nom * 0.5;
        const RotFwd M(mkq(QUAT(0, g), QUAT(1, g), QUAT(2, g), QUAT(3, g)));
        part = part + (mk3(POS(cur, 0, g), POS(cur, 1, g), POS(cur, 2, g)) + M(mk3((corner & 4) ? hx : -hx, (corner & 2) ? hy : -hy, (corner & 1) ? hz : -hz)));
        ++count;
    }
    const double inv = vrcp((double)count);
    const d3 v0 = mk3(B.vert_v0[i], B.vert_v0[tm + i], B.vert_v0[2u * tm + i]);
    const d3 np = part * inv;
    const d3 now = v0 + (np - v0);                            // v + DrawOffset, as the reference stores it
    B.mesh_pos[i] = now.x; B.mesh_pos[tm + i] = now.y; B.mesh_pos[2u * tm + i] = now.z;
}

static __global__ __launch_bounds__(256) void k_facets(DBatch B)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= B.n_facet) return;
    const int r = B.facet_robot[f];
    const DRobot& R = B.robot[r];
    const DRobotState& rs = B.rstate[r];
    if (!B.streamed[r] || !(R.flags & RF_FLUID) || !rs.active) return;
    const unsigned tm = B.total_mv, tf = B.total_facet;
    const int u = R.vox_begin + B.facet_vox[f];
    const d3 speed = mk3(LINMOM(0, u), LINMOM(1, u), LINMOM(2, u)) * B.vclass_tab[R.vtab_begin + B.vclass[u]].mass_inv;
    const unsigned ia = R.vert_begin + B.facet_vert[f], ib = R.vert_begin + B.facet_vert[tf + f], ic = R.vert_begin + B.facet_vert[2u * tf + f];
    const d3 contrib = facet_drag_force(speed, normalized3(speed), mk3(B.mesh_pos[ia], B.mesh_pos[tm + ia], B.mesh_pos[2u * tm + ia]),
                                        mk3(B.mesh_pos[ib], B.mesh_pos[tm + ib], B.mesh_pos[2u * tm + ib]),
                                        mk3(B.mesh_pos[ic], B.mesh_pos[tm + ic], B.mesh_pos[2u * tm + ic]), R.drag_coef);
    B.fdrag[f] = contrib.x; B.fdrag[tf + f] = contrib.y; B.fdrag[2u * tf + f] = contrib.z;
}

// blocks [0, bond_blocks): one thread per bond slot; blocks beyond: collision-list rebuilds (reb_robot/reb_i0 tables),
// which overlap with the bond work of the other robots
static __global__ __launch_bounds__(256) void k_bonds(DBatch B, int bond_blocks, const int* __restrict__ reb_robot, const int* __restrict__ reb_i0)
{
    if ((int)blockIdx.x >= bond_blocks) {
        __shared__ double sh[4 * 512 + 256];
        const int k = blockIdx.x - bond_blocks;
        const int r = reb_robot[k];
        DRobotState& rs = B.rstate[r];
        if (!B.streamed[r] || !rs.active || !rs.rebuild_now) return;
        const int i = reb_i0[k] + (int)threadIdx.x;
        rebuild_rows(B, B.robot[r], rs, PoseFromState{B, rs.steps & 1}, i, i < B.robot[r].nsurf, sh, 512);
        return;
    }
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= 3 * B.nv) return;
    const int axis = tid / B.nv;            // wave-uniform: nv is a multiple of 64
    const int v1 = tid - axis * B.nv;
    const int r = robot_of(B, v1);
    if (r < 0 || !B.streamed[r]) return;
    const DRobotState& rs = B.rstate[r];
    if (!rs.active) return;
    const int bc = B.bclass[tid];
    if (bc < 0) return;
    const DRobot& R = B.robot[r];
    if (axis == 0) stream_bond<0>(B, R, rs, r, tid, v1, bc);
    else if (axis == 1) stream_bond<1>(B, R, rs, r, tid, v1, bc);
    else stream_bond<2>(B, R, rs, r, tid, v1, bc);
}

static __global__ __launch_bounds__(256) void k_voxels(DBatch B)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= B.nv) return;
    const int r = robot_of(B, v);
    if (r < 0 || !B.streamed[r]) return;
    DRobotState& rs = B.rstate[r];
    if (!rs.active || rs.diverged) return;    // Integrate() returns before the voxel loop when a bond diverged
    const DRobot& R = B.robot[r];
    const bool valid = (v - R.vox_begin) < R.nvox;   // padding slots stay in the wave for the reduction below
    double vel2 = 0;
    if (valid) {
        const DVoxClass& C = B.vclass_tab[R.vtab_begin + B.vclass[v]];
        const int cur = rs.steps & 1, nxt = cur ^ 1;
        VoxState S;
        S.pos = mk3(POS(cur, 0, v), POS(cur, 1, v), POS(cur, 2, v));
        S.lm = mk3(LINMOM(0, v), LINMOM(1, v), LINMOM(2, v));
        S.am = mk3(ANGMOM(0, v), ANGMOM(1, v), ANGMOM(2, v));
        S.ang = mkq(QUAT(0, v), QUAT(1, v), QUAT(2, v), QUAT(3, v));
        S.scale = SCALE(cur, v);
        d3 vel = S.lm * C.mass_inv;           // Vel as left by the previous EulerStep (VXS_Voxel.cpp:409)
        // CalcTotalForce / CalcTotalMoment: fixed order PX,NX,PY,NY,PZ,NZ (VXS_Voxel.cpp:496-501,659-665)
        d3 F = (vel * (-R.slow_z)) * C.c_lin;
        d3 M = mk3(0, 0, 0);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (B.nbr[(2 * a) * B.nv + v] >= 0) {
                const int s = a * B.nv + v;
                F = F + mk3(BOUT(0, s), BOUT(1, s), BOUT(2, s));
                M = M - mk3(BOUT(3, s), BOUT(4, s), BOUT(5, s));
            }
            const int n = B.nbr[(2 * a + 1) * B.nv + v];
            if (n >= 0) {
                const int s = a * B.nv + n;
                F = F + mk3(BOUT(6, s), BOUT(7, s), BOUT(8, s));
                M = M - mk3(BOUT(9, s), BOUT(10, s), BOUT(11, s));
            }
        }
        int row = -1, ccnt = 0;
        if (R.flags & RF_SELF_COL) { const int so = B.surf_ord[v]; if (so >= 0) { row = R.surf_begin + so; ccnt = B.col_cnt[row]; } }
        const FetchGlobal fetch{B, cur};
        const bool fluid = (R.flags & RF_FLUID) != 0;
        d3 drag = mk3(0, 0, 0);
        if (fluid) {                          // my facets in the reference's order (k_facets ran earlier in this step)
            const unsigned tf = B.total_facet, f0 = R.facet_begin + B.facet_first[v];
            for (int j = 0; j < (int)B.facet_count[v]; ++j) drag = drag + mk3(B.fdrag[f0 + j], B.fdrag[tf + f0 + j], B.fdrag[2u * tf + f0 + j]);
        }
        vel2 = voxel_update(B, R, C, v, fetch, rs.cur_time, rs.act_sin, rs.act_cos, actuation_prenatal_c(R, rs.cur_time), F, M, vel, S, row, ccnt, fluid,
                             drag, B.act_sb[v], B.act_cb[v], B.amp_damp[v]);
        POS(nxt, 0, v) = S.pos.x; POS(nxt, 1, v) = S.pos.y; POS(nxt, 2, v) = S.pos.z;
        SCALE(nxt, v) = S.scale;
        LINMOM(0, v) = S.lm.x; LINMOM(1, v) = S.lm.y; LINMOM(2, v) = S.lm.z;
        ANGMOM(0, v) = S.am.x; ANGMOM(1, v) = S.am.y; ANGMOM(2, v) = S.am.z;
        QUAT(0, v) = S.ang.w; QUAT(1, v) = S.ang.x; QUAT(2, v) = S.ang.y; QUAT(3, v) = S.ang.z;
    }
    if (R.flags & RF_SELF_COL) {              // SS.MaxVoxVel for the collision horizon (VX_Sim.cpp:1625-1649)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { double o = __shfl_xor(vel2, off); vel2 = o > vel2 ? o : vel2; }
        if ((threadIdx.x & 63) == 0) atomicMax(&rs.maxvel2_bits, (unsigned long long)__double_as_longlong(vel2));
    }
}

}  // namespace vxh
