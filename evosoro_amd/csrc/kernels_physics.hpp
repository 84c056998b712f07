// Layer 2 of the device code of the batched Voxelyze time-stepper (gfx950): the physics of one bond, one voxel and one robot step.
// FP64 throughout, SoA state in HBM (device_types.hpp).  Reference loops being replaced (paths under evosoro/_voxcad/Voxelyze/):
//   step_control    CVX_Sim::TimeStep prologue + StopConditionMet + UpdateCollisions and the `CurTime += dt`
//                   epilogue (VX_Sim.cpp:1054-1135,1398-1423,1729-1755,1929)
//   rebuild_rows    CVX_Sim::CalcL1Bonds (VX_Sim.cpp:2357-2413)
//   bond_compute    CVXS_BondInternal::CalcLinForce / UpdateBondStrain / AddDampForces (VXS_BondInternal.cpp:56-346)
//   voxel_update    CVXS_Voxel::EulerStep / CalcTotalForce / CalcTotalMoment / CalcFloorEffect (VXS_Voxel.cpp:169-758),
//                   CVXS_BondCollision::CalcContactForce (VXS_BondCollision.cpp:41-59), MaxVoxVel of UpdateStats
// Four launch shapes share those device functions (the first three also the workgroup-level parts of kernels_group.hpp):
//   k_robot_steps<BLOCK,NACC,MESH,TABG,COST>  resident kernel (kernels_fused.hpp): ONE workgroup per robot (robots up to BLOCK voxels),
//                         the robot RESIDENT in the CU for a whole launch of many time steps: voxel momenta in registers,
//                         poses and force accumulators in LDS, bonds taken from per-axis compacted lists.  Per step only
//                         the bond history crosses L2/HBM.
//   k_robot_wide<512,MESH,TABG>  wide kernel (kernels_wide.hpp): one workgroup per SMALL robot, more threads than voxels: every bond a lane of its
//                         own, all three axes in one round.
//   k_tile_steps<TABG,MESH,FLUID,SMALL>  tiled kernel (kernels_tiled.hpp): a robot cut into tiles, one workgroup each, poses exchanged
//                         through memory.
//   k_step_begin / k_bonds / k_voxels   streaming kernels (kernels_stream.hpp) for lattices of any size (one thread per bond slot / voxel,
//                         state and bond outputs through HBM).
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.hpp"
#include "kernels_math.hpp"

namespace vxh {

// SoA component planes behind three base pointers (few SGPRs): see DBatch in device_types.hpp
#define VS(comp, v) B.vs[(unsigned)(comp) * (unsigned)B.nv + (unsigned)(v)]
#define POS(cur, k, v) VS((cur) * 4 + (k), v)
#define SCALE(cur, v) VS((cur) * 4 + 3, v)
#define QUAT(k, v) VS(8 + (k), v)
#define LINMOM(k, v) VS(12 + (k), v)
#define ANGMOM(k, v) VS(15 + (k), v)
#define HIST(k, slot) B.hist[(unsigned)(k) * 3u * (unsigned)B.nv + (unsigned)(slot)]
#define BOUT(k, slot) B.bout[(unsigned)(k) * 3u * (unsigned)B.nv + (unsigned)(slot)]

// Contact rows (DBatch::col_partner / col_a1 / col_code): robot r owns the block [col_begin, col_begin + col_cap * nsurf), entry k of
// the row of its surface voxel i at col_begin + k * nsurf + i (partner-major inside the block: coalesced across a wavefront).
// `row` = the batch-wide row number surf_begin + i, as DBatch::col_cnt is indexed.
__device__ __forceinline__ size_t col_at(const DRobot& R, int k, int row)
{
    return (size_t)R.col_begin + (size_t)k * (size_t)R.nsurf + (size_t)(row - R.surf_begin);
}

__device__ __forceinline__ int robot_of(const DBatch& B, int vslot)
{
    return __builtin_amdgcn_readfirstlane(B.wave_robot[vslot >> 6]);
}

struct BondOut { d3 f1, m1, f2, m2; double strain1, strain2; bool diverged; };
// History of one bond in the 6-double layout of DBatch::hist + its flag bits (bit 0 SmallAngle, bit 1 large layout).
// Loaded by the caller BEFORE the arithmetic and stored after it, so the memory operations of a bond are issued
// together instead of being scattered through the math.
struct BondHist { double p0, p1, p2, g0, g1, g2; unsigned flags; bool store_hist; };

__device__ __forceinline__ BondHist load_bond_hist(const DBatch& B, int slot)
{
    BondHist h;
    h.p0 = HIST(0, slot); h.p1 = HIST(1, slot); h.p2 = HIST(2, slot);
    h.g0 = HIST(3, slot); h.g1 = HIST(4, slot); h.g2 = HIST(5, slot);
    h.flags = B.small_angle[slot];
    h.store_hist = false;
    return h;
}
__device__ __forceinline__ void store_bond_hist(const DBatch& B, int slot, const BondHist& h, unsigned old_flags)
{
    if (h.store_hist) {
        HIST(0, slot) = h.p0; HIST(1, slot) = h.p1; HIST(2, slot) = h.p2;
        HIST(3, slot) = h.g0; HIST(4, slot) = h.g1; HIST(5, slot) = h.g2;
    }
    if (h.flags != old_flags) B.small_angle[slot] = (unsigned char)h.flags;
}

// One internal bond in the BOND frame (the bond lies along +x: the caller has applied ToXDirBond to the relative position and
// to both orientations): pure arithmetic, `H` in/out.  The outputs are still in the permuted global frame (the caller applies
// ToOrigDirBond); f2 is only computed for heterogeneous bonds (F2 = -F1 is enforced after the back-rotation otherwise).
// damp_on = a previous step exists (no damping on the first one, dt == 0 then: VXS_BondInternal.cpp:311).
template <bool SEL = false>
__device__ __forceinline__ BondOut bond_compute_xframe(const DBatch& B, const DBondClass& C, BondHist& H,
                                                       d3 xrel, dq a1, dq a2, double nom_dist, bool damp_on)
{
    BondOut o;
    d3 rel = rotinv(a1, xrel);
    // Angle2 in voxel 1's frame, conj(a1) a2 (NewAng2): its w now, for the mode test; the vector part only where it is used, in the
    // small-angle branch (a wavefront of large-angle bonds skips those 12 operations)
    const double new2w = a1.w * a2.w + a1.x * a2.x + a1.y * a2.y + a1.z * a2.z;

    // small/large-angle switch with hysteresis (VXS_BondInternal.cpp:72-77).  SmallTurn = (|z|+|y|)/x and
    // ExtendPerc = x/NomDistance are only ever compared with constants, so the comparisons are made on the
    // cross-multiplied form (no division); the sign cases keep the IEEE outcome of the quotient (x < 0: quotient <= 0,
    // x == 0: +inf or NaN).
    // (Round 6: written as lane masks -- bitwise operators on the comparisons' results -- instead of nested ifs: the compiler had turned
    // every `if` into a save-exec / branch pair, a dozen scalar round trips at the head of a chain that issues one instruction per ~7
    // cycles; the same truth table, NaN cases included: rel.x unordered -> neither xpos nor xneg -> the reference's `else` arm.)
    bool small = (H.flags & 1u) != 0, changed = false;
    {
        const double t = fabs(rel.z) + fabs(rel.y);
        const bool xpos = rel.x > 0, xneg = rel.x < 0;
        const bool turn_lt = (xpos & (t < VXH_SA_BOND_BEND_RAD * rel.x)) | xneg;                                  // SmallTurn < BEND
        const bool turn_gt = (xpos & (t > (VXH_HYST * VXH_SA_BOND_BEND_RAD) * rel.x)) | (!xpos & !xneg & (t > 0));   // SmallTurn > HYST * BEND
        const bool ext_lt = rel.x < VXH_SA_BOND_EXT_PERC * nom_dist, ext_gt = rel.x > (VXH_HYST * VXH_SA_BOND_EXT_PERC) * nom_dist;
        const bool to_small = !small & (new2w > B.small_angle_w) & turn_lt & ext_lt;
        const bool to_large = small & (!(new2w > B.smallish_angle_w) | turn_gt | ext_gt);
        changed = to_small | to_large;
        small = (small | to_small) & !to_large;
    }
    // (Round 4, measured: a wavefront whose 64 bonds are of both modes runs both branches below, and in the bench population 6 % of the
    // bonds are small-angle, so nearly every wavefront does.  The ceiling of sorting the bonds by mode -- every bond forced large-angle, the
    // small branch compiled out, timing only -- is 25.15 -> 24.92 us per step: not worth a per-launch re-sort of DBatch::bsched.)

    // Angle1 is (0, y, z) in both modes: zero in the small one, and the rotation vector of FromAngleToPosX's quaternion, whose x is
    // an exact zero, in the large one -- the x component is left out of everything below (0 - a == -a, a - 0 == a: the same bits)
    d3 pos2;
    double ang1y, ang1z;
    dq rot, qb2;                               // qb2: Angle2 in the bond frame
    if (small) {
        ang1y = 0; ang1z = 0;
        qb2 = mkq(new2w, a1.w * a2.x - a1.x * a2.w - a1.y * a2.z + a1.z * a2.y,
                         a1.w * a2.y + a1.x * a2.z - a1.y * a2.w - a1.z * a2.x,
                         a1.w * a2.z - a1.x * a2.y + a1.y * a2.x - a1.z * a2.w);      // qmul(conj(a1), a2)
        pos2 = mk3(rel.x - nom_dist, rel.y, rel.z);
        rot = conj(a1);
    } else {
        double len;
        const dq align = from_angle_to_pos_x(rel, len);
        rot = qmul_x0(align, conj(a1));
        pos2 = mk3(len - nom_dist, 0, 0);
        const double f1 = rotvec_factor<SEL>(align.w, B.slthresh_acos2sqrt);
        ang1y = align.y * f1; ang1z = align.z * f1;
        qb2 = qmul(rot, a2);               // (re-associated as align (conj(a1) a2): needs all of conj(a1) a2, 12 operations more than it saves)
    }
    const d3 ang2 = to_rotvec<SEL>(qb2, B.slthresh_acos2sqrt);   // one instance for both modes: a mixed wave runs it once

    // axial stress (UpdateBondStrain, VXS_BondInternal.cpp:189-307; linear materials): the reference's series-spring
    // iteration is linear in the strain = elongation / L, its three factors (with the 1 / L) are constants of the bond
    // class (model.cpp make_bond_class, DBondClass)
    o.strain1 = C.strain_a1_L * pos2.x;        // CurStrainV1 / CurStrainV2 (SetStrainDir), read by the land_water surface mesh
    o.strain2 = C.strain_a2_L * pos2.x;
    o.diverged = pos2.x > C.L100;              // strain > 100, VX_Sim.cpp:1775

    // beam equations (VXS_BondInternal.cpp:128-153)
    d3 f1 = mk3(C.kf_L * pos2.x, C.b1 * pos2.y - C.b2 * (ang1z + ang2.z), C.b1 * pos2.z + C.b2 * (ang1y + ang2.y));
    d3 f2 = -f1;
    const double tors = C.a2 * ang2.x;         // a2 (Angle2.x - Angle1.x); Moment1.x is its negative
    d3 m1 = mk3(-tors, C.b2 * pos2.z + C.b3 * (2 * ang1y + ang2.y), -C.b2 * pos2.y + C.b3 * (2 * ang1z + ang2.z));
    d3 m2 = mk3(tors, C.b2 * pos2.z + C.b3 * (ang1y + 2 * ang2.y), -C.b2 * pos2.y + C.b3 * (ang1z + 2 * ang2.z));

    // velocity damping from the finite-differenced bond-frame pose (AddDampForces :310-346); skipped on the step the
    // mode flips, and the history is only refreshed when it runs
    if (!changed) {
        if (damp_on) {
            const bool hl = (H.flags & 2u) != 0;        // expand the stored history (see DBatch::hist)
            const d3 hpos2 = mk3(H.p0, hl ? 0.0 : H.p1, hl ? 0.0 : H.p2);
            const double hang1y = hl ? H.p1 : 0.0, hang1z = hl ? H.p2 : 0.0;
            const d3 hang2 = mk3(H.g0, H.g1, H.g2);
            // differences of the bond-frame pose; 1/dt and BondDampingZ/2 are inside the d* constants (DBondClass)
            const d3 v = pos2 - hpos2, w2 = ang2 - hang2;
            const double w1y = ang1y - hang1y, w1z = ang1z - hang1z;      // (w1.x == 0)
            f1 = f1 + mk3(C.dA1 * v.x, C.dB1 * v.y - C.dF1 * (w1z + w2.z), C.dB1 * v.z + C.dF1 * (w1y + w2.y));
            if (!C.homogeneous)
                f2 = f2 + mk3(-C.dA2 * v.x, -C.dB2 * v.y + C.dF2 * (w1z + w2.z), -C.dB2 * v.z - C.dF2 * (w1y + w2.y));
            m1 = m1 + mk3(-C.dT1 * w2.x, C.dG1 * v.z + C.dH1 * (2 * w1y + w2.y), -C.dG1 * v.y + C.dH1 * (2 * w1z + w2.z));
            m2 = m2 + mk3(C.dT2 * w2.x, C.dG2 * v.z + C.dH2 * (w1y + 2 * w2.y), -C.dG2 * v.y + C.dH2 * (w1z + 2 * w2.z));
        }
        // _LastPos2 / _LastAngle1 / _LastAngle2 in the layout of the mode that produced them (ang1 == 0 in small mode;
        // pos2.y == pos2.z == ang1.x == 0 in large mode)
        H.p0 = pos2.x; H.p1 = small ? pos2.y : ang1y; H.p2 = small ? pos2.z : ang1z;
        H.g0 = ang2.x; H.g1 = ang2.y; H.g2 = ang2.z;
        H.flags = (small ? 1u : 2u);
        H.store_hist = true;
    } else {
        H.flags = (H.flags & 2u) | (small ? 1u : 0u);
    }

    // back to the global frame (:158-171): three or four vectors go through the same RotateVec3DInv(rot, .), so the
    // rotation is expanded once into its matrix (conj(q) v q = R^T v for a unit quaternion; |rot| = 1 to rounding)
    const RotInv T(rot);
    o.f1 = T(f1);
    if (!C.homogeneous) o.f2 = T(f2);
    o.m1 = T(m1);
    o.m2 = T(m2);
    return o;
}

// ... along axis A between voxel 1 (negative side) and voxel 2, the axis a compile-time constant (fused and streaming kernels)
template <int A, bool SEL = false>
__device__ __forceinline__ BondOut bond_compute(const DBatch& B, const DBondClass& C, BondHist& H,
                                                d3 p1, dq q1, double s1, d3 p2, dq q2, double s2,
                                                bool damp_on)
{
    BondOut o = bond_compute_xframe<SEL>(B, C, H, to_xdir<A>(p2 - p1), to_xdir<A>(q1), to_xdir<A>(q2), (s1 + s2) * 0.5, damp_on);
    o.f1 = to_orig<A>(o.f1);
    o.f2 = C.homogeneous ? -o.f1 : to_orig<A>(o.f2);
    o.m1 = to_orig<A>(o.m1);
    o.m2 = to_orig<A>(o.m2);
    return o;
}

// ... the axis a per-lane run-time value (tiled kernel: one flat bond list per tile, all axes in one round).  The same
// permutations as to_xdir<A> / to_orig<A> written with selects: bit-identical results (negation is exact).
__device__ __forceinline__ BondOut bond_compute_rt(int axis, const DBatch& B, const DBondClass& C, BondHist& H,
                                                   d3 p1, dq q1, double s1, d3 p2, dq q2, double s2, bool damp_on)
{
    BondOut o = bond_compute_xframe(B, C, H, to_xdir_rt(axis, p2 - p1), to_xdir_rt(axis, q1), to_xdir_rt(axis, q2), (s1 + s2) * 0.5, damp_on);
    o.f1 = to_orig_rt(axis, o.f1);
    o.f2 = C.homogeneous ? -o.f1 : to_orig_rt(axis, o.f2);
    o.m1 = to_orig_rt(axis, o.m1);
    o.m2 = to_orig_rt(axis, o.m2);
    return o;
}

// ---- land_water surface mesh and fluid drag (LW/VX_Sim.cpp:1516-1597), arithmetic shared by the resident kernel
// (kernels_fused.hpp: fused_drag) and the streaming kernels (k_mesh_vertices / k_facets below).  Every deformable surface
// vertex = mean over the <= 7 voxels touching that lattice corner of Pos + R(Angle) * corner offset, corner offsets from the
// bond strains of the PREVIOUS step (CornerPosCur/CornerNegCur, LW/VXS_Voxel.cpp:472-475; GetCurVLoc
// LW/VX_MeshUtil.cpp:388-428); every voxel sums the quadratic drag of the two triangles on each of its exposed faces, in the
// reference's facet order.
// drag of one facet (A, Bv, Cv) on its voxel moving with `speed` (sdir = speed normalised)
__device__ __forceinline__ d3 facet_drag_force(d3 speed, d3 sdir, d3 A, d3 Bv, d3 Cv, double drag_coef)
{
    const d3 AB = Bv - A, AC = Cv - A;
    const d3 cr = cross3(AB, AC);
    const double cl = vsqrt_nn(len2(cr));
    const double area = cl * 0.5;
    const d3 n = cl > 0 ? cr * vrcp(cl) : cr;           // CalcFaceNormals; the reference normalises the stored normal
                                                        // twice more before using it: identity to an ulp, skipped
    // LW/VX_Sim.cpp:1556-1559 tests (float)acos(c) < PI/2 with c = v^ . n^.  The largest float below PI/2 is
    // 1.57079625 and acos(c) rounds to it or below iff acos(c) <= 1.570796310901641845703125 (the midpoint
    // to the next float, a tie going to the even mantissa below), i.e. iff c >= cos(midpoint); c > 1
    // (two parallel unit vectors, rounding) makes the reference's acos a NaN and the facet drag-free.
    const double c = dot3(sdir, n);
    d3 contrib = mk3(0, 0, 0);
    if (c >= 1.5893254773528196e-08 && c <= 1.0) {
        const d3 proj = n * dot3(speed, n);             // ProjectOnTo
        // proj^ * (-k * area * |proj|^2) = proj * (-k * area * |proj|)
        contrib = proj * (-drag_coef * area * vsqrt_nn(len2(proj)));
    }
    return contrib;
}

struct VoxState { d3 pos, lm, am; dq ang; double scale; };

// CalcContactForce (VXS_BondCollision.cpp:41-59) of one listed partner at (qx, qy, qz), scale qs, on the voxel at `pos`: Force2 =
// unit(p2 - p1) * a1 * overlap on Vox2 (the later surface voxel), -Force2 on Vox1.  Seen from this voxel that is
// -unit(partner - me) * a1 * overlap in both roles, bit for bit (negation is exact, the sums commute).
// The function is inlined into every stepping kernel (resident: LDS rows and rows in memory; tiled; streaming); its roundings are
// pinned -- every product and sum rounded on its own, like the reference's x86-64 build, which has no fused multiply-add -- so
// that all of these sites produce the same bits: with contraction left to the compiler two sites of one kernel came out differently
// (measured: scripts/dev_gpu_diag.py contactcheck).  contact_in_reach is the reject test alone (resident kernel, pass 1).
#pragma clang fp contract(off)
__device__ __forceinline__ bool contact_in_reach(double dx, double dy, double dz, double nom)
{
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    return d2 < nom * nom;
}
__device__ __forceinline__ d3 contact_force_add(d3 F, d3 pos, double scale, double qx, double qy, double qz, double qs, double a1)
{
    const double dx = qx - pos.x, dy = qy - pos.y, dz = qz - pos.z;
    const double nom = (qs + scale) * 0.75;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 < nom * nom) {                                  // cheap reject: most listed partners are out of reach
        const double l = vsqrt_nn(d2);
        const double reld = nom - l;
        if (reld > 0) {
            const double il = vrcp(l);
            F.x = F.x - ((dx * il) * a1) * reld;
            F.y = F.y - ((dy * il) * a1) * reld;
            F.z = F.z - ((dz * il) * a1) * reld;
        }
    }
    return F;
}
#pragma clang fp contract(fast)

// position + scale of another voxel of the same robot, for the contact forces
struct FetchGlobal {       // streaming path: previous-step buffer in HBM
    const DBatch& B; int cur;
    __device__ __forceinline__ void operator()(int slot, double& x, double& y, double& z, double& s) const
    { x = POS(cur, 0, slot); y = POS(cur, 1, slot); z = POS(cur, 2, slot); s = SCALE(cur, slot); }
};
template <int BLOCK>
struct FetchLds {          // fused path: the workgroup's pose tile
    const double* ps; int base;
    __device__ __forceinline__ void operator()(int slot, double& x, double& y, double& z, double& s) const
    { const int l = slot - base; x = ps[l]; y = ps[BLOCK + l]; z = ps[2 * BLOCK + l]; s = ps[3 * BLOCK + l]; }
};

// per-voxel development parameters (float members of CVXS_Voxel, VXS_Voxel.h:92-111), only loaded for RF_DEV robots
struct DevParams { float init_size, final_size, start_growth, growth_time, phase, final_phase, final_tad; };
__device__ __forceinline__ DevParams load_dev(const DBatch& B, int v)
{
    DevParams d;
    const unsigned nv = B.nv;
    d.init_size = B.dev[v]; d.final_size = B.dev[nv + v]; d.start_growth = B.dev[2 * nv + v]; d.growth_time = B.dev[3 * nv + v];
    d.phase = B.dev[4 * nv + v]; d.final_phase = B.dev[5 * nv + v]; d.final_tad = B.dev[6 * nv + v];
    return d;
}

// Everything of EulerStep after the internal-bond sums, in two independent halves (a voxel's translation and its rotation + size
// never read each other's results within a step): voxel_update_lin -- collision bonds, gravity, drag, floor, linear integration --
// and voxel_update_ang -- angular integration, quaternion update, actuation -> new scale.  voxel_update runs one after the other on
// one lane (resident, tiled and streaming kernels); the wide kernel (kernels_wide.hpp) gives the halves of a small robot's voxels
// to different wavefronts.
// F arrives holding slow damping + internal bond forces.  `scale`: the voxel's size at the start of the step.  Returns |new velocity|^2.
template <class Fetch>
__device__ __forceinline__ double voxel_update_lin(const DBatch& B, const DRobot& R, const DVoxClass& C, int v, const Fetch& fetch,
                                                   d3 F, d3 vel, d3& pos, d3& lm, double scale, int row, int ccnt, bool fluid, d3 drag)
{
    // (v: global voxel slot = what the contact rows and `fetch` speak)
    const int flags = R.flags;
    const double dt = R.dt;
    if (ccnt > 0) {
        // collision bonds in creation order (VXS_Voxel.cpp:519-530, VXS_BondCollision.cpp:41-59); partner slots and the
        // pair stiffness a1 were stored by rebuild_rows.  Loads are issued four partners at a time.
        for (int k0 = 0; k0 < ccnt; k0 += 4) {
            int o[4]; double a1[4], qx[4], qy[4], qz[4], qs[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool on = k0 + j < ccnt;
                const size_t at = col_at(R, k0 + j, row);                // partner-major: coalesced across the wave
                o[j] = on ? B.col_partner[at] : -1;
                a1[j] = on ? B.col_a1[at] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) fetch(o[j] < 0 ? v : o[j], qx[j], qy[j], qz[j], qs[j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (o[j] < 0) continue;
                F = contact_force_add(F, pos, scale, qx[j], qy[j], qz[j], qs[j], a1[j]);
            }
        }
    }
    if ((flags & RF_GRAV) && !fluid) F.z += C.mass * R.grav_acc;
    if (fluid) F = F + drag;                  // LW/VXS_Voxel.cpp:372-373

    if ((flags & RF_FLOOR) && !fluid) {       // CalcFloorEffect, VXS_Voxel.cpp:708-758
        const double pen = 0.5 * scale - pos.z;
        bool static_fric = false;
        if (pen > 0) {
            const double normal = C.k_floor * pen;
            const double fz = normal - R.col_z * C.c_lin * vel.z;
            const double surf_vel = vsqrt_nn(vel.x * vel.x + vel.y * vel.y);
            const double surf_force = vsqrt_nn(F.x * F.x + F.y * F.y);
            const double fric = C.u_dynamic * normal;
            double fx = 0, fy = 0;
            bool stopped = (vel.x == 0 && vel.y == 0);
            if (flags & RF_STICKY) { lm.x = 0; lm.y = 0; static_fric = true; stopped = true; }
            if (stopped) {
                if (surf_force < C.u_static * normal) static_fric = true;
            } else if (fric * dt < C.mass * surf_vel) {
                // -(cos, sin)(atan2(vy, vx)) * fric == -(vx, vy)/|v| * fric
                const double inv = vdiv(fric, surf_vel);
                fx = -vel.x * inv; fy = -vel.y * inv;
            } else { static_fric = true; lm.x = 0; lm.y = 0; }
            F.x += fx; F.y += fy; F.z += fz;
        }
        if (static_fric) { F.x = 0; F.y = 0; }
    }

    // EulerStep, VXS_Voxel.cpp:183-189
    lm = lm + F * dt;
    pos = pos + lm * (dt * C.mass_inv);
    return len2(lm * C.mass_inv);
}

// M arrives holding minus the internal bond moments.  `scale` in: the size at the start of the step, out: the new one.
__device__ __forceinline__ void voxel_update_ang(const DBatch& B, const DRobot& R, const DVoxClass& C, int v, double t, double act_sin,
                                                 double act_cos, double prenatal_c, d3 M, d3& am, dq& q, double& scale,
                                                 double ph_sin, double ph_cos, float amp_damp)
{
    const int flags = R.flags;
    const double dt = R.dt;
    // EulerStep, VXS_Voxel.cpp:190-222
    am = am + M * dt;
    const double amf = 1 - 10 * R.slow_z * C.inertia_inv * C.c_ang * dt;
    am = am * amf;
    d3 w = am * C.inertia_inv;
    dq spin = qmul(mkq(0, w.x * 0.5, w.y * 0.5, w.z * 0.5), q);
    dq ang = mkq(q.w + spin.w * dt, q.x + spin.x * dt, q.y + spin.y * dt, q.z + spin.z * dt);
    {
        // NormalizeFast with the reference's own two roundings (sqrt, then 1 / l): the `w >= 1 -> identity` snap below
        // discards rotations smaller than ~1.5e-8 rad, and whether w lands on 1.0 depends on the last bit of 1 / l
        // (a single-rounding rsqrt here moved probe6 by 5e-9 voxel within ten steps)
        const double l = vsqrt_nn(ang.x * ang.x + ang.y * ang.y + ang.z * ang.z + ang.w * ang.w);
        if (l != 0) { const double li = vrcp(l); ang.w *= li; ang.x *= li; ang.y *= li; ang.z *= li; }
        if (ang.w >= 1.0) ang = mkq(1.0, 0, 0, 0);
    }
    q = ang;

    // thermal actuation -> new scale (VXS_Voxel.cpp:224-340 without development; LW/VXS_Voxel.cpp:211-235)
    // sin(2 pi' (t/T + phase)) of the reference = sin(a + b) with a = 2 pi' t/T, the same for every voxel (sincos once
    // per robot and step, actuation_sincos), and b = 2 pi' phase, fixed per voxel (DBatch::act_sb / act_cb)
    double new_scale;
    const double act = act_sin * ph_cos + act_cos * ph_sin;
    if (!(flags & RF_LW) && (flags & RF_DEV)) {
        // _voxcad with development layers (VXS_Voxel.cpp:236-340; the reference mixes float members and double locals, kept)
        const DevParams D = load_dev(B, v);
        const double nom = C.nom_size;
        const double prenatal = prenatal_c * (((double)D.init_size / nom) - 1);
        double dev_tf = 0, dphase = 0, dtad = 0, frozen = 0, freeze_init = 1;
        if (R.midlife_freeze_time > 0) {                                 // :247-264
            const double middle = 0.5 * (R.stop_value - R.init_cm_time);
            const double fs = middle - 0.5 * R.midlife_freeze_time, fe = middle + 0.5 * R.midlife_freeze_time;
            if (t > fs && t < fe) { frozen = t - fs; if (t < fs + R.init_cm_time) freeze_init = 0; }
            if (t > fe) frozen = R.midlife_freeze_time;
        }
        if (t >= (double)D.start_growth && D.growth_time > 0) {          // postnatal linear development :267-296
            const float sg = D.start_growth + D.growth_time;             // float sum, as in the reference
            double eff = (t <= (double)sg + R.midlife_freeze_time) ? t : (double)sg + R.midlife_freeze_time;
            eff = eff - frozen;
            const double k = (eff - (double)D.start_growth) / (double)D.growth_time;
            if (flags & RF_DEV_FSIZE) { const float ratio = D.final_size / D.init_size; dev_tf = k * ((double)ratio - 1.0); }
            if (flags & RF_DEV_FPHASE) { const float d = D.final_phase - D.phase; dphase = k * (double)d; }
            if (flags & RF_DEV_FTAD) { const float d = D.final_tad - amp_damp; dtad = k * (double)d; }
        }
        double ctrl = 0;
        if ((flags & RF_TEMP) && t >= R.init_cm_time)
            ctrl = ((double)amp_damp + dtad) * ((double)R.temp_amplitude * sin((double)(2 * 3.1415926f) * (t / (double)R.temp_period + ((double)D.phase + dphase)))) * C.cte * freeze_init;
        if (flags & RF_DEV_SIZE) {                                       // actuation limited by the current size :316-328
            const double cur_size = (1 + prenatal) * (1 + dev_tf) * nom;
            const double sig = ((cur_size / nom - 1) / R.growth_amplitude + 1) * 0.5;
            ctrl = ctrl * (sig > 0.5 ? 0.5 : sig) * 2;
        }
        new_scale = ctrl * nom + (1 + prenatal) * (1 + dev_tf) * nom;
        const double max_scale = (1 + R.growth_amplitude) * nom, min_scale = R.min_temp_fact * nom;
        if (new_scale < scale && new_scale < min_scale) new_scale = scale;
        if (new_scale > scale && new_scale > max_scale) new_scale = scale;
    } else if (!(flags & RF_LW)) {
        const double prenatal = prenatal_c * C.prenatal_k;       // prenatal_c * ((float)nom / nom - 1), the quotient formed at import (same rounding)
        double ctrl = 0;
        if ((flags & RF_TEMP) && t >= R.init_cm_time)
            ctrl = (double)amp_damp * ((double)R.temp_amplitude * act) * C.cte;
        new_scale = ctrl * C.nom_size + (1 + prenatal) * C.nom_size;
        const double max_scale = (1 + R.growth_amplitude) * C.nom_size, min_scale = R.min_temp_fact * C.nom_size;
        if (new_scale < scale && new_scale < min_scale) new_scale = scale;
        if (new_scale > scale && new_scale > max_scale) new_scale = scale;
    } else {
        double tf = 1.0;
        if ((flags & RF_TEMP) && t >= R.init_cm_time)
            tf = 1 + ((double)R.temp_amplitude * act) * C.cte;
        if (tf < 0.1) tf = 0.1;
        new_scale = tf * C.nom_size;
    }
    scale = new_scale;
}

template <class Fetch>
__device__ __forceinline__ double voxel_update(const DBatch& B, const DRobot& R, const DVoxClass& C, int v, const Fetch& fetch,
                                               double t, double act_sin, double act_cos, double prenatal_c, d3 F, d3 M, d3 vel,
                                               VoxState& S, int row, int ccnt, bool fluid, d3 drag, double ph_sin, double ph_cos, float amp_damp)
{
    const double vel2 = voxel_update_lin(B, R, C, v, fetch, F, vel, S.pos, S.lm, S.scale, row, ccnt, fluid, drag);
    voxel_update_ang(B, R, C, v, t, act_sin, act_cos, prenatal_c, M, S.am, S.ang, S.scale, ph_sin, ph_cos, amp_damp);
    return vel2;
}

// uniform per-step factors of the actuation, evaluated once per robot and step instead of once per voxel
__device__ __forceinline__ void actuation_sincos(const DRobot& R, double t, double& s, double& c)
{
    s = 0; c = 0;
    if ((R.flags & RF_TEMP) && t >= R.init_cm_time) sincos((double)(2 * 3.1415926f) * (t / (double)R.temp_period), &s, &c);
}
__device__ __forceinline__ double actuation_prenatal_c(const DRobot& R, double t) { return (t >= 0.5 * R.init_cm_time) ? 1.0 : 2 * t / R.init_cm_time; }

// ------------------------------------------------------------------------------------- per-robot step control
// `trace`: mask of the traces that get a point from this step (bit VXH_TRACE_LIFE / _AFTERLIFE / _FROZEN); `trace_index`: entry of the life trace
struct StepCtl { int go, latch, eol, rebuild, trace, trace_index; };

// One point of a RF_NORM_VOL robot's traces (executed by the one thread that holds the sums): the volume next to the life trace's entry,
// a whole entry of the after-life / frozen trace.  `cm`: GetCM() of the step, `vol`: getTotalVolume().
__device__ __forceinline__ void store_norm_vol_points(const DBatch& B, const DRobot& R, const DRobotState& rs, int mask, int life_index,
                                                      double cx, double cy, double cz, double vol)
{
    if (mask & (1 << VXH_TRACE_LIFE)) B.trace_vol[R.vol_begin + life_index] = vol;
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (mask & (2 << k)) {
            double* e = B.xtrace + (size_t)(R.xt_begin[k] + rs.nxtrace[k] - 1) * 5;
            e[0] = rs.cur_time; e[1] = cx; e[2] = cy; e[3] = cz; e[4] = vol;
        }
}

// Executed by ONE thread per robot before every step (and once after the last): completes the previous step's
// accounting, evaluates the stop condition and decides what this step needs.  Two parts: step_control_begin needs
// nothing of the previous step's voxel phase; step_control_horizon consumes its MaxVoxVel.
__device__ __forceinline__ StepCtl step_control_begin(const DRobot& R, DRobotState& rs, long long step_cap, int begin_new_step)
{
    StepCtl c; c.go = c.latch = c.eol = c.rebuild = c.trace = c.trace_index = 0;
    if (rs.status != 0) return c;
    if (rs.active) {                         // finish the step the previous round computed
        if (rs.diverged) rs.status = 2;
        else {
            const double t_before = rs.cur_time;
            rs.cur_time += R.dt; rs.steps += 1; rs.dt_prev = R.dt;
            // UpdateStats of that step (VX_Sim.cpp:1537-1547): a point of the centre-of-mass trace is due; the pass that latches
            // IniCM computes it from the poses the step left (also when the robot stops now: c.go stays 0, c.trace is set)
            if (R.trace_dt > 0 && rs.cur_time > R.init_cm_time && (rs.ntrace == 0 || rs.last_trace_time + R.trace_dt <= rs.cur_time)) {
                if (rs.ntrace < R.trace_cap) { c.trace = 1 << VXH_TRACE_LIFE; c.trace_index = rs.ntrace; }
                rs.ntrace += 1; rs.last_trace_time = rs.cur_time;
            }
            // <NormDistByVol>: the after-life and the frozen trace (:1549-1565, :1580-1596), each with the cadence of its own.  Their points go
            // to entry nxtrace - 1 of the robot's range (latch_cm / fused_latch_cm read the index from the control block).  DevelopmentFrozen is
            // what the top of that TimeStep set (:1090-1104) from the time BEFORE the step; UpdateStats uses it with the time after it.
            if (R.flags & RF_NORM_VOL) {
                bool due[2];
                due[0] = R.afterlife > 0 && rs.cur_time > R.stop_value;
                due[1] = false;
                if (R.midlife_freeze_time > 0) {
                    const double middle = 0.5 * (R.stop_value - R.init_cm_time);
                    const double fs = middle - 0.5 * R.midlife_freeze_time, fe = middle + 0.5 * R.midlife_freeze_time;
                    due[1] = t_before > fs + R.init_cm_time && t_before < fe;
                }
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    if (due[k] && (rs.nxtrace[k] == 0 || rs.last_xtrace_time[k] + R.trace_dt <= rs.cur_time)) {
                        if (rs.nxtrace[k] < R.xt_cap[k]) c.trace |= 2 << k;
                        rs.nxtrace[k] += 1; rs.last_xtrace_time[k] = rs.cur_time;
                    }
            }
        }
        rs.active = 0;
    }
    if (rs.status != 0) return c;
    const double t = rs.cur_time;
    bool stop = false;                       // StopConditionMet, VX_Sim.cpp:1398-1423 (LW/VX_Sim.cpp:1160-1172)
    if ((R.flags & RF_LW) || !(t <= R.init_cm_time)) {
        if (R.stop_type == 1) stop = rs.steps > (int)(R.stop_value + 0.5);
        else if (R.stop_type == 2) stop = t > (R.stop_value + R.afterlife);
        else if (R.stop_type == 3) stop = t > R.temp_period_d * R.stop_value;
    }
    if (stop) { rs.status = 1; return c; }
    if (!begin_new_step || (long long)rs.steps >= step_cap) return c;
    c.go = 1;
    if (!rs.cm_init && t > R.init_cm_time) c.latch = 1;                          // VX_Sim.cpp:1064
    if (!(R.flags & RF_LW) && t >= R.stop_value && rs.eol_post_y == 0) c.eol = 1;   // :1078
    rs.active = 1;
    return c;
}
// (dt_prev: the step length of the step before the one being decided -- rs.dt_prev, unless the caller has already let
// step_control_begin of the NEXT step overwrite it)
__device__ __forceinline__ void step_control_horizon(const DRobot& R, DRobotState& rs, StepCtl& c, double dt_prev)
{
    if (c.go && (R.flags & RF_SELF_COL)) {                                       // UpdateCollisions :1729-1755
        // (lean sqrt / divide: bit-identical for the finite non-negative operands here, a third of the instructions -- this runs
        // on one thread while its workgroup waits)
        const double mv = vsqrt_nn(__longlong_as_double((long long)rs.maxvel2_bits));
        rs.max_disp += fabs(vdiv(mv * dt_prev, R.lat));
        rs.maxvel2_bits = 0ull;
        if (!(R.flags & RF_HORIZON_COL) || rs.max_disp > (R.col_horizon - 1.0) / 2) { c.rebuild = 1; rs.max_disp = 0.0; rs.rebuilds += 1; rs.col_tiled = 0; rs.reb_step = rs.steps; }
    }
    rs.rebuild_now = c.rebuild;
}
__device__ __forceinline__ StepCtl step_control(const DRobot& R, DRobotState& rs, long long step_cap, int begin_new_step)
{
    StepCtl c = step_control_begin(R, rs, step_cap, begin_new_step);
    step_control_horizon(R, rs, c, rs.dt_prev);
    return c;
}

// IniCM latch (= SS.CurCM of the previous step: mass-weighted SEQUENTIAL sum in voxel order, GetCM VX_Sim.cpp:2415-2430)
// and EndOfLifetimePosteriorY (getPosteriorY :2640-2656).  Whole workgroup; `sh` holds 5*CH doubles of LDS scratch.
template <class Pose>
__device__ __forceinline__ void latch_cm(const DBatch& B, const DRobot& R, DRobotState& rs, const Pose& pose, bool latch, bool eol, double* sh, int CH,
                                         int trace = 0, int trace_index = 0)      // (trace: StepCtl::trace, a mask)
{
    // The sums keep the reference's order (one thread adds voxel after voxel), but only the additions are serial: the products
    // x * m are formed by the staging threads (the same single rounding), and the y / lat of getPosteriorY is taken once, of the
    // smallest y (v -> v / lat is monotone for lat > 0, so the minimum of the rounded quotients is the rounded quotient of the minimum)
    const int tid = threadIdx.x, T = blockDim.x, base = R.vox_begin;
    double sx = 0, sy = 0, sz = 0, sm = 0, miny = 1.0e300;
    for (int c0 = 0; c0 < R.nvox; c0 += CH) {
        for (int k = tid; k < CH && c0 + k < R.nvox; k += T) {
            const int g = base + c0 + k;
            const DVoxClass& C = B.vclass_tab[R.vtab_begin + B.vclass[g]];
            double x, y, z, unused_scale;
            pose(g, x, y, z, unused_scale);
            sh[k] = __dmul_rn(x, C.mass); sh[CH + k] = __dmul_rn(y, C.mass); sh[2 * CH + k] = __dmul_rn(z, C.mass);
            sh[3 * CH + k] = C.mass;
            sh[4 * CH + k] = (C.mat == 5) ? 1.0e300 : y;        // material 5 is excluded from PosteriorY
        }
        __syncthreads();
        if (tid == 0) {
            const int n = min(CH, R.nvox - c0);
            for (int k = 0; k < n; ++k) {
                sx = __dadd_rn(sx, sh[k]); sy = __dadd_rn(sy, sh[CH + k]); sz = __dadd_rn(sz, sh[2 * CH + k]); sm += sh[3 * CH + k];
                miny = sh[4 * CH + k] < miny ? sh[4 * CH + k] : miny;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (latch) { const double inv = 1.0 / sm; rs.ini_cm[0] = inv * sx; rs.ini_cm[1] = inv * sy; rs.ini_cm[2] = inv * sz; rs.cm_init = 1; }
        if (eol) { const double q = miny / R.lat; rs.eol_post_y = q < 100000.0 ? q : 100000.0; }
        if (trace & (1 << VXH_TRACE_LIFE)) {   // SS.CMTraceTime / SS.CMTrace: (CurTime, GetCM()) of the step just finished
            const double inv = 1.0 / sm;
            double* e = B.trace + (size_t)(R.trace_begin + trace_index) * 4;
            e[0] = rs.cur_time; e[1] = inv * sx; e[2] = inv * sy; e[3] = inv * sz;
        }
    }
    // <NormDistByVol> (uniform: a flag of the robot): getTotalVolume() (VX_Sim.cpp:2574-2581) of the same poses, a second pass of the same
    // shape -- the staging threads form (scale / lat)^3, one thread adds them in voxel order.  The cube is x * x * x, each product rounded:
    // at most an ulp per voxel from the reference's pow(x, 3), eleven orders below the six digits the result file prints.
    if ((R.flags & RF_NORM_VOL) && trace) {
        double vol = 0;
        for (int c0 = 0; c0 < R.nvox; c0 += CH) {
            for (int k = tid; k < CH && c0 + k < R.nvox; k += T) {
                double x, y, z, scale;
                pose(base + c0 + k, x, y, z, scale);
                const double q = scale / R.lat;
                sh[k] = __dmul_rn(__dmul_rn(q, q), q);
            }
            __syncthreads();
            if (tid == 0) { const int n = min(CH, R.nvox - c0); for (int k = 0; k < n; ++k) vol = __dadd_rn(vol, sh[k]); }
            __syncthreads();
        }
        if (tid == 0) { const double inv = 1.0 / sm; store_norm_vol_points(B, R, rs, trace, trace_index, inv * sx, inv * sy, inv * sz, vol); }
    }
}

// stiffness of the collision bond between two voxel classes, first = the earlier voxel (CVX_Bond::LinkVoxels +
// UpdateConstants for the pair, VX_Bond.cpp:65-173: a1 = E*A/L of a cubic bond)
__device__ __forceinline__ double contact_a1(const DVoxClass& C1, const DVoxClass& C2)
{
    const double E = (C1.E * C2.E / (C1.E + C2.E)) * 2;
    const double L = (C1.nom_size + C2.nom_size) * 0.5;
    return E * (L * L) / L;
}

// CalcL1Bonds (VX_Sim.cpp:2357-2413).  The calling workgroup builds the partner rows of the surface voxels its
// threads own: every surface voxel tests all others (staged through LDS in chunks of
// CH) and keeps, in ascending partner order = creation order of its collision bonds in the reference, those that
// pass the distance filter, are more than `hops` bonds away and lie within CollisionHorizon scaled voxel sizes.
// `sh`: 4*CH doubles + CH ints of LDS.
// Thread `tid` owns surface ordinal i (`mine` = it has one).
template <class Pose>
__device__ __forceinline__ void rebuild_rows(const DBatch& B, const DRobot& R, DRobotState& rs, const Pose& pose, int i, bool mine, double* sh, int CH)
{
    const int tid = threadIdx.x, T = blockDim.x;
    int* shv = (int*)(sh + 4 * CH);
    int vi = 0, cnt = 0;
    const unsigned long long* row = B.excl + R.excl_begin + (long long)(mine ? i : 0) * R.excl_wpr;
    d3 pi = mk3(0, 0, 0); double si = 0;
    if (mine) {
        vi = B.surf[R.surf_begin + i];
        pose(vi, pi.x, pi.y, pi.z, si);
    }
    const double H = R.col_horizon;
    for (int c0 = 0; c0 < R.nsurf; c0 += CH) {
        const int n = min(CH, R.nsurf - c0);
        for (int k = tid; k < n; k += T) {
            const int vj = B.surf[R.surf_begin + c0 + k];
            pose(vj, sh[k], sh[CH + k], sh[2 * CH + k], sh[3 * CH + k]); shv[k] = vj;
        }
        __syncthreads();
        if (mine) {
            unsigned long long word = 0;
            for (int k = 0; k < n; ++k) {
                const int j = c0 + k;
                if ((j & 63) == 0) word = row[j >> 6];            // chunk starts are multiples of 64
                if (j == i) continue;
                const d3 d = pi - mk3(sh[k], sh[CH + k], sh[2 * CH + k]);
                const double d2 = len2(d);
                if (!(d2 < R.filter_dist2)) continue;
                if ((word >> (j & 63)) & 1ull) continue;          // !pV1->IsNearbyVox(SIndex2)
                const double s1 = (j > i) ? si : sh[3 * CH + k];   // scale of Vox1 = the earlier one, used twice (:2382)
                const double act = H * (s1 + s1) * 0.5;
                if (d2 < act * act) {
                    if (cnt < R.col_cap) {
                        const int vj = shv[k];
                        const DVoxClass& Ci = B.vclass_tab[R.vtab_begin + B.vclass[vi]];
                        const DVoxClass& Cj = B.vclass_tab[R.vtab_begin + B.vclass[vj]];
                        const size_t at = col_at(R, cnt, R.surf_begin + i);
                        B.col_partner[at] = vj;
                        B.col_a1[at] = (j > i) ? contact_a1(Ci, Cj) : contact_a1(Cj, Ci);
                    }
                    ++cnt;
                }
            }
        }
        __syncthreads();
    }
    if (mine) {
        if (cnt > R.col_cap) { cnt = R.col_cap; atomicOr(&rs.col_overflow, 1); }
        B.col_cnt[R.surf_begin + i] = cnt;
    }
}

}  // namespace vxh
