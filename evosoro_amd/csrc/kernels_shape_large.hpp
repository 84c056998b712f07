// k_shape_results_large: the RobotVolume and ConvexHullVolume tags of land_water robots of more than VXH_SHAPE_MAX_VERT mesh vertices
// (engine option device_shape_large), one workgroup per robot.  Same passes, same arithmetic and same fallback rule as k_shape_results
// (kernels_shape.hpp, whose rounding, plane, reduction, scan and compaction functions it shares); what differs is where the data lives
// and how the points reach the hull:
//   * the points -- as computed and rounded to six digits -- lie in the robot's range of a table in HBM (DShape::large_pts), written
//     by step (a) and read back by this workgroup alone (it stays in L2); the facet sums and the four sweeps that choose the first
//     tetrahedron are lane-strided reads of it, a new face fetches its two older vertices from it by id
//   * LDS holds the hull alone: the face records, one 16-bit cone-linking word per vertex, and a ring of two blocks of T points
//     (device_types.hpp shape_large_lds_bytes); the face capacity is what the CU has left, NOT 2 n + slack: a hull of more vertices
//     than half the capacity ends the pass with the fallback flag, the robot then takes the host path
//   * the points enter block by block.  Every lane takes one point of the block and walks the live faces (all lanes read the same
//     face: broadcast LDS reads) with the host's `nx px + ny py + nz pz - d > eps`; a point no face sees is dropped for good with no
//     barrier spent on it.  The survivors are inserted one after the other in ascending order, each tested again against the hull as
//     it then is, exactly as shape_hull does.  While a block is consumed, the loads of the next one are in flight.
// Why dropping is safe: the hull only grows, and a point inside or on a convex body is inside or on every larger one, so a point no
// face of an earlier hull sees is one the host, testing it later against a larger hull, does not insert either.  With the tolerance
// this holds for the distance to the BODY; the test measures the distance to the face PLANES, which for a point beyond an edge is the
// smaller of the two by the sine of the angle between the faces there.  The two tests can therefore disagree about a point that lies
// within eps = 1e-9 diag of every plane of the earlier hull and farther than eps from a plane of the later one: faces meeting at
// less than ~1e-8 rad, which the eps rule itself keeps from forming, or a distance equal to eps to the last bit.
#pragma once
#include "kernels_shape.hpp"

namespace vxh {

#pragma clang fp contract(off)      // to the end of this header, as kernels_shape.hpp

enum { SHAPE_LARGE_T = VXH_SHAPE_LARGE_THREADS, SHAPE_LARGE_NW = VXH_SHAPE_LARGE_THREADS / 64 };
typedef ShapeSharedN<SHAPE_LARGE_NW> ShapeLargeShared;

struct ShapeLargeLds {
    ShapeLds F;                   // the faces (LDS); F.raw / F.pt: the robot's planes [3][n] of the point table (HBM), F.np = n their stride
    double* ring;                 // [2][3][T] the points of the current block and of the next
    unsigned short* vstart;       // [n] the cone face that starts at this horizon vertex, SHAPE_NONE = none
    unsigned long long* cand;     // [wavefronts] the lanes whose point of the current block some face sees
};

// (a) mesh vertex gi of the batch (pass 0: the rest state, 1: the state in buffer cur) as mesh_vertices (results.cpp) places it, operation for
// operation; the same statements as step (a) of k_shape_results, which keeps them in its body so that its code stays what it was
__device__ __forceinline__ void shape_vertex(const DBatch& B, const DShape& Q, unsigned gi, double nom, int pass, int cur, double& x, double& y, double& z)
{
    const unsigned tm = B.total_mv, nv = B.nv;
    double ax = 0, ay = 0, az = 0, tw = 0;
    for (int q = 0; q < 8; ++q) {
        const int e = Q.vert[(unsigned)q * tm + gi];
        if (e < 0) break;
        const unsigned u = (unsigned)e >> 3;
        const int corner = e & 7;
        double st[6] = {0, 0, 0, 0, 0, 0};
        double px = Q.nom[u], py = Q.nom[nv + u], pz = Q.nom[2u * nv + u];
        double qw = 1, qx = 0, qy = 0, qz = 0;
        if (pass == 1) {
            for (int k = 0; k < 6; ++k) st[k] = B.strain[(unsigned)k * nv + u];
            px = B.vs[(unsigned)(4 * cur) * nv + u]; py = B.vs[(unsigned)(4 * cur + 1) * nv + u]; pz = B.vs[(unsigned)(4 * cur + 2) * nv + u];
            qw = B.vs[8u * nv + u]; qx = B.vs[9u * nv + u]; qy = B.vs[10u * nv + u]; qz = B.vs[11u * nv + u];
        }
        const double ox = (corner & 4) ? (1 + st[0]) * nom * 0.5 : -(1 + st[3]) * nom * 0.5;
        const double oy = (corner & 2) ? (1 + st[1]) * nom * 0.5 : -(1 + st[4]) * nom * 0.5;
        const double oz = (corner & 1) ? (1 + st[2]) * nom * 0.5 : -(1 + st[5]) * nom * 0.5;
        const double tw_ = ox * qx + oy * qy + oz * qz, tx = ox * qw - oy * qz + oz * qy, ty = ox * qz + oy * qw - oz * qx, tz = -ox * qy + oy * qx + oz * qw;
        ax += px + (qw * tx + qx * tw_ + qy * tz - qz * ty);
        ay += py + (qw * ty - qx * tz + qy * tw_ + qz * tx);
        az += pz + (qw * tz + qx * ty - qy * tx + qz * tw_);
        tw += 1.0;
    }
    const double inv = 1.0 / tw;
    const double v0x = B.vert_v0[gi], v0y = B.vert_v0[tm + gi], v0z = B.vert_v0[2u * tm + gi];
    x = v0x + (ax * inv - v0x); y = v0y + (ay * inv - v0y); z = v0z + (az * inv - v0z);
}

// One point into the hull: steps 1 to 6 of shape_hull's point loop.  false: the pass ends here (fallback).  The cone-linking word is a
// plain 16-bit store: when two horizon edges leave one vertex, one cone face of the h is nobody's successor, and the last loop finds it.
__device__ inline bool shape_large_insert(const ShapeLargeLds& L, int p, double px, double py, double pz, double eps, int& nf, int& it, ShapeLargeShared& S, int tid)
{
    const ShapeLds& F = L.F;
    const int fc = F.fc;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const int w = it % 3;
        ++it;
        bool any = false;
        for (int f = tid; f < nf; f += SHAPE_LARGE_T) {
            const bool vis = F.fv[f] != SHAPE_NONE && F.plane[f] * px + F.plane[fc + f] * py + F.plane[2 * fc + f] * pz - F.plane[3 * fc + f] > eps;
            F.mark[f] = vis ? 1 : 0;
            any = any || vis;
        }
        if (__ballot(any) != 0 && (tid & 63) == 0) S.any[w] = 1;
        if (tid == 0) S.any[(w + 1) % 3] = 0;
        __syncthreads();
        if (S.bad) return false;
        if (!S.any[w]) return true;                            // (the hull grew over it since the block was culled)
        int cnt = 0;
        for (int f = tid; f < nf; f += SHAPE_LARGE_T)
            if (F.mark[f]) for (int k = 0; k < 3; ++k) cnt += F.mark[F.fn[k * fc + f]] ? 0 : 1;
        int h;
        const int off = shape_block_scan(cnt, h, S, tid);
        if (h < 3) return false;
        if (nf + h > fc) {
            if (attempt == 1) return false;                    // more live faces than the capacity
            nf = shape_compact(F, nf, S, tid);
            continue;
        }
        int s = nf + off;
        for (int f = tid; f < nf; f += SHAPE_LARGE_T) {
            if (!F.mark[f]) continue;
            for (int k = 0; k < 3; ++k) {
                const int g = F.fn[k * fc + f];
                if (F.mark[g]) continue;
                const int a = F.fv[k * fc + f], b = F.fv[(k + 1) % 3 * fc + f];
                shape_put_face(F, s, a, b, p, g, SHAPE_NONE, SHAPE_NONE);      // (a and b: per-lane loads from the table)
                for (int j = 0; j < 3; ++j) if (F.fv[j * fc + g] == b) F.fn[j * fc + g] = (unsigned short)s;
                L.vstart[a] = (unsigned short)s;
                ++s;
            }
            F.fv[f] = SHAPE_NONE;
        }
        __syncthreads();
        for (int q = nf + off; q < nf + off + cnt; ++q) {
            const unsigned short nx = L.vstart[F.fv[fc + q]];
            if (nx == SHAPE_NONE) S.bad = 1;
            else { F.fn[fc + q] = nx; F.fn[2 * fc + nx] = (unsigned short)q; }
        }
        __syncthreads();
        for (int q = nf + off; q < nf + off + cnt; ++q) {
            if (F.fn[2 * fc + q] == SHAPE_NONE) S.bad = 1;     // nobody ends at its first vertex: the horizon is no simple closed loop
            L.vstart[F.fv[q]] = SHAPE_NONE;
        }
        nf += h;
        return true;
    }
    return true;
}

// (d) as shape_hull: the same tetrahedron, eps and visibility test, the points in the same order.  ok = false: no answer (fewer than
// four points, degenerate input, a full face list after compaction, a horizon that does not close).  Every loop is bounded by n or fc.
__device__ inline double shape_large_hull(const ShapeLargeLds& L, int n, ShapeLargeShared& S, int tid, bool& ok)
{
    constexpr int T = SHAPE_LARGE_T;
    const ShapeLds& F = L.F;
    const double *X = F.pt, *Y = F.pt + n, *Z = F.pt + 2 * n;
    const int fc = F.fc;
    ok = false;
    if (n < 4) return 0.0;
    double ext[6];                                             // -lo xyz, hi xyz
    {
        double m[6] = {-1e300, -1e300, -1e300, -1e300, -1e300, -1e300};
        for (int i = tid; i < n; i += T) {
            const double p[3] = {X[i], Y[i], Z[i]};
            for (int k = 0; k < 3; ++k) { m[k] = -p[k] > m[k] ? -p[k] : m[k]; m[3 + k] = p[k] > m[3 + k] ? p[k] : m[3 + k]; }
        }
        for (int k = 0; k < 6; ++k) ext[k] = shape_block_max(m[k], S, tid);
    }
    const double ex = ext[3] - -ext[0], ey = ext[4] - -ext[1], ez = ext[5] - -ext[2];
    const double diag = sqrt(ex * ex + ey * ey + ez * ez);
    if (!(diag > 0) || !(diag < 1e300)) return 0.0;
    const double eps = 1e-9 * diag;
    int i0 = 0, i1 = 0;
    for (int axis = 0; axis < 3 && i0 == i1; ++axis) {
        const double* C = F.pt + axis * n;
        ShapeBest lo, hi; lo.i = hi.i = -1; lo.v = hi.v = 0;
        for (int i = tid; i < n; i += T) {
            ShapeBest c; c.i = i;
            const double v = C[i];
            c.v = -v; lo = shape_better(lo, c);
            c.v = v; hi = shape_better(hi, c);
        }
        i0 = shape_block_best(lo, S, tid).i; i1 = shape_block_best(hi, S, tid).i;
    }
    if (i0 == i1 || i0 < 0 || i1 < 0) return 0.0;
    int i2, i3;
    {
        const double x0 = X[i0], y0 = Y[i0], z0 = Z[i0];
        const double lx = X[i1] - x0, ly = Y[i1] - y0, lz = Z[i1] - z0;
        ShapeBest b; b.i = -1; b.v = 0;
        for (int i = tid; i < n; i += T) {
            const double px = X[i] - x0, py = Y[i] - y0, pz = Z[i] - z0;
            const double cx = ly * pz - lz * py, cy = lz * px - lx * pz, cz = lx * py - ly * px;
            ShapeBest c; c.i = i; c.v = cx * cx + cy * cy + cz * cz;
            if (c.v > 0) b = shape_better(b, c);
        }
        b = shape_block_best(b, S, tid);
        i2 = b.i;
        if (i2 < 0 || !(sqrt(b.v) > eps * diag)) return 0.0;
    }
    {
        double nx, ny, nz, d;
        shape_plane(X, Y, Z, i0, i1, i2, nx, ny, nz, d);
        ShapeBest b; b.i = -1; b.v = 0;
        for (int i = tid; i < n; i += T) {
            ShapeBest c; c.i = i; c.v = fabs(nx * X[i] + ny * Y[i] + nz * Z[i] - d);
            if (c.v > 0) b = shape_better(b, c);
        }
        b = shape_block_best(b, S, tid);
        i3 = b.i;
        if (i3 < 0 || !(b.v > eps)) return 0.0;                // all points in one plane
        if (nx * X[i3] + ny * Y[i3] + nz * Z[i3] - d > 0) { const int t = i1; i1 = i2; i2 = t; }
    }
    if (tid == 0) {
        shape_put_face(F, 0, i0, i1, i2, 1, 2, 3);
        shape_put_face(F, 1, i0, i3, i1, 3, 2, 0);
        shape_put_face(F, 2, i1, i3, i2, 1, 3, 0);
        shape_put_face(F, 3, i2, i3, i0, 2, 1, 0);
        S.any[0] = S.any[1] = S.any[2] = 0; S.bad = 0;
    }
    for (int i = tid; i < n; i += T) L.vstart[i] = SHAPE_NONE;
    {                                                          // block 0 into slot 0 of the ring
        double x = 0, y = 0, z = 0;
        if (tid < n) { x = X[tid]; y = Y[tid]; z = Z[tid]; }
        L.ring[tid] = x; L.ring[T + tid] = y; L.ring[2 * T + tid] = z;
    }
    __syncthreads();
    int nf = 4, it = 0;
    for (int b0 = 0, slot = 0; b0 < n; b0 += T, slot ^= 1) {
        const double* R = L.ring + slot * 3 * T;
        double* Rn = L.ring + (slot ^ 1) * 3 * T;
        const int q = b0 + tid;
        const double px = R[tid], py = R[T + tid], pz = R[2 * T + tid];
        double x = 0, y = 0, z = 0;                            // the next block: its loads are in flight while this one is consumed
        if (q + T < n) { x = X[q + T]; y = Y[q + T]; z = Z[q + T]; }
        // pre-cull: my point against every live face
        const bool mine = q < n && q != i0 && q != i1 && q != i2 && q != i3;
        bool seen = false;
        for (int f = 0; f < nf; ++f) {
            if (__all(seen || !mine)) break;
            const bool vis = F.fv[f] != SHAPE_NONE && F.plane[f] * px + F.plane[fc + f] * py + F.plane[2 * fc + f] * pz - F.plane[3 * fc + f] > eps;
            seen = seen || vis;
        }
        const unsigned long long mask = __ballot(seen && mine);
        if ((tid & 63) == 0) L.cand[tid >> 6] = mask;
        __syncthreads();
        // the survivors, in ascending order (the mask is the same in every lane: made uniform for the compiler)
        for (int w = 0; w < SHAPE_LARGE_NW; ++w) {
            const unsigned long long c = L.cand[w];
            unsigned long long m = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(c >> 32)) << 32 | (unsigned)__builtin_amdgcn_readfirstlane((int)c);
            while (m) {
                const int k = w * 64 + __builtin_ctzll(m);
                m &= m - 1;
                if (!shape_large_insert(L, b0 + k, R[k], R[T + k], R[2 * T + k], eps, nf, it, S, tid)) return 0.0;
            }
        }
        Rn[tid] = x; Rn[T + tid] = y; Rn[2 * T + tid] = z;
        __syncthreads();                                       // (also: the last insertion's links are done, the masks are free)
    }
    if (S.bad) return 0.0;
    // signed tetrahedra against an interior point
    const double cx = 0.25 * (X[i0] + X[i1] + X[i2] + X[i3]), cy = 0.25 * (Y[i0] + Y[i1] + Y[i2] + Y[i3]), cz = 0.25 * (Z[i0] + Z[i1] + Z[i2] + Z[i3]);
    double volume = 0;
    for (int f = tid; f < nf; f += T) {
        if (F.fv[f] == SHAPE_NONE) continue;
        const int ia = F.fv[f], ib = F.fv[fc + f], ic = F.fv[2 * fc + f];
        const double a[3] = {X[ia] - cx, Y[ia] - cy, Z[ia] - cz}, b[3] = {X[ib] - cx, Y[ib] - cy, Z[ib] - cz}, c[3] = {X[ic] - cx, Y[ic] - cy, Z[ic] - cz};
        volume += (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0])) / 6.0;
    }
    volume = shape_block_sum(volume, S, tid);
    ok = true;
    return fabs(volume);
}

static __global__ __launch_bounds__(VXH_SHAPE_LARGE_THREADS) void k_shape_results_large(DBatch B, DShape Q)
{
    constexpr int T = SHAPE_LARGE_T;
    extern __shared__ double shape_large_lds[];
    __shared__ ShapeLargeShared S;
    __shared__ unsigned long long cand[SHAPE_LARGE_NW];
    const int r = Q.large_list[blockIdx.x], tid = threadIdx.x;
    const DRobot& R = B.robot[r];
    const int n = R.nmv, steps = B.rstate[r].steps;
    double* const tab = Q.large_pts + Q.large_off[blockIdx.x];
    ShapeLargeLds L;
    L.F.np = n; L.F.fc = shape_large_face_cap(n);
    L.F.raw = tab; L.F.pt = tab + 3 * (size_t)n; L.F.vstart = nullptr;
    L.ring = shape_large_lds; L.F.plane = L.ring + 6 * T;
    L.F.fv = (unsigned short*)(L.F.plane + 4 * L.F.fc); L.F.fn = L.F.fv + 3 * L.F.fc; L.F.mark = L.F.fn + 3 * L.F.fc;
    L.vstart = L.F.mark + L.F.fc; L.cand = cand;
    const unsigned tf = B.total_facet;
    const double nom = R.lat;
    const double *RX = tab, *RY = tab + n, *RZ = tab + 2 * (size_t)n;
    DShapeResult o;
    o.fallback = 0; o.pad = 0;
    o.robot_volume[1] = o.hull_volume[1] = 0;
    for (int pass = 0; pass < 2 && !o.fallback; ++pass) {
        if (pass == 1 && steps == 0) { o.robot_volume[1] = o.robot_volume[0]; o.hull_volume[1] = o.hull_volume[0]; break; }      // (as compute_result)
        // a. + c. the vertices, as computed and rounded, into the robot's range of the table
        for (int i = tid; i < n; i += T) {
            double x, y, z;
            shape_vertex(B, Q, R.vert_begin + i, nom, pass, steps & 1, x, y, z);
            tab[i] = x; tab[n + i] = y; tab[2 * (size_t)n + i] = z;
            L.F.pt[i] = shape_round6(x); L.F.pt[n + i] = shape_round6(y); L.F.pt[2 * (size_t)n + i] = shape_round6(z);
        }
        __syncthreads();                                       // (the table is this workgroup's own: its stores are visible to it behind the barrier)
        // b. robot_volume: lane t adds the facets t, t + T, ... in that order, then the fixed-shape reduction
        double vol = 0.0;
        for (int f = tid; f < R.nfacet; f += T) {
            const unsigned gf = R.facet_begin + f;
            const int ia = B.facet_vert[gf], ib = B.facet_vert[tf + gf], ic = B.facet_vert[2u * tf + gf];
            const double a[3] = {RX[ia], RY[ia], RZ[ia]}, b[3] = {RX[ib], RY[ib], RZ[ib]}, c[3] = {RX[ic], RY[ic], RZ[ic]};
            const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
            vol += (1.0 / 6.0) * (cx * c[0] + cy * c[1] + cz * c[2]);
        }
        o.robot_volume[pass] = shape_block_sum(vol, S, tid);
        bool ok;
        o.hull_volume[pass] = shape_large_hull(L, n, S, tid, ok);
        if (!ok) o.fallback = 1;
        __syncthreads();                                       // (the next pass overwrites the table)
    }
    if (tid == 0) Q.out[r] = o;
}

}  // namespace vxh
