// k_shape_results: the RobotVolume and ConvexHullVolume tags of land_water robots on the device (engine option device_shape), one workgroup of
// four wavefronts per robot.  The host routines it stands in for are robot_volume, mesh_vertices, robot_hull_volume and
// convex_hull_volume (results.cpp); the kernel keeps their arithmetic -- every product, sum, quotient and square root rounded on its
// own, in the host's order -- so that it places the same vertices and builds the same hull faces, and differs from the host only in the
// order of the two final sums.  Launched by launch_shape.hip.
//
// Per robot two passes, the rest state and the final state, each:
//   a. one lane per mesh vertex: the mean of the <= 7 voxel corners meeting there -> LDS planes raw[3][np]
//   b. one lane per facet: signed tetrahedra against the origin, summed in an order that depends on the robot alone
//   c. every coordinate rounded to six significant digits (the reference prints them for qhull) -> LDS planes pt[3][np]
//   d. incremental convex hull of pt, points in the host's order, every loop over faces spread across the workgroup
// LDS (device_types.hpp shape_lds_bytes): raw | pt | face planes [4][fc] | face vertices [3][fc] | face neighbours [3][fc] | face marks [fc];
// during (d) the raw planes are dead and their first words hold the per-vertex scratch of the cone linking.
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.hpp"

namespace vxh {

#pragma clang fp contract(off)      // to the end of this header: the host's roundings (results.cpp is compiled without contraction)

enum : unsigned short { SHAPE_NONE = 0xFFFFu };      // a dead face (in its first vertex) / a neighbour not linked yet

template <int NW>                 // NW wavefronts: k_shape_results has four, k_shape_results_large (kernels_shape_large.hpp) its own count
struct ShapeSharedN {             // static LDS of the workgroup
    double red[NW];
    double best_v[NW];
    int best_i[NW];
    int scan[NW];
    int any[3];                   // "some lane sees a face" of the current point, rotating (one barrier per point)
    int bad;                      // the pass cannot go on: capacity, a horizon that does not close
};
typedef ShapeSharedN<VXH_SHAPE_THREADS / 64> ShapeShared;

struct ShapeLds {
    double *raw, *pt, *plane;
    unsigned short *fv, *fn, *mark;
    int* vstart;                  // [n] (aliases raw) the cone face that starts at this horizon vertex, -1 = none
    int np, fc;
};

// fixed-shape reductions over the workgroup: butterfly inside a wavefront (every lane ends with the same bits: the operands of each
// level commute), then the wavefronts as a fixed pairwise tree -- four of them: (0 + 1) + (2 + 3)
template <int NW>
__device__ __forceinline__ double shape_block_sum(double v, ShapeSharedN<NW>& S, int tid)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
    if ((tid & 63) == 0) S.red[tid >> 6] = v;
    __syncthreads();
    double t[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) t[w] = S.red[w];
#pragma unroll
    for (int s = 1; s < NW; s <<= 1)
#pragma unroll
        for (int w = 0; w < NW; w += 2 * s) t[w] = t[w] + t[w + s];
    __syncthreads();
    return t[0];
}

template <int NW>
__device__ __forceinline__ double shape_block_max(double v, ShapeSharedN<NW>& S, int tid)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_xor(v, off); v = o > v ? o : v; }
    if ((tid & 63) == 0) S.red[tid >> 6] = v;
    __syncthreads();
    double t = S.red[0];
    for (int w = 1; w < NW; ++w) t = S.red[w] > t ? S.red[w] : t;
    __syncthreads();
    return t;
}

// the host's `if (value(i) > best) { best = value(i); i_best = i; }` over ascending i: the largest value, of equal ones the lowest index
struct ShapeBest { double v; int i; };      // i < 0: none
__device__ __forceinline__ ShapeBest shape_better(ShapeBest a, ShapeBest b)
{
    if (b.i < 0) return a;
    if (a.i < 0) return b;
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
template <int NW>
__device__ __forceinline__ ShapeBest shape_block_best(ShapeBest b, ShapeSharedN<NW>& S, int tid)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { ShapeBest o; o.v = __shfl_xor(b.v, off); o.i = __shfl_xor(b.i, off); b = shape_better(b, o); }
    if ((tid & 63) == 0) { S.best_v[tid >> 6] = b.v; S.best_i[tid >> 6] = b.i; }
    __syncthreads();
    ShapeBest t; t.v = S.best_v[0]; t.i = S.best_i[0];
    for (int w = 1; w < NW; ++w) { ShapeBest o; o.v = S.best_v[w]; o.i = S.best_i[w]; t = shape_better(t, o); }
    __syncthreads();
    return t;
}

// exclusive prefix sum of one int per thread, in thread order; total: the sum
template <int NW>
__device__ __forceinline__ int shape_block_scan(int c, int& total, ShapeSharedN<NW>& S, int tid)
{
    const int lane = tid & 63, w = tid >> 6;
    int inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
    if (lane == 63) S.scan[w] = inc;
    __syncthreads();
    int base = 0;
    for (int k = 0; k < w; ++k) base += S.scan[k];
    total = S.scan[0];
    for (int k = 1; k < NW; ++k) total += S.scan[k];
    __syncthreads();
    return base + inc - c;
}

// (c) x as `printf("%g")` / `atof` return it: six significant decimal digits.  Decade by comparison with a table of exact powers of ten,
// scale into [1e5, 1e6), rint, unscale.  The scaling is a rounded product, which alone would misplace values within an ulp of a tie
// xxxxxx.5; its error term (fma) says on which side of the tie the exact product lies, an exact tie goes to even as glibc prints it, and
// the quotient n / 10^k of two exact doubles is the double nearest to the decimal, which is what atof returns.  So for
// 1e-15 <= |x| < 1e21 the result IS the printf round trip.  Below 1e-15 -- round-off left around a zero coordinate, thirteen orders
// under the lattice constant -- the value is first multiplied by 1e22 and the result divided by it again, both rounded: there, and only
// there, the result can differ from the round trip, in its last bit or, next to a tie, by one unit of the sixth digit (of a number
// that small).  Zero, NaN, infinities and |x| >= 1e21 pass through.  (Checked on the host against snprintf / atof: 14 million values,
// ties and their neighbours included.)
__device__ inline double shape_round6(double x)
{
    const double p10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    double a = fabs(x);
    if (!(a > 0.0) || !(a < 1e21)) return x;
    int sh = 0;
    while (a < 1e-15 && sh < 16) { a = a * 1e22; ++sh; }
    int k;                                                     // the power of ten that brings a into [1e5, 1e6)
    if (a >= 1.0) { int e = 0; while (e < 21 && a >= p10[e + 1]) ++e; k = 5 - e; }
    else { int m = 1; while (m < 16 && a * p10[m] < 1.0) ++m; k = 5 + m; }
    double hi = 0, lo = 0;
    for (int pass = 0; pass < 3; ++pass) {                     // (the comparison above may be off by a decade at a power of ten)
        if (k >= 0) { hi = a * p10[k]; lo = fma(a, p10[k], -hi); }
        else { hi = a / p10[-k]; lo = fma(-hi, p10[-k], a); }  // (the sign of the remainder)
        if (pass == 2) break;
        if (hi < 1e5 && k < 22) ++k; else if (hi >= 1e6 && k > -16) --k; else break;
    }
    double n = rint(hi);
    if (fabs(hi - n) == 0.5 && lo != 0.0) n = lo > 0.0 ? hi + 0.5 : hi - 0.5;
    double r = k >= 0 ? n / p10[k] : n * p10[-k];
    for (; sh > 0; --sh) r = r / 1e22;
    return x < 0.0 ? -r : r;
}

// the plane of face (a, b, c) as convex_hull_volume's `make` computes it
__device__ __forceinline__ void shape_plane(const double* X, const double* Y, const double* Z, int a, int b, int c, double& nx, double& ny, double& nz, double& d)
{
    const double ux = X[b] - X[a], uy = Y[b] - Y[a], uz = Z[b] - Z[a], vx = X[c] - X[a], vy = Y[c] - Y[a], vz = Z[c] - Z[a];
    nx = uy * vz - uz * vy; ny = uz * vx - ux * vz; nz = ux * vy - uy * vx;
    const double l = sqrt(nx * nx + ny * ny + nz * nz);
    if (l > 0) { nx /= l; ny /= l; nz /= l; }
    d = nx * X[a] + ny * Y[a] + nz * Z[a];
}

__device__ __forceinline__ void shape_put_face(const ShapeLds& L, int s, int a, int b, int c, int n0, int n1, int n2)
{
    const double *X = L.pt, *Y = L.pt + L.np, *Z = L.pt + 2 * L.np;
    double nx, ny, nz, d;
    shape_plane(X, Y, Z, a, b, c, nx, ny, nz, d);
    L.plane[s] = nx; L.plane[L.fc + s] = ny; L.plane[2 * L.fc + s] = nz; L.plane[3 * L.fc + s] = d;
    L.fv[s] = (unsigned short)a; L.fv[L.fc + s] = (unsigned short)b; L.fv[2 * L.fc + s] = (unsigned short)c;
    L.fn[s] = (unsigned short)n0; L.fn[L.fc + s] = (unsigned short)n1; L.fn[2 * L.fc + s] = (unsigned short)n2;
}

// Dead faces out of the list, in place, order kept; returns the new length.  The new index of every live face goes into its mark, then
// the list moves tile by tile (one face per thread: read, barrier, write -- a face only ever moves down, into slots whose faces have been read).
template <int NW>
__device__ inline int shape_compact(const ShapeLds& L, int nf, ShapeSharedN<NW>& S, int tid)
{
    int live = 0;
    for (int t0 = 0; t0 < nf; t0 += 64 * NW) {
        const int f = t0 + tid;
        const int alive = (f < nf && L.fv[f] != SHAPE_NONE) ? 1 : 0;
        int total;
        const int ex = shape_block_scan(alive, total, S, tid);
        if (alive) L.mark[f] = (unsigned short)(live + ex);
        live += total;
    }
    __syncthreads();
    for (int t0 = 0; t0 < nf; t0 += 64 * NW) {
        const int f = t0 + tid;
        const bool alive = f < nf && L.fv[f] != SHAPE_NONE;
        double pl[4] = {0, 0, 0, 0};
        unsigned short v[3] = {0, 0, 0}, nb[3] = {0, 0, 0};
        int to = 0;
        if (alive) {
            to = L.mark[f];
            for (int k = 0; k < 4; ++k) pl[k] = L.plane[k * L.fc + f];
            for (int k = 0; k < 3; ++k) { v[k] = L.fv[k * L.fc + f]; nb[k] = L.mark[L.fn[k * L.fc + f]]; }
        }
        __syncthreads();
        if (alive) {
            for (int k = 0; k < 4; ++k) L.plane[k * L.fc + to] = pl[k];
            for (int k = 0; k < 3; ++k) { L.fv[k * L.fc + to] = v[k]; L.fn[k * L.fc + to] = nb[k]; }
        }
    }
    __syncthreads();
    return live;
}

// (d) volume of the convex hull of pt[0 .. n): convex_hull_volume (results.cpp) with the face loops spread over the workgroup.  The same
// initial tetrahedron, eps = 1e-9 diag and `dist > eps` visibility, the points in the same order: the same faces.  ok = false: the
// pass ended without an answer (fewer than four points, degenerate input, more faces than the capacity, a horizon that is no closed
// loop); the robot then takes the host path.  Every loop is bounded by n or by the face capacity.
__device__ inline double shape_hull(const ShapeLds& L, int n, ShapeShared& S, int tid, bool& ok)
{
    const double *X = L.pt, *Y = L.pt + L.np, *Z = L.pt + 2 * L.np;
    const int fc = L.fc;
    ok = false;
    if (n < 4) return 0.0;
    double ext[6];                                             // -lo xyz, hi xyz
    {
        double m[6] = {-1e300, -1e300, -1e300, -1e300, -1e300, -1e300};
        for (int i = tid; i < n; i += VXH_SHAPE_THREADS) {
            const double p[3] = {X[i], Y[i], Z[i]};
            for (int k = 0; k < 3; ++k) { m[k] = -p[k] > m[k] ? -p[k] : m[k]; m[3 + k] = p[k] > m[3 + k] ? p[k] : m[3 + k]; }
        }
        for (int k = 0; k < 6; ++k) ext[k] = shape_block_max(m[k], S, tid);
    }
    const double ex = ext[3] - -ext[0], ey = ext[4] - -ext[1], ez = ext[5] - -ext[2];
    const double diag = sqrt(ex * ex + ey * ey + ez * ez);
    if (!(diag > 0) || !(diag < 1e300)) return 0.0;
    const double eps = 1e-9 * diag;
    // initial tetrahedron: extreme points along x (y, z when all x are equal), farthest from their line, farthest from that plane
    int i0 = 0, i1 = 0;
    for (int axis = 0; axis < 3 && i0 == i1; ++axis) {
        const double* C = L.pt + axis * L.np;
        ShapeBest lo, hi; lo.i = hi.i = -1; lo.v = hi.v = 0;
        for (int i = tid; i < n; i += VXH_SHAPE_THREADS) {
            ShapeBest c; c.i = i;
            c.v = -C[i]; lo = shape_better(lo, c);
            c.v = C[i]; hi = shape_better(hi, c);
        }
        i0 = shape_block_best(lo, S, tid).i; i1 = shape_block_best(hi, S, tid).i;
    }
    if (i0 == i1 || i0 < 0 || i1 < 0) return 0.0;
    int i2, i3;
    {
        const double lx = X[i1] - X[i0], ly = Y[i1] - Y[i0], lz = Z[i1] - Z[i0];
        ShapeBest b; b.i = -1; b.v = 0;
        for (int i = tid; i < n; i += VXH_SHAPE_THREADS) {
            const double px = X[i] - X[i0], py = Y[i] - Y[i0], pz = Z[i] - Z[i0];
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
        for (int i = tid; i < n; i += VXH_SHAPE_THREADS) {
            ShapeBest c; c.i = i; c.v = fabs(nx * X[i] + ny * Y[i] + nz * Z[i] - d);
            if (c.v > 0) b = shape_better(b, c);
        }
        b = shape_block_best(b, S, tid);
        i3 = b.i;
        if (i3 < 0 || !(b.v > eps)) return 0.0;                // all points in one plane
        if (nx * X[i3] + ny * Y[i3] + nz * Z[i3] - d > 0) { const int t = i1; i1 = i2; i2 = t; }      // orient (i0, i1, i2) away from i3
    }
    if (tid == 0) {
        shape_put_face(L, 0, i0, i1, i2, 1, 2, 3);             // neighbours across the edges (v0 v1), (v1 v2), (v2 v0)
        shape_put_face(L, 1, i0, i3, i1, 3, 2, 0);
        shape_put_face(L, 2, i1, i3, i2, 1, 3, 0);
        shape_put_face(L, 3, i2, i3, i0, 2, 1, 0);
        S.any[0] = S.any[1] = S.any[2] = 0; S.bad = 0;
    }
    for (int i = tid; i < n; i += VXH_SHAPE_THREADS) L.vstart[i] = -1;
    __syncthreads();
    int nf = 4, it = 0;
    for (int p = 0; p < n; ++p) {
        if (p == i0 || p == i1 || p == i2 || p == i3) continue;
        const double px = X[p], py = Y[p], pz = Z[p];
        bool placed = false;
        for (int attempt = 0; attempt < 2 && !placed; ++attempt) {
            // 1. every lane tests its faces; 2. one ballot per wavefront and one LDS word: seen by nobody -> next point.  The word
            // rotates through three: the one of the next round is cleared in this one, behind the barrier that ended its last use
            const int w = it % 3;
            ++it;
            bool any = false;
            for (int f = tid; f < nf; f += VXH_SHAPE_THREADS) {
                const bool vis = L.fv[f] != SHAPE_NONE && L.plane[f] * px + L.plane[fc + f] * py + L.plane[2 * fc + f] * pz - L.plane[3 * fc + f] > eps;
                L.mark[f] = vis ? 1 : 0;
                any = any || vis;
            }
            if (__ballot(any) != 0 && (tid & 63) == 0) S.any[w] = 1;
            if (tid == 0) S.any[(w + 1) % 3] = 0;
            __syncthreads();
            if (S.bad) return 0.0;
            if (!S.any[w]) { placed = true; break; }
            // 3. horizon: the edges of visible faces whose neighbour is not visible; 4. a prefix sum gives every cone face its slot
            int cnt = 0;
            for (int f = tid; f < nf; f += VXH_SHAPE_THREADS)
                if (L.mark[f]) for (int k = 0; k < 3; ++k) cnt += L.mark[L.fn[k * fc + f]] ? 0 : 1;
            int h;
            const int off = shape_block_scan(cnt, h, S, tid);
            if (h < 3) return 0.0;                             // (every face visible: no hull left)
            if (nf + h > fc) {                                 // 6. the list is full: dead faces out, and this point once more
                if (attempt == 1) return 0.0;                  // more live faces than the capacity
                nf = shape_compact(L, nf, S, tid);
                continue;
            }
            int s = nf + off;
            for (int f = tid; f < nf; f += VXH_SHAPE_THREADS) {
                if (!L.mark[f]) continue;
                for (int k = 0; k < 3; ++k) {
                    const int g = L.fn[k * fc + f];
                    if (L.mark[g]) continue;
                    const int a = L.fv[k * fc + f], b = L.fv[(k + 1) % 3 * fc + f];
                    shape_put_face(L, s, a, b, p, g, SHAPE_NONE, SHAPE_NONE);
                    for (int j = 0; j < 3; ++j) if (L.fv[j * fc + g] == b) L.fn[j * fc + g] = (unsigned short)s;      // g's edge (b a) now borders the cone
                    if (atomicExch(&L.vstart[a], s) != -1) S.bad = 1;      // two horizon edges leave one vertex: not a simple loop
                    ++s;
                }
                L.fv[f] = SHAPE_NONE;
            }
            __syncthreads();
            // 5. cone face (a, b, p): across (b p) lies the cone face that starts at b, and that one has this one across its (p b')
            for (int q = nf + off; q < nf + off + cnt; ++q) {
                const int nx = L.vstart[L.fv[fc + q]];
                if (nx < 0) S.bad = 1;
                else { L.fn[fc + q] = (unsigned short)nx; L.fn[2 * fc + nx] = (unsigned short)q; }
            }
            __syncthreads();
            for (int q = nf + off; q < nf + off + cnt; ++q) {
                if (L.fn[2 * fc + q] == SHAPE_NONE) S.bad = 1;  // nobody ends at its first vertex: the horizon does not close
                L.vstart[L.fv[q]] = -1;
            }
            nf += h;
            placed = true;
        }
    }
    __syncthreads();
    if (S.bad) return 0.0;
    // signed tetrahedra against an interior point
    const double cx = 0.25 * (X[i0] + X[i1] + X[i2] + X[i3]), cy = 0.25 * (Y[i0] + Y[i1] + Y[i2] + Y[i3]), cz = 0.25 * (Z[i0] + Z[i1] + Z[i2] + Z[i3]);
    double volume = 0;
    for (int f = tid; f < nf; f += VXH_SHAPE_THREADS) {
        if (L.fv[f] == SHAPE_NONE) continue;
        const int ia = L.fv[f], ib = L.fv[fc + f], ic = L.fv[2 * fc + f];
        const double a[3] = {X[ia] - cx, Y[ia] - cy, Z[ia] - cz}, b[3] = {X[ib] - cx, Y[ib] - cy, Z[ib] - cz}, c[3] = {X[ic] - cx, Y[ic] - cy, Z[ic] - cz};
        volume += (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0])) / 6.0;
    }
    volume = shape_block_sum(volume, S, tid);
    ok = true;
    return fabs(volume);
}

static __global__ __launch_bounds__(VXH_SHAPE_THREADS) void k_shape_results(DBatch B, DShape Q)
{
    extern __shared__ double shape_lds[];
    __shared__ ShapeShared S;
    const int r = Q.list[blockIdx.x], tid = threadIdx.x;
    const DRobot& R = B.robot[r];
    const int n = R.nmv, steps = B.rstate[r].steps;
    ShapeLds L;
    L.np = (n + 1) & ~1; L.fc = shape_face_cap(n);
    L.raw = shape_lds; L.pt = L.raw + 3 * L.np; L.plane = L.pt + 3 * L.np;
    L.fv = (unsigned short*)(L.plane + 4 * L.fc); L.fn = L.fv + 3 * L.fc; L.mark = L.fn + 3 * L.fc;
    L.vstart = (int*)L.raw;
    const unsigned tm = B.total_mv, tf = B.total_facet, nv = B.nv;
    const double nom = R.lat;
    DShapeResult o;
    o.fallback = 0; o.pad = 0;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && steps == 0) { o.robot_volume[1] = o.robot_volume[0]; o.hull_volume[1] = o.hull_volume[0]; break; }      // (as compute_result)
        const int cur = steps & 1;
        // a. the vertices as mesh_vertices (results.cpp) places them, operation for operation: corner offset from the strains,
        //    CQuat::RotateVec3D, the voxels in the host's order, v0 + (mean - v0)
        for (int i = tid; i < n; i += VXH_SHAPE_THREADS) {
            const unsigned gi = R.vert_begin + i;
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
            const double x = v0x + (ax * inv - v0x), y = v0y + (ay * inv - v0y), z = v0z + (az * inv - v0z);
            L.raw[i] = x; L.raw[L.np + i] = y; L.raw[2 * L.np + i] = z;
            L.pt[i] = shape_round6(x); L.pt[L.np + i] = shape_round6(y); L.pt[2 * L.np + i] = shape_round6(z);      // c.
        }
        __syncthreads();
        // b. robot_volume: lane t adds the facets t, t + 256, ... in that order, then the fixed-shape reduction
        double vol = 0.0;
        for (int f = tid; f < R.nfacet; f += VXH_SHAPE_THREADS) {
            const unsigned gf = R.facet_begin + f;
            const int ia = B.facet_vert[gf], ib = B.facet_vert[tf + gf], ic = B.facet_vert[2u * tf + gf];
            const double a[3] = {L.raw[ia], L.raw[L.np + ia], L.raw[2 * L.np + ia]}, b[3] = {L.raw[ib], L.raw[L.np + ib], L.raw[2 * L.np + ib]};
            const double c[3] = {L.raw[ic], L.raw[L.np + ic], L.raw[2 * L.np + ic]};
            const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
            vol += (1.0 / 6.0) * (cx * c[0] + cy * c[1] + cz * c[2]);
        }
        o.robot_volume[pass] = shape_block_sum(vol, S, tid);      // (ends with a barrier: the raw planes are free for the hull's scratch)
        bool ok;
        o.hull_volume[pass] = shape_hull(L, n, S, tid, ok);
        if (!ok) o.fallback = 1;
        __syncthreads();
    }
    if (tid == 0) Q.out[r] = o;
}

}  // namespace vxh
