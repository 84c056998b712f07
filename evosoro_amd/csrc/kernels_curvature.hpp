// k_shape_curvature: the per-vertex angle excess of the surface mesh of land_water robots on the device (engine option device_curvature),
// one workgroup of four wavefronts per robot.  The host routine it stands in for is mesh_angle_excess (results.cpp), the reference
// CVX_MeshUtil::computeShapeComplexity (LW/VX_MeshUtil.cpp:956-1014).  The kernel keeps the host's arithmetic -- every product, sum,
// quotient and square root rounded on its own, in the host's order -- and the host's order of summation, so that the only place the two
// can differ is acos itself.  Launched by launch_curvature.hip.
//
// Per robot two passes, the rest state and the final state, each:
//   a. one lane per mesh vertex: the mean of the <= 7 voxel corners meeting there -> point planes P[3][np]
//   b. one lane per record of the robot's corner table (device_types.hpp), chunk by chunk, a chunk per wavefront: the two edge vectors
//      from P, their lengths, the three guarded divisions each, the dot product, acos.  The corners of a vertex are neighbouring
//      lanes of one wavefront, in facet order: the lane of the first adds them left to right, from 0.0, fetching the angles of the
//      lanes behind it with wavefront shuffles, and writes 2 pi - sum.  No LDS staging of the angles, no atomics, no barrier.
// HBM = false: P is the workgroup's dynamic LDS (robots of up to VXH_CURV_LDS_MAX_VERT vertices); true: the robot's range of
// DCurv::pts, written and read by this workgroup alone (it stays in L2), everything else the same.
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.hpp"

namespace vxh {

#pragma clang fp contract(off)      // to the end of this header: the host's roundings (results.cpp is compiled without contraction)

// the angle at `at` between the edges to p and q: angle_at of mesh_angle_excess, operation for operation (Vec3D::Normalize: sqrt, then
// three divisions when the length is positive)
__device__ __forceinline__ double curv_angle(const double* X, const double* Y, const double* Z, int at, int p, int q)
{
    const double ax = X[at], ay = Y[at], az = Z[at];
    double v1x = X[p] - ax, v1y = Y[p] - ay, v1z = Z[p] - az, v2x = X[q] - ax, v2y = Y[q] - ay, v2z = Z[q] - az;
    const double l1 = sqrt(v1x * v1x + v1y * v1y + v1z * v1z), l2 = sqrt(v2x * v2x + v2y * v2y + v2z * v2z);
    if (l1 > 0) { v1x /= l1; v1y /= l1; v1z /= l1; }
    if (l2 > 0) { v2x /= l2; v2y /= l2; v2z /= l2; }
    return acos(v1x * v2x + v1y * v2y + v1z * v2z);
}

template <bool HBM>
static __global__ __launch_bounds__(VXH_CURV_THREADS) void k_shape_curvature(DBatch B, DCurv C)
{
    extern __shared__ double curv_lds[];
    const int r = (HBM ? C.hbm_list : C.list)[blockIdx.x], tid = threadIdx.x, lane = tid & 63;
    const DRobot& R = B.robot[r];
    const int n = R.nmv, steps = B.rstate[r].steps;
    const int np = HBM ? n : (n + 1) & ~1;
    double* const X = HBM ? C.pts + C.pts_begin[r] : curv_lds;
    double* const Y = X + np;
    double* const Z = Y + np;
    const unsigned long long* const rec = C.rec + C.rec_begin[r];
    const int n_rec = C.n_chunk[r] * VXH_CURV_CHUNK;
    const unsigned tm = B.total_mv, nv = B.nv;
    const double nom = R.lat;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && steps == 0) break;                    // (the rest pass has written both vectors, as the host returns the rest state twice)
        const int cur = steps & 1;
        // a. the vertices as mesh_vertices (results.cpp) places them, operation for operation: the statements of step (a) of
        //    k_shape_results (kernels_shape.hpp), without its rounding to six digits
        for (int i = tid; i < n; i += VXH_CURV_THREADS) {
            const unsigned gi = R.vert_begin + i;
            double ax = 0, ay = 0, az = 0, tw = 0;
            for (int q = 0; q < 8; ++q) {
                const int e = C.vert[(unsigned)q * tm + gi];
                if (e < 0) break;
                const unsigned u = (unsigned)e >> 3;
                const int corner = e & 7;
                double st[6] = {0, 0, 0, 0, 0, 0};
                double px = C.nom[u], py = C.nom[nv + u], pz = C.nom[2u * nv + u];
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
            X[i] = v0x + (ax * inv - v0x); Y[i] = v0y + (ay * inv - v0y); Z[i] = v0z + (az * inv - v0z);
        }
        __syncthreads();                                       // (HBM: the table is this workgroup's own, its stores are visible to it behind the barrier)
        // b. every thread makes the same number of rounds (the shuffles want whole wavefronts); a wavefront's 64 records are one chunk
        for (int base = 0; base < n_rec; base += VXH_CURV_THREADS) {
            const int k = base + tid;
            const unsigned long long w = k < n_rec ? rec[k] : curv_record(0, 0, 0, 0, VXH_CURV_IDLE);
            const int at = (int)(w & 0xFFFFu), len = (int)(w >> 48 & 0xFFu);
            const bool idle = (int)(w >> 56) == VXH_CURV_IDLE;
            const double angle = idle ? 0.0 : curv_angle(X, Y, Z, at, (int)(w >> 16 & 0xFFFFu), (int)(w >> 32 & 0xFFFFu));
            int longest = len;                                 // ... group of this chunk: how far its shuffles reach
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(longest, off); longest = o > longest ? o : longest; }
            double sum = 0.0;
            for (int j = 0; j < longest; ++j) {
                const double a = __shfl(angle, (lane + j) & 63);
                if (j < len) sum = sum + a;
            }
            if (len > 0) {
                const double excess = (2.0 * 3.14159265358979) - sum;
                C.out[(size_t)pass * tm + R.vert_begin + at] = excess;
                if (steps == 0) C.out[(size_t)tm + R.vert_begin + at] = excess;
            }
        }
        __syncthreads();                                       // (the next pass overwrites the points)
    }
}

}  // namespace vxh
