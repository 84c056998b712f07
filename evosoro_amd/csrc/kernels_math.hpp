// Layer 1 of the device code: vectors and quaternions, the lean FP64 sqrt / divide / rsqrt forms, wavefront reductions and the quaternion
// functions of Vec3D.h.  Nothing here knows a DBatch.  The angle constants (VXH_*_RAD, VXH_HYST) are in device_types.hpp, where host
// code reads them too.  Layers above: kernels_physics.hpp, kernels_group.hpp, then one header per kernel family.
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.hpp"

namespace vxh {

struct d3 { double x, y, z; };
struct dq { double w, x, y, z; };

__device__ __forceinline__ d3 mk3(double x, double y, double z) { d3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ dq mkq(double w, double x, double y, double z) { dq r; r.w = w; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ d3 operator+(d3 a, d3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ d3 operator-(d3 a, d3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ d3 operator-(d3 a) { return mk3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ d3 operator*(d3 a, double f) { return mk3(f * a.x, f * a.y, f * a.z); }
__device__ __forceinline__ double len2(d3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
__device__ __forceinline__ dq conj(dq a) { return mkq(a.w, -a.x, -a.y, -a.z); }
__device__ __forceinline__ dq qmul(dq a, dq f)      // Vec3D.h:193
{
    return mkq(a.w * f.w - a.x * f.x - a.y * f.y - a.z * f.z,
               a.w * f.x + a.x * f.w + a.y * f.z - a.z * f.y,
               a.w * f.y - a.x * f.z + a.y * f.w + a.z * f.x,
               a.w * f.z + a.x * f.y - a.y * f.x + a.z * f.w);
}
// qmul(a, f) for a quaternion whose x component is an exact zero (what FromAngleToPosX returns): the four products with it and their
// additions left out -- x +- 0 == x, so the same values; the compiler may not drop a multiplication by a zero it cannot prove finite
__device__ __forceinline__ dq qmul_x0(dq a, dq f)
{
    return mkq(a.w * f.w - a.y * f.y - a.z * f.z,
               a.w * f.x + a.y * f.z - a.z * f.y,
               a.w * f.y + a.y * f.w + a.z * f.x,
               a.w * f.z - a.y * f.x + a.z * f.w);
}
__device__ __forceinline__ d3 rotinv(dq q, d3 f)    // CQuat::RotateVec3DInv, Vec3D.h:300-314
{
    double tw = q.x * f.x + q.y * f.y + q.z * f.z;
    double tx = q.w * f.x - q.y * f.z + q.z * f.y;
    double ty = q.w * f.y + q.x * f.z - q.z * f.x;
    double tz = q.w * f.z - q.x * f.y + q.y * f.x;
    return mk3(tw * q.x + tx * q.w + ty * q.z - tz * q.y,
               tw * q.y - tx * q.z + ty * q.w + tz * q.x,
               tw * q.z + tx * q.y - ty * q.x + tz * q.w);
}
// v -> conj(q) v q as a matrix-vector product: 28 operations once, 9 per vector (rotinv: 24 each).  NOT for unit quaternions only:
// the diagonal carries |q|^2, as the sandwich does.  The bond frame's quaternion is not always a unit one -- FromAngleToPosX's
// small-angle branch returns (1 - (y^2 + z^2) / 2, 0, y, z), of norm^2 1 + (y^2 + z^2)^2 / 4, up to 1 + 5e-9 -- and the reference's
// RotateVec3DInv scales the back-rotated forces and moments of such a bond by it.  Until round 3 the diagonal was 1 - 2 (y^2 + z^2):
// every large-angle bond with a small bend differed from the reference by that factor, 1e-13 .. 1e-9 of its force, step after step
// in the same direction -- the "creep" of the long runs (scripts/dev_gpu_diag.py drift7: one step of engine and oracle from the
// same state differed by 1e-12 voxel, 500 x what a one-ulp change of the inputs does to the oracle).
struct RotInv {
    double m00, m01, m02, m10, m11, m12, m20, m21, m22;
    __device__ __forceinline__ explicit RotInv(dq q)
    {
        const double x2 = q.x + q.x, y2 = q.y + q.y, z2 = q.z + q.z;
        const double xx = x2 * q.x, yy = y2 * q.y, zz = z2 * q.z, xy = x2 * q.y, xz = x2 * q.z, yz = y2 * q.z, wx = x2 * q.w, wy = y2 * q.w, wz = z2 * q.w;
        const double n = (q.w * q.w + q.x * q.x) + (q.y * q.y + q.z * q.z);
        m00 = n - (yy + zz); m11 = n - (xx + zz); m22 = n - (xx + yy);
        m01 = xy + wz; m10 = xy - wz;        // row i of R^T = column i of the rotation matrix of q
        m02 = xz - wy; m20 = xz + wy;
        m12 = yz + wx; m21 = yz - wx;
    }
    __device__ __forceinline__ d3 operator()(d3 f) const
    {
        return mk3(m00 * f.x + m01 * f.y + m02 * f.z, m10 * f.x + m11 * f.y + m12 * f.z, m20 * f.x + m21 * f.y + m22 * f.z);
    }
};

// ToXDirBond / ToOrigDirBond, VX_Bond.h:45-48 ; axis 0 = X, 1 = Y, 2 = Z.  The axis is a template argument: the frame
// change is a compile-time permutation, not a chain of selects.
template <int A> __device__ __forceinline__ d3 to_xdir(d3 p)
{
    if constexpr (A == 1) return mk3(p.y, -p.x, p.z);
    else if constexpr (A == 2) return mk3(p.z, p.y, -p.x);
    else return p;
}
template <int A> __device__ __forceinline__ dq to_xdir(dq q)
{
    if constexpr (A == 1) return mkq(q.w, q.y, -q.x, q.z);
    else if constexpr (A == 2) return mkq(q.w, q.z, q.y, -q.x);
    else return q;
}
template <int A> __device__ __forceinline__ d3 to_orig(d3 p)
{
    if constexpr (A == 1) return mk3(-p.y, p.x, p.z);
    else if constexpr (A == 2) return mk3(-p.z, p.y, p.x);
    else return p;
}

// FP64 sqrt / divide / reciprocal as the instruction sequences the device library emits for them, minus the operand
// range scaling (v_div_scale / v_ldexp) and the special-value fix-up (v_div_fixup, v_cmp_class): for finite, normal,
// non-zero operands -- everything on this path, which works in metres, newtons and unit quaternions -- the results are
// bit-identical to sqrt(), a / b and 1.0 / b at 10, 8 and 7 instead of 18, 11 and 11 instructions.  The *_nn variant
// also returns 0 for a zero argument.
__device__ __forceinline__ double vsqrt(double x)
{
    double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = y * 0.5;
    double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g); h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    return __builtin_fma(d, h, g);
}
// 1 / sqrt(x), x > 0 normal: v_rsq_f64 + ONE third-order step, <= 1 ulp.  With e = 1 - x y0^2 the exact value is y0 / sqrt(1 - e) =
// y0 (1 + e/2 + 3 e^2/8 + 5 e^3/16 + ...); v_rsq_f64 is good to 2^-23 (|e| <= 2^-22), so the series cut after e^2 is off by 2^-68
// and what is left is rounding: half an ulp from the product x y0 inside e, half from the final fused multiply-add.  (Until round
// 4 a second, second-order step followed: four more instructions per call, five to six calls per large-angle bond, for the last
// quarter of an ulp.)
__device__ __forceinline__ double vrsqrt(double x)
{
    double y = __builtin_amdgcn_rsq(x);
    double e = __builtin_fma(-x * y, y, 1.0);
    return __builtin_fma(y * e, __builtin_fma(e, 0.375, 0.5), y);      // y (1 + e/2 + 3 e^2/8)
}
__device__ __forceinline__ double vsqrt_nn(double x) { const double s = vsqrt(x); return x == 0 ? 0.0 : s; }
__device__ __forceinline__ double vrcp(double b)
{
    double r = __builtin_amdgcn_rcp(b);
    double e = __builtin_fma(-b, r, 1.0); r = __builtin_fma(r, e, r);
    e = __builtin_fma(-b, r, 1.0); r = __builtin_fma(r, e, r);
    e = __builtin_fma(-b, r, 1.0);
    return __builtin_fma(e, r, r);
}
__device__ __forceinline__ double vdiv(double a, double b)
{
    double r = __builtin_amdgcn_rcp(b);
    double e = __builtin_fma(-b, r, 1.0); r = __builtin_fma(r, e, r);
    e = __builtin_fma(-b, r, 1.0); r = __builtin_fma(r, e, r);
    double q = a * r;
    e = __builtin_fma(-b, q, a);
    return __builtin_fma(e, r, q);
}

// acos for |x| <= 1, <= 1 ulp: the usual reduction (|x| < 0.5: pi/2 - asin x; else 2 asin sqrt((1 - |x|)/2)) with
// asin(s) = s + s z R(z), z = s^2 in [0, 1/4], R a degree-11 polynomial (Chebyshev-node interpolant of
// (asin(sqrt z) - sqrt z)/(z sqrt z), relative error 6e-17).  The coefficients are pinned to scalar registers: as
// literals the compiler moves each of them into a vector register pair per evaluation (FP64 has no 64-bit literals).
__device__ __forceinline__ double sconst(double c) { asm volatile("" : "+s"(c)); return c; }
// z P(z) of asin(s) = s (1 + z P(z)), z = s^2 <= 1/4 (the device library's acos polynomial)
__device__ __forceinline__ double asin_zp(double z)
{
    double p = sconst(0.028169218060881414);
    p = __builtin_fma(p, z, sconst(-0.010749050339697808));
    p = __builtin_fma(p, z, sconst(0.01603551434914882));
    p = __builtin_fma(p, z, sconst(0.0078029494773533175));
    p = __builtin_fma(p, z, sconst(0.011875494382636922));
    p = __builtin_fma(p, z, sconst(0.013929652902326633));
    p = __builtin_fma(p, z, sconst(0.017355259955786323));
    p = __builtin_fma(p, z, sconst(0.02237204763174451));
    p = __builtin_fma(p, z, sconst(0.03038194736709848));
    p = __builtin_fma(p, z, sconst(0.044642857103423646));
    p = __builtin_fma(p, z, sconst(0.07500000000020764));
    p = __builtin_fma(p, z, sconst(0.1666666666666665));
    p *= z;
    return p;
}
__device__ __forceinline__ double vacos(double x)
{
    const double ax = fabs(x);
    const bool big = ax >= 0.5;
    const double z = big ? __builtin_fma(ax, -0.5, 0.5) : x * x;
    const double p = asin_zp(z);
    if (big) {
        const double s = vsqrt_nn(z);
        const double r = 2.0 * __builtin_fma(s, p, s);
        return x > 0 ? r : 3.141592653589793 - (r - 1.2246467991473532e-16);
    }
    return 1.5707963267948966 - (x + __builtin_fma(x, p, -6.123233995736766e-17));
}

// max of a non-negative double over the 64 lanes of a (fully active) wavefront, returned in every lane.  Non-negative doubles order
// like their bit patterns read as unsigned 64-bit integers, i.e. lexicographically by (high word, low word): the maximum of the
// high words first (v_max_u32 takes a DPP source: ONE instruction per stage -- four row shifts, two row broadcasts), then the
// maximum of the low words among the lanes that hold that high word.  14 vector instructions where the FP64 compare-and-select
// version (v_max_f64 is VOP3: no DPP) took 36; same bits.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_umax_stage(unsigned v)
{
    const unsigned o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);     // 0 where no lane feeds this one
    return o > v ? o : v;
}
__device__ __forceinline__ unsigned wave_umax(unsigned v)
{
    v = dpp_umax_stage<0x111, 0xf>(v);      // row_shr:1
    v = dpp_umax_stage<0x112, 0xf>(v);      // row_shr:2
    v = dpp_umax_stage<0x114, 0xf>(v);      // row_shr:4
    v = dpp_umax_stage<0x118, 0xf>(v);      // row_shr:8   -> lane 15 of every row of 16 holds the row's maximum
    v = dpp_umax_stage<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
    v = dpp_umax_stage<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3 -> lane 63 holds the maximum
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ double wave_max_nonneg(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned hi = wave_umax((unsigned)(b >> 32));
    const unsigned lo = wave_umax((unsigned)(b >> 32) == hi ? (unsigned)b : 0u);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// min / max of any doubles over the 64 lanes of a (fully active) wavefront, returned in every lane (a lane without a source keeps its
// own value, so no sign convention is needed)
template <int CTRL, int ROW_MASK, bool MAX>
__device__ __forceinline__ double dpp_minmax_stage(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)b, (int)(unsigned)b, CTRL, ROW_MASK, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(b >> 32), (int)(unsigned)(b >> 32), CTRL, ROW_MASK, 0xf, false);
    const double o = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    return MAX ? (o > v ? o : v) : (o < v ? o : v);
}
template <bool MAX>
__device__ __forceinline__ double wave_minmax(double v)
{
    v = dpp_minmax_stage<0x111, 0xf, MAX>(v);
    v = dpp_minmax_stage<0x112, 0xf, MAX>(v);
    v = dpp_minmax_stage<0x114, 0xf, MAX>(v);
    v = dpp_minmax_stage<0x118, 0xf, MAX>(v);
    v = dpp_minmax_stage<0x142, 0xa, MAX>(v);
    v = dpp_minmax_stage<0x143, 0xc, MAX>(v);
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), 63);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// CQuat::FromAngleToPosX, Vec3D.h:208-237: the rotation that takes `from` onto +X, axis (0, n.z, -n.y)/sin(theta), angle
// theta = acos(n.x).  The reference evaluates (cos, sin)(theta/2) through acos + sincos; here the same quaternion is
// written with the half-angle identities cos(theta/2) = sqrt((1 + n.x)/2), sin(theta/2)/sin(theta) = 1/(2 cos(theta/2)):
//     (c, 0, n.z/(2c), -n.y/(2c)),  c = sqrt((1 + n.x)/2)
// acos is ill-conditioned near n.x = 1 (d theta = d n.x / sin theta), so the reference's own value moves by up to 1e-12
// (relative) under a 1-ulp change of `from`; the identity form agrees with it to 8e-13 max / 4e-15 median over bend angles
// of 1..35 degrees (DESIGN.md "Numerics") at a quarter of the instructions.  The theta > PI - 1e-7 cut is kept on n.x.
// Round 4 (instruction diet): the function also returns |from| -- the large-angle branch of CalcLinForce needs the bond's length
// (Pos2.x = |x2 - x1| - NomDistance, VXS_BondInternal.cpp:104) and this normalisation needs 1 / |from|: one refined v_rsq_f64 gives
// both (len = L2 * rsqrt(L2), <= 1.5 ulp, where the reference takes a correctly rounded sqrt of the un-rotated difference: a relative
// 2e-16 on a length whose elongation is 1e-4 .. 1e-1 of it); and the SmallAngle test |y/x|, |z/x| < SMALL_ANGLE_RAD is made on the
// cross-multiplied form |y|, |z| < SMALL_ANGLE_RAD |x| (x == 0: false, like the reference's inf / NaN quotients), so that the
// reciprocal of x is only formed for the lanes that take that branch.
__device__ __forceinline__ dq from_angle_to_pos_x(d3 from, double& len)
{
    const double L2 = from.x * from.x + from.y * from.y + from.z * from.z;
    if (from.x == 0 && from.y == 0 && from.z == 0) { len = 0.0; return mkq(1, 0, 0, 0); }
    const double li = vrsqrt(L2);             // NormalizeFast: from * (1 / |from|)
    len = L2 * li;
    const double ax = VXH_SMALL_ANGLE_RAD * fabs(from.x);
    if (fabs(from.y) < ax && fabs(from.z) < ax) {
        const double rx = vrcp(from.x);
        const double y = 0.5 * (from.z * rx), z = -0.5 * (from.y * rx);
        return mkq(1 + 0.5 * (-y * y - z * z), 0, y, z);
    }
    const d3 n = from * li;
    if (n.x < -0.999999999999995) return mkq(0, 0, 1, 0);     // cos(PI - DISCARD_ANGLE_RAD)
    const double s = 0.5 + 0.5 * n.x, ri = vrsqrt(s);         // c = sqrt(s), 1 / (2 c) = ri / 2
    const double c = s * ri, h = 0.5 * ri;
    return mkq(c, 0, n.z * h, -n.y * h);
}
// CQuat::ToRotationVector, Vec3D.h:270-285
// 1 - w * w with the product rounded on its own, as the reference's FMA-less build forms it.  For a small rotation (w within 1e-4
// of 1) the rounding of w * w is a relative error of 1e-12 in the difference; contracted into one fused multiply-add the engine's
// value was the more accurate one -- and 1e-12 away from the reference's, which showed as a jump of the error against the oracle
// from 1e-14 to 6e-12 (relative, angular velocity) on the step the first bonds of a violently starting robot turn large-angle
// (tests/golden/vxa/lw_hexapus.vxa, step 4; scripts/dev_gpu_diag.py drift3, round 3).
#pragma clang fp contract(off)
__device__ __forceinline__ double one_minus_square(double w) { const double ww = w * w; return 1.0 - ww; }
#pragma clang fp contract(fast)
// Round 4 (instruction diet).  f = 2 * (angle / sin(angle/2) / 2) in three branches:
//   sl < SLTHRESH   the reference's sqrt((2 - 2w) / sl) as (2 - 2w) * rsqrt((2 - 2w) * sl), sl = 1 - fl(w w) with the reference's own
//                   rounding of w w (one_minus_square above: for a small rotation that rounding is a relative 1e-12 of sl, and the
//                   engine must make the same "error");
//   else, w >= 0.5  (every bond that is not folded back on itself)  acos(w) = 2 asin(s), s = sqrt(z), z = (1 - w)/2, asin(s) = s (1 + z P(z))
//                   with vacos' polynomial; and sqrt(sl) = sqrt((1 - w)(1 + w)) = s sqrt(2 + 2w), so that
//                       acos(w) / sqrt(sl) = (2 + 2 z P(z)) * rsqrt(2 + 2w)
//                   -- ONE refined v_rsq_f64 of a well-conditioned argument where acos-then-divide takes a sqrt and a rsqrt (-14 vector
//                   instructions per call, two calls per large-angle bond).  It does not go through sl, hence not through the
//                   rounding of w w: on this branch sl > 2.4e-3, that rounding is a relative < 2.5e-14 of the result.
//   else            acos(w) * rsqrt(sl) as before (never taken by a sane bond; kept for the function's contract).
// The factor 2 of the rotation vector is folded into f (exact).
// SEL (the 768-thread resident kernel, kernels_fused.hpp fused_bond): the select form -- numerator and rsqrt argument of the lane's branch chosen first, ONE refined v_rsq_f64
// for both (the same operations on the same values per lane as the branched form: same bits, scripts/dev_gpu_diag.py statehash).
// Measured, same box: resident kernel 25.15 -> 24.96 us per step (its wavefronts are of both kinds, and run both branches); the wide
// kernel the other way, 64 x 6^3 5.6 -> 5.7, swimmers 13.8 -> 14.0, 512 x 8^3 16.75 -> 17.05 -- hence a switch.
template <bool SEL = false>
__device__ __forceinline__ double rotvec_factor(double w, double slthresh)
{
    const double sl = one_minus_square(w);
    if constexpr (SEL) {
        if (__builtin_expect(w < 0.5 && sl >= slthresh, 0)) return 2.0 * vacos(w) * vrsqrt(sl);
        const double z = __builtin_fma(w, -0.5, 0.5);
        const double p = asin_zp(z);
        const bool approx = sl < slthresh;
        const double a = __builtin_fma(w, -2.0, 2.0), a2 = __builtin_fma(w, -4.0, 4.0);
        const double num = approx ? a2 : __builtin_fma(p, 4.0, 4.0);
        const double arg = approx ? a * sl : __builtin_fma(w, 2.0, 2.0);
        const double f = num * vrsqrt(arg);
        return sl <= 0 ? 0.0 : f;
    }
    if (sl <= 0) return 0.0;                   // (sl > 0 from here: |w| < 1, the reference's clamp of w to 1 cannot act)
    if (sl < slthresh) {
        const double a = __builtin_fma(w, -2.0, 2.0), a2 = __builtin_fma(w, -4.0, 4.0);
        return a2 * vrsqrt(a * sl);
    }
    if (w >= 0.5) {
        const double z = __builtin_fma(w, -0.5, 0.5);
        const double p = asin_zp(z);
        return __builtin_fma(p, 4.0, 4.0) * vrsqrt(__builtin_fma(w, 2.0, 2.0));
    }
    return 2.0 * vacos(w) * vrsqrt(sl);
}
template <bool SEL = false>
__device__ __forceinline__ d3 to_rotvec(dq q, double slthresh)
{
    const double f = rotvec_factor<SEL>(q.w, slthresh);
    return mk3(q.x * f, q.y * f, q.z * f);
}

// to_xdir<A> / to_orig<A> for an axis that is a per-lane run-time value (bond_compute_rt, kernels_physics.hpp): the same permutations
// written with selects: bit-identical results (negation is exact).
__device__ __forceinline__ d3 to_xdir_rt(int a, d3 p) { return mk3(a == 0 ? p.x : (a == 1 ? p.y : p.z), a == 1 ? -p.x : p.y, a == 2 ? -p.x : p.z); }
__device__ __forceinline__ dq to_xdir_rt(int a, dq q) { return mkq(q.w, a == 0 ? q.x : (a == 1 ? q.y : q.z), a == 1 ? -q.x : q.y, a == 2 ? -q.x : q.z); }
__device__ __forceinline__ d3 to_orig_rt(int a, d3 p) { return mk3(a == 0 ? p.x : (a == 1 ? -p.y : -p.z), a == 1 ? p.x : p.y, a == 2 ? p.x : p.z); }

__device__ __forceinline__ d3 cross3(d3 a, d3 b) { return mk3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ double dot3(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ d3 normalized3(d3 a) { const double l = vsqrt_nn(len2(a)); return l > 0 ? a * vrcp(l) : a; }

// CQuat::RotateVec3D (Vec3D.h:293-299) as a matrix: q f q* = M f for a unit quaternion (|q| = 1 to rounding).  A voxel's eight
// mesh corners go through the same rotation, so it is expanded once per voxel (§ Numerics).
struct RotFwd {
    double m[9];
    __device__ __forceinline__ RotFwd() {}
    __device__ __forceinline__ explicit RotFwd(dq q)
    {
        const double x2 = q.x + q.x, y2 = q.y + q.y, z2 = q.z + q.z;
        const double xx = q.x * x2, yy = q.y * y2, zz = q.z * z2, xy = q.x * y2, xz = q.x * z2, yz = q.y * z2, wx = q.w * x2, wy = q.w * y2, wz = q.w * z2;
        m[0] = 1 - (yy + zz); m[1] = xy - wz; m[2] = xz + wy;
        m[3] = xy + wz; m[4] = 1 - (xx + zz); m[5] = yz - wx;
        m[6] = xz - wy; m[7] = yz + wx; m[8] = 1 - (xx + yy);
    }
    __device__ __forceinline__ d3 operator()(d3 f) const
    { return mk3(m[0] * f.x + m[1] * f.y + m[2] * f.z, m[3] * f.x + m[4] * f.y + m[5] * f.z, m[6] * f.x + m[7] * f.y + m[8] * f.z); }
};

}  // namespace vxh
