// Cross-checks of the developer library (libvxhip_prof.so, -DVXH_PHASE_TIMING; switched on by DBatch::dbg bits, scripts/dev_gpu_diag.py):
// the resident kernel includes this header in that build only and calls each check from one line of its step loop.  The counters are
// the XREB / XROW words of ProfSlot (device_types.hpp); dev_report.cpp prints them.
#pragma once
#ifndef VXH_PHASE_TIMING
#error "kernels_dev.hpp is part of the developer build only"
#endif
#include <hip/hip_runtime.h>

#include "device_types.hpp"
#include "kernels_group.hpp"

namespace vxh {

// dbg 16, behind a broad-phase run of fused_rebuild: the plain scan must leave the same rows (count, partners, stiffness bits).
// Every thread of the workgroup calls (barriers inside); shi: the scratch of fused_rebuild_plain.
template <int BLOCK>
__device__ __forceinline__ void dev_check_rebuild(const DBatch& B, const DRobot& R, DRobotState& rs, const double* ps, int* shi, const DVoxClass* vct, int tid)
{
    int my_row = -1, n_new = 0; unsigned long long sum_new = 0;
    if (tid < R.nsurf) {
        my_row = R.surf_begin + tid; n_new = B.col_cnt[my_row];
        for (int k = 0; k < n_new; ++k) { const size_t at = col_at(R, k, my_row); sum_new += (unsigned long long)(k + 1) * ((unsigned long long)B.col_partner[at] * 1000003ull + (unsigned long long)__double_as_longlong(B.col_a1[at])); }
    }
    __syncthreads();
    fused_rebuild_plain<BLOCK>(B, R, rs, ps, shi, vct);
    if (tid < R.nsurf) {
        const int n_old = B.col_cnt[my_row]; unsigned long long sum_old = 0;
        for (int k = 0; k < n_old; ++k) { const size_t at = col_at(R, k, my_row); sum_old += (unsigned long long)(k + 1) * ((unsigned long long)B.col_partner[at] * 1000003ull + (unsigned long long)__double_as_longlong(B.col_a1[at])); }
        atomicAdd(&B.prof[VXH_PROF_XREB_ROWS], 1ull);
        if (n_old != n_new || sum_old != sum_new) atomicAdd(&B.prof[VXH_PROF_XREB_DIFFER], 1ull);
        if (n_new > n_old) atomicAdd(&B.prof[VXH_PROF_XREB_LONGER], 1ull);
        if (n_new < n_old) atomicAdd(&B.prof[VXH_PROF_XREB_SHORTER], 1ull);
        atomicMax(&B.prof[VXH_PROF_XREB_MAX_NEW], (unsigned long long)n_new);
        atomicMax(&B.prof[VXH_PROF_XREB_MAX_OLD], (unsigned long long)n_old);
        atomicAdd(&B.prof[VXH_PROF_XREB_SUM_NEW], (unsigned long long)n_new);
        atomicAdd(&B.prof[VXH_PROF_XREB_SUM_OLD], (unsigned long long)n_old);
    }
    __syncthreads();
}

// dbg 8, a lane whose contact row is in the workgroup's LDS copy, behind its fused_contact_forces: the same sum through the rows in memory
// must give the same bits.  F_before / F: the force in front of and behind the contact forces; mask_seen: the reach bits pass 2 consumed.
template <int BLOCK>
__device__ __forceinline__ void dev_check_contact_rows(const DBatch& B, const DRobot& R, const double* ps, d3 F_before, d3 F, const VoxState& S, int tid, int vv,
                                                       int rowd, unsigned long long mask_seen, unsigned long long* cmask, const int* rc_code, const double* rc_a1)
{
    const int base = R.vox_begin;
    const d3 G = fused_contact_forces<BLOCK>(B, R, ps, F_before, S.pos, S.scale, tid, vv, rowd & VXH_ROWD_MASK, cmask, rc_code, rc_a1);
    atomicAdd(&B.prof[VXH_PROF_XROW_LANES], 1ull);
    if (!(G.x == F.x && G.y == F.y && G.z == F.z)) {
        atomicAdd(&B.prof[VXH_PROF_XROW_DIFFER], 1ull);
        // pairs of my row in reach by CalcContactForce's own test, against the bits pass 1 set for me
        int reach = 0;
        const int crow0 = R.surf_begin + B.surf_ord[vv];
        for (int k = 0; k < (rowd & VXH_ROWD_MASK); ++k) {
            const int q = B.col_partner[col_at(R, k, crow0)] - base;
            if (contact_in_reach(ps[q] - S.pos.x, ps[BLOCK + q] - S.pos.y, ps[2 * BLOCK + q] - S.pos.z, (ps[3 * BLOCK + q] + S.scale) * 0.75)) ++reach;
        }
        const int bits = __builtin_popcountll(mask_seen);
        atomicAdd(&B.prof[bits < reach ? VXH_PROF_XROW_FEWER : (bits > reach ? VXH_PROF_XROW_MORE : VXH_PROF_XROW_AS_MANY)], 1ull);
    }
    // is the LDS copy of my row what memory holds now?  (partner and stiffness of every entry, bit for bit)
    const int crow = R.surf_begin + B.surf_ord[vv], coff = (rowd >> VXH_ROWD_BITS) - 1;
    bool same = true;
    for (int k = 0; k < (rowd & VXH_ROWD_MASK); ++k) {
        const size_t at = col_at(R, k, crow);
        same = same && (rc_code[coff + k] & 1023) == B.col_partner[at] - base && rc_a1[coff + k] == B.col_a1[at];
    }
    if (B.col_cnt[crow] != (rowd & VXH_ROWD_MASK)) same = false;
    if (!same) atomicAdd(&B.prof[VXH_PROF_XROW_LDS_DIFFERS], 1ull);
}

}  // namespace vxh
