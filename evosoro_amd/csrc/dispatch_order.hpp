// Dispatch order of a launch group by measured cost, longest first: the rule as plain C++, shared by the ordering kernel
// (kernels_order.hpp), the resident kernel that leaves the cost words (kernels_fused.hpp) and the host check (order_check.cpp).
//
// A launch ends with its slowest CU, and a CU steps its robots one after the other (two per CU for the 512-robot population): handing
// the workgroups out by descending cost pairs the expensive robots with the cheap ones.  What a robot costs is measured, not guessed:
// every workgroup of k_robot_steps leaves a DispatchCost for its robot when its launch ends, and the next launch is ordered by the key
// below.  The robots do not interact, so the order changes no result.
#pragma once

#if defined(__HIP__)
#define VXH_ORDER_HD __host__ __device__
#else
#define VXH_ORDER_HD
#endif

namespace vxh {

// What a launch leaves for each robot of its list (indexed by list position).  Times in ticks of the constant-rate clock.
struct DispatchCost {
    float step_ticks;     // wall time per step of the launch, broad-phase runs excluded (for a robot that runs one every step: included)
    float reb_ticks;      // its last broad-phase run (0: none seen yet)
    float disp_frac;      // displacement since the last run as a fraction of what triggers the next one (max_disp / ((col_horizon - 1) / 2))
    float rate_frac;      // ... and how much of that fraction a step adds, averaged since the last run (0: no horizon, no runs to predict)
    int left;             // steps until the robot's own stop condition (0: stopped)
    int launch_ticks;     // the whole launch, runs included (the engine's VXH_PROF_ORDER report; not part of the key)
};

// A launch group's workspace, one allocation of 8-byte words: the permutation of the next long launch [n ints], then the cost words [n]
VXH_ORDER_HD inline int order_ws_words(int n) { return (n + 1) / 2 + 3 * n; }
VXH_ORDER_HD inline DispatchCost* order_ws_cost(const int* perm, int n) { return (DispatchCost*)(perm + 2 * ((n + 1) / 2)); }
static_assert(sizeof(DispatchCost) == 24, "three 8-byte words per cost word");

// time the robot is expected to keep its CU in a launch of `len` steps
VXH_ORDER_HD inline float dispatch_key(const DispatchCost& c, int len)
{
    const int m = len < c.left ? len : c.left;
    if (m <= 0) return 0.f;
    const float runs_f = c.disp_frac + c.rate_frac * (float)m;               // broad-phase runs predicted within the launch
    const int runs = !(runs_f >= 1.f) ? 0 : (runs_f >= (float)m ? m : (int)runs_f);
    const float key = (float)m * c.step_ticks + (float)runs * c.reb_ticks;
    return key > 0.f && key < 3e38f ? key : 0.f;                              // (whatever the words hold: a finite, non-negative key)
}

// Key and list index as one word with a strict total order: a larger key first, equal keys by ascending index.  (A non-negative float's
// bit pattern orders like its value.)
VXH_ORDER_HD inline unsigned long long dispatch_word(float key, int index)
{
    union { float f; unsigned u; } b; b.f = key;
    return ((unsigned long long)b.u << 32) | (unsigned long long)(0xffffffffu - (unsigned)index);
}

// rank of entry i among words[0 .. n): the number of entries that go before it.  All words differ, so the ranks are a permutation.
VXH_ORDER_HD inline int dispatch_rank(const unsigned long long* words, int n, unsigned long long mine)
{
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += words[j] > mine ? 1 : 0;
    return rank;
}

// the whole order on the host (order_check.cpp; the engine's VXH_PROF_ORDER report): perm[k] = list index of the k-th workgroup
inline void dispatch_order_host(const DispatchCost* cost, int n, int len, unsigned long long* words, int* perm)
{
    for (int i = 0; i < n; ++i) words[i] = dispatch_word(dispatch_key(cost[i], len), i);
    for (int i = 0; i < n; ++i) perm[dispatch_rank(words, n, words[i])] = i;
}

}  // namespace vxh
