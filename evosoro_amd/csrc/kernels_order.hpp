// k_dispatch_order: the dispatch order of a launch group's next launch from the cost words its last launch left (dispatch_order.hpp).
// Queued in front of the launch on the same stream -- launches of one call are queued without a host synchronisation, so the order is made
// on the device.  A rank by counting: thread i counts the entries that go before its own and writes perm[rank] = i.  The words of all
// entries differ (the list index is part of them), so the ranks are a permutation whatever the cost words hold.  Any list length: one
// workgroup per 256 entries, the words staged through LDS 1024 at a time; no workgroup waits for another.
// Cost (MI355X, 512 robots): two workgroups, 512 broadcast LDS reads per thread -- see DESIGN.md "The cost of a launch".
#pragma once
#include <hip/hip_runtime.h>
#include "dispatch_order.hpp"

namespace vxh {

enum { VXH_ORDER_BLOCK = 256, VXH_ORDER_CHUNK = 1024 };

static __global__ __launch_bounds__(VXH_ORDER_BLOCK) void k_dispatch_order(const DispatchCost* __restrict__ cost, int n, int len, int* __restrict__ perm)
{
    __shared__ unsigned long long s_words[VXH_ORDER_CHUNK];
    const int i = (int)blockIdx.x * VXH_ORDER_BLOCK + (int)threadIdx.x;
    const unsigned long long mine = i < n ? dispatch_word(dispatch_key(cost[i], len), i) : 0ull;
    int rank = 0;
    for (int c0 = 0; c0 < n; c0 += VXH_ORDER_CHUNK) {
        const int cn = min((int)VXH_ORDER_CHUNK, n - c0);
        __syncthreads();                       // (the previous chunk has been read)
        for (int k = (int)threadIdx.x; k < cn; k += VXH_ORDER_BLOCK) s_words[k] = dispatch_word(dispatch_key(cost[c0 + k], len), c0 + k);
        __syncthreads();
        rank += dispatch_rank(s_words, cn, mine);
    }
    if (i < n) perm[rank] = i;                 // (rank < n: at most n - 1 entries go before one of the list)
}

}  // namespace vxh
