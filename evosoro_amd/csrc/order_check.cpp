// Host check of the dispatch-order rule (dispatch_order.hpp; no HIP, plain C++): seeded random tables of costs, remaining steps and
// states, the order built exactly as k_dispatch_order builds it (word per entry, rank by counting), and the two properties the engine
// relies on: the result is a permutation whatever the cost words hold, and it is non-increasing in the key, ties by list index.
//   make order_check [CHECK_OUT=dir] [SAN=-fsanitize=address,undefined] && ./order_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "dispatch_order.hpp"

using namespace vxh;

namespace {

enum Table { RANDOM, TIES, ALL_ZERO, STOPPED, GARBAGE };
const char* const table_names[] = {"random", "ties", "all-zero keys", "stopped robots", "garbage words"};

std::vector<DispatchCost> make_table(Table kind, int n, std::mt19937& rng)
{
    std::uniform_real_distribution<float> step(900.f, 1400.f), reb(0.f, 6000.f), frac(0.f, 1.2f), rate(0.f, 0.05f);
    std::uniform_int_distribution<int> left(0, 5000), coin(0, 2), bits(0, 0x7fffffff);
    std::vector<DispatchCost> t(n);
    for (int i = 0; i < n; ++i) {
        DispatchCost& c = t[i];
        c.step_ticks = step(rng); c.reb_ticks = reb(rng); c.disp_frac = frac(rng); c.rate_frac = coin(rng) ? rate(rng) : 0.f; c.left = 1 + left(rng); c.launch_ticks = 0;
        if (kind == TIES) { c.step_ticks = 1000.f + 100.f * (float)coin(rng); c.reb_ticks = 0.f; c.left = 100000; }     // three distinct keys in all
        if (kind == ALL_ZERO) { c.step_ticks = 0.f; c.reb_ticks = 0.f; }
        if (kind == STOPPED && coin(rng) == 0) c.left = 0;
        if (kind == GARBAGE) {                  // what an unwritten buffer might hold: any bit pattern, NaN and infinities included
            unsigned w[6];
            for (unsigned& x : w) x = (unsigned)bits(rng) * 2u + (unsigned)coin(rng);
            std::memcpy(&c, w, sizeof(c));
            if (i % 7 == 0) c.step_ticks = std::numeric_limits<float>::quiet_NaN();
            if (i % 11 == 0) c.reb_ticks = std::numeric_limits<float>::infinity();
            if (i % 13 == 0) c.step_ticks = -1.f;
        }
    }
    return t;
}

int check(Table kind, int n, int len, unsigned seed)
{
    std::mt19937 rng(seed);
    const std::vector<DispatchCost> cost = make_table(kind, n, rng);
    std::vector<unsigned long long> words(n);
    std::vector<int> perm(n, -1);
    dispatch_order_host(cost.data(), n, len, words.data(), perm.data());
    int bad = 0;
    std::vector<int> seen(n, 0);
    for (int k = 0; k < n; ++k) {
        if (perm[k] < 0 || perm[k] >= n) { ++bad; continue; }
        ++seen[perm[k]];
    }
    for (int i = 0; i < n; ++i) if (seen[i] != 1) ++bad;                       // every robot exactly once
    if (!bad)
        for (int k = 0; k + 1 < n; ++k) {
            const float a = dispatch_key(cost[perm[k]], len), b = dispatch_key(cost[perm[k + 1]], len);
            if (!(a >= 0.f) || !std::isfinite(a)) ++bad;                       // finite, non-negative keys
            if (!(a >= b)) ++bad;                                              // non-increasing in key
            if (a == b && !(perm[k] < perm[k + 1])) ++bad;                     // ties by list index
        }
    if (!bad && kind == STOPPED)
        for (int i = 0; i < n; ++i) if (cost[i].left == 0 && dispatch_key(cost[i], len) != 0.f) ++bad;      // a stopped robot has key 0
    if (!bad && kind == ALL_ZERO)
        for (int k = 0; k < n; ++k) if (perm[k] != k) ++bad;                   // nothing to tell the robots apart: the list order
    if (bad) std::printf("order_check: %s, n = %d, len = %d, seed %u: %d violations\n", table_names[kind], n, len, seed, bad);
    return bad;
}

}  // namespace

int main()
{
    const int lengths[] = {1, 63, 64, 65, 70, 512, 800, 4096};
    const int lens[] = {0, 1, 20, 128, 1024, 200000};
    int bad = 0, cases = 0;
    for (int n : lengths)
        for (int kind = RANDOM; kind <= GARBAGE; ++kind)
            for (int len : lens) { bad += check((Table)kind, n, len, 1000u * (unsigned)n + 10u * (unsigned)kind + (unsigned)(len % 7)); ++cases; }
    // the key itself: the launch length is capped by the steps left, a run is charged only when one is predicted within the launch
    DispatchCost c = {1000.f, 4000.f, 0.5f, 0.01f, 30, 0};
    if (dispatch_key(c, 20) != 20000.f) { ++bad; std::printf("order_check: key without a predicted run\n"); }
    if (dispatch_key(c, 100) != 30000.f) { ++bad; std::printf("order_check: key capped by the steps left\n"); }
    c.left = 1000;
    if (dispatch_key(c, 60) != 64000.f) { ++bad; std::printf("order_check: key with one predicted run\n"); }
    if (dispatch_key(c, 260) != 260000.f + 3 * 4000.f) { ++bad; std::printf("order_check: key with three predicted runs\n"); }
    c.left = 0;
    if (dispatch_key(c, 60) != 0.f) { ++bad; std::printf("order_check: key of a stopped robot\n"); }
    std::printf("order_check: %d tables, %s\n", cases, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
