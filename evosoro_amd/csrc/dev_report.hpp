// What the developer switches print on stderr, as functions of plain data: engine.hip downloads the words and calls them.
// scripts/dev_gpu_diag.py and scripts/tile_timeline_sum.py parse the text.
#pragma once
#include <cstddef>
#include <vector>

#include "dispatch_order.hpp"

namespace vxh {

// VXH_PROF_ORDER=1: the spread of the robots' cost in the last long launch of launch group `group` (`count` robots: their cost words, and
// the order `perm` they were dispatched in), and what that order made of it on n_cu compute units
void report_dispatch_cost(size_t group, const std::vector<DispatchCost>& cost, const std::vector<int>& perm, int block, size_t lds, long long last_len,
                          bool last_ordered, int n_cu, double us_per_tick);
// developer library, VXH_COL_STATS=1: lengths of the contact rows (DBatch::col_cnt); robot r owns rows [surf_begin[r], surf_begin[r] + nsurf[r])
void report_contact_rows(const std::vector<int>& cnt, const std::vector<int>& surf_begin, const std::vector<int>& nsurf);
// developer library: the VXH_PROF_WORDS counters of DBatch::prof (ProfSlot, device_types.hpp)
void report_phase_counters(const unsigned long long* h, int n_tiles, bool tiled);

}  // namespace vxh
