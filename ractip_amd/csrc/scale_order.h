// scale_order.h -- the order in which the scale-exponent ladders try the exponents of the scaled linear path.  Plain C++ (no HIP):
// tools/exponent_order_check.cpp calls it on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

namespace rh::host {

// The models to try after a pass on model `start` left something outside the double range: the larger exponents in ascending
// order (for what overflowed), then the smaller ones in descending order (for what vanished).  A model is an index into
// rungs[0..n_rungs), or -1 for the default exponent; `start` itself is not in the list.  *n_larger: how many of them are larger.
inline std::vector<int> exponent_order(int start, double s_default, const double* rungs, int n_rungs, size_t* n_larger = nullptr)
{
    std::vector<std::pair<double, int>> all = {{s_default, -1}};
    for (int r = 0; r < n_rungs; r++) all.push_back({rungs[r], r});
    std::sort(all.begin(), all.end());
    const double s0 = start < 0 ? s_default : rungs[start];
    std::vector<int> order;
    for (const auto& e : all) if (e.first > s0 + 1e-12) order.push_back(e.second);
    if (n_larger) *n_larger = order.size();
    for (auto it = all.rbegin(); it != all.rend(); ++it) if (it->first < s0 - 1e-12) order.push_back(it->second);
    return order;
}

}  // namespace rh::host
