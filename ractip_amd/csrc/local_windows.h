// local_windows.h -- the window arithmetic of local folding (rh_local_fold), host only: no HIP, no context (local_windows.cpp;
// checked on the CPU by tools/local_windows_check.cpp).  The two functions the accumulate and finish kernels of local_fold.hip need
// as well -- the start of a window, the windows that contain a run of letters -- are inline here and compile for both sides.
//
// A sequence of n letters is folded in windows of W letters every S letters, We = min(W, n):
//   n <= W: one window, start 0, n letters;
//   else m = ceil((n - W) / S) windows on the grid 0, S, .., (m-1) S and a last one at n - W, which ends at the last letter: nw = m + 1.
// The starts are distinct and increasing.  A run of len letters from i (0-based) lies in window k iff start(k) <= i and
// i + len <= start(k) + We; the windows that contain a run are consecutive.  With S > 1 a run longer than We - S + 1 letters may lie
// in no window.
#pragma once
#include <cstddef>
#include <string>

#if defined(__HIPCC__)
#define RH_LW_HD __host__ __device__ inline
#else
#define RH_LW_HD inline
#endif

namespace rh::host {

struct LocalPlan {
    int n = 0, W = 0, S = 0;   // as asked for
    int We = 0;                // letters per window = min(W, n)
    int nw = 0;                // windows
    int ld = 0;                // row pitch of the band = We: bp_band[i*ld + d] = bp_loc(i, i+d), column 0 and i + d >= n hold 0
};

// RH_OK with *P filled, or RH_ERR_ARG with the reason in *why; reads nothing of seq but whether it is NULL
int local_check(const char* seq, int n, int window, int step, LocalPlan* P, std::string* why);
// doubles of the band and of up, as size_t (n = 1e6, W = 1000: 1e9 doubles)
inline size_t local_band_size(const LocalPlan& P) { return (size_t)P.n * (size_t)P.ld; }
inline size_t local_up_size(const LocalPlan& P, int max_w) { return (size_t)P.n * (size_t)max_w; }

RH_LW_HD int local_start(const LocalPlan& P, int k) { return k + 1 < P.nw ? k * P.S : P.n - P.We; }

// the windows lo..hi that contain letters i .. i+len-1 (lo > hi: none does)
RH_LW_HD void local_window_range(const LocalPlan& P, int i, int len, int* lo, int* hi)
{
    const int m = P.nw - 1;                        // windows on the grid; window m starts at n - We
    const int a = i + len - P.We, last = P.n - P.We;   // a start s contains the run iff a <= s <= i
    int l = a > 0 ? (a + P.S - 1) / P.S : 0, h = i / P.S;
    if (h > m - 1) h = m - 1;
    if (len >= 1 && i >= 0 && a <= last && last <= i) {   // the last window does: behind the grid windows that do, or alone
        if (l > h) l = m;
        h = m;
    }
    *lo = l; *hi = h;
}

}  // namespace rh::host
