// local_windows.cpp -- the argument checks of rh_local_fold and the shape they give (local_windows.h).  Host only: no HIP, no context.
#include "local_windows.h"

#include "../../include/ractip_hot.h"

namespace rh::host {

static int reject(std::string* why, const std::string& text) { *why = text; return RH_ERR_ARG; }

int local_check(const char* seq, int n, int window, int step, LocalPlan* P, std::string* why)
{
    if (!seq) return reject(why, "local fold: the sequence is NULL");
    if (n < 1) return reject(why, "local fold: the sequence has length " + std::to_string(n) + " (must be >= 1)");
    if (window < 2) return reject(why, "local fold: window " + std::to_string(window) + " (must be >= 2)");
    if (step < 1) return reject(why, "local fold: step " + std::to_string(step) + " (must be >= 1)");
    if (step > window) return reject(why, "local fold: step " + std::to_string(step) + " exceeds the window " + std::to_string(window));
    *P = LocalPlan();
    P->n = n; P->W = window; P->S = step;
    P->We = n < window ? n : window;
    P->nw = n <= window ? 1 : (n - window + step - 1) / step + 1;
    P->ld = P->We;
    return RH_OK;
}

}  // namespace rh::host
