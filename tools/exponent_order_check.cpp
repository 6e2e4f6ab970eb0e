// exponent_order_check.cpp -- stand-alone host program around exponent_order (ractip_amd/csrc/scale_order.h), the order in which the
// scale-exponent ladders try the exponents of the scaled linear path.  No GPU, no HIP; meant to be built with the sanitizers too:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc \
//       tools/exponent_order_check.cpp -o exponent_order_check
//   ./exponent_order_check retry|attempts DEFAULT RUNG0 [RUNG1 ...]
//
// Prints one line per start model (-1 = the default exponent, then every rung): the start, a colon, and the models in order.
// retry: what a pass on the start model tries next (retry_mc_lin_rungs, CONTRAfold model); attempts: the same behind the start
// model itself (compute, Vienna-BL model: the whole batch runs on each).  tests/test_scale_order_cpu.py compares the lines.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scale_order.h"

int main(int argc, char** argv)
{
    if (argc < 4 || (std::strcmp(argv[1], "retry") && std::strcmp(argv[1], "attempts"))) {
        std::fprintf(stderr, "usage: %s retry|attempts DEFAULT RUNG0 [RUNG1 ...]\n", argv[0]);
        return 2;
    }
    const bool attempts = !std::strcmp(argv[1], "attempts");
    const double s_default = std::atof(argv[2]);
    std::vector<double> rungs;
    for (int k = 3; k < argc; k++) rungs.push_back(std::atof(argv[k]));
    for (int start = -1; start < (int)rungs.size(); start++) {
        size_t n_larger = 0;
        const std::vector<int> order = rh::host::exponent_order(start, s_default, rungs.data(), (int)rungs.size(), &n_larger);
        if (n_larger > order.size() || order.size() != rungs.size()) return 1;   // every other model, once
        std::printf("%d:", start);
        if (attempts) std::printf(" %d", start);
        for (int model : order) std::printf(" %d", model);
        std::printf("\n");
    }
    return 0;
}
