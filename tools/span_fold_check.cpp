// span_fold_check.cpp -- stand-alone host program around the plan and the exterior recurrence of span-limited folding
// (ractip_amd/csrc/span_fold.{h,cpp}; the kernels are in mccaskill_span.hip).  No GPU, no HIP; meant to be built with the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc tools/span_fold_check.cpp \
//       ractip_amd/csrc/span_fold.cpp -o span_fold_check
//
//   span_fold_check plan N L [null]    "ok n L Le ldn table tables band ext" or "err CODE TEXT" as span_check answers
//   span_fold_check acc N L MAX_W      "ok n L max_w up gaps" (the sizes of the accessibility stage, span_acc_check) or "err CODE TEXT"
//   span_fold_check exterior N L       both exterior passes on the CPU in the kernel's order (span_ext_pass_host: blocks of 64 entries, lane
//                                      by lane, the butterfly) over a synthetic FCA band whose free energy is front-loaded: the first quarter
//                                      of the letters carries 3.5 nats each, the rest 0.01.  Compared with a long-double recurrence in
//                                      log space over the same stored cells.  Prints "logz Z ref R dz E gi E go E"; exit status 0
//                                      only if log Z > 3000 and every difference is at most 1e-9.
// tests/test_span_fold_cpu.py runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "span_fold.h"

using namespace rh::host;

namespace {

int plan(int n, int L, bool null)
{
    SpanPlan P;
    std::string why;
    const std::string seq((size_t)(n > 0 && n < 100 ? n : 1), 'A');   // span_check reads nothing of it
    const int rc = span_check(null ? nullptr : seq.c_str(), n, L, &P, &why);
    if (rc) { std::printf("err %d %s\n", rc, why.c_str()); return 0; }
    std::printf("ok %d %d %d %zu %zu %zu %zu %zu\n", P.n, P.L, P.Le, P.ldn, P.table, P.tables, P.band, P.ext);
    return 0;
}

int acc(int n, int L, int max_w)
{
    SpanPlan P;
    SpanAccPlan A;
    std::string why;
    const std::string seq(1, 'A');
    int rc = span_check(seq.c_str(), n, L, &P, &why);
    if (!rc) rc = span_acc_check(P, max_w, &A, &why);
    if (rc) { std::printf("err %d %s\n", rc, why.c_str()); return 0; }
    std::printf("ok %d %d %d %zu %zu\n", P.n, P.L, A.max_w, A.up, A.gaps);
    return 0;
}

long double logaddl(long double x, long double y)
{
    if (x == -INFINITY) return y;
    if (y == -INFINITY) return x;
    return x > y ? x + log1pl(expl(y - x)) : y + log1pl(expl(x - y));
}

int exterior(int n, int L)
{
    SpanPlan P;
    std::string why;
    const std::string seq(1, 'A');
    if (span_check(seq.c_str(), n, L, &P, &why)) { std::printf("err %s\n", why.c_str()); return 2; }
    const int Le = P.Le;
    const double s = 0.28;
    // FCA~[d * ldn + i]: pair (i, i+d+1), d >= 3 and d + 1 < L; every third cell does not exist (0)
    std::vector<double> fca(P.table, 0.0);
    for (int d = 3; d < Le && d + 1 < L; d++)
        for (int i = 1; i <= n - 1 - d; i++) {
            const double x = ((double)d * 2003.0 + i) * 0.6180339887498949, u = x - std::floor(x);
            if (((size_t)d * 5 + i) % 3 == 0) continue;   // (5 d + i = 4 d + j - 1: the holes differ from entry to entry)
            const double rate = i < n / 4 ? 3.5 : 0.01;
            fca[(size_t)d * P.ldn + i] = std::exp(std::log(0.5 + u) + rate * (d + 2) - 8.0 - s * d);
        }
    std::vector<double> gi((size_t)n + 1, 0.0), go((size_t)n + 1, 0.0);
    const auto cell = [&](int d, int col) { return fca[(size_t)d * P.ldn + col]; };
    span_ext_pass_host(0, n, Le, s, gi.data(), cell);
    span_ext_pass_host(1, n, Le, s, go.data(), cell);
    // the reference: the same sums in log space, long double, one term after the other
    std::vector<long double> ri((size_t)n + 1, 0.0L), ro((size_t)n + 1, 0.0L);
    for (int j = 1; j <= n; j++) {
        long double acc = ri[j - 1];
        for (int d = 0; d < Le && d <= j - 2; d++) {
            const double f = fca[(size_t)d * P.ldn + (j - 1 - d)];
            if (f != 0.0) acc = logaddl(acc, ri[j - 2 - d] + logl((long double)f) + (long double)s * d);
        }
        ri[j] = acc;
    }
    for (int k = n - 1; k >= 0; k--) {
        long double acc = ro[k + 1];
        for (int d = 0; d < Le && d <= n - k - 2; d++) {
            const double f = fca[(size_t)d * P.ldn + (k + 1)];
            if (f != 0.0) acc = logaddl(acc, ro[k + 2 + d] + logl((long double)f) + (long double)s * d);
        }
        ro[k] = acc;
    }
    double ei = 0.0, eo = 0.0;
    for (int j = 0; j <= n; j++) {
        ei = std::fmax(ei, (double)fabsl(ri[j] - (long double)gi[j]));
        eo = std::fmax(eo, (double)fabsl(ro[j] - (long double)go[j]));
    }
    const double dz = (double)fabsl(ri[n] - (long double)gi[n]), dio = std::fabs(gi[n] - go[0]);
    std::printf("logz %.12f ref %.12Lf dz %.3e gi %.3e go %.3e inout %.3e\n", gi[n], ri[n], dz, ei, eo, dio);
    const bool ok = gi[n] > 3000.0 && dz <= 1e-9 && ei <= 1e-9 && eo <= 1e-9 && dio <= 1e-9;
    return ok ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc >= 4 && !std::strcmp(argv[1], "plan")) return plan(std::atoi(argv[2]), std::atoi(argv[3]), argc >= 5 && !std::strcmp(argv[4], "null"));
    if (argc >= 4 && !std::strcmp(argv[1], "exterior")) return exterior(std::atoi(argv[2]), std::atoi(argv[3]));
    if (argc >= 5 && !std::strcmp(argv[1], "acc")) return acc(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
    std::fprintf(stderr, "usage: span_fold_check plan N L [null] | exterior N L | acc N L MAX_W\n");
    return 2;
}
