// adapter_timing.cpp -- pairs per second of ProbabilityEngine::solve_probabilities (ractip_amd/host/ractip_prob.hpp), the member a
// stock RactIP's z-score loop calls: upload, compute, dense fetch and the unpacking into VF / VVF, per call.
//   adapter_timing [pairs=256] [n=500] [rounds=7]
// The sequences are those of ractip_amd/seqgen.py (std::mt19937 g(12345), "ACGU"[g() & 3], s1 drawn before s2).  The first call
// allocates tables and buffers and is not counted; prints the median of the rounds and a checksum of the floats.
//   g++ -O2 -std=c++17 -I ractip_amd/host tools/adapter_timing.cpp -L ractip_amd/host -lractip_prob -L ractip_amd -lractip_hot \
//       -Wl,-rpath,$PWD/ractip_amd/host -Wl,-rpath,$PWD/ractip_amd -pthread -o adapter_timing
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "ractip_prob.hpp"

using namespace ractip_amd;

int main(int argc, char** argv)
{
    const int pairs = argc > 1 ? std::atoi(argv[1]) : 256, n = argc > 2 ? std::atoi(argv[2]) : 500, rounds = argc > 3 ? std::atoi(argv[3]) : 7;
    try {
        std::mt19937 g(12345);
        std::vector<std::pair<std::string, std::string>> batch(pairs);
        for (auto& pr : batch) {
            for (int i = 0; i < n; i++) pr.first += "ACGU"[g() & 3];
            for (int i = 0; i < n; i++) pr.second += "ACGU"[g() & 3];
        }
        ProbabilityEngine en(0);
        std::vector<double> ms;
        double sum = 0.0;
        for (int r = 0; r <= rounds; r++) {
            const auto t0 = std::chrono::steady_clock::now();
            const std::vector<PairProbabilities> out = en.solve_probabilities(batch);
            const auto t1 = std::chrono::steady_clock::now();
            if (r) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
            if (r == rounds) {
                for (const PairProbabilities& p : out) {
                    for (float v : p.bp1) sum += v;
                    for (const VF& row : p.up2) sum += row[0];
                    for (const VF& row : p.hp) for (float v : row) sum += v;
                }
            }
        }
        std::sort(ms.begin(), ms.end());
        const double med = ms[ms.size() / 2];
        std::printf("{\"pairs\": %d, \"n\": %d, \"rounds\": %d, \"median_ms\": %.2f, \"min_ms\": %.2f, \"max_ms\": %.2f, \"pairs_per_s\": %.0f, \"checksum\": %.9g}\n",
                    pairs, n, rounds, med, ms.front(), ms.back(), pairs * 1e3 / med, sum);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
