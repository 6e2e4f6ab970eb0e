// local_windows_check.cpp -- stand-alone host check of the window arithmetic of local folding (ractip_amd/csrc/local_windows.{h,cpp}):
// the argument checks, the starts, the windows that contain a run, the sizes of the band, the chunks of a walk over one molecule.  No GPU, no HIP; meant to be built with
// the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc tools/local_windows_check.cpp
//       ractip_amd/csrc/local_windows.cpp -o local_windows_check                                                 (one command)
//
//   local_windows_check plan N W S [null]   "ok We nw ld : start ..." or "err <code> <message>" (null: the sequence pointer is NULL)
//   local_windows_check ranges N W S        one line "i len lo hi" for every i = 0..N-1 and len = 1..N-i+1 (the last one runs past the end)
//   local_windows_check sizes N W S MAXW    "band <doubles> up <doubles>"
//   local_windows_check chunks N W S CHUNK  one line "kA kB lA lB" per tile of the walk without a second molecule (local_tile_at with
//                                           P2.nw = 0, cols = 0), CHUNK clipped to the window count as the scheduler clips it
// tests/test_local_windows_cpu.py restates the definition and holds the cases.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "local_windows.h"

using namespace rh::host;

int main(int argc, char** argv)
{
    if (argc < 5) { fprintf(stderr, "usage: local_windows_check plan|ranges|sizes|chunks N W S [null | MAXW | CHUNK]\n"); return 2; }
    const std::string mode = argv[1];
    const int n = std::atoi(argv[2]), W = std::atoi(argv[3]), S = std::atoi(argv[4]);
    const bool null_seq = argc > 5 && !std::strcmp(argv[5], "null");
    const std::vector<char> letters(n > 0 ? (size_t)n : 1, 'A');
    LocalPlan P;
    std::string why;
    const int rc = local_check(null_seq ? nullptr : letters.data(), n, W, S, &P, &why);
    if (rc) { printf("err %d %s\n", rc, why.c_str()); return 0; }
    if (mode == "plan") {
        printf("ok %d %d %d :", P.We, P.nw, P.ld);
        for (int k = 0; k < P.nw; k++) printf(" %d", local_start(P, k));
        printf("\n");
    } else if (mode == "ranges") {
        for (int i = 0; i < n; i++)
            for (int len = 1; len <= n - i + 1; len++) {
                int lo, hi;
                local_window_range(P, i, len, &lo, &hi);
                printf("%d %d %d %d\n", i, len, lo, hi);
            }
    } else if (mode == "sizes") {
        printf("band %zu up %zu\n", local_band_size(P), local_up_size(P, argc > 5 ? std::atoi(argv[5]) : 1));
    } else if (mode == "chunks") {
        if (argc < 6) return 2;
        LocalDuplex2Plan D;
        D.P1 = P;
        const int chunk = std::atoi(argv[5]) < P.nw ? std::atoi(argv[5]) : P.nw;
        LocalTile t;
        for (size_t ti = 0; local_tile_at(D, chunk, 0, ti, &t); ti++) printf("%d %d %d %d\n", t.kA, t.kB, t.lA, t.lB);
    } else {
        return 2;
    }
    return 0;
}
