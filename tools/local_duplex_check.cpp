// local_duplex_check.cpp -- stand-alone host check of the arguments, shapes and chunk sizes of local hybridization (rh_local_duplex;
// ractip_amd/csrc/local_windows.{h,cpp}).  No GPU, no HIP; meant to be built with the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc tools/local_duplex_check.cpp
//       ractip_amd/csrc/local_windows.cpp -o local_duplex_check                                                  (one command)
//
//   local_duplex_check plan N1 N2 WINDOWED W S [null1 | null2]
//       "ok n1 n2 windowed nq We nw n1max n2max : start ..." or "err <code> <message>" (nullK: the pointer of sequence K is NULL)
//   local_duplex_check sizes N1 N2 WINDOWED W S        "hp <doubles> logz <doubles>"
//   local_duplex_check chunk N1 N2 WINDOWED W S MODEL  "chunk <windows> fold <bytes> pair <bytes> fold_only <windows>"
//       MODEL: contrafold | vienna-duplex | vienna-cofold | vienna20-duplex -- the table counts staging.hip sizes a batch by
// tests/test_local_duplex_cpu.py restates the definitions and holds the cases.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "local_windows.h"

using namespace rh;
using namespace rh::host;

int main(int argc, char** argv)
{
    if (argc < 7) { fprintf(stderr, "usage: local_duplex_check plan|sizes|chunk N1 N2 WINDOWED W S [null1 | null2 | MODEL]\n"); return 2; }
    const std::string mode = argv[1], extra = argc > 7 ? argv[7] : "";
    const int n1 = std::atoi(argv[2]), n2 = std::atoi(argv[3]), windowed = std::atoi(argv[4]), W = std::atoi(argv[5]), S = std::atoi(argv[6]);
    const std::vector<char> a(n1 > 0 ? (size_t)n1 : 1, 'A'), b(n2 > 0 ? (size_t)n2 : 1, 'U');
    LocalDuplexPlan D;
    std::string why;
    const int rc = local_duplex_check(extra == "null1" ? nullptr : a.data(), n1, extra == "null2" ? nullptr : b.data(), n2, windowed, W, S, &D, &why);
    if (rc) { printf("err %d %s\n", rc, why.c_str()); return 0; }
    if (mode == "plan") {
        printf("ok %d %d %d %d %d %d %d %d :", D.n1, D.n2, D.windowed, D.nq, D.P.We, D.P.nw, local_n1max(D), local_n2max(D));
        for (int k = 0; k < D.P.nw; k++) printf(" %d", local_start(D.P, k));
        printf("\n");
    } else if (mode == "sizes") {
        printf("hp %zu logz %zu\n", local_hp_size(D), (size_t)D.P.nw);
    } else if (mode == "chunk") {
        LocalTables T;
        const bool vienna = extra != "contrafold";
        if (extra != "contrafold" && extra != "vienna-duplex" && extra != "vienna-cofold" && extra != "vienna20-duplex") return 2;
        T.fold = vienna ? (int)VM_COUNT : (int)T_COUNT;
        T.dx = (int)D_COUNT > (int)V_COUNT ? (int)D_COUNT : (int)V_COUNT;
        T.dxl = !vienna ? (int)DL_COUNT : extra == "vienna20-duplex" ? (int)VD_COUNT20 : (int)VD_COUNT;
        T.cofold = extra == "vienna-cofold";
        const int nmax = D.nq > D.P.We ? D.nq : D.P.We;
        printf("chunk %d fold %zu pair %zu fold_only %d\n", local_duplex_chunk_auto(D, T), local_fold_bytes(nmax, T),
               local_pair_bytes(local_n1max(D), local_n2max(D), T), local_chunk_auto(D.P, T));
    } else {
        return 2;
    }
    return 0;
}
