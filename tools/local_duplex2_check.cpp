// local_duplex2_check.cpp -- stand-alone host check of the arguments, shapes, tile sizes and tile walk of local hybridization of two
// windowed molecules (rh_local_duplex2; ractip_amd/csrc/local_windows.{h,cpp}).  No GPU, no HIP; meant to be built with the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc tools/local_duplex2_check.cpp
//       ractip_amd/csrc/local_windows.cpp -o local_duplex2_check                                                 (one command)
//
//   local_duplex2_check plan N1 N2 W1 S1 W2 S2 [null1 | null2]
//       "ok n1 n2 We1 nw1 We2 nw2 : start1 .. | start2 .." or "err <code> <message>" (nullK: the pointer of sequence K is NULL)
//   local_duplex2_check sizes N1 N2 W1 S1 W2 S2         "hp <doubles> logz <doubles> rowbuf <doubles of one k>"
//   local_duplex2_check tile N1 N2 W1 S1 W2 S2 MODEL    "rows <k> cols <l> fold <bytes> pair <bytes> rowbuf <bytes>"
//       MODEL: contrafold | vienna-duplex | vienna-cofold | vienna20-duplex -- the table counts staging.hip sizes a batch by
//   local_duplex2_check walk N1 N2 W1 S1 W2 S2 MODEL ROWS COLS
//       one line "kA kB lA lB" per tile in the order the scheduler runs them; ROWS COLS = 0 0: the automatic tile of MODEL, otherwise
//       each clipped to nw1 / nw2 as rh_set_local_tile's are at run time
// tests/test_local_duplex2_cpu.py restates the definitions and holds the cases.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "local_windows.h"

using namespace rh;
using namespace rh::host;

static bool tables_of(const std::string& model, LocalTables* T)
{
    const bool vienna = model != "contrafold";
    if (model != "contrafold" && model != "vienna-duplex" && model != "vienna-cofold" && model != "vienna20-duplex") return false;
    T->fold = vienna ? (int)VM_COUNT : (int)T_COUNT;
    T->dx = (int)D_COUNT > (int)V_COUNT ? (int)D_COUNT : (int)V_COUNT;
    T->dxl = !vienna ? (int)DL_COUNT : model == "vienna20-duplex" ? (int)VD_COUNT20 : (int)VD_COUNT;
    T->cofold = model == "vienna-cofold";
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 8) { fprintf(stderr, "usage: local_duplex2_check plan|sizes|tile|walk N1 N2 W1 S1 W2 S2 [null1 | null2 | MODEL [ROWS COLS]]\n"); return 2; }
    const std::string mode = argv[1], extra = argc > 8 ? argv[8] : "";
    const int n1 = std::atoi(argv[2]), n2 = std::atoi(argv[3]), W1 = std::atoi(argv[4]), S1 = std::atoi(argv[5]), W2 = std::atoi(argv[6]),
              S2 = std::atoi(argv[7]);
    // (the check reads nothing of the letters: one letter stands for each molecule, whatever its length)
    const char a[] = "A", b[] = "U";
    LocalDuplex2Plan D;
    std::string why;
    const int rc = local_duplex2_check(extra == "null1" ? nullptr : a, n1, extra == "null2" ? nullptr : b, n2, W1, S1, W2, S2, &D, &why);
    if (rc) { printf("err %d %s\n", rc, why.c_str()); return 0; }
    if (mode == "plan") {
        printf("ok %d %d %d %d %d %d :", D.P1.n, D.P2.n, D.P1.We, D.P1.nw, D.P2.We, D.P2.nw);
        for (int k = 0; k < D.P1.nw; k++) printf(" %d", local_start(D.P1, k));
        printf(" |");
        for (int l = 0; l < D.P2.nw; l++) printf(" %d", local_start(D.P2, l));
        printf("\n");
    } else if (mode == "sizes") {
        printf("hp %zu logz %zu rowbuf %zu\n", local_hp2_size(D), local_hp2_logz_size(D), local_hp2_rowbuf_size(D, 1));
    } else if (mode == "tile" || mode == "walk") {
        LocalTables T;
        if (!tables_of(extra, &T)) return 2;
        int rows = 0, cols = 0;
        local_tile_auto(D, T, &rows, &cols);
        if (mode == "tile") {
            printf("rows %d cols %d fold %zu pair %zu rowbuf %zu\n", rows, cols, local_fold_bytes(D.P1.We > D.P2.We ? D.P1.We : D.P2.We, T),
                   local_pair_bytes(D.P1.We, D.P2.We, T), sizeof(double) * local_hp2_rowbuf_size(D, 1));
            return 0;
        }
        if (argc < 11) return 2;
        const int ask_rows = std::atoi(argv[9]), ask_cols = std::atoi(argv[10]);
        if (ask_rows > 0 && ask_cols > 0) { rows = ask_rows; cols = ask_cols; }
        if (rows > D.P1.nw) rows = D.P1.nw;
        if (cols > D.P2.nw) cols = D.P2.nw;
        LocalTile t;
        for (size_t ti = 0; local_tile_at(D, rows, cols, ti, &t); ti++) printf("%d %d %d %d\n", t.kA, t.kB, t.lA, t.lB);
    } else {
        return 2;
    }
    return 0;
}
