// batch_request_check.cpp -- stand-alone host check of what an upload is checked and sized by: check_batch
// (ractip_amd/csrc/batch_request.cpp) and the layout functions of ractip_amd/csrc/batch.h.  No GPU, no HIP; meant to be built with
// the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc tools/batch_request_check.cpp
//       ractip_amd/csrc/batch_request.cpp ractip_amd/csrc/constraint_prepass.cpp -o batch_request_check        (one command)
//
//   batch_request_check layouts   the table counts, then mc_layout for nmax = 1..200 under both counts and dx_layout / dxl_layout /
//                                 lz_chunks for every (n1max, n2max) of the edge set squared, one line each
//   batch_request_check hairpin   hairpin_length_weights against the expression it stands for, bit for bit, across d = 30
//   batch_request_check check     requests from standard input (format: read_request), one answer line each: "ok <shape>" or
//                                 "err <code> <message>"
// tests/test_batch_request_cpu.py restates the layouts and holds the requests.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "batch.h"
#include "batch_request.h"

using namespace rh;
using namespace rh::host;

static int layouts()
{
    printf("counts T %d VM %d D %d V %d DL %d VD %d VD20 %d\n", (int)T_COUNT, (int)VM_COUNT, (int)D_COUNT, (int)V_COUNT, (int)DL_COUNT, (int)VD_COUNT, (int)VD_COUNT20);
    int unset = 0;   // what a layout function leaves alone is zero: pointers, cut / seeded, the launch powers
    for (int nmax = 1; nmax <= 200; nmax++)
        for (int tables : {(int)T_COUNT, (int)VM_COUNT}) {
            const McBatch B = mc_layout(7, nmax, tables);
            printf("mc %d %d : %d %d %d %d %zu %zu %zu %d %zu\n", nmax, tables, B.ns, B.nmax, B.ld, B.lds, B.tab_stride, B.seq_stride, B.tri_stride, B.nb, B.pk_stride);
            unset += B.seq || B.n || B.tab || B.f5i || B.f5o || B.bp || B.up || B.allow || B.cut || B.xp || B.xs || B.xpo || B.xso || B.rowp || B.pk || B.seeded;
            if (seq_lds(nmax) != B.lds) unset++;
        }
    const int edge[] = {1, 2, 13, 14, 15, 16, 17, 29, 30, 31, 57, 58, 59, 64, 109, 110};
    for (int n1 : edge)
        for (int n2 : edge) {
            const int lds = seq_lds(n1 > n2 ? n1 : n2);
            const DxBatch D = dx_layout(5, n1, n2, lds, (int)V_COUNT);
            const DxLinBatch X = dxl_layout(5, n1, n2, lds, D.ldd, (int)VD_COUNT20);
            printf("dx %d %d : %d %d %d %d %d %zu %zu\n", n1, n2, D.np, D.n1max, D.n2max, D.ldd, D.lds, D.tab_stride, D.pair_stride);
            printf("dxl %d %d : %d %d %d %d %d %d %zu %zu %d\n", n1, n2, X.np, X.n1max, X.n2max, X.lda, X.lds, X.ldd, X.tab_stride, X.pair_stride, lz_chunks(n1, n2));
            unset += D.seq || D.n || D.tab || D.hp || D.logz || X.seq || X.n || X.tab || X.hp || X.hp_stride;
            for (double v : X.pw8) unset += v != 0.0;
        }
    printf("unset %d\n", unset);
    return unset != 0;
}

// the fields of VLinModel (vienna_model.h, which needs HIP) that the weights are made of
struct HairpinModel {
    double E_hairpin[32];
    double s, hairpin30, lxc;
};

static int hairpin()
{
    HairpinModel H;
    for (int d = 0; d < 32; d++) H.E_hairpin[d] = d < 3 ? 0.0 : std::exp(-(3.1 + 0.17 * d));
    H.s = 0.28; H.hairpin30 = -8.3; H.lxc = 1.75;
    int differ = 0, entries = 0;
    for (int count : {5, 40}) {
        std::vector<double> got(count + 1, -1.0);
        hairpin_length_weights(H, count, got.data());
        for (int d = 0; d < count; d++, entries++) {
            const double want = (d <= 30 ? H.E_hairpin[d] : std::exp(H.hairpin30 - H.lxc * std::log(d / 30.0))) * std::exp(-H.s * d);
            differ += std::memcmp(&want, &got[d], sizeof want) != 0;
        }
        differ += got[count] != -1.0;   // nothing behind the count
    }
    printf("entries %d differ %d\n", entries, differ);
    return differ != 0;
}

// One request: lines of words up to "end".
//   model vienna | contrafold          folds / pairs            (with_mc, with_dx)
//   seq LEN LETTERS | seq LEN NULL     one sequence (LEN need not be the string's length)
//   index A B                          one pair of an indexed batch;  "indexed" alone: an indexed batch (of no pair so far)
//   fold K TEXT, joint P TEXT, first K TEXT, second K TEXT      an entry of a constraint array ("" = the empty string);
//   fold / joint / first / second alone: the array is there, its entries NULL so far
struct Request {
    bool vienna = false, with_mc = false, with_dx = false, indexed = false;
    std::vector<std::string> text;
    std::vector<bool> null;
    std::vector<int> lens, first, second;
    std::vector<std::pair<int, std::string>> cons[4];
    bool present[4] = {false, false, false, false};
};

static bool read_request(Request* q)
{
    static const char* const kArrays[4] = {"fold", "joint", "first", "second"};
    std::string line;
    bool any = false;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string w;
        if (!(in >> w)) continue;
        any = true;
        if (w == "end") return true;
        if (w == "model") { in >> w; q->vienna = w == "vienna"; }
        else if (w == "folds") q->with_mc = true;
        else if (w == "pairs") q->with_dx = true;
        else if (w == "indexed") q->indexed = true;
        else if (w == "seq") {
            int n; in >> n >> w;
            q->lens.push_back(n); q->null.push_back(w == "NULL"); q->text.push_back(w);
        } else if (w == "index") {
            int a, b; in >> a >> b;
            q->indexed = true; q->first.push_back(a); q->second.push_back(b);
        } else
            for (int k = 0; k < 4; k++)
                if (w == kArrays[k]) {
                    int at; std::string t;
                    q->present[k] = true;
                    if (in >> at >> t) q->cons[k].push_back({at, t == "\"\"" ? "" : t});
                }
    }
    return any;
}

static void answer(const Request& q)
{
    const int ns = (int)q.lens.size();
    std::vector<const char*> seqs(ns);
    for (int k = 0; k < ns; k++) seqs[k] = q.null[k] ? nullptr : q.text[k].c_str();
    std::vector<const char*> arr[4];
    for (int k = 0; k < 4; k++) {
        arr[k].assign(k == 1 ? ns / 2 + 1 : ns + 1, nullptr);
        for (auto& e : q.cons[k]) arr[k].at(e.first) = e.second.c_str();
    }
    const std::vector<int> none(1, 0);
    BatchRequest r;
    r.ns = ns; r.seqs = seqs.data(); r.lens = q.lens.data();
    r.with_mc = q.with_mc; r.with_dx = q.with_dx;
    if (q.present[0]) r.fold_cons = arr[0].data();
    if (q.present[1]) r.joint_cons = arr[1].data();
    if (q.indexed) { r.npairs = (int)q.first.size(); r.first = q.first.empty() ? none.data() : q.first.data(); r.second = q.second.empty() ? none.data() : q.second.data(); }
    if (q.present[2]) r.share_first = arr[2].data();
    if (q.present[3]) r.share_second = arr[3].data();
    BatchShape S;
    std::string why;
    const int rc = check_batch(r, q.vienna, &S, &why);
    if (rc) { printf("err %d %s\n", rc, why.c_str()); return; }
    printf("ok indexed %d np %d nmax %d n1max %d n2max %d cut_min %d cut_max %d lds %d co_lds %d fold %d joint %d shares %d pair_seq", (int)S.indexed, S.np, S.nmax,
           S.n1max, S.n2max, S.cut_min, S.cut_max, S.lds, S.co_lds, (int)S.has_fold, (int)S.has_joint, (int)S.has_shares);
    for (int v : S.pair_seq) printf(" %d", v);
    printf(" codes ");
    for (size_t k = 0; k < S.codes.size(); k++) printf("%d", (int)S.codes[k]);
    printf(" cells %zu %zu %zu\n", S.fold.ch.size(), S.joint.ch.size(), S.share.L.ch.size());
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "layouts") return layouts();
    if (mode == "hairpin") return hairpin();
    if (mode != "check") { fprintf(stderr, "usage: batch_request_check layouts | hairpin | check < requests\n"); return 2; }
    for (;;) {
        Request q;
        if (!read_request(&q)) break;
        answer(q);
    }
    return 0;
}
