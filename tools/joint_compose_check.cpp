// joint_compose_check.cpp -- stand-alone host check of joint constraints built from shares (ractip_amd/csrc/constraint_prepass.h:
// share_prepass, joint_pair_check, compose_joint_letter -- what rh_batch_upload_indexed_constrained stages and the kernel
// joint_cons_gather evaluates) against constraint_prepass on the materialised joint string pad(share1, n1) + pad(share2, n2).
// No GPU, no HIP; may be built with the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc \
//       tools/joint_compose_check.cpp ractip_amd/csrc/constraint_prepass.cpp -o joint_compose_check
//   ./joint_compose_check [S1 SHARE1 S2 SHARE2 ...]
//
// Per case: the shares are accepted iff the joint string is, and then every cell of the (ld x ld) mask that allow_pair gives on the
// composed ch / P / enc equals the one it gives on the joint string's, as do the three arrays themselves.  Checks its built-in
// cases, 4000 random share pairs of 1..40 letters each over "x().<>|" (unbalanced ones and forced pairs of arbitrary letters among
// them) and every quadruple given on the command line; exit status 0 iff all agree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "constraint_prepass.h"

using namespace rh::host;

static int failures = 0, accepted = 0, rejected = 0;

static std::string pad(const std::string& share, int n)
{
    std::string s = share.substr(0, (size_t)n);
    s.append((size_t)n - s.size(), '.');
    return s;
}

struct Share {
    std::vector<uint8_t> ch;
    std::vector<int> P, enc, open;
    explicit Share(int lds) : ch(lds, '.'), P(lds, 0), enc(lds, 0) {}
    ShareRef ref() const { return ShareRef{ch.data(), P.data(), enc.data(), open.data()}; }
};

static void check(const std::string& s1, const std::string& sh1, const std::string& s2, const std::string& sh2)
{
    const int n1 = (int)s1.size(), n2 = (int)s2.size(), n = n1 + n2, ld = (n + 3) & ~1, lds = (n + 3 + 15) & ~15;
    const std::string seq = s1 + s2, joint = pad(sh1, n1) + pad(sh2, n2);
    std::vector<uint8_t> ch(lds, '.');
    std::vector<int> P(lds, 0), enc(lds, 0);
    std::string why, why2;
    const bool want = constraint_prepass(seq.c_str(), n, joint.c_str(), ch.data(), P.data(), enc.data(), &why);
    Share A((n1 + 3 + 15) & ~15), B((n2 + 3 + 15) & ~15);
    const bool ok = share_prepass(s1.c_str(), n1, sh1.c_str(), 0, A.ch.data(), A.P.data(), A.enc.data(), &A.open, &why2) &&
                    share_prepass(s2.c_str(), n2, sh2.c_str(), 1, B.ch.data(), B.P.data(), B.enc.data(), &B.open, &why2) &&
                    joint_pair_check(s1.c_str(), A.open.data(), (int)A.open.size(), s2.c_str(), B.open.data(), (int)B.open.size(), &why2);
    if (ok != want) {
        std::printf("FAIL: '%s' + '%s' on %s + %s: joint string accepted = %d (%s), shares accepted = %d (%s)\n", sh1.c_str(), sh2.c_str(), s1.c_str(),
                    s2.c_str(), want, why.c_str(), ok, why2.c_str());
        failures++;
        return;
    }
    if (!ok) { rejected++; return; }
    accepted++;
    const int m = (int)A.open.size();
    std::vector<uint8_t> jch(lds);
    std::vector<int> jP(lds), jenc(lds);
    for (int j = 0; j < lds; j++) compose_joint_letter(j, n1, n2, m, A.ref(), B.ref(), &jch[j], &jP[j], &jenc[j]);
    for (int j = 0; j < lds; j++)
        if (jch[j] != ch[j] || jP[j] != P[j] || jenc[j] != enc[j]) {
            std::printf("FAIL: '%s' + '%s' letter %d: composed %c %d %d, joint string %c %d %d\n", sh1.c_str(), sh2.c_str(), j, jch[j], jP[j], jenc[j], ch[j],
                        P[j], enc[j]);
            failures++;
            return;
        }
    for (int a = 0; a < ld; a++)
        for (int b = 0; b < ld; b++)
            if (allow_pair(a, b, n, jch.data(), jP.data(), jenc.data()) != allow_pair(a, b, n, ch.data(), P.data(), enc.data())) {
                std::printf("FAIL: '%s' + '%s' cell (%d, %d)\n", sh1.c_str(), sh2.c_str(), a, b);
                failures++;
                return;
            }
}

// letters under which every bracket pair of the joint string is G-C
static void complementary(const std::string& sh1, int n1, const std::string& sh2, int n2, std::string* s1, std::string* s2)
{
    const std::string joint = pad(sh1, n1) + pad(sh2, n2);
    std::string s((size_t)(n1 + n2), 'A');
    std::vector<int> stack;
    for (int j = 0; j < n1 + n2; j++) {
        if (joint[j] == '(') stack.push_back(j);
        else if (joint[j] == ')' && !stack.empty()) { s[stack.back()] = 'G'; s[j] = 'C'; stack.pop_back(); }
    }
    *s1 = s.substr(0, (size_t)n1);
    *s2 = s.substr((size_t)n1);
}

int main(int argc, char** argv)
{
    int count = 0;
    struct Fixed { const char *a, *b; };
    const Fixed fixed[] = {{"", ""}, {"(", ")"}, {"((", "))"}, {"(.(", ").)"}, {"(.(..).(", ").(..).)"}, {"x(.x", "x.)x"}, {"(<|(.).>(", ")..(x)|)"},
                           {"((.(.).(", ")(.))x)"}, {"(((", ").).)"}, {"(.)", "(.)"}, {"..(..(.(..)..(..", "..)..(..)x.)..)"}, {"<(|", ">)|"}};
    for (const Fixed& f : fixed)
        for (int extra : {0, 1, 5}) {   // the shares as long as their sequences, and shorter
            const int n1 = (int)std::strlen(f.a) + extra, n2 = (int)std::strlen(f.b) + extra;
            if (n1 < 1 || n2 < 1) continue;
            std::string s1, s2;
            complementary(f.a, n1, f.b, n2, &s1, &s2);
            check(s1, f.a, s2, f.b);
            check(s1, std::string(f.a) + "((", s2, std::string(f.b) + "))");   // longer than the sequences: the tails are not read
            count += 2;
        }
    const int acc0 = accepted;
    check("GGA", "((", "CA", ")");      // more open in the first share
    check("GA", "(", "ACC", ".))");     // more open in the second
    check("GAC", "(.)", "C", ")");      // ... none in the first
    check("GAC", ".)", "C", ".");       // a ')' left open in a first share
    check("GA", "(.", "GAC", "(.)");    // the second share closes only its own bracket
    check("GA", "(.", "GAC", "(.");     // a '(' left open in a second share
    check("GA", "(.", "AG", ".)");      // a forced pair G-G across the cut
    check("GAAG", "(..)", "A", ".");    // ... inside a share
    check("A", ".", "GAAG", "(..)");
    count += 9;
    if (accepted != acc0) { std::printf("FAIL: %d of the rejected forms were accepted\n", accepted - acc0); failures++; }
    unsigned long long rng = 88172645463325252ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (int t = 0; t < 4000; t++) {
        const int n1 = 1 + (int)(next() % 40), n2 = 1 + (int)(next() % 40);
        const int len1 = (int)(next() % (n1 + 3)), len2 = (int)(next() % (n2 + 3));
        std::string a, b;
        int open = 0, want = (int)(next() % 4);
        for (int k = 0; k < len1; k++) {   // first share: mostly balanced but for `want` open '('
            const int r = (int)(next() % 12);
            if (r < 3) { a += '('; open++; }
            else if (r < 6 && open > want) { a += ')'; open--; }
            else a += ".x<>|."[next() % 6];
        }
        if (next() % 8) while (open > want && (int)a.size() < n1) { a += ')'; open--; }
        int need = 0, depth = 0;
        for (int k = 0; k < n1 && k < (int)a.size(); k++) need += a[k] == '(' ? 1 : a[k] == ')' ? -1 : 0;   // what the cut share leaves open
        if (next() % 8 == 0) need = (int)(next() % 4);
        for (int k = 0; k < len2; k++) {   // second share: brackets of its own, and `need` open ')'
            const int r = (int)(next() % 12);
            if (r < 2) { b += '('; depth++; }
            else if (r < 4 && depth > 0) { b += ')'; depth--; }
            else if (r < 6 && depth == 0 && need > 0) { b += ')'; need--; }
            else b += ".x<>|."[next() % 6];
        }
        if (next() % 8) {
            while (depth-- > 0) b += ')';
            while (need-- > 0) b += ')';
        }
        std::string s1, s2;
        complementary(a, n1, b, n2, &s1, &s2);
        if (next() % 6 == 0) {   // arbitrary letters where a pair may be forced
            s1[next() % n1] = "ACGU"[next() % 4];
            s2[next() % n2] = "ACGU"[next() % 4];
        }
        check(s1, a, s2, b);
        count++;
    }
    if (accepted < 1500 || rejected < 300) { std::printf("FAIL: the random cases are lopsided\n"); failures++; }
    for (int k = 1; k + 3 < argc; k += 4) { check(argv[k], argv[k + 1], argv[k + 2], argv[k + 3]); count++; }
    if ((argc - 1) % 4) { std::printf("FAIL: arguments come as S1 SHARE1 S2 SHARE2\n"); failures++; }
    std::printf("%d share pairs checked (%d accepted, %d rejected), %d failures\n", count, accepted, rejected, failures);
    return failures ? 1 : 0;
}
