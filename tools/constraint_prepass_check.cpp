// constraint_prepass_check.cpp -- stand-alone host check of the structure-constraint pre-pass (ractip_amd/csrc/constraint_prepass.cpp)
// and of the per-cell rule allow_pair the mask kernel evaluates, against the rectangle-clearing rule of ViennaRNA-1.8 make_ptypes
// restated here.  No GPU, no HIP; meant to be built with the sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc \
//       tools/constraint_prepass_check.cpp ractip_amd/csrc/constraint_prepass.cpp -o constraint_prepass_check
//   ./constraint_prepass_check [CONSTRAINT ...]
//
// Checks its built-in strings (every class character, nesting, siblings, short and empty strings, a 2000-letter line, the three
// rejected forms), 3000 random strings of 1..40 letters and every string given on the command line; exit status 0 iff all agree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "constraint_prepass.h"

using rh::host::allow_pair;
using rh::host::constraint_prepass;

// make_ptypes under fold_constrained, by clearing: M[a*ld + b], 1 <= a < b <= n.  Returns false on unbalanced brackets.
static bool mask_by_clearing(const std::string& cons, int n, int ld, std::vector<uint8_t>& M)
{
    M.assign((size_t)ld * ld, 0);
    for (int a = 1; a <= n; a++)
        for (int b = a + 1; b <= n; b++) M[(size_t)a * ld + b] = 1;
    std::vector<int> stack;
    for (int j = 1; j <= n; j++) {
        const char ch = (size_t)(j - 1) < cons.size() ? cons[j - 1] : '.';
        if (ch == 'x') {
            for (int l = 1; l <= n; l++) M[(size_t)l * ld + j] = M[(size_t)j * ld + l] = 0;
        } else if (ch == '(' || ch == '<') {
            if (ch == '(') stack.push_back(j);
            for (int l = 1; l < j; l++) M[(size_t)l * ld + j] = 0;
        } else if (ch == ')' || ch == '>') {
            if (ch == ')') {
                if (stack.empty()) return false;
                const int i = stack.back();
                stack.pop_back();
                const uint8_t keep = M[(size_t)i * ld + j];
                for (int k = i; k <= j; k++) for (int l = j; l <= n; l++) M[(size_t)k * ld + l] = 0;
                for (int k = 1; k <= i; k++) for (int l = i; l <= j; l++) M[(size_t)k * ld + l] = 0;
                M[(size_t)i * ld + j] = keep;
            }
            for (int l = j + 1; l <= n; l++) M[(size_t)j * ld + l] = 0;
        }
    }
    return stack.empty();
}

// a sequence whose matched brackets are G-C pairs (so that only the constraint's shape decides)
static std::string complementary_sequence(const std::string& cons, int n)
{
    std::string s(n, 'A');
    std::vector<int> stack;
    for (int j = 0; j < n && j < (int)cons.size(); j++) {
        if (cons[j] == '(') stack.push_back(j);
        else if (cons[j] == ')' && !stack.empty()) { s[stack.back()] = 'G'; s[j] = 'C'; stack.pop_back(); }
    }
    return s;
}

static int failures = 0;

static void check(const std::string& seq, const std::string& cons, const char* expect_error = nullptr)
{
    const int n = (int)seq.size(), ld = (n + 3) & ~1, lds = (n + 3 + 15) & ~15;
    std::vector<uint8_t> ch(lds, '.'), M;
    std::vector<int> P(lds, 0), enc(lds, 0);
    std::string why;
    const bool ok = constraint_prepass(seq.c_str(), n, cons.c_str(), ch.data(), P.data(), enc.data(), &why);
    if (expect_error) {
        if (ok || why.find(expect_error) == std::string::npos) {
            std::printf("FAIL: '%s' on '%s' should be rejected with '%s' (got '%s')\n", cons.c_str(), seq.c_str(), expect_error, why.c_str());
            failures++;
        }
        return;
    }
    const bool balanced = mask_by_clearing(cons, n, ld, M);
    if (ok != balanced) { std::printf("FAIL: '%s' accepted = %d, balanced = %d (%s)\n", cons.c_str(), ok, balanced, why.c_str()); failures++; return; }
    if (!ok) return;
    for (int a = 0; a < ld; a++)
        for (int b = 0; b < ld; b++)
            if ((allow_pair(a, b, n, ch.data(), P.data(), enc.data()) ? 1 : 0) != M[(size_t)a * ld + b]) {
                std::printf("FAIL: '%.60s' n = %d cell (%d, %d)\n", cons.c_str(), n, a, b);
                failures++;
                return;
            }
}

int main(int argc, char** argv)
{
    int count = 0;
    const char* fixed[] = {"", ".", "x", "(.)", "((..))", "(((...)))", "((.)(.))", "(.)(.)", "<(..)>", "(<.>)", "|x.<>()", "..((..((..))..((...))..))..",
                           "(((...)))..", "xx<<..>>||", "(..)x<.>(..(.).)", "....................", "((....))..(((...)))."};
    for (const char* c : fixed) {
        for (int extra : {0, 1, 7}) {   // the string as long as the sequence, and shorter
            const int n = (int)std::strlen(c) + extra;
            if (n < 1) continue;
            check(complementary_sequence(c, n), c);
            count++;
        }
    }
    {   // a 2000-letter line: 200 stems of three nested pairs, class characters between them
        std::string line;
        for (int k = 0; k < 200; k++) line += "(((x.)))<|";
        check(complementary_sequence(line, 2000), line);
        check(complementary_sequence(line, 1990), line);   // the string longer than the sequence: its tail is not read
        count += 2;
    }
    check("GGGAAACCC", "(((", "unbalanced '('");
    check("GGGAAACCC", ")", "unbalanced ')'");
    check("GAAG", "(..)", "non-complementary");
    count += 3;
    unsigned long long rng = 88172645463325252ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (int t = 0; t < 3000; t++) {
        const int n = 1 + (int)(next() % 40), len = (int)(next() % (n + 3));
        std::string c;
        int open = 0;
        for (int k = 0; k < len; k++) {   // mostly balanced; the rest is rejected by both sides alike
            const int r = (int)(next() % 12);
            if (r < 3) { c += '('; open++; }
            else if (r < 6 && open > 0) { c += ')'; open--; }
            else c += ".x<>|."[next() % 6];
        }
        if (next() % 8) while (open-- > 0) c += ')';
        check(complementary_sequence(c, n), c);
        count++;
    }
    for (int k = 1; k < argc; k++) {
        const std::string c = argv[k];
        for (int extra : {0, 3}) { check(complementary_sequence(c, (int)c.size() + extra), c); count++; }
    }
    std::printf("%d constraint strings checked, %d failures\n", count, failures);
    return failures ? 1 : 0;
}
