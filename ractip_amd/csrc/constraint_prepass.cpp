// constraint_prepass.cpp -- see constraint_prepass.h.  Host only: one stack walk per constraint string, all of its validation.
#include "constraint_prepass.h"

#include <cstring>
#include <vector>

namespace rh::host {

uint8_t nuc_code(char ch)
{  // InferenceEngine.ipp:379-384: case-insensitive ACGU, anything else (incl. T, N) is code 4
    switch (ch) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'U': case 'u': return 3;
        default: return 4;
    }
}

uint8_t vienna_code(char ch)
{
    switch (ch) {
        case 'A': case 'a': return 1;
        case 'C': case 'c': return 2;
        case 'G': case 'g': return 3;
        case 'U': case 'u': case 'T': case 't': return 4;
        default: return 0;
    }
}

bool constraint_prepass(const char* seq, int n, const char* cons, uint8_t* ch, int* P, int* enc, std::string* why)
{
    static const int T[5][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 5}, {0, 0, 0, 1, 0}, {0, 0, 2, 0, 3}, {0, 6, 0, 4, 0}};   // pair types of the letter codes
    const size_t clen = cons ? std::strlen(cons) : 0;
    std::vector<int> stack;   // open brackets, innermost last
    for (int j = 1; j <= n; j++) {
        const char c = (size_t)(j - 1) < clen ? cons[j - 1] : '.';
        ch[j] = (uint8_t)c;
        P[j] = 0;
        if (c == ')') {
            if (stack.empty()) { *why = "unbalanced ')' in the structure constraint"; return false; }
            const int i = stack.back();
            stack.pop_back();
            if (!T[vienna_code(seq[i - 1])][vienna_code(seq[j - 1])]) {
                *why = "a forced pair of non-complementary letters (pair type 7) is not supported";
                return false;
            }
            P[i] = j; P[j] = i;
        }
        enc[j] = stack.empty() ? 0 : stack.back();   // ('(' : before it is pushed; ')' : after its partner is popped)
        if (c == '(') stack.push_back(j);
    }
    if (!stack.empty()) { *why = "unbalanced '(' in the structure constraint"; return false; }
    return true;
}

}  // namespace rh::host
