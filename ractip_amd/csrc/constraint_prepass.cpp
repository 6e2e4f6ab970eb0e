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

static const int T[5][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 5}, {0, 0, 0, 1, 0}, {0, 0, 2, 0, 3}, {0, 6, 0, 4, 0}};   // pair types of the letter codes
static const char* const kNonComplementary = "a forced pair of non-complementary letters (pair type 7) is not supported";

bool constraint_prepass(const char* seq, int n, const char* cons, uint8_t* ch, int* P, int* enc, std::string* why)
{
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
                *why = kNonComplementary;
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

// The walk of constraint_prepass over one share.  A first share's walk IS the joint string's over 1..n1 (what it leaves on the stack
// is open); in a second share a ')' that finds the share's own stack empty is open: in the joint string it pops s1's stack.
bool share_prepass(const char* seq, int n, const char* share, int role, uint8_t* ch, int* P, int* enc, std::vector<int>* open, std::string* why)
{
    const size_t clen = share ? std::strlen(share) : 0;
    std::vector<int> stack;   // brackets opened in this share, innermost last
    int closes = 0;           // second share: open ')' so far
    for (int j = 1; j <= n; j++) {
        const char c = (size_t)(j - 1) < clen ? share[j - 1] : '.';
        ch[j] = (uint8_t)c;
        P[j] = 0;
        if (c == ')' && stack.empty()) {
            if (role == 0) { *why = "unbalanced ')' in the structure constraint (left open in the first share)"; return false; }
            open->push_back(j);
            P[j] = -(++closes);
        } else if (c == ')') {
            const int i = stack.back();
            stack.pop_back();
            if (!T[vienna_code(seq[i - 1])][vienna_code(seq[j - 1])]) { *why = kNonComplementary; return false; }
            P[i] = j; P[j] = i;
        }
        enc[j] = !stack.empty() ? stack.back() : role == 0 ? 0 : -(closes + 1);
        if (c == '(') stack.push_back(j);
    }
    if (role == 0) {
        for (size_t k = 0; k < stack.size(); k++) { P[stack[k]] = -(int)(k + 1); open->push_back(stack[k]); }   // (pushed left to right: ascending)
        return true;
    }
    if (!stack.empty()) { *why = "unbalanced '(' in the structure constraint (left open in the second share)"; return false; }
    for (int j = 1; j <= n; j++)
        if (enc[j] == -(closes + 1)) enc[j] = 0;   // no open ')' to the right: nothing of s1 encloses j either
    return true;
}

bool joint_pair_check(const char* s1, const int* open1, int m1, const char* s2, const int* open2, int m2, std::string* why)
{
    if (m1 != m2) {
        *why = std::string(m1 > m2 ? "unbalanced '('" : "unbalanced ')'") + " in the structure constraint (" + std::to_string(m1) +
               " open in the first share, " + std::to_string(m2) + " in the second)";
        return false;
    }
    for (int k = 0; k < m1; k++)
        if (!T[vienna_code(s1[open1[k] - 1])][vienna_code(s2[open2[m1 - 1 - k] - 1])]) { *why = kNonComplementary; return false; }
    return true;
}

}  // namespace rh::host
