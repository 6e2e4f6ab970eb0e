// constraint_prepass.h -- the O(n) host pass over one structure-constraint string (constraint_prepass.cpp, host only: no HIP).
//
// Allowed-pair mask of pf_fold under fold_constrained (ViennaRNA 1.8 make_ptypes), letters 1 <= a < b <= n:
//   'x' the letter never pairs; '<' it pairs only with a later letter, '>' only with an earlier one; a matched '(' ')'
//   is kept and every pair inconsistent with it (crossing it, or sharing a letter) is removed; '|' and '.' do not
//   restrict the partition function.
// The pass leaves three values per letter, from which allow_mask_build (allow_mask.hip) writes every cell on its own:
//   ch[k]   the constraint character ('.' beyond the string's end)
//   P[k]    the forced partner of a matched bracket, 0 if none
//   enc[k]  the opening letter of the innermost matched bracket pair that strictly encloses k, 0 if none
// allow_pair below is the one statement of the rule: the kernel evaluates it per byte.
#pragma once
#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define RH_HOST_DEVICE __host__ __device__
#else
#define RH_HOST_DEVICE
#endif

namespace rh::host {

// May letters a and b pair?  a, b index the three arrays (0 .. their length - 1); n = the sequence's length.
RH_HOST_DEVICE inline bool allow_pair(int a, int b, int n, const uint8_t* ch, const int* P, const int* enc)
{
    if (a < 1 || b <= a || b > n) return false;
    const uint8_t ca = ch[a], cb = ch[b];
    if (ca == 'x' || ca == ')' || ca == '>') return false;   // a does not pair downstream
    if (cb == 'x' || cb == '(' || cb == '<') return false;   // b does not pair upstream
    return P[a] == b || (P[a] == 0 && P[b] == 0 && enc[a] == enc[b]);   // the forced pair itself, or two free letters of one loop
}

uint8_t nuc_code(char ch);      // CONTRAfold model: A,C,G,U -> 0..3 in either case, anything else (T and N included) 4; host only, here so that a CPU program can call it
uint8_t vienna_code(char ch);   // ViennaRNA encode_char with energy_set 0: A,C,G,U -> 1..4 (T reads as U), anything else 0

// Fills ch / P / enc at 1..n (the caller presets '.' / 0 / 0 everywhere else).  cons may be shorter or longer than n.
// Returns false for unbalanced brackets or a forced pair of non-complementary letters, with the reason in *why.
bool constraint_prepass(const char* seq, int n, const char* cons, uint8_t* ch, int* P, int* enc, std::string* why);

}  // namespace rh::host
