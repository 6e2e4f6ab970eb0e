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
// allow_pair_values below is the one statement of the rule; allow_pair reads it off the three arrays (the mask kernel evaluates it per
// byte), allow_pair_rec off two packed records (the span kernels, which have no mask).
// Second half of this file: the same three values for a joint string that is given as two shares (indexed batches).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define RH_HOST_DEVICE __host__ __device__
#else
#define RH_HOST_DEVICE
#endif

namespace rh::host {

// The two facts the rule takes from a constraint character
RH_HOST_DEVICE inline bool cons_no_downstream(uint8_t c) { return c == 'x' || c == ')' || c == '>'; }   // the letter pairs with no later letter
RH_HOST_DEVICE inline bool cons_no_upstream(uint8_t c) { return c == 'x' || c == '(' || c == '<'; }     // ... with no earlier letter

// The rule on the values of the two letters alone: a_down = cons_no_downstream(ch[a]), b_up = cons_no_upstream(ch[b]), P and enc of both.
RH_HOST_DEVICE inline bool allow_pair_values(int a, int b, int n, bool a_down, bool b_up, int Pa, int Pb, int enca, int encb)
{
    if (a < 1 || b <= a || b > n) return false;
    if (a_down || b_up) return false;
    return Pa == b || (Pa == 0 && Pb == 0 && enca == encb);   // the forced pair itself, or two free letters of one loop
}

// May letters a and b pair?  a, b index the three arrays (0 .. their length - 1); n = the sequence's length.
RH_HOST_DEVICE inline bool allow_pair(int a, int b, int n, const uint8_t* ch, const int* P, const int* enc)
{
    if (a < 1 || b <= a || b > n) return false;   // (before the arrays are read)
    return allow_pair_values(a, b, n, cons_no_downstream(ch[a]), cons_no_upstream(ch[b]), P[a], P[b], enc[a], enc[b]);
}

// ---- per-letter records: ch / P / enc of one letter in 8 bytes, for the kernels that cannot afford the n x n byte mask (span folds
// under a constraint, mccaskill_span.hip).  A pair test is two records and allow_pair_values.  P and enc are letters of the sequence,
// below 2^30 (span_cons_records, span_fold.h, refuses longer ones), so the two facts of ch sit beside P.
struct alignas(8) ConsRec {
    uint32_t p;   // P | kConsRecDown | kConsRecUp
    uint32_t e;   // enc
};
static_assert(sizeof(ConsRec) == 8);
constexpr uint32_t kConsRecIndex = (1u << 30) - 1, kConsRecDown = 1u << 30, kConsRecUp = 1u << 31;
constexpr int kConsRecMaxN = (int)kConsRecIndex;

RH_HOST_DEVICE inline ConsRec cons_rec_pack(uint8_t ch, int P, int enc)
{
    return ConsRec{(uint32_t)P | (cons_no_downstream(ch) ? kConsRecDown : 0u) | (cons_no_upstream(ch) ? kConsRecUp : 0u), (uint32_t)enc};
}
RH_HOST_DEVICE inline int cons_rec_partner(ConsRec r) { return (int)(r.p & kConsRecIndex); }
RH_HOST_DEVICE inline int cons_rec_enc(ConsRec r) { return (int)r.e; }
// allow_pair on the records of letters a and b
RH_HOST_DEVICE inline bool allow_pair_rec(int a, int b, int n, ConsRec ra, ConsRec rb)
{
    return allow_pair_values(a, b, n, (ra.p & kConsRecDown) != 0, (rb.p & kConsRecUp) != 0, cons_rec_partner(ra), cons_rec_partner(rb), cons_rec_enc(ra), cons_rec_enc(rb));
}

uint8_t nuc_code(char ch);      // CONTRAfold model: A,C,G,U -> 0..3 in either case, anything else (T and N included) 4; host only, here so that a CPU program can call it
uint8_t vienna_code(char ch);   // ViennaRNA encode_char with energy_set 0: A,C,G,U -> 1..4 (T reads as U), anything else 0

// Fills ch / P / enc at 1..n (the caller presets '.' / 0 / 0 everywhere else).  cons may be shorter or longer than n.
// Returns false for unbalanced brackets or a forced pair of non-complementary letters, with the reason in *why.
bool constraint_prepass(const char* seq, int n, const char* cons, uint8_t* ch, int* P, int* enc, std::string* why);

// ---- joint constraints by shares (indexed batches: rh_batch_upload_indexed_constrained)
//
// The joint constraint of a pair is first share (over s1, cut at n1, filled with '.') + second share (over s2).  A share is passed
// once per distinct sequence and role, without knowing the partner; compose_joint_letter puts two shares together into the ch / P /
// enc that constraint_prepass leaves for the materialised joint string, letter by letter, so the masks of all pairs are built on the
// device from the shares of the distinct sequences (joint_cons_gather, allow_mask.hip).
//
// Open brackets of a share: a '(' of a first share without a ')' in it, a ')' of a second share without a '(' in it.  In the joint
// string the open '(' are still on the stack when s2 begins, and every open ')' pops the innermost of them: the r-th open ')' from
// the left pairs with the r-th open '(' from the right.  A first share must not leave a ')' open nor a second share a '(', and both
// must leave the same number open (the joint string is unbalanced otherwise).
//
// Per letter k = 1..n of a share (the caller presets '.' / 0 / 0 elsewhere):
//   ch[k]   the constraint character
//   P[k]    > 0: the partner of a bracket matched inside the share (a position of the share);
//           < 0: an open bracket, -P[k] = its place among the share's open brackets counted from the left (1 = leftmost); 0: no bracket
//   enc[k]  > 0: the innermost bracket of the share that strictly encloses k -- a matched one or, first share, an open '(';
//           < 0: second share, no bracket of the share encloses k: -enc[k] = the place (as above) of the next open ')' to the right of
//                k, whose partner in the first share encloses k in the joint string;  0: nothing encloses k
// open[]: the positions of the share's open brackets, ascending.
struct ShareRef {
    const uint8_t* ch;
    const int* P;
    const int* enc;
    const int* open;
};

// ch / P / enc of letter j of the joint string of n1 + n2 letters, from the first share A (of s1) and the second share B (of s2),
// which both leave m brackets open.  Outside 1..n1+n2: '.' / 0 / 0.  The kernel and the CPU check both call this.
RH_HOST_DEVICE inline void compose_joint_letter(int j, int n1, int n2, int m, const ShareRef& A, const ShareRef& B, uint8_t* ch, int* P, int* enc)
{
    if (j < 1 || j > n1 + n2) { *ch = '.'; *P = 0; *enc = 0; return; }
    if (j <= n1) {
        const int p = A.P[j];
        *ch = A.ch[j];
        *P = p >= 0 ? p : n1 + B.open[m + p];   // open '(' number -p from the left = number m + p + 1 from the right: that open ')' of s2
        *enc = A.enc[j];
        return;
    }
    const int k = j - n1, p = B.P[k], e = B.enc[k];
    *ch = B.ch[k];
    *P = p > 0 ? n1 + p : p < 0 ? A.open[m + p] : 0;
    *enc = e > 0 ? n1 + e : e < 0 ? A.open[m + e] : 0;
}

// role 0: `share` as the first share of a joint constraint over seq, role 1: as the second.  Fills ch / P / enc at 1..n and appends
// the open positions to *open.  share may be nullptr (all '.'), shorter or longer than n.  Returns false, with the reason in *why,
// for a share no joint string can hold in that role (a ')' left open in a first share, a '(' in a second) and for a forced pair of
// non-complementary letters inside the share.
bool share_prepass(const char* seq, int n, const char* share, int role, uint8_t* ch, int* P, int* enc, std::vector<int>* open, std::string* why);

// What of a joint constraint only the pair shows: the two shares leave the same number of brackets open (m1 open '(' of s1 at open1,
// m2 open ')' of s2 at open2) and the pairs they force across the cut are of complementary letters.  O(open brackets).
bool joint_pair_check(const char* s1, const int* open1, int m1, const char* s2, const int* open2, int m2, std::string* why);

}  // namespace rh::host
