/* vienna2x_oracle.c -- TEST-ONLY.  PARITY UNPINNED (ViennaRNA is absent; see oracle/vienna2x.py).
 *
 * Polynomial-time CPU restatement, plain C, double precision, log space, of what the product computes for ONE sequence (or two
 * concatenated molecules) under the ViennaRNA-2.x energy functions with dangles = 2: McCaskill's partition function (pf_fold),
 * base-pair probabilities, region accessibility (pf_unstru) and the two-molecule ensemble of co_pf_fold.
 *
 * The energy model is the one oracle/vienna2x.py states (E_IntLoop, w_stem with SMOOTH, w_hairpin, the multiloop terms of
 * brute_fold, the exterior-like gap loop of brute_cofold); the tables come from Python as flat arrays of the T dict, so that
 * vienna2x.py stays the only reader of parameter files.  tests/test_vienna2x_oracle.py pins this file to vienna2x.E_IntLoop and to
 * enumeration of every structure (brute_fold / brute_cofold).
 *
 * The recurrences are the textbook ones over LETTERS (1-based, a pair is (i, j) with i < j):
 *     QB[i][j]   i pairs j:   hairpin  (+)  QB[p][q] * interior(i,j,p,q)  (+)  (+)_k QM[i+1][k-1] * QM1[k][j-1] * closing(i,j)
 *     QM1[i][j]  one stem (i, l), l <= j, then unpaired letters:   QM1[i][j-1] * b  (+)  QB[i][j] * stemM(i,j)
 *     QM[i][j]   one stem or more:   (+)_k ( b^(k-i)  (+)  QM[i][k-1] ) * QM1[k][j]
 *     Q5[j]      exterior loop of letters 1..j:   Q5[j-1]  (+)  (+)_k Q5[k-1] * QB[k][j] * stemE(k,j)
 * and an outside pass in pull form over the same productions (QBo, QM1o, QMo, Q5o), rows i ascending and j descending, so that
 * every enclosing interval is final when a cell is computed.
 *
 * cut > 0 (two molecules, the backbone gap between letters cut and cut+1 does not exist): a pair (i, j) with i <= cut < j whose
 * loop holds the gap closes an exterior-like loop, XS[i+1] * XP[j-1] * stemE(the pair seen from inside), XS[a] / XP[b] the
 * exterior partition functions of letters a..cut / cut+1..b; no hairpin, interior-loop side or multiloop backbone may hold the
 * gap, and a stem's neighbour letter counts only on its own strand.  Pairs keep 3 letters between them across the gap too.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define MAXLOOP 30
#define TURN 3
#define VINF 1000000
#define NINF (-INFINITY)

enum { O_STACK = 0, O_MMH = 64, O_MMI = 264, O_MM1N = 464, O_MM23 = 664, O_MMM = 864, O_MMEXT = 1064, O_D5 = 1264, O_D3 = 1304,
       O_INT11 = 1344, O_INT21 = 2944, O_INT22 = 10944, O_HAIRPIN = 50944, O_BULGE = 50975, O_INTERIOR = 51006, O_MISC = 51037,
       O_COUNT = 51043 };
#define MAX_SPECIAL 64

/* ints: stack[8][8] mismatchH / I / 1nI / 23I / M / Ext [8][5][5] dangle5 / dangle3 [8][5] int11[8][8][5][5] int21[8][8][5][5][5]
 * int22[8][8][5][5][5][5] hairpin / bulge / interior [31], then ninio, max_ninio, ML_base, ML_closing, ML_intern, TerminalAU */
typedef struct v2o_model {
    int v[O_COUNT];
    double lxc, kT;
    int n_special;
    char special[MAX_SPECIAL][10];   /* closing pair + loop letters: 5 (triloop), 6 (tetraloop) or 8 (hexaloop) letters */
    int special_e[MAX_SPECIAL];
} v2o_model;

static const int RTYPE[8] = {0, 2, 1, 4, 3, 6, 5, 7};

/* loops: the keys of Triloops, Tetraloops and Hexaloops, separated by blanks; loop_e: their energies in the same order */
v2o_model* v2o_new(const int* ints, int n_ints, double lxc, const char* loops, const int* loop_e)
{
    if (n_ints != O_COUNT) return NULL;
    v2o_model* m = (v2o_model*)calloc(1, sizeof(v2o_model));
    memcpy(m->v, ints, sizeof(int) * O_COUNT);
    m->lxc = lxc;
    m->kT = (37.0 + 273.15) * 1.98717;
    const char* p = loops;
    while (*p && m->n_special < MAX_SPECIAL) {
        while (*p == ' ') p++;
        int len = 0;
        while (p[len] && p[len] != ' ') len++;
        if (len == 0) break;
        if (len <= 8) {
            memcpy(m->special[m->n_special], p, len);
            m->special_e[m->n_special] = loop_e[m->n_special];
            m->n_special++;
        } else { free(m); return NULL; }
        p += len;
    }
    return m;
}
void v2o_free(v2o_model* m) { free(m); }

static int code(char c)
{
    switch (c) {
        case 'A': case 'a': return 1;
        case 'C': case 'c': return 2;
        case 'G': case 'g': return 3;
        case 'U': case 'u': case 'T': case 't': return 4;
        default: return 0;
    }
}
static int pair_type(int a, int b)
{   /* CG=1 GC=2 GU=3 UG=4 AU=5 UA=6 */
    static const int PT[5][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 5}, {0, 0, 0, 1, 0}, {0, 0, 2, 0, 3}, {0, 6, 0, 4, 0}};
    return PT[a][b];
}
static int imin(int a, int b) { return a < b ? a : b; }

/* E_IntLoop of ViennaRNA 2.x in 10 cal/mol: n1 / n2 unpaired letters on the 5' / 3' side, t the outer pair's type, t2 the inner
 * pair's type seen from inside (rtype), si1 / sj1 the letters after / before the outer pair's letters, sp1 / sq1 the letters
 * before / after the inner pair's */
int v2o_int_loop(const v2o_model* m, int n1, int n2, int t, int t2, int si1, int sj1, int sp1, int sq1)
{
    const int* v = m->v;
    const int nl = n1 > n2 ? n1 : n2, ns = n1 > n2 ? n2 : n1;
    const int tau = v[O_MISC + 5], ninio = v[O_MISC + 0], max_ninio = v[O_MISC + 1];
    if (nl == 0) return v[O_STACK + t * 8 + t2];
    if (ns == 0) {
        int e = nl <= MAXLOOP ? v[O_BULGE + nl] : v[O_BULGE + 30] + (int)(m->lxc * log(nl / 30.0));
        if (nl == 1) e += v[O_STACK + t * 8 + t2];
        else e += (t > 2 ? tau : 0) + (t2 > 2 ? tau : 0);
        return e;
    }
    if (ns == 1) {
        if (nl == 1) return v[O_INT11 + ((t * 8 + t2) * 5 + si1) * 5 + sj1];
        if (nl == 2)
            return n1 == 1 ? v[O_INT21 + (((t * 8 + t2) * 5 + si1) * 5 + sq1) * 5 + sj1]
                           : v[O_INT21 + (((t2 * 8 + t) * 5 + sq1) * 5 + si1) * 5 + sp1];
        int e = nl + 1 <= MAXLOOP ? v[O_INTERIOR + nl + 1] : v[O_INTERIOR + 30] + (int)(m->lxc * log((nl + 1) / 30.0));
        e += imin(max_ninio, (nl - ns) * ninio);
        return e + v[O_MM1N + (t * 5 + si1) * 5 + sj1] + v[O_MM1N + (t2 * 5 + sq1) * 5 + sp1];
    }
    if (ns == 2) {
        if (nl == 2) return v[O_INT22 + ((((t * 8 + t2) * 5 + si1) * 5 + sp1) * 5 + sq1) * 5 + sj1];
        if (nl == 3) return v[O_INTERIOR + 5] + ninio + v[O_MM23 + (t * 5 + si1) * 5 + sj1] + v[O_MM23 + (t2 * 5 + sq1) * 5 + sp1];
    }
    const int u = nl + ns;
    int e = u <= MAXLOOP ? v[O_INTERIOR + u] : v[O_INTERIOR + 30] + (int)(m->lxc * log(u / 30.0));
    e += imin(max_ninio, (nl - ns) * ninio);
    return e + v[O_MMI + (t * 5 + si1) * 5 + sj1] + v[O_MMI + (t2 * 5 + sq1) * 5 + sp1];
}

/* log Boltzmann weight of a dangle / mismatch_multi / mismatch_exterior energy: exp(SMOOTH(-E) * 10 / kT) */
static double smooth_w(const v2o_model* m, int E)
{
    const double X = -(double)E, x = X / 10.0;
    double s;
    if (x < -1.2283697) s = 0.0;
    else if (x > 0.8660254) s = X;
    else { const double q = sin(x - 0.34242663) + 1.0; s = 10.0 * 0.38490018 * q * q; }
    return s * 10.0 / m->kT;
}
/* a stem of type t in the exterior loop (mm = O_MMEXT) or a multiloop (mm = O_MMM): si1 / sj1 its 5' / 3' neighbour letters,
 * 0 where there is none (an unknown letter counts as none); TerminalAU included, ML_intern not */
static double stem_w(const v2o_model* m, int mm, int t, int si1, int sj1)
{
    double w = 0.0;
    if (si1 > 0 && sj1 > 0) w = smooth_w(m, m->v[mm + (t * 5 + si1) * 5 + sj1]);
    else if (si1 > 0) w = smooth_w(m, m->v[O_D5 + t * 5 + si1]);
    else if (sj1 > 0) w = smooth_w(m, m->v[O_D3 + t * 5 + sj1]);
    return w - (t > 2 ? m->v[O_MISC + 5] * 10.0 / m->kT : 0.0);
}

/* streaming log-sum-exp: one exp per term */
typedef struct { double m, s; } lse_t;
static const lse_t LSE0 = {NINF, 0.0};
static inline void lse_add(lse_t* a, double x)
{
    if (!(x > NINF)) return;
    if (x <= a->m) a->s += exp(x - a->m);
    else { a->s = a->s * exp(a->m - x) + 1.0; a->m = x; }
}
static inline double lse_value(const lse_t* a) { return a->s > 0.0 ? a->m + log(a->s) : NINF; }

typedef struct {
    const v2o_model* m;
    const int* S;              /* S[0] = S[n+1] = 0 */
    const char* L;             /* letters normalised to ACGU / N, 1-based */
    const unsigned char* allow;   /* (n+1) x (n+1), allow[a*(n+1)+b] != 0 iff letters a < b may pair; NULL: no constraint */
    int n, cut;
    double sc;                 /* 10 / kT */
} ctx_t;

static int can_pair(const ctx_t* c, int i, int j)
{
    if (i < 1 || j > c->n || j - i - 1 < TURN) return 0;
    if (c->allow && !c->allow[(size_t)i * (c->n + 1) + j]) return 0;
    return pair_type(c->S[i], c->S[j]);
}
/* the backbone between letters g and g+1 is the one that does not exist */
static inline int gap(const ctx_t* c, int g) { return c->cut > 0 && g == c->cut; }
/* one of the backbone pieces lo|lo+1 .. hi|hi+1 is */
static inline int crosses(const ctx_t* c, int lo, int hi) { return c->cut > 0 && lo <= c->cut && c->cut <= hi; }

static double hairpin_w(const ctx_t* c, int i, int j)
{   /* exp_E_Hairpin: above 30 letters the logarithmic extrapolation enters the Boltzmann factor as it is (it is only the
       minimum-free-energy E_Hairpin that rounds it to an integer energy) */
    const v2o_model* m = c->m;
    const int u = j - i - 1, t = pair_type(c->S[i], c->S[j]);
    const double e = u <= 30 ? (double)m->v[O_HAIRPIN + u] : m->v[O_HAIRPIN + 30] + m->lxc * log(u / 30.0);
    if (u == 3 || u == 4 || u == 6)
        for (int k = 0; k < m->n_special; k++)
            if ((int)strlen(m->special[k]) == u + 2 && strncmp(m->special[k], c->L + i, u + 2) == 0) return -m->special_e[k] * c->sc;
    if (u == 3) return -(e + (t > 2 ? m->v[O_MISC + 5] : 0)) * c->sc;
    return -(e + m->v[O_MMH + (t * 5 + c->S[i + 1]) * 5 + c->S[j - 1]]) * c->sc;
}
static double interior_w(const ctx_t* c, int i, int j, int p, int q)
{
    const int* S = c->S;
    return -c->sc * v2o_int_loop(c->m, p - i - 1, j - q - 1, pair_type(S[i], S[j]), RTYPE[pair_type(S[p], S[q])], S[i + 1], S[j - 1],
                                 S[p - 1], S[q + 1]);
}
/* (i, j) closes a multiloop: ML_closing + ML_intern + its mismatch seen from inside */
static double mlclose_w(const ctx_t* c, int i, int j)
{
    const v2o_model* m = c->m;
    return -(m->v[O_MISC + 3] + m->v[O_MISC + 4]) * c->sc + stem_w(m, O_MMM, RTYPE[pair_type(c->S[i], c->S[j])], c->S[j - 1], c->S[i + 1]);
}
/* (p, q) is a branch of a multiloop */
static double mlstem_w(const ctx_t* c, int p, int q)
{
    return -c->m->v[O_MISC + 4] * c->sc + stem_w(c->m, O_MMM, pair_type(c->S[p], c->S[q]), c->S[p - 1], c->S[q + 1]);
}
/* (p, q) is a stem of the exterior loop or of the loop that holds the missing backbone piece */
static double extstem_w(const ctx_t* c, int p, int q)
{
    return stem_w(c->m, O_MMEXT, pair_type(c->S[p], c->S[q]), gap(c, p - 1) ? 0 : c->S[p - 1], gap(c, q) ? 0 : c->S[q + 1]);
}
/* (i, j) closes the loop that holds the missing backbone piece: an exterior stem seen from inside */
static double gapclose_w(const ctx_t* c, int i, int j)
{
    return stem_w(c->m, O_MMEXT, RTYPE[pair_type(c->S[i], c->S[j])], gap(c, j - 1) ? 0 : c->S[j - 1], gap(c, i) ? 0 : c->S[i + 1]);
}

/* seq: n letters (s1 + s2 when cut = n1 > 0); allow: see ctx_t, or NULL.  post: (n+1)(n+2)/2 doubles, post[off(i) + j] =
 * P(i pairs j) with off(i) = i(2(n+1)-i-1)/2 (the reference's triangular layout), or NULL.  up: n * max_w doubles,
 * up[(a-1)*max_w + w] = P(letters a .. a+w unpaired), 0 where the run leaves the sequence, or NULL; one molecule only.
 * Returns log Z of the inside pass; *logz_out = log Z of the outside pass. */
double v2o_fold(const v2o_model* m, const char* seq, int n, int cut, const unsigned char* allow, int max_w, double* post, double* up,
                double* logz_out)
{
    if (n < 1 || cut < 0 || cut >= n || (cut > 0 && up)) return NAN;
    const size_t W = (size_t)n + 2;
    int* S = (int*)calloc(W, sizeof(int));
    char* L = (char*)calloc(W + 1, 1);
    for (int i = 1; i <= n; i++) { S[i] = code(seq[i - 1]); L[i] = "NACGU"[S[i]]; }
    ctx_t c = {m, S, L, allow, n, cut, 10.0 / m->kT};
    const double mlb = -m->v[O_MISC + 2] * c.sc;
    double* buf = (double*)malloc(sizeof(double) * (6 * W * W + 6 * W));
    for (size_t k = 0; k < 6 * W * W + 6 * W; k++) buf[k] = NINF;
    double *QB = buf, *QM = buf + W * W, *QM1 = buf + 2 * W * W, *QBo = buf + 3 * W * W, *QMo = buf + 4 * W * W, *QM1o = buf + 5 * W * W;
    double *Q5 = buf + 6 * W * W, *Q5o = Q5 + W, *XS = Q5o + W, *XP = XS + W, *XSo = XP + W, *XPo = XSo + W;
#define AT(i, j) ((size_t)(i) * W + (j))
    /* b^(k-i): letters i .. k-1 unpaired in a multiloop, before a branch that starts at k */
#define LEAD(i, k) (crosses(&c, (i), (k) - 2) ? NINF : ((k) - (i)) * mlb)

    /* ------------------------------------------------------------ inside */
    if (cut > 0) XS[cut + 1] = 0.0;
    for (int i = n; i >= 1; i--) {
        for (int j = i; j <= n; j++) {
            if (can_pair(&c, i, j)) {
                lse_t a = LSE0;
                if (crosses(&c, i, j - 1)) lse_add(&a, XS[i + 1] + XP[j - 1] + gapclose_w(&c, i, j));
                else lse_add(&a, hairpin_w(&c, i, j));
                for (int p = i + 1; p <= i + MAXLOOP + 1 && p < j; p++) {
                    if (crosses(&c, i, p - 1)) break;
                    for (int q = j - 1; q > p && (p - i - 1) + (j - q - 1) <= MAXLOOP; q--) {
                        if (crosses(&c, q, j - 1)) break;
                        if (can_pair(&c, p, q)) lse_add(&a, QB[AT(p, q)] + interior_w(&c, i, j, p, q));
                    }
                }
                if (!gap(&c, i) && !gap(&c, j - 1)) {
                    lse_t ml = LSE0;
                    for (int k = i + 2; k <= j - 1; k++) lse_add(&ml, QM[AT(i + 1, k - 1)] + QM1[AT(k, j - 1)]);
                    lse_add(&a, lse_value(&ml) + mlclose_w(&c, i, j));
                }
                QB[AT(i, j)] = lse_value(&a);
            }
            lse_t a1 = LSE0;
            if (j > i && !gap(&c, j - 1)) lse_add(&a1, QM1[AT(i, j - 1)] + mlb);
            if (QB[AT(i, j)] > NINF && !gap(&c, i - 1) && !gap(&c, j)) lse_add(&a1, QB[AT(i, j)] + mlstem_w(&c, i, j));
            QM1[AT(i, j)] = lse_value(&a1);
            lse_t am = LSE0;
            for (int k = i; k <= j; k++) {
                const double right = QM1[AT(k, j)];
                if (!(right > NINF)) continue;
                lse_add(&am, LEAD(i, k) + right);
                if (k > i) lse_add(&am, QM[AT(i, k - 1)] + right);
            }
            QM[AT(i, j)] = lse_value(&am);
        }
        if (cut > 0 && i == cut + 1) {   /* rows above the cut are final: exterior partition function of letters cut+1 .. b */
            XP[cut] = 0.0;
            for (int b = cut + 1; b <= n; b++) {
                lse_t a = LSE0;
                lse_add(&a, XP[b - 1]);
                for (int k = cut + 1; k < b; k++)
                    if (can_pair(&c, k, b)) lse_add(&a, XP[k - 1] + QB[AT(k, b)] + extstem_w(&c, k, b));
                XP[b] = lse_value(&a);
            }
        }
        if (cut > 0 && i <= cut) {       /* row i is final: exterior partition function of letters i .. cut */
            lse_t a = LSE0;
            lse_add(&a, XS[i + 1]);
            for (int l = i + 1; l <= cut; l++)
                if (can_pair(&c, i, l)) lse_add(&a, QB[AT(i, l)] + extstem_w(&c, i, l) + XS[l + 1]);
            XS[i] = lse_value(&a);
        }
    }
    Q5[0] = 0.0;
    for (int j = 1; j <= n; j++) {
        lse_t a = LSE0;
        lse_add(&a, Q5[j - 1]);
        for (int k = 1; k < j; k++)
            if (can_pair(&c, k, j)) lse_add(&a, Q5[k - 1] + QB[AT(k, j)] + extstem_w(&c, k, j));
        Q5[j] = lse_value(&a);
    }
    const double Z = Q5[n];

    /* ------------------------------------------------------------ outside, pull form */
    Q5o[n] = 0.0;
    for (int j = n - 1; j >= 0; j--) {
        lse_t a = LSE0;
        lse_add(&a, Q5o[j + 1]);
        for (int l = j + 2; l <= n; l++)
            if (can_pair(&c, j + 1, l)) lse_add(&a, QB[AT(j + 1, l)] + extstem_w(&c, j + 1, l) + Q5o[l]);
        Q5o[j] = lse_value(&a);
    }
    for (int i = 1; i <= n; i++) {
        if (cut > 0 && i == cut + 1)     /* every pair around the gap is final: what surrounds XP[b] */
            for (int b = n - 1; b >= cut; b--) {
                lse_t a = LSE0;
                for (int ii = 1; ii <= cut; ii++)
                    if (can_pair(&c, ii, b + 1)) lse_add(&a, QBo[AT(ii, b + 1)] + XS[ii + 1] + gapclose_w(&c, ii, b + 1));
                lse_add(&a, XPo[b + 1]);
                for (int bb = b + 2; bb <= n; bb++)
                    if (can_pair(&c, b + 1, bb)) lse_add(&a, XPo[bb] + QB[AT(b + 1, bb)] + extstem_w(&c, b + 1, bb));
                XPo[b] = lse_value(&a);
            }
        if (cut > 0 && i >= 2 && i <= cut + 1) {   /* row i-1 is final: what surrounds XS[i] */
            lse_t a = LSE0;
            for (int j = cut + 1; j <= n; j++)
                if (can_pair(&c, i - 1, j)) lse_add(&a, QBo[AT(i - 1, j)] + XP[j - 1] + gapclose_w(&c, i - 1, j));
            lse_add(&a, XSo[i - 1]);
            for (int aa = 1; aa < i - 1; aa++)
                if (can_pair(&c, aa, i - 1)) lse_add(&a, XSo[aa] + QB[AT(aa, i - 1)] + extstem_w(&c, aa, i - 1));
            XSo[i] = lse_value(&a);
        }
        for (int j = n; j >= i; j--) {
            /* QM[i][j] is the left part under a closing pair (i-1, jj) with the last branch starting at j+1, or of a longer QM[i][jj] */
            lse_t am = LSE0;
            if (i >= 2 && !gap(&c, i - 1))
                for (int jj = j + 2; jj <= n; jj++)
                    if (can_pair(&c, i - 1, jj) && !gap(&c, jj - 1))
                        lse_add(&am, QBo[AT(i - 1, jj)] + QM1[AT(j + 1, jj - 1)] + mlclose_w(&c, i - 1, jj));
            for (int jj = j + 1; jj <= n; jj++) lse_add(&am, QMo[AT(i, jj)] + QM1[AT(j + 1, jj)]);
            QMo[AT(i, j)] = lse_value(&am);
            /* QM1[i][j]: extended by letter j+1, the last branch under a closing pair (ii, j+1), or the last branch of a QM[ii][j] */
            lse_t a1 = LSE0;
            if (j + 1 <= n && !gap(&c, j)) lse_add(&a1, QM1o[AT(i, j + 1)] + mlb);
            if (j + 1 <= n && !gap(&c, j))
                for (int ii = 1; ii <= i - 2; ii++)
                    if (can_pair(&c, ii, j + 1) && !gap(&c, ii))
                        lse_add(&a1, QBo[AT(ii, j + 1)] + QM[AT(ii + 1, i - 1)] + mlclose_w(&c, ii, j + 1));
            for (int ii = 1; ii <= i; ii++) {
                const double o = QMo[AT(ii, j)];
                if (!(o > NINF)) continue;
                lse_add(&a1, o + LEAD(ii, i));
                if (ii < i) lse_add(&a1, o + QM[AT(ii, i - 1)]);
            }
            QM1o[AT(i, j)] = lse_value(&a1);
            if (!can_pair(&c, i, j)) continue;
            lse_t a = LSE0;
            lse_add(&a, Q5[i - 1] + extstem_w(&c, i, j) + Q5o[j]);
            for (int ii = i - 1; ii >= 1 && ii >= i - MAXLOOP - 1; ii--) {
                if (crosses(&c, ii, i - 1)) break;
                for (int jj = j + 1; jj <= n && (i - ii - 1) + (jj - j - 1) <= MAXLOOP; jj++) {
                    if (crosses(&c, j, jj - 1)) break;
                    if (can_pair(&c, ii, jj)) lse_add(&a, QBo[AT(ii, jj)] + interior_w(&c, ii, jj, i, j));
                }
            }
            if (!gap(&c, i - 1) && !gap(&c, j)) lse_add(&a, QM1o[AT(i, j)] + mlstem_w(&c, i, j));
            if (cut > 0 && j <= cut) lse_add(&a, XSo[i] + extstem_w(&c, i, j) + XS[j + 1]);
            if (cut > 0 && i > cut) lse_add(&a, XPo[j] + XP[i - 1] + extstem_w(&c, i, j));
            QBo[AT(i, j)] = lse_value(&a);
        }
    }
    if (logz_out) *logz_out = Q5o[0];

    if (post) {
        memset(post, 0, sizeof(double) * ((size_t)(n + 1) * (n + 2) / 2));
        for (int i = 1; i <= n; i++) {
            const size_t off = (size_t)i * (2 * (n + 1) - i - 1) / 2;
            for (int j = i + 1; j <= n; j++) {
                const double e = QB[AT(i, j)] + QBo[AT(i, j)] - Z;
                if (e > NINF) post[off + j] = exp(e);
            }
        }
    }

    if (up && max_w > 0) {
        /* a run a..b of unpaired letters lies in one loop:
         *   exterior    Q5[a-1] * Q5o[b]
         *   hairpin     (p, q) with p < a, b < q
         *   interior    the run inside the 5' gap (i < a, b < p) or the 3' gap (q < a, b < j) of a loop (i, j, p, q)
         *   multiloop   inside the letters a QM1 appends after its stem: QM1[i][a-1] -> QM1[i][b],
         *               or inside the unpaired letters i..k-1 that a QM puts before its only branch: i <= a, b < k
         * every class is summed as probabilities; the hairpin and leading-run sums over (<= a, > b) are 2-D running sums */
        double* HS = (double*)calloc(W * W, sizeof(double));   /* HS[a][b] = sum over hairpins p < a, q > b */
        double* PL = (double*)calloc(W * W, sizeof(double));   /* PL[a][b] = sum over leading runs i <= a, k > b */
        double* GL = (double*)calloc(W * (MAXLOOP + 2), sizeof(double));   /* GL[i][l1]: loops with 5' gap i+1 .. i+l1 */
        double* GR = (double*)calloc(W * (MAXLOOP + 2), sizeof(double));   /* GR[j][l2]: loops with 3' gap j-l2 .. j-1 */
        for (int i = 1; i <= n; i++)
            for (int j = i + TURN + 1; j <= n; j++) {
                if (!can_pair(&c, i, j) || !(QBo[AT(i, j)] > NINF)) continue;
                HS[AT(i + 1, j - 1)] += exp(QBo[AT(i, j)] + hairpin_w(&c, i, j) - Z);   /* the largest run it holds */
                for (int p = i + 1; p <= i + MAXLOOP + 1 && p < j; p++)
                    for (int q = j - 1; q > p && (p - i - 1) + (j - q - 1) <= MAXLOOP; q--) {
                        if (!can_pair(&c, p, q)) continue;
                        const double pr = exp(QBo[AT(i, j)] + interior_w(&c, i, j, p, q) + QB[AT(p, q)] - Z);
                        GL[(size_t)i * (MAXLOOP + 2) + (p - i - 1)] += pr;
                        GR[(size_t)j * (MAXLOOP + 2) + (j - q - 1)] += pr;
                    }
            }
        for (int i = 1; i <= n; i++)
            for (int k = i + 1; k <= n; k++) {
                lse_t a = LSE0;
                for (int j = k; j <= n; j++) lse_add(&a, QMo[AT(i, j)] + QM1[AT(k, j)]);
                const double e = lse_value(&a) + (k - i) * mlb - Z;
                if (e > NINF) PL[AT(i, k - 1)] += exp(e);   /* letters i .. k-1 */
            }
        for (int a = 1; a <= n; a++)
            for (int b = n; b >= 1; b--) {
                HS[AT(a, b)] += HS[AT(a - 1, b)] + HS[AT(a, b + 1)] - HS[AT(a - 1, b + 1)];
                PL[AT(a, b)] += PL[AT(a - 1, b)] + PL[AT(a, b + 1)] - PL[AT(a - 1, b + 1)];
            }
        for (int a = 1; a <= n; a++)
            for (int w = 0; w < max_w; w++) {
                const int b = a + w, len = w + 1;
                double pu = 0.0;
                if (b <= n) {
                    pu += exp(Q5[a - 1] + Q5o[b] - Z);
                    pu += HS[AT(a, b)] + PL[AT(a, b)];
                    for (int i = a - 1; i >= 1 && i >= b - MAXLOOP; i--)
                        for (int l1 = b - i; l1 <= MAXLOOP; l1++) pu += GL[(size_t)i * (MAXLOOP + 2) + l1];
                    for (int j = b + 1; j <= n && j <= a + MAXLOOP; j++)
                        for (int l2 = j - a; l2 <= MAXLOOP; l2++) pu += GR[(size_t)j * (MAXLOOP + 2) + l2];
                    for (int i = 1; i < a - 1; i++) {
                        const double e = QM1o[AT(i, b)] + len * mlb + QM1[AT(i, a - 1)] - Z;
                        if (e > NINF) pu += exp(e);
                    }
                }
                up[(size_t)(a - 1) * max_w + w] = pu;
            }
        free(HS); free(PL); free(GL); free(GR);
    }
#undef AT
#undef LEAD
    free(buf); free(S); free(L);
    return Z;
}
