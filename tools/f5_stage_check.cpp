// f5_stage_check.cpp -- stand-alone host program around the index maps of the exterior-sum passes (ractip_amd/csrc/f5_stage.h; the
// kernels are lin_f5i_pass / lin_f5o_pass, mccaskill_strip.hip).  No GPU, no HIP; meant to be built with the sanitizers too:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ractip_amd/csrc tools/f5_stage_check.cpp -o f5_stage_check
//   ./f5_stage_check [quick]
//
// Both passes run on the CPU, thread by thread and in the kernels' order (stage a chunk, sum it, next chunk, chain), through the maps of
// the header, over a synthetic FCA table of distinct values whose cells that do not exist are NaN.  Every F5i and F5o entry is compared
// AS BITS with the serial recurrences of lin_f5i_tail / lin_f5o_head under the same 256-way partition (thread t takes terms t, t+256, ..
// ascending by fma from 0, the wavefront's butterfly sum, the four partial sums in order, f5_entry).  Also checked: every term that
// exists is delivered exactly once, to thread (term mod 256), from a slot that was staged from a cell that exists; no staged address
// leaves the cells of the sequence's own table; no LDS slot is written twice within a chunk or lies outside the chunk buffer; the
// dynamic LDS stays within 64 KB at every ld.
// Lengths: every n from 32 to 600, 1025 and 2000 at ld = (n+3) & ~1 (staging.hip); every fifth of them in a batch with a 2000-letter
// sequence (ld = 2002), and 40 / 300 / 600 at ld = 4088, the largest that the pass kernels launch at, where the chunk is smaller.
// `quick`: every seventh length.  Prints one summary line; exit status 0 only if nothing differs.  tests/test_f5_stage_cpu.py runs it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "f5_stage.h"

namespace {

using namespace rh;

constexpr double kWeu = 0.9, kWep2 = 0.1;   // F5 stays within e^-210 .. e^100 over 2000 entries
constexpr int kJlo = 32;                     // the bootstrap diagonals leave F5i[0..31]

struct Counts { long lengths = 0, entries = 0, terms = 0, differ = 0, misdelivered = 0, stray = 0, rewritten = 0, lds = 0; } G;

struct Table {
    int n, ld;
    std::vector<double> fca;   // rows 0 .. n-2, row d has columns 1 .. n-1-d
    Table(int n_, int ld_) : n(n_), ld(ld_), fca((size_t)(n_ - 1) * ld_, std::numeric_limits<double>::quiet_NaN())
    {
        for (int d = 0; d <= n - 2; d++)
            for (int i = 1; i <= n - 1 - d; i++) {
                const double x = ((size_t)d * 2003 + i) * 0.6180339887498949;
                fca[(size_t)d * ld + i] = (0.5 + (x - std::floor(x))) / n;
            }
    }
    bool cell(size_t a) const { const size_t d = a / ld, i = a % ld; return d <= (size_t)(n - 2) && i >= 1 && i <= (size_t)(n - 1) - d; }
};

double f5_term(double f5, double fca, double acc) { return std::fma(f5, fca, acc); }
double f5_entry(double prev, const double* r, double w_eu, double w_ep2) { return std::fma(prev, w_eu, (r[0] + r[1] + r[2] + r[3]) * w_ep2); }
// wsum of every wavefront of the workgroup: the butterfly of dev_util.h, lane 0
void reduce(const double* a, double* red)
{
    for (int w = 0; w < 4; w++) {
        double v[64], u[64];
        std::memcpy(v, a + 64 * w, sizeof v);
        for (int o = 32; o > 0; o >>= 1) {
            for (int l = 0; l < 64; l++) u[l] = v[l] + v[l ^ o];
            std::memcpy(v, u, sizeof v);
        }
        red[w] = v[0];
    }
}

// lin_f5i_tail / lin_f5o_head
void serial(const Table& T, std::vector<double>& f5i, std::vector<double>& f5o)
{
    const int n = T.n, ld = T.ld;
    double acc[kF5Threads], red[4];
    f5i.assign(ld, 0.0); f5o.assign(ld, 0.0);
    f5i[0] = 1.0;
    for (int jj = 1; jj <= n; jj++) {
        for (int t = 0; t < kF5Threads; t++) {
            acc[t] = 0.0;
            for (int k = t; k <= jj - 2; k += 256) acc[t] = f5_term(f5i[k], T.fca[(size_t)(jj - 2 - k) * ld + (k + 1)], acc[t]);
        }
        reduce(acc, red);
        f5i[jj] = f5_entry(f5i[jj - 1], red, kWeu, kWep2);
    }
    f5o[n] = 1.0;
    for (int k = n - 1; k >= 1; k--) {
        for (int t = 0; t < kF5Threads; t++) {
            acc[t] = 0.0;
            for (int jj = k + 2 + t; jj <= n; jj += 256) acc[t] = f5_term(f5o[jj], T.fca[(size_t)(jj - 2 - k) * ld + (k + 1)], acc[t]);
        }
        reduce(acc, red);
        f5o[k] = f5_entry(f5o[k + 1], red, kWeu, kWep2);
    }
}

// the chunk buffer of one workgroup, with what the checks need to know about every slot
struct Stage {
    int R;
    std::vector<double> v;
    std::vector<char> written, real;
    explicit Stage(int R_) : R(R_), v((size_t)R_ * kF5StageStride), written(v.size()), real(v.size()) {}
    // f5_stage_issue + f5_stage_store of all threads; last(e) = the last row that exists for entry e, addr(row, e) its cell
    template <typename Last, typename Addr>
    void fill(const Table& T, F5Chunk ch, Last last, Addr addr)
    {
        std::fill(written.begin(), written.end(), 0);
        for (int t = 0; t < kF5Threads; t++)
            for (int i = 0; i < kF5StageLoads; i++) {
                if (kF5Blk * i >= R) continue;
                const int e = f5_stage_entry(t), row = ch.lo + f5_stage_row(t, i), lim = last(e) < ch.hi ? last(e) : ch.hi;
                const bool ex = row <= lim;
                const size_t a = ex ? addr(row, e) : (size_t)1;
                if (a >= T.fca.size() || !T.cell(a)) { G.stray++; continue; }
                const int slot = f5_stage_slot(f5_stage_row(t, i), e);
                if (slot < 0 || slot >= (int)v.size()) { G.stray++; continue; }
                if (written[slot]) G.rewritten++;
                written[slot] = 1; real[slot] = ex; v[slot] = T.fca[a];
            }
    }
    // a read by the thread that sums the operand
    double take(int slot)
    {
        if (slot < 0 || slot >= (int)v.size() || !written[slot] || !real[slot]) { G.misdelivered++; return std::numeric_limits<double>::quiet_NaN(); }
        return v[slot];
    }
};

void compare(const std::vector<double>& a, const std::vector<double>& b, int lo, int hi)
{
    for (int k = lo; k <= hi; k++) {
        G.entries++;
        if (std::memcmp(&a[k], &b[k], sizeof(double)) != 0 || !std::isfinite(a[k]) || a[k] == 0.0) G.differ++;
    }
}

// lin_f5i_pass
void pass_inside(const Table& T, const std::vector<double>& ref)
{
    const int n = T.n, ld = T.ld, R = f5_stage_rows(ld, 0);
    if (f5_lds_doubles(ld, 0) > kF5LdsDoubles || R < kF5StageRowsMin || R % (kF5Threads / kF5Blk)) G.lds++;
    Stage S(R);
    std::vector<double> f5s(ref.begin(), ref.begin() + kJlo);
    f5s.resize(ld, std::numeric_limits<double>::quiet_NaN());
    double prev = f5s[kJlo - 1];
    std::vector<double> acc(kF5Threads * kF5Blk);
    std::vector<int> kin(kF5Threads), got;
    for (int jj0 = kJlo; jj0 <= n; jj0 += kF5Blk) {
        const int ne = n - jj0 + 1 < kF5Blk ? n - jj0 + 1 : kF5Blk, top = jj0 + ne - 3;
        std::fill(acc.begin(), acc.end(), 0.0);
        std::fill(kin.begin(), kin.end(), 0x7fffffff);
        got.assign((size_t)(top + 1) * kF5Blk, 0);   // deliveries of term k of entry e
        const int nc = f5_chunks(top, R);
        for (int c = 0; c < nc; c++) {
            const F5Chunk ch = f5i_chunk(top, R, c);
            if (ch.hi - ch.lo + 1 > R || ch.lo < 0 || (c + 1 == nc && ch.lo != 0)) G.stray++;
            S.fill(T, ch, [&](int e) { return f5i_last_row(jj0, ne, e); }, [&](int d, int e) { return f5i_addr(ld, jj0, d, e); });
            for (int t = 0; t < kF5Threads; t++)
                for (int e = 0; e < kF5Blk; e++) {
                    const int k = f5i_owned_term(jj0, ch.hi, e, t), d = f5i_term(jj0, k, e);
                    const bool own = e < ne && k >= 0 && d >= ch.lo;
                    if (!own) continue;
                    if ((k & (kF5Threads - 1)) != t || d > ch.hi) G.misdelivered++;
                    if (k >= jj0) { kin[t] = k; continue; }   // (summed in the chain, from the buffer)
                    got[(size_t)k * kF5Blk + e]++;
                    acc[t * kF5Blk + e] = f5_term(f5s[k], S.take(f5_stage_slot(d - ch.lo, e)), acc[t * kF5Blk + e]);
                }
        }
        for (int e = 0; e < ne; e++) {
            const int jj = jj0 + e;
            double a[kF5Threads], red[4];
            for (int t = 0; t < kF5Threads; t++) {
                a[t] = acc[t * kF5Blk + e];
                if (e >= 2 && kin[t] <= jj - 2) {
                    got[(size_t)kin[t] * kF5Blk + e]++;
                    a[t] = f5_term(f5s[kin[t]], S.take(f5_stage_slot(f5i_term(jj0, kin[t], e), e)), a[t]);
                }
            }
            reduce(a, red);
            prev = f5_entry(prev, red, kWeu, kWep2);
            f5s[jj] = prev;
        }
        for (int e = 0; e < kF5Blk; e++)
            for (int k = 0; k <= top; k++) {
                const int want = e < ne && k <= jj0 + e - 2;
                G.terms += want;
                if (got[(size_t)k * kF5Blk + e] != want) G.misdelivered++;
            }
    }
    compare(f5s, ref, kJlo, n);
}

// lin_f5o_pass
void pass_outside(const Table& T, const std::vector<double>& ref)
{
    const int n = T.n, ld = T.ld, R = f5_stage_rows(ld, 1);
    if (f5_lds_doubles(ld, 1) > kF5LdsDoubles || R < kF5StageRowsMin || R % (kF5Threads / kF5Blk)) G.lds++;
    Stage S(R);
    const int npark = f5_fixed_doubles(ld, 1) - f5_fixed_doubles(ld, 0);
    std::vector<double> f5s(ld, std::numeric_limits<double>::quiet_NaN()), park(npark);
    std::vector<int> parked_by(npark);
    f5s[n] = ref[n];
    double prev = f5s[n];
    std::vector<double> acc(kF5Threads * kF5Blk);
    std::vector<int> got;
    for (int k0 = n - 1; k0 >= 1; k0 -= kF5Blk) {
        const int ne = k0 < kF5Blk ? k0 : kF5Blk, rmax = n - 2 - (k0 - ne + 1);
        std::fill(acc.begin(), acc.end(), 0.0);
        std::fill(parked_by.begin(), parked_by.end(), -1);
        got.assign((size_t)(rmax + 1 > 0 ? rmax + 1 : 0) * kF5Blk, 0);   // deliveries of term r of entry e
        const int nc = f5_chunks(rmax, R);
        for (int c = 0; c < nc; c++) {
            const F5Chunk ch = f5o_chunk(rmax, R, c);
            if (ch.hi - ch.lo + 1 > R || ch.lo < 0) G.stray++;
            S.fill(T, ch, [&](int e) { return f5o_last_row(n, k0, ne, e); }, [&](int r, int e) { return f5o_addr(ld, k0, r, e); });
            for (int t = 0; t < kF5Threads; t++) {
                const int r = f5o_owned_row(ch.lo, t), q = r >> 8;
                if (r > ch.hi) continue;
                if (r != t + 256 * q) G.misdelivered++;
                for (int e = 0; e < kF5Blk; e++) {
                    if (r > f5o_last_row(n, k0, ne, e)) continue;
                    const double op = S.take(f5_stage_slot(r - ch.lo, e));
                    if (e >= 2 && t <= e - 2) {
                        const int p = f5_park_slot(q, e, t);
                        if (p < 0 || p >= npark || parked_by[p] >= 0) { G.stray++; continue; }
                        park[p] = op; parked_by[p] = t;
                    } else {
                        got[(size_t)r * kF5Blk + e]++;
                        acc[t * kF5Blk + e] = f5_term(f5s[k0 - e + 2 + r], op, acc[t * kF5Blk + e]);
                    }
                }
            }
        }
        for (int e = 0; e < ne; e++) {
            const int k = k0 - e;
            double a[kF5Threads], red[4];
            for (int t = 0; t < kF5Threads; t++) {
                a[t] = acc[t * kF5Blk + e];
                if (e >= 2 && t <= e - 2) {
                    a[t] = 0.0;
                    for (int q = 0; k + 2 + t + 256 * q <= n; q++) {
                        const int p = f5_park_slot(q, e, t);
                        if (p < 0 || p >= npark || parked_by[p] != t) { G.misdelivered++; continue; }
                        got[(size_t)(t + 256 * q) * kF5Blk + e]++;
                        a[t] = f5_term(f5s[k + 2 + t + 256 * q], park[p], a[t]);
                    }
                }
            }
            reduce(a, red);
            prev = f5_entry(prev, red, kWeu, kWep2);
            f5s[k] = prev;
        }
        for (int e = 0; e < kF5Blk; e++)
            for (int r = 0; r <= rmax; r++) {
                const int want = e < ne && k0 - e + 2 + r <= n;
                G.terms += want;
                if (got[(size_t)r * kF5Blk + e] != want) G.misdelivered++;
            }
    }
    compare(f5s, ref, 1, n - 1);
}

void run(int n, int ld)
{
    const Table T(n, ld);
    std::vector<double> f5i, f5o;
    serial(T, f5i, f5o);
    pass_inside(T, f5i);
    pass_outside(T, f5o);
    G.lengths++;
}

}  // namespace

int main(int argc, char** argv)
{
    const int step = argc > 1 && !std::strcmp(argv[1], "quick") ? 7 : 1;
    std::vector<int> lens;
    for (int n = 32; n <= 600; n += step) lens.push_back(n);
    lens.push_back(1025); lens.push_back(2000);
    for (int n : lens) run(n, (n + 3) & ~1);
    for (size_t q = 0; q < lens.size(); q += 5)
        if (lens[q] < 2000) run(lens[q], (2000 + 3) & ~1);
    for (int n : {40, 300, 600}) run(n, 4088);
    // every ld that launched the pass kernels when the parked operands took ceil(ld/256)*256 doubles still does
    for (int ld = 4; ld + 8 + (ld + 255) / 256 * 256 <= kF5LdsDoubles; ld += 2)
        for (int phase = 0; phase < 2; phase++)
            if (f5_lds_doubles(ld, phase) > kF5LdsDoubles || f5_stage_rows(ld, phase) < kF5StageRowsMin || f5_stage_rows(ld, phase) % (kF5Threads / kF5Blk)) G.lds++;
    std::printf("lengths %ld entries %ld terms %ld differ %ld misdelivered %ld stray %ld rewritten %ld lds %ld\n", G.lengths, G.entries, G.terms, G.differ,
                G.misdelivered, G.stray, G.rewritten, G.lds);
    return G.differ || G.misdelivered || G.stray || G.rewritten || G.lds ? 1 : 0;
}
