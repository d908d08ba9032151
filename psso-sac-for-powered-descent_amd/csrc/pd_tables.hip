// pd_tables.hip -- the host table builder of libpdenv.so (pd_tables.h): the hash tables of solved
// neighbourhoods, the clamped query lines and their Taylor pieces, the atmosphere polynomials, the
// candidate grids with their bisector records and the cell pieces.  It decides every bit the step
// kernel reads, so it is built with the host flags of the whole library (-O3 -ffp-contract=off).
// Host code only: no kernel and no HIP runtime call (a HIP source for the shared headers' sake).
#include "pd_tables.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>

using namespace pd;

namespace {

pd_status fail(pd_status s, const char* m) { return set_error(s, m); }

int log2ceil(int64_t v) { int l = 0; while ((1ll << l) < v) ++l; return l; }

template <typename R>
int table_insert(const pd_aero_table& t, Table<R>& T, uint64_t key, std::vector<double>& work, std::vector<double>& pay) {
    int64_t cap = 1ll << T.logcap;
    uint32_t mask = (uint32_t)(cap - 1), h = key_hash(key, T.logcap);
    while (T.keys[h] != kEmptyKey && T.keys[h] != key) h = (h + 1) & mask;
    if (T.keys[h] == key) return (int)h;
    if ((T.entries + 1) * 2 > cap) return -1;   // full (load factor 1/2): no solve
    double aoa[kCols];
    for (int c = 0; c < kCols; ++c) aoa[c] = t.col_aoa[c];
    if (solve_neighbourhood(t.mach, t.coef, t.col_start, aoa, key, work.data(), pay.data()) != 0) return -1;
    T.keys[h] = key;
    pay_store<R>(pay.data(), T.pay.data() + h * pay_stride<R>());
    ++T.entries;
    return (int)h;
}

template <typename R>
pd_status build_table(const pd_aero_table& t, const uint64_t* keys, int64_t nk, Table<R>& T) {
    int64_t cap_need = std::max<int64_t>(4 * std::max<int64_t>(nk, 64), 1024);
    T.logcap = log2ceil(cap_need);
    int64_t cap = 1ll << T.logcap;
    T.keys.assign(cap, kEmptyKey);
    T.pay.assign(cap * pay_stride<R>(), R(0));
    std::vector<double> work(kScratch), pay(kPay);
    for (int64_t e = 0; e < nk; ++e)
        if (table_insert<R>(t, T, keys[e], work, pay) < 0)
            return fail(PD_ERR_INVALID, "invalid/singular neighbourhood key in param pack");
    return PD_OK;
}

// Exact neighbourhood intervals along one horizontal query line a = const: the 50-NN set only
// changes where two points swap distance order, i.e. at pair-bisector crossings; evaluate the
// set between consecutive crossings and merge equal neighbours.  (The device still verifies
// every looked-up set, so a query exactly on a breakpoint stays exact.)
template <typename R>
pd_status build_line(const pd_aero_table& t, double a, Table<R>& T, int li, DevParams<R>& D) {
    std::vector<double> m(t.n_pts), dz(t.n_pts);
    for (int c = 0; c < kCols; ++c)
        for (int k = 0; k < t.col_len[c]; ++k) {
            m[t.col_start[c] + k] = t.mach[t.col_start[c] + k];
            double da = a - t.col_aoa[c];
            dz[t.col_start[c] + k] = da * da;
        }
    std::vector<double> xs;
    for (int i = 0; i < t.n_pts; ++i)
        for (int j = i + 1; j < t.n_pts; ++j) {
            double den = 2.0 * (m[j] - m[i]);
            if (den == 0.0) continue;
            double x = (m[j] * m[j] - m[i] * m[i] + dz[j] - dz[i]) / den;
            if (x > 0.0 && x < 10.0) xs.push_back(x);
        }
    std::sort(xs.begin(), xs.end());
    xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
    std::vector<double> bps;
    bps.push_back(0.0);
    bps.insert(bps.end(), xs.begin(), xs.end());
    bps.push_back(10.0);
    std::vector<double> B;
    std::vector<uint64_t> K;
    for (size_t k = 0; k + 1 < bps.size(); ++k) {
        uint64_t key = host_knn_key(t, 0.5 * (bps[k] + bps[k + 1]), a);
        if (K.empty()) K.push_back(key);
        else if (key != K.back()) { B.push_back(bps[k]); K.push_back(key); }
    }
    D.line_a[li] = (R)a;
    if ((int)B.size() > kLineMax) { D.line_nbp[li] = -1; return PD_OK; }   // too fine: cache path only
    std::vector<double> work(kScratch), pay(kPay);
    D.line_nbp[li] = (int)B.size();
    for (size_t k = 0; k < B.size(); ++k) D.line_bp[li][k] = (R)B[k];
    // search buckets (pd_physics.h kLineBuckets), on the handle-precision breakpoints
    for (int b = 0; b < kLineBuckets; ++b) {
        const double w = 10.0 / kLineBuckets, lo = b * w - 1e-4, hi = (b + 1) * w + 1e-4;
        int nlo = 0, nhi = 0;
        for (size_t k = 0; k < B.size(); ++k) {
            nlo += (double)D.line_bp[li][k] < lo;
            nhi += (double)D.line_bp[li][k] < hi;
        }
        D.line_lb[li][b] = (uint16_t)(nlo | (nhi << 8));
    }
    for (size_t k = 0; k < K.size(); ++k) {
        D.line_key[li][k] = K[k];
        D.line_slot[li][k] = table_insert<R>(t, T, K[k], work, pay);
    }
    return PD_OK;
}

// Taylor pieces of clamped query line li (kTayCells cells of Mach [0, 10], one piece per (cell,
// neighbourhood interval) pair, piece index cell + l with l the interval's index -- the device's
// binary-search result -- so no piece table is needed).  Along the line a = const the thin-plate
// sum f(M) = sum_j c_j phi(|(M, a) - y_j|) + poly is analytic except at the points ON the line
// (d_a = 0, the C_L +10 line lies on the AoA-10 column): each term's singularities are at
// M = m_j +- i d_a.  A piece keeps the kTayExact terms whose singularity is nearest to its cell
// centre x0 as exact terms and expands the rest to degree kTayDeg in t = M - x0 (long double):
//   log((u0 + t)^2 + d^2) = log|z|^2 + sum_k 2 (-1)^(k+1) Re(z^-k) t^k / k,   z = u0 + i d,
//   times (|z|^2 + 2 u0 t + t^2), halved (phi = d2 log(d2) / 2), plus the degree-1 polynomial.
// The remaining singularities are >= 10x the cell half-width away (>= 0.17 on the C_D lines,
// >= 0.024 past the two nearest AoA-10 points), so the truncation is below binary64 rounding;
// every piece is checked at five points against the long double sum and a line whose worst
// error exceeds 1e-13 relative to sum |c_j phi_j| is left to the exact path (tay_off = -1).
// ---------------------------------------------------------------- smooth-function tables
// Least-squares fit of a degree-deg polynomial in t = x - c to f on [lo, hi] (c the centre), from
// 4 (deg + 1) Chebyshev nodes, in long double (monomials in s = t / h on [-1, 1]: well conditioned
// at these degrees); coefficients of t^k into out[0..deg].
template <typename F>
void fit_poly_ld(F&& f, long double lo, long double hi, int deg, long double* out) {
    const int M = 4 * (deg + 1), n = deg + 1;
    const long double c = (lo + hi) / 2, h = (hi - lo) / 2;
    long double A[12][12] = {}, b[12] = {};
    for (int m = 0; m < M; ++m) {
        const long double s = cosl(3.14159265358979323846264338327950288L * (m + 0.5L) / M);
        const long double v = f(c + h * s);
        long double pw[12];
        pw[0] = 1;
        for (int k = 1; k < n; ++k) pw[k] = pw[k - 1] * s;
        for (int i = 0; i < n; ++i) {
            b[i] += pw[i] * v;
            for (int j = 0; j < n; ++j) A[i][j] += pw[i] * pw[j];
        }
    }
    for (int k = 0; k < n; ++k) {   // Gaussian elimination with partial pivoting (normal equations)
        int pv = k;
        for (int i = k + 1; i < n; ++i) if (fabsl(A[i][k]) > fabsl(A[pv][k])) pv = i;
        for (int j = 0; j < n; ++j) std::swap(A[k][j], A[pv][j]);
        std::swap(b[k], b[pv]);
        for (int i = k + 1; i < n; ++i) {
            const long double l = A[i][k] / A[k][k];
            for (int j = k; j < n; ++j) A[i][j] -= l * A[k][j];
            b[i] -= l * b[k];
        }
    }
    long double x[12];
    for (int i = n - 1; i >= 0; --i) {
        long double s = b[i];
        for (int j = i + 1; j < n; ++j) s -= A[i][j] * x[j];
        x[i] = s / A[i][i];
    }
    long double hk = 1;
    for (int k = 0; k < n; ++k) { out[k] = x[k] / hk; hk *= h; }
}

// The ISA atmosphere of atmosphere_dynamics.py:5-27 (ambiance restated, as the device's exact
// path and the oracle compute it) in long double, in layer i: rho, p, a at geometric altitude y
struct AtmLd { long double rho, p, a; };
AtmLd atm_exact_ld(const pd_params* P, int i, long double y) {
    const long double r = P->isa_r, R_ = P->isa_R, g0 = P->isa_g0;
    const long double H = r * y / (r + y), dH = H - (long double)P->isa_Hb[i];
    const long double Tb = P->isa_Tb[i], b = P->isa_beta[i], pb = P->isa_pb[i];
    const long double T = Tb + b * dH;
    const long double p = b != 0 ? pb * powl(1 + b / Tb * dH, -g0 / (b * R_)) : pb * expl(-g0 / (R_ * Tb) * dH);
    return {p / (R_ * T), p, sqrtl((long double)P->isa_kappa * R_ * T)};
}

struct TayStats { double max_abs = 0, max_rel = 0; int64_t pieces = 0; };

template <typename R>
void build_taylor(const pd_aero_table& t, int li, DevParams<R>& D, std::vector<R>& out, TayStats& ts) {
    D.tay_off[li] = -1;
    const int nb = D.line_nbp[li];
    if (nb < 0) return;
    const long double a = (long double)D.line_a[li];
    const double w = 10.0 / kTayCells;
    std::vector<double> bp(nb);
    for (int k = 0; k < nb; ++k) bp[k] = (double)D.line_bp[li][k];
    auto count_below = [&](double x) { return (int)(std::lower_bound(bp.begin(), bp.end(), x) - bp.begin()); };
    // the binary64 payload of every interval (the same solve as the tables')
    std::vector<std::vector<double>> pays(nb + 1, std::vector<double>(kPay));
    std::vector<double> work(kScratch);
    std::vector<double> aoa(kCols);
    for (int c = 0; c < kCols; ++c) aoa[c] = t.col_aoa[c];
    for (int l = 0; l <= nb; ++l)
        if (solve_neighbourhood(t.mach, t.coef, t.col_start, aoa.data(), D.line_key[li][l], work.data(), pays[l].data()) != 0)
            return;
    const size_t base = out.size();
    out.resize(base + (size_t)(kTayCells + nb) * kTayStride, R(0));
    double worst_rel = 0.0;
    for (int cell = 0; cell < kTayCells; ++cell) {
        const double lo = cell * w, hi = (cell + 1) * w;
        const long double x0 = (long double)cell * w + 0.5L * w;
        for (int l = count_below(lo); l <= count_below(hi) && l <= nb; ++l) {
            const double* pay = pays[l].data();
            const uint8_t* ib = (const uint8_t*)(pay + kPayIdx);
            // the terms: Mach, d_a^2, coefficient
            long double m[2 * kPairs], dl2[2 * kPairs], cf[2 * kPairs], z2[2 * kPairs];
            int nt = 0;
            for (int k = 0; k < kPairs; ++k)
                for (int i = 0; i < 2; ++i) {
                    const double c = pay[2 * k + i];
                    if (c == 0.0) continue;
                    const bool g2 = i == 1 && slot_general(k);   // a general slot's second point
                    const int pidx = g2 ? ib[second_entry_pos(k)] : ib[pair_entry_pos(k)] + i;
                    const long double da = a - (long double)ib[g2 ? second_aoa_pos(k) : pair_aoa_pos(k)];
                    m[nt] = t.mach[pidx]; dl2[nt] = da * da; cf[nt] = c;
                    const long double u0 = x0 - m[nt];
                    z2[nt] = u0 * u0 + dl2[nt];
                    ++nt;
                }
            int ex[kTayExact];
            for (int e = 0; e < kTayExact; ++e) {
                int best = -1;
                for (int j = 0; j < nt; ++j) {
                    bool used = false;
                    for (int q = 0; q < e; ++q) used |= ex[q] == j;
                    if (!used && (best < 0 || z2[j] < z2[best])) best = j;
                }
                ex[e] = best;
            }
            long double B[kTayDeg + 1] = {};
            for (int j = 0; j < nt; ++j) {
                bool is_ex = false;
                for (int e = 0; e < kTayExact; ++e) is_ex |= ex[e] == j;
                if (is_ex) continue;
                const long double u0 = x0 - m[j], d = sqrtl(dl2[j]);
                // z^-k = conj(z)^k / |z|^(2k): real parts by the recurrence on (re, im)
                long double L[kTayDeg + 1];
                L[0] = logl(z2[j]);
                long double zr = 1.0L, zi = 0.0L;   // (conj(z) / |z|^2)^k
                const long double ir = u0 / z2[j], ii = -d / z2[j];
                for (int k = 1; k <= kTayDeg; ++k) {
                    const long double nr = zr * ir - zi * ii, ni = zr * ii + zi * ir;
                    zr = nr; zi = ni;
                    L[k] = 2.0L * ((k & 1) ? 1.0L : -1.0L) * zr / k;
                }
                const long double Q[3] = {z2[j], 2.0L * u0, 1.0L};
                for (int n = 0; n <= kTayDeg; ++n) {
                    long double b = 0.0L;
                    for (int q = 0; q < 3 && q <= n; ++q) b += Q[q] * L[n - q];
                    B[n] += 0.5L * cf[j] * b;
                }
            }
            const long double p0 = pay[kPayPoly], p1 = pay[kPayPoly + 1], p2 = pay[kPayPoly + 2];
            const long double sh0 = pay[kPaySS + 0], sh1 = pay[kPaySS + 1], sc0 = pay[kPaySS + 2], sc1 = pay[kPaySS + 3];
            B[0] += p0 + (x0 - sh0) / sc0 * p1 + (a - sh1) / sc1 * p2;
            B[1] += p1 / sc0;
            R* rec = out.data() + base + (size_t)(cell + l) * kTayStride;
            for (int n = 0; n <= kTayDeg; ++n) rec[n] = (R)B[n];
            for (int e = 0; e < kTayExact; ++e) {
                R* x = rec + kTayDeg + 1 + 3 * e;
                if (ex[e] < 0) { x[0] = R(0); x[1] = R(0); x[2] = R(1); continue; }
                x[0] = (R)m[ex[e]]; x[1] = (R)(cf[ex[e]] * 0.125L); x[2] = (R)dl2[ex[e]];
            }
            // check: five points of the piece's part of the cell
            const double plo = std::max(lo, l > 0 ? bp[l - 1] : lo), phi = std::min(hi, l < nb ? bp[l] : hi);
            for (int q = 0; q < 5; ++q) {
                const double M = plo + (phi - plo) * (0.02 + 0.24 * q);
                long double exact = p0 + ((long double)M - sh0) / sc0 * p1 + (a - sh1) / sc1 * p2, mag = 0.0L;
                for (int j = 0; j < nt; ++j) {
                    const long double dm = M - m[j], d2 = dm * dm + dl2[j];
                    const long double ph = d2 > 0 ? 0.5L * cf[j] * d2 * logl(d2) : 0.0L;
                    exact += ph; mag += fabsl(ph);
                }
                const double tt = M - (double)x0;
                double f = (double)rec[kTayDeg];
                for (int n = kTayDeg - 1; n >= 0; --n) f = std::fma(f, tt, (double)rec[n]);
                for (int e = 0; e < kTayExact; ++e) {
                    const R* x = rec + kTayDeg + 1 + 3 * e;
                    const double dm = M - (double)x[0], d2 = std::fma(dm, dm, (double)x[2]);
                    if (d2 > 0) f = std::fma((double)x[1] * d2, 4.0 * std::log(d2), f);
                }
                const double err = std::fabs(f - (double)exact);
                ts.max_abs = std::max(ts.max_abs, err);
                const double rel = err / (double)(mag + fabsl(exact) + 1e-300L);
                worst_rel = std::max(worst_rel, rel);
            }
            ++ts.pieces;
        }
    }
    ts.max_rel = std::max(ts.max_rel, worst_rel);
    const double lim = sizeof(R) == 8 ? 1e-13 : 1e-6;
    if (worst_rel > lim) { out.resize(base); return; }
    D.tay_off[li] = (int)(base / kTayStride);
}

// The same 50-NN key by selection instead of a full sort: the 50 smallest under the total order
// (distance, point index) are exactly stable_sort's first 50, so the key is host_knn_key's.
uint64_t knn_key_select(const pd_aero_table& t, double M, double a) {
    double d[PD_MAX_PTS];
    int id[PD_MAX_PTS], col[PD_MAX_PTS];
    int n = 0;
    for (int c = 0; c < t.n_cols; ++c)
        for (int k = 0; k < t.col_len[c]; ++k, ++n) {
            double dm = M - t.mach[t.col_start[c] + k], da = a - t.col_aoa[c];
            d[n] = dm * dm + da * da;
            id[n] = n;
            col[n] = c;
        }
    std::nth_element(id, id + (kNbr - 1), id + n, [&](int x, int y) { return d[x] < d[y] || (d[x] == d[y] && x < y); });
    int lo[kCols], hi[kCols];
    for (int c = 0; c < kCols; ++c) { lo[c] = 1 << 20; hi[c] = -1; }
    int base[kCols] = {0, 0, 0, 0, 0};
    for (int c = 1; c < t.n_cols; ++c) base[c] = base[c - 1] + t.col_len[c - 1];
    for (int j = 0; j < kNbr; ++j) {
        const int p = id[j], c = col[p], k = p - base[c];
        lo[c] = std::min(lo[c], k); hi[c] = std::max(hi[c], k);
    }
    int L[kCols], N[kCols];
    for (int c = 0; c < kCols; ++c) {
        if (hi[c] < 0) { L[c] = 0; N[c] = 0; } else { L[c] = lo[c]; N[c] = hi[c] - lo[c] + 1; }
    }
    return key_pack(L, N);
}

// Keys of one interior candidate grid: cell centres and corners, and for every cell whose
// corners disagree with its centre a kGridSub x kGridSub sub-grid (centres and corners).  Pure
// functions of the table, so they are computed once per process (threads over cells) and
// cached; slots are assigned per handle.
struct BisectHost { double nx, ny, c, tau; uint64_t key_a, key_b; bool ok_a, ok_b; };
struct GridKeys {
    int nm = 0, na = 0;
    std::vector<uint64_t> centre, corner;            // [nm][na], [nm + 1][na + 1]
    std::vector<int> refined;                        // cell index of each refined cell
    std::vector<uint64_t> sub_centre, sub_corner;    // [ref][S][S], [ref][S + 1][S + 1]
    std::vector<int> sub_bis;                        // [ref][S][S]: index into bis, -1 none
    std::vector<BisectHost> bis;
};

// The one point swap between two keys (A \ B = {p}, B \ A = {q}), as table point indices;
// false if the keys differ otherwise
bool single_swap(const pd_aero_table& t, uint64_t ka, uint64_t kb, int& p, int& q) {
    int la[kCols], na[kCols], lb[kCols], nb[kCols];
    key_unpack(ka, la, na);
    key_unpack(kb, lb, nb);
    int np = 0, nq = 0;
    p = q = -1;
    for (int c = 0; c < kCols; ++c) {
        for (int i = la[c]; i < la[c] + na[c]; ++i)
            if (!(nb[c] > 0 && i >= lb[c] && i < lb[c] + nb[c])) { ++np; p = t.col_start[c] + i; }
        for (int i = lb[c]; i < lb[c] + nb[c]; ++i)
            if (!(na[c] > 0 && i >= la[c] && i < la[c] + na[c])) { ++nq; q = t.col_start[c] + i; }
    }
    return np == 1 && nq == 1;
}
double point_aoa(const pd_aero_table& t, int idx) {
    int c = 0;
    while (c + 1 < t.n_cols && idx >= t.col_start[c + 1]) ++c;
    return t.col_aoa[c];
}

// Bisector record of a non-exact sub-cell [m0, m1] x [a0, a1] whose sample keys are {A, B} (see
// GridBisect): the bisector of the swapped points, and for each side whether its part of the
// cell, tau off the line, provably has the side's key (every vertex of the clipped polygon does).
bool make_bisect(const pd_aero_table& t, double m0, double m1, double a0, double a1, uint64_t ka, uint64_t kb,
                 BisectHost& out) {
    int p, q;
    if (!single_swap(t, ka, kb, p, q)) {
        if (!single_swap(t, kb, ka, p, q)) return false;
        std::swap(ka, kb);
    }
    const double pm = t.mach[p], pa = point_aoa(t, p), qm = t.mach[q], qa = point_aoa(t, q);
    out.nx = 2.0 * (qm - pm); out.ny = 2.0 * (qa - pa);
    out.c = (qm * qm + qa * qa) - (pm * pm + pa * pa);
    out.tau = 1e-9 * (std::fabs(out.nx) * 10.0 + std::fabs(out.ny) * 10.0 + std::fabs(out.c) + 1.0);
    out.key_a = ka; out.key_b = kb;
    auto side_ok = [&](double sign) {
        // the side's part of the cell kept 2 tau off the line (A: s <= -2 tau, B: s >= 2 tau) is
        // the convex polygon f <= 0; every vertex must carry the side's key (the device trusts
        // |s| > 3 tau, inside it)
        const double cx[4] = {m0, m1, m1, m0}, cy[4] = {a0, a0, a1, a1};
        std::vector<std::pair<double, double>> poly;
        auto f = [&](double x, double y) { return -sign * (out.nx * x + out.ny * y - out.c) + 2.0 * out.tau; };
        for (int k = 0; k < 4; ++k) {
            const int k1 = (k + 1) & 3;
            const double f0 = f(cx[k], cy[k]), f1 = f(cx[k1], cy[k1]);
            if (f0 <= 0) poly.push_back({cx[k], cy[k]});
            if ((f0 < 0) != (f1 < 0) && f0 != f1) {
                const double u = f0 / (f0 - f1);
                poly.push_back({cx[k] + u * (cx[k1] - cx[k]), cy[k] + u * (cy[k1] - cy[k])});
            }
        }
        if (poly.empty()) return false;
        const uint64_t want = sign < 0 ? ka : kb;
        for (auto& v : poly)
            if (knn_key_select(t, std::min(std::max(v.first, m0), m1), std::min(std::max(v.second, a0), a1)) != want)
                return false;
        return true;
    };
    out.ok_a = side_ok(-1.0);
    out.ok_b = side_ok(+1.0);
    return out.ok_a || out.ok_b;
}

template <typename F> void parallel_for(int64_t n, F f) {
    unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    if (n < 64) nt = 1;
    std::vector<std::thread> th;
    for (unsigned k = 0; k < nt; ++k)
        th.emplace_back([=] { for (int64_t i = (int64_t)k; i < n; i += nt) f(i); });
    for (auto& x : th) x.join();
}

const GridKeys& grid_keys(const pd_aero_table& t, double a0, double a1, int nm, int na) {
    static std::mutex mu;
    static std::map<uint64_t, GridKeys> cache;
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n) {
        for (size_t i = 0; i < n; ++i) { h ^= ((const uint8_t*)p)[i]; h *= 1099511628211ull; }
    };
    mix(&t, sizeof(t)); mix(&a0, 8); mix(&a1, 8); mix(&nm, 4); mix(&na, 4);
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(h);
    if (it != cache.end()) return it->second;
    GridKeys& g = cache[h];
    g.nm = nm; g.na = na;
    const double dm = 10.0 / nm, da = (a1 - a0) / na;
    const int S = kGridSub;
    g.corner.resize((size_t)(nm + 1) * (na + 1));
    g.centre.resize((size_t)nm * na);
    parallel_for(nm + 1, [&](int64_t im) {
        for (int ia = 0; ia <= na; ++ia) g.corner[(size_t)im * (na + 1) + ia] = knn_key_select(t, im * dm, a0 + ia * da);
        if (im < nm)
            for (int ia = 0; ia < na; ++ia)
                g.centre[(size_t)im * na + ia] = knn_key_select(t, (im + 0.5) * dm, a0 + (ia + 0.5) * da);
    });
    for (int im = 0; im < nm; ++im)
        for (int ia = 0; ia < na; ++ia) {
            const uint64_t key = g.centre[(size_t)im * na + ia];
            bool same = true;
            for (int c = 0; c < 4 && same; ++c) same = g.corner[(size_t)(im + (c >> 1)) * (na + 1) + ia + (c & 1)] == key;
            if (!same) g.refined.push_back(im * na + ia);
        }
    const int64_t nr = (int64_t)g.refined.size();
    g.sub_corner.resize((size_t)nr * (S + 1) * (S + 1));
    g.sub_centre.resize((size_t)nr * S * S);
    parallel_for(nr, [&](int64_t r) {
        const int im = g.refined[r] / na, ia = g.refined[r] % na;
        for (int jm = 0; jm <= S; ++jm)
            for (int ja = 0; ja <= S; ++ja) {
                g.sub_corner[((size_t)r * (S + 1) + jm) * (S + 1) + ja] =
                    knn_key_select(t, (im + (double)jm / S) * dm, a0 + (ia + (double)ja / S) * da);
                if (jm < S && ja < S)
                    g.sub_centre[((size_t)r * S + jm) * S + ja] =
                        knn_key_select(t, (im + (jm + 0.5) / S) * dm, a0 + (ia + (ja + 0.5) / S) * da);
            }
    });
    // non-exact sub-cells split by one bisector between two keys: records (threads per refined
    // cell, then gathered in order)
    g.sub_bis.assign((size_t)nr * S * S, -1);
    std::vector<std::vector<std::pair<int, BisectHost>>> found((size_t)nr);
    parallel_for(nr, [&](int64_t r) {
        const int im = g.refined[r] / na, ia = g.refined[r] % na;
        for (int jm = 0; jm < S; ++jm)
            for (int ja = 0; ja < S; ++ja) {
                const uint64_t kc = g.sub_centre[((size_t)r * S + jm) * S + ja];
                uint64_t other = kc;
                bool two = true, exact = true;
                for (int c = 0; c < 4 && two; ++c) {
                    const uint64_t k = g.sub_corner[((size_t)r * (S + 1) + jm + (c >> 1)) * (S + 1) + ja + (c & 1)];
                    if (k == kc) continue;
                    exact = false;
                    if (other == kc) other = k;
                    else if (k != other) two = false;
                }
                if (exact || !two) continue;
                BisectHost b;
                const double m0 = (im + (double)jm / S) * dm, m1 = (im + (double)(jm + 1) / S) * dm;
                const double c0 = a0 + (ia + (double)ja / S) * da, c1 = a0 + (ia + (double)(ja + 1) / S) * da;
                if (make_bisect(t, m0, m1, c0, c1, kc, other, b)) found[r].push_back({jm * S + ja, b});
            }
    });
    for (int64_t r = 0; r < nr; ++r)
        for (auto& fb : found[r]) {
            g.sub_bis[(size_t)r * S * S + fb.first] = (int)g.bis.size();
            g.bis.push_back(fb.second);
        }
    return g;
}

// Candidate grid over the interior query domain [0, 10] Mach x [a0, a1]: the 50-NN key at
// every cell centre, inserted into the table.  A 50-NN region is an intersection of
// half-planes (order-k Voronoi cell), hence convex: when all four corners of a cell carry the
// centre's key, the whole cell does, and the slot is flagged kGridExact so that device lookups
// skip the verification.  A cell whose corners disagree is refined into kGridSub x kGridSub
// sub-cells with the same construction (flagged kGridRefine, its sub-grid index in the low
// bits), so that only queries near a region boundary are verified on the device.
bool cell_ok(const CellPieces* cp, int64_t cell, bool f32);
bool fine_is(const CellPieces* cp, int im, int ia, int jm, int ja, int na, uint32_t want, bool f32);
int cell_bis(const CellPieces* cp, int bi, bool side_b, bool f32);

template <typename R>
pd_status build_grid(const pd_aero_table& t, double a0, double a1, int nm, int na, Table<R>& T,
                     std::vector<unsigned long long>& gk, std::vector<int>& gs,
                     std::vector<unsigned long long>& sk, std::vector<int>& ss, std::vector<GridBisect>& bs,
                     const CellPieces* cp = nullptr) {
    const GridKeys& g = grid_keys(t, a0, a1, nm, na);
    const int S = kGridSub;
    const bool f32 = sizeof(R) == 4;
    gk.assign((size_t)nm * na, 0); gs.assign((size_t)nm * na, -1);
    std::vector<double> work(kScratch), pay(kPay);
    auto slot_of = [&](uint64_t key, bool exact) {
        int slot = table_insert<R>(t, T, key, work, pay);
        return slot < 0 ? -1 : (slot | (exact ? kGridExact : 0));
    };
    for (int im = 0; im < nm; ++im)
        for (int ia = 0; ia < na; ++ia) {
            const uint64_t key = g.centre[(size_t)im * na + ia];
            gk[(size_t)im * na + ia] = key;
            gs[(size_t)im * na + ia] = slot_of(key, true);   // refined cells overwritten below
            if (gs[(size_t)im * na + ia] >= 0 && cell_ok(cp, (int64_t)im * na + ia, f32)) gs[(size_t)im * na + ia] |= kGridPiece;
        }
    const int64_t nr = (int64_t)g.refined.size();
    if (nr >= kGridRefine) return fail(PD_ERR_INVALID, "too many refined grid cells");
    sk.assign((size_t)nr * S * S, 0); ss.assign((size_t)nr * S * S, -1);
    for (int64_t r = 0; r < nr; ++r) {
        gs[g.refined[r]] = kGridRefine | (int)r;
        for (int jm = 0; jm < S; ++jm)
            for (int ja = 0; ja < S; ++ja) {
                const size_t q = ((size_t)r * S + jm) * S + ja;
                const uint64_t key = g.sub_centre[q];
                bool exact = true;
                for (int c = 0; c < 4 && exact; ++c)
                    exact = g.sub_corner[((size_t)r * (S + 1) + jm + (c >> 1)) * (S + 1) + ja + (c & 1)] == key;
                sk[q] = key;
                ss[q] = slot_of(key, exact);
                const int bi = g.sub_bis[q];
                // (binary32 handles read the bisector records through the fine index only: their
                // record path verifies refined cells)
                if (!exact && bi >= 0 && (sizeof(R) == 8 || cp) && bs.size() < (size_t)kGridBisect) {
                    const BisectHost& h = g.bis[bi];
                    GridBisect b{};
                    b.nx = h.nx; b.ny = h.ny; b.c = h.c; b.tau = h.tau; b.key_a = h.key_a; b.key_b = h.key_b;
                    const int sa = table_insert<R>(t, T, h.key_a, work, pay), sb = table_insert<R>(t, T, h.key_b, work, pay);
                    b.slot_a = sa < 0 ? -1 : (sa | (h.ok_a ? kGridExact : 0));
                    b.slot_b = sb < 0 ? -1 : (sb | (h.ok_b ? kGridExact : 0));
                    b.piece_a = cell_bis(cp, bi, false, f32); b.piece_b = cell_bis(cp, bi, true, f32);
                    if (cp && !fine_is(cp, g.refined[r] / na, g.refined[r] % na, jm, ja, na,
                                       kFineBisect | kFineRefined | (uint32_t)bs.size(), f32))
                        return fail(PD_ERR_INVALID, "cell pieces: fine index does not match the bisector records");
                    ss[q] = kGridBisect | (int)bs.size();
                    bs.push_back(b);
                }
            }
    }
    return PD_OK;
}

// ---------------------------------------------------------------- cell pieces
// Interior queries of the binary64 handle are evaluated from cell pieces (pd_step.h kCellDeg):
// for every interior grid cell and every neighbourhood that owns part of it, the thin-plate sum
// s(x) = sum_j c_j phi(|x - y_j|) + poly(x) of that neighbourhood restricted to the cell.  s is
// analytic over the cell except at the table points themselves (phi = r^2 log r), so the
// kCellExact points nearest to the cell centre stay exact terms and the rest, with scipy's
// degree-1 polynomial, is a polynomial of total degree kCellDeg in the cell coordinates (u, v) in
// [-1, 1]^2 (the device's 2 (M inv_dm - im) - 1 and 2 ((a - a0) inv_da - ia) - 1): the least-
// squares fit (long double Householder QR, once) on the cell's 10 x 10 tensor Chebyshev grid of
// the far terms evaluated there.  Every piece is then evaluated as the device does (binary64
// Horner, exact terms) at 8 quasi-random points of the cell and compared with the long double
// sum of all 50 terms: a piece whose error exceeds kCellTol relative to sum |c_j phi_j| is not
// used (the query goes to the payload sum).  Pure functions of the table and the grid: built once
// per process (threads over pieces) and cached, like the grid keys.
constexpr double kCellTol = 1e-14;
constexpr int kCellNodes = 10;

// binary32 pieces: error bound relative to sum |c_j phi_j| + |s| (the binary32 balanced payload
// sums, which these replace, round at ~50 eps_32 of the same scale)
constexpr double kCellTol32 = 2e-6;

// The fit operator: pinv[c][node] of the (node x coefficient) monomial design matrix, columns in
// record order (u^i v^j, i = kCellDeg .. 0, j = kCellDeg - i .. 0), nodes (k, l) -> (x_k, x_l)
const std::vector<long double>& cell_fit_operator() {
    static std::vector<long double> pinv;
    static std::once_flag once;
    std::call_once(once, [] {
        const int NN = kCellNodes * kCellNodes, NC = kCellCoef;
        long double x[kCellNodes];
        for (int k = 0; k < kCellNodes; ++k) x[k] = cosl((2 * k + 1) * 3.141592653589793238462643383279502884L / (2 * kCellNodes));
        std::vector<long double> A((size_t)NN * NC), Q((size_t)NN * NN, 0.0L);
        for (int k = 0; k < kCellNodes; ++k)
            for (int l = 0; l < kCellNodes; ++l) {
                int c = 0;
                for (int i = kCellDeg; i >= 0; --i)
                    for (int j = kCellDeg - i; j >= 0; --j) A[(size_t)(k * kCellNodes + l) * NC + c++] = powl(x[k], i) * powl(x[l], j);
            }
        for (int r = 0; r < NN; ++r) Q[(size_t)r * NN + r] = 1.0L;   // accumulates Q^T
        for (int c = 0; c < NC; ++c) {
            long double nrm = 0.0L;
            for (int r = c; r < NN; ++r) nrm += A[(size_t)r * NC + c] * A[(size_t)r * NC + c];
            nrm = sqrtl(nrm);
            const long double alpha = A[(size_t)c * NC + c] > 0 ? -nrm : nrm;
            std::vector<long double> v(NN, 0.0L);
            for (int r = c; r < NN; ++r) v[r] = A[(size_t)r * NC + c];
            v[c] -= alpha;
            long double vv = 0.0L;
            for (int r = c; r < NN; ++r) vv += v[r] * v[r];
            if (vv == 0.0L) continue;
            for (int cc = c; cc < NC; ++cc) {
                long double d = 0.0L;
                for (int r = c; r < NN; ++r) d += v[r] * A[(size_t)r * NC + cc];
                d = 2.0L * d / vv;
                for (int r = c; r < NN; ++r) A[(size_t)r * NC + cc] -= d * v[r];
            }
            for (int cc = 0; cc < NN; ++cc) {
                long double d = 0.0L;
                for (int r = c; r < NN; ++r) d += v[r] * Q[(size_t)r * NN + cc];
                d = 2.0L * d / vv;
                for (int r = c; r < NN; ++r) Q[(size_t)r * NN + cc] -= d * v[r];
            }
        }
        // R X = (Q^T)[0:NC]  ->  X = pinv
        pinv.assign((size_t)NC * NN, 0.0L);
        for (int cc = 0; cc < NN; ++cc)
            for (int c = NC - 1; c >= 0; --c) {
                long double s = Q[(size_t)c * NN + cc];
                for (int k = c + 1; k < NC; ++k) s -= A[(size_t)c * NC + k] * pinv[(size_t)k * NN + cc];
                pinv[(size_t)c * NN + cc] = s / A[(size_t)c * NC + c];
            }
    });
    return pinv;
}

// The terms of a neighbourhood's payload (Mach, AoA, coefficient) and its polynomial
struct NbrTerms {
    int nt = 0;
    double m[2 * kPairs], a[2 * kPairs], c[2 * kPairs];
    double p0 = 0, p1 = 0, p2 = 0, sh0 = 0, sh1 = 0, sc0 = 1, sc1 = 1;
    bool ok = false;
};
NbrTerms nbr_terms(const pd_aero_table& t, uint64_t key) {
    NbrTerms T;
    std::vector<double> work(kScratch), pay(kPay);
    double aoa[kCols];
    for (int c = 0; c < kCols; ++c) aoa[c] = t.col_aoa[c];
    if (solve_neighbourhood(t.mach, t.coef, t.col_start, aoa, key, work.data(), pay.data()) != 0) return T;
    const uint8_t* ib = (const uint8_t*)(pay.data() + kPayIdx);
    for (int k = 0; k < kPairs; ++k)
        for (int i = 0; i < 2; ++i) {
            const double c = pay[2 * k + i];
            if (c == 0.0) continue;
            const bool g2 = i == 1 && slot_general(k);
            T.m[T.nt] = t.mach[g2 ? ib[second_entry_pos(k)] : ib[pair_entry_pos(k)] + i];
            T.a[T.nt] = ib[g2 ? second_aoa_pos(k) : pair_aoa_pos(k)];
            T.c[T.nt] = c;
            ++T.nt;
        }
    T.p0 = pay[kPayPoly]; T.p1 = pay[kPayPoly + 1]; T.p2 = pay[kPayPoly + 2];
    T.sh0 = pay[kPaySS + 0]; T.sh1 = pay[kPaySS + 1]; T.sc0 = pay[kPaySS + 2]; T.sc1 = pay[kPaySS + 3];
    T.ok = true;
    return T;
}

// One piece: key's sum over cell (im, ia) into rec; returns the validation error (relative to
// sum |c_j phi_j|), or +inf if the neighbourhood did not solve
double make_cell_piece(const NbrTerms& T, int im, int ia, double dm, double da, double a0, double* rec,
                       double* scale = nullptr) {
    if (!T.ok) return INFINITY;
    const std::vector<long double>& pinv = cell_fit_operator();
    const double cm = (im + 0.5) * dm, ca = a0 + (ia + 0.5) * da, hm = 0.5 * dm, ha = 0.5 * da;
    // exact terms: the kCellExact nearest to the centre (ties by term order)
    int ex[kCellExact];
    bool is_ex[2 * kPairs] = {};
    for (int e = 0; e < kCellExact; ++e) {
        int best = -1;
        double bd = 0;
        for (int j = 0; j < T.nt; ++j) {
            if (is_ex[j]) continue;
            const double d = (cm - T.m[j]) * (cm - T.m[j]) + (ca - T.a[j]) * (ca - T.a[j]);
            if (best < 0 || d < bd) { best = j; bd = d; }
        }
        ex[e] = best;
        if (best >= 0) is_ex[best] = true;
    }
    const int NN = kCellNodes * kCellNodes;
    long double F[kCellNodes * kCellNodes];
    long double xn[kCellNodes];
    for (int k = 0; k < kCellNodes; ++k) xn[k] = cosl((2 * k + 1) * 3.141592653589793238462643383279502884L / (2 * kCellNodes));
    for (int k = 0; k < kCellNodes; ++k)
        for (int l = 0; l < kCellNodes; ++l) {
            const long double M = cm + xn[k] * hm, a = ca + xn[l] * ha;
            long double s = T.p0 + (M - T.sh0) / T.sc0 * T.p1 + (a - T.sh1) / T.sc1 * T.p2;
            for (int j = 0; j < T.nt; ++j) {
                if (is_ex[j]) continue;
                const long double dmj = M - T.m[j], daj = a - T.a[j], d2 = dmj * dmj + daj * daj;
                if (d2 > 0) s += 0.5L * T.c[j] * d2 * (long double)std::log((double)d2);
            }
            F[k * kCellNodes + l] = s;
        }
    for (int c = 0; c < kCellCoef; ++c) {
        long double s = 0.0L;
        for (int r = 0; r < NN; ++r) s += pinv[(size_t)c * NN + r] * F[r];
        rec[c] = (double)s;
    }
    for (int e = 0; e < kCellExact; ++e) {
        double* x = rec + kCellCoef + 3 * e;
        if (ex[e] < 0) { x[0] = 0.0; x[1] = 0.0; x[2] = 1e3; continue; }
        x[0] = T.m[ex[e]]; x[1] = T.c[ex[e]] * 0.125; x[2] = T.a[ex[e]];
    }
    for (int c = kCellCoef + 3 * kCellExact; c < kCellStride; ++c) rec[c] = 0.0;
    // validation: 8 Halton (2, 3) points of the cell, evaluated in the device's order
    double worst = 0.0;
    for (int q = 1; q <= 8; ++q) {
        double h2 = 0, h3 = 0, f2 = 0.5, f3 = 1.0 / 3;
        for (int n = q; n; n >>= 1, f2 *= 0.5) h2 += f2 * (n & 1);
        for (int n = q; n; n /= 3, f3 /= 3) h3 += f3 * (n % 3);
        const double u = 2 * h2 - 1, v = 2 * h3 - 1, M = cm + u * hm, a = ca + v * ha;
        double f = 0.0;
        int c = 0;
        for (int i = kCellDeg; i >= 0; --i) {
            double qi = rec[c++];
            for (int j = kCellDeg - i - 1; j >= 0; --j) qi = std::fma(qi, v, rec[c++]);
            f = i == kCellDeg ? qi : std::fma(f, u, qi);
        }
        for (int e = 0; e < kCellExact; ++e) {
            const double* x = rec + kCellCoef + 3 * e;
            const double dmx = M - x[0], dax = a - x[2], d2 = std::fma(dmx, dmx, dax * dax);
            if (d2 > 0) f = std::fma(x[1] * d2, 4.0 * std::log(d2), f);
        }
        long double exact = T.p0 + ((long double)M - T.sh0) / T.sc0 * T.p1 + ((long double)a - T.sh1) / T.sc1 * T.p2, mag = 0.0L;
        for (int j = 0; j < T.nt; ++j) {
            const long double dmj = M - T.m[j], daj = a - T.a[j], d2 = dmj * dmj + daj * daj;
            const long double ph = d2 > 0 ? 0.5L * T.c[j] * d2 * logl(d2) : 0.0L;
            exact += ph; mag += fabsl(ph);
        }
        worst = std::max(worst, (double)(fabsl((long double)f - exact) / (mag + fabsl(exact) + 1e-300L)));
        if (scale) *scale = std::max(*scale, (double)(mag + fabsl(exact)));
    }
    return worst;
}

// A piece record in binary32 (kCellStrideF floats, the key's bits at kCellKeyF) and its check:
// evaluated as the binary32 device does (Horner in fmaf, exact terms with the hardware log2) at
// the binary64 check's 8 points, against the binary64 record there; returns |error| / scale
double make_cell_piece_f32(const double* rec, int im, int ia, double dm, double da, double a0, double scale,
                           float* out) {
    for (int c = 0; c < kCellStrideF; ++c) out[c] = 0.0f;
    for (int c = 0; c < kCellKey; ++c) out[c] = (float)rec[c];
    std::memcpy(out + kCellKeyF, rec + kCellKey, 8);
    const double cm = (im + 0.5) * dm, ca = a0 + (ia + 0.5) * da, hm = 0.5 * dm, ha = 0.5 * da;
    double worst = 0.0;
    for (int q = 1; q <= 8; ++q) {
        double h2 = 0, h3 = 0, f2 = 0.5, f3 = 1.0 / 3;
        for (int n = q; n; n >>= 1, f2 *= 0.5) h2 += f2 * (n & 1);
        for (int n = q; n; n /= 3, f3 /= 3) h3 += f3 * (n % 3);
        const float u = (float)(2 * h2 - 1), v = (float)(2 * h3 - 1);
        const float M = (float)(cm + u * hm), a = (float)(ca + v * ha);
        float f = 0.0f;
        int c = 0;
        for (int i = kCellDeg; i >= 0; --i) {
            float qi = out[c++];
            for (int j = kCellDeg - i - 1; j >= 0; --j) qi = std::fma(qi, v, out[c++]);
            f = i == kCellDeg ? qi : std::fma(f, u, qi);
        }
        for (int e = 0; e < kCellExact; ++e) {
            const float* x = out + kCellCoef + 3 * e;
            const float dmx = M - x[0], dax = a - x[2], d2 = std::fma(dmx, dmx, dax * dax);
            f = std::fma(x[1] * d2, std::log2(d2 > 1e-30f ? d2 : 1e-30f) * (4.0f * 0.693147180559945309f), f);
        }
        // the binary64 record at the same point
        const double uu = u, vv = v, MM = M, aa = a;
        double g = 0.0;
        c = 0;
        for (int i = kCellDeg; i >= 0; --i) {
            double qi = rec[c++];
            for (int j = kCellDeg - i - 1; j >= 0; --j) qi = std::fma(qi, vv, rec[c++]);
            g = i == kCellDeg ? qi : std::fma(g, uu, qi);
        }
        for (int e = 0; e < kCellExact; ++e) {
            const double* x = rec + kCellCoef + 3 * e;
            const double dmx = MM - x[0], dax = aa - x[2], d2 = std::fma(dmx, dmx, dax * dax);
            if (d2 > 0) g = std::fma(x[1] * d2, 4.0 * std::log(d2), g);
        }
        worst = std::max(worst, std::fabs((double)f - g) / (scale + 1e-300));
    }
    return worst;
}

// The fine index of one precision's valid pieces (cell_ok, sub_piece) over the grid of cp
void build_fine(const CellPieces& cp, const std::vector<uint8_t>& cell_ok, const std::vector<int>& sub_piece,
                std::vector<uint32_t>& fine) {
    const int S = kGridSub, nm = cp.nm, na = cp.na;
    fine.assign((size_t)nm * S * na * S, 0u);
    parallel_for(nm, [&](int64_t im) {
        for (int ia = 0; ia < na; ++ia) {
            const int64_t c = im * na + ia;
            for (int jm = 0; jm < S; ++jm)
                for (int ja = 0; ja < S; ++ja) {
                    uint32_t e = 0u;
                    if (!cp.refined[c]) {
                        if (cell_ok[c]) e = kFinePiece | (uint32_t)c;
                    } else {
                        const size_t sq = (size_t)cp.ridx[c] * S * S + jm * S + ja;
                        if (sub_piece[sq] >= 0) e = kFinePiece | kFineRefined | (uint32_t)sub_piece[sq];
                        else if (cp.bs_of[sq] >= 0) e = kFineBisect | kFineRefined | (uint32_t)cp.bs_of[sq];
                    }
                    fine[(size_t)(im * S + jm) * ((size_t)na * S) + (size_t)ia * S + ja] = e;
                }
        }
    });
}

bool cell_ok(const CellPieces* cp, int64_t cell, bool f32) {
    return cp != nullptr && (f32 ? cp->cell_ok32[cell] : cp->cell_ok[cell]);
}
bool fine_is(const CellPieces* cp, int im, int ia, int jm, int ja, int na, uint32_t want, bool f32) {
    const int S = kGridSub;
    return (f32 ? cp->fine32 : cp->fine)[(size_t)(im * S + jm) * ((size_t)na * S) + (size_t)ia * S + ja] == want;
}
int cell_bis(const CellPieces* cp, int bi, bool side_b, bool f32) {
    if (cp == nullptr) return -1;
    if (f32) return side_b ? cp->bis_b32[bi] : cp->bis_a32[bi];
    return side_b ? cp->bis_b[bi] : cp->bis_a[bi];
}

template <typename R> void fill_params(const pd_params* p, const pd_config* c, DevParams<R>& D) {
    std::memset(&D, 0, sizeof(D));
    D.T_e = (R)p->thrust_per_engine; D.p_e = (R)p->nozzle_exit_pressure; D.A_e = (R)p->nozzle_exit_area;
    D.v_ex = (R)p->v_exhaust; D.S_gf = (R)p->grid_fin_area; D.d_base_gf = (R)p->d_base_grid_fin;
    D.R_rocket = (R)p->rocket_radius; D.A_front = (R)p->frontal_area; D.m_prop0 = (R)p->m_prop0;
    D.C_gust_x = (R)p->C_gust_x; D.C_gust_y = (R)p->C_gust_y; D.n_eng = p->n_engines_gimballed;
    // compile_physics constants (rockets_physics.py:808-835, 914-916), in binary64 as Python does
    double nom_pt = (0 * 0.4) / (double)p->n_engines_gimballed;
    double nom_lb = (3 * 0.4) / (double)p->n_engines_gimballed;
    double te_vex = p->thrust_per_engine / p->v_exhaust;
    double mg = 5.0 * kDeg2Rad, md = 20.0 * kDeg2Rad;
    D.f_Te_over_vex = (float)te_vex; D.f_one_minus_nom_pt = (float)(1 - nom_pt); D.f_nom_pt = (float)nom_pt;
    D.f_one_minus_nom_lb = (float)(1 - nom_lb); D.f_nom_lb = (float)nom_lb; D.f_dt_pt = (float)0.025;
    D.f_dt_lb = (float)0.1; D.f_max_gimbal_rad = (float)mg; D.f_max_defl_rad = (float)md;
    D.Te_over_vex = (R)te_vex; D.one_minus_nom_pt = (R)(1 - nom_pt); D.nom_pt = (R)nom_pt;
    D.one_minus_nom_lb = (R)(1 - nom_lb); D.nom_lb = (R)nom_lb; D.max_gimbal_rad = (R)mg;
    D.max_gimbal_deg = (R)(mg * kRad2Deg); D.max_defl_rad = (R)md;
    D.h_ox = (R)p->h_ox; D.h_f = (R)p->h_f; D.m_ox = (R)p->m_ox; D.m_f = (R)p->m_f; D.h_lower = (R)p->h_lower;
    D.m_dry = (R)p->m_dry; D.x_dry = (R)p->x_dry; D.I_dry = (R)p->I_dry; D.engine_height = (R)p->engine_height;
    D.cop = (R)p->cop;
    for (int k = 0; k < 9; ++k) {
        double b = p->isa_beta[k], Tb = p->isa_Tb[k];
        D.isa_Hb[k] = (R)p->isa_Hb[k]; D.isa_Tb[k] = (R)Tb; D.isa_beta[k] = (R)b; D.isa_pb[k] = (R)p->isa_pb[k];
        D.isa_bt[k] = (R)(b / Tb);
        D.isa_ex[k] = (R)(b != 0.0 ? -p->isa_g0 / (b * p->isa_R) : 0.0);
        D.isa_iso[k] = (R)(-p->isa_g0 / (p->isa_R * Tb));
    }
    D.isa_r = (R)p->isa_r; D.isa_R = (R)p->isa_R; D.isa_kappaR = (R)(p->isa_kappa * p->isa_R);
    D.isa_alt_max = (R)p->isa_alt_max; D.grav_R = (R)p->grav_R; D.grav_g0 = (R)p->grav_g0;
    for (int cc = 0; cc < kCols; ++cc) {
        D.cd_start[cc] = p->cd.col_start[cc]; D.cd_len[cc] = p->cd.col_len[cc]; D.cd_aoa[cc] = (R)p->cd.col_aoa[cc];
        D.cl_start[cc] = p->cl.col_start[cc]; D.cl_len[cc] = p->cl.col_len[cc]; D.cl_aoa[cc] = (R)p->cl.col_aoa[cc];
        D.cd_aoa_d[cc] = p->cd.col_aoa[cc]; D.cl_aoa_d[cc] = p->cl.col_aoa[cc];
    }
    D.cd_n = p->cd.n_pts; D.cl_n = p->cl.n_pts;
    for (int cc = 0; cc < kCols; ++cc) {
        for (int k = 0; k < p->cd.col_len[cc]; ++k) D.cd_pt_aoa[p->cd.col_start[cc] + k] = (R)p->cd.col_aoa[cc];
        for (int k = 0; k < p->cl.col_len[cc]; ++k) D.cl_pt_aoa[p->cl.col_start[cc] + k] = (R)p->cl.col_aoa[cc];
    }
    for (int k = 0; k < 256; ++k) {
        D.cd_mach[k] = (R)p->cd.mach[k]; D.cl_mach[k] = (R)p->cl.mach[k];
        D.cd_mach_d[k] = p->cd.mach[k]; D.cl_mach_d[k] = p->cl.mach[k];
        D.cd_coef_d[k] = p->cd.coef[k]; D.cl_coef_d[k] = p->cl.coef[k];
    }
    D.ca_n = p->ca_n; D.cn_n = p->cn_n;
    for (int k = 0; k < 64; ++k) {
        D.ca_x[k] = (R)p->ca_x[k]; D.ca_y[k] = (R)p->ca_y[k]; D.cn_x[k] = (R)p->cn_x[k]; D.cn_y[k] = (R)p->cn_y[k];
    }
    D.ca_min_mach = (R)p->ca_min_mach; D.ca_min_val = (R)p->ca_min_val;
    for (int b = 0; b < 64; ++b) {   // grid_fin_ca search buckets (handle-precision abscissae)
        const double w = 10.0 / 64, lo = b * w - 1e-4, hi = (b + 1) * w + 1e-4;
        int nlo = 0, nhi = 0;
        for (int k = 0; k < p->ca_n; ++k) { nlo += (double)D.ca_x[k] < lo; nhi += (double)D.ca_x[k] < hi; }
        D.ca_lb[b] = (uint16_t)(nlo | (nhi << 8));
    }
    D.cn_min_mach = (R)p->cn_min_mach; D.cn_max_mach = (R)p->cn_max_mach; D.cn_min_val = (R)p->cn_min_val;
    D.cn_max_val = (R)p->cn_max_val; D.cn_slope = (R)p->cn_slope;
    for (int w = 0; w < 50; ++w) {
        D.wind_n[w] = p->wind_n[w];
        for (int k = 0; k < 16; ++k) { D.wind_alt_km[w][k] = (R)p->wind_alt_km[w][k]; D.wind_speed[w][k] = (R)p->wind_speed[w][k]; }
    }
    for (int k = 0; k < 4; ++k) { D.vk_Ad_u[k] = (R)p->vk_Ad_u[k]; D.vk_Ad_v[k] = (R)p->vk_Ad_v[k]; }
    for (int k = 0; k < 2; ++k) { D.vk_Bd_u[k] = (R)p->vk_Bd_u[k]; D.vk_Bd_v[k] = (R)p->vk_Bd_v[k]; }
    D.vk_y_threshold = (R)p->vk_y_threshold;
    D.sigma_u_lo = p->sigma_u_lo; D.sigma_u_hi = p->sigma_u_hi; D.sigma_v_lo = p->sigma_v_lo; D.sigma_v_hi = p->sigma_v_hi;
    for (int k = 0; k < 11; ++k) { D.state0[k] = (R)p->state0[k]; D.state0_d[k] = p->state0[k]; }
    D.norm_y = (R)p->norm_y; D.norm_vy = (R)p->norm_vy; D.norm_x = (R)p->norm_x; D.norm_vx = (R)p->norm_vx;
    D.k_theta_pso = (R)(std::atanh(0.75) / (25.0 * kDeg2Rad));
    log_table_fill(D.logtab);
    log_table_fill(D.logtab_d);
    D.y0_rl = (R)p->state0[1]; D.m0_rl = (R)p->state0[8];
    // the divisors' correctly rounded reciprocals (div_known): one IEEE division each, in R
    D.inv_m_prop0 = R(1) / D.m_prop0; D.inv_y0_rl = R(1) / D.y0_rl; D.inv_m0_rl = R(1) / D.m0_rl;
    D.inv_norm_y = R(1) / D.norm_y; D.inv_norm_vy = R(1) / D.norm_vy; D.inv_norm_x = R(1) / D.norm_x;
    D.inv_norm_vx = R(1) / D.norm_vx;
    {
        const R b[7] = {D.m_prop0, D.y0_rl, D.m0_rl, D.norm_y, D.norm_vy, D.norm_x, D.norm_vx};
        const R rb[7] = {D.inv_m_prop0, D.inv_y0_rl, D.inv_m0_rl, D.inv_norm_y, D.inv_norm_vy, D.inv_norm_x, D.inv_norm_vx};
        D.div2 = 0;
        for (int k = 0; k < 7; ++k) if (!one_step_ok<R>(b[k], rb[k])) D.div2 |= 1u << k;
    }
    // ---- phase of the handle: its initial state, observation, and the constants of the
    // other compile_physics phases (rockets_physics.py:17-166,402-451,728-802,959-997)
    D.phase = c->phase;
    D.obs_kind = obs_kind_of(c->phase, c->rtd);
    if (c->phase >= PD_PHASE_PCONTROL)
        for (int k = 0; k < 11; ++k) { D.state0[k] = (R)p->state0_phase[c->phase][k]; D.state0_d[k] = p->state0_phase[c->phase][k]; }
    for (int k = 0; k < 13; ++k) D.fr[k] = (R)p->full_rocket[k];
    D.cop_ascent = (R)p->cop_ascent; D.n_eng_stage1 = p->n_engines_stage1;
    double mg_ascent = 7.0 * kDeg2Rad;
    D.mg_ascent = (R)mg_ascent; D.f_mg_ascent = (float)mg_ascent;
    D.kp_pc = (R)-0.08; D.f_kp_pc = (float)-0.08;
    D.rcs_force = (R)p->rcs_force; D.f_rcs_force = (float)p->rcs_force;
    D.rcs_d_bottom = (R)p->rcs_d_bottom; D.rcs_d_top = (R)p->rcs_d_top;
    // rl_wrapped_env_pytorch.augment_state (env_wrapped_rl_pytorch.py:178-194) constants
    D.f_k_theta_rl = (float)(std::atanh(0.75) / (5.0 * kDeg2Rad));
    D.f_k_thetad_rl = (float)(std::atanh(0.75) / 0.01);
    D.f_k_gamma_rl = (float)(std::atanh(0.75) / (5.0 * kDeg2Rad));
    D.f_pi_2 = (float)(kPi / 2); D.f_pi_3_2 = (float)(3.0 / 2 * kPi);
    for (int k = 0; k < 8; ++k) D.norm_ph[k] = (R)p->norm_phase[c->phase][k];
    int which = c->phase == PD_PHASE_SUPERSONIC ? 1 : 0;
    for (int r = 0; r < 12; ++r) for (int f = 0; f < 9; ++f) D.hyper[r][f] = (R)p->hyper[which][r][f];
    D.terminal_mach = (R)p->terminal_mach[which];
    D.n_ref = p->n_ref;
    // rtd_rl.py:267 (n-step scale, Python float ** int -> C pow), :472 (alive bonus), :250
    double g = c->discount_factor;
    D.rl_scale = (R)((1 - g) / (1 - std::pow(g, (double)c->trajectory_length)));
    D.alive_bonus = (R)(0.01 * (1 - g));
    D.log_1p_max_ae = (R)std::log(1 + 20.0 * kDeg2Rad);
}

}  // namespace

namespace pd {

// observation layout (obs_write) and widths of a (phase, rtd) pair
int obs_kind_of(int phase, int rtd) {
    if (rtd == PD_RTD_PSO) return phase == PD_PHASE_PURE_THROTTLE ? 1 : 2;
    switch (phase) {
        case PD_PHASE_PURE_THROTTLE: return 0;
        case PD_PHASE_LANDING_BURN: return 3;
        case PD_PHASE_PCONTROL: return 4;
        case PD_PHASE_BALLISTIC_ARC: return 5;
        case PD_PHASE_FLIP_OVER: return 6;
        default: return 7;
    }
}

// brute-force 50-NN key at a query (host), used for the initial cache and key checks
uint64_t host_knn_key(const pd_aero_table& t, double M, double a) {
    std::vector<std::pair<double, int>> d;
    for (int c = 0; c < t.n_cols; ++c)
        for (int k = 0; k < t.col_len[c]; ++k) {
            double dm = M - t.mach[t.col_start[c] + k], da = a - t.col_aoa[c];
            d.push_back({dm * dm + da * da, t.col_start[c] + k});
        }
    std::stable_sort(d.begin(), d.end(), [](auto& x, auto& y) { return x.first < y.first; });
    int lo[kCols], hi[kCols];
    for (int c = 0; c < kCols; ++c) { lo[c] = 1 << 20; hi[c] = -1; }
    for (int j = 0; j < kNbr; ++j) {
        int p = d[j].second, c = 0;
        while (c + 1 < t.n_cols && p >= t.col_start[c + 1]) ++c;
        int k = p - t.col_start[c];
        lo[c] = std::min(lo[c], k); hi[c] = std::max(hi[c], k);
    }
    int L[kCols], N[kCols];
    for (int c = 0; c < kCols; ++c) {
        if (hi[c] < 0) { L[c] = 0; N[c] = 0; } else { L[c] = lo[c]; N[c] = hi[c] - lo[c] + 1; }
    }
    return key_pack(L, N);
}

// rho, p, a as piecewise polynomials in the geometric altitude (atmosphere_tab, pd_physics.h):
// cells of kAtmW metres over [0, isa_alt_max); a cell holds its piece and, past a layer boundary
// inside it (H = Hb: a kink of T, and a jump of p by the rounding of the tabulated pb), a second
// piece, with the boundary's Hb as the split (record word 1).  Every piece is
// checked at 33 points in R arithmetic (the device's Horner order) against the long double ISA;
// the worst relative error goes to max_rel (binary64: 2e-16 typical, 2e-15 at worst next to a
// layer boundary -- the closed form's own binary64 rounding is up to 5e-15 there, the pow of
// 1 + b/Tb dH rounded once amplified by its exponent, about 34).
template <typename R>
void build_atm_table(const pd_params* P, std::vector<R>& out, int& n_cells, double& max_rel) {
    const double w = kAtmW, top = P->isa_alt_max;
    n_cells = (int)std::ceil(top / w);
    out.assign((size_t)n_cells * kAtmStride, R(0));
    max_rel = 0;
    const long double r = P->isa_r;
    auto layer_of = [&](long double y) {
        const long double H = r * y / (r + y);
        int i = 0;
        for (int k = 0; k < 9; ++k) if ((long double)P->isa_Hb[k] <= H) i = k;
        return i;
    };
    for (int k = 0; k < n_cells; ++k) {
        const long double lo = (long double)k * w, hi = std::min<long double>((long double)(k + 1) * w, top);
        const int il = layer_of(lo), ih = layer_of(hi - 1e-9L);
        long double split = hi;
        if (ih != il) {   // the boundary y of H = Hb[ih]: y = r Hb / (r - Hb)
            const long double Hb = P->isa_Hb[ih];
            split = r * Hb / (r - Hb);
        }
        for (int half = 0; half < (ih != il ? 2 : 1); ++half) {
            const long double a0 = half ? split : lo, a1 = half ? hi : split;
            const int li = half ? ih : il;
            R* rec = out.data() + (size_t)k * kAtmStride + half * kAtmRec;
            long double q[3][kAtmDeg + 1];
            for (int fn = 0; fn < 3; ++fn)
                fit_poly_ld([&](long double y) { const AtmLd v = atm_exact_ld(P, li, y);
                                                 return fn == 0 ? v.p : (fn == 1 ? v.rho : v.a); },
                            a0, a1, kAtmDeg, q[fn]);
            const long double c = (a0 + a1) / 2;
            rec[0] = (R)c;
            // the split as the layer's base H: the device takes the upper piece where the exact path
            // takes the upper layer, Hb <= r alt / (r + alt) in R (the ISA's pb are rounded
            // constants: p jumps by ~4e-6 across 47 km, so the side must be the exact path's)
            rec[1] = half || ih == il ? (R)1e30 : (R)P->isa_Hb[ih];
            for (int fn = 0; fn < 3; ++fn)
                for (int j = 0; j <= kAtmDeg; ++j) rec[2 + fn * (kAtmDeg + 1) + j] = (R)q[fn][j];
            for (int m = 0; m <= 32; ++m) {
                const long double y = a0 + (a1 - a0) * (m == 0 ? 1e-6L : (m == 32 ? 0.999999L : m / 32.0L));
                const AtmLd v = atm_exact_ld(P, li, y);
                const R t = (R)y - rec[0];
                const long double ex[3] = {v.p, v.rho, v.a};
                for (int fn = 0; fn < 3; ++fn) {
                    const R f = horner_host<R>(rec + 2 + fn * (kAtmDeg + 1), kAtmDeg, t);
                    max_rel = std::max(max_rel, (double)(fabsl((long double)f - ex[fn]) / fabsl(ex[fn])));
                }
            }
        }
        if (ih == il) {   // (no second piece: the split never triggers; mirror the first anyway)
            R* rec = out.data() + (size_t)k * kAtmStride;
            std::copy(rec, rec + kAtmRec, rec + kAtmRec);
        }
    }
}

// The coarse table of the 512-thread step kernels' LDS (pd_physics.h kAtl*, atmosphere_lds): the
// same method over cells of kAtlW metres at degree kAtlDeg.  Records [0, n_cells): the cells'
// pieces (of a cell holding a layer boundary the lower layer's, word 1 the boundary's Hb); then one
// record per boundary cell with its upper layer's piece, its index in the cell record's last word.
// out holds n_rec records; more than kAtlMaxCells of them (no such ISA): max_rel = infinity.
template <typename R>
void build_atm_lds_table(const pd_params* P, std::vector<R>& out, int& n_cells, int& n_rec, double& max_rel) {
    const double w = kAtlW, top = P->isa_alt_max;
    n_cells = (int)std::ceil(top / w);
    n_rec = n_cells;
    out.assign((size_t)n_cells * kAtlStride, R(0));
    max_rel = 0;
    const long double r = P->isa_r;
    auto layer_of = [&](long double y) {
        const long double H = r * y / (r + y);
        int i = 0;
        for (int k = 0; k < 9; ++k) if ((long double)P->isa_Hb[k] <= H) i = k;
        return i;
    };
    for (int k = 0; k < n_cells; ++k) {
        const long double lo = (long double)k * w, hi = std::min<long double>((long double)(k + 1) * w, top);
        const int il = layer_of(lo), ih = layer_of(hi - 1e-9L);
        // (a cell spans one boundary at most: the ISA's layers are kilometres apart)
        if (ih > il + 1) { max_rel = INFINITY; return; }
        long double split = hi;
        if (ih != il) {   // the boundary y of H = Hb[ih]: y = r Hb / (r - Hb)
            const long double Hb = P->isa_Hb[ih];
            split = r * Hb / (r - Hb);
        }
        for (int half = 0; half < (ih != il ? 2 : 1); ++half) {
            const long double a0 = half ? split : lo, a1 = half ? hi : split;
            const int li = half ? ih : il;
            if (half) { out.resize((size_t)(n_rec + 1) * kAtlStride, R(0)); }
            R* rec = out.data() + (size_t)(half ? n_rec : k) * kAtlStride;
            long double q[3][kAtlDeg + 1];
            for (int fn = 0; fn < 3; ++fn)
                fit_poly_ld([&](long double y) { const AtmLd v = atm_exact_ld(P, li, y);
                                                 return fn == 0 ? v.p : (fn == 1 ? v.rho : v.a); },
                            a0, a1, kAtlDeg, q[fn]);
            rec[0] = (R)((a0 + a1) / 2);
            // (the split as the layer's base H and the exact path's own test, as build_atm_table)
            rec[1] = half || ih == il ? (R)1e30 : (R)P->isa_Hb[ih];
            for (int fn = 0; fn < 3; ++fn)
                for (int j = 0; j <= kAtlDeg; ++j) rec[2 + fn * (kAtlDeg + 1) + j] = (R)q[fn][j];
            rec[kAtlRec - 1] = R(0);
            if (half) { out[(size_t)k * kAtlStride + kAtlRec - 1] = (R)n_rec; ++n_rec; }
            for (int m = 0; m <= 32; ++m) {
                const long double y = a0 + (a1 - a0) * (m == 0 ? 1e-6L : (m == 32 ? 0.999999L : m / 32.0L));
                const AtmLd v = atm_exact_ld(P, li, y);
                const R t = (R)y - rec[0];
                const long double ex[3] = {v.p, v.rho, v.a};
                for (int fn = 0; fn < 3; ++fn) {
                    const R f = horner_host<R>(rec + 2 + fn * (kAtlDeg + 1), kAtlDeg, t);
                    max_rel = std::max(max_rel, (double)(fabsl((long double)f - ex[fn]) / fabsl(ex[fn])));
                }
            }
        }
    }
    if (n_rec > kAtlMaxCells) max_rel = INFINITY;
}

// The interior candidate grid of table tb (0: C_D, 1: C_L): Mach [0, 10] x AoA abscissa [a0, a1]
// (C_D in [-radians(10), radians(10)], C_L in [0, 10]) in nm x na cells.  800 x 32 / 800 x 400
// cells, refined cells in 8 x 8 sub-cells, two-region sub-cells split by their bisector: < 0.1 %
// of queries verified (measured against 400 x 200 and 1600 x 800)
void grid_geometry(int tb, int& nm, int& na, double& a0, double& a1) {
    const int d[4] = {800, 32, 800, 400};
    nm = d[2 * tb]; na = d[2 * tb + 1];
    a0 = tb ? 0.0 : -10.0 * kDeg2Rad;
    a1 = tb ? 10.0 : 10.0 * kDeg2Rad;
}

const CellPieces& cell_pieces(const pd_aero_table& t, double a0, double a1, int nm, int na) {
    static std::mutex mu;
    static std::map<uint64_t, CellPieces> cache;
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n) {
        for (size_t i = 0; i < n; ++i) { h ^= ((const uint8_t*)p)[i]; h *= 1099511628211ull; }
    };
    mix(&t, sizeof(t)); mix(&a0, 8); mix(&a1, 8); mix(&nm, 4); mix(&na, 4);
    const GridKeys& g = grid_keys(t, a0, a1, nm, na);
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(h);
    if (it != cache.end()) return it->second;
    const auto t0 = std::chrono::steady_clock::now();
    CellPieces& cp = cache[h];
    const int S = kGridSub;
    const double dm = 10.0 / nm, da = (a1 - a0) / na;
    const int64_t ncell = (int64_t)nm * na, nr = (int64_t)g.refined.size();
    // the pieces: (cell, key) pairs -- exact cells at their index, then each refined cell's keys
    // (its exact sub-cells' and trusted bisector sides'), one piece per distinct key
    std::vector<std::pair<int, uint64_t>> job((size_t)ncell);
    std::vector<uint8_t> refined(ncell, 0);
    for (int r : g.refined) refined[r] = 1;
    for (int64_t c = 0; c < ncell; ++c) job[c] = {(int)c, g.centre[c]};
    cp.sub_piece.assign((size_t)nr * S * S, -1);
    cp.bis_a.assign(g.bis.size(), -1);
    cp.bis_b.assign(g.bis.size(), -1);
    for (int64_t r = 0; r < nr; ++r) {
        std::map<uint64_t, int> own;
        auto piece_of = [&](uint64_t key) {
            auto f = own.find(key);
            if (f != own.end()) return f->second;
            const int p = (int)job.size();
            job.push_back({g.refined[r], key});
            own[key] = p;
            return p;
        };
        const int im = g.refined[r] / na, ia = g.refined[r] % na;
        (void)im; (void)ia;
        for (int q = 0; q < S * S; ++q) {
            const size_t sq = (size_t)r * S * S + q;
            const int jm = q / S, ja = q % S;
            const uint64_t key = g.sub_centre[sq];
            bool exact = true;
            for (int c = 0; c < 4 && exact; ++c)
                exact = g.sub_corner[((size_t)r * (S + 1) + jm + (c >> 1)) * (S + 1) + ja + (c & 1)] == key;
            if (exact) cp.sub_piece[sq] = piece_of(key);
            const int bi = g.sub_bis[sq];
            if (!exact && bi >= 0) {
                if (g.bis[bi].ok_a) cp.bis_a[bi] = piece_of(g.bis[bi].key_a);
                if (g.bis[bi].ok_b) cp.bis_b[bi] = piece_of(g.bis[bi].key_b);
            }
        }
    }
    // the neighbourhoods' terms, solved once per key
    std::map<uint64_t, int> kidx;
    std::vector<uint64_t> keys;
    for (auto& j : job)
        if (kidx.emplace(j.second, (int)keys.size()).second) keys.push_back(j.second);
    std::vector<NbrTerms> terms(keys.size());
    parallel_for((int64_t)keys.size(), [&](int64_t k) { terms[k] = nbr_terms(t, keys[k]); });
    cell_fit_operator();
    cp.rec.assign(job.size() * kCellStride, 0.0);
    cp.err.assign(job.size(), INFINITY);
    cp.scale.assign(job.size(), 0.0);
    cp.cell_of.resize(job.size());
    std::vector<double>& err = cp.err;
    parallel_for((int64_t)job.size(), [&](int64_t p) {
        const int c = job[p].first;
        cp.cell_of[p] = c;
        if (p < ncell && refined[c]) { err[p] = INFINITY; return; }   // (a refined cell's own index: unused)
        double* rec = cp.rec.data() + (size_t)p * kCellStride;
        err[p] = make_cell_piece(terms[kidx.at(job[p].second)], c / na, c % na, dm, da, a0, rec, &cp.scale[p]);
        const uint64_t key = job[p].second;
        std::memcpy(rec + kCellKey, &key, 8);
    });
    auto valid = [&](int p) { return p >= 0 && err[p] <= kCellTol; };
    cp.cell_ok.assign(ncell, 0);
    for (int64_t c = 0; c < ncell; ++c) cp.cell_ok[c] = !refined[c] && valid((int)c);
    for (auto& s : cp.sub_piece) if (!valid(s)) s = -1;
    for (auto& s : cp.bis_a) if (!valid(s)) s = -1;
    for (auto& s : cp.bis_b) if (!valid(s)) s = -1;
    for (size_t p = 0; p < job.size(); ++p) {
        if ((int64_t)p < ncell && refined[job[p].first]) continue;
        ++cp.pieces;
        if (err[p] <= kCellTol) cp.max_rel = std::max(cp.max_rel, err[p]);
        else ++cp.rejected;
    }
    // the fine index: per sub-cell of every cell the piece all its points use, or the bisector
    // record splitting it (numbered as build_grid numbers them: refined cells, then sub-cells in
    // order, every non-exact sub-cell with a bisector)
    cp.nm = nm; cp.na = na; cp.a0 = a0; cp.dm = dm; cp.da = da;
    cp.refined = refined;
    cp.ridx.assign(ncell, -1);
    for (int64_t r = 0; r < nr; ++r) cp.ridx[g.refined[r]] = (int)r;
    cp.bs_of.assign((size_t)nr * S * S, -1);
    {
        int64_t nbs = 0;
        for (int64_t r = 0; r < nr; ++r)
            for (int q = 0; q < S * S; ++q) {
                const size_t sq = (size_t)r * S * S + q;
                const int jm = q / S, ja = q % S;
                bool exact = true;
                for (int c = 0; c < 4 && exact; ++c)
                    exact = g.sub_corner[((size_t)r * (S + 1) + jm + (c >> 1)) * (S + 1) + ja + (c & 1)] == g.sub_centre[sq];
                if (!exact && g.sub_bis[sq] >= 0 && nbs < (int64_t)kGridBisect) cp.bs_of[sq] = nbs++;
            }
    }
    build_fine(cp, cp.cell_ok, cp.sub_piece, cp.fine);
    cp.build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return cp;
}

// The binary32 variant of cp (once per process and table): every binary64-valid piece rounded to
// floats and checked in binary32 (make_cell_piece_f32); the pieces within kCellTol32 keep their
// places, the others drop out of the binary32 validity, sub-cell, bisector and fine-index tables
// (their queries take the record path: verified, payload sums)
void ensure_f32(CellPieces& cp) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (cp.have32) return;
    const int64_t np = (int64_t)cp.err.size();
    cp.rec32.assign((size_t)np * kCellStrideF, 0.0f);
    std::vector<double> e32(np, INFINITY);
    parallel_for(np, [&](int64_t p) {
        if (!(cp.err[p] <= kCellTol)) return;
        const int c = cp.cell_of[p];
        e32[p] = make_cell_piece_f32(cp.rec.data() + (size_t)p * kCellStride, c / cp.na, c % cp.na, cp.dm, cp.da,
                                     cp.a0, cp.scale[p], cp.rec32.data() + (size_t)p * kCellStrideF);
    });
    auto ok = [&](int p) { return p >= 0 && e32[p] <= kCellTol32; };
    const int64_t ncell = (int64_t)cp.cell_ok.size();
    cp.cell_ok32.assign(ncell, 0);
    for (int64_t c = 0; c < ncell; ++c) cp.cell_ok32[c] = cp.cell_ok[c] && ok((int)c);
    cp.sub_piece32 = cp.sub_piece; cp.bis_a32 = cp.bis_a; cp.bis_b32 = cp.bis_b;
    for (auto* v : {&cp.sub_piece32, &cp.bis_a32, &cp.bis_b32})
        for (auto& x : *v) if (!ok(x)) x = -1;
    for (int64_t p = 0; p < np; ++p) {
        if (!(cp.err[p] <= kCellTol)) continue;
        if (e32[p] <= kCellTol32) cp.max_rel32 = std::max(cp.max_rel32, e32[p]);
        else ++cp.rejected32;
    }
    build_fine(cp, cp.cell_ok32, cp.sub_piece32, cp.fine32);
    cp.have32 = true;
}

// ---------------------------------------------------------------- a handle's tables
template <typename R> pd_status build_host_tables(const pd_params* p, const pd_config* c, HostTables<R>& H) {
    DevParams<R>& D = H.D;
    fill_params<R>(p, c, D);
    Table<R>&tcd = H.cd, &tcl = H.cl;
    pd_status st;
    if ((st = build_table<R>(p->cd, p->keys_cd, p->n_keys_cd, tcd)) != PD_OK) return st;
    if ((st = build_table<R>(p->cl, p->keys_cl, p->n_keys_cl, tcl)) != PD_OK) return st;
    // clamped query lines: C_D at +-radians(10) (aerodynamic_coefficients.py:108-114), C_L at
    // +-10 (:122-125); the device computes these abscissae with the same expressions
    if ((st = build_line<R>(p->cd, 10.0 * kDeg2Rad, tcd, 0, D)) != PD_OK) return st;
    if ((st = build_line<R>(p->cd, -10.0 * kDeg2Rad, tcd, 1, D)) != PD_OK) return st;
    if ((st = build_line<R>(p->cl, 10.0, tcl, 2, D)) != PD_OK) return st;
    if ((st = build_line<R>(p->cl, -10.0, tcl, 3, D)) != PD_OK) return st;
    // Taylor pieces of the lines (evaluated instead of the payload sums by the LPE-2 kernels)
    TayStats tst;
    for (int li = 0; li < 4; ++li) build_taylor<R>(li < 2 ? p->cd : p->cl, li, D, H.tay, tst);
    const bool verbose = (c->table_flags & PD_TABLES_VERBOSE) != 0;
    if (verbose)
        fprintf(stderr, "pdenv taylor: %lld pieces, max abs err %.3g, max rel err %.3g, lines %d %d %d %d\n",
                (long long)tst.pieces, tst.max_abs, tst.max_rel, D.tay_off[0], D.tay_off[1], D.tay_off[2], D.tay_off[3]);
    // the atmosphere as piecewise polynomials (PD_TABLES_EXACT_ATMOSPHERE: the exact formulas on the device)
    if (!(c->table_flags & PD_TABLES_EXACT_ATMOSPHERE)) {
        int n_atm = 0;
        double err_atm = 0;
        build_atm_table<R>(p, H.atm, n_atm, err_atm);
        if (verbose) fprintf(stderr, "pdenv atmosphere table: %d cells, max rel err %.3g\n", n_atm, err_atm);
        // (else: the exact formulas; binary32: its y rounds by 8 mm at 80 km, 1e-6 of p)
        if (err_atm <= (sizeof(R) == 8 ? 1e-14 : 4e-6)) { D.atm_n = n_atm; D.atm_inv_w = (R)(1.0 / kAtmW); }
        else H.atm.clear();
    }
    // the coarse table of the 512-thread step kernels' LDS image (binary64 wind handles: c3);
    // PD_TABLES_NO_ATM_LDS or a table past 1e-14: none, those kernels take the exact formulas
    D.atl_n = 0; D.atl_inv_w = (R)(1.0 / kAtlW);
    if constexpr (sizeof(R) == 8) if (c->enable_wind && !(c->table_flags & PD_TABLES_NO_ATM_LDS)) {
        int n_cells = 0, n_rec = 0;
        double err_atl = 0;
        build_atm_lds_table<R>(p, H.atl, n_cells, n_rec, err_atl);
        if (verbose) fprintf(stderr, "pdenv LDS atmosphere table: %d cells, %d records, max rel err %.3g\n", n_cells, n_rec, err_atl);
        if (err_atl <= 1e-14) D.atl_n = n_cells;
        else H.atl.clear();
    }
    // interior candidate grids: C_D abscissa in [-radians(10), radians(10)], C_L in [0, 10]
    for (int tb = 0; tb < 2; ++tb) grid_geometry(tb, H.grid[tb].nm, H.grid[tb].na, H.grid[tb].a0, H.grid[tb].a1);
    // cell pieces for the interior queries (PD_TABLES_NO_CELL_PIECES: payload sums only): binary64
    // records for binary64 handles, their binary32 roundings (each checked in binary32,
    // ensure_f32) for binary32 handles
    if (!(c->table_flags & PD_TABLES_NO_CELL_PIECES))
        for (int tb = 0; tb < 2; ++tb) {
            const auto& G = H.grid[tb];
            CellPieces* cp = const_cast<CellPieces*>(&cell_pieces(tb ? p->cl : p->cd, G.a0, G.a1, G.nm, G.na));
            if (sizeof(R) == 4) ensure_f32(*cp);
            H.grid[tb].pieces = cp;
        }
    for (int tb = 0; tb < 2; ++tb) {
        auto& G = H.grid[tb];
        if ((st = build_grid<R>(tb ? p->cl : p->cd, G.a0, G.a1, G.nm, G.na, tb ? tcl : tcd, G.key, G.slot, G.sub_key,
                                G.sub_slot, G.bis, G.pieces)) != PD_OK) return st;
    }
    if (verbose)
        for (int tb = 0; tb < 2; ++tb) {
            const auto& G = H.grid[tb];
            int64_t nref = 0, nne = 0, nce = 0;
            for (int v : G.slot) { nref += v >= 0 && (v & kGridRefine); nce += v >= 0 && !(v & kGridRefine) && !(v & kGridExact); }
            int64_t nbs = 0, nbs2 = 0;
            for (int v : G.sub_slot) nne += v < 0 || !(v & kGridExact);
            for (auto& b : G.bis) { nbs += 1; nbs2 += (b.slot_a >= 0 && (b.slot_a & kGridExact)) + (b.slot_b >= 0 && (b.slot_b & kGridExact)); }
            fprintf(stderr, "pdenv grid %d: %lld bisector sub-cells, %lld trusted sides\n", tb, (long long)nbs, (long long)nbs2);
            if (G.pieces) fprintf(stderr, "pdenv grid %d: %lld cell pieces (%.1f MB), %lld rejected, max error %.2e of sum |c phi|, built in %.2f s\n", tb,
                                  (long long)G.pieces->pieces, G.pieces->rec.size() * 8e-6, (long long)G.pieces->rejected, G.pieces->max_rel, G.pieces->build_s);
            fprintf(stderr, "pdenv grid %d: %d x %d cells, %lld refined, %lld non-exact cells, %lld of %zu sub-cells non-exact\n", tb,
                    G.nm, G.na, (long long)nref, (long long)nce, (long long)nne, G.sub_slot.size());
        }
    for (int tb = 0; tb < 2; ++tb) {
        const auto& G = H.grid[tb];
        D.grid_nm[tb] = G.nm; D.grid_na[tb] = G.na; D.grid_a0[tb] = (R)G.a0;
        D.grid_inv_da[tb] = (R)(G.na / (G.a1 - G.a0)); D.grid_inv_dm[tb] = (R)(G.nm / 10.0);
    }
    D.logcap_cd = tcd.logcap; D.logcap_cl = tcl.logcap;
    // initial neighbourhood caches: the 50-NN at the initial state's clamped query points
    // (any valid 50-set works; the in-kernel swap search repairs it)
    D.init_key_cd = host_knn_key(p->cd, 3.0, 0.0);
    D.init_key_cl = host_knn_key(p->cl, 3.0, 10.0);
    return PD_OK;
}
template pd_status build_host_tables<double>(const pd_params*, const pd_config*, HostTables<double>&);
template pd_status build_host_tables<float>(const pd_params*, const pd_config*, HostTables<float>&);
template void build_atm_table<double>(const pd_params*, std::vector<double>&, int&, double&);
template void build_atm_table<float>(const pd_params*, std::vector<float>&, int&, double&);
template void build_atm_lds_table<double>(const pd_params*, std::vector<double>&, int&, int&, double&);

}  // namespace pd
