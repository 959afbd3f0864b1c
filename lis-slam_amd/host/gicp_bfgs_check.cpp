// gicp_bfgs_check.cpp — the host half of PCL's GICP (../csrc/lisreg_gicp_host.hpp) on its own: plain C++, no library, no
// device.  Random pair sets with random positive definite M; the 74 moments formed here in plain loops; then
//   * f and grad f from the moments against the per-pair sums and against central differences of f,
//   * the inner BFGS from a perturbed state: f never rises over the accepted steps, every successful line search satisfies both of
//     Fletcher's tests, no line search takes more than its 100 trials, the result is no worse than the start,
//   * scripted 1-D problems for the exits the random sets do not reach (a start at the minimiser, slopes below the rounding of the
//     no-progress test, an iteration cap of 2),
// and a census of the branches taken, printed.  Exit 0 and "gicp_bfgs_check ok" if everything holds.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "lisreg_gicp_host.hpp"

using namespace lisreg::gicp_host;

namespace {

struct Pair { double p[3], q[3], M[6]; };

int failures = 0;
void expect(bool ok, const char* what, double a = 0.0, double b = 0.0)
{
    if (!ok) { ++failures; std::printf("FAILED: %s (%.17g, %.17g)\n", what, a, b); }
}

// the record of the pairs at the outer iterate xk (G = identity), about c — the order of tests/gicp_ref.py
void moments_of(const std::vector<Pair>& pairs, const double xk[6], const double c[3], double rec[kRec])
{
    double R[9];
    euler_R(xk, R);
    for (int k = 0; k < kRec; ++k) rec[k] = 0.0;
    for (const Pair& P : pairs) {
        double xp[3], yt[4], r[3], Mr[3];
        for (int a = 0; a < 3; ++a) xp[a] = ((R[3 * a] * P.p[0] + R[3 * a + 1] * P.p[1]) + R[3 * a + 2] * P.p[2]) + xk[a];
        for (int a = 0; a < 3; ++a) { yt[a] = xp[a] - c[a]; r[a] = xp[a] - P.q[a]; }
        yt[3] = 1.0;
        for (int a = 0; a < 3; ++a) Mr[a] = (P.M[kSym3[a][0]] * r[0] + P.M[kSym3[a][1]] * r[1]) + P.M[kSym3[a][2]] * r[2];
        rec[0] += (r[0] * Mr[0] + r[1] * Mr[1]) + r[2] * Mr[2];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 4; ++b) rec[1 + 4 * a + b] += Mr[a] * yt[b];
        for (int p = 0; p < 6; ++p)
            for (int b = 0; b < 4; ++b)
                for (int b2 = b; b2 < 4; ++b2) rec[13 + 10 * p + kSym4[b][b2]] += P.M[p] * (yt[b] * yt[b2]);
        rec[73] += 1.0;
    }
}

// PCL's literal sums at x
double pair_form(const std::vector<Pair>& pairs, const double x[6], double g[6])
{
    double R[9], dR[3][9];
    euler_R(x, R);
    euler_dR(x, dR);
    const double m = (double)pairs.size();
    double f = 0.0;
    for (int k = 0; k < 6; ++k) g[k] = 0.0;
    for (const Pair& P : pairs) {
        double res[3], Mres[3];
        for (int a = 0; a < 3; ++a) res[a] = ((R[3 * a] * P.p[0] + R[3 * a + 1] * P.p[1]) + R[3 * a + 2] * P.p[2]) + x[a] - P.q[a];
        for (int a = 0; a < 3; ++a) Mres[a] = (P.M[kSym3[a][0]] * res[0] + P.M[kSym3[a][1]] * res[1]) + P.M[kSym3[a][2]] * res[2];
        f += (res[0] * Mres[0] + res[1] * Mres[1]) + res[2] * Mres[2];
        for (int a = 0; a < 3; ++a) g[a] += 2.0 * Mres[a];
        for (int j = 0; j < 3; ++j)
            for (int a = 0; a < 3; ++a)
                g[3 + j] += 2.0 * ((dR[j][3 * a] * P.p[0] + dR[j][3 * a + 1] * P.p[1]) + dR[j][3 * a + 2] * P.p[2]) * Mres[a];
    }
    for (int k = 0; k < 6; ++k) g[k] /= m;
    return f / m;
}

// what every run of bfgs_minimise must satisfy, from its census
void check_run(const Census& cs, const InnerCounts& cnt, double f_start, double f_end, const BfgsParams& P)
{
    expect(cnt.exit >= kExitGradient && cnt.exit <= kExitNoProgress, "exit code", cnt.exit);
    expect(cnt.iters >= 1 && cnt.iters <= P.max_inner_iters, "iteration count", cnt.iters, P.max_inner_iters);
    expect(cs.max_trials <= 100, "a line search took more than 100 trials", cs.max_trials);
    expect(f_end <= f_start, "the result is worse than the start", f_start, f_end);
    expect(cs.n_steps == (cnt.exit == kExitNoProgress ? cnt.iters - 1 : cnt.iters), "steps against iterations", cs.n_steps, cnt.iters);
    double prev = f_start;
    for (int s = 0; s < std::min(cs.n_steps, (int)Census::kMaxSteps); ++s) {
        const Step& st = cs.steps[s];
        expect(st.f0 == prev, "a step does not start where the last one ended", st.f0, prev);
        expect(st.f <= st.f0, "f rose over an accepted step", st.f0, st.f);
        expect(st.fp0 < 0.0 && st.alpha > 0.0, "not a descent direction", st.fp0, st.alpha);
        if (st.trials < 100) {                                      // (a search that spent its trials returns its last alpha untested)
            expect(st.f <= st.f0 + P.rho * st.alpha * st.fp0, "Fletcher's rho test on Success", st.f, st.f0 + P.rho * st.alpha * st.fp0);
            expect(fabs(st.fp) <= -P.sigma * st.fp0, "Fletcher's sigma test on Success", st.fp, -P.sigma * st.fp0);
        }
        prev = st.f;
    }
    if (cs.n_steps <= Census::kMaxSteps) expect(prev == f_end, "the last step's f is not the result's", prev, f_end);
}

}  // namespace

int main()
{
    const BfgsParams P0{ 0.01, 0.01, 9.0, 0.05, 0.5, 0.01, 1.0e-2, 3, 20 };
    std::mt19937_64 rng(20260);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    Census total;
    double worst_f = 0.0, worst_g = 0.0, worst_fd = 0.0;
    int runs = 0;
    for (int set = 0; set < 60; ++set) {
        const int m = set < 4 ? 4 + set : 50 + 37 * set;            // from PCL's minimum of 4 pairs up
        const double noise = set % 3 == 0 ? 0.0 : 0.02;
        const double truth[6] = { 0.3 * U(rng), 0.3 * U(rng), 0.1 * U(rng), 0.03 * U(rng), 0.03 * U(rng), 0.05 * U(rng) };
        double Rt[9];
        euler_R(truth, Rt);
        std::vector<Pair> pairs((size_t)m);
        for (Pair& Q : pairs) {
            for (int a = 0; a < 3; ++a) Q.p[a] = (a == 2 ? 3.0 : 25.0) * U(rng) + (a == 0 ? 40.0 : 0.0);    // a map-frame box away from the origin
            for (int a = 0; a < 3; ++a) Q.q[a] = ((Rt[3 * a] * Q.p[0] + Rt[3 * a + 1] * Q.p[1]) + Rt[3 * a + 2] * Q.p[2]) + truth[a] + noise * N(rng);
            // M = (I - (1 - eps) n n^T)^-1 / 2 of a random plane normal: eigenvalues 0.5, 0.5, 500
            double n[3] = { N(rng), N(rng), N(rng) };
            const double nn = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            for (int a = 0; a < 3; ++a) n[a] /= nn;
            int k = 0;
            for (int a = 0; a < 3; ++a)
                for (int b = a; b < 3; ++b) Q.M[k++] = 0.5 * ((a == b ? 1.0 : 0.0) + 999.0 * n[a] * n[b]);
        }
        const double c[3] = { 40.0 + 2.0 * U(rng), 2.0 * U(rng), U(rng) };
        double xk[6];
        for (int j = 0; j < 6; ++j) xk[j] = truth[j] + (j < 3 ? 0.2 : 0.03) * U(rng) * (set % 5 == 4 ? 1.0e-3 : 1.0);
        double rec[kRec];
        moments_of(pairs, xk, c, rec);
        // ---- the moment form against the per-pair form and against central differences, at states 1e0 .. 1e-6 of (0.3 m, 2 deg) away
        for (int trial = 0; trial < 4; ++trial) {
            const double scale = pow(10.0, -2.0 * trial);
            double x[6], g[6], g2[6];
            for (int j = 0; j < 6; ++j) x[j] = xk[j] + scale * (j < 3 ? 0.3 : 0.035) * U(rng);
            const double f = fdf(rec, c, xk, x, g), f2 = pair_form(pairs, x, g2);
            expect(fdf(rec, c, xk, x, nullptr) == f, "f with and without the gradient", f);
            double gmax = 0.0;
            for (int j = 0; j < 6; ++j) gmax = std::max(gmax, fabs(g2[j]));
            if (f2 > 0.0) worst_f = std::max(worst_f, fabs(f - f2) / f2);
            for (int j = 0; j < 6; ++j) {
                if (gmax > 0.0) worst_g = std::max(worst_g, fabs(g[j] - g2[j]) / gmax);
                const double h = j < 3 ? 1.0e-5 : 1.0e-6;
                double xp[6], xm[6];
                for (int i = 0; i < 6; ++i) xp[i] = xm[i] = x[i];
                xp[j] += h; xm[j] -= h;
                const double num = (fdf(rec, c, xk, xp, nullptr) - fdf(rec, c, xk, xm, nullptr)) / (xp[j] - xm[j]);
                if (gmax > 1.0e-3) worst_fd = std::max(worst_fd, fabs(num - g[j]) / gmax);
            }
        }
        // ---- the inner BFGS from the outer iterate, with PCL's settings and with a tight tolerance and many iterations
        for (int variant = 0; variant < 2; ++variant) {
            BfgsParams P = P0;
            if (variant) { P.gradient_tol = 1.0e-7; P.max_inner_iters = 200; }
            Census cs;
            InnerCounts cnt;
            double x[6];
            for (int j = 0; j < 6; ++j) x[j] = xk[j];
            const double f_start = fdf(rec, c, xk, xk, nullptr);
            const double f_end = inner(rec, c, x, P, &cnt, &cs);
            check_run(cs, cnt, f_start, f_end, P);
            expect(f_end == fdf(rec, c, xk, x, nullptr), "the returned f is not f at the returned state", f_end);
            if (variant && cnt.exit == kExitGradient && noise == 0.0 && m >= 50) {      // exact data: the minimiser is the truth
                for (int j = 0; j < 6; ++j) expect(fabs(x[j] - truth[j]) <= 1.0e-5, "the minimiser of exact data is not the truth", x[j], truth[j]);
            }
            for (int e = 0; e < kEvents; ++e) total.events[e] += cs.events[e];
            total.max_trials = std::max(total.max_trials, cs.max_trials);
            ++runs;
        }
    }
    // the per-pair form rounds coordinates of tens of metres (1e-14 m per residual); f of exact data is 0 and is skipped above
    expect(worst_f <= 1.0e-9, "moment f against per-pair f", worst_f);
    expect(worst_g <= 1.0e-7, "moment gradient against per-pair gradient", worst_g);
    expect(worst_fd <= 1.0e-5, "moment gradient against central differences", worst_fd);
    // ---- scripted 1-D problems
    {
        BfgsParams P = P0;
        P.gradient_tol = 1.0e-6; P.max_inner_iters = 100;
        auto quartic = [](const double* x, double* g) { const double d = x[0] - 2.0; if (g) g[0] = 2.0 * d + 0.4 * d * d * d; return d * d + 0.1 * d * d * d * d + 1.0; };
        auto flat = [](const double* x, double* g) { if (g) g[0] = 2.0e-20 * x[0]; return 1.0e-20 * x[0] * x[0]; };
        Census cs;
        InnerCounts cnt;
        double x[1] = { 0.0 };
        double f = bfgs_minimise<1>(quartic, x, P, &cnt, &cs);
        const double at0[1] = { 0.0 };
        check_run(cs, cnt, quartic(at0, nullptr), f, P);
        expect(cnt.exit == kExitGradient && fabs(x[0] - 2.0) <= 1.0e-6, "the quartic's minimiser", x[0], cnt.exit);
        for (int e = 0; e < kEvents; ++e) total.events[e] += cs.events[e];
        Census c2;
        x[0] = 2.0;                                                  // a start at the minimiser: a zero gradient
        f = bfgs_minimise<1>(quartic, x, P, &cnt, &c2);
        expect(cnt.exit == kExitNoProgress && cnt.iters == 1 && x[0] == 2.0 && c2.events[kStepDegenerate] == 1, "a zero gradient at the start", cnt.exit);
        for (int e = 0; e < kEvents; ++e) total.events[e] += c2.events[e];
        Census c3;
        x[0] = 1.0;                                                  // slopes of 1e-20: below the rounding of the no-progress test
        f = bfgs_minimise<1>(flat, x, P, &cnt, &c3);
        expect(cnt.exit == kExitNoProgress && c3.events[kSectionNoProgress] == 1 && x[0] == 1.0, "no progress on a flat function", cnt.exit, x[0]);
        for (int e = 0; e < kEvents; ++e) total.events[e] += c3.events[e];
        Census c4;
        P.max_inner_iters = 2; P.gradient_tol = 1.0e-12;
        x[0] = 0.0;
        f = bfgs_minimise<1>(quartic, x, P, &cnt, &c4);
        expect(cnt.exit == kExitCap && cnt.iters == 2, "the iteration cap", cnt.exit, cnt.iters);
        for (int e = 0; e < kEvents; ++e) total.events[e] += c4.events[e];
        (void)f;
    }
    static const char* names[kEvents] = { "bracket:rho", "bracket:sigma", "bracket:slope", "bracket:extend", "section:noprogress", "section:shrink",
                                          "section:sigma", "section:flip", "section:advance", "linesearch:limit", "step:degenerate",
                                          "inner:gradient", "inner:cap", "inner:noprogress" };
    std::printf("census over %d runs (most trials of one line search %d):", runs, total.max_trials);
    for (int e = 0; e < kEvents; ++e) std::printf(" %s %ld", names[e], total.events[e]);
    std::printf("\nmoment form against per-pair form: worst %.3g relative in f, %.3g of max |grad|; against central differences %.3g\n",
                worst_f, worst_g, worst_fd);
    for (int e : { (int)kBracketRho, (int)kBracketSigma, (int)kBracketSlope, (int)kBracketExtend, (int)kSectionNoProgress, (int)kSectionShrink,
                   (int)kSectionSigma, (int)kSectionFlip, (int)kStepDegenerate, (int)kInnerGradient, (int)kInnerCap, (int)kInnerNoProgress })
        expect(total.events[e] >= 1, names[e]);
    if (failures) { std::printf("ERROR: gicp_bfgs_check failed (%d)\n", failures); return 1; }
    std::printf("gicp_bfgs_check ok\n");
    return 0;
}
