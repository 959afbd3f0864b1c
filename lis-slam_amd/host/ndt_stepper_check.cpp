// ndt_stepper_check.cpp — NdtStepper (csrc/lisreg_ndt_stepper.hpp), the library's only Newton / More-Thuente loop, against the same
// loop in closed form (ndt_closed_loop and line_search_mt below: what lisreg_ndt_align ran before it went through the stepper; kept
// here as the independent restatement, never a wrapper around the stepper) on scripted evaluations.  A script is a
// function of the pose p that holds no GPU code: a score with its exact gradient and Hessian (a concave or convex quadratic with
// sinusoidal ripples, whose amplitude steers how rough the line searches are), or one of the degenerate records (zero gradient, a
// direction without a slope, a singular or NaN Hessian, no pairs, a table of jumping scores with zero slopes).  Both drivers are given
// the same function, so they see the same answers as long as they ask the same questions in the same order.  Compared per script: the
// request sequence (the bytes of p and the with_hessian flag of every call) and the bytes of every field of the result.  The closed
// form counts which case of the trial value (1-4), which interval update (U1-U3) and which way out of the search and of the loop
// occurred; the program prints the counts (tests/test_ndt_batch_host.py wants every one above zero but interval_converged: that way
// out needs a trial whose slope is exactly zero and which still fails the Wolfe test, and no script reaches it; the stepper carries
// the statement all the same).  Plain C++: g++ -std=c++17 -I../csrc ndt_stepper_check.cpp.
#include "lisreg_ndt_stepper.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace lisreg::ndt_host;

namespace {

enum Hit { kCase1, kCase2, kCase3, kCase4, kU1, kU2, kU3, kTrialAtLow, kNoTrialValue, kIntervalConverged, kWolfe, kOutOfTrials, kFirstTrialAccepted,
           kExtraHessianPass, kReversal, kNoSlope, kZeroStep, kNanStep, kSingleStep, kMaxIters, kEpsilon, kHits };
const char* const kHitName[kHits] = { "case1", "case2", "case3", "case4", "U1", "U2", "U3", "trial_at_low", "no_trial_value", "interval_converged",
                                      "wolfe", "out_of_trials", "first_trial_accepted", "extra_hessian_pass", "reversal", "no_slope", "zero_step",
                                      "nan_step", "single_step", "max_iters", "epsilon" };
long long hits[kHits];

// eval(a, with_hessian, &phi, &dphi) -> 0 or an error code (returned at once).  The first trial carries the Hessian, those inside the
// loop do not.  *a_out = the step, *trials_out = trials made inside the loop.
template <class Eval>
int line_search_mt(Eval&& eval, double phi_0, double d_phi_0, double step_init, double step_max, double step_min, double* a_out,
                   int* trials_out)
{
    double I[6] = { 0.0, 0.0, d_phi_0 - kMu * d_phi_0, 0.0, 0.0, d_phi_0 - kMu * d_phi_0 };
    auto clamp = [&](double a) { if (a > step_max) a = step_max; if (a < step_min) a = step_min; return a; };
    double a_t = clamp(step_init), phi_t, d_phi_t;
    int rc = eval(a_t, true, &phi_t, &d_phi_t);
    if (rc) return rc;
    double psi_t = phi_t - phi_0 - kMu * d_phi_0 * a_t, d_psi_t = d_phi_t - kMu * d_phi_0;
    bool open_interval = true, converged = false;
    int trials = 0;
    while (!converged && trials < kMaxTrials && !(psi_t <= 0.0 && fabs(d_phi_t) <= kNu * fabs(d_phi_0))) {
        if (open_interval && psi_t <= 0.0 && d_psi_t >= 0.0) {
            open_interval = false;
            I[1] += phi_0 - kMu * d_phi_0 * I[0]; I[2] += kMu * d_phi_0;
            I[4] += phi_0 - kMu * d_phi_0 * I[3]; I[5] += kMu * d_phi_0;
        }
        const double f_t = open_interval ? psi_t : phi_t, g_t = open_interval ? d_psi_t : d_phi_t;
        if (a_t == I[0]) { ++hits[kTrialAtLow]; break; }                     // the trial coincides with a_l: it is the step
        double a_next;
        if (!trial_value(I, a_t, f_t, g_t, &a_next) || !std::isfinite(a_next)) { ++hits[kNoTrialValue]; break; }
        ++hits[f_t > I[1] ? kCase1 : (g_t * I[2] < 0.0 ? kCase2 : (fabs(g_t) <= fabs(I[2]) ? kCase3 : kCase4))];
        { const double s = g_t * (I[0] - a_t); if (f_t > I[1]) ++hits[kU1]; else if (s > 0) ++hits[kU2]; else if (s < 0) ++hits[kU3]; }
        converged = update_interval(I, a_t, f_t, g_t);
        a_t = clamp(a_next);
        rc = eval(a_t, false, &phi_t, &d_phi_t);
        if (rc) return rc;
        psi_t = phi_t - phi_0 - kMu * d_phi_0 * a_t; d_psi_t = d_phi_t - kMu * d_phi_0;
        ++trials;
    }
    if (converged) ++hits[kIntervalConverged];
    else if (trials >= kMaxTrials) ++hits[kOutOfTrials];
    else if (psi_t <= 0.0 && fabs(d_phi_t) <= kNu * fabs(d_phi_0)) ++hits[kWolfe];
    *a_out = a_t; *trials_out = trials;
    return 0;
}

// The Newton loop of pcl::NormalDistributionsTransform::computeTransformation as tests/ndt_ref.py restates it.
// eval(p, with_hessian, out[29]) -> 0 or an error code (returned at once)
template <class Eval>
int ndt_closed_loop(Eval&& eval, const double p0[6], const NdtLoopParams& P, int n, NdtLoopResult* res)
{
    double p[6], out[kNdtOut];
    int n_evals = 0;
    memcpy(p, p0, sizeof p);
    auto evaluate = [&](const double at[6], bool hess) { const int rc = eval(at, hess, out); if (!rc) ++n_evals; return rc; };
    // phi(a), phi'(a) along `dir` from `base`
    auto eval_along = [&](const double base[6], const double dir[6], double a, bool hess, double* phi, double* dphi) {
        double q[6];
        for (int k = 0; k < 6; ++k) q[k] = base[k] + a * dir[k];
        const int rc = evaluate(q, hess);
        if (rc) return rc;
        *phi = -out[0];
        double d = 0;
        for (int k = 0; k < 6; ++k) d += out[1 + k] * dir[k];
        *dphi = -d;
        return 0;
    };
    const double eps = P.transformation_epsilon;
    int rc = evaluate(p, true);
    if (rc) return rc;
    int iters = 0;
    bool converged = false;
    while (!converged) {
        double Hm[36], g[6], delta[6];
        for (int k = 0; k < 6; ++k) g[k] = out[1 + k];
        for (int i = 0, k = 7; i < 6; ++i)
            for (int j = i; j < 6; ++j, ++k) Hm[6 * i + j] = Hm[6 * j + i] = out[k];
        solve_step(Hm, g, delta);
        double nrm = 0;
        for (int k = 0; k < 6; ++k) nrm += delta[k] * delta[k];
        nrm = sqrt(nrm);
        if (nrm == 0 || std::isnan(nrm)) { converged = !std::isnan(nrm); ++hits[converged ? kZeroStep : kNanStep]; break; }
        for (int k = 0; k < 6; ++k) delta[k] /= nrm;
        const double phi_0 = -out[0];
        double d_phi_0 = 0;
        for (int k = 0; k < 6; ++k) d_phi_0 += g[k] * delta[k];
        d_phi_0 = -d_phi_0;
        double a_t = 0.0;
        if (d_phi_0 != 0) {
            if (d_phi_0 > 0) { d_phi_0 = -d_phi_0; for (int k = 0; k < 6; ++k) delta[k] = -delta[k]; ++hits[kReversal]; }
            double base[6];
            memcpy(base, p, sizeof base);
            if (P.line_search) {
                int trials = 0;
                rc = line_search_mt([&](double a, bool hess, double* f, double* gd) { return eval_along(base, delta, a, hess, f, gd); },
                                    phi_0, d_phi_0, nrm, P.step_size, eps / 2, &a_t, &trials);
                if (rc) return rc;
                if (trials) {                               // one Hessian pass at the accepted step
                    double f, gd;
                    rc = eval_along(base, delta, a_t, true, &f, &gd);
                    if (rc) return rc;
                    ++hits[kExtraHessianPass];
                } else {
                    ++hits[kFirstTrialAccepted];
                }
            } else {
                a_t = std::min(std::max(nrm, eps / 2), P.step_size);
                double f, gd;
                rc = eval_along(base, delta, a_t, true, &f, &gd);
                if (rc) return rc;
                ++hits[kSingleStep];
            }
            for (int k = 0; k < 6; ++k) p[k] = base[k] + a_t * delta[k];
        } else {
            ++hits[kNoSlope];
        }
        if (iters > P.max_iters || (iters && fabs(a_t) < eps)) { converged = true; ++hits[iters > P.max_iters ? kMaxIters : kEpsilon]; }
        ++iters;
    }
    memcpy(res->p, p, sizeof p);
    res->converged = converged ? 1 : 0; res->iters = iters; res->n_evals = n_evals;
    res->n_pairs_last = (long long)out[28];
    res->score = out[0]; res->trans_probability = out[0] / (double)n;
    return 0;
}

struct Rng {                                          // splitmix64: the same scripts everywhere
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }      // [0, 1)
    int pick(int n) { return (int)(next() % (uint64_t)n); }
};

// score(p) = sign * -1/2 (p - c)^T Q (p - c) + sum_j amp_j sin(k_j . p + ph_j), with its exact gradient and Hessian; sign = +1: concave
// (Newton steps ascend), -1: convex (the Newton direction is no descent direction of phi = -score: the reversal).  The degenerate
// kinds replace the record outright.
enum Kind { kSmooth, kRough, kConvex, kZeroGradient, kSlopeless, kSingular, kNanHessian, kNoPairs, kNanLater, kTable, kKinds };
struct Script {
    int    kind;
    double sign, c[6], Q[6][6], amp[4], kv[4][6], ph[4];
    double pairs;
    int    nan_from;                                  // kNanLater: the Hessian is NaN from this call on
    uint64_t table_seed;                              // kTable
    double table_jump;
    NdtLoopParams P;
    double p0[6];
    int    n;
};

Script make_script(uint64_t seed)
{
    Rng r{ seed * 0x2545f4914f6cdd1dull + 29 };
    Script s;
    memset(&s, 0, sizeof s);
    s.kind = (int)(seed % kKinds);
    static const int iters[6] = { 0, 1, 2, 5, 35, 35 };
    s.P = NdtLoopParams{ 0.1 * (0.2 + 2.0 * r.uni()), 0.01 * (0.1 + r.uni()), iters[r.pick(6)], r.pick(4) ? 1 : 0 };
    s.n = 1 + r.pick(2000);
    s.pairs = (double)r.pick(9000);
    s.sign = s.kind == kConvex ? -1.0 : 1.0;
    s.nan_from = 1 + r.pick(6);
    s.table_seed = r.next(); s.table_jump = r.pick(2) ? 1.0 : 0.01;
    double L[6][6];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) L[i][j] = j < i ? 0.3 * (2.0 * r.uni() - 1.0) : (j == i ? 0.5 + 2.0 * r.uni() : 0.0);
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) { double a = 0; for (int k = 0; k < 6; ++k) a += L[i][k] * L[j][k]; s.Q[i][j] = 20.0 * a; }
    for (int k = 0; k < 6; ++k) { s.c[k] = 0.5 * (2.0 * r.uni() - 1.0); s.p0[k] = s.c[k] + (k < 3 ? 0.4 : 0.05) * (2.0 * r.uni() - 1.0); }
    const double rough = s.kind == kRough ? 3.0 * r.uni() : (s.kind == kSmooth || s.kind == kConvex ? 0.02 * (double)r.pick(2) : 0.3 * r.uni());
    for (int j = 0; j < 4; ++j) {
        s.amp[j] = rough * r.uni();
        s.ph[j] = 6.283 * r.uni();
        for (int k = 0; k < 6; ++k) s.kv[j][k] = (s.kind == kRough ? 40.0 : 8.0) * (2.0 * r.uni() - 1.0);
    }
    return s;
}

void answer(const Script& s, const double p[6], bool hess, int call, double out[kNdtOut])
{
    for (int k = 0; k < kNdtOut; ++k) out[k] = 0.0;
    if (s.kind == kNoPairs) return;                                                        // all zeros: no pair at any pose
    out[28] = s.pairs;
    double d[6], Qd[6], H[6][6];
    for (int k = 0; k < 6; ++k) d[k] = p[k] - s.c[k];
    double f = 0;
    for (int i = 0; i < 6; ++i) { Qd[i] = 0; for (int j = 0; j < 6; ++j) Qd[i] += s.Q[i][j] * d[j]; f += 0.5 * d[i] * Qd[i]; }
    out[0] = -s.sign * f;
    for (int i = 0; i < 6; ++i) { out[1 + i] = -s.sign * Qd[i]; for (int j = 0; j < 6; ++j) H[i][j] = -s.sign * s.Q[i][j]; }
    for (int j = 0; j < 4; ++j) {
        double ang = s.ph[j];
        for (int k = 0; k < 6; ++k) ang += s.kv[j][k] * p[k];
        out[0] += s.amp[j] * sin(ang);
        for (int i = 0; i < 6; ++i) {
            out[1 + i] += s.amp[j] * cos(ang) * s.kv[j][i];
            for (int k = 0; k < 6; ++k) H[i][k] -= s.amp[j] * sin(ang) * s.kv[j][i] * s.kv[j][k];
        }
    }
    switch (s.kind) {
    case kZeroGradient: for (int i = 0; i < 6; ++i) out[1 + i] = 0.0; break;
    case kSlopeless:                                                                       // delta = -H^+ g is at right angles to g, exactly
        for (int i = 0; i < 6; ++i) { out[1 + i] = i == 0 ? 1.0 : 0.0; for (int j = 0; j < 6; ++j) H[i][j] = (i == j && i > 1) || i + j == 1 ? 1.0 : 0.0; }
        break;
    case kSingular: for (int i = 0; i < 6; ++i) H[i][5] = H[5][i] = H[i][2] = H[2][i] = 0.0; break;   // rank 4
    case kNanHessian: H[1][3] = H[3][1] = NAN; break;
    case kNanLater: if (call >= s.nan_from) H[0][0] = NAN; break;
    case kTable:                                                                           // behind the first record: the score jumps about, and
        if (call) {                                                                        // every other gradient is exactly zero (phi' = 0)
            Rng r{ s.table_seed + 977ull * (uint64_t)call };
            out[0] += 0.2 * s.table_jump * (2.0 * r.uni() - 1.0);
            if (r.pick(2)) for (int i = 0; i < 6; ++i) out[1 + i] = 0.0;
        }
        break;
    default: break;
    }
    if (hess)
        for (int i = 0, q = 7; i < 6; ++i)
            for (int j = i; j < 6; ++j, ++q) out[q] = H[i][j];
}

struct Call { double p[6]; int hessian; };

bool same_result(const NdtLoopResult& a, const NdtLoopResult& b)
{
    return !memcmp(a.p, b.p, sizeof a.p) && a.converged == b.converged && a.iters == b.iters && a.n_evals == b.n_evals &&
           a.n_pairs_last == b.n_pairs_last && !memcmp(&a.score, &b.score, 8) && !memcmp(&a.trans_probability, &b.trans_probability, 8);
}

}  // namespace

int main(int argc, char** argv)
{
    const int n_scripts = argc > 1 ? atoi(argv[1]) : 900;
    long long calls_total = 0, iters_total = 0;
    for (int i = 0; i < n_scripts; ++i) {
        const Script s = make_script((uint64_t)i);
        std::vector<Call> a, b;
        auto record = [&](std::vector<Call>& to, const double p[6], bool hess, double out[kNdtOut]) {
            Call c; memcpy(c.p, p, sizeof c.p); c.hessian = hess ? 1 : 0;
            answer(s, p, hess, (int)to.size(), out);
            to.push_back(c);
        };
        NdtLoopResult want;
        memset(&want, 0, sizeof want);
        const int rc = ndt_closed_loop([&](const double p[6], bool hess, double out[kNdtOut]) { record(a, p, hess, out); return 0; }, s.p0, s.P, s.n, &want);
        NdtStepper st;
        double out[kNdtOut];
        st.start(s.p0, s.P, s.n);
        for (bool more = true; more;) {
            record(b, st.req_p, st.req_hessian, out);
            more = st.feed(out);
            if (b.size() > a.size() + 4) break;                     // (a stepper that does not end is a difference, not a hang)
        }
        bool ok = rc == 0 && st.finished() && a.size() == b.size() && same_result(want, st.res) && (int)a.size() == want.n_evals;
        for (size_t k = 0; ok && k < a.size(); ++k) ok = !memcmp(a[k].p, b[k].p, sizeof a[k].p) && a[k].hessian == b[k].hessian;
        ok = ok && !a.empty() && a[0].hessian == 1 && !st.feed(out);                           // (a finished stepper stays finished)
        if (!ok) {
            printf("script %d (kind %d) differs: %zu / %zu calls, evals %d / %d, iters %d / %d, converged %d / %d\n", i, s.kind, a.size(), b.size(),
                   want.n_evals, st.res.n_evals, want.iters, st.res.iters, want.converged, st.res.converged);
            return 1;
        }
        calls_total += (long long)a.size();
        iters_total += want.iters;
    }
    printf("scripts %d calls %lld iterations %lld hits", n_scripts, calls_total, iters_total);
    for (int k = 0; k < kHits; ++k) printf(" %s=%lld", kHitName[k], hits[k]);
    printf("\nndt_stepper_check ok\n");
    return 0;
}
