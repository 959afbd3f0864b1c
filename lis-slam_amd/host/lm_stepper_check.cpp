// lm_stepper_check.cpp — LmStepper (csrc/lisreg_lm_stepper.hpp), the library's only Levenberg-Marquardt loop, against the same loop
// in closed form (lm_closed_loop below: what the single aligners ran as lm_optimise before they, too, went through the stepper; it is
// kept here as the independent restatement and is never a wrapper around the stepper) on scripted
// evaluations.  A script is a table of out[29] records: call k of eval gets record k (the last one again when the
// table runs out), whatever T is asked for, so both drivers see the same answers as long as they ask the same questions in the same
// order.  Compared per script: the request sequence (the bytes of T and the with_hessian flag of every call) and the bytes of every
// field of LmResult.  The scripts are seeded and built so that every way out of the loop occurs; the program prints how often each one
// did (tests/test_fgicp_batch_host.py wants every count above zero).  Plain C++: g++ -std=c++17 -I../csrc lm_stepper_check.cpp.
#include "lisreg_lm_stepper.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace lisreg::vgicp_host;

namespace {

// The Levenberg-Marquardt loop of LsqRegistration::step_lm as tests/vgicp_ref.py restates it.  eval(T, with_hessian, out[29]) -> 0 or an
// error code (returned at once).  lambda starts at init_lambda_factor max|diag H| of the first linearisation and is carried across the
// outer iterations; NOT (rho >= 0) is a rejection; a trial loop that runs out, or a system that is not positive definite, ends the
// alignment unconverged.  No NaN can reach T: a step is applied only after solve_damped vouched for a finite delta.
template <class Eval>
int lm_closed_loop(Eval&& eval, const double T0[16], const LmParams& P, LmResult* res)
{
    double T[16], out[kOut];
    memcpy(T, T0, sizeof T);
    int rc = eval(T, true, out);
    if (rc) return rc;
    res->converged = 0; res->iters = 0; res->n_evals = 1; res->n_rejected = 0;
    double e = out[0], lam = 0.0;
    long long pairs = (long long)out[28];
    if (pairs > 0) {
        for (int k = 0, q = 7; k < 6; q += 6 - k, ++k) lam = std::max(lam, fabs(out[q]));         // the diagonal of the packed triangle
        lam *= P.init_lambda_factor;
        for (int it = 0; it < P.max_iters; ++it) {
            if (it) {
                rc = eval(T, true, out);
                if (rc) return rc;
                ++res->n_evals;
                e = out[0]; pairs = (long long)out[28];
            }
            res->iters = it + 1;
            double H[36], b[6];
            for (int k = 0; k < 6; ++k) b[k] = out[1 + k];
            for (int i = 0, q = 7; i < 6; ++i)
                for (int j = i; j < 6; ++j, ++q) H[6 * i + j] = H[6 * j + i] = out[q];
            double nu = 2.0;
            bool stop = false, accepted = false;
            for (int trial = 0; trial < P.lm_max_iterations; ++trial) {
                double delta[6], E[16], Tn[16], o2[kOut];
                if (!solve_damped(H, b, lam, delta)) { stop = true; break; }
                se3_exp(delta, E);
                mul_rigid(E, T, Tn);
                rc = eval(Tn, false, o2);
                if (rc) return rc;
                ++res->n_evals;
                const double en = o2[0];
                pairs = (long long)o2[28];
                double den = 0.0;
                for (int k = 0; k < 6; ++k) den += delta[k] * (lam * delta[k] - b[k]);
                const double rho = (e - en) / den;
                const bool dconv = delta_converged(delta, P.rotation_epsilon, P.transformation_epsilon);
                if (!(rho >= 0.0)) {
                    ++res->n_rejected;
                    if (dconv) { res->converged = 1; stop = true; break; }
                    lam = nu * lam; nu = 2.0 * nu;
                    continue;
                }
                memcpy(T, Tn, sizeof T);
                e = en;
                const double c = 2.0 * rho - 1.0;
                lam = lam * std::max(1.0 / 3.0, 1.0 - c * c * c);
                accepted = true;
                if (dconv) { res->converged = 1; stop = true; }
                break;
            }
            if (!accepted) stop = true;                             // rejected while converged, not positive definite, or out of trials
            if (stop) break;
        }
    }
    memcpy(res->T, T, sizeof T);
    res->error = e; res->lambda = lam; res->n_pairs_last = pairs;
    return 0;
}

struct Rng {                                          // splitmix64: the same scripts everywhere
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }      // [0, 1)
    int pick(int n) { return (int)(next() % (uint64_t)n); }
};

struct Record { double out[kOut]; };
struct Call { double T[16]; int hessian; };

// one record: the error `e`, a gradient of size `bscale`, H = hscale (I + a small random symmetric part) (negative hscale: not positive
// definite), `pairs` pairs
Record record(Rng& r, double e, double bscale, double hscale, double pairs)
{
    Record o;
    o.out[0] = e;
    for (int k = 0; k < 6; ++k) o.out[1 + k] = bscale * (2.0 * r.uni() - 1.0);
    for (int i = 0, q = 7; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++q) o.out[q] = hscale * ((i == j ? 1.0 : 0.0) + 0.05 * (2.0 * r.uni() - 1.0));
    o.out[28] = pairs;
    return o;
}

struct Script { std::vector<Record> rec; LmParams P; double T0[16]; };

// kind steers which way out the script is built for; the rest is random
Script make_script(uint64_t seed)
{
    Rng r{ seed * 0x2545f4914f6cdd1dull + 17 };
    Script s;
    const int kind = (int)(seed % 8);
    static const int iters[5] = { 0, 1, 2, 3, 6 }, trials[4] = { 1, 2, 3, 10 };
    s.P = LmParams{ 0.01 * (0.1 + r.uni()), 2.0e-3 * (0.1 + r.uni()), 1.0e-9 * (1.0 + 1.0e6 * r.uni() * (double)r.pick(2)), iters[r.pick(5)], trials[r.pick(4)] };
    if (kind == 1) s.P.max_iters = 0;
    if (kind == 5 || kind == 3) s.P.max_iters = std::max(s.P.max_iters, 1);
    double d[6];
    for (int k = 0; k < 6; ++k) d[k] = (k < 3 ? 0.3 : 2.0) * (2.0 * r.uni() - 1.0);
    se3_exp(d, s.T0);
    double e = 100.0 * (0.5 + r.uni());
    const int n = 4 + r.pick(60);
    for (int k = 0; k < n; ++k) {
        double bscale = r.pick(3) ? 1.0 : 1.0e-7, hscale = 10.0 * (0.5 + r.uni()), pairs = 1.0 + (double)r.pick(5000), step = r.pick(3) ? -1.0 : 1.0;
        switch (kind) {
        case 0: if (k == 0) pairs = 0.0; break;                                   // no pair at the guess
        case 2: bscale = 1.0e-7; step = k >= 1 + r.pick(3) ? 1.0 : -1.0; break;   // a rejection while the step is converged
        case 3: if (k == 0 || r.pick(4) == 0) hscale = -hscale; break;            // not positive definite
        case 4: bscale = 1.0; if (k >= 1) step = 1.0; break;                      // every trial rejected: out of trials
        case 5: bscale = 1.0; step = -1.0; break;                                 // every step accepted and large: max_iters
        case 6: if (r.pick(5) == 0) e = NAN; break;                               // a NaN error: rho is NaN, a rejection
        default: break;
        }
        if (e == e) e = std::max(e + step * e * 0.2 * r.uni(), 1.0e-3);
        s.rec.push_back(record(r, kind == 6 && r.pick(7) == 0 ? (double)NAN : e, bscale, hscale, pairs));
        if (!(e == e)) e = 50.0;
    }
    return s;
}

struct Scripted {
    const Script& s;
    size_t k = 0;
    std::vector<Call> calls;
    const double* answer(const double T[16], bool hess)
    {
        Call c; memcpy(c.T, T, sizeof c.T); c.hessian = hess ? 1 : 0;
        calls.push_back(c);
        const Record& rec = s.rec[std::min(k, s.rec.size() - 1)];
        ++k;
        return rec.out;
    }
};

bool same_result(const LmResult& a, const LmResult& b)
{
    return !memcmp(a.T, b.T, sizeof a.T) && a.converged == b.converged && a.iters == b.iters && a.n_evals == b.n_evals &&
           a.n_rejected == b.n_rejected && a.n_pairs_last == b.n_pairs_last && !memcmp(&a.error, &b.error, 8) && !memcmp(&a.lambda, &b.lambda, 8);
}

}  // namespace

int main(int argc, char** argv)
{
    const int n_scripts = argc > 1 ? atoi(argv[1]) : 800;
    static const char* names[8] = { "running", "no_pair", "max_iters_zero", "converged", "rejected_while_converged", "not_positive_definite",
                                    "out_of_trials", "max_iters" };
    long long hits[8] = { 0 }, calls_total = 0, rejected_total = 0;
    for (int i = 0; i < n_scripts; ++i) {
        const Script s = make_script((uint64_t)i);
        Scripted a{ s, 0, {} }, b{ s, 0, {} };
        LmResult want;
        memset(&want, 0, sizeof want);
        const int rc = lm_closed_loop([&](const double T[16], bool hess, double out[kOut]) { memcpy(out, a.answer(T, hess), sizeof(double) * kOut); return 0; },
                                      s.T0, s.P, &want);
        LmStepper st;
        st.start(s.T0, s.P);
        for (bool more = true; more;) more = st.feed(b.answer(st.req_T, st.req_hessian));
        bool ok = rc == 0 && st.finished() && a.calls.size() == b.calls.size() && same_result(want, st.res) && (int)a.calls.size() == want.n_evals;
        for (size_t k = 0; ok && k < a.calls.size(); ++k)
            ok = !memcmp(a.calls[k].T, b.calls[k].T, sizeof a.calls[k].T) && a.calls[k].hessian == b.calls[k].hessian;
        // the way out the stepper names must be the one the result shows
        const LmStepper::Exit x = st.exit;
        if (x == LmStepper::kNoPair) ok = ok && want.n_pairs_last <= 0 && want.n_evals == 1 && want.iters == 0;
        if (x == LmStepper::kNoIterations) ok = ok && s.P.max_iters == 0 && want.n_evals == 1 && want.n_pairs_last > 0;
        if (x == LmStepper::kConverged || x == LmStepper::kRejectedConverged) ok = ok && want.converged == 1;
        if (x == LmStepper::kRejectedConverged) ok = ok && want.n_rejected >= 1 && a.calls.back().hessian == 0;
        if (x == LmStepper::kNotPositiveDefinite || x == LmStepper::kOutOfTrials || x == LmStepper::kMaxIters) ok = ok && want.converged == 0;
        if (x == LmStepper::kOutOfTrials) ok = ok && want.n_rejected >= s.P.lm_max_iterations;
        if (x == LmStepper::kMaxIters) ok = ok && want.iters == s.P.max_iters && s.P.max_iters > 0;
        if (x == LmStepper::kRunning) ok = false;
        if (!ok) {
            printf("script %d differs: exit %s, %zu / %zu calls, evals %d / %d, iters %d / %d\n", i, names[x], a.calls.size(), b.calls.size(),
                   want.n_evals, st.res.n_evals, want.iters, st.res.iters);
            return 1;
        }
        ++hits[x];
        calls_total += (long long)a.calls.size();
        rejected_total += want.n_rejected;
    }
    printf("scripts %d calls %lld rejected %lld\n", n_scripts, calls_total, rejected_total);
    for (int k = 1; k < 8; ++k) printf("hit %s %lld\n", names[k], hits[k]);
    printf("lm_stepper_check ok\n");
    return 0;
}
