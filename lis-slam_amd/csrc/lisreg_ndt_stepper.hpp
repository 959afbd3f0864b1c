// lisreg_ndt_stepper.hpp — the Newton loop of the NDT registration with its More-Thuente line search (tests/ndt_ref.py: align and
// line_search_mt), the only one in csrc/: the state of one run that asks for one evaluation at a time and is resumed with its answer,
// the way LmStepper (lisreg_lm_stepper.hpp) holds the Levenberg-Marquardt loop.  A batch driver holds many runs and answers the
// outstanding requests of all of them with one round of launches (lisreg_batch_driver.hpp); the single aligner answers
// them one by one (ndt_optimise below).  The pieces without a state (the 6 x 6 solve, the trial value, the interval update) are
// lisreg_ndt_host.hpp's.  host/ndt_stepper_check.cpp holds the same loop in closed form and compares the two on scripted evaluations.
// Plain C++ (no HIP).  Not installed.
#pragma once
#include "lisreg_ndt_host.hpp"

namespace lisreg {
namespace ndt_host {

constexpr int kNdtOut = 29;       // score, gradient [6], upper triangle of the Hessian row by row [21], pairs

struct NdtLoopParams { double step_size, transformation_epsilon; int max_iters, line_search; };
struct NdtLoopResult {
    double p[6];
    int    converged, iters, n_evals;
    long long n_pairs_last;
    double score, trans_probability;
};

struct NdtStepper {
    // the outstanding request: evaluate at req_p, with the Hessian or without
    double        req_p[6];
    bool          req_hessian = true;
    NdtLoopResult res;            // complete once feed() has returned false

    // n_records: what trans_probability divides the score by (the source's records, NaN ones included)
    void start(const double p0[6], const NdtLoopParams& params, int n_records)
    {
        P = params; n = n_records;
        memcpy(p, p0, sizeof p);
        iters = 0; n_evals = 0;
        state = kFirst;
        ask(p, true);
    }

    bool finished() const { return state == kDone; }

    // the answer to the outstanding request; true: there is a next request, false: the run is finished and res is filled
    bool feed(const double out[kNdtOut])
    {
        if (state == kDone) return false;
        ++n_evals;
        score = out[0]; pairs = (long long)out[28];
        double d = 0;
        switch (state) {
        case kFirst:
            memcpy(rec, out, sizeof rec);
            return newton();
        case kFirstTrial:                                           // it carries the Hessian: the record of the next solve if it is the step
            memcpy(rec, out, sizeof rec);
            open_interval = true; ls_converged = false; trials = -1;
            [[fallthrough]];
        case kTrial:
            ++trials;
            phi_t = -out[0];
            for (int k = 0; k < 6; ++k) d += out[1 + k] * delta[k];
            d_phi_t = -d;
            psi_t = phi_t - phi_0 - kMu * d_phi_0 * a_t; d_psi_t = d_phi_t - kMu * d_phi_0;
            return line_search_mt();
        case kAccepted:                                             // the Hessian pass at the accepted step
            memcpy(rec, out, sizeof rec);
            return step_taken() ? finish(true) : newton();
        default:
            return false;
        }
    }

private:
    enum State { kFirst, kFirstTrial, kTrial, kAccepted, kDone };
    NdtLoopParams P;
    State     state = kDone;
    int       n = 0, iters = 0, n_evals = 0, trials = 0;
    double    p[6], base[6], delta[6], rec[kNdtOut], I[6];
    double    nrm = 0, phi_0 = 0, d_phi_0 = 0, a_t = 0, phi_t = 0, d_phi_t = 0, psi_t = 0, d_psi_t = 0, score = 0;
    long long pairs = 0;
    bool      open_interval = true, ls_converged = false;

    void ask(const double at[6], bool hessian) { memcpy(req_p, at, sizeof req_p); req_hessian = hessian; }
    void ask_along(bool hessian, State next)
    {
        double q[6];
        for (int k = 0; k < 6; ++k) q[k] = base[k] + a_t * delta[k];
        ask(q, hessian);
        state = next;
    }
    double clamp(double a) const
    {
        const double step_max = P.step_size, step_min = P.transformation_epsilon / 2;
        if (a > step_max) a = step_max;
        if (a < step_min) a = step_min;
        return a;
    }

    // the iterations on the record `rec` up to the next request: the solve, the direction and its first trial; a direction without a
    // slope asks for nothing, and the loop goes on with the same record until its end rule fires
    bool newton()
    {
        for (;;) {
            double Hm[36], g[6];
            for (int k = 0; k < 6; ++k) g[k] = rec[1 + k];
            for (int i = 0, k = 7; i < 6; ++i)
                for (int j = i; j < 6; ++j, ++k) Hm[6 * i + j] = Hm[6 * j + i] = rec[k];
            solve_step(Hm, g, delta);
            nrm = 0;
            for (int k = 0; k < 6; ++k) nrm += delta[k] * delta[k];
            nrm = sqrt(nrm);
            if (nrm == 0 || std::isnan(nrm)) return finish(!std::isnan(nrm));
            for (int k = 0; k < 6; ++k) delta[k] /= nrm;
            phi_0 = -rec[0];
            d_phi_0 = 0;
            for (int k = 0; k < 6; ++k) d_phi_0 += g[k] * delta[k];
            d_phi_0 = -d_phi_0;
            a_t = 0.0;
            if (d_phi_0 != 0) {
                if (d_phi_0 > 0) { d_phi_0 = -d_phi_0; for (int k = 0; k < 6; ++k) delta[k] = -delta[k]; }
                memcpy(base, p, sizeof base);
                if (P.line_search) {
                    I[0] = 0.0; I[1] = 0.0; I[2] = d_phi_0 - kMu * d_phi_0; I[3] = 0.0; I[4] = 0.0; I[5] = d_phi_0 - kMu * d_phi_0;
                    a_t = clamp(nrm);
                    ask_along(true, kFirstTrial);
                } else {
                    a_t = std::min(std::max(nrm, P.transformation_epsilon / 2), P.step_size);
                    ask_along(true, kAccepted);
                }
                return true;
            }
            if (end_of_iteration()) return finish(true);
        }
    }

    // More-Thuente on the trial just answered (strong Wolfe conditions, at most kMaxTrials trials behind the first, the next trial
    // selected before the interval is updated): the next trial, or the end of the search
    bool line_search_mt()
    {
        if (!ls_converged && trials < kMaxTrials && !(psi_t <= 0.0 && fabs(d_phi_t) <= kNu * fabs(d_phi_0))) {
            if (open_interval && psi_t <= 0.0 && d_psi_t >= 0.0) {
                open_interval = false;
                I[1] += phi_0 - kMu * d_phi_0 * I[0]; I[2] += kMu * d_phi_0;
                I[4] += phi_0 - kMu * d_phi_0 * I[3]; I[5] += kMu * d_phi_0;
            }
            const double f_t = open_interval ? psi_t : phi_t, g_t = open_interval ? d_psi_t : d_phi_t;
            double a_next;
            // (a trial that coincides with a_l is the step; so is one behind which there is no finite trial value)
            if (a_t != I[0] && trial_value(I, a_t, f_t, g_t, &a_next) && std::isfinite(a_next)) {
                ls_converged = update_interval(I, a_t, f_t, g_t);
                a_t = clamp(a_next);
                ask_along(false, kTrial);
                return true;
            }
        }
        if (trials) {                                               // one Hessian pass at the accepted step
            ask_along(true, kAccepted);
            return true;
        }
        return step_taken() ? finish(true) : newton();              // the first trial is the step: its record has the Hessian
    }

    // p moves by the step; true: the loop's end rule fired
    bool step_taken()
    {
        for (int k = 0; k < 6; ++k) p[k] = base[k] + a_t * delta[k];
        return end_of_iteration();
    }

    bool end_of_iteration()
    {
        const bool end = iters > P.max_iters || (iters && fabs(a_t) < P.transformation_epsilon);
        ++iters;
        return end;
    }

    bool finish(bool converged)
    {
        memcpy(res.p, p, sizeof p);
        res.converged = converged ? 1 : 0; res.iters = iters; res.n_evals = n_evals;
        res.n_pairs_last = pairs; res.score = score; res.trans_probability = score / (double)n;
        state = kDone;
        return false;
    }
};

// One run with its evaluations answered on the spot: eval(p, with_hessian, out[29]) -> 0 or an error code (returned at once)
template <class Eval>
int ndt_optimise(Eval&& eval, const double p0[6], const NdtLoopParams& P, int n_records, NdtLoopResult* res)
{
    NdtStepper st;
    double out[kNdtOut];
    st.start(p0, P, n_records);
    do {
        if (const int rc = eval(st.req_p, st.req_hessian, out)) return rc;
    } while (st.feed(out));
    *res = st.res;
    return 0;
}

}  // namespace ndt_host
}  // namespace lisreg
