// lisreg_lm_stepper.hpp — the Levenberg-Marquardt loop of the fast_gicp family (LsqRegistration::step_lm as tests/vgicp_ref.py restates
// it), the only one in csrc/: the state of one run that asks for one evaluation at a time and is resumed with its answer.  A batch
// driver holds many runs and answers the outstanding requests of all of them with one round of launches (lisreg_batch_driver.hpp,
// DESIGN.md §7m); a single aligner answers them one by one (lm_optimise below).  lambda starts at init_lambda_factor max|diag H| of the
// first linearisation and is carried across the outer iterations; NOT (rho >= 0) is a rejection; a trial loop that runs out, or a system
// that is not positive definite, ends the alignment unconverged.  No NaN can reach T: a step is applied only after solve_damped vouched
// for a finite delta.  host/lm_stepper_check.cpp holds the same loop in closed form and compares the two on scripted evaluations.
// Plain C++ (no HIP).  Not installed.
#pragma once
#include "lisreg_vgicp_host.hpp"

namespace lisreg {
namespace vgicp_host {

struct LmStepper {
    // why the run ended (kRunning until it has)
    enum Exit { kRunning = 0, kNoPair, kNoIterations, kConverged, kRejectedConverged, kNotPositiveDefinite, kOutOfTrials, kMaxIters };

    // the outstanding request: evaluate at req_T, with the Hessian (a linearisation) or the error alone
    double   req_T[16];
    bool     req_hessian = true;
    LmResult res;                 // complete once feed() has returned false
    Exit     exit = kRunning;

    void start(const double T0[16], const LmParams& params)
    {
        P = params;
        memcpy(T, T0, sizeof T);
        state = kFirst; exit = kRunning;
        ask(T, true);
    }

    bool finished() const { return state == kDone; }

    // the answer to the outstanding request; true: there is a next request, false: the run is finished and res is filled
    bool feed(const double out[kOut])
    {
        switch (state) {
        case kFirst:
            res.converged = 0; res.iters = 0; res.n_evals = 1; res.n_rejected = 0;
            e = out[0]; lam = 0.0;
            pairs = (long long)out[28];
            if (!(pairs > 0)) return finish(kNoPair);
            for (int k = 0, q = 7; k < 6; q += 6 - k, ++k) lam = std::max(lam, fabs(out[q]));     // the diagonal of the packed triangle
            lam *= P.init_lambda_factor;
            it = 0;
            if (!(it < P.max_iters)) return finish(kNoIterations);
            return iterate(out);
        case kLinearise:
            ++res.n_evals;
            e = out[0]; pairs = (long long)out[28];
            return iterate(out);
        case kTrial: {
            ++res.n_evals;
            const double en = out[0];
            pairs = (long long)out[28];
            double den = 0.0;
            for (int k = 0; k < 6; ++k) den += delta[k] * (lam * delta[k] - b[k]);
            const double rho = (e - en) / den;
            const bool dconv = delta_converged(delta, P.rotation_epsilon, P.transformation_epsilon);
            if (!(rho >= 0.0)) {
                ++res.n_rejected;
                if (dconv) { res.converged = 1; return finish(kRejectedConverged); }
                lam = nu * lam; nu = 2.0 * nu;
                ++trial;
                return try_step();
            }
            memcpy(T, Tn, sizeof T);
            e = en;
            const double c = 2.0 * rho - 1.0;
            lam = lam * std::max(1.0 / 3.0, 1.0 - c * c * c);
            if (dconv) { res.converged = 1; return finish(kConverged); }
            if (!(++it < P.max_iters)) return finish(kMaxIters);
            state = kLinearise;
            ask(T, true);
            return true;
        }
        default:
            return false;
        }
    }

private:
    enum State { kFirst, kLinearise, kTrial, kDone };
    LmParams  P;
    State     state = kDone;
    double    T[16], Tn[16], H[36], b[6], delta[6];
    double    e = 0.0, lam = 0.0, nu = 2.0;
    long long pairs = 0;
    int       it = 0, trial = 0;

    void ask(const double at[16], bool hessian) { memcpy(req_T, at, sizeof req_T); req_hessian = hessian; }

    // outer iteration `it` on its linearisation `out`
    bool iterate(const double out[kOut])
    {
        res.iters = it + 1;
        for (int k = 0; k < 6; ++k) b[k] = out[1 + k];
        for (int i = 0, q = 7; i < 6; ++i)
            for (int j = i; j < 6; ++j, ++q) H[6 * i + j] = H[6 * j + i] = out[q];
        nu = 2.0;
        trial = 0;
        return try_step();
    }

    // trial `trial` of the iteration: the damped step and the request for its error, or the end of the run
    bool try_step()
    {
        if (!(trial < P.lm_max_iterations)) return finish(kOutOfTrials);
        if (!solve_damped(H, b, lam, delta)) return finish(kNotPositiveDefinite);
        double E[16];
        se3_exp(delta, E);
        mul_rigid(E, T, Tn);
        state = kTrial;
        ask(Tn, false);
        return true;
    }

    bool finish(Exit why)
    {
        memcpy(res.T, T, sizeof T);
        res.error = e; res.lambda = lam; res.n_pairs_last = pairs;
        state = kDone; exit = why;
        return false;
    }
};

// One run with its evaluations answered on the spot: eval(T, with_hessian, out[29]) -> 0 or an error code (returned at once)
template <class Eval>
int lm_optimise(Eval&& eval, const double T0[16], const LmParams& P, LmResult* res)
{
    LmStepper lm;
    double out[kOut];
    lm.start(T0, P);
    do {
        if (const int rc = eval(lm.req_T, lm.req_hessian, out)) return rc;
    } while (lm.feed(out));
    *res = lm.res;
    return 0;
}

}  // namespace vgicp_host
}  // namespace lisreg
