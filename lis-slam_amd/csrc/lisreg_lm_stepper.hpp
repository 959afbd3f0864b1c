// lisreg_lm_stepper.hpp — lm_optimise (lisreg_vgicp_host.hpp) turned inside out: the state of one Levenberg-Marquardt run that asks for
// one evaluation at a time and is resumed with its answer, so that a driver can hold many runs and answer the outstanding requests of
// all of them with one round of launches (lisreg_fgicp_batch.hip).  Fed the out[29] records lm_optimise's eval would
// return, it asks for the same (T, with_hessian) sequence and fills the same LmResult, bit for bit: every statement below is the one of
// lm_optimise at the same place of the loop, only the loop counters live in the struct.  Plain C++ (no HIP).  Not installed.
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

}  // namespace vgicp_host
}  // namespace lisreg
