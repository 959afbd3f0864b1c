// lisreg_gicp_stepper.hpp — the outer loop of PCL's GICP (computeTransformation; tests/gicp_ref.py: align), the only one in csrc/: the
// state of one run that asks for the 74 moments of one outer iteration at a time and is resumed with them, the way LmStepper
// (lisreg_lm_stepper.hpp) and NdtStepper (lisreg_ndt_stepper.hpp) hold the loops of their families.  A batch driver holds many runs and
// answers the outstanding requests of all of them with one round of launches (lisreg_batch_driver.hpp); the single
// aligner answers them one by one (gicp_closed_loop below).  The inner minimisation, the Euler algebra and the end rule's distance are
// lisreg_gicp_host.hpp's: nothing of them is written a second time here.  host/gicp_stepper_check.cpp holds the same loop written out
// and compares the two on scripted records.  Plain C++, no device code.  Not installed.
#pragma once
#include "lisreg_gicp_host.hpp"

namespace lisreg {
namespace gicp_host {

struct GicpLoopParams {
    BfgsParams B;
    double     rotation_epsilon, transformation_epsilon;
    int        max_iters;
};
template <class Params>
inline GicpLoopParams gicp_loop_params_of(const Params& P)
{
    return GicpLoopParams{ bfgs_params_of(P), P.rotation_epsilon, P.transformation_epsilon, P.max_iters };
}

// what lisreg_gicp_result holds, in double and int
struct GicpLoopResult {
    double    T[16];
    int       converged, iters, inner_iters, n_evals, n_rounds, inner_exit;
    long long n_pairs_last;
    double    error, last_delta;
};
template <class Result>
inline void gicp_result_to(const GicpLoopResult& lr, Result* res)
{
    memset(res, 0, sizeof *res);
    memcpy(res->final_transform, lr.T, sizeof lr.T);
    res->converged = lr.converged; res->iters = lr.iters; res->inner_iters = lr.inner_iters; res->n_evals = lr.n_evals;
    res->n_rounds = lr.n_rounds; res->inner_exit = lr.inner_exit; res->n_pairs_last = lr.n_pairs_last;
    res->error = lr.error; res->last_delta = lr.last_delta;
}

struct GicpStepper {
    // the outstanding request: the search and the moments at req_T = X(x) G.  Every request is of one kind (the batch driver sorts
    // requests by req_hessian: all of GICP's sit in the first group)
    double                req_T[16];
    static constexpr bool req_hessian = true;
    GicpLoopResult        res;        // complete once feed() has returned false

    // G: the guess matrix; centre: the point the target's moments are taken about
    void start(const double G0[16], const GicpLoopParams& params, const double centre[3])
    {
        P = params;
        memcpy(G, G0, sizeof G);
        memcpy(c, centre, sizeof c);
        for (int k = 0; k < 6; ++k) x[k] = 0.0;
        memset(&res, 0, sizeof res);
        res.inner_exit = -1;
        done = false;
        pose_of_state(x, G, req_T);
    }

    bool finished() const { return done; }

    // the answer to the outstanding request; true: there is a next request, false: the run is finished and res is filled
    bool feed(const double rec[kRec])
    {
        if (done) return false;
        ++res.n_rounds;
        res.n_pairs_last = (long long)rec[73];
        if (rec[73] < 4.0) {                                        // PCL's "need at least 4 points": not converged, the pose of this round
            res.error = rec[73] > 0.0 ? rec[0] / rec[73] : 0.0;
            return finish();
        }
        double xn[6];
        memcpy(xn, x, sizeof x);
        InnerCounts cnt;
        const double f = inner(rec, c, xn, P.B, &cnt);
        const double delta = outer_delta(x, xn, P.rotation_epsilon, P.transformation_epsilon);
        memcpy(x, xn, sizeof x);
        ++res.iters;
        res.inner_iters += cnt.iters;
        res.n_evals += cnt.n_f + cnt.n_df;
        res.error = f; res.last_delta = delta; res.inner_exit = cnt.exit;
        if (res.iters >= P.max_iters || delta < 1.0) {              // both ends count as converged (PCL 1.8)
            res.converged = 1;
            return finish();
        }
        pose_of_state(x, G, req_T);
        return true;
    }

private:
    GicpLoopParams P;
    double G[16], c[3], x[6];
    bool   done = true;

    bool finish()
    {
        pose_of_state(x, G, res.T);
        done = true;
        return false;
    }
};

// One run with its rounds answered on the spot: eval(T, rec[74]) -> 0 or an error code (returned at once)
template <class Eval>
int gicp_closed_loop(Eval&& eval, const double G[16], const GicpLoopParams& P, const double centre[3], GicpLoopResult* res)
{
    GicpStepper st;
    double rec[kRec];
    st.start(G, P, centre);
    do {
        if (const int rc = eval(st.req_T, rec)) return rc;
    } while (st.feed(rec));
    *res = st.res;
    return 0;
}

}  // namespace gicp_host
}  // namespace lisreg
