// gicp_stepper_check.cpp — the resumable outer loop of PCL's GICP (../csrc/lisreg_gicp_stepper.hpp) against the same loop
// written out below, on its own: plain C++, no library, no device.  A script is a random pair set with random positive definite M, a
// guess matrix, a parameter set and a schedule that says how many of the pairs each round sees; the record source answers a request
// pose T with the 74 moments of those pairs at T, formed here in plain loops (as host/gicp_bfgs_check.cpp forms them).  GicpStepper is
// driven from that source request by request, gicp_closed_loop in one go, and the plain loop computes what lisreg_gicp_align computed
// before the stepper existed.  Every request pose and every field of the final result must be equal bit for bit, and every way out of
// the loop must occur: delta < 1, the max_iters cap (with max_iters 1 and 3), fewer than 4 pairs in the first round and in a later one.
// Prints a census; exit 0 and "gicp_stepper_check ok" if everything holds.  An argument sets the number of scripts (default 100).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "lisreg_gicp_stepper.hpp"

using namespace lisreg::gicp_host;

namespace {

struct Pair { double p[3], q[3], M[6]; };
enum Exit { kDelta, kCap1, kCap3, kCapOther, kFewFirst, kFewLater, kExits };
const char* const kExitNames[kExits] = { "delta", "cap1", "cap3", "cap_other", "few_first", "few_later" };

struct Script {
    std::vector<Pair> pairs;
    std::vector<int>  seen;        // pairs the record of round r is made of (the last entry holds for every later round)
    double G[16], c[3];
    GicpLoopParams P;
};

int failures = 0;
void expect(bool ok, const char* what, int script, double a = 0.0, double b = 0.0)
{
    if (!ok) { ++failures; std::printf("FAILED: script %d: %s (%.17g, %.17g)\n", script, what, a, b); }
}

// the record of the first m pairs at the pose T (row-major 4 x 4), about c — the order of tests/gicp_ref.py
void moments_at(const Script& S, int round, const double T[16], double rec[kRec])
{
    const int m = S.seen[(size_t)std::min(round, (int)S.seen.size() - 1)];
    for (int k = 0; k < kRec; ++k) rec[k] = 0.0;
    for (int i = 0; i < m; ++i) {
        const Pair& Q = S.pairs[(size_t)i];
        double xp[3], yt[4], r[3], Mr[3];
        for (int a = 0; a < 3; ++a) xp[a] = ((T[4 * a] * Q.p[0] + T[4 * a + 1] * Q.p[1]) + T[4 * a + 2] * Q.p[2]) + T[4 * a + 3];
        for (int a = 0; a < 3; ++a) { yt[a] = xp[a] - S.c[a]; r[a] = xp[a] - Q.q[a]; }
        yt[3] = 1.0;
        for (int a = 0; a < 3; ++a) Mr[a] = (Q.M[kSym3[a][0]] * r[0] + Q.M[kSym3[a][1]] * r[1]) + Q.M[kSym3[a][2]] * r[2];
        rec[0] += (r[0] * Mr[0] + r[1] * Mr[1]) + r[2] * Mr[2];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 4; ++b) rec[1 + 4 * a + b] += Mr[a] * yt[b];
        for (int p = 0; p < 6; ++p)
            for (int b = 0; b < 4; ++b)
                for (int b2 = b; b2 < 4; ++b2) rec[13 + 10 * p + kSym4[b][b2]] += Q.M[p] * (yt[b] * yt[b2]);
        rec[73] += 1.0;
    }
}

// computeTransformation written out: what lisreg_gicp_align ran before GicpStepper.  poses: every pose a round searched at
Exit plain_loop(const Script& S, std::vector<double>* poses, GicpLoopResult* out_res)
{
    double T[16], rec[kRec];
    double x[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    GicpLoopResult out;
    memset(&out, 0, sizeof out);
    out.inner_exit = -1;
    Exit how;
    for (;;) {
        pose_of_state(x, S.G, T);
        poses->insert(poses->end(), T, T + 16);
        moments_at(S, out.n_rounds, T, rec);
        ++out.n_rounds;
        out.n_pairs_last = (long long)rec[73];
        if (rec[73] < 4.0) {
            out.error = rec[73] > 0.0 ? rec[0] / rec[73] : 0.0;
            how = out.n_rounds == 1 ? kFewFirst : kFewLater;
            break;
        }
        double xn[6];
        memcpy(xn, x, sizeof x);
        InnerCounts cnt;
        const double f = inner(rec, S.c, xn, S.P.B, &cnt);
        const double delta = outer_delta(x, xn, S.P.rotation_epsilon, S.P.transformation_epsilon);
        memcpy(x, xn, sizeof x);
        ++out.iters;
        out.inner_iters += cnt.iters;
        out.n_evals += cnt.n_f + cnt.n_df;
        out.error = f; out.last_delta = delta; out.inner_exit = cnt.exit;
        if (out.iters >= S.P.max_iters || delta < 1.0) {
            out.converged = 1;
            how = delta < 1.0 ? kDelta : S.P.max_iters == 1 ? kCap1 : S.P.max_iters == 3 ? kCap3 : kCapOther;
            break;
        }
    }
    pose_of_state(x, S.G, out.T);
    *out_res = out;
    return how;
}

bool same_result(const GicpLoopResult& a, const GicpLoopResult& b)
{
    return !memcmp(a.T, b.T, sizeof a.T) && a.converged == b.converged && a.iters == b.iters && a.inner_iters == b.inner_iters &&
           a.n_evals == b.n_evals && a.n_rounds == b.n_rounds && a.inner_exit == b.inner_exit && a.n_pairs_last == b.n_pairs_last &&
           !memcmp(&a.error, &b.error, sizeof a.error) && !memcmp(&a.last_delta, &b.last_delta, sizeof a.last_delta);
}

}  // namespace

int main(int argc, char** argv)
{
    const int n_scripts = argc > 1 ? std::atoi(argv[1]) : 100;
    const BfgsParams B0{ 0.01, 0.01, 9.0, 0.05, 0.5, 0.01, 1.0e-2, 3, 20 };
    std::mt19937_64 rng(20261);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    long census[kExits] = {};
    long rounds = 0;
    int most_rounds = 0;
    for (int s = 0; s < n_scripts; ++s) {
        Script S;
        const int m = 40 + 23 * (s % 17);
        const double noise = s % 3 == 0 ? 0.0 : 0.02;
        const double truth[6] = { 0.3 * U(rng), 0.3 * U(rng), 0.1 * U(rng), 0.03 * U(rng), 0.03 * U(rng), 0.05 * U(rng) };
        double Rt[9];
        euler_R(truth, Rt);
        S.pairs.resize((size_t)m);
        for (Pair& Q : S.pairs) {
            for (int a = 0; a < 3; ++a) Q.p[a] = (a == 2 ? 3.0 : 25.0) * U(rng) + (a == 0 ? 40.0 : 0.0);
            for (int a = 0; a < 3; ++a) Q.q[a] = ((Rt[3 * a] * Q.p[0] + Rt[3 * a + 1] * Q.p[1]) + Rt[3 * a + 2] * Q.p[2]) + truth[a] + noise * N(rng);
            double n[3] = { N(rng), N(rng), N(rng) };               // M of a random plane normal: eigenvalues 0.5, 0.5, 500
            const double nn = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            for (int a = 0; a < 3; ++a) n[a] /= nn;
            int k = 0;
            for (int a = 0; a < 3; ++a)
                for (int b = a; b < 3; ++b) Q.M[k++] = 0.5 * ((a == b ? 1.0 : 0.0) + 999.0 * n[a] * n[b]);
        }
        for (int a = 0; a < 3; ++a) S.c[a] = (a == 0 ? 40.0 : 0.0) + 2.0 * U(rng);
        // the guess: the identity for every fourth script, a small rigid motion otherwise (rounded to float, as a caller's guess is)
        const double gx[6] = { 0.1 * U(rng), 0.1 * U(rng), 0.05 * U(rng), 0.01 * U(rng), 0.01 * U(rng), 0.02 * U(rng) };
        const double zero[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        state_matrix(s % 4 == 0 ? zero : gx, S.G);
        for (int k = 0; k < 16; ++k) S.G[k] = (double)(float)S.G[k];
        S.P = GicpLoopParams{ B0, 2.0e-3, 1.0e-4, 30 };
        S.seen.assign(1, m);
        switch (s % 5) {
        case 0: S.P.max_iters = 1; break;
        case 1: S.P.max_iters = 3; S.P.transformation_epsilon = 1.0e-13; S.P.rotation_epsilon = 1.0e-13; break;
        case 2: S.P.transformation_epsilon = s % 2 ? 1.0e-6 : 1.0e-4; break;
        case 3: S.seen.assign(1, (s / 5) % 4); break;              // 0 .. 3 pairs in the first round
        default:                                                    // fewer than 4 pairs in the second or third round, the loop still running
            S.P.transformation_epsilon = 1.0e-13; S.P.rotation_epsilon = 1.0e-13;
            S.seen.assign((size_t)(1 + (s / 5) % 2), m);
            S.seen.push_back((s / 10) % 4);
            break;
        }
        if (s % 7 == 6) S.P.B.max_inner_iters = 3;

        std::vector<double> want_poses, got_poses;
        GicpLoopResult want, closed;
        const Exit how = plain_loop(S, &want_poses, &want);
        ++census[how];
        rounds += want.n_rounds;
        most_rounds = std::max(most_rounds, want.n_rounds);

        // the stepper, request by request
        GicpStepper st;
        expect(st.finished(), "a stepper that was never started is not finished", s);
        st.start(S.G, S.P, S.c);
        double rec[kRec];
        int round = 0;
        bool more = true;
        while (more) {
            expect(!st.finished() && st.req_hessian, "finished before feed() said so", s, round);
            got_poses.insert(got_poses.end(), st.req_T, st.req_T + 16);
            moments_at(S, round, st.req_T, rec);
            more = st.feed(rec);
            ++round;
            if (round > 1000) { expect(false, "the stepper does not end", s); break; }
        }
        expect(st.finished(), "not finished after feed() returned false", s);
        expect(round == want.n_rounds, "rounds", s, round, want.n_rounds);
        expect(got_poses.size() == want_poses.size() && !memcmp(got_poses.data(), want_poses.data(), sizeof(double) * want_poses.size()),
               "the request poses differ from the plain loop's", s);
        expect(same_result(st.res, want), "the result differs from the plain loop's", s, st.res.error, want.error);
        const GicpLoopResult kept = st.res;
        expect(!st.feed(rec) && same_result(st.res, kept), "feed() after the end changed the result", s);

        // the closed loop over the stepper, as lisreg_gicp_align calls it
        int asked = 0;
        const int rc = gicp_closed_loop([&](const double T[16], double out[kRec]) { moments_at(S, asked++, T, out); return 0; }, S.G, S.P, S.c, &closed);
        expect(rc == 0 && asked == want.n_rounds && same_result(closed, want), "gicp_closed_loop differs from the plain loop", s, asked);
        // an evaluation that fails ends the closed loop at once with its code
        if (want.n_rounds >= 2) {
            asked = 0;
            const int rc2 = gicp_closed_loop([&](const double T[16], double out[kRec]) { if (asked == 1) return -7; moments_at(S, asked++, T, out); return 0; },
                                             S.G, S.P, S.c, &closed);
            expect(rc2 == -7 && asked == 1, "a failing evaluation did not end the closed loop", s, rc2, asked);
        }
    }
    std::printf("census over %d scripts (%ld rounds, at most %d in one):", n_scripts, rounds, most_rounds);
    for (int e = 0; e < kExits; ++e) std::printf(" %s=%ld", kExitNames[e], census[e]);
    std::printf("\n");
    if (n_scripts >= 60)
        for (int e : { (int)kDelta, (int)kCap1, (int)kCap3, (int)kFewFirst, (int)kFewLater }) {
            if (census[e] < 1) { ++failures; std::printf("FAILED: the exit %s never occurred\n", kExitNames[e]); }
        }
    if (failures) { std::printf("ERROR: gicp_stepper_check failed (%d)\n", failures); return 1; }
    std::printf("gicp_stepper_check ok\n");
    return 0;
}
