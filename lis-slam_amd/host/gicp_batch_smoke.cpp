// gicp_batch_smoke.cpp — GicpVerifier of the host mirror (plain g++, no HIP headers): the candidate loop of
// detectLoopClosureForSubMap (src/node/subMapOptmizationNode.cpp:2779-2846) as one call, with the verifier of
// select_registration_method("GICP") (src/core/registration.cpp:137-146).  Three candidate submaps (the true one, the same one shifted
// by 0.4 m, one 200 m away) and one key-frame cloud.  With a GPU: alignAll() must give every candidate the result a GicpRegistration
// gives it alone, byte for byte, a fitness score close to that path's float one, and best() the candidate the loop's test keeps; the
// candidate 200 m away finds no pair, which PCL's GICP calls not converged.  Without a GPU: verifies the loud failure path (no CPU
// fallback) and exits 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "lis_slam_registration.hpp"

using namespace lis_slam;

static void add(PointCloud<PointType>& c, float x, float y, float z) { PointType p{}; p.x = x; p.y = y; p.z = z; c.push_back(p); }

int main()
{
    if (lisreg_device_count() == 0) {
        try { Scan2SubMapRegistration<> reg(Variant::Odom); }
        catch (const RegistrationError& e) { std::printf("no HIP device: constructor failed loudly as designed (%d: %s)\n", e.code, e.what()); return 0; }
        std::printf("ERROR: context creation succeeded without a device\n");
        return 1;
    }
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> U(0.f, 1.f);
    std::normal_distribution<float> N(0.f, 0.01f);
    PointCloud<PointType> map, scan;
    for (int i = 0; i < 6000; ++i) {             // floor z = 0, wall x = 10, wall y = -8
        const float u = U(rng) * 40 - 20, v = U(rng) * 40 - 20, h = U(rng) * 6;
        add(map, u + N(rng), v + N(rng), N(rng));
        if (i % 2 == 0) add(map, 10 + N(rng), v + N(rng), h);
        else add(map, u + N(rng), -8 + N(rng), h);
    }
    const float poles[6][2] = { { 3, 4 }, { -5, 6 }, { 7, -3 }, { -6, -4 }, { 1, -6 }, { -2, 9 } };
    for (int i = 0; i < 1500; ++i) { const int k = i % 6; const float a = U(rng) * 6.2831853f; add(map, poles[k][0] + 0.1f * std::cos(a) + N(rng), poles[k][1] + 0.1f * std::sin(a) + N(rng), U(rng) * 5); }
    const float yaw = 0.03f, tx = 0.2f, ty = -0.15f, tz = 0.05f, cy = std::cos(yaw), sy = std::sin(yaw);
    for (size_t i = 0; i < map.size(); i += 5) {
        const PointType& p = map.points[i];
        const float x = p.x - tx, y = p.y - ty;
        add(scan, cy * x + sy * y, -sy * x + cy * y, p.z - tz);
    }
    PointCloud<PointType> shifted = map, far = map;
    for (auto& p : shifted.points) { p.x += 0.4f; p.z += 0.05f * std::sin(p.y); }      // a neighbouring submap: close, and bent
    for (auto& p : far.points) p.x += 200.f;
    Scan2SubMapRegistration<> reg(Variant::Odom);
    bool ok = true;
    const PointCloud<PointType>* maps[3] = { &shifted, &map, &far };
    const float eye[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    GicpVerifier<PointType> ver(reg.handle());
    ver.setTransformationEpsilon(1e-4);          // the settings of subMapOptmizationNode.cpp:2765-2769 read for GICP
    ver.setMaximumIterations(30);
    for (int k = 0; k < 3; ++k) { ver.setCandidateTarget(k, *maps[k]); ver.addCandidate(k, k == 1 ? nullptr : eye); }
    ver.alignAll(scan);
    std::printf("GicpVerifier: %zu candidates, %d rounds, %d source distributions, best %d\n", ver.size(), ver.info().n_rounds,
                ver.info().n_sources_staged, ver.best());
    ok = ok && ver.best() == 1 && ver.info().n_sources_staged == 1 && ver.size() == 3;
    int max_rounds = 0;
    for (int k = 0; k < 3; ++k) {
        // the loop as the reference writes it: one registration per candidate
        GicpRegistration<PointType> one(reg.handle(), 10 + k, 3);
        one.setTransformationEpsilon(1e-4);
        one.setMaximumIterations(30);
        one.setInputTarget(*maps[k]);
        one.setInputSource(&scan);
        PointCloud<PointType> out;
        one.align(out, k == 1 ? nullptr : eye);
        const lisreg_gicp_result &a = ver.result(k), &b = one.result();
        const bool same = !std::memcmp(&a, &b, sizeof a);
        // getFitnessScore of the single path is a float search of the float-transformed cloud: close to the batch's double score, not equal
        const double fa = ver.fitness(k), fb = one.getFitnessScore();
        std::printf("candidate %d: converged=%d outer=%d rounds=%d evaluations=%d pairs=%lld fitness=%.6g (single path %.6g) same as alone: %d\n", k,
                    a.converged, a.iters, a.n_rounds, a.n_evals, a.n_pairs_last, fa, fb, (int)same);
        ok = ok && same && std::fabs(fa - fb) <= 1e-3 * fb + 1e-7;
        max_rounds = a.n_rounds > max_rounds ? a.n_rounds : max_rounds;
    }
    ok = ok && ver.info().n_rounds == max_rounds && ver.hasConverged(1) && !ver.hasConverged(2) && ver.result(2).n_rounds == 1 && ver.result(2).iters == 0;
    ok = ok && ver.fitness(1) < 1e-2 && ver.fitness(1) < ver.fitness(0) && ver.fitness(2) > 100.0;
    const double* F = ver.result(1).final_transform;
    ok = ok && std::fabs(F[3] - tx) < 2e-2 && std::fabs(F[7] - ty) < 2e-2 && std::fabs(F[11] - tz) < 2e-2 && std::fabs(std::atan2(F[4], F[0]) - yaw) < 5e-3;
    // no candidate: nothing to align, no winner; a slot without a target is reported, not swallowed
    ver.clearCandidates();
    ver.alignAll(scan);
    ok = ok && ver.best() == -1 && ver.size() == 0;
    ver.addCandidate(777, nullptr);
    bool refused = false;
    try { ver.alignAll(scan); } catch (const RegistrationError& e) { refused = e.code == LISREG_ERR_ARG; }
    ok = ok && refused;
    if (!ok) { std::printf("ERROR: gicp_batch_smoke failed\n"); return 1; }
    std::printf("gicp_batch_smoke ok\n");
    return 0;
}
