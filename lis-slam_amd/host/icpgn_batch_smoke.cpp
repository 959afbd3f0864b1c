// icpgn_batch_smoke.cpp — IcpGnVerifier of the host mirror (plain g++, no HIP headers): the candidate loop of
// detectLoopClosureForSubMapICP (src/node/subMapOptmizationNode.cpp:2496-2621) as one call, with its `static OptimizedICPGN
// myICP(30, 10)` (src/core/registration.cpp:19-115).  Three candidate submaps (the true one, the same one shifted by 0.4 m, one 1 000 m
// away) and one key-frame cloud.  With a GPU: matchAll() must give every candidate the result an OptimizedICPGN gives it alone, byte
// for byte, and best() the candidate the loop's test keeps; the candidate 1 000 m away finds no correspondence and applies no step.
// Without a GPU: verifies the loud failure path (no CPU fallback) and exits 0.
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
    for (auto& p : far.points) p.x += 1000.f;
    Scan2SubMapRegistration<> reg(Variant::Odom);
    bool ok = true;
    const PointCloud<PointType>* maps[3] = { &shifted, &map, &far };
    const float eye[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    IcpGnVerifier<PointType> ver(reg.handle(), 30, 10.f);      // myICP(30, 10)
    for (int k = 0; k < 3; ++k) { ver.setCandidateTarget(20 + k, *maps[k]); ver.addCandidate(20 + k, k == 1 ? nullptr : eye); }
    ver.matchAll(scan);
    std::printf("IcpGnVerifier: %zu candidates, %d host synchronisations, %d source staged, best %d\n", ver.size(), ver.info().n_syncs,
                ver.info().n_sources_staged, ver.best());
    ok = ok && ver.best() == 1 && ver.info().n_sources_staged == 1 && ver.info().n_syncs == 1 && ver.size() == 3;
    for (int k = 0; k < 3; ++k) {
        // the loop as the reference writes it: one match per candidate
        OptimizedICPGN<PointType> one(reg.handle(), 30 + k, 30, 10.f);
        one.SetTargetCloud(*maps[k]);
        PointCloud<PointType> out;
        float pose[16];
        one.Match(scan, eye, out, pose);
        const lisreg_icpgn_result& a = ver.result(k);
        const float fit = one.GetFitnessScore();
        const bool same = !std::memcmp(a.final_transform, pose, sizeof pose) && !std::memcmp(&a.fitness, &fit, sizeof fit);
        std::printf("candidate %d: steps=%d correspondences=%d fitness=%.6g same as alone: %d\n", k, a.steps_applied, a.n_corr_last, (double)a.fitness, (int)same);
        ok = ok && same && ver.hasConverged(k);
    }
    ok = ok && ver.result(1).steps_applied == 30 && ver.result(2).steps_applied == 0 && ver.result(2).n_corr_last == 0;
    // (sanity only: thirty point-to-point steps from 0.2 m / 0.03 rad off end near the pose, not at it)
    ok = ok && ver.fitness(1) < 0.05f && ver.fitness(1) < ver.fitness(0) && ver.fitness(2) > 1e5f;
    const float* F = ver.result(1).final_transform;
    ok = ok && std::fabs(F[3] - tx) < 0.1 && std::fabs(F[7] - ty) < 0.1 && std::fabs(F[11] - tz) < 0.1 && std::fabs(std::atan2(F[4], F[0]) - yaw) < 0.02;
    // no candidate: nothing to match, no winner; a slot without a map index is reported, not swallowed
    ver.clearCandidates();
    ver.matchAll(scan);
    ok = ok && ver.best() == -1 && ver.size() == 0;
    ver.addCandidate(777, nullptr);
    bool refused = false;
    try { ver.matchAll(scan); } catch (const RegistrationError& e) { refused = e.code == LISREG_ERR_NO_TARGET; }
    ok = ok && refused;
    if (!ok) { std::printf("ERROR: icpgn_batch_smoke failed\n"); return 1; }
    std::printf("icpgn_batch_smoke ok\n");
    return 0;
}
