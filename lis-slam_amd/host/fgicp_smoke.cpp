// fgicp_smoke.cpp — FastGicpRegistration of the host mirror (plain g++, no HIP headers) as select_registration_method("FAST_GICP") sets
// it up (src/core/registration.cpp:157-166): a floor, two walls and six poles, the source a subsample moved by the inverse of a known pose.
// With a GPU: aligns from the identity and checks the pose, the pcl::Registration surface and the setters.  Without a GPU: verifies the
// loud failure path (no CPU fallback) and exits 0.
#include <cmath>
#include <cstdio>
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
    for (int i = 0; i < 12000; ++i) {            // floor z = 0, wall x = 10, wall y = -8
        const float u = U(rng) * 40 - 20, v = U(rng) * 40 - 20, h = U(rng) * 6;
        add(map, u + N(rng), v + N(rng), N(rng));
        if (i % 2 == 0) add(map, 10 + N(rng), v + N(rng), h);
        else add(map, u + N(rng), -8 + N(rng), h);
    }
    const float poles[6][2] = { { 3, 4 }, { -5, 6 }, { 7, -3 }, { -6, -4 }, { 1, -6 }, { -2, 9 } };
    for (int i = 0; i < 3000; ++i) { const int k = i % 6; const float a = U(rng) * 6.2831853f; add(map, poles[k][0] + 0.1f * std::cos(a) + N(rng), poles[k][1] + 0.1f * std::sin(a) + N(rng), U(rng) * 5); }
    const float yaw = 0.03f, tx = 0.2f, ty = -0.15f, tz = 0.05f, cy = std::cos(yaw), sy = std::sin(yaw);
    for (size_t i = 0; i < map.size(); i += 5) {
        const PointType& p = map.points[i];
        const float x = p.x - tx, y = p.y - ty;
        add(scan, cy * x + sy * y, -sy * x + cy * y, p.z - tz);
    }
    Scan2SubMapRegistration<> reg(Variant::Odom);
    bool ok = true;
    FastGicpRegistration<PointType> gicp(reg.handle(), 0, 3);
    gicp.setTransformationEpsilon(0.01);         // the block of registration.cpp:157-166
    gicp.setMaximumIterations(50);
    gicp.setMaxCorrespondenceDistance(5.0);
    gicp.setCorrespondenceRandomness(20);
    gicp.setInputTarget(map);
    gicp.setInputSource(&scan);
    PointCloud<PointType> out;
    gicp.align(out);
    const float* F = gicp.getFinalTransformation();
    std::printf("FastGICP: target of %d points (search grid %d x %d x %d), converged=%d iterations=%d evaluations=%d rejected=%d pairs=%lld "
                "error=%g fitness=%g t=[%g %g %g] yaw=%g\n", gicp.info().n_points, gicp.info().grid_dims[0], gicp.info().grid_dims[1],
                gicp.info().grid_dims[2], (int)gicp.hasConverged(), gicp.getFinalNumIteration(), gicp.result().n_evals, gicp.result().n_rejected,
                gicp.result().n_pairs_last, gicp.result().error, gicp.getFitnessScore(), F[3], F[7], F[11], std::atan2(F[4], F[0]));
    ok = ok && gicp.hasConverged() && out.size() == scan.size() && gicp.info().n_points == (int)map.size();
    ok = ok && std::fabs(F[3] - tx) < 2e-2f && std::fabs(F[7] - ty) < 2e-2f && std::fabs(F[11] - tz) < 2e-2f && std::fabs(std::atan2(F[4], F[0]) - yaw) < 5e-3f;
    ok = ok && gicp.getFitnessScore() < 1e-2 && gicp.result().n_pairs_last == (long long)scan.size();
    // a cut-off below the displacement leaves fewer pairs at the guess (no iteration: the pairs reported are those of the first
    // linearisation); a randomness the library refuses is reported, not swallowed
    gicp.setMaxCorrespondenceDistance(0.05);
    gicp.setMaximumIterations(0);
    PointCloud<PointType> out2;
    gicp.align(out2);
    std::printf("FastGICP with a 0.05 m cut-off at the guess: pairs=%lld iterations=%d\n", gicp.result().n_pairs_last, gicp.getFinalNumIteration());
    ok = ok && gicp.result().n_pairs_last < (long long)scan.size() && gicp.getFinalNumIteration() == 0 && !gicp.hasConverged();
    bool refused = false;
    try { gicp.setCorrespondenceRandomness(3); } catch (const RegistrationError& e) { refused = e.code == LISREG_ERR_ARG; }
    ok = ok && refused;
    if (!ok) { std::printf("ERROR: fgicp_smoke failed\n"); return 1; }
    std::printf("fgicp_smoke ok\n");
    return 0;
}
