// gicp_smoke.cpp — GicpRegistration of the host mirror (plain g++, no HIP headers) as select_registration_method("GICP") sets it up
// (src/core/registration.cpp:137-146): a floor, two walls and six poles, the source a subsample moved by the inverse of a known pose.
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
    GicpRegistration<PointType> gicp(reg.handle(), 0, 3);
    gicp.setMaxCorrespondenceDistance(10);       // the block of registration.cpp:137-146
    gicp.setMaximumIterations(30);
    gicp.setTransformationEpsilon(1e-6);
    gicp.setEuclideanFitnessEpsilon(1e-3);
    gicp.setRANSACIterations(0);
    gicp.setInputTarget(map);
    gicp.setInputSource(&scan);
    PointCloud<PointType> out;
    gicp.align(out);
    const float* F = gicp.getFinalTransformation();
    const lisreg_gicp_result& r = gicp.result();
    std::printf("GICP: target of %d points (search grid %d x %d x %d), converged=%d outer=%d inner=%d evaluations=%d rounds=%d pairs=%lld "
                "error=%g delta=%g inner_exit=%d fitness=%g t=[%g %g %g] yaw=%g\n", gicp.info().n_points, gicp.info().grid_dims[0],
                gicp.info().grid_dims[1], gicp.info().grid_dims[2], (int)gicp.hasConverged(), gicp.getFinalNumIteration(), r.inner_iters, r.n_evals,
                r.n_rounds, r.n_pairs_last, r.error, r.last_delta, r.inner_exit, gicp.getFitnessScore(), F[3], F[7], F[11], std::atan2(F[4], F[0]));
    ok = ok && gicp.hasConverged() && out.size() == scan.size() && gicp.info().n_points == (int)map.size();
    ok = ok && std::fabs(F[3] - tx) < 2e-2f && std::fabs(F[7] - ty) < 2e-2f && std::fabs(F[11] - tz) < 2e-2f && std::fabs(std::atan2(F[4], F[0]) - yaw) < 5e-3f;
    ok = ok && gicp.getFitnessScore() < 1e-2 && r.n_pairs_last == (long long)scan.size();
    ok = ok && r.n_rounds == r.iters && r.iters >= 1 && r.iters <= 30 && r.inner_iters >= r.iters && r.n_evals >= 2 * r.inner_iters;
    // one outer iteration is the cap: converged all the same (PCL 1.8); a cut-off that leaves no pair is PCL's "need at least 4 points":
    // not converged, the guess, one round and no iteration; a randomness the library refuses is reported, not swallowed
    gicp.setMaximumIterations(1);
    PointCloud<PointType> out2;
    gicp.align(out2);
    std::printf("GICP with one outer iteration: converged=%d outer=%d rounds=%d delta=%g\n", (int)gicp.hasConverged(), gicp.getFinalNumIteration(),
                gicp.result().n_rounds, gicp.result().last_delta);
    ok = ok && gicp.hasConverged() && gicp.getFinalNumIteration() == 1 && gicp.result().n_rounds == 1 && gicp.result().last_delta >= 1.0;
    gicp.setMaxCorrespondenceDistance(1e-4);
    gicp.align(out2);
    std::printf("GICP with a 0.1 mm cut-off at the guess: pairs=%lld converged=%d outer=%d rounds=%d\n", gicp.result().n_pairs_last,
                (int)gicp.hasConverged(), gicp.getFinalNumIteration(), gicp.result().n_rounds);
    F = gicp.getFinalTransformation();
    ok = ok && gicp.result().n_pairs_last < 4 && !gicp.hasConverged() && gicp.getFinalNumIteration() == 0 && gicp.result().n_rounds == 1 &&
         gicp.result().inner_exit == -1 && F[0] == 1.f && F[3] == 0.f && F[5] == 1.f;
    bool refused = false;
    try { gicp.setCorrespondenceRandomness(3); } catch (const RegistrationError& e) { refused = e.code == LISREG_ERR_ARG; }
    ok = ok && refused;
    if (!ok) { std::printf("ERROR: gicp_smoke failed\n"); return 1; }
    std::printf("gicp_smoke ok\n");
    return 0;
}
