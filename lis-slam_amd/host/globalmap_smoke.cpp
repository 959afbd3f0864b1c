// globalmap_smoke.cpp — publishGlobalMap() and SubMap::merged() of the host mirror (plain g++, no HIP headers) against the per-class calls
// they replace: for every submap and class, lisreg_localmap_get + transformPointCloud, concatenated on the host.  Bit for bit.
// With a GPU: four small submaps (one of them empty), the map with and without the newest submap, the loop-verification target and
// laserCloudFromPre of one submap.  Without a GPU: verifies the loud failure path (no CPU fallback) and exits 0.
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <vector>

#include "lis_slam_registration.hpp"

using namespace lis_slam;

// class k of a submap as the per-class path delivers it: the 16-byte records out of the store, as PointXYZIL, moved by `pose`
static PointCloud<PointXYZIL> class_cloud(lisreg_ctx* ctx, int id, int k, const float* pose)
{
    int n = 0;
    lisreg_localmap_get(ctx, id, k, nullptr, 0, &n);
    std::vector<float> rec((size_t)n * 4 + 4);
    if (lisreg_localmap_get(ctx, id, k, rec.data(), n, &n) != LISREG_OK) throw RegistrationError(LISREG_ERR_ARG, lisreg_last_error(ctx));
    PointCloud<PointXYZIL> c;
    for (int i = 0; i < n; ++i) {
        PointXYZIL p{};
        p.x = rec[4 * (size_t)i]; p.y = rec[4 * (size_t)i + 1]; p.z = rec[4 * (size_t)i + 2];
        uint32_t w; std::memcpy(&w, &rec[4 * (size_t)i + 3], 4);
        p.label = (uint16_t)w;
        c.push_back(p);
    }
    return pose && n > 0 ? transformPointCloud(ctx, c, pose) : c;
}

static bool same(const PointCloud<PointXYZIL>& a, const PointCloud<PointXYZIL>& b, const char* what)
{
    if (a.size() != b.size()) { std::printf("ERROR %s: %zu points, expected %zu\n", what, a.size(), b.size()); return false; }
    if (a.size() && std::memcmp(a.points.data(), b.points.data(), a.size() * sizeof(PointXYZIL)) != 0) {
        std::printf("ERROR %s: the clouds differ\n", what);
        return false;
    }
    return true;
}

int main()
{
    if (lisreg_device_count() == 0) {
        try { Scan2SubMapRegistration<PointXYZIL> reg(Variant::SubMap); }
        catch (const RegistrationError& e) { std::printf("no HIP device: constructor failed loudly as designed (%d: %s)\n", e.code, e.what()); return 0; }
        std::printf("ERROR: context creation succeeded without a device\n");
        return 1;
    }
    Scan2SubMapRegistration<PointXYZIL> reg(Variant::SubMap);
    lisreg_ctx* ctx = reg.handle();
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> U(-40.f, 40.f);
    const int counts[4][5] = { { 300, 65, 1000, 257, 40 }, { 0, 0, 0, 0, 0 }, { 1, 256, 0, 700, 63 }, { 500, 0, 900, 64, 255 } };
    const float poses[4][6] = { { 0.01f, -0.02f, 0.5f, 10.f, -20.f, 0.3f }, { 0.f, 0.f, 1.f, 50.f, 60.f, 0.f },
                                { -0.03f, 0.02f, -2.8f, -120.f, 80.f, 1.5f }, { 0.02f, 0.01f, 3.1f, 300.f, -450.f, -2.f } };
    std::vector<std::unique_ptr<SubMap<>>> owned;
    std::map<int, SubMap<>*> subMapInfo;
    for (int m = 0; m < 4; ++m) {
        owned.emplace_back(new SubMap<>(ctx, 20 + m));
        PointCloud<PointXYZIL> down[5];
        for (int k = 0; k < 5; ++k)
            for (int i = 0; i < counts[m][k]; ++i) {
                PointXYZIL p{};
                p.x = U(rng); p.y = U(rng); p.z = 0.1f * U(rng); p.label = (uint16_t)(rng() % 20);
                down[k].push_back(p);
            }
        owned.back()->fisrt_submap(down, poses[m]);
        subMapInfo[m] = owned.back().get();
    }
    bool ok = true;
    for (int finish = 0; finish < 2; ++finish) {
        PointCloud<PointXYZIL> map, want;
        publishGlobalMap(ctx, subMapInfo, finish != 0, map);
        for (int m = 0; m < (finish ? 4 : 3); ++m)
            for (int k = 0; k < 5; ++k) {
                const PointCloud<PointXYZIL> c = class_cloud(ctx, 20 + m, k, poses[m]);
                want.points.insert(want.points.end(), c.points.begin(), c.points.end());
            }
        ok = same(map, want, finish ? "publishGlobalMap(FINISHMAP)" : "publishGlobalMap") && ok;
        std::printf("global map of %d submaps: %zu points\n", finish ? 4 : 3, map.size());
    }
    {   // the loop-verification target (:2787-2790): dynamic + pole + ground + building in the submap's own frame
        PointCloud<PointXYZIL> got, want;
        subMapInfo[2]->merged(LISREG_CLS_DYNAMIC | LISREG_CLS_POLE | LISREG_CLS_GROUND | LISREG_CLS_BUILDING, nullptr, got);
        for (int k = 0; k < 4; ++k) { const auto c = class_cloud(ctx, 22, k, nullptr); want.points.insert(want.points.end(), c.points.begin(), c.points.end()); }
        ok = same(got, want, "merged(15, own frame)") && ok;
    }
    {   // laserCloudFromPre (:1151-1154): the pole class under the submap pose
        PointCloud<PointXYZIL> got;
        subMapInfo[2]->merged(LISREG_CLS_POLE, subMapInfo[2]->submap_pose_6D_optimized, got);
        ok = same(got, class_cloud(ctx, 22, 1, poses[2]), "merged(pole, submap pose)") && ok;
    }
    if (!ok) return 1;
    std::printf("globalmap_smoke ok\n");
    return 0;
}
