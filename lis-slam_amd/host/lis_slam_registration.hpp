// lis_slam_registration.hpp — C++ host-side mirror of the reference's scan-to-submap interface, above the C ABI.
//
// The reference has no library seam for this path: three node classes each own a private
// scan2SubMapOptimization() that talks to ~15 member variables.  This header keeps their names
// and meaning so a maintainer can swap each body for one call:
//   OdomEstimationNode      /root/reference/src/node/odomEstimationNode.cpp:29-97 (members), :596-626 (driver)
//   SubMapOdometryNode      src/node/subMapOptmizationNode.cpp:151-203, :1509-1541
//   SubMapOptmizationNode   src/node/subMapOptmizationNode.cpp:3302-3333, :4485-4540
// plus POD mirrors of the message surface (msg/cloud_info.msg, msg/semantic_info.msg) and a PointCloud2
// byte-layout view, because ROS/PCL are not part of this build.  Header-only, C++17, no dependencies.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/lisreg.h"

namespace lis_slam {

// ---- point types (src/include/common.h:9,25-35): 32 bytes, 16-byte aligned, PCL_ADD_POINT4D + intensity -------
struct alignas(16) PointXYZI  { float x, y, z, _pad0; float intensity; float _pad1[3]; };
struct alignas(16) PointXYZIL { float x, y, z, _pad0; float intensity; uint16_t label; uint16_t _pad1; float _pad2[2]; };
static_assert(sizeof(PointXYZI) == 32 && sizeof(PointXYZIL) == 32, "PCL point layout");
using PointType = PointXYZI;                       // typedef pcl::PointXYZI PointType (common.h:9)

template <class P> struct PointCloud {             // the slice of pcl::PointCloud<P> the path touches
    std::vector<P> points;
    size_t size() const { return points.size(); }
    void clear() { points.clear(); }
    void push_back(const P& p) { points.push_back(p); }
};

// ---- sensor_msgs/PointCloud2 byte-layout view: pass a ROS message buffer straight through ---------------------
struct PointCloud2View {
    const uint8_t* data = nullptr;
    uint32_t width = 0, height = 1, point_step = 32;
    int off_x = 0, off_y = 4, off_z = 8, off_intensity = 16, off_label = -1;   // field offsets by name
    size_t size() const { return (size_t)width * height; }
    int fmt() const { return off_label >= 0 ? LISREG_FMT_XYZIL : LISREG_FMT_XYZI; }
};

// ---- msg/cloud_info.msg:1-25 and msg/semantic_info.msg:1-34 (scalars + the clouds the path reads) --------------
struct cloud_info {
    bool  imuAvailable = false, odomAvailable = false;
    float imuRollInit = 0, imuPitchInit = 0, imuYawInit = 0;
    float initialGuessX = 0, initialGuessY = 0, initialGuessZ = 0;
    float initialGuessRoll = 0, initialGuessPitch = 0, initialGuessYaw = 0;
    PointCloud2View cloud_deskewed, cloud_corner, cloud_surface, cloud_corner_sharp, cloud_surface_sharp;
};
struct semantic_info : cloud_info {
    PointCloud2View semantic_raw, semantic_dynamic, semantic_pole, semantic_ground, semantic_building, semantic_outlier;
};

enum class Variant { Odom = LISREG_VARIANT_ODOM, KeyFrame = LISREG_VARIANT_KEYFRAME, SubMap = LISREG_VARIANT_SUBMAP };

class RegistrationError : public std::runtime_error { public: int code; RegistrationError(int c, const std::string& m) : std::runtime_error(m), code(c) {} };

// One instance per reference node class (each owns a lisreg context = its own HIP stream; #2 and #3 run
// concurrently in one process, subMapOptmizationNode.cpp:5188-5195).
template <class PointT = PointType>
class Scan2SubMapRegistration {
public:
    // members the reference's callers read after the call (odomEstimationNode.cpp:66-71)
    float transformTobeMapped[6] = { 0, 0, 0, 0, 0, 0 };
    bool  isDegenerate = false;
    float deltaR = 100, deltaT = 100;
    int   iterCount = 0;
    int   laserCloudSelNum = 0;
    lisreg_params params;

    explicit Scan2SubMapRegistration(Variant v, int device = 0) {
        lisreg_default_params((int)v, &params);
        int rc = lisreg_create(device, &ctx_);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(nullptr));
    }
    ~Scan2SubMapRegistration() { lisreg_destroy(ctx_); }
    Scan2SubMapRegistration(const Scan2SubMapRegistration&) = delete;
    Scan2SubMapRegistration& operator=(const Scan2SubMapRegistration&) = delete;

    // kdtreeCornerFromMap->setInputCloud(...); kdtreeSurfFromMap->setInputCloud(...)   (:602-603)
    void setInputTarget(const PointCloud<PointT>& laserCloudCornerFromMapDS, const PointCloud<PointT>& laserCloudSurfFromMapDS) {
        check(lisreg_set_target(ctx_, laserCloudCornerFromMapDS.points.data(), (int)laserCloudCornerFromMapDS.size(),
                                laserCloudSurfFromMapDS.points.data(), (int)laserCloudSurfFromMapDS.size(),
                                (int)sizeof(PointT), fmt()));
    }
    // submap API (subMap.h:435-777): corner = pole; surf = ground + building + dynamic (:1408-1419)
    void setInputTargetFromClasses(const PointCloud<PointT>& pole, const PointCloud<PointT>& ground,
                                   const PointCloud<PointT>& building, const PointCloud<PointT>& dynamic) {
        check(lisreg_target_from_classes(ctx_, 0, pole.points.data(), (int)pole.size(), ground.points.data(), (int)ground.size(),
                                         building.points.data(), (int)building.size(), dynamic.points.data(), (int)dynamic.size(),
                                         (int)sizeof(PointT), fmt()));
    }

    // The body of scan2SubMapOptimization() (:596-626): guard, GN loop, transformUpdate.  Returns the lisreg
    // status: LISREG_OK, LISREG_NOT_ENOUGH_FEATURES (the reference's ROS_WARN branch, pose untouched) or
    // LISREG_TOO_FEW_CORRESPONDENCES.  transformTobeMapped is in/out exactly like the member.
    int scan2SubMapOptimization(const PointCloud<PointT>& laserCloudCornerLastDS, const PointCloud<PointT>& laserCloudSurfLastDS,
                                const cloud_info& cloudInfo) {
        lisreg_imu imu{ cloudInfo.imuAvailable ? 1 : 0, cloudInfo.imuRollInit, cloudInfo.imuPitchInit };
        lisreg_stats st{};
        int rc = lisreg_align(ctx_, laserCloudCornerLastDS.points.data(), (int)laserCloudCornerLastDS.size(),
                              laserCloudSurfLastDS.points.data(), (int)laserCloudSurfLastDS.size(), (int)sizeof(PointT), fmt(),
                              &params, &imu, transformTobeMapped, &st);
        if (rc < 0) throw RegistrationError(rc, lisreg_last_error(ctx_));
        iterCount = st.iters; laserCloudSelNum = st.n_corr_last;
        if (rc != LISREG_NOT_ENOUGH_FEATURES) { isDegenerate = st.degenerate != 0; deltaR = st.deltaR; deltaT = st.deltaT; }
        return rc;
    }
    // same, reading the feature clouds straight out of PointCloud2 message buffers
    int scan2SubMapOptimization(const PointCloud2View& corner, const PointCloud2View& surf, const cloud_info& cloudInfo) {
        lisreg_imu imu{ cloudInfo.imuAvailable ? 1 : 0, cloudInfo.imuRollInit, cloudInfo.imuPitchInit };
        lisreg_stats st{};
        int rc = lisreg_align(ctx_, corner.data, (int)corner.size(), surf.data, (int)surf.size(), (int)corner.point_step, corner.fmt(),
                              &params, &imu, transformTobeMapped, &st);
        if (rc < 0) throw RegistrationError(rc, lisreg_last_error(ctx_));
        iterCount = st.iters; laserCloudSelNum = st.n_corr_last;
        if (rc != LISREG_NOT_ENOUGH_FEATURES) { isDegenerate = st.degenerate != 0; deltaR = st.deltaR; deltaT = st.deltaT; }
        return rc;
    }
    // subMap2SubMapOptimization() of SubMapOptmizationNode is the same call with Variant::SubMap (:4485-4540)
    int subMap2SubMapOptimization(const PointCloud<PointT>& c, const PointCloud<PointT>& s, const cloud_info& ci) { return scan2SubMapOptimization(c, s, ci); }

    // the same with the sources already in HBM as 16-byte records (what SubMap<>::extractSubMapCloud and the device-resident maps hand over)
    int subMap2SubMapOptimization(const lisreg_submap_extract_out& x, const cloud_info& cloudInfo) {
        lisreg_imu imu{ cloudInfo.imuAvailable ? 1 : 0, cloudInfo.imuRollInit, cloudInfo.imuPitchInit };
        lisreg_stats st{};
        int rc = lisreg_align(ctx_, x.src_corner, x.n_src_corner, x.src_surf, x.n_src_surf, 16, LISREG_FMT_DEVICE, &params, &imu, transformTobeMapped, &st);
        if (rc < 0) throw RegistrationError(rc, lisreg_last_error(ctx_));
        iterCount = st.iters; laserCloudSelNum = st.n_corr_last;
        if (rc != LISREG_NOT_ENOUGH_FEATURES) { isDegenerate = st.degenerate != 0; deltaR = st.deltaR; deltaT = st.deltaT; }
        return rc;
    }

    lisreg_ctx* handle() { return ctx_; }

private:
    static constexpr int fmt() { return std::is_same<PointT, PointXYZIL>::value ? LISREG_FMT_XYZIL : LISREG_FMT_XYZI; }
    void check(int rc) { if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_)); }
    lisreg_ctx* ctx_ = nullptr;
};

// ---- the pcl::VoxelGrid surface the nodes use ------------------------------------------------------
// downSizeFilterCorner / downSizeFilterSurf (odomEstimationNode.cpp:34-35, 110-111, 196-201, 272-277) and
// voxel_downsample_pcl (src/include/subMap.h:1207-1249) call exactly setLeafSize / setInputCloud / filter.
// Shares the registration object's context (and stream), so down-sampling and registration stay ordered.
template <class PointT = PointType>
class VoxelGrid {
public:
    explicit VoxelGrid(lisreg_ctx* ctx) : ctx_(ctx) {}
    void setLeafSize(float lx, float ly, float lz) {
        if (lx != ly || ly != lz) throw RegistrationError(LISREG_ERR_ARG, "VoxelGrid: the reference only uses cubic leaves");
        leaf_ = lx;
    }
    void setInputCloud(const PointCloud<PointT>* cloud) { input_ = cloud; }
    // returns LISREG_OK or LISREG_LEAF_TOO_SMALL (PCL's warning case: output = input)
    int filter(PointCloud<PointT>& output) {
        if (!input_) throw RegistrationError(LISREG_ERR_ARG, "VoxelGrid: no input cloud");
        std::vector<PointT> tmp(input_->size());
        int n_out = 0;
        const int fmt = std::is_same<PointT, PointXYZIL>::value ? LISREG_FMT_XYZIL : LISREG_FMT_XYZI;
        int rc = lisreg_voxel_downsample(ctx_, input_->points.data(), (int)input_->size(), (int)sizeof(PointT), fmt, leaf_,
                                         tmp.data(), (int)tmp.size(), &n_out);
        if (rc < 0) throw RegistrationError(rc, lisreg_last_error(ctx_));
        tmp.resize((size_t)n_out);
        output.points.swap(tmp);
        return rc;
    }
private:
    lisreg_ctx* ctx_;
    const PointCloud<PointT>* input_ = nullptr;
    float leaf_ = 0.4f;
};

// transformPointCloud(cloudIn, &pose6D) (src/core/common.cpp:130-173); pose = {roll, pitch, yaw, x, y, z}
template <class PointT>
inline PointCloud<PointT> transformPointCloud(lisreg_ctx* ctx, const PointCloud<PointT>& cloudIn, const float pose[6]) {
    PointCloud<PointT> out;
    out.points.resize(cloudIn.size());
    const int fmt = std::is_same<PointT, PointXYZIL>::value ? LISREG_FMT_XYZIL : LISREG_FMT_XYZI;
    int rc = lisreg_transform_cloud(ctx, cloudIn.points.data(), (int)cloudIn.size(), (int)sizeof(PointT), fmt, pose, out.points.data());
    if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx));
    return out;
}

// ---- the producer of cloud_info ------------------------------------------------------------------------
// PointXYZIRT (src/include/common.h:12-23) and the part of LaserProcessing that turns one sweep into the five clouds of
// cloud_info (src/core/laserProcessing.cpp:467-713: projectPointCloud, cloudExtraction, calculateSmoothness,
// markOccludedPoints, extractFeatures), without the IMU de-skew.
struct alignas(16) PointXYZIRT { float x, y, z, _pad0; float intensity; uint16_t ring; uint16_t _pad1; float time; float _pad2; };
static_assert(sizeof(PointXYZIRT) == 32, "PCL point layout");

struct ExtractedFeatures {             // what assignCouldInfo/publishClouds put into cloud_info (:718-760)
    PointCloud<PointXYZIRT> extractedCloud, cornerCloud, surfaceCloud, sharpCornerCloud, SharpSurfaceCloud;
};

class LaserProcessing {
public:
    lisreg_feature_params params;
    // de-skew state, named as in src/include/laserProcessing.h:105-123
    std::vector<double> imuTime, imuRotX, imuRotY, imuRotZ;
    int    imuPointerCur = 0;
    int    deskewFlag = 1;                  // 1: the cloud has a `time` channel (:158-170)
    bool   imuAvailable = false;            // cloudInfo.imuAvailable
    double timeScanCur = 0.0;
    explicit LaserProcessing(lisreg_ctx* ctx) : ctx_(ctx) { lisreg_default_feature_params(&params); }
    // imuDeskewInfo (laserProcessing.cpp:222-266): integrate the angular velocities of the IMU messages around this scan.
    // stamp[i], (ang_x, ang_y, ang_z)[i] = header stamp and ros-frame angular velocity of message i (after imuConverter).
    void imuDeskewInfo(const double* stamp, const double* ang_x, const double* ang_y, const double* ang_z, int n, double scanCur, double scanEnd) {
        timeScanCur = scanCur; imuAvailable = false; imuPointerCur = 0;
        imuTime.assign((size_t)n + 1, 0.0); imuRotX.assign((size_t)n + 1, 0.0); imuRotY.assign((size_t)n + 1, 0.0); imuRotZ.assign((size_t)n + 1, 0.0);
        for (int i = 0; i < n; ++i) {
            const double t = stamp[i];
            if (t > scanEnd + 0.01) break;
            if (imuPointerCur == 0) { imuRotX[0] = imuRotY[0] = imuRotZ[0] = 0; imuTime[0] = t; ++imuPointerCur; continue; }
            const double dt = t - imuTime[(size_t)imuPointerCur - 1];
            imuRotX[(size_t)imuPointerCur] = imuRotX[(size_t)imuPointerCur - 1] + ang_x[i] * dt;
            imuRotY[(size_t)imuPointerCur] = imuRotY[(size_t)imuPointerCur - 1] + ang_y[i] * dt;
            imuRotZ[(size_t)imuPointerCur] = imuRotZ[(size_t)imuPointerCur - 1] + ang_z[i] * dt;
            imuTime[(size_t)imuPointerCur] = t;
            ++imuPointerCur;
        }
        --imuPointerCur;
        if (imuPointerCur <= 0) return;
        imuAvailable = true;
    }
    ExtractedFeatures process(const PointCloud<PointXYZIRT>& laserCloudIn) {
        ExtractedFeatures f;
        const size_t cap = (size_t)params.n_scan * (size_t)params.horizon_scan;
        PointCloud<PointXYZIRT>* clouds[5] = { &f.extractedCloud, &f.cornerCloud, &f.surfaceCloud, &f.sharpCornerCloud, &f.SharpSurfaceCloud };
        for (auto* c : clouds) c->points.resize(cap);
        lisreg_feature_out o{};
        o.deskewed = f.extractedCloud.points.data();       o.cap_deskewed = (int)cap;
        o.corner = f.cornerCloud.points.data();            o.cap_corner = (int)cap;
        o.surface = f.surfaceCloud.points.data();          o.cap_surface = (int)cap;
        o.corner_sharp = f.sharpCornerCloud.points.data(); o.cap_corner_sharp = (int)cap;
        o.surface_sharp = f.SharpSurfaceCloud.points.data(); o.cap_surface_sharp = (int)cap;
        lisreg_deskew dk{};
        dk.enabled = (deskewFlag == 1 && imuAvailable) ? 1 : 0;       // deskewPoint :429
        dk.imu_pointer_cur = imuPointerCur; dk.imu_time = imuTime.data(); dk.imu_rot_x = imuRotX.data(); dk.imu_rot_y = imuRotY.data();
        dk.imu_rot_z = imuRotZ.data(); dk.time_scan_cur = timeScanCur;
        int rc = lisreg_extract_features_deskew(ctx_, laserCloudIn.points.data(), (int)laserCloudIn.size(), (int)sizeof(PointXYZIRT),
                                                LISREG_FMT_XYZIRT, &params, &dk, &o);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
        const int n[5] = { o.n_deskewed, o.n_corner, o.n_surface, o.n_corner_sharp, o.n_surface_sharp };
        for (int k = 0; k < 5; ++k) clouds[k]->points.resize((size_t)n[k]);
        return f;
    }
    // the throughput form: n_sweeps sweeps of device records, each with its own de-skew (deskews[s].time_device: the sweep's device
    // times, e.g. lisreg_pretreat_batch's; deskews == nullptr: none), into the caller's device buffers; the counts come back in outs
    void processBatch(int n_sweeps, const void* const* sweeps, const int* n, const lisreg_deskew* deskews, lisreg_feature_out* outs) {
        const int rc = lisreg_extract_features_deskew_batch(ctx_, n_sweeps, sweeps, n, &params, deskews, outs);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
    }
private:
    lisreg_ctx* ctx_;
};

// ---- laser pretreatment: the node in front of LaserProcessing -------------------------------------------------------------
// LaserPretreatment (src/include/laserPretreatment.h:57-69, src/core/laserPretreatment.cpp:4-161): a raw sweep (PointIn: x y z + float i
// at byte 16, the layout of pcl::PointXYZI) becomes PointXYZIRT — non-finite and out-of-range points dropped, ring from the elevation
// angle with the N_SCAN 16 / 32 / 64 table, time from the azimuth.  N_SCAN, lidarMinRange and lidarMaxRange are ParamServer members in
// the reference; here they are `params`.
using PointIn = PointXYZI;
class LaserPretreatment {
public:
    lisreg_pretreat_params params;
    float startOri = 0.f, endOri = 0.f;     // of the last sweep
    int   halfIndex = -1;                   // output index of the point at which halfPassed became true, -1 if never
    explicit LaserPretreatment(lisreg_ctx* ctx) : ctx_(ctx) { lisreg_default_pretreat_params(&params); }
    PointCloud<PointXYZIRT> Pretreatment(const PointCloud<PointIn>& cloudIn) {
        return run(cloudIn.points.data(), (int)cloudIn.size(), (int)sizeof(PointIn), LISREG_FMT_XYZI);
    }
    // the same for a packed buffer of x y z intensity floats (a KITTI velodyne file, a PointCloud2 with point_step 16)
    PointCloud<PointXYZIRT> Pretreatment(const float* xyzi, int n) { return run(xyzi, n, 16, LISREG_FMT_XYZI_PACKED); }
private:
    PointCloud<PointXYZIRT> run(const void* cloud, int n, int stride, int fmt) {
        PointCloud<PointXYZIRT> out;
        out.points.resize((size_t)n);
        lisreg_pretreat_out o{};
        o.cloud = out.points.data(); o.capacity = n;
        const int rc = lisreg_pretreat(ctx_, cloud, n, stride, fmt, &params, &o);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
        out.points.resize((size_t)o.n);
        startOri = o.start_ori; endOri = o.end_ori; halfIndex = o.half_index;
        return out;
    }
    lisreg_ctx* ctx_;
};

// ---- motion compensation: the stage between LaserPretreatment and FeatureExtraction ----------------------------------------------------
// DistortionAdjust (src/core/distortionAdjust.cpp:412-480): SetMotionInfo keeps the scan period and the velocity, AdjustCloud drops point
// 0 and moves every other point by the constant-velocity model at its own time.  The deques and their synchronisation (SyncData,
// TransformCoordinate, NED2ENU) stay with the node; which velocity to pass is the caller's choice (the reference's deskewInfo takes
// vel_data_.front() of a deque it never pops, :245).
struct VelocityData { double linear_velocity[3] = { 0, 0, 0 }, angular_velocity[3] = { 0, 0, 0 }; };
class DistortionAdjust {
public:
    lisreg_motion motion;
    explicit DistortionAdjust(lisreg_ctx* ctx) : ctx_(ctx) { lisreg_default_motion(&motion); }
    void SetMotionInfo(float scan_period, const VelocityData& velocity_data) {
        motion.scan_period = scan_period;
        for (int k = 0; k < 3; ++k) { motion.linear_velocity[k] = velocity_data.linear_velocity[k]; motion.angular_velocity[k] = velocity_data.angular_velocity[k]; }
    }
    PointCloud<PointXYZIRT> AdjustCloud(const PointCloud<PointXYZIRT>& cloudIn) {
        PointCloud<PointXYZIRT> out;
        const int n = (int)cloudIn.size();
        out.points.resize((size_t)(n > 1 ? n - 1 : 0));
        lisreg_adjust_out o{};
        o.cloud = out.points.data(); o.capacity = (int)out.points.size();
        const int rc = lisreg_adjust_cloud(ctx_, cloudIn.points.data(), n, (int)sizeof(PointXYZIRT), LISREG_FMT_XYZIRT, nullptr, &motion, &o);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
        out.points.resize((size_t)o.n);
        return out;
    }
    // n_sweeps sweeps of device records with their device times (lisreg_pretreat_batch's outputs), one motion each, in one launch;
    // outs[s].cloud / time_device / capacity are the caller's device buffers, outs[s].n comes back
    void AdjustCloudBatch(int n_sweeps, const void* const* sweeps, const int* n, const float* const* time_device, const lisreg_motion* motions,
                          lisreg_adjust_out* outs) {
        const int rc = lisreg_adjust_cloud_batch(ctx_, n_sweeps, sweeps, n, time_device, motions, outs);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
    }
private:
    lisreg_ctx* ctx_;
};

// ---- RangeNet++ around the network: the semantic labeller --------------------------------------------------------------------
// RangenetAPI (src/include/rangenetAPI.h:16-68, src/core/rangenetAPI.cpp) without the network: infer() projects the sweep into the
// network's 5 x H x W input tensor, hands tensor and logits to the caller's model as DEVICE pointers, and labels the points from the
// logits — nothing crosses the link but the valid-pixel count.  The model is a callable `void(const float* tensor, float* logits)` that
// has finished writing `logits` (n_classes x H x W floats) when it returns.  This header has no HIP dependency, so the node — which
// owns a HIP runtime for its model anyway — provides the device memory: the sweep as lisreg_dpoint records with the float intensity in
// the payload (lisreg_upload_cloud with LISREG_FMT_XYZI_PACKED, or the output of lisreg_extract_features*), and the workspace below.
// The RGB clouds of the reference's class are not mirrored.  With use_knn set, the labels come from lisreg_rangenet_label_knn — the kNN
// clean-up of RangeNet++, with `knn` taken from the `post: KNN: params:` block of the model's arch_cfg.yaml — instead of the plain argmax.
struct RangenetWorkspace {              // caller-owned device memory for sweeps of up to max_points points
    float*         tensor = nullptr;    // 5 * H * W floats
    float*         logits = nullptr;    // n_classes * H * W floats
    unsigned char* invalid_mask = nullptr;   // H * W bytes
    unsigned char* label_image = nullptr;    // H * W bytes, or NULL
    int*           pixel_index = nullptr;    // max_points ints
    void*          labelled = nullptr;       // max_points lisreg_dpoint records: getLabelPointCloud() on the device
    int            max_points = 0;
};
class RangenetAPI {
public:
    lisreg_rangenet_params params;
    lisreg_rangenet_knn_params knn;     // read only when use_knn is set
    bool use_knn = false;
    int validPixels = 0;                // of the last sweep
    RangenetAPI(lisreg_ctx* ctx, const RangenetWorkspace& ws) : ctx_(ctx), ws_(ws) {
        lisreg_default_rangenet_params(&params);
        lisreg_default_rangenet_knn_params(&knn);
    }
    // infer (rangenetAPI.cpp:16-125): returns the labelled device records (ws.labelled; x y z bit for bit, label in the payload) —
    // what lisreg_semantic_split takes with LISREG_FMT_DEVICE
    template <class Network>
    const void* infer(const void* currentCloudInDevice, int num_points, Network&& network) {
        if (num_points > ws_.max_points) throw RegistrationError(LISREG_ERR_ARG, "RangenetAPI::infer: the workspace is too small");
        lisreg_rangenet_out o{};
        o.tensor = ws_.tensor; o.invalid_mask = ws_.invalid_mask; o.pixel_index = ws_.pixel_index;
        int rc = lisreg_rangenet_project(ctx_, currentCloudInDevice, num_points, 16, LISREG_FMT_DEVICE_XYZI, &params, &o);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
        validPixels = o.n_valid;
        network(static_cast<const float*>(ws_.tensor), ws_.logits);
        rc = use_knn ? lisreg_rangenet_label_knn(ctx_, currentCloudInDevice, num_points, LISREG_FMT_DEVICE_XYZI, ws_.pixel_index, ws_.invalid_mask,
                                                 ws_.logits, &params, &knn, ws_.labelled, ws_.label_image)
                     : lisreg_rangenet_label(ctx_, currentCloudInDevice, num_points, LISREG_FMT_DEVICE_XYZI, ws_.pixel_index, ws_.invalid_mask,
                                             ws_.logits, &params, ws_.labelled, ws_.label_image);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
        num_points_ = num_points;
        return ws_.labelled;
    }
    const void* getLabelPointCloud() const { return ws_.labelled; }
    int size() const { return num_points_; }
private:
    lisreg_ctx* ctx_;
    RangenetWorkspace ws_;
    int num_points_ = 0;
};

// ---- the compute steps of SubMapManager (src/include/subMap.h) ---------------------------------------------
struct bounds_t { double min_x, min_y, min_z, max_x, max_y, max_z; };     // src/include/subMap.h:32-39
struct centerpoint_t { double x, y, z; };                                  // src/include/subMap.h:11-16

// pcl::search::KdTree<PointT> as SubMapManager uses it (setInputCloud once, k = 1 queries): an HBM-resident grid index.
template <class PointT>
class SearchTree {
public:
    SearchTree(lisreg_ctx* ctx, int slot) : ctx_(ctx), slot_(slot) {}
    void setInputCloud(const PointCloud<PointT>& cloud) {
        int rc = lisreg_map_index_set(ctx_, slot_, cloud.points.data(), (int)cloud.size(), (int)sizeof(PointT), fmt());
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
    }
    int slot() const { return slot_; }
    lisreg_ctx* ctx() const { return ctx_; }
    static int fmt() { return std::is_same<PointT, PointXYZIL>::value ? LISREG_FMT_XYZIL : LISREG_FMT_XYZI; }
private:
    lisreg_ctx* ctx_;
    int slot_;
};

template <class PointT>
class SubMapManager {
public:
    explicit SubMapManager(lisreg_ctx* ctx) : ctx_(ctx) {}
    // subMap.h:131-163
    void get_cloud_bbx(const PointCloud<PointT>& cloud, bounds_t& bound) {
        double b[6];
        check(lisreg_cloud_bounds(ctx_, cloud.points.data(), (int)cloud.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(), b));
        bound = { b[0], b[1], b[2], b[3], b[4], b[5] };
    }
    // subMap.h:173-181 (host arithmetic)
    static void get_intersection_bbx(const bounds_t& a, const bounds_t& b, bounds_t& out, float pad = 2.0f) {
        out.min_x = std::max(a.min_x, b.min_x) - pad; out.min_y = std::max(a.min_y, b.min_y) - pad; out.min_z = std::max(a.min_z, b.min_z) - pad;
        out.max_x = std::min(a.max_x, b.max_x) + pad; out.max_y = std::min(a.max_y, b.max_y) + pad; out.max_z = std::min(a.max_z, b.max_z) + pad;
    }
    // subMap.h:123-128 get_bound_cpt and :214-228 transform_bbx (host arithmetic; transCur = row-major 3x4 [R|t] in float, the
    // products are float x double like Eigen::Affine3f(i, j) * double in the reference)
    static void get_bound_cpt(const bounds_t& b, centerpoint_t& cp) { cp = { 0.5 * (b.min_x + b.max_x), 0.5 * (b.min_y + b.max_y), 0.5 * (b.min_z + b.max_z) }; }
    static void transform_bbx(const bounds_t& bound_in, const centerpoint_t& cp_in, bounds_t& bound_out, centerpoint_t& cp_out, const float transCur[12]) {
        const bounds_t b = bound_in; const centerpoint_t c = cp_in;
        cp_out.x = transCur[0] * c.x + transCur[1] * c.y + transCur[2] * c.z + transCur[3];
        cp_out.y = transCur[4] * c.x + transCur[5] * c.y + transCur[6] * c.z + transCur[7];
        cp_out.z = transCur[8] * c.x + transCur[9] * c.y + transCur[10] * c.z + transCur[11];
        bound_out.max_x = b.max_x - c.x + cp_out.x; bound_out.max_y = b.max_y - c.y + cp_out.y; bound_out.max_z = b.max_z - c.z + cp_out.z;
        bound_out.min_x = b.min_x - c.x + cp_out.x; bound_out.min_y = b.min_y - c.y + cp_out.y; bound_out.min_z = b.min_z - c.z + cp_out.z;
    }
    // subMap.h:1124-1152
    bool bbx_filter(PointCloud<PointT>& cloud_in_out, const bounds_t& bbx, bool delete_box = false) {
        const double b[6] = { bbx.min_x, bbx.min_y, bbx.min_z, bbx.max_x, bbx.max_y, bbx.max_z };
        int n_out = 0;
        check(lisreg_bbx_filter(ctx_, cloud_in_out.points.data(), (int)cloud_in_out.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(), b,
                                delete_box ? 1 : 0, cloud_in_out.points.data(), &n_out));
        cloud_in_out.points.resize((size_t)n_out);
        return true;
    }
    // subMap.h:1064-1100; returns false (cloud untouched) for <= 10 points like the reference
    bool map_scan_feature_pts_distance_removal(PointCloud<PointT>& feature_pts, const SearchTree<PointT>& map_kdtree, float center_radius,
                                               float dynamic_dist_thre_min = 3.402823466e38f, float dynamic_dist_thre_max = 3.402823466e38f,
                                               float near_dist_thre = 0.0f) {
        int n_out = 0;
        int rc = lisreg_dynamic_filter(ctx_, map_kdtree.slot(), feature_pts.points.data(), (int)feature_pts.size(), (int)sizeof(PointT),
                                       SearchTree<PointT>::fmt(), center_radius, dynamic_dist_thre_min, dynamic_dist_thre_max, near_dist_thre,
                                       feature_pts.points.data(), &n_out);
        if (rc < 0) throw RegistrationError(rc, lisreg_last_error(ctx_));
        feature_pts.points.resize((size_t)n_out);
        return rc == LISREG_OK;
    }
private:
    void check(int rc) { if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_)); }
    lisreg_ctx* ctx_;
};

// ---- pcl::IterativeClosestPoint as the loop-closure code uses it --------------------------------------------
// (src/node/subMapOptmizationNode.cpp:2763-2833: setters, setInputTarget, setInputSource, align, getFitnessScore, hasConverged,
// getFinalTransformation).  Like the reference's `static` objects, an instance carries correspondences_prev_mse_ across align().
template <class PointT>
class IterativeClosestPoint {
public:
    IterativeClosestPoint(lisreg_ctx* ctx, int slot) : tree_(ctx, slot) { lisreg_icp_default_params(0, &prm_); prm_.max_corr_dist = 1.3407807929942596e154; /* sqrt(DBL_MAX), PCL's default */ prm_.max_iters = 10; prm_.transformation_epsilon = 0; prm_.euclidean_fitness_epsilon = -1.7976931348623157e308; }
    void setMaxCorrespondenceDistance(double d) { prm_.max_corr_dist = d; }
    void setMaximumIterations(int n) { prm_.max_iters = n; }
    void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
    void setEuclideanFitnessEpsilon(double e) { prm_.euclidean_fitness_epsilon = e; }
    void setRANSACIterations(int n) { if (n != 0) throw RegistrationError(LISREG_ERR_ARG, "ICP: the reference runs with 0 RANSAC iterations"); }
    void setInputTarget(const PointCloud<PointT>& cloud) { tree_.setInputCloud(cloud); }
    void setInputSource(const PointCloud<PointT>* cloud) { source_ = cloud; }
    void align(PointCloud<PointT>& output, const float* guess = nullptr) {
        if (!source_) throw RegistrationError(LISREG_ERR_ARG, "ICP: no input source");
        output.points.resize(source_->size());
        int rc = lisreg_icp_align(tree_.ctx(), tree_.slot(), source_->points.data(), (int)source_->size(), (int)sizeof(PointT),
                                  SearchTree<PointT>::fmt(), &prm_, guess, &res_, output.points.data());
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(tree_.ctx()));
        prm_.prev_mse = res_.prev_mse;
    }
    bool hasConverged() const { return res_.converged != 0; }
    double getFitnessScore() const { return res_.fitness; }
    const float* getFinalTransformation() const { return res_.final_transform; }     // row-major 4x4
    int nr_iterations() const { return res_.iters; }
private:
    SearchTree<PointT> tree_;
    const PointCloud<PointT>* source_ = nullptr;
    lisreg_icp_params prm_{};
    lisreg_icp_result res_{};
};

// ---- pcl::NormalDistributionsTransform as select_registration_method("NDT") sets it up -------------------------
// (src/core/registration.cpp:147-155; subMapOptmizationNode.cpp:2756-2760: epsilon 0.01, step size 0.1, resolution 1.0, 35 iterations),
// with the pcl::Registration surface the loop-closure code uses.  ndt_slot: the NDT target slot; map_slot: a map-index slot of the same
// target for getFitnessScore (mean squared k = 1 distance of the aligned source, unbounded like PCL's default).
template <class PointT>
class NdtRegistration {
public:
    NdtRegistration(lisreg_ctx* ctx, int ndt_slot, int map_slot) : tree_(ctx, map_slot), ndt_slot_(ndt_slot) { lisreg_ndt_default_params(0, &prm_); }
    void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
    void setStepSize(double s) { prm_.step_size = s; }
    void setResolution(float r) { prm_.resolution = r; if (target_) setInputTarget(*target_); }
    void setMaximumIterations(int n) { prm_.max_iters = n; }
    void setOulierRatio(double o) { prm_.outlier_ratio = o; }          // PCL's spelling
    void setLineSearch(bool more_thuente) { prm_.line_search = more_thuente ? 1 : 0; }
    void setInputTarget(const PointCloud<PointT>& cloud) {
        target_ = &cloud;
        check(lisreg_ndt_set_target(tree_.ctx(), ndt_slot_, cloud.points.data(), (int)cloud.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(), &prm_, &info_));
        tree_.setInputCloud(cloud);
    }
    void setInputSource(const PointCloud<PointT>* cloud) { source_ = cloud; }
    void align(PointCloud<PointT>& output, const float* guess = nullptr) {
        if (!source_) throw RegistrationError(LISREG_ERR_ARG, "NDT: no input source");
        output.points.resize(source_->size());
        check(lisreg_ndt_align(tree_.ctx(), ndt_slot_, source_->points.data(), (int)source_->size(), (int)sizeof(PointT),
                               SearchTree<PointT>::fmt(), &prm_, guess, &res_, output.points.data()));
        std::vector<int> idx(output.size());
        std::vector<float> d2(output.size());
        check(lisreg_nearest(tree_.ctx(), tree_.slot(), output.points.data(), (int)output.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(),
                             1e18f, idx.data(), d2.data()));
        double sum = 0; size_t nr = 0;
        for (size_t i = 0; i < d2.size(); ++i) if (idx[i] >= 0) { sum += d2[i]; ++nr; }
        fitness_ = nr ? sum / (double)nr : 1.7976931348623157e308;
    }
    bool hasConverged() const { return res_.converged != 0; }
    double getFitnessScore() const { return fitness_; }
    double getTransformationProbability() const { return res_.trans_probability; }
    const float* getFinalTransformation() const { return res_.final_transform; }     // row-major 4x4
    int getFinalNumIteration() const { return res_.iters; }
    const lisreg_ndt_info& info() const { return info_; }
    const lisreg_ndt_result& result() const { return res_; }
private:
    void check(int rc) { if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(tree_.ctx())); }
    SearchTree<PointT> tree_;
    int ndt_slot_;
    const PointCloud<PointT>* target_ = nullptr;
    const PointCloud<PointT>* source_ = nullptr;
    lisreg_ndt_params prm_{};
    lisreg_ndt_info   info_{};
    lisreg_ndt_result res_{};
    double fitness_ = 1.7976931348623157e308;
};

// ---- fast_gicp::FastVGICP as select_registration_method("FAST_VGICP") would set it up ----------------------------------
// (src/core/registration.cpp:156-187 and subMapOptmizationNode.cpp:2771, both commented out in the reference: the library would not
// link), with the pcl::Registration surface the loop-closure code uses.  vgicp_slot: the VGICP target slot; map_slot: a map-index slot
// of the same target for getFitnessScore (mean squared k = 1 distance of the aligned source, unbounded like PCL's default) — a single
// VGICP alignment has no fitness score; VgicpVerifier below (§7n) gets one per candidate from the batch call, without the second slot.
template <class PointT>
class VgicpRegistration {
public:
    VgicpRegistration(lisreg_ctx* ctx, int vgicp_slot, int map_slot) : tree_(ctx, map_slot), vgicp_slot_(vgicp_slot) { lisreg_vgicp_default_params(0, &prm_); }
    void setResolution(double r) { prm_.resolution = r; if (target_) setInputTarget(*target_); }
    void setCorrespondenceRandomness(int k) { prm_.k_correspondences = k; if (target_) setInputTarget(*target_); }
    void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
    void setRotationEpsilon(double e) { prm_.rotation_epsilon = e; }
    void setMaximumIterations(int n) { prm_.max_iters = n; }
    // fast_gicp's setNeighborSearchMethod (§7w): LISREG_VGICP_DIRECT1 / 7 / 27; of the alignment, so the target is not built again
    void setNeighborSearchMethod(int mode) { prm_.reserved = mode; }
    void setInputTarget(const PointCloud<PointT>& cloud) {
        target_ = &cloud;
        check(lisreg_vgicp_set_target(tree_.ctx(), vgicp_slot_, cloud.points.data(), (int)cloud.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(), &prm_, &info_));
        tree_.setInputCloud(cloud);
    }
    void setInputSource(const PointCloud<PointT>* cloud) { source_ = cloud; }
    void align(PointCloud<PointT>& output, const float* guess = nullptr) {
        if (!source_) throw RegistrationError(LISREG_ERR_ARG, "VGICP: no input source");
        output.points.resize(source_->size());
        check(lisreg_vgicp_align(tree_.ctx(), vgicp_slot_, source_->points.data(), (int)source_->size(), (int)sizeof(PointT),
                                 SearchTree<PointT>::fmt(), &prm_, guess, &res_, output.points.data()));
        for (int k = 0; k < 16; ++k) final_[k] = (float)res_.final_transform[k];
        std::vector<int> idx(output.size());
        std::vector<float> d2(output.size());
        check(lisreg_nearest(tree_.ctx(), tree_.slot(), output.points.data(), (int)output.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(),
                             1e18f, idx.data(), d2.data()));
        double sum = 0; size_t nr = 0;
        for (size_t i = 0; i < d2.size(); ++i) if (idx[i] >= 0) { sum += d2[i]; ++nr; }
        fitness_ = nr ? sum / (double)nr : 1.7976931348623157e308;
    }
    bool hasConverged() const { return res_.converged != 0; }
    double getFitnessScore() const { return fitness_; }
    const float* getFinalTransformation() const { return final_; }                  // row-major 4x4 (result().final_transform holds it in double)
    int getFinalNumIteration() const { return res_.iters; }
    const lisreg_vgicp_info& info() const { return info_; }
    const lisreg_vgicp_result& result() const { return res_; }
private:
    void check(int rc) { if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(tree_.ctx())); }
    SearchTree<PointT> tree_;
    int vgicp_slot_;
    const PointCloud<PointT>* target_ = nullptr;
    const PointCloud<PointT>* source_ = nullptr;
    lisreg_vgicp_params prm_{};
    lisreg_vgicp_info   info_{};
    lisreg_vgicp_result res_{};
    float  final_[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    double fitness_ = 1.7976931348623157e308;
};

// ---- fast_gicp::FastGICP as select_registration_method("FAST_GICP") sets it up -------------------------------------------
// (src/core/registration.cpp:157-166, commented out in the reference like the rest of the fast_gicp family), with the pcl::Registration
// surface the loop-closure code uses.  fgicp_slot: the FastGICP target slot; map_slot: a map-index slot of the same target for
// getFitnessScore (mean squared k = 1 distance of the aligned source, unbounded like PCL's default) — FastGICP itself has no fitness score.
template <class PointT>
class FastGicpRegistration {
public:
    FastGicpRegistration(lisreg_ctx* ctx, int fgicp_slot, int map_slot) : tree_(ctx, map_slot), fgicp_slot_(fgicp_slot) { lisreg_fgicp_default_params(0, &prm_); }
    void setMaxCorrespondenceDistance(double d) { prm_.max_correspondence_distance = d; }
    void setCorrespondenceRandomness(int k) { prm_.k_correspondences = k; if (target_) setInputTarget(*target_); }
    void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
    void setRotationEpsilon(double e) { prm_.rotation_epsilon = e; }
    void setMaximumIterations(int n) { prm_.max_iters = n; }
    void setInputTarget(const PointCloud<PointT>& cloud) {
        target_ = &cloud;
        check(lisreg_fgicp_set_target(tree_.ctx(), fgicp_slot_, cloud.points.data(), (int)cloud.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(), &prm_, &info_, 0.f));
        tree_.setInputCloud(cloud);
    }
    void setInputSource(const PointCloud<PointT>* cloud) { source_ = cloud; }
    void align(PointCloud<PointT>& output, const float* guess = nullptr) {
        if (!source_) throw RegistrationError(LISREG_ERR_ARG, "FastGICP: no input source");
        output.points.resize(source_->size());
        check(lisreg_fgicp_align(tree_.ctx(), fgicp_slot_, source_->points.data(), (int)source_->size(), (int)sizeof(PointT),
                                 SearchTree<PointT>::fmt(), &prm_, guess, &res_, output.points.data()));
        for (int k = 0; k < 16; ++k) final_[k] = (float)res_.final_transform[k];
        std::vector<int> idx(output.size());
        std::vector<float> d2(output.size());
        check(lisreg_nearest(tree_.ctx(), tree_.slot(), output.points.data(), (int)output.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(),
                             1e18f, idx.data(), d2.data()));
        double sum = 0; size_t nr = 0;
        for (size_t i = 0; i < d2.size(); ++i) if (idx[i] >= 0) { sum += d2[i]; ++nr; }
        fitness_ = nr ? sum / (double)nr : 1.7976931348623157e308;
    }
    bool hasConverged() const { return res_.converged != 0; }
    double getFitnessScore() const { return fitness_; }
    const float* getFinalTransformation() const { return final_; }                  // row-major 4x4 (result().final_transform holds it in double)
    int getFinalNumIteration() const { return res_.iters; }
    const lisreg_fgicp_info& info() const { return info_; }
    const lisreg_fgicp_result& result() const { return res_; }
private:
    void check(int rc) { if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(tree_.ctx())); }
    SearchTree<PointT> tree_;
    int fgicp_slot_;
    const PointCloud<PointT>* target_ = nullptr;
    const PointCloud<PointT>* source_ = nullptr;
    lisreg_fgicp_params prm_{};
    lisreg_fgicp_info   info_{};
    lisreg_fgicp_result res_{};
    float  final_[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    double fitness_ = 1.7976931348623157e308;
};

// ---- pcl::GeneralizedIterativeClosestPoint as select_registration_method("GICP") sets it up -----------------------------
// (src/core/registration.cpp:137-146: max correspondence distance 10, 30 iterations, transformation epsilon 1e-6, Euclidean fitness
// epsilon 1e-3, RANSAC 0 — the one verifier of the five that is NOT commented out there), with the pcl::Registration surface the
// loop-closure code uses.  The target lives in a FastGICP slot (a GICP target is a FastGICP target); map_slot: a map-index slot of the
// same target for getFitnessScore, as FastGicpRegistration's.  setEuclideanFitnessEpsilon and setRANSACIterations are kept and unused:
// PCL's GICP reads neither in its loop.
template <class PointT>
class GicpRegistration {
public:
    GicpRegistration(lisreg_ctx* ctx, int fgicp_slot, int map_slot) : tree_(ctx, map_slot), fgicp_slot_(fgicp_slot) { lisreg_gicp_default_params(0, &prm_); }
    void setMaxCorrespondenceDistance(double d) { prm_.max_correspondence_distance = d; }
    void setMaximumIterations(int n) { prm_.max_iters = n; }
    void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
    void setRotationEpsilon(double e) { prm_.rotation_epsilon = e; }
    void setEuclideanFitnessEpsilon(double e) { euclidean_fitness_epsilon_ = e; }
    void setRANSACIterations(int n) { ransac_iterations_ = n; }
    void setCorrespondenceRandomness(int k) { prm_.k_correspondences = k; if (target_) setInputTarget(*target_); }
    void setMaximumOptimizerIterations(int n) { prm_.max_inner_iters = n; }
    void setInputTarget(const PointCloud<PointT>& cloud) {
        target_ = &cloud;
        lisreg_fgicp_params tp;
        lisreg_fgicp_default_params(0, &tp);
        tp.max_correspondence_distance = prm_.max_correspondence_distance;
        tp.k_correspondences = prm_.k_correspondences;
        tp.plane_epsilon = prm_.gicp_epsilon;
        check(lisreg_fgicp_set_target(tree_.ctx(), fgicp_slot_, cloud.points.data(), (int)cloud.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(), &tp, &info_, 0.f));
        tree_.setInputCloud(cloud);
    }
    void setInputSource(const PointCloud<PointT>* cloud) { source_ = cloud; }
    void align(PointCloud<PointT>& output, const float* guess = nullptr) {
        if (!source_) throw RegistrationError(LISREG_ERR_ARG, "GICP: no input source");
        output.points.resize(source_->size());
        check(lisreg_gicp_align(tree_.ctx(), fgicp_slot_, source_->points.data(), (int)source_->size(), (int)sizeof(PointT),
                                SearchTree<PointT>::fmt(), &prm_, guess, &res_, output.points.data()));
        for (int k = 0; k < 16; ++k) final_[k] = (float)res_.final_transform[k];
        std::vector<int> idx(output.size());
        std::vector<float> d2(output.size());
        check(lisreg_nearest(tree_.ctx(), tree_.slot(), output.points.data(), (int)output.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(),
                             1e18f, idx.data(), d2.data()));
        double sum = 0; size_t nr = 0;
        for (size_t i = 0; i < d2.size(); ++i) if (idx[i] >= 0) { sum += d2[i]; ++nr; }
        fitness_ = nr ? sum / (double)nr : 1.7976931348623157e308;
    }
    bool hasConverged() const { return res_.converged != 0; }
    double getFitnessScore() const { return fitness_; }
    const float* getFinalTransformation() const { return final_; }                  // row-major 4x4 (result().final_transform holds it in double)
    int getFinalNumIteration() const { return res_.iters; }
    const lisreg_fgicp_info& info() const { return info_; }
    const lisreg_gicp_result& result() const { return res_; }
    const lisreg_gicp_params& params() const { return prm_; }
private:
    void check(int rc) { if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(tree_.ctx())); }
    SearchTree<PointT> tree_;
    int fgicp_slot_;
    const PointCloud<PointT>* target_ = nullptr;
    const PointCloud<PointT>* source_ = nullptr;
    lisreg_gicp_params prm_{};
    lisreg_fgicp_info  info_{};
    lisreg_gicp_result res_{};
    double euclidean_fitness_epsilon_ = 0.0;
    int    ransac_iterations_ = 0;
    float  final_[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    double fitness_ = 1.7976931348623157e308;
};

// ---- the candidate loop of detectLoopClosureForSubMap (src/node/subMapOptmizationNode.cpp:2779-2846) as one call ------
// Every candidate submap is a FastGICP slot with its initial pose; alignAll(source) aligns the key-frame cloud against all of them
// (lisreg_fgicp_align_batch: the source's distributions once, the LM loops in lockstep rounds) and best() is the candidate the loop's
// `hasConverged() == false || score > bestScore` test would have kept (-1: none), with result(i) / fitness(i) per candidate.
template <class PointT>
class FastGicpVerifier {
public:
    explicit FastGicpVerifier(lisreg_ctx* ctx) : ctx_(ctx) { lisreg_fgicp_default_params(0, &prm_); }
    void setMaxCorrespondenceDistance(double d) { prm_.max_correspondence_distance = d; }
    void setCorrespondenceRandomness(int k) { prm_.k_correspondences = k; }
    void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
    void setRotationEpsilon(double e) { prm_.rotation_epsilon = e; }
    void setMaximumIterations(int n) { prm_.max_iters = n; }
    const lisreg_fgicp_params& params() const { return prm_; }
    // the submap of a candidate into its slot (a submap that stays resident between key frames is set once)
    void setCandidateTarget(int slot, const PointCloud<PointT>& cloud) {
        check(lisreg_fgicp_set_target(ctx_, slot, cloud.points.data(), (int)cloud.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(), &prm_, nullptr, 0.f));
    }
    void clearCandidates() { slots_.clear(); guesses_.clear(); }
    // guess: row-major 4x4 (key2PreSubMapTrans), nullptr = identity; returns the candidate's index
    int addCandidate(int slot, const float* guess = nullptr) {
        slots_.push_back(slot);
        std::vector<float> g;
        if (guess) g.assign(guess, guess + 16);
        guesses_.push_back(g);
        return (int)slots_.size() - 1;
    }
    size_t size() const { return slots_.size(); }
    void alignAll(const PointCloud<PointT>& source) {
        const size_t n = slots_.size();
        std::vector<lisreg_fgicp_item> items(n);
        for (size_t i = 0; i < n; ++i) items[i] = lisreg_fgicp_item{ 0, slots_[i], guesses_[i].empty() ? nullptr : guesses_[i].data() };
        res_.assign(n, lisreg_fgicp_result{});
        fit_.assign(n, 1.7976931348623157e308);
        const void* src = source.points.data();
        const int ns = (int)source.size();
        check(lisreg_fgicp_align_batch(ctx_, &src, &ns, 1, (int)sizeof(PointT), SearchTree<PointT>::fmt(), items.data(), (int)n, &prm_,
                                       res_.data(), fit_.data(), &info_));
    }
    int best() const { return info_.best; }
    bool hasConverged(int i) const { return res_.at((size_t)i).converged != 0; }
    double fitness(int i) const { return fit_.at((size_t)i); }
    const lisreg_fgicp_result& result(int i) const { return res_.at((size_t)i); }
    const lisreg_fgicp_batch_info& info() const { return info_; }
private:
    void check(int rc) { if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_)); }
    lisreg_ctx* ctx_;
    lisreg_fgicp_params prm_{};
    std::vector<int> slots_;
    std::vector<std::vector<float>> guesses_;
    std::vector<lisreg_fgicp_result> res_;
    std::vector<double> fit_;
    lisreg_fgicp_batch_info info_{ -1, 0, 0, 0 };
};

// ---- the same candidate loop with the verifier of subMapOptmizationNode.cpp:2771 (FAST_VGICP) ---------------------------
// Every candidate submap is a VGICP slot with its initial pose; alignAll(source) aligns the key-frame cloud against all of them
// (lisreg_vgicp_align_batch: the source's distributions once, the LM loops in lockstep rounds, the fitness scores from the search grid
// the slot keeps) and best() is the candidate the loop's `hasConverged() == false || score > bestScore` test would have kept (-1: none),
// with result(i) / fitness(i) per candidate.  All candidate targets share the resolution: set it before the targets.
template <class PointT>
class VgicpVerifier {
public:
    explicit VgicpVerifier(lisreg_ctx* ctx) : ctx_(ctx) { lisreg_vgicp_default_params(0, &prm_); }
    void setResolution(double r) { prm_.resolution = r; }
    void setCorrespondenceRandomness(int k) { prm_.k_correspondences = k; }
    void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
    void setRotationEpsilon(double e) { prm_.rotation_epsilon = e; }
    void setMaximumIterations(int n) { prm_.max_iters = n; }
    // fast_gicp's setNeighborSearchMethod (§7w): LISREG_VGICP_DIRECT1 / 7 / 27, one for all candidates of a batch
    void setNeighborSearchMethod(int mode) { prm_.reserved = mode; }
    const lisreg_vgicp_params& params() const { return prm_; }
    // the submap of a candidate into its slot (a submap that stays resident between key frames is set once)
    void setCandidateTarget(int slot, const PointCloud<PointT>& cloud) {
        check(lisreg_vgicp_set_target(ctx_, slot, cloud.points.data(), (int)cloud.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(), &prm_, nullptr));
    }
    void clearCandidates() { slots_.clear(); guesses_.clear(); }
    // guess: row-major 4x4 (key2PreSubMapTrans), nullptr = identity; returns the candidate's index
    int addCandidate(int slot, const float* guess = nullptr) {
        slots_.push_back(slot);
        std::vector<float> g;
        if (guess) g.assign(guess, guess + 16);
        guesses_.push_back(g);
        return (int)slots_.size() - 1;
    }
    size_t size() const { return slots_.size(); }
    void alignAll(const PointCloud<PointT>& source) {
        const size_t n = slots_.size();
        std::vector<lisreg_vgicp_item> items(n);
        for (size_t i = 0; i < n; ++i) items[i] = lisreg_vgicp_item{ 0, slots_[i], guesses_[i].empty() ? nullptr : guesses_[i].data() };
        res_.assign(n, lisreg_vgicp_result{});
        fit_.assign(n, 1.7976931348623157e308);
        const void* src = source.points.data();
        const int ns = (int)source.size();
        check(lisreg_vgicp_align_batch(ctx_, &src, &ns, 1, (int)sizeof(PointT), SearchTree<PointT>::fmt(), items.data(), (int)n, &prm_,
                                       res_.data(), fit_.data(), &info_));
    }
    int best() const { return info_.best; }
    bool hasConverged(int i) const { return res_.at((size_t)i).converged != 0; }
    double fitness(int i) const { return fit_.at((size_t)i); }
    const lisreg_vgicp_result& result(int i) const { return res_.at((size_t)i); }
    const lisreg_vgicp_batch_info& info() const { return info_; }
private:
    void check(int rc) { if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_)); }
    lisreg_ctx* ctx_;
    lisreg_vgicp_params prm_{};
    std::vector<int> slots_;
    std::vector<std::vector<float>> guesses_;
    std::vector<lisreg_vgicp_result> res_;
    std::vector<double> fit_;
    lisreg_vgicp_batch_info info_{ -1, 0, 0, 0 };
};

// ---- the same candidate loop with the verifier the reference names first (NDT, registration.cpp:147-155) ----------------
// Every candidate submap is an NDT slot with its initial pose; alignAll(source) aligns the key-frame cloud against all of them
// (lisreg_ndt_align_batch: the source uploaded once, the Newton loops with their line searches in lockstep rounds, the fitness scores
// from the search grid the slot keeps) and best() is the candidate the loop's `hasConverged() == false || score > bestScore` test would
// have kept (-1: none), with result(i) / fitness(i) per candidate.  All candidate targets share the resolution: set it before the targets.
template <class PointT>
class NdtVerifier {
public:
    explicit NdtVerifier(lisreg_ctx* ctx) : ctx_(ctx) { lisreg_ndt_default_params(0, &prm_); }
    void setResolution(double r) { prm_.resolution = r; }
    void setStepSize(double s) { prm_.step_size = s; }
    void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
    void setMaximumIterations(int n) { prm_.max_iters = n; }
    void setLineSearch(bool more_thuente) { prm_.line_search = more_thuente ? 1 : 0; }
    const lisreg_ndt_params& params() const { return prm_; }
    // the submap of a candidate into its slot (a submap that stays resident between key frames is set once)
    void setCandidateTarget(int slot, const PointCloud<PointT>& cloud) {
        check(lisreg_ndt_set_target(ctx_, slot, cloud.points.data(), (int)cloud.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(), &prm_, nullptr));
    }
    void clearCandidates() { slots_.clear(); guesses_.clear(); }
    // guess: row-major 4x4 (key2PreSubMapTrans), nullptr = identity; returns the candidate's index
    int addCandidate(int slot, const float* guess = nullptr) {
        slots_.push_back(slot);
        std::vector<float> g;
        if (guess) g.assign(guess, guess + 16);
        guesses_.push_back(g);
        return (int)slots_.size() - 1;
    }
    size_t size() const { return slots_.size(); }
    void alignAll(const PointCloud<PointT>& source) {
        const size_t n = slots_.size();
        std::vector<lisreg_ndt_item> items(n);
        for (size_t i = 0; i < n; ++i) items[i] = lisreg_ndt_item{ 0, slots_[i], guesses_[i].empty() ? nullptr : guesses_[i].data() };
        res_.assign(n, lisreg_ndt_result{});
        fit_.assign(n, 1.7976931348623157e308);
        const void* src = source.points.data();
        const int ns = (int)source.size();
        check(lisreg_ndt_align_batch(ctx_, &src, &ns, 1, (int)sizeof(PointT), SearchTree<PointT>::fmt(), items.data(), (int)n, &prm_,
                                     res_.data(), fit_.data(), &info_));
    }
    int best() const { return info_.best; }
    bool hasConverged(int i) const { return res_.at((size_t)i).converged != 0; }
    double fitness(int i) const { return fit_.at((size_t)i); }
    const lisreg_ndt_result& result(int i) const { return res_.at((size_t)i); }
    const lisreg_ndt_batch_info& info() const { return info_; }
private:
    void check(int rc) { if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_)); }
    lisreg_ctx* ctx_;
    lisreg_ndt_params prm_{};
    std::vector<int> slots_;
    std::vector<std::vector<float>> guesses_;
    std::vector<lisreg_ndt_result> res_;
    std::vector<double> fit_;
    lisreg_ndt_batch_info info_{ -1, 0, 0, 0 };
};

// ---- the same candidate loop with the one verifier whose block is live (GICP, registration.cpp:137-146) --------------------
// Every candidate submap is a FastGICP slot (a GICP target is a FastGICP target, set with plane_epsilon = gicp_epsilon) with its initial
// pose; alignAll(source) aligns the key-frame cloud against all of them (lisreg_gicp_align_batch: the source's distributions once, the
// outer loops in lockstep rounds of one moments launch each, the inner BFGS on the host) and best() is the candidate the loop's
// `hasConverged() == false || score > bestScore` test would have kept (-1: none), with result(i) / fitness(i) per candidate.
template <class PointT>
class GicpVerifier {
public:
    explicit GicpVerifier(lisreg_ctx* ctx) : ctx_(ctx) { lisreg_gicp_default_params(0, &prm_); }
    void setMaxCorrespondenceDistance(double d) { prm_.max_correspondence_distance = d; }
    void setCorrespondenceRandomness(int k) { prm_.k_correspondences = k; }
    void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
    void setRotationEpsilon(double e) { prm_.rotation_epsilon = e; }
    void setMaximumIterations(int n) { prm_.max_iters = n; }
    void setMaximumOptimizerIterations(int n) { prm_.max_inner_iters = n; }
    const lisreg_gicp_params& params() const { return prm_; }
    // the submap of a candidate into its slot (a submap that stays resident between key frames is set once)
    void setCandidateTarget(int slot, const PointCloud<PointT>& cloud) {
        lisreg_fgicp_params tp;
        lisreg_fgicp_default_params(0, &tp);
        tp.max_correspondence_distance = prm_.max_correspondence_distance;
        tp.k_correspondences = prm_.k_correspondences;
        tp.plane_epsilon = prm_.gicp_epsilon;
        check(lisreg_fgicp_set_target(ctx_, slot, cloud.points.data(), (int)cloud.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt(), &tp, nullptr, 0.f));
    }
    void clearCandidates() { slots_.clear(); guesses_.clear(); }
    // guess: row-major 4x4 (key2PreSubMapTrans), nullptr = identity; returns the candidate's index
    int addCandidate(int slot, const float* guess = nullptr) {
        slots_.push_back(slot);
        std::vector<float> g;
        if (guess) g.assign(guess, guess + 16);
        guesses_.push_back(g);
        return (int)slots_.size() - 1;
    }
    size_t size() const { return slots_.size(); }
    void alignAll(const PointCloud<PointT>& source) {
        const size_t n = slots_.size();
        std::vector<lisreg_gicp_item> items(n);
        for (size_t i = 0; i < n; ++i) items[i] = lisreg_gicp_item{ 0, slots_[i], guesses_[i].empty() ? nullptr : guesses_[i].data() };
        res_.assign(n, lisreg_gicp_result{});
        fit_.assign(n, 1.7976931348623157e308);
        const void* src = source.points.data();
        const int ns = (int)source.size();
        check(lisreg_gicp_align_batch(ctx_, &src, &ns, 1, (int)sizeof(PointT), SearchTree<PointT>::fmt(), items.data(), (int)n, &prm_,
                                      res_.data(), fit_.data(), &info_));
    }
    int best() const { return info_.best; }
    bool hasConverged(int i) const { return res_.at((size_t)i).converged != 0; }
    double fitness(int i) const { return fit_.at((size_t)i); }
    const lisreg_gicp_result& result(int i) const { return res_.at((size_t)i); }
    const lisreg_gicp_batch_info& info() const { return info_; }
private:
    void check(int rc) { if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_)); }
    lisreg_ctx* ctx_;
    lisreg_gicp_params prm_{};
    std::vector<int> slots_;
    std::vector<std::vector<float>> guesses_;
    std::vector<lisreg_gicp_result> res_;
    std::vector<double> fit_;
    lisreg_gicp_batch_info info_{ -1, 0, 0, 0 };
};

// OptimizedICPGN (src/include/registration.h:44-70, src/core/registration.cpp:8-115): same constructor and calls
template <class PointT>
class OptimizedICPGN {
public:
    OptimizedICPGN(lisreg_ctx* ctx, int slot, unsigned max_iterations, float max_correspond_distance)
        : tree_(ctx, slot), max_iterations_(max_iterations), max_correspond_distance_(max_correspond_distance) {}
    bool SetTargetCloud(const PointCloud<PointT>& target_cloud) { tree_.setInputCloud(target_cloud); return true; }
    bool Match(const PointCloud<PointT>& source_cloud, const float predict_pose[16], PointCloud<PointT>& transformed_source_cloud, float result_pose[16]) {
        transformed_source_cloud.points.resize(source_cloud.size());
        int rc = lisreg_icp_gn_match(tree_.ctx(), tree_.slot(), source_cloud.points.data(), (int)source_cloud.size(), (int)sizeof(PointT),
                                     SearchTree<PointT>::fmt(), max_iterations_, max_correspond_distance_, predict_pose, &res_,
                                     transformed_source_cloud.points.data());
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(tree_.ctx()));
        std::memcpy(result_pose, res_.final_transform, sizeof res_.final_transform);
        return true;
    }
    float GetFitnessScore() const { return res_.fitness; }
    bool HasConverged() const { return true; }                      // registration.cpp:110-113
private:
    SearchTree<PointT> tree_;
    unsigned max_iterations_;
    float max_correspond_distance_;
    lisreg_icpgn_result res_{};
};

// ---- the candidate loop of detectLoopClosureForSubMapICP (src/node/subMapOptmizationNode.cpp:2496-2621) as one call -------
// `static OptimizedICPGN myICP(30, 10)` and, per candidate, SetTargetCloud / Match / GetFitnessScore / HasConverged.  Every candidate
// submap is a map-index slot with its predict_pose (the caller composes the loop's correctionKey2PreSubMap carry into it); matchAll(source)
// matches the key-frame cloud against all of them (lisreg_icp_gn_match_batch: the source staged once, every iteration one launch
// sequence over all candidates) and best() is the candidate the loop's `score > bestScore` test keeps (-1: none), with result(i) /
// fitness(i) per candidate — what an OptimizedICPGN gives each of them alone, byte for byte.
template <class PointT>
class IcpGnVerifier {
public:
    explicit IcpGnVerifier(lisreg_ctx* ctx, unsigned max_iterations = 30, float max_correspond_distance = 10.f)
        : ctx_(ctx), max_iterations_(max_iterations), max_correspond_distance_(max_correspond_distance) {}
    // the submap of a candidate into its slot (a submap that stays resident between key frames is set once)
    void setCandidateTarget(int slot, const PointCloud<PointT>& cloud) {
        check(lisreg_map_index_set(ctx_, slot, cloud.points.data(), (int)cloud.size(), (int)sizeof(PointT), SearchTree<PointT>::fmt()));
    }
    void clearCandidates() { slots_.clear(); poses_.clear(); }
    // predict_pose: row-major 4x4, nullptr = identity; returns the candidate's index
    int addCandidate(int slot, const float* predict_pose = nullptr) {
        slots_.push_back(slot);
        std::vector<float> g;
        if (predict_pose) g.assign(predict_pose, predict_pose + 16);
        poses_.push_back(g);
        return (int)slots_.size() - 1;
    }
    size_t size() const { return slots_.size(); }
    void matchAll(const PointCloud<PointT>& source) {
        const size_t n = slots_.size();
        std::vector<lisreg_icpgn_item> items(n);
        for (size_t i = 0; i < n; ++i) items[i] = lisreg_icpgn_item{ 0, slots_[i], poses_[i].empty() ? nullptr : poses_[i].data() };
        res_.assign(n, lisreg_icpgn_result{});
        info_ = lisreg_icpgn_batch_info{ -1, 0, 0, 0 };
        const void* src = source.points.data();
        const int ns = (int)source.size();
        check(lisreg_icp_gn_match_batch(ctx_, &src, &ns, 1, (int)sizeof(PointT), SearchTree<PointT>::fmt(), items.data(), (int)n,
                                        max_iterations_, max_correspond_distance_, res_.data(), &info_));
    }
    int best() const { return info_.best; }
    bool hasConverged(int) const { return true; }                   // registration.cpp:110-113
    float fitness(int i) const { return res_.at((size_t)i).fitness; }
    const lisreg_icpgn_result& result(int i) const { return res_.at((size_t)i); }
    const lisreg_icpgn_batch_info& info() const { return info_; }
private:
    void check(int rc) { if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_)); }
    lisreg_ctx* ctx_;
    unsigned max_iterations_;
    float max_correspond_distance_;
    std::vector<int> slots_;
    std::vector<std::vector<float>> poses_;
    std::vector<lisreg_icpgn_result> res_;
    lisreg_icpgn_batch_info info_{ -1, 0, 0, 0 };
};

// ---- SURVEY.md §8 f-3 composite: the sliding local map kept in HBM -------------------------------------------------------
// localMap_t + SubMapManager::insert_local_map (src/include/subMap.h:979-1059) + SubMapOptmizationNode::extractSlidingCloud
// (src/node/subMapOptmizationNode.cpp:1369-1432).  Class order of the arrays: dynamic, pole, ground, building, outlier
// (append_feature, subMap.h:742-753).  The makeSubMapThread loop (:597-755) becomes
//     localMap.extractSlidingCloud(transformTobeSubMapped);  reg.scan2SubMapOptimization(...);  localMap.insert_local_map(cls, pose);
template <class PointT = PointXYZIL>
class LocalMap {
public:
    lisreg_localmap_params params;          // local_map_radius etc. of makeSubMapThread (:603-612) that the path actually reads
    LocalMap(lisreg_ctx* ctx, int map_id = 0) : ctx_(ctx), id_(map_id) {
        lisreg_localmap_default_params(&params);
        int rc = lisreg_localmap_reset(ctx_, id_);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
    }
    // this->insert_local_map(localMap, currentKeyFrame, ...): the key frame's un-downsampled class clouds + its optimized_pose
    lisreg_localmap_info insert_local_map(const PointCloud<PointT> cls[5], const float optimized_pose[6]) {
        const void* ptr[5]; int n[5];
        for (int k = 0; k < 5; ++k) { ptr[k] = cls[k].points.data(); n[k] = (int)cls[k].size(); }
        lisreg_localmap_info info{};
        int rc = lisreg_localmap_insert(ctx_, id_, ptr, n, (int)sizeof(PointT), fmt(), optimized_pose, &params, &info);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
        return info;
    }
    // extractSlidingCloud(currentKeyFrame, cur_pose) + both kd-tree setInputCloud calls: the target lands in `target_slot`
    lisreg_localmap_info extractSlidingCloud(const float cur_pose[6], int target_slot = 0) {
        lisreg_localmap_info info{};
        int rc = lisreg_localmap_extract(ctx_, id_, cur_pose, &params, target_slot, &info);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
        return info;
    }
private:
    static constexpr int fmt() { return std::is_same<PointT, PointXYZIL>::value ? LISREG_FMT_XYZIL : LISREG_FMT_XYZI; }
    lisreg_ctx* ctx_;
    int id_;
};

// Copy #3's side: submap_t + SubMapManager::fisrt_submap / insert_submap (src/include/subMap.h:785-978) and
// SubMapOptmizationNode::extractSubMapCloud (src/node/subMapOptmizationNode.cpp:3976-4081), kept in HBM.  subMapOptmizationThread becomes
//     cur.fisrt_submap(down, pose); cur.insert_submap(down, relative_pose) ...;
//     auto x = SubMap<>::extractSubMapCloud(ctx, pre, cur, transformTobeMapped);          // target installed, sources as device records
//     reg.subMap2SubMapOptimization(x, cloudInfo);                                        // copy #3 on the device records
template <class PointT = PointXYZIL>
class SubMap {
public:
    lisreg_localmap_params params;          // max_num_pts, map_based_dynamic_removal_on, ... of makeSubMapThread (:603-612)
    float submap_pose_6D_optimized[6] = { 0, 0, 0, 0, 0, 0 };
    lisreg_submap_info info{};
    SubMap(lisreg_ctx* ctx, int map_id) : ctx_(ctx), id_(map_id) {
        lisreg_localmap_default_params(&params);
        int rc = lisreg_localmap_reset(ctx_, id_);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
    }
    int id() const { return id_; }
    // this->fisrt_submap(currentSubMap, currentKeyFrame): the key frame's *_down class clouds as they are; the submap takes its optimized_pose
    void fisrt_submap(const PointCloud<PointT> down[5], const float optimized_pose[6]) {
        for (int k = 0; k < 6; ++k) submap_pose_6D_optimized[k] = optimized_pose[k];
        insert(down, nullptr);
    }
    // this->insert_submap(currentSubMap, currentKeyFrame, ...): the *_down clouds moved by the frame's relative_pose, all five classes
    void insert_submap(const PointCloud<PointT> down[5], const float relative_pose[6]) { insert(down, relative_pose); }
    // extractSubMapCloud() for (preSubMap, curSubMapPtr) under the guess transformTobeMapped; bbx pad 10 m, voxel grids 0.2 / 0.5
    static lisreg_submap_extract_out extractSubMapCloud(lisreg_ctx* ctx, const SubMap& pre, const SubMap& cur, const float transformTobeMapped[6],
                                                        int target_slot = 0) {
        lisreg_submap_extract_out out{};
        int rc = lisreg_submap_extract(ctx, pre.id_, cur.id_, pre.submap_pose_6D_optimized, transformTobeMapped, 10.0f, 0.2f, 0.5f, target_slot, &out);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx));
        return out;
    }
    // The chosen class clouds of this submap end to end (dynamic, pole, ground, building, outlier: LISREG_CLS_*), transformPointCloud'ed by
    // `pose` (nullptr: as they are, in the submap's own frame), as one host cloud out of one launch: the loop-verification target
    // (subMapOptmizationNode.cpp:2787-2790 = merged(15, nullptr, ..)), laserCloudFromPre (:1151-1154 = merged(LISREG_CLS_POLE,
    // submap_pose_6D_optimized, ..)).  The store keeps no intensity: it reads 0.
    void merged(unsigned class_mask, const float* pose, PointCloud<PointXYZIL>& out) const {
        lisreg_gather_params gp;
        lisreg_default_gather_params(&gp);
        gp.class_mask = class_mask; gp.out_fmt = LISREG_FMT_XYZIL;
        long long n = 0;
        int rc = lisreg_submap_gather_count(ctx_, 1, &id_, class_mask, &n, nullptr);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
        out.points.resize((size_t)n);
        rc = lisreg_submap_gather(ctx_, 1, &id_, pose, &gp, out.points.data(), n, &n, nullptr);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
    }
private:
    void insert(const PointCloud<PointT> down[5], const float* rel) {
        const void* ptr[5]; int n[5];
        for (int k = 0; k < 5; ++k) { ptr[k] = down[k].points.data(); n[k] = (int)down[k].size(); }
        int rc = lisreg_submap_insert(ctx_, id_, ptr, n, (int)sizeof(PointT), fmt(), rel, submap_pose_6D_optimized, &params, &info);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
    }
    static constexpr int fmt() { return std::is_same<PointT, PointXYZIL>::value ? LISREG_FMT_XYZIL : LISREG_FMT_XYZI; }
    lisreg_ctx* ctx_;
    int id_;
};

// publishGlobalMap() (subMapOptmizationNode.cpp:3553-3574) and, with finishMap = true, the map of the PCD export (:3502-3514): every submap
// of subMapInfo in id order — all but the newest unless finishMap (FINISHMAP, :3561-3562) — its five class clouds under its
// submap_pose_6D_optimized, concatenated.  One gather over the resident submaps, whatever their number; after a loop closure has moved
// the poses the same call rebuilds the whole map.
inline void publishGlobalMap(lisreg_ctx* ctx, const std::map<int, SubMap<>*>& subMapInfo, bool finishMap, PointCloud<PointXYZIL>& globalMapCloud) {
    std::vector<int> ids;
    std::vector<float> poses;
    for (auto it = subMapInfo.begin(); it != subMapInfo.end(); ++it) {
        auto itEnd = subMapInfo.end(); --itEnd;
        if (!finishMap && it == itEnd) continue;
        ids.push_back(it->second->id());
        poses.insert(poses.end(), it->second->submap_pose_6D_optimized, it->second->submap_pose_6D_optimized + 6);
    }
    lisreg_gather_params gp;
    lisreg_default_gather_params(&gp);
    gp.out_fmt = LISREG_FMT_XYZIL;
    long long n = 0;
    int rc = lisreg_submap_gather_count(ctx, (int)ids.size(), ids.data(), gp.class_mask, &n, nullptr);
    if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx));
    globalMapCloud.points.resize((size_t)n);
    rc = lisreg_submap_gather(ctx, (int)ids.size(), ids.data(), poses.data(), &gp, globalMapCloud.points.data(), n, &n, nullptr);
    if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx));
}

// The odometry node's multi-frame target (odomEstimationNode.cpp, USING_MULTI_FRAME_TARGET), device-resident: replaces
// laserCloud{Corner,Surf}Vec + the concatenation loop + the two VoxelGrid filters of laserCloudInfoHandler (:185-207) and the
// transformPointCloud / push_back / erase of saveKeyFrames (:452-467).  The frame loop becomes
//     keyframes.extractTarget(mappingCornerLeafSize, mappingSurfLeafSize);  reg.scan2SubMapOptimization(...);
//     if (key frame) keyframes.saveKeyFrame(*laserCloudCornerLast, *laserCloudSurfLast, reg.transformTobeMapped);
template <class PointT = PointType>
class KeyframeTarget {
public:
    explicit KeyframeTarget(lisreg_ctx* ctx, int ring_id = 0, int max_keep = 19) : ctx_(ctx), id_(ring_id), keep_(max_keep) {
        int rc = lisreg_keyframes_reset(ctx_, id_);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
    }
    // saveKeyFrames(): the frame's FULL feature clouds (sensor frame) + thisPose6D
    int saveKeyFrame(const PointCloud<PointT>& cornerLast, const PointCloud<PointT>& surfLast, const float pose[6]) {
        lisreg_keyframes_info info{};
        int rc = lisreg_keyframes_push(ctx_, id_, cornerLast.points.data(), (int)cornerLast.size(), surfLast.points.data(), (int)surfLast.size(),
                                       (int)sizeof(PointT), fmt(), pose, keep_, &info);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
        return info.n_keyframes;
    }
    // laserCloud{Corner,Surf}FromMapDS + both kd-tree setInputCloud calls: the target lands in `target_slot`
    lisreg_keyframes_info extractTarget(float cornerLeaf, float surfLeaf, int target_slot = 0) {
        lisreg_keyframes_info info{};
        int rc = lisreg_keyframes_target(ctx_, id_, cornerLeaf, surfLeaf, target_slot, &info);
        if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_));
        return info;
    }
private:
    static constexpr int fmt() { return std::is_same<PointT, PointXYZIL>::value ? LISREG_FMT_XYZIL : LISREG_FMT_XYZI; }
    lisreg_ctx* ctx_;
    int id_, keep_;
};

// updateInitialGuess with neither IMU nor odometry (odomEstimationNode.cpp:351-392): constant-velocity pose guess
inline void updateInitialGuess(const float lastTransformTobeMapped[6], float transformTobeMapped[6]) {
    float g[6];
    lisreg_predict_pose(lastTransformTobeMapped, transformTobeMapped, g);
    for (int k = 0; k < 6; ++k) transformTobeMapped[k] = g[k];
}

// updateInitialGuess as a whole (odomEstimationNode.cpp:297-419 = NodeCopy::Odom; subMapOptmizationNode.cpp:896-1032 = NodeCopy::SubMap):
// the function-local statics of the reference are this object's state.  One instance per node; call once per sweep BEFORE
// scan2SubMapOptimization, exactly where the reference calls updateInitialGuess().
enum class NodeCopy { Odom = 0, SubMap = 1 };
class InitialGuess {
public:
    explicit InitialGuess(NodeCopy copy, bool useImuHeadingInitialization = false) : copy_(copy), heading_(useImuHeadingInitialization) {
        lisreg_guess_state_init(&st_);
    }
    // transformTobeMapped is updated in place; transPredictionMapped (may be null) where the reference assigns it
    void updateInitialGuess(const cloud_info& cloudInfo, float transformTobeMapped[6], float* transPredictionMapped = nullptr) {
        lisreg_guess_input in{ cloudInfo.odomAvailable ? 1 : 0, cloudInfo.imuAvailable ? 1 : 0,
                               cloudInfo.imuRollInit, cloudInfo.imuPitchInit, cloudInfo.imuYawInit,
                               cloudInfo.initialGuessX, cloudInfo.initialGuessY, cloudInfo.initialGuessZ,
                               cloudInfo.initialGuessRoll, cloudInfo.initialGuessPitch, cloudInfo.initialGuessYaw };
        lisreg_update_initial_guess((int)copy_, heading_ ? 1 : 0, &in, &st_, transformTobeMapped, transPredictionMapped);
    }
    const lisreg_guess_state& state() const { return st_; }
private:
    NodeCopy copy_; bool heading_; lisreg_guess_state st_;
};

// The candidate loop of detectLoopClosureForSubMap (subMapOptmizationNode.cpp:2776-2840) as one call: candidate k = (target slot set by
// IterativeClosestPoint::setInputTarget / lisreg_map_index_set, source cloud, guess).  chain = true reproduces the reference's `static`
// ICP object (correspondences_prev_mse_ carried from one align() to the next, :2763).
template <class PointT>
inline std::vector<lisreg_icp_result> alignLoopCandidates(lisreg_ctx* ctx, const std::vector<lisreg_icp_item>& candidates,
                                                          const lisreg_icp_params& params, bool chain = true) {
    std::vector<lisreg_icp_result> res(candidates.size());
    const int fmt = std::is_same<PointT, PointXYZIL>::value ? LISREG_FMT_XYZIL : LISREG_FMT_XYZI;
    const int rc = lisreg_icp_align_batch(ctx, candidates.data(), (int)candidates.size(), (int)sizeof(PointT), fmt, &params, chain ? 1 : 0, res.data());
    if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx));
    return res;
}

// EPSCGeneration (src/include/epscGeneration.h, src/core/epscGeneration.cpp:663-992): loopDetection per key frame with the selectors of a
// LISREG_LOOP_* mask (the Using*Flag rosparams; default UsingFEPSCFlag alone),
// the public current_frame_id / matched_frame_id / matched_frame_transform that loopClosureThread reads (subMapOptmizationNode.cpp:
// 2328-2362).  odom is the row-major 3 x 4 of pclPointToAffine3f(optimized_pose) (lisreg_pose_to_matrix); matched_frame_transform
// holds row-major 4 x 4 matrices (the EPSC init pose of detectLoopClosureForSubMap, :2796-2805).  The history lives in database
// db_id of the context, so several generators may share one context.
class EPSCGeneration {
public:
    explicit EPSCGeneration(lisreg_ctx* ctx, int db_id = 0, unsigned kinds = LISREG_LOOP_FEPSC,
                            double label_threshold = LISREG_LOOP_LABEL_THRESHOLD) : ctx_(ctx), db_(db_id)
    {
        check(lisreg_loopdet_reset(ctx_, db_));
        check(lisreg_loopdet_configure(ctx_, db_, kinds, label_threshold));
    }
    void loopDetection(const PointCloud<PointXYZI>& corner_pc, const PointCloud<PointXYZI>& surf_pc, const PointCloud<PointXYZIL>& semantic_pc,
                       const float odom[12]) {
        lisreg_loopdet_frame f;
        f.corner = corner_pc.points.data(); f.n_corner = (int)corner_pc.size();
        f.surf = surf_pc.points.data(); f.n_surf = (int)surf_pc.size();
        f.semantic = semantic_pc.points.data(); f.n_semantic = (int)semantic_pc.size();
        std::memcpy(f.odom, odom, sizeof f.odom);
        lisreg_loopdet_result r;
        check(lisreg_loopdet_detect(ctx_, db_, &f, 1, (int)sizeof(PointXYZIL), LISREG_FMT_XYZIL, nullptr, &r));
        current_frame_id = r.current_frame_id;
        matched_frame_id.clear();
        matched_frame_transform.clear();
        matched_kind.clear();
        lisreg_loopdet_match m[LISREG_LOOP_KINDS];
        int n = 0;
        check(lisreg_loopdet_matches(ctx_, db_, 0, m, LISREG_LOOP_KINDS, &n));
        for (int j = 0; j < n; ++j) {                     // ISC, SC, EPSC, SEPSC, FEPSC, SSC, POSE (:894-990)
            matched_frame_id.push_back(m[j].history_id);
            matched_frame_transform.emplace_back(m[j].transform, m[j].transform + 16);
            matched_kind.push_back((unsigned)m[j].kind);
        }
        if (r.matched_frame_id >= 0) last_score = r.score;
    }
    int current_frame_id = 0;
    std::vector<int> matched_frame_id;
    std::vector<std::vector<float>> matched_frame_transform;
    std::vector<unsigned> matched_kind;                   // the LISREG_LOOP_* selector of each entry
    double last_score = 0.0;                              // the last FEPSC match's score
private:
    void check(int rc) { if (rc != LISREG_OK) throw RegistrationError(rc, lisreg_last_error(ctx_)); }
    lisreg_ctx* ctx_;
    int db_;
};

}  // namespace lis_slam
