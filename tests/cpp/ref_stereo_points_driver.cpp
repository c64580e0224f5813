// tests/cpp/ref_stereo_points_driver.cpp — TEST INFRASTRUCTURE ONLY (compiled at test time by tests/test_stereo_points.py where the reference tree is
// present, with the flags of oracle/Makefile's libref_mappoint.so rule, and linked against that library; never committed as a binary).
//
// The checker of orbm_map_stereo_points.  No reference library exports the second half of Tracking::CreateNewKeyFrame (src/Tracking.cc:3868-3960) or
// the loop of Tracking::UpdateLastFrame (:3264-3341): Tracking.cc cannot be built here.  This driver RESTATES those two loops (the candidate list
// :3876-3887 / :3269-3280, std::sort :3892 / :3286, the visit with its bCreateNew test :3897-3911 / :3292-3305 and the stop :3954 / :3338) around the
// reference's OWN code, compiled in place into libref_mappoint.so:
//   Frame::SetPose / UpdatePoseMatrices (src/Frame.cc:533-540, :592-599), Frame::UnprojectStereo (:1396-1409),
//   mode 1: MapPoint(Pos, pMap, pFrame, idxF) (src/MapPoint.cc:90-128),
//   mode 0: MapPoint(Pos, pRefKF, pMap) (:45-62) + AddObservation (:175-201) + ComputeDistinctiveDescriptors (:438-529) + UpdateNormalAndDepth (:567-642).
// Results leave as raw bits.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>
#define protected public    // mfMinDistance / mfMaxDistance are read directly (access specifiers do not change the layout)
#include "MapPoint.h"       // the reference headers
#undef protected

using namespace ORB_SLAM3;

extern "C" {

// One frame.  holds[i]: 0 = mvpMapPoints[i] is NULL, 1 = a point with an observation (the feature keeps it), 2 = a point nobody observes (replaced, :3907).
// pose: Tcw as unit quaternion (w, x, y, z) and translation.  Out: Rwc [9] row-major and Ow [3] as UpdatePoseMatrices left them (the inputs the device
// call is given), processed = entries visited, feat [created], fields [created][8] = {pos 3, normal 3, mfMinDistance, mfMaxDistance} as bits,
// desc_out [created][32].  Returns created.
int ref_stereo_points(int N, const float* kx, const float* ky, const int* octave, const float* depth, const uint8_t* desc, int nlevels, const float* scale,
                      const float* cam, const float* q_wxyz, const float* t, const uint8_t* holds, float th_depth, int max_points, int mode, float* Rwc_out,
                      float* Ow_out, int* processed, int* feat, uint32_t* fields, uint8_t* desc_out) {
    Map map;
    Frame F;
    F.N = N; F.Nleft = -1; F.Nright = -1;
    F.mvKeysUn.resize(N); F.mvDepth.assign(depth, depth + N); F.mvuRight.assign(N, -1.0f);
    for (int i = 0; i < N; i++) { F.mvKeysUn[i].pt.x = kx[i]; F.mvKeysUn[i].pt.y = ky[i]; F.mvKeysUn[i].octave = octave[i]; }
    F.mvKeys = F.mvKeysUn;
    F.mDescriptors.create(N > 0 ? N : 1, 32, CV_8UC1);
    for (int i = 0; i < N; i++) memcpy(F.mDescriptors.ptr(i), desc + 32 * (size_t)i, 32);
    F.mnScaleLevels = nlevels; F.mvScaleFactors.assign(scale, scale + nlevels);
    Frame::cx = cam[0]; Frame::cy = cam[1]; Frame::invfx = cam[2]; Frame::invfy = cam[3];
    const Sophus::SE3f Tcw(Eigen::Quaternionf(q_wxyz[0], q_wxyz[1], q_wxyz[2], q_wxyz[3]), Eigen::Vector3f(t[0], t[1], t[2]));
    F.SetPose(Tcw);
    const Eigen::Matrix3f Rwc = F.GetRwc(); const Eigen::Vector3f Ow = F.GetOw();
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Rwc_out[3 * r + c] = Rwc(r, c);
    for (int k = 0; k < 3; k++) Ow_out[k] = Ow(k);

    // the key frame CreateNewKeyFrame has just made of the frame (mode 0), and one elsewhere that observes the points the frame keeps
    KeyFrame kf, other;
    kf.N = N; kf.mvKeysUn = F.mvKeysUn; kf.mvKeys = F.mvKeysUn; kf.mvuRight.assign(N > 0 ? N : 1, -1.0f); kf.mDescriptors = F.mDescriptors;
    kf.mnScaleLevels = nlevels; kf.mvScaleFactors = F.mvScaleFactors; kf.mTcw = Tcw; kf.mvpMapPoints.assign(N, nullptr);
    other.N = 1; other.mvuRight.assign(1, -1.0f); other.mDescriptors.create(1, 32, CV_8UC1); memset(other.mDescriptors.ptr(0), 0, 32);
    std::vector<MapPoint*> owned;
    F.mvpMapPoints.assign(N, nullptr);
    for (int i = 0; i < N; i++)
        if (holds && holds[i]) {
            MapPoint* p = new MapPoint(Eigen::Vector3f(0, 0, 1), &other, &map);
            if (holds[i] == 1) p->AddObservation(&other, 0);
            F.mvpMapPoints[i] = p; owned.push_back(p);
        }

    // Tracking.cc:3876-3887 / :3269-3280
    std::vector<std::pair<float, int> > vDepthIdx;
    vDepthIdx.reserve(N);
    for (int i = 0; i < N; i++) {
        float z = F.mvDepth[i];
        if (z > 0) vDepthIdx.push_back(std::make_pair(z, i));
    }
    int created = 0;
    *processed = 0;
    if (!vDepthIdx.empty()) {
        std::sort(vDepthIdx.begin(), vDepthIdx.end());                      // :3892 / :3286
        int nPoints = 0;
        for (size_t j = 0; j < vDepthIdx.size(); j++) {
            int i = vDepthIdx[j].second;
            bool bCreateNew = false;
            MapPoint* pMP = F.mvpMapPoints[i];
            if (!pMP) bCreateNew = true;
            else if (pMP->Observations() < 1) bCreateNew = true;            // :3907 / :3303
            if (bCreateNew) {
                Eigen::Vector3f x3D;
                F.UnprojectStereo(i, x3D);                                  // :3919 / :3314 (Nleft == -1)
                MapPoint* pNewMP;
                if (mode == 1) {
                    pNewMP = new MapPoint(x3D, &map, &F, i);                // :3321
                } else {
                    pNewMP = new MapPoint(x3D, &kf, &map);                  // :3925
                    pNewMP->AddObservation(&kf, i);                         // :3927
                    kf.AddMapPoint(pNewMP, i);                              // :3937
                    pNewMP->ComputeDistinctiveDescriptors();                // :3938
                    pNewMP->UpdateNormalAndDepth();                         // :3939
                }
                F.mvpMapPoints[i] = pNewMP; owned.push_back(pNewMP);
                const Eigen::Vector3f P = pNewMP->GetWorldPos(), Nv = pNewMP->GetNormal();
                const float v[8] = {P(0), P(1), P(2), Nv(0), Nv(1), Nv(2), pNewMP->mfMinDistance, pNewMP->mfMaxDistance};
                memcpy(fields + 8 * (size_t)created, v, sizeof v);
                const cv::Mat d = pNewMP->GetDescriptor();
                memcpy(desc_out + 32 * (size_t)created, d.ptr(0), 32);
                feat[created++] = i;
                nPoints++;
            } else {
                nPoints++;
            }
            *processed = nPoints;
            if (vDepthIdx[j].first > th_depth && nPoints > max_points) break;      // :3954 / :3338
        }
    }
    for (MapPoint* p : owned) delete p;
    return created;
}

}  // extern "C"
