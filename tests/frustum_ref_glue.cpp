// frustum_ref_glue.cpp — the reference's own Frame::isInFrustum (src/Frame.cc:602-664), MapPoint::PredictScale(…, Frame*)
// (src/MapPoint.cc:531-546), MapPoint::Get{Min,Max}DistanceInvariance (:500-512) and Pinhole::project
// (src/CameraModels/Pinhole.cpp:43-49), UNMODIFIED: tests/frustum_golden.py cuts the five function definitions out of the
// reference's sources by signature into frustum_ref_bodies.inc in the build directory (never committed) and compiles this
// file against the stand-in types of frustum_ref_types.h with -O2 -ffp-contract=off.  TEST INFRASTRUCTURE.
#include <stdint.h>

#include "frustum_ref_types.h"

namespace ORB_SLAM3 {
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
#include "frustum_ref_bodies.inc"
}  // namespace ORB_SLAM3

// One isInFrustum call per considered point, each on a fresh MapPoint.  rec: 5 floats per point (mTrackProjX, mTrackProjY,
// mTrackProjXR, mTrackDepth, mTrackViewCos), level: mnTrackScaleLevel - the last four as the call left them (-7: not written).
extern "C" void ref_frustum(int n1, const uint8_t* consider, const float* pos, const float* normal, const float* min_dist,
                            const float* max_dist, const float* Rcw, const float* tcw, const float* Ow, const float* K,
                            const float* bounds, float mbf, float log_scale_factor, int n_levels, float viewing_cos_limit,
                            uint8_t* in_view, uint8_t* returned, float* rec, int32_t* level) {
  using namespace ORB_SLAM3;
  Pinhole cam;
  cam.mvParameters.assign(K, K + 4);
  Frame F;
  F.mpCamera = &cam;
  F.mbf = mbf; F.mfLogScaleFactor = log_scale_factor; F.mnScaleLevels = n_levels;
  Frame::mnMinX = bounds[0]; Frame::mnMinY = bounds[1]; Frame::mnMaxX = bounds[2]; Frame::mnMaxY = bounds[3];
  for (int i = 0; i < 3; ++i) {
    F.mtcw(i) = tcw[i]; F.mOw(i) = Ow[i];
    for (int j = 0; j < 3; ++j) F.mRcw(i, j) = Rcw[3 * i + j];
  }
  for (int i = 0; i < n1; ++i) {
    MapPoint mp;
    if (!consider || consider[i]) {
      for (int k = 0; k < 3; ++k) { mp.mWorldPos(k) = pos[3 * i + k]; mp.mNormalVector(k) = normal[3 * i + k]; }
      mp.mfMinDistance = min_dist[i]; mp.mfMaxDistance = max_dist[i];
      returned[i] = F.isInFrustum(&mp, viewing_cos_limit) ? 1 : 0;
    } else {
      mp.mbTrackInView = false;
      returned[i] = 0;
    }
    in_view[i] = mp.mbTrackInView ? 1 : 0;
    rec[5 * i] = mp.mTrackProjX; rec[5 * i + 1] = mp.mTrackProjY; rec[5 * i + 2] = mp.mTrackProjXR; rec[5 * i + 3] = mp.mTrackDepth;
    rec[5 * i + 4] = mp.mTrackViewCos;
    level[i] = mp.mnTrackScaleLevel;
  }
}
