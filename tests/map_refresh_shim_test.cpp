// map_refresh_shim_test.cpp — rgbl_shim::DeviceLocalMap::Refresh (orb_slam3_rgbl_amd/shim/LocalMap.h) on stand-in MapPoint /
// KeyFrame types of its own, against a literal host transcription of MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:426-494)
// and MapPoint::ComputeDistinctiveDescriptors (:329-403) on those types.
//   usage: map_refresh_shim_test
// Two copies of one random map (key frames on a trajectory, some bad, some without a resident copy; points with 0 .. 30
// observations, some bad, some whose reference key frame does not observe them): the transcription runs on one, Refresh on
// the other; compared are every MapPoint's normal, mfMinDistance, mfMaxDistance and descriptor, bit for bit, and the pool's
// slots read back with rgbl_map_points_download - after both functions at once, after each alone, after moved positions,
// and for points that have to fall back to Update.
// Build with -ffp-contract=off: the transcription's float arithmetic must not be fused.
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

#include "../orb_slam3_rgbl_amd/shim/cv_compat.h"
#include "../orb_slam3_rgbl_amd/shim/LocalMap.h"

namespace {

// the slice of Eigen the transcribed lines use, with the evaluation order of oracle/cvcompat/sophus/sim3.hpp
struct V3 {
  float v[3];
  float operator()(int i) const { return v[i]; }
  float& operator()(int i) { return v[i]; }
  void setZero() { v[0] = v[1] = v[2] = 0.f; }
  V3 operator-(const V3& o) const { return V3{{v[0] - o.v[0], v[1] - o.v[1], v[2] - o.v[2]}}; }
  V3 operator+(const V3& o) const { return V3{{v[0] + o.v[0], v[1] + o.v[1], v[2] + o.v[2]}}; }
  V3 operator/(float s) const { return V3{{v[0] / s, v[1] / s, v[2] / s}}; }
  float squaredNorm() const { float s = v[0] * v[0]; s += v[1] * v[1]; s += v[2] * v[2]; return s; }
  float norm() const { return sqrtf(squaredNorm()); }
};

int DescriptorDistance(const cv::Mat& a, const cv::Mat& b) {   // src/ORBmatcher.cc:2058-2074
  const int32_t* pa = a.ptr<int32_t>();
  const int32_t* pb = b.ptr<int32_t>();
  int dist = 0;
  for (int i = 0; i < 8; i++, pa++, pb++) {
    unsigned int v = *pa ^ *pb;
    v = v - ((v >> 1) & 0x55555555);
    v = (v & 0x33333333) + ((v >> 2) & 0x33333333);
    dist += (((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) >> 24;
  }
  return dist;
}

struct KeyFrame {
  int NLeft = -1;
  bool bad = false;
  V3 Ow;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvScaleFactors;
  int mnScaleLevels = 0;
  cv::Mat mDescriptors;
  rgbl_device_frame* mpDeviceFrame = nullptr;
  bool isBad() { return bad; }
  V3 GetCameraCenter() { return Ow; }
};

struct MapPoint {
  std::map<KeyFrame*, std::tuple<int, int>> mObservations;
  KeyFrame* mpRefKF = nullptr;
  V3 mWorldPos, mNormalVector;
  float mfMinDistance = 0, mfMaxDistance = 0;
  cv::Mat mDescriptor;
  bool mbBad = false;
  bool isBad() { return mbBad; }
  std::map<KeyFrame*, std::tuple<int, int>> GetObservations() { return mObservations; }
  KeyFrame* GetReferenceKeyFrame() { return mpRefKF; }
  V3 GetWorldPos() { return mWorldPos; }
  V3 GetNormal() { return mNormalVector; }
  float GetMinDistance() { return mfMinDistance; }
  float GetMaxDistance() { return mfMaxDistance; }
  cv::Mat GetDescriptor() { return mDescriptor.clone(); }
  void SetNormalVector(const V3& normal) { mNormalVector = normal; }
  void SetMinMaxDistance(float fMin, float fMax) { mfMinDistance = fMin; mfMaxDistance = fMax; }
  void SetDescriptor(const cv::Mat& d) { mDescriptor = d.clone(); }
  void ComputeDistinctiveDescriptors();
  void UpdateNormalAndDepth();
};

// src/MapPoint.cc:329-403 (single-camera key frames: rightIndex == -1)
void MapPoint::ComputeDistinctiveDescriptors() {
  std::vector<cv::Mat> vDescriptors;
  std::map<KeyFrame*, std::tuple<int, int>> observations;
  {
    if (mbBad) return;
    observations = mObservations;
  }
  if (observations.empty()) return;
  vDescriptors.reserve(observations.size());
  for (std::map<KeyFrame*, std::tuple<int, int>>::iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
    KeyFrame* pKF = mit->first;
    if (!pKF->isBad()) {
      std::tuple<int, int> indexes = mit->second;
      int leftIndex = std::get<0>(indexes), rightIndex = std::get<1>(indexes);
      if (leftIndex != -1) {
        vDescriptors.push_back(pKF->mDescriptors.row(leftIndex));
      }
      if (rightIndex != -1) {
        vDescriptors.push_back(pKF->mDescriptors.row(rightIndex));
      }
    }
  }
  if (vDescriptors.empty()) return;
  const size_t N = vDescriptors.size();
  std::vector<std::vector<float>> Distances(N, std::vector<float>(N));   // float Distances[N][N]
  for (size_t i = 0; i < N; i++) {
    Distances[i][i] = 0;
    for (size_t j = i + 1; j < N; j++) {
      int distij = DescriptorDistance(vDescriptors[i], vDescriptors[j]);
      Distances[i][j] = distij;
      Distances[j][i] = distij;
    }
  }
  int BestMedian = INT_MAX;
  int BestIdx = 0;
  for (size_t i = 0; i < N; i++) {
    std::vector<int> vDists(Distances[i].begin(), Distances[i].end());
    std::sort(vDists.begin(), vDists.end());
    int median = vDists[0.5 * (N - 1)];
    if (median < BestMedian) {
      BestMedian = median;
      BestIdx = i;
    }
  }
  {
    mDescriptor = vDescriptors[BestIdx].clone();
  }
}

// src/MapPoint.cc:426-494 (NLeft == -1)
void MapPoint::UpdateNormalAndDepth() {
  std::map<KeyFrame*, std::tuple<int, int>> observations;
  KeyFrame* pRefKF;
  V3 Pos;
  {
    if (mbBad) return;
    observations = mObservations;
    pRefKF = mpRefKF;
    Pos = mWorldPos;
  }
  if (observations.empty()) return;
  V3 normal;
  normal.setZero();
  int n = 0;
  for (std::map<KeyFrame*, std::tuple<int, int>>::iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
    KeyFrame* pKF = mit->first;
    std::tuple<int, int> indexes = mit->second;
    int leftIndex = std::get<0>(indexes), rightIndex = std::get<1>(indexes);
    if (leftIndex != -1) {
      V3 Owi = pKF->GetCameraCenter();
      V3 normali = Pos - Owi;
      normal = normal + normali / normali.norm();
      n++;
    }
    (void)rightIndex;
  }
  V3 PC = Pos - pRefKF->GetCameraCenter();
  const float dist = PC.norm();
  std::tuple<int, int> indexes = observations[pRefKF];
  int leftIndex = std::get<0>(indexes);
  int level;
  level = pRefKF->mvKeysUn[leftIndex].octave;
  const float levelScaleFactor = pRefKF->mvScaleFactors[level];
  const int nLevels = pRefKF->mnScaleLevels;
  {
    mfMaxDistance = dist * levelScaleFactor;
    mfMinDistance = mfMaxDistance / pRefKF->mvScaleFactors[nLevels - 1];
    mNormalVector = normal / n;
  }
}

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  int below(int n) { return (int)(next() % (uint32_t)n); }
  float unit() { return (float)(next() & 0xffffff) / 16777216.f; }
};

struct World {
  std::vector<KeyFrame> kfs;
  std::vector<MapPoint> points;
};

// the same map twice (A for the transcription, B for Refresh): pointers differ, contents and orders do not
void build(World& W, int nKFs, int nPoints, bool resident, std::vector<rgbl_device_frame*>& frames) {
  Rng rng{12345};
  W.kfs.resize(nKFs);
  W.points.resize(nPoints);
  for (int k = 0; k < nKFs; ++k) {
    KeyFrame& kf = W.kfs[k];
    const int n = 150 + rng.below(120);
    kf.Ow = V3{{0.9f * k, 0.1f * sinf(0.7f * k), 4.f * sinf(0.11f * k)}};
    kf.bad = k % 9 == 4;
    kf.mnScaleLevels = 8;
    kf.mvScaleFactors.assign(8, 1.f);
    for (int l = 1; l < 8; ++l) kf.mvScaleFactors[l] = kf.mvScaleFactors[l - 1] * 1.2f;
    kf.mvKeysUn.resize(n);
    kf.mDescriptors.create(n, 32, CV_8U);
    for (int i = 0; i < n; ++i) {
      kf.mvKeysUn[i].pt.x = 1200.f * rng.unit(); kf.mvKeysUn[i].pt.y = 370.f * rng.unit(); kf.mvKeysUn[i].octave = rng.below(8);
      for (int b = 0; b < 32; ++b) kf.mDescriptors.ptr<uint8_t>(i)[b] = (uint8_t)rng.below(256);
    }
  }
  std::vector<int> used(nKFs, 0);
  for (int p = 0; p < nPoints; ++p) {
    MapPoint& mp = W.points[p];
    const int cat = rng.below(100);
    int c = cat < 4 ? 0 : cat < 8 ? 1 : cat < 97 ? 2 + rng.below(std::min(20, nKFs - 2)) : nKFs;   // key frames are distinct per point
    uint8_t base[32];
    for (int b = 0; b < 32; ++b) base[b] = (uint8_t)rng.below(256);
    std::vector<int> order(nKFs);
    for (int k = 0; k < nKFs; ++k) order[k] = k;
    for (int k = nKFs - 1; k > 0; --k) std::swap(order[k], order[rng.below(k + 1)]);
    const uint8_t* prev = nullptr;
    for (int i = 0; i < c; ++i) {
      KeyFrame& kf = W.kfs[order[i]];
      const int f = used[order[i]]++ % (int)kf.mvKeysUn.size();
      uint8_t* row = kf.mDescriptors.ptr<uint8_t>(f);
      if (prev && rng.below(100) < 15) memcpy(row, prev, 32);   // an exact copy: ties
      else
        for (int b = 0; b < 32; ++b) { uint8_t flip = 0; for (int j = 0; j < 8; ++j) flip |= (uint8_t)((rng.below(100) < 8) << j); row[b] = base[b] ^ flip; }
      prev = row;
      mp.mObservations[&kf] = std::make_tuple(f, -1);
    }
    mp.mpRefKF = c && rng.below(10) ? mp.mObservations.begin()->first : &W.kfs[order[nKFs - 1]];   // the latter observes it only when c == nKFs
    const KeyFrame& anchor = W.kfs[order[0]];
    for (int k = 0; k < 3; ++k) mp.mWorldPos.v[k] = anchor.Ow.v[k] + (rng.unit() - 0.5f) * 60.f;
    for (int k = 0; k < 3; ++k) mp.mNormalVector.v[k] = rng.unit();
    mp.mfMinDistance = 1.f + rng.unit(); mp.mfMaxDistance = 30.f + rng.unit();
    mp.mDescriptor.create(1, 32, CV_8U);
    for (int b = 0; b < 32; ++b) mp.mDescriptor.ptr<uint8_t>()[b] = (uint8_t)rng.below(256);
    mp.mbBad = p % 17 == 3;
  }
  if (!resident) return;
  for (int k = 0; k < nKFs; ++k) {
    KeyFrame& kf = W.kfs[k];
    const int n = (int)kf.mvKeysUn.size();
    std::vector<float> xy(2 * n);
    std::vector<int32_t> oct(n);
    for (int i = 0; i < n; ++i) { xy[2 * i] = kf.mvKeysUn[i].pt.x; xy[2 * i + 1] = kf.mvKeysUn[i].pt.y; oct[i] = kf.mvKeysUn[i].octave; }
    rgbl_device_frame* f = nullptr;
    if (rgbl_device_frame_create(0, n, &f) != RGBL_OK || rgbl_device_frame_upload(f, n, kf.mDescriptors.ptr<uint8_t>(), xy.data(), oct.data(), nullptr) != RGBL_OK) {
      fprintf(stderr, "device frame: %s\n", rgbl_last_error());
      exit(2);
    }
    frames.push_back(f);
    kf.mpDeviceFrame = f;
  }
}

bool same_float(float a, float b) { return memcmp(&a, &b, 4) == 0 || (a != a && b != b); }
bool same_point(const MapPoint& a, const MapPoint& b) {
  for (int k = 0; k < 3; ++k)
    if (!same_float(a.mNormalVector.v[k], b.mNormalVector.v[k]) || !same_float(a.mWorldPos.v[k], b.mWorldPos.v[k])) return false;
  return same_float(a.mfMinDistance, b.mfMinDistance) && same_float(a.mfMaxDistance, b.mfMaxDistance) &&
         memcmp(a.mDescriptor.ptr<uint8_t>(), b.mDescriptor.ptr<uint8_t>(), 32) == 0;
}
int count_differing(const World& A, const World& B) {
  int n = 0;
  for (size_t i = 0; i < A.points.size(); ++i) n += !same_point(A.points[i], B.points[i]);
  return n;
}
// every registered point's slot holds what the MapPoint holds
int count_stale_slots(World& B, rgbl_shim::DeviceLocalMap& lm, int* registered) {
  int n = 0;
  *registered = 0;
  for (MapPoint& p : B.points) {
    const int32_t slot = lm.SlotOf(&p);
    if (slot < 0) continue;
    ++*registered;
    MapPoint q;
    q.mDescriptor.create(1, 32, CV_8U);
    if (rgbl_map_points_download(lm.handle(), 1, &slot, q.mWorldPos.v, q.mNormalVector.v, &q.mfMinDistance, &q.mfMaxDistance, q.mDescriptor.ptr<uint8_t>()) != RGBL_OK) return -1;
    n += !same_point(p, q);
  }
  return n;
}

}  // namespace

int main() {
  const int nKFs = 30, nPoints = 400;
  World A, B;
  std::vector<rgbl_device_frame*> none, frames;
  build(A, nKFs, nPoints, false, none);
  build(B, nKFs, nPoints, true, frames);
  int failures = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { ++failures; printf("MISMATCH: %s\n", what); } };
  std::vector<MapPoint*> all;
  for (MapPoint& p : B.points) all.push_back(&p);
  all.push_back(&B.points[7]);   // a point listed twice is refreshed once
  int live = 0, outsiders = 0, onBad = 0;
  for (MapPoint& p : A.points) {
    if (p.mbBad || p.mObservations.empty()) continue;
    ++live;
    outsiders += !p.mObservations.count(p.mpRefKF);
    for (auto& o : p.mObservations) onBad += o.first->bad;
  }
  expect(live > 300 && outsiders > 10 && onBad > 100, "the map exercises the rules");
  expect(count_differing(A, B) == 0, "both copies start equal");
  {
    rgbl_shim::DeviceLocalMap lm(0, 64);   // grows
    int onDevice = -1, registered = 0;
    // 1. both functions, half of the points registered beforehand
    std::vector<MapPoint*> half(all.begin(), all.begin() + nPoints / 2);
    expect(lm.Update(half), "Update");
    for (MapPoint& p : A.points) { p.UpdateNormalAndDepth(); p.ComputeDistinctiveDescriptors(); }
    expect(lm.Refresh(all, true, true, &onDevice) && onDevice == live, "Refresh(normal, descriptor) takes every live point the device way");
    expect(count_differing(A, B) == 0, "Refresh(normal, descriptor) against the transcription");
    expect(count_stale_slots(B, lm, &registered) == 0 && registered >= live, "the slots hold what the MapPoints hold");
    // 2. moved positions (bundle adjustment), the normals alone: the descriptors stay
    Rng rng{77};
    for (int i = 0; i < nPoints; ++i) {
      const float d[3] = {rng.unit() - 0.5f, rng.unit() - 0.5f, rng.unit() - 0.5f};
      for (int k = 0; k < 3; ++k) { A.points[i].mWorldPos.v[k] += d[k]; B.points[i].mWorldPos.v[k] += d[k]; }
      if (i % 5 == 0) { A.points[i].mDescriptor.ptr<uint8_t>()[3] ^= 0x10; B.points[i].mDescriptor.ptr<uint8_t>()[3] ^= 0x10; }   // would be undone by ComputeDistinctiveDescriptors
    }
    for (MapPoint& p : A.points) p.UpdateNormalAndDepth();
    expect(lm.Refresh(all, true, false, &onDevice) && onDevice == live, "Refresh(normal)");
    expect(count_differing(A, B) == 0, "Refresh(normal) against UpdateNormalAndDepth");
    // (the slots of the points whose descriptor was touched on the host alone are stale in that field until the next Update)
    // 3. the descriptors alone, after a key frame has turned bad: the normals stay
    A.kfs[2].bad = B.kfs[2].bad = true;
    for (int i = 0; i < nPoints; i += 3) { A.points[i].mfMaxDistance += 1.f; B.points[i].mfMaxDistance += 1.f; }
    for (MapPoint& p : A.points) p.ComputeDistinctiveDescriptors();
    expect(lm.Refresh(all, false, true, &onDevice) && onDevice == live, "Refresh(descriptor)");
    expect(count_differing(A, B) == 0, "Refresh(descriptor) against ComputeDistinctiveDescriptors");
    expect(lm.Update(all), "Update of every point");
    expect(count_stale_slots(B, lm, &registered) == 0 && registered == nPoints, "after Update the slots hold what the MapPoints hold");
    // 4. a key frame without a resident copy: its points get the MapPoint's own two functions on the host and are uploaded as they come out
    B.kfs[5].mpDeviceFrame = nullptr;
    int through5 = 0;
    for (MapPoint& p : B.points) through5 += !p.mbBad && !p.mObservations.empty() && (p.mObservations.count(&B.kfs[5]) || p.mpRefKF == &B.kfs[5]);
    for (int i = 0; i < nPoints; ++i) {
      for (int k = 0; k < 3; ++k) { A.points[i].mWorldPos.v[k] *= 1.01f; B.points[i].mWorldPos.v[k] *= 1.01f; }
      A.points[i].UpdateNormalAndDepth();
      A.points[i].ComputeDistinctiveDescriptors();
    }
    expect(through5 > 20 && lm.Refresh(all, true, true, &onDevice) && onDevice == live - through5, "Refresh runs the host functions for the points of a non-resident key frame");
    expect(count_differing(A, B) == 0, "Refresh with a non-resident key frame");
    // the descriptors alone do not need the reference key frame: only the points kf 5 observes take the host way
    int observed5 = 0;
    for (MapPoint& p : B.points) observed5 += !p.mbBad && p.mObservations.count(&B.kfs[5]);
    A.kfs[7].bad = B.kfs[7].bad = true;
    for (MapPoint& p : A.points) p.ComputeDistinctiveDescriptors();
    expect(observed5 < through5 && lm.Refresh(all, false, true, &onDevice) && onDevice == live - observed5, "Refresh(descriptor) ignores a non-resident reference key frame");
    expect(count_differing(A, B) == 0, "Refresh(descriptor) with a non-resident key frame");
    int stale = 0;
    for (MapPoint& p : B.points) {   // the slots of the live points - device way or Update - hold the present values; bad / unobserved points were not touched
      if (p.mbBad || p.mObservations.empty()) continue;
      const int32_t slot = lm.SlotOf(&p);
      MapPoint q;
      q.mDescriptor.create(1, 32, CV_8U);
      if (slot < 0 || rgbl_map_points_download(lm.handle(), 1, &slot, q.mWorldPos.v, q.mNormalVector.v, &q.mfMinDistance, &q.mfMaxDistance, q.mDescriptor.ptr<uint8_t>()) != RGBL_OK) { ++stale; continue; }
      stale += !same_point(p, q);
    }
    expect(stale == 0, "every live point's slot holds its present values");
    // 5. nothing to do
    std::vector<MapPoint*> empty;
    expect(lm.Refresh(empty, true, true, &onDevice) && onDevice == 0, "empty list");
    expect(lm.Refresh(all, false, false, &onDevice) && onDevice == 0, "neither function");
  }
  for (rgbl_device_frame* f : frames) rgbl_device_frame_destroy(f);
  rgbl_matcher_pool_clear();
  if (failures) return 1;
  printf("points %d live %d reference key frame not an observer %d observations on bad key frames %d\n", nPoints, live, outsiders, onBad);
  printf("MAP_REFRESH_SHIM_OK\n");
  return 0;
}
