// local_map_shim_test.cpp — the drop-in ORBmatcher::SearchLocalPoints (orb_slam3_rgbl_amd/shim/ORBmatcher.h) and
// rgbl_shim::DeviceLocalMap (shim/LocalMap.h) on stand-in Frame / MapPoint types of its own, against a literal host
// transcription of Tracking::SearchLocalPoints' second half (src/Tracking.cc:3399-3448) with Frame::isInFrustum
// (src/Frame.cc:602-664) and MapPoint::PredictScale (src/MapPoint.cc:531-546) on those types, followed by the drop-in
// SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) as the reference calls it.
//   usage: local_map_shim_test <case.bin> <out.bin> [threads | abi_threads]
// Compared after each variant (host arrays; DeviceLocalMap with half of the points registered beforehand; after Erase and
// re-use of slots): every MapPoint field the loop writes, the IncreaseVisible counts, F.mmProjectPoints, F.mvpMapPoints,
// nToMatch and the return value.  out.bin carries the transcription's results for the Python side (tests/test_local_map_shim.py),
// which holds them to the restatement and the oracle.  `threads`: one thread searches while another registers, updates and
// erases OTHER points of the same DeviceLocalMap; `abi_threads`: the same on the C ABI itself (rgbl_track_local_points on slots
// [0, n) next to rgbl_map_points_update / _reserve on [n, 2n)); every search must equal the single-threaded one.
// Build with -ffp-contract=off: the transcription's float arithmetic must not be fused.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <map>
#include <thread>
#include <vector>

#include "../orb_slam3_rgbl_amd/shim/ORBmatcher.h"

namespace {

// the slice of Eigen the transcribed lines use, with the evaluation order of oracle/cvcompat/sophus/sim3.hpp
struct V3 {
  float v[3];
  float operator()(int i) const { return v[i]; }
  V3 operator-(const V3& o) const { return V3{{v[0] - o.v[0], v[1] - o.v[1], v[2] - o.v[2]}}; }
  V3 operator+(const V3& o) const { return V3{{v[0] + o.v[0], v[1] + o.v[1], v[2] + o.v[2]}}; }
  float dot(const V3& o) const { float s = v[0] * o.v[0]; s += v[1] * o.v[1]; s += v[2] * o.v[2]; return s; }
  float norm() const { return sqrtf(dot(*this)); }
};
struct V2 { float v[2]; float operator()(int i) const { return v[i]; } };
struct M3 {
  float m[9];
  float operator()(int i, int j) const { return m[3 * i + j]; }
  V3 operator*(const V3& p) const {
    return V3{{m[0] * p(0) + m[1] * p(1) + m[2] * p(2), m[3] * p(0) + m[4] * p(1) + m[5] * p(2), m[6] * p(0) + m[7] * p(1) + m[8] * p(2)}};
  }
};
struct SE3 {
  M3 R; V3 t;
  M3 rotationMatrix() const { return R; }
  V3 translation() const { return t; }
};
struct Camera {
  float p[4];
  float getParameter(int i) const { return p[i]; }
  V2 project(const V3& c) const { return V2{{p[0] * c(0) / c(2) + p[2], p[1] * c(1) / c(2) + p[3]}}; }   // Pinhole.cpp:43-49
};

struct Frame;
struct MapPoint {
  long unsigned int mnId = 0, mnLastFrameSeen = 0;
  float mTrackProjX = -7, mTrackProjY = -7, mTrackDepth = -7, mTrackProjXR = -7, mTrackViewCos = -7;
  bool mbTrackInView = true;   // stale values: the loop has to overwrite what the reference overwrites, and nothing else
  int mnTrackScaleLevel = -7;
  V3 pos, normal;
  float mfMinDistance = 0, mfMaxDistance = 0;
  cv::Mat desc;
  int nObs = 0, mnVisible = 1;
  bool bad = false;
  V3 GetWorldPos() { return pos; }
  V3 GetNormal() { return normal; }
  float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
  float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
  float GetMinDistance() { return mfMinDistance; }
  float GetMaxDistance() { return mfMaxDistance; }
  cv::Mat GetDescriptor() { return desc.clone(); }
  int Observations() { return nObs; }
  bool isBad() { return bad; }
  void IncreaseVisible(int n = 1) { mnVisible += n; }
  int PredictScale(const float& currentDist, Frame* pF);
};

struct Frame {
  long unsigned int mnId = 5;
  int N = 0, Nleft = -1;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvuRight, mvScaleFactors;
  cv::Mat mDescriptors;
  std::vector<MapPoint*> mvpMapPoints;
  std::map<long unsigned int, cv::Point2f> mmProjectPoints;
  int mnScaleLevels = 0;
  float mfLogScaleFactor = 0, mbf = 0;
  Camera* mpCamera = nullptr;
  static float mnMinX, mnMinY, mnMaxX, mnMaxY, mfGridElementWidthInv, mfGridElementHeightInv;
  M3 mRcw; V3 mtcw, mOw;
  SE3 GetPose() const { return SE3{mRcw, mtcw}; }
  V3 GetOw() const { return mOw; }
  bool isInFrustum(MapPoint* pMP, float viewingCosLimit);
};
float Frame::mnMinX, Frame::mnMinY, Frame::mnMaxX, Frame::mnMaxY, Frame::mfGridElementWidthInv, Frame::mfGridElementHeightInv;

// src/MapPoint.cc:531-546
int MapPoint::PredictScale(const float& currentDist, Frame* pF) {
  float ratio;
  {
    ratio = mfMaxDistance / currentDist;
  }
  int nScale = ceil(logf(ratio) / pF->mfLogScaleFactor);
  if (nScale < 0)
    nScale = 0;
  else if (nScale >= pF->mnScaleLevels)
    nScale = pF->mnScaleLevels - 1;
  return nScale;
}

// src/Frame.cc:602-664, the Nleft == -1 branch
bool Frame::isInFrustum(MapPoint* pMP, float viewingCosLimit) {
  pMP->mbTrackInView = false;
  pMP->mTrackProjX = -1;
  pMP->mTrackProjY = -1;
  V3 P = pMP->GetWorldPos();
  const V3 Pc = mRcw * P + mtcw;
  const float Pc_dist = Pc.norm();
  const float PcZ = Pc(2);
  const float invz = 1.0f / PcZ;
  if (PcZ < 0.0f) return false;
  const V2 uv = mpCamera->project(Pc);
  if (uv(0) < mnMinX || uv(0) > mnMaxX) return false;
  if (uv(1) < mnMinY || uv(1) > mnMaxY) return false;
  pMP->mTrackProjX = uv(0);
  pMP->mTrackProjY = uv(1);
  const float maxDistance = pMP->GetMaxDistanceInvariance();
  const float minDistance = pMP->GetMinDistanceInvariance();
  const V3 PO = P - mOw;
  const float dist = PO.norm();
  if (dist < minDistance || dist > maxDistance) return false;
  V3 Pn = pMP->GetNormal();
  const float viewCos = PO.dot(Pn) / dist;
  if (viewCos < viewingCosLimit) return false;
  const int nPredictedLevel = pMP->PredictScale(dist, this);
  pMP->mbTrackInView = true;
  pMP->mTrackProjX = uv(0);
  pMP->mTrackProjXR = uv(0) - mbf * invz;
  pMP->mTrackDepth = Pc_dist;
  pMP->mTrackProjY = uv(1);
  pMP->mnTrackScaleLevel = nPredictedLevel;
  pMP->mTrackViewCos = viewCos;
  return true;
}

struct World {
  Frame F;
  Camera cam;
  std::vector<MapPoint> points;
  std::vector<MapPoint*> local;
  std::vector<MapPoint> holders;   // what F.mvpMapPoints holds on entry
  float th = 3, thFar = 40;
  int farPoints = 0;
};

template <class T> bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

bool load(const char* path, World& W) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int hdr[4];   // n1, n2, n_levels, far_points
  float fl[30];  // th, th_far, grid[6], Rcw[9], tcw[3], Ow[3], K[4], mbf, log_scale_factor
  if (!rd(f, hdr, 4) || !rd(f, fl, 30)) return false;
  const int n1 = hdr[0], n2 = hdr[1];
  W.th = fl[0]; W.thFar = fl[1]; W.farPoints = hdr[3];
  Frame& F = W.F;
  Frame::mnMinX = fl[2]; Frame::mnMinY = fl[3]; Frame::mnMaxX = fl[4]; Frame::mnMaxY = fl[5];
  Frame::mfGridElementWidthInv = fl[6]; Frame::mfGridElementHeightInv = fl[7];
  memcpy(F.mRcw.m, fl + 8, 36); memcpy(F.mtcw.v, fl + 17, 12); memcpy(F.mOw.v, fl + 20, 12);
  memcpy(W.cam.p, fl + 23, 16);
  F.mpCamera = &W.cam;
  F.mbf = fl[27]; F.mfLogScaleFactor = fl[28];
  F.mnScaleLevels = hdr[2];
  F.mvScaleFactors.resize(hdr[2]);
  if (!rd(f, F.mvScaleFactors.data(), hdr[2])) return false;
  std::vector<float> pos(3 * n1), nrm(3 * n1), dmin(n1), dmax(n1), xy(2 * n2);
  std::vector<uint8_t> desc(32 * n1), obs(n1), cons(n1), blocked(n2);
  std::vector<int32_t> oct(n2);
  F.mvuRight.resize(n2);
  F.mDescriptors.create(n2, 32, CV_8U);
  if (!rd(f, pos.data(), pos.size()) || !rd(f, nrm.data(), nrm.size()) || !rd(f, dmin.data(), n1) || !rd(f, dmax.data(), n1) ||
      !rd(f, desc.data(), desc.size()) || !rd(f, obs.data(), n1) || !rd(f, cons.data(), n1) || !rd(f, xy.data(), xy.size()) ||
      !rd(f, oct.data(), n2) || !rd(f, F.mvuRight.data(), n2) || !rd(f, F.mDescriptors.ptr<uint8_t>(), (size_t)32 * n2) ||
      !rd(f, blocked.data(), n2))
    return false;
  fclose(f);
  W.points.resize(n1);
  for (int i = 0; i < n1; ++i) {
    MapPoint& p = W.points[i];
    p.mnId = 1000 + i;
    memcpy(p.pos.v, &pos[3 * i], 12); memcpy(p.normal.v, &nrm[3 * i], 12);
    p.mfMinDistance = dmin[i]; p.mfMaxDistance = dmax[i];
    p.desc.create(1, 32, CV_8U);
    memcpy(p.desc.ptr<uint8_t>(), &desc[32 * i], 32);
    p.nObs = obs[i];
    // consider1 == 0: alternately a bad point and one already seen in this frame (Tracking.cc:3406-3409; the loop in front,
    // :3380-3397, has cleared mbTrackInView of the latter)
    if (!cons[i]) { if (i & 1) p.bad = true; else { p.mnLastFrameSeen = F.mnId; p.mbTrackInView = false; } }
  }
  F.N = n2;
  F.mvKeysUn.resize(n2);
  W.holders.resize(2);
  W.holders[0].nObs = 1; W.holders[1].nObs = 0;
  F.mvpMapPoints.assign(n2, nullptr);
  for (int i = 0; i < n2; ++i) {
    F.mvKeysUn[i].pt.x = xy[2 * i]; F.mvKeysUn[i].pt.y = xy[2 * i + 1]; F.mvKeysUn[i].octave = oct[i];
    if (blocked[i]) F.mvpMapPoints[i] = &W.holders[0];
    else if (i % 7 == 0) F.mvpMapPoints[i] = &W.holders[1];   // holds a point without observations: not blocked
  }
  return true;
}

// what a run leaves behind
struct Outcome {
  int nToMatch = 0, ret = 0;
  std::vector<int32_t> inView, level, visible, match;   // match: index into the local map per feature, -1 = entry untouched
  std::vector<float> px, py, pxr, depth, vcos;
  std::map<long unsigned int, cv::Point2f> proj;
  bool operator==(const Outcome& o) const {
    auto same = [](const std::vector<float>& a, const std::vector<float>& b) {
      if (a.size() != b.size()) return false;
      for (size_t i = 0; i < a.size(); ++i)
        if (memcmp(&a[i], &b[i], 4) != 0 && !(a[i] != a[i] && b[i] != b[i])) return false;
      return true;
    };
    if (proj.size() != o.proj.size()) return false;
    for (auto it = proj.begin(), jt = o.proj.begin(); it != proj.end(); ++it, ++jt)
      if (it->first != jt->first || !same({it->second.x, it->second.y}, {jt->second.x, jt->second.y})) return false;
    return nToMatch == o.nToMatch && ret == o.ret && inView == o.inView && level == o.level && visible == o.visible && match == o.match &&
           same(px, o.px) && same(py, o.py) && same(pxr, o.pxr) && same(depth, o.depth) && same(vcos, o.vcos);
  }
};

Outcome collect(World& W, const std::vector<MapPoint*>& entry, int nToMatch, int ret) {
  Outcome o;
  o.nToMatch = nToMatch; o.ret = ret;
  for (MapPoint* p : W.local) {
    o.inView.push_back(p->mbTrackInView); o.level.push_back(p->mnTrackScaleLevel); o.visible.push_back(p->mnVisible);
    o.px.push_back(p->mTrackProjX); o.py.push_back(p->mTrackProjY); o.pxr.push_back(p->mTrackProjXR);
    o.depth.push_back(p->mTrackDepth); o.vcos.push_back(p->mTrackViewCos);
  }
  for (size_t i = 0; i < W.F.mvpMapPoints.size(); ++i) {
    MapPoint* p = W.F.mvpMapPoints[i];
    int32_t m = -1;
    if (p != entry[i]) {
      m = -2;
      for (size_t k = 0; k < W.local.size(); ++k) if (W.local[k] == p) { m = (int32_t)k; break; }   // the first entry that is this point
    }
    o.match.push_back(m);
  }
  o.proj = W.F.mmProjectPoints;
  return o;
}

// Tracking.cc:3399-3448 on the stand-in types (th, bFarPoints, thFarPoints as the caller passes them)
Outcome transcription(World& W) {
  const std::vector<MapPoint*> entry = W.F.mvpMapPoints;
  int nToMatch = 0, matches = 0;
  for (std::vector<MapPoint*>::iterator vit = W.local.begin(), vend = W.local.end(); vit != vend; vit++) {
    MapPoint* pMP = *vit;
    if (pMP->mnLastFrameSeen == W.F.mnId) continue;
    if (pMP->isBad()) continue;
    if (W.F.isInFrustum(pMP, 0.5)) {
      pMP->IncreaseVisible();
      nToMatch++;
    }
    if (pMP->mbTrackInView) {
      W.F.mmProjectPoints[pMP->mnId] = cv::Point2f(pMP->mTrackProjX, pMP->mTrackProjY);
    }
  }
  if (nToMatch > 0) {
    ORB_SLAM3::ORBmatcher matcher(0.8);
    matches = matcher.SearchByProjection(W.F, W.local, W.th, W.farPoints != 0, W.thFar);
  }
  return collect(W, entry, nToMatch, matches);
}

Outcome dropin(World& W, rgbl_shim::DeviceLocalMap* pLocalMap) {
  const std::vector<MapPoint*> entry = W.F.mvpMapPoints;
  ORB_SLAM3::ORBmatcher matcher(0.8);
  int nToMatch = -1;
  const int ret = matcher.SearchLocalPoints(W.F, W.local, W.th, W.farPoints != 0, W.thFar, 0.5f, pLocalMap, &nToMatch);
  return collect(W, entry, nToMatch, ret);
}

void fill_local(World& W, size_t n) {
  W.local.clear();
  for (size_t i = 0; i < n && i < W.points.size(); ++i) W.local.push_back(&W.points[i]);
  if (W.local.size() > 40) W.local[33] = W.local[5];   // a point listed twice is projected twice (and counted visible twice)
}

// The pool on the C ABI itself: one thread runs rgbl_track_local_points on slots [0, n) while another rewrites slots [n, 2n)
// and grows the pool (rgbl_map_points_update / _reserve); every search must return what it returns single-threaded.
bool abi_threads(World& W) {
  const int n = (int)W.points.size() / 2, n2 = W.F.N;
  std::vector<float> pos(6 * n), nrm(6 * n), dmin(2 * n), dmax(2 * n), xy2(2 * n2);
  std::vector<uint8_t> desc(64 * n), obs(n), blocked(n2, 0);
  std::vector<int32_t> slot(2 * n), oct2(n2);
  for (int i = 0; i < 2 * n; ++i) {
    MapPoint& p = W.points[i];
    memcpy(&pos[3 * i], p.pos.v, 12); memcpy(&nrm[3 * i], p.normal.v, 12);
    dmin[i] = p.mfMinDistance; dmax[i] = p.mfMaxDistance;
    memcpy(&desc[32 * i], p.desc.ptr<uint8_t>(), 32);
    slot[i] = i;
    if (i < n) obs[i] = p.nObs > 0;
  }
  for (int i = 0; i < n2; ++i) { xy2[2 * i] = W.F.mvKeysUn[i].pt.x; xy2[2 * i + 1] = W.F.mvKeysUn[i].pt.y; oct2[i] = W.F.mvKeysUn[i].octave; }
  rgbl_map_points* pool = nullptr;
  if (rgbl_map_points_create(0, 2 * n, &pool) != RGBL_OK) return false;
  if (rgbl_map_points_update(pool, n, slot.data(), pos.data(), nrm.data(), dmin.data(), dmax.data(), desc.data()) != RGBL_OK) return false;
  rgbl_track_local_input in{};
  in.n1 = n; in.pool = pool; in.slot1 = slot.data(); in.mp_observed1 = obs.data();
  in.n2 = n2; in.kp2_xy = xy2.data(); in.kp2_octave = oct2.data(); in.uright2 = W.F.mvuRight.data();
  in.desc2 = W.F.mDescriptors.ptr<uint8_t>(); in.blocked2 = blocked.data();
  in.grid[0] = Frame::mnMinX; in.grid[1] = Frame::mnMinY; in.grid[2] = Frame::mnMaxX; in.grid[3] = Frame::mnMaxY;
  in.grid[4] = Frame::mfGridElementWidthInv; in.grid[5] = Frame::mfGridElementHeightInv;
  in.scale_factors = W.F.mvScaleFactors.data(); in.n_levels = W.F.mnScaleLevels; in.th = W.th; in.nnratio = 0.8f;
  memcpy(in.Rcw, W.F.mRcw.m, 36); memcpy(in.tcw, W.F.mtcw.v, 12); memcpy(in.Ow, W.F.mOw.v, 12); memcpy(in.K, W.cam.p, 16);
  in.mbf = W.F.mbf; in.log_scale_factor = W.F.mfLogScaleFactor; in.viewing_cos_limit = 0.5f; in.th_far_points = W.thFar;
  struct Result {
    std::vector<uint8_t> iv; std::vector<rgbl_frustum_record> rec; std::vector<int32_t> m; int ntm = 0, nm = 0;
    bool run(rgbl_matcher* h, const rgbl_track_local_input& in) {
      iv.assign(in.n1, 0); rec.assign(in.n1, rgbl_frustum_record{}); m.assign(in.n2, -1);
      return rgbl_track_local_points(h, &in, iv.data(), rec.data(), &ntm, m.data(), &nm) == RGBL_OK;
    }
    bool operator==(const Result& o) const {
      return ntm == o.ntm && nm == o.nm && iv == o.iv && m == o.m && memcmp(rec.data(), o.rec.data(), rec.size() * sizeof(rgbl_frustum_record)) == 0;
    }
  } want;
  rgbl_matcher* h0 = nullptr;
  if (rgbl_matcher_create(0, &h0) != RGBL_OK || !want.run(h0, in) || want.ntm < 10) return false;
  std::atomic<int> bad{0};
  std::thread search([&]() {
    rgbl_matcher* h = nullptr;
    if (rgbl_matcher_create(0, &h) != RGBL_OK) { ++bad; return; }
    for (int r = 0; r < 4; ++r) {
      Result got;
      if (!got.run(h, in) || !(got == want)) ++bad;
    }
    rgbl_matcher_destroy(h);
  });
  std::thread update([&]() {
    for (int r = 0; r < 4; ++r) {
      // other values every round: the points of the first half, rotated by r
      std::vector<float> p2(3 * n), d2(n);
      for (int i = 0; i < n; ++i) { memcpy(&p2[3 * i], &pos[3 * ((i + r) % n)], 12); d2[i] = dmax[(i + r) % n]; }
      if (rgbl_map_points_update(pool, n, slot.data() + n, p2.data(), nrm.data(), dmin.data(), d2.data(), desc.data()) != RGBL_OK) ++bad;
      if (r == 2 && rgbl_map_points_reserve(pool, 3 * n) != RGBL_OK) ++bad;
    }
  });
  search.join();
  update.join();
  Result after;
  const bool ok = bad.load() == 0 && after.run(h0, in) && after == want;
  rgbl_matcher_destroy(h0);
  rgbl_map_points_destroy(pool);
  return ok;
}

template <class T> void wr(FILE* f, const std::vector<T>& v) { fwrite(v.data(), sizeof(T), v.size(), f); }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s case.bin out.bin [threads]\n", argv[0]); return 2; }
  const bool abi = argc > 3 && strcmp(argv[3], "abi_threads") == 0;
  const bool threads = abi || (argc > 3 && strcmp(argv[3], "threads") == 0);
  World base;
  if (!load(argv[1], base)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  auto fresh = [&](World& W, size_t n) {
    W = base;
    W.F.mpCamera = &W.cam;
    for (size_t i = 0; i < W.F.mvpMapPoints.size(); ++i)
      if (W.F.mvpMapPoints[i]) W.F.mvpMapPoints[i] = &W.holders[W.F.mvpMapPoints[i] - &base.holders[0]];
    fill_local(W, n);
  };
  int failures = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { ++failures; printf("MISMATCH: %s\n", what); } };
  if (!threads) {
    World A, B;
    const size_t n = base.points.size();
    fresh(A, n);
    const Outcome want = transcription(A);
    fresh(B, n);
    expect(dropin(B, nullptr) == want, "host arrays");
    {
      rgbl_shim::DeviceLocalMap lm(0, 64);   // grows several times
      fresh(B, n);
      std::vector<MapPoint*> half(B.local.begin(), B.local.begin() + (long)(n / 2));
      expect(lm.Update(half), "DeviceLocalMap::Update");
      expect(dropin(B, &lm) == want, "DeviceLocalMap, half of the points registered beforehand");
      expect(lm.size() > n / 2, "points met without a slot were registered");
      // a changed point: without Update the old values stay in use, with it the new ones
      fresh(A, n);
      A.points[40].pos = A.points[41].pos; A.points[40].mfMaxDistance = A.points[41].mfMaxDistance; A.points[40].normal = A.points[41].normal;
      const Outcome moved = transcription(A);
      fresh(B, n);
      // (B's objects live at the addresses of the run before: the slots stay valid)
      B.points[40].pos = B.points[41].pos; B.points[40].mfMaxDistance = B.points[41].mfMaxDistance; B.points[40].normal = B.points[41].normal;
      expect(lm.Update(&B.points[40]) >= 0, "Update of one point");
      expect(dropin(B, &lm) == moved, "DeviceLocalMap after the Update of a changed point");
      // Erase: the slots go to new points, the erased ones come back through the search
      fresh(B, n);
      expect(lm.Update(&B.points[40]) >= 0, "Update of the point that changed back");
      for (size_t i = 0; i < n; i += 3) lm.Erase(&B.points[i]);
      const size_t left = lm.size();
      std::vector<MapPoint> extra(50, base.points[0]);
      std::vector<MapPoint*> pe;
      for (MapPoint& e : extra) pe.push_back(&e);
      expect(lm.Update(pe) && lm.size() == left + 50, "erased slots are re-used");
      expect(dropin(B, &lm) == want, "DeviceLocalMap after Erase and re-use of slots");
      // a slot erased while a search is running is not handed out before that search has ended
      lm.BeginSearch();
      const int held = lm.SlotOf(&B.points[1]);
      lm.Erase(&B.points[1]);
      MapPoint late1 = base.points[2], late2 = base.points[3];
      expect(held >= 0 && lm.Update(&late1) >= 0 && lm.Update(&late1) != held, "an erased slot is not re-used during a search");
      lm.EndSearch();
      expect(lm.Update(&late2) == held, "... and is re-used after it");
    }
    // a shorter local map, bFarPoints, an empty one
    fresh(A, 65); fresh(B, 65);
    A.farPoints = B.farPoints = 1;
    const Outcome w65 = transcription(A);
    expect(dropin(B, nullptr) == w65, "65 points, bFarPoints");
    fresh(A, 0); fresh(B, 0);
    expect(dropin(B, nullptr) == transcription(A), "empty local map");
    // nothing to match: every point already seen in this frame
    fresh(A, n); fresh(B, n);
    for (MapPoint& p : A.points) p.mnLastFrameSeen = A.F.mnId;
    for (MapPoint& p : B.points) p.mnLastFrameSeen = B.F.mnId;
    const Outcome none = transcription(A);
    expect(none.nToMatch == 0 && dropin(B, nullptr) == none, "nothing considered");
    FILE* f = fopen(argv[2], "wb");
    if (!f) return 2;
    const int32_t hdr[4] = {(int32_t)want.inView.size(), (int32_t)want.match.size(), want.nToMatch, want.ret};
    fwrite(hdr, 4, 4, f);
    wr(f, want.inView); wr(f, want.level); wr(f, want.visible); wr(f, want.px); wr(f, want.py); wr(f, want.pxr); wr(f, want.depth);
    wr(f, want.vcos); wr(f, want.match);
    fclose(f);
    printf("nToMatch %d matches %d projected %zu\n", want.nToMatch, want.ret, want.proj.size());
  } else if (abi) {
    expect(abi_threads(base), "rgbl_track_local_points on slots [0, n) next to rgbl_map_points_update on [n, 2n)");
  } else {
    const size_t n = base.points.size() / 2;
    World A, B;
    fresh(A, n);
    const Outcome want = transcription(A);
    rgbl_shim::DeviceLocalMap lm(0, 32);
    std::atomic<int> bad{0};
    std::thread search([&]() {
      for (int r = 0; r < 6; ++r) {
        World W;
        fresh(W, n);
        // every round has its own objects: register them under their own addresses, search, forget them
        if (!(dropin(W, &lm) == want)) ++bad;
        for (MapPoint* p : W.local) lm.Erase(p);
      }
    });
    std::thread update([&]() {
      std::vector<MapPoint> other(base.points.begin() + (long)n, base.points.end());
      std::vector<MapPoint*> po;
      for (MapPoint& p : other) po.push_back(&p);
      for (int r = 0; r < 6; ++r) {
        if (!lm.Update(po)) ++bad;
        for (size_t i = r % 2; i < po.size(); i += 2) lm.Erase(po[i]);
        if (lm.Update(po[0]) < 0) ++bad;
      }
    });
    search.join();
    update.join();
    expect(bad.load() == 0, "searches next to updates");
    fresh(B, n);
    expect(dropin(B, &lm) == want, "after the threads");
  }
  if (failures) return 1;
  printf("LOCAL_MAP_SHIM_OK\n");
  return 0;
}
