// rgbl_shim::DeviceLocalMap - the map points of a map, resident on the device (rgbl_map_points, include/rgbl_frontend.h), for
// ORBmatcher::SearchLocalPoints (shim/ORBmatcher.h): what Frame::isInFrustum (src/Frame.cc:602-664) and
// ORBmatcher::SearchByProjection (src/ORBmatcher.cc:43-213) read from a MapPoint - GetWorldPos(), GetNormal(), mfMinDistance,
// mfMaxDistance, GetDescriptor() - is uploaded when it changes instead of once per tracked frame.
//
// Who calls what: Update(pMP) wherever the reference changes one of those members - the MapPoint
// constructors, SetWorldPos, UpdateNormalAndDepth, ComputeDistinctiveDescriptors (src/MapPoint.cc:81-90, 329-403, 431-486) -
// or, coarser, once per new key frame for the points LocalMapping touched; Erase(pMP) from MapPoint::SetBadFlag
// (src/MapPoint.cc:231-256).  Update reads the point through GetWorldPos / GetNormal / GetDescriptor, which take the MapPoint's
// own mutexes: call it AFTER the member that changed the point has released its lock (behind the closing brace of the
// unique_lock scope in SetWorldPos / UpdateNormalAndDepth), never inside it.  A point SearchLocalPoints meets without a slot is
// uploaded on the spot, so a missed Update of a NEW point costs time only; a missed Update of a CHANGED point leaves the old
// values in use.  A slot that Erase frees while a search is between reading its slots and finishing (BeginSearch /
// EndSearch, called by ORBmatcher::SearchLocalPoints) is not handed to another point before that search has ended, so a
// search never reads another point's data under an old MapPoint's slot.
// The class needs two accessors the reference's MapPoint does not have: the raw scale-invariance distances
//   float GetMinDistance() { unique_lock<mutex> lock(mMutexPos); return mfMinDistance; }      (and GetMaxDistance)
// because GetMinDistanceInvariance() returns 0.8f * mfMinDistance, from which the raw value cannot be recovered bit for bit,
// and MapPoint::PredictScale divides the raw mfMaxDistance.
// Thread-safe: LocalMapping updates while Tracking searches (the pool serialises device work; mMutex guards the slot table).
#ifndef RGBL_SHIM_LOCALMAP_H
#define RGBL_SHIM_LOCALMAP_H

#include <stdint.h>
#include <string.h>

#include <iostream>
#include <mutex>
#include <tuple>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/rgbl_frontend.h"

namespace rgbl_shim {

// A Frame / KeyFrame class with a member `rgbl_device_frame* mpDeviceFrame` (one line in Frame.h / KeyFrame.h,
// filled by ORBextractor::CaptureDeviceFrame in the Frame constructor) is matched from its resident copy: descriptors,
// mvKeysUn and mvuRight are not uploaded again.  Classes without the member behave as before.
template <class T> auto device_frame_of(const T& f, int) -> decltype(static_cast<const rgbl_device_frame*>(f.mpDeviceFrame)) { return f.mpDeviceFrame; }
template <class T> const rgbl_device_frame* device_frame_of(const T&, long) { return nullptr; }

class DeviceLocalMap {
 public:
  explicit DeviceLocalMap(int device = 0, int capacity = 4096) : mnDevice(device), mnCapacity(capacity < 1 ? 1 : capacity) {
    if (rgbl_map_points_create(device, mnCapacity, &mpPool) != RGBL_OK) {
      std::cerr << "[DeviceLocalMap] " << rgbl_last_error() << std::endl;
      mpPool = nullptr;
    }
  }
  ~DeviceLocalMap() { rgbl_map_points_destroy(mpPool); }
  DeviceLocalMap(const DeviceLocalMap&) = delete;
  DeviceLocalMap& operator=(const DeviceLocalMap&) = delete;

  rgbl_map_points* handle() const { return mpPool; }
  size_t size() {
    std::lock_guard<std::mutex> lock(mMutex);
    return mSlot.size();
  }
  // the point's slot, -1 when it has none
  int SlotOf(const void* pMP) {
    std::lock_guard<std::mutex> lock(mMutex);
    auto it = mSlot.find(pMP);
    return it == mSlot.end() ? -1 : it->second;
  }
  // uploads the point's present values (into a new slot when it has none); returns the slot, -1 on error
  template <class MapPointT> int Update(MapPointT* pMP) {
    std::vector<MapPointT*> one(1, pMP);
    std::vector<int32_t> slot;
    return Update(one, &slot) ? slot[0] : -1;
  }
  // the same for many points with one upload
  template <class MapPointT> bool Update(const std::vector<MapPointT*>& vpMPs, std::vector<int32_t>* pSlots = nullptr) {
    const size_t n = vpMPs.size();
    std::vector<int32_t> slot(n);
    std::vector<float> pos(3 * n), normal(3 * n), dmin(n), dmax(n);
    std::vector<uint8_t> desc(32 * n);
    if (!mpPool) return false;
    // the MapPoints' own mutexes are taken here, before mMutex: no lock of this class is held while theirs are
    for (size_t i = 0; i < n; ++i) {
      const auto P = vpMPs[i]->GetWorldPos();
      const auto Pn = vpMPs[i]->GetNormal();
      for (int k = 0; k < 3; ++k) { pos[3 * i + k] = P(k); normal[3 * i + k] = Pn(k); }
      dmin[i] = vpMPs[i]->GetMinDistance();
      dmax[i] = vpMPs[i]->GetMaxDistance();
      const auto d = vpMPs[i]->GetDescriptor();
      memcpy(&desc[32 * i], d.template ptr<uint8_t>(), 32);
    }
    // held until the values are on the device: a search that finds the slot finds the point
    std::lock_guard<std::mutex> lock(mMutex);
    std::vector<const void*> added;
    bool ok = true;
    for (size_t i = 0; i < n && ok; ++i) {
      auto it = mSlot.find(vpMPs[i]);
      if (it != mSlot.end()) { slot[i] = it->second; continue; }
      if (!mFree.empty()) { slot[i] = mFree.back(); mFree.pop_back(); }
      else {
        if (mnNext == mnCapacity) {   // growth: doubling, the contents stay
          if (rgbl_map_points_reserve(mpPool, 2 * mnCapacity) != RGBL_OK) { ok = false; break; }
          mnCapacity *= 2;
        }
        slot[i] = mnNext++;
      }
      mSlot[vpMPs[i]] = slot[i];
      added.push_back(vpMPs[i]);
    }
    if (ok) ok = rgbl_map_points_update(mpPool, (int)n, slot.data(), pos.data(), normal.data(), dmin.data(), dmax.data(), desc.data()) == RGBL_OK;
    if (!ok) {
      std::cerr << "[DeviceLocalMap] " << rgbl_last_error() << std::endl;
      for (const void* p : added) {   // no point stays registered on a slot that does not hold it
        auto it = mSlot.find(p);
        mFree.push_back(it->second);
        mSlot.erase(it);
      }
      return false;
    }
    if (pSlots) pSlots->swap(slot);
    return true;
  }
  // MapPoint::UpdateNormalAndDepth (`normal`) and / or MapPoint::ComputeDistinctiveDescriptors (`descriptor`) for many points
  // with ONE device call (rgbl_map_points_refresh): the observations go up as (key frame, feature) pairs, the descriptors
  // are read from the key frames' resident copies (KeyFrame::mpDeviceFrame), the slots take the results and
  // the MapPoint objects get them back through SetNormalVector / SetMinMaxDistance / SetDescriptor.  The
  // slots also take the points' present GetWorldPos() (SetWorldPos after bundle adjustment needs no Update of its own).
  // Bad points are skipped, as the two functions return at once for them.  A point that cannot go this way - a key frame
  // among its observers without a resident copy, an observation with a right index and, when `normal` is asked for, a
  // reference key frame without a resident copy or with another scale table than the call's - gets the MapPoint's own
  // UpdateNormalAndDepth() / ComputeDistinctiveDescriptors() on the host and is uploaded with Update: no listed point is
  // left stale, whichever way it went.
  // Locks as for Update: the MapPoints' and KeyFrames' own mutexes are taken (by their accessors) and released before
  // mMutex, mMutex is held until the device call has returned, and the setters run after it has been released.  Call it
  // where the reference calls the two functions, outside the MapPoint's own locks.  *pnOnDevice: points that went the device way.
  template <class MapPointT> bool Refresh(const std::vector<MapPointT*>& vpMPs, bool normal, bool descriptor, int* pnOnDevice = nullptr) {
    if (pnOnDevice) *pnOnDevice = 0;
    if (!mpPool) return false;
    if (!normal && !descriptor) return true;
    std::vector<MapPointT*> device, host, unregistered;
    std::vector<float> pos, center, scale;
    std::vector<int32_t> off(1, 0), obsKF, obsFeat, refKF, refLevel;
    std::vector<const rgbl_device_frame*> frame;
    std::vector<uint8_t> bad;
    std::unordered_map<const void*, int32_t> table;   // key frame -> index
    int nLevels = 0;
    auto index_of = [&](auto* pKF) -> int32_t {   // -1: no resident copy
      auto it = table.find(pKF);
      if (it != table.end()) return it->second;
      const rgbl_device_frame* f = device_frame_of(*pKF, 0);
      int32_t k = -1;
      if (f) {
        k = (int32_t)frame.size();
        frame.push_back(f);
        const auto Ow = pKF->GetCameraCenter();
        for (int c = 0; c < 3; ++c) center.push_back(Ow(c));
        bad.push_back(pKF->isBad() ? 1 : 0);
      }
      table[pKF] = k;
      return k;
    };
    std::unordered_set<const void*> listed;
    for (MapPointT* pMP : vpMPs) {
      if (!listed.insert(pMP).second) continue;                // a point listed twice is refreshed once
      if (pMP->isBad()) continue;                              // MapPoint.cc:338, 434
      auto observations = pMP->GetObservations();              // :340, 436
      auto* pRefKF = pMP->GetReferenceKeyFrame();              // :437
      const auto Pos = pMP->GetWorldPos();                     // :438
      if (observations.empty()) continue;                      // :343, 441
      const size_t mark = obsKF.size();
      bool ok = !normal || pRefKF != nullptr;
      for (auto mit = observations.begin(); ok && mit != observations.end(); ++mit) {
        const int leftIndex = std::get<0>(mit->second), rightIndex = std::get<1>(mit->second);
        const int32_t k = (leftIndex == -1 || rightIndex != -1) ? -1 : index_of(mit->first);
        ok = k >= 0;
        obsKF.push_back(k);
        obsFeat.push_back(leftIndex);
      }
      int32_t kRef = 0, level = 0;
      if (ok && normal) {
        kRef = index_of(pRefKF);
        // :471-475 observations[pRefKF] inserts (0, 0) for a reference key frame that does not observe the point
        auto it = observations.find(pRefKF);
        const int leftIndex = it == observations.end() ? 0 : std::get<0>(it->second);
        ok = kRef >= 0 && pRefKF->NLeft == -1 && leftIndex >= 0 && leftIndex < (int)pRefKF->mvKeysUn.size();
        if (ok) level = pRefKF->mvKeysUn[leftIndex].octave;
      }
      if (ok && normal) {   // one scale table per call: the first point's
        const std::vector<float>& sf = pRefKF->mvScaleFactors;
        if (scale.empty()) { scale = sf; nLevels = pRefKF->mnScaleLevels; }
        ok = nLevels == pRefKF->mnScaleLevels && sf.size() == scale.size() && memcmp(sf.data(), scale.data(), sizeof(float) * sf.size()) == 0 &&
             nLevels >= 1 && nLevels <= (int)sf.size() && level >= 0 && level < nLevels;
      }
      if (!ok) {
        obsKF.resize(mark); obsFeat.resize(mark);
        host.push_back(pMP);
        continue;
      }
      device.push_back(pMP);
      for (int c = 0; c < 3; ++c) pos.push_back(Pos(c));
      off.push_back((int32_t)obsKF.size());
      refKF.push_back(kRef);
      refLevel.push_back(level);
    }
    for (MapPointT* pMP : host) {   // the reference's own functions, as before this class
      if (normal) pMP->UpdateNormalAndDepth();
      if (descriptor) pMP->ComputeDistinctiveDescriptors();
    }
    bool ok = host.empty() || Update(host);
    const size_t n = device.size();
    if (n == 0) return ok;
    for (MapPointT* pMP : device)
      if (SlotOf(pMP) < 0) unregistered.push_back(pMP);
    if (!unregistered.empty() && !Update(unregistered)) return false;   // a new slot starts from the point's present values
    std::vector<int32_t> slot(n);
    std::vector<float> outNormal(3 * n), outMin(n), outMax(n);
    std::vector<uint8_t> outDesc(32 * n), status(n, 0);
    {
      std::lock_guard<std::mutex> lock(mMutex);   // held until the call has returned: no slot below is erased and re-used meanwhile
      for (size_t i = 0; i < n; ++i) {
        auto it = mSlot.find(device[i]);
        if (it == mSlot.end()) { std::cerr << "[DeviceLocalMap] a point was erased during Refresh" << std::endl; return false; }
        slot[i] = it->second;
      }
      rgbl_map_refresh_input in{};
      in.n_points = (int)n; in.slot = slot.data(); in.world_pos = pos.data();
      in.obs_off = off.data(); in.obs_kf = obsKF.data(); in.obs_feat = obsFeat.data();
      in.ref_kf = refKF.data(); in.ref_level = refLevel.data();
      in.n_kfs = (int)frame.size(); in.kf_frame = frame.data(); in.kf_center = center.data(); in.kf_bad = bad.data();
      in.scale_factors = scale.data(); in.n_levels = nLevels;
      in.do_normal = normal; in.do_descriptor = descriptor;
      rgbl_map_refresh_output out{};
      out.normal = outNormal.data(); out.min_dist = outMin.data(); out.max_dist = outMax.data();
      out.desc = outDesc.data(); out.status = status.data();
      rgbl_matcher* handle = nullptr;
      int rc = rgbl_matcher_acquire(mnDevice, &handle);
      if (rc == RGBL_OK) {
        rc = rgbl_map_points_refresh(handle, mpPool, &in, &out);
        rgbl_matcher_release(handle);
      }
      if (rc != RGBL_OK) {
        std::cerr << "[DeviceLocalMap] " << rgbl_last_error() << std::endl;
        return false;
      }
    }
    // the MapPoint objects stay in step (their setters take the MapPoint's own mutexes: no lock of this class is held)
    for (size_t i = 0; i < n; ++i) {
      if (status[i] & 1) {
        auto nv = device[i]->GetNormal();
        for (int c = 0; c < 3; ++c) nv(c) = outNormal[3 * i + c];
        device[i]->SetNormalVector(nv);                                  // MapPoint.cc:492
        device[i]->SetMinMaxDistance(outMin[i], outMax[i]);              // :490-491
      }
      if (status[i] & 2) {
        auto d = device[i]->GetDescriptor();
        if (d.rows != 1 || d.cols != 32) d.create(1, 32, 0 /* CV_8U */);
        memcpy(d.template ptr<uint8_t>(), &outDesc[32 * i], 32);
        device[i]->SetDescriptor(d);                                     // :401
      }
    }
    if (pnOnDevice) *pnOnDevice = (int)n;
    return ok;
  }
  // the point's slot becomes free for the next new point (MapPoint::SetBadFlag); a point without a slot: nothing happens
  void Erase(const void* pMP) {
    std::lock_guard<std::mutex> lock(mMutex);
    auto it = mSlot.find(pMP);
    if (it == mSlot.end()) return;
    (mnSearching > 0 ? mPending : mFree).push_back(it->second);   // a running search may still read this slot as pMP's
    mSlot.erase(it);
  }
  // Brackets of a search: from before its first SlotOf() until its device call has returned.  Slots erased in between are
  // kept out of reuse until no search is running.
  void BeginSearch() {
    std::lock_guard<std::mutex> lock(mMutex);
    ++mnSearching;
  }
  void EndSearch() {
    std::lock_guard<std::mutex> lock(mMutex);
    if (--mnSearching == 0) {
      mFree.insert(mFree.end(), mPending.begin(), mPending.end());
      mPending.clear();
    }
  }

 private:
  std::mutex mMutex;
  std::unordered_map<const void*, int32_t> mSlot;
  std::vector<int32_t> mFree, mPending;   // mPending: erased while a search was running
  int mnDevice;
  int mnNext = 0, mnCapacity, mnSearching = 0;
  rgbl_map_points* mpPool = nullptr;
};

}  // namespace rgbl_shim

#endif  // RGBL_SHIM_LOCALMAP_H
