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
#include <unordered_map>
#include <vector>

#include "../../include/rgbl_frontend.h"

namespace rgbl_shim {

class DeviceLocalMap {
 public:
  explicit DeviceLocalMap(int device = 0, int capacity = 4096) : mnCapacity(capacity < 1 ? 1 : capacity) {
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
  int mnNext = 0, mnCapacity, mnSearching = 0;
  rgbl_map_points* mpPool = nullptr;
};

}  // namespace rgbl_shim

#endif  // RGBL_SHIM_LOCALMAP_H
