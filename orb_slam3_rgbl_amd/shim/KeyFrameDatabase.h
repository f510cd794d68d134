// Drop-in replacement of the live part of /root/reference/include/KeyFrameDatabase.h on librgbl_frontend.so:
//   KeyFrameDatabase(voc)                                              (KeyFrameDatabase.cc:32-36)
//   add(pKF) / erase(pKF) / clear() / clearMap(pMap)                   (:39-98)
//   DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates) (:604-730; LoopClosing.cc:491)
//   DetectRelocalizationCandidates(F, pMap)                            (:733-845; Tracking.cc:3651)
// DetectLoopCandidates, DetectCandidates and DetectBestCandidates have no caller in the reference and are not provided.
//
// The stored BowVectors live on the device (rgbl_kfdb_*): the words shared with every stored key frame, maxCommonWords,
// minCommonWords and the L1 scores come from there, in the reference's order and bit for bit.  What touches the caller's
// objects stays here: the stamps mnRelocQuery / mnRelocWords / mRelocScore and
// mnPlaceRecognitionQuery / mnPlaceRecognitionWords / mPlaceRecognitionScore, the covisibility accumulation over
// GetBestCovisibilityKeyFrames(10) in `float`, and the selection by GetMap() / isBad().
//
// The class is a template over the key-frame, frame and map types so that this file needs none of KeyFrame.h / Frame.h /
// Map.h; in the ORB_SLAM3 tree one line names the instance:
//   typedef KeyFrameDatabaseT<KeyFrame, Frame, Map> KeyFrameDatabase;
// It uses the members the reference functions themselves touch: mnId, mBowVec, GetMap(), GetConnectedKeyFrames(),
// GetBestCovisibilityKeyFrames(N), isBad(), Map::IsBad() and the six stamps.
//
// Two differences from the reference, both documented in INTEGRATION.md:
//   - DetectNBestCandidates steps over a bad key frame in the sorted list.  The reference's `if(pKFi->isBad()) continue;`
//     (:712) advances neither `i` nor `it` and would spin; it is unreachable there because KeyFrame::SetBadFlag erases a
//     key frame from the database (KeyFrame.cc:678) before it is marked bad.
//   - a key frame that is in the database is not added a second time (the reference would count its words twice).
// clearMap goes by the key frames' GetMap() at the time of the call, as the reference does.
#ifndef RGBL_KEYFRAMEDATABASE_H
#define RGBL_KEYFRAMEDATABASE_H

#include <stdint.h>

#include <algorithm>
#include <iostream>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "../../include/rgbl_frontend.h"

namespace ORB_SLAM3 {

template <class KeyFrameT, class FrameT, class MapT>
class KeyFrameDatabaseT {
 public:
  // voc: anything with size() = the number of words (ORBVocabulary, DeviceORBVocabulary)
  template <class VocT>
  explicit KeyFrameDatabaseT(const VocT& voc, int device = 0) { Create((int)voc.size(), device); }
  explicit KeyFrameDatabaseT(int nWords, int device = 0) { Create(nWords, device); }
  ~KeyFrameDatabaseT() { rgbl_kfdb_destroy(mpHandle); }
  KeyFrameDatabaseT(const KeyFrameDatabaseT&) = delete;
  KeyFrameDatabaseT& operator=(const KeyFrameDatabaseT&) = delete;

  void add(KeyFrameT* pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    std::vector<uint32_t> id;
    std::vector<double> val;
    Flatten(pKF->mBowVec, id, val);
    // the device's map id is not used: a key frame's map can change after add() (LoopClosing's UpdateMap), so clearMap
    // below asks the objects themselves
    if (rgbl_kfdb_add(mpHandle, (int64_t)pKF->mnId, 0, (int)id.size(), id.data(), val.data()) != RGBL_OK) {
      std::cerr << "[KeyFrameDatabase] " << rgbl_last_error() << std::endl;
      return;
    }
    mKeyFrames[(int64_t)pKF->mnId] = pKF;
  }

  void erase(KeyFrameT* pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    typename KeyFrameMap::iterator it = mKeyFrames.find((int64_t)pKF->mnId);
    if (it == mKeyFrames.end() || it->second != pKF) return;
    rgbl_kfdb_erase(mpHandle, it->first);
    mKeyFrames.erase(it);
  }

  void clear() {
    std::unique_lock<std::mutex> lock(mMutex);
    rgbl_kfdb_clear(mpHandle);
    mKeyFrames.clear();
  }

  // Every stored key frame whose GetMap() is pMap NOW leaves (KeyFrameDatabase.cc:87 tests the map at clear time, not at add).
  void clearMap(MapT* pMap) {
    std::unique_lock<std::mutex> lock(mMutex);
    for (typename KeyFrameMap::iterator it = mKeyFrames.begin(); it != mKeyFrames.end();) {
      if (it->second->GetMap() == pMap) {
        rgbl_kfdb_erase(mpHandle, it->first);
        it = mKeyFrames.erase(it);
      } else {
        ++it;
      }
    }
  }

  void DetectNBestCandidates(KeyFrameT* pKF, std::vector<KeyFrameT*>& vpLoopCand, std::vector<KeyFrameT*>& vpMergeCand, int nNumCandidates) {
    std::vector<int64_t> connected;
    const std::set<KeyFrameT*> conn = pKF->GetConnectedKeyFrames();
    for (KeyFrameT* c : conn) connected.push_back((int64_t)c->mnId);
    std::vector<Group> groups = Groups<PlaceStamps>(pKF->mBowVec, connected, pKF->mnId);
    // best accumulated score first; equal scores keep their order, as a stable list sort by `first >` does
    std::stable_sort(groups.begin(), groups.end(), [](const Group& a, const Group& b) { return a.acc > b.acc; });
    const size_t want = (size_t)(nNumCandidates > 0 ? nNumCandidates : 0);
    std::set<KeyFrameT*> taken;
    for (size_t g = 0; g < groups.size() && (vpLoopCand.size() < want || vpMergeCand.size() < want); ++g) {
      KeyFrameT* kf = groups[g].best;
      if (kf->isBad() || !taken.insert(kf).second) continue;   // a bad key frame is stepped over (head of this file)
      const bool same_map = pKF->GetMap() == kf->GetMap();
      if (same_map && vpLoopCand.size() < want) vpLoopCand.push_back(kf);
      else if (!same_map && vpMergeCand.size() < want && !kf->GetMap()->IsBad()) vpMergeCand.push_back(kf);
    }
  }

  std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F, MapT* pMap) {
    const std::vector<Group> groups = Groups<RelocStamps>(F->mBowVec, std::vector<int64_t>(), F->mnId);
    float top = 0.f;
    for (const Group& g : groups) top = g.acc > top ? g.acc : top;
    const float keep_above = 0.75f * top;
    std::vector<KeyFrameT*> out;
    std::set<KeyFrameT*> taken;
    for (const Group& g : groups)
      if (g.acc > keep_above && g.best->GetMap() == pMap && taken.insert(g.best).second) out.push_back(g.best);
    return out;
  }

  rgbl_kf_database* Handle() const { return mpHandle; }

 protected:
  typedef std::map<int64_t, KeyFrameT*> KeyFrameMap;
  // which trio of members a query stamps
  struct RelocStamps {
    static auto& query(KeyFrameT* k) { return k->mnRelocQuery; }
    static auto& words(KeyFrameT* k) { return k->mnRelocWords; }
    static auto& score(KeyFrameT* k) { return k->mRelocScore; }
  };
  struct PlaceStamps {
    static auto& query(KeyFrameT* k) { return k->mnPlaceRecognitionQuery; }
    static auto& words(KeyFrameT* k) { return k->mnPlaceRecognitionWords; }
    static auto& score(KeyFrameT* k) { return k->mPlaceRecognitionScore; }
  };
  // a scored key frame with its covisible neighbours: the summed score and the best-scoring member
  struct Group { float acc; KeyFrameT* best; };

  void Create(int nWords, int device) {
    if (rgbl_kfdb_create(device, nWords, &mpHandle) != RGBL_OK) {
      std::cerr << "[KeyFrameDatabase] " << rgbl_last_error() << std::endl;
      mpHandle = nullptr;
    }
  }

  template <class BowVectorT>
  static void Flatten(const BowVectorT& v, std::vector<uint32_t>& id, std::vector<double>& val) {
    id.reserve(v.size());
    val.reserve(v.size());
    for (typename BowVectorT::const_iterator it = v.begin(); it != v.end(); ++it) {
      id.push_back((uint32_t)it->first);
      val.push_back((double)it->second);
    }
  }

  // The device query, the stamps on every sharing key frame, then one Group per scored key frame in the query's order:
  // its score plus the scores of those of its 10 best covisible key frames that this query stamped, in float.
  template <class Stamps, class BowVectorT, class IdT>
  std::vector<Group> Groups(const BowVectorT& bow, const std::vector<int64_t>& excluded, IdT queryId) {
    std::vector<KeyFrameT*> scoredKFs;
    {
      std::unique_lock<std::mutex> lock(mMutex);
      std::vector<uint32_t> id;
      std::vector<double> val;
      Flatten(bow, id, val);
      int cap = 0;
      rgbl_kfdb_size(mpHandle, &cap, nullptr);
      const size_t room = cap > 0 ? (size_t)cap : 1;
      std::vector<int64_t> kf(room);
      std::vector<int32_t> words(room);
      std::vector<float> score(room);
      std::vector<uint8_t> scored(room);
      rgbl_kfdb_query_input in;
      in.n_words = (int)id.size(); in.word_id = id.data(); in.word_val = val.data();
      in.n_excluded = (int)excluded.size(); in.excluded_kf = excluded.empty() ? nullptr : excluded.data();
      in.min_words_floor = 0;
      rgbl_kfdb_query_output out;
      out.cap = cap; out.share_kf = kf.data(); out.share_words = words.data(); out.share_score = score.data(); out.scored = scored.data();
      out.n_share = out.max_common_words = out.min_common_words = 0;
      if (rgbl_kfdb_query(mpHandle, &in, &out) != RGBL_OK) {
        std::cerr << "[KeyFrameDatabase] " << rgbl_last_error() << std::endl;
        return std::vector<Group>();
      }
      for (int i = 0; i < out.n_share; ++i) {
        typename KeyFrameMap::iterator it = mKeyFrames.find(kf[i]);
        if (it == mKeyFrames.end()) continue;   // cannot happen: both sides change together under mMutex
        KeyFrameT* k = it->second;
        Stamps::query(k) = queryId;
        Stamps::words(k) = words[i];
        if (scored[i]) {
          Stamps::score(k) = score[i];
          scoredKFs.push_back(k);
        }
      }
    }
    std::vector<Group> groups;
    groups.reserve(scoredKFs.size());
    for (KeyFrameT* k : scoredKFs) {
      Group g = {Stamps::score(k), k};
      float best = g.acc;
      const std::vector<KeyFrameT*> neighbours = k->GetBestCovisibilityKeyFrames(10);
      for (KeyFrameT* n : neighbours) {
        if (Stamps::query(n) != queryId) continue;
        const float s = Stamps::score(n);
        g.acc += s;
        if (s > best) { best = s; g.best = n; }
      }
      groups.push_back(g);
    }
    return groups;
  }

  rgbl_kf_database* mpHandle = nullptr;
  KeyFrameMap mKeyFrames;   // mnId -> the caller's object, for the key frames in the database
  std::mutex mMutex;
};

}  // namespace ORB_SLAM3

#endif  // RGBL_KEYFRAMEDATABASE_H
