// Stand-ins for ORB_SLAM3::KeyFrame / Frame / Map / ORBVocabulary, force-included (-include) in front of the reference's OWN
// src/KeyFrameDatabase.cc so that the file compiles unmodified where it lies (TEST INFRASTRUCTURE, tests/test_kfdb_reference.py).
// Defining the include guards of the real headers turns them into empty files; the plain classes below provide exactly the
// members KeyFrameDatabase.cc touches.  BowVector and L1Scoring are the reference's own vendored DBoW2.
#pragma once
#define KEYFRAME_H
#define FRAME_H
#define MAP_H
#define ORBVOCABULARY_H

#include <list>
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "Thirdparty/DBoW2/DBoW2/BowVector.h"
#include "Thirdparty/DBoW2/DBoW2/ScoringObject.h"

using namespace std;  // the reference's headers name vector / list / map unqualified
#define EIGEN_MAKE_ALIGNED_OPERATOR_NEW

namespace ORB_SLAM3 {

class Map {
 public:
  long unsigned int mnId = 0;
  bool bad = false;
  bool IsBad() { return bad; }
};

// include/ORBVocabulary.h: TemplatedVocabulary<FORB::TDescriptor, FORB>; score() forwards to the scoring object, which is
// L1Scoring for ORBvoc.txt (TemplatedVocabulary.h: m_scoring_object->score(v1, v2))
class ORBVocabulary {
 public:
  unsigned int n_words = 0;
  DBoW2::L1Scoring l1;
  unsigned int size() const { return n_words; }
  double score(const DBoW2::BowVector& a, const DBoW2::BowVector& b) const { return l1.score(a, b); }
};

class KeyFrame {
 public:
  long unsigned int mnId = 0;
  DBoW2::BowVector mBowVec;
  long unsigned int mnLoopQuery = 0, mnMergeQuery = 0, mnRelocQuery = 0, mnPlaceRecognitionQuery = 0;
  int mnLoopWords = 0, mnMergeWords = 0, mnRelocWords = 0, mnPlaceRecognitionWords = 0;
  float mLoopScore = 0, mMergeScore = 0, mRelocScore = 0, mPlaceRecognitionScore = 0;
  Map* map = nullptr;
  bool bad = false;
  std::vector<KeyFrame*> covisible;      // best first
  std::set<KeyFrame*> connected;
  Map* GetMap() { return map; }
  bool isBad() { return bad; }
  std::set<KeyFrame*> GetConnectedKeyFrames() { return connected; }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
    return (int)covisible.size() < N ? covisible : std::vector<KeyFrame*>(covisible.begin(), covisible.begin() + N);
  }
};

class Frame {
 public:
  long unsigned int mnId = 0;
  DBoW2::BowVector mBowVec;
};

}  // namespace ORB_SLAM3
