// kfdb_ref_glue.cpp — C entry points around the reference's OWN src/KeyFrameDatabase.cc (compiled unmodified where it lies,
// behind the stand-ins of tests/kfdb_ref_types.h) and its vendored DBoW2 BowVector / L1Scoring.  TEST INFRASTRUCTURE: built
// into the git-ignored tests/_build by tests/test_kfdb_reference.py and tools/kfdb_bench.py where the reference is present.
#include <chrono>
#include <map>
#include <vector>

#include "KeyFrameDatabase.h"

using namespace ORB_SLAM3;

struct RefDb {
  ORBVocabulary voc;
  KeyFrameDatabase* db = nullptr;
  std::map<long long, KeyFrame*> kfs;      // every key frame ever made (erased ones keep their object, as in the reference)
  std::map<int, Map*> maps;
  double seconds = 0;
  Map* map(int id) {
    Map*& m = maps[id];
    if (!m) { m = new Map; m->mnId = id; }
    return m;
  }
};

static void fill(DBoW2::BowVector& v, int n, const unsigned* id, const double* val) {
  for (int i = 0; i < n; ++i) v.insert(v.end(), std::make_pair(id[i], val[i]));
}

extern "C" {

void* ref_kfdb_create(int n_vocab) {
  RefDb* r = new RefDb;
  r->voc.n_words = n_vocab;
  r->db = new KeyFrameDatabase(r->voc);
  return r;
}
void ref_kfdb_destroy(void* h) {
  RefDb* r = static_cast<RefDb*>(h);
  delete r->db;
  for (auto& p : r->kfs) delete p.second;
  for (auto& p : r->maps) delete p.second;
  delete r;
}
// a key frame that was erased and comes back is a new object in the lists' eyes only through its position: the reference
// re-adds the same object, so do we
void ref_kfdb_add(void* h, long long kf_id, int map_id, int n, const unsigned* id, const double* val) {
  RefDb* r = static_cast<RefDb*>(h);
  KeyFrame*& kf = r->kfs[kf_id];
  if (!kf) { kf = new KeyFrame; kf->mnId = kf_id; }
  kf->map = r->map(map_id);
  kf->mBowVec.clear();
  fill(kf->mBowVec, n, id, val);
  r->db->add(kf);
}
void ref_kfdb_erase(void* h, long long kf_id) {
  RefDb* r = static_cast<RefDb*>(h);
  auto it = r->kfs.find(kf_id);
  if (it != r->kfs.end()) r->db->erase(it->second);
}
void ref_kfdb_clear_map(void* h, int map_id) { RefDb* r = static_cast<RefDb*>(h); r->db->clearMap(r->map(map_id)); }
// KeyFrame::UpdateMap
void ref_kfdb_set_map(void* h, long long kf_id, int map_id) {
  RefDb* r = static_cast<RefDb*>(h);
  auto it = r->kfs.find(kf_id);
  if (it != r->kfs.end()) it->second->map = r->map(map_id);
}
void ref_kfdb_clear(void* h) { static_cast<RefDb*>(h)->db->clear(); }
void ref_kfdb_set_covisible(void* h, long long kf_id, int n, const long long* ids) {
  RefDb* r = static_cast<RefDb*>(h);
  KeyFrame* kf = r->kfs.at(kf_id);
  kf->covisible.clear();
  for (int i = 0; i < n; ++i) { auto it = r->kfs.find(ids[i]); if (it != r->kfs.end()) kf->covisible.push_back(it->second); }
}
void ref_kfdb_set_map_bad(void* h, int map_id, int bad) { static_cast<RefDb*>(h)->map(map_id)->bad = bad != 0; }

// DetectRelocalizationCandidates(F, pMap); returns the number of candidates (at most cap are written)
int ref_kfdb_reloc(void* h, long long frame_id, int n, const unsigned* id, const double* val, int map_id, long long* out, int cap) {
  RefDb* r = static_cast<RefDb*>(h);
  Frame F;
  F.mnId = frame_id;
  fill(F.mBowVec, n, id, val);
  Map* m = r->map(map_id);
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<KeyFrame*> c = r->db->DetectRelocalizationCandidates(&F, m);
  r->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  for (int i = 0; i < (int)c.size() && i < cap; ++i) out[i] = (long long)c[i]->mnId;
  return (int)c.size();
}
// The order of lKFsSharingWords as far as the function itself shows it: with every key frame in the query's map and no
// covisibility lists, DetectRelocalizationCandidates returns the scored key frames above 0.75 x the best score in list order.
int ref_kfdb_reloc_order(void* h, long long frame_id, int n, const unsigned* id, const double* val, long long* out, int cap) {
  RefDb* r = static_cast<RefDb*>(h);
  std::map<KeyFrame*, std::pair<Map*, std::vector<KeyFrame*> > > saved;
  Map one;
  for (auto& p : r->kfs) {
    saved[p.second] = std::make_pair(p.second->map, p.second->covisible);
    p.second->map = &one;
    p.second->covisible.clear();
  }
  Frame F;
  F.mnId = frame_id;
  fill(F.mBowVec, n, id, val);
  std::vector<KeyFrame*> c = r->db->DetectRelocalizationCandidates(&F, &one);
  for (auto& p : saved) { p.first->map = p.second.first; p.first->covisible = p.second.second; }
  for (int i = 0; i < (int)c.size() && i < cap; ++i) out[i] = (long long)c[i]->mnId;
  return (int)c.size();
}
double ref_kfdb_last_call_seconds(void* h) { return static_cast<RefDb*>(h)->seconds; }

// DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates) for a query key frame that is not in the database
void ref_kfdb_nbest(void* h, long long kf_id, int n, const unsigned* id, const double* val, int map_id, int n_conn,
                    const long long* conn, int n_cand, long long* loop, int* n_loop, long long* merge, int* n_merge) {
  RefDb* r = static_cast<RefDb*>(h);
  KeyFrame K;
  K.mnId = kf_id;
  K.map = r->map(map_id);
  fill(K.mBowVec, n, id, val);
  for (int i = 0; i < n_conn; ++i) { auto it = r->kfs.find(conn[i]); if (it != r->kfs.end()) K.connected.insert(it->second); }
  std::vector<KeyFrame*> vl, vm;
  r->db->DetectNBestCandidates(&K, vl, vm, n_cand);
  *n_loop = (int)vl.size();
  *n_merge = (int)vm.size();
  for (size_t i = 0; i < vl.size(); ++i) loop[i] = (long long)vl[i]->mnId;
  for (size_t i = 0; i < vm.size(); ++i) merge[i] = (long long)vm[i]->mnId;
}

// the stamps a query left on the key frames: which = 0 reloc, 1 place recognition; one row per key frame id asked for
void ref_kfdb_stamps(void* h, int which, int n, const long long* kf_id, long long* query, int* words, float* score) {
  RefDb* r = static_cast<RefDb*>(h);
  for (int i = 0; i < n; ++i) {
    KeyFrame* kf = r->kfs.at(kf_id[i]);
    query[i] = (long long)(which ? kf->mnPlaceRecognitionQuery : kf->mnRelocQuery);
    words[i] = which ? kf->mnPlaceRecognitionWords : kf->mnRelocWords;
    score[i] = which ? kf->mPlaceRecognitionScore : kf->mRelocScore;
  }
}

}  // extern "C"
