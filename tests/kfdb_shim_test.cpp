// kfdb_shim_test.cpp — the drop-in ORB_SLAM3::KeyFrameDatabase (orb_slam3_rgbl_amd/shim/KeyFrameDatabase.h) driven the way
// LoopClosing / Tracking / KeyFrame drive the reference's, on tiny stand-in KeyFrame / Frame / Map types of its own.
// It replays a script written by tests/test_kfdb_shim.py (key frames, adds, erases, clearMap, the two Detect* calls) and
// prints, per query, the candidates and the stamps the query left on the key-frame objects; the Python side compares them
// with the restatement of the reference (tests/kfdb_ref.py).
//   usage: kfdb_shim_test <script>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../orb_slam3_rgbl_amd/shim/KeyFrameDatabase.h"

namespace {

struct Map {
  bool bad = false;
  bool IsBad() { return bad; }
};

struct KeyFrame {
  long unsigned int mnId = 0;
  std::map<unsigned int, double> mBowVec;   // DBoW2::BowVector is a std::map<WordId, WordValue>
  long unsigned int mnRelocQuery = 0, mnPlaceRecognitionQuery = 0;
  int mnRelocWords = 0, mnPlaceRecognitionWords = 0;
  float mRelocScore = 0, mPlaceRecognitionScore = 0;
  Map* map = nullptr;
  bool bad = false;
  std::vector<KeyFrame*> covisible;
  std::set<KeyFrame*> connected;
  Map* GetMap() { return map; }
  bool isBad() { return bad; }
  std::set<KeyFrame*> GetConnectedKeyFrames() { return connected; }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
    return (int)covisible.size() < N ? covisible : std::vector<KeyFrame*>(covisible.begin(), covisible.begin() + N);
  }
};

struct Frame {
  long unsigned int mnId = 0;
  std::map<unsigned int, double> mBowVec;
};

struct Vocabulary {
  unsigned n = 0;
  unsigned size() const { return n; }
};

typedef ORB_SLAM3::KeyFrameDatabaseT<KeyFrame, Frame, Map> KeyFrameDatabase;

void read_bow(std::istream& in, std::map<unsigned int, double>& bow) {
  int n = 0;
  in >> n;
  std::vector<unsigned> id(n);
  for (int i = 0; i < n; ++i) in >> id[i];
  bow.clear();
  for (int i = 0; i < n; ++i) {
    std::string tok;
    in >> tok;
    bow[id[i]] = strtod(tok.c_str(), nullptr);   // hexadecimal floats: exact
  }
}

unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <script>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::map<long long, KeyFrame*> kfs;
  std::map<int, Map*> maps;
  auto map_of = [&](int id) { Map*& m = maps[id]; if (!m) m = new Map; return m; };
  KeyFrameDatabase* db = nullptr;
  std::string op;
  while (in >> op) {
    if (op == "V") {
      Vocabulary voc;
      in >> voc.n;
      db = new KeyFrameDatabase(voc);
      if (!db->Handle()) { fprintf(stderr, "no database handle\n"); return 1; }
    } else if (op == "K") {
      long long id; int m;
      in >> id >> m;
      KeyFrame*& kf = kfs[id];
      if (!kf) { kf = new KeyFrame; kf->mnId = (long unsigned int)id; }
      kf->map = map_of(m);
      read_bow(in, kf->mBowVec);
    } else if (op == "C") {
      long long id; int n;
      in >> id >> n;
      KeyFrame* kf = kfs.at(id);
      kf->covisible.clear();
      for (int i = 0; i < n; ++i) { long long o; in >> o; if (kfs.count(o)) kf->covisible.push_back(kfs[o]); }
    } else if (op == "A") {
      long long id; in >> id; db->add(kfs.at(id));
    } else if (op == "E") {
      long long id; in >> id; db->erase(kfs.at(id));
    } else if (op == "M") {
      int m; in >> m; db->clearMap(map_of(m));
    } else if (op == "U") {   // KeyFrame::UpdateMap: the object changes map, the database is not told
      long long id; int m;
      in >> id >> m;
      kfs.at(id)->map = map_of(m);
    } else if (op == "B") {
      int m; in >> m; map_of(m)->bad = true;
    } else if (op == "R") {
      long long fid; int m;
      in >> fid >> m;
      Frame F;
      F.mnId = (long unsigned int)fid;
      read_bow(in, F.mBowVec);
      std::vector<KeyFrame*> c = db->DetectRelocalizationCandidates(&F, map_of(m));
      printf("R %zu", c.size());
      for (KeyFrame* k : c) printf(" %lu", k->mnId);
      std::vector<KeyFrame*> st;
      for (auto& p : kfs) if (p.second->mnRelocQuery == F.mnId) st.push_back(p.second);
      printf(" %zu", st.size());
      for (KeyFrame* k : st) printf(" %lu %d %u", k->mnId, k->mnRelocWords, bits(k->mRelocScore));
      printf("\n");
    } else if (op == "O") {   // the candidates without covisibility lists and map filter: list order of the scored key frames
      long long fid;
      in >> fid;
      Frame F;
      F.mnId = (long unsigned int)fid;
      read_bow(in, F.mBowVec);
      Map one;
      std::map<KeyFrame*, std::pair<Map*, std::vector<KeyFrame*> > > saved;
      for (auto& p : kfs) {
        saved[p.second] = std::make_pair(p.second->map, p.second->covisible);
        p.second->map = &one;
        p.second->covisible.clear();
      }
      std::vector<KeyFrame*> c = db->DetectRelocalizationCandidates(&F, &one);
      for (auto& p : saved) { p.first->map = p.second.first; p.first->covisible = p.second.second; }
      printf("O %zu", c.size());
      for (KeyFrame* k : c) printf(" %lu", k->mnId);
      printf("\n");
    } else if (op == "N") {
      long long kid; int m, nconn, ncand;
      in >> kid >> m;
      KeyFrame K;
      K.mnId = (long unsigned int)kid;
      K.map = map_of(m);
      read_bow(in, K.mBowVec);
      in >> nconn;
      for (int i = 0; i < nconn; ++i) { long long o; in >> o; if (kfs.count(o)) K.connected.insert(kfs[o]); }
      in >> ncand;
      std::vector<KeyFrame*> vl, vm;
      db->DetectNBestCandidates(&K, vl, vm, ncand);
      printf("N %zu", vl.size());
      for (KeyFrame* k : vl) printf(" %lu", k->mnId);
      printf(" %zu", vm.size());
      for (KeyFrame* k : vm) printf(" %lu", k->mnId);
      std::vector<KeyFrame*> st;
      for (auto& p : kfs) if (p.second->mnPlaceRecognitionQuery == K.mnId) st.push_back(p.second);
      printf(" %zu", st.size());
      for (KeyFrame* k : st) printf(" %lu %d %u", k->mnId, k->mnPlaceRecognitionWords, bits(k->mPlaceRecognitionScore));
      printf("\n");
    } else {
      fprintf(stderr, "unknown op %s\n", op.c_str());
      return 2;
    }
  }
  delete db;
  printf("KFDB_SHIM_OK\n");
  return 0;
}
