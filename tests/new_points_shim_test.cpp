// The C++ drop-in rgbl_shim::CreateNewMapPoints (orb_slam3_rgbl_amd/shim/NewMapPoints.h) on stand-in KeyFrame types, held to a
// host transcription of the loop of LocalMapping.cc:434-711 on the same types: per neighbour the baseline test, the drop-in
// ORBmatcher::SearchForTriangulation, the per-match block (the library's host build of csrc/newpoint_math.h) and AddMapPoint.
// The transcription's records, F12 and epipoles are dumped for tests/test_new_points_shim.py, which holds them to the
// restatement with the oracle's search.  TEST INFRASTRUCTURE.
//   new_points_shim_test <case.bin> <out.bin>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../orb_slam3_rgbl_amd/shim/NewMapPoints.h"
#include "shim_standins.h"

struct KeyFrameNP : KeyFrame {
  std::vector<float> mvDepth;
  float mb = 0, mbf = 0, mfScaleFactor = 1.2f;
  rgbl_device_frame* own = nullptr;
};

static bool load(FILE* f, KeyFrameNP& kf, Camera* cam, MapPoint* some, float mb, float mbf, bool resident) {
  if (!load_kf(f, kf, cam, some)) return false;
  kf.mvDepth.resize(kf.N); kf.mvKeys.resize(kf.N);
  std::vector<float> raw(2 * (size_t)kf.N);
  rd(f, kf.mvDepth.data(), kf.N); rd(f, raw.data(), raw.size());
  for (int i = 0; i < kf.N; ++i) { kf.mvKeys[i] = kf.mvKeysUn[i]; kf.mvKeys[i].pt.x = raw[2 * i]; kf.mvKeys[i].pt.y = raw[2 * i + 1]; }
  kf.mb = mb; kf.mbf = mbf;
  if (resident) {
    std::vector<float> xy(2 * (size_t)kf.N); std::vector<int32_t> oct(kf.N), off(1, 0), feat;
    for (int i = 0; i < kf.N; ++i) { xy[2 * i] = kf.mvKeysUn[i].pt.x; xy[2 * i + 1] = kf.mvKeysUn[i].pt.y; oct[i] = kf.mvKeysUn[i].octave; }
    for (auto& e : kf.mFeatVec) { for (unsigned v : e.second) feat.push_back((int32_t)v); off.push_back((int32_t)feat.size()); }
    if (rgbl_device_frame_create(0, kf.N > 0 ? kf.N : 1, &kf.own) != RGBL_OK) return false;
    if (rgbl_device_frame_upload(kf.own, kf.N, kf.mDescriptors.data, xy.data(), oct.data(), kf.mvuRight.data()) != RGBL_OK) return false;
    if (rgbl_device_frame_set_feature_vector(kf.own, (int)off.size() - 1, off.data(), feat.data()) != RGBL_OK) return false;
    kf.mpDeviceFrame = kf.own;
  }
  return true;
}

// one run of drop-in and transcription on freshly loaded key frames; returns the number of failures, -1: cannot run
static int run(FILE* f, long start, int nn, const float* hdr, int far_points, Camera* cam, MapPoint* some, const std::vector<unsigned char>& skip,
               bool resident, bool mono, bool inertial, bool with_skip, std::vector<rgbl_new_point>& want, std::vector<int>& want_per,
               std::vector<float>& geometry) {
  fseek(f, start, SEEK_SET);
  KeyFrameNP kf1;
  std::vector<KeyFrameNP> kfs((size_t)nn);
  if (!load(f, kf1, cam, some, hdr[4], hdr[5], resident)) return -1;
  for (auto& k : kfs) if (!load(f, k, cam, some, hdr[4], hdr[5], resident)) return -1;
  std::vector<KeyFrameNP*> neigh;
  for (auto& k : kfs) neigh.push_back(&k);
  int failures = 0;
  {
    ORB_SLAM3::ORBmatcher matcher(0.6f, false);
    const int idle = rgbl_matcher_pool_size();
    // the drop-in
    std::vector<rgbl_shim::NewMapPoint<KeyFrameNP> > got;
    std::vector<int> per;
    if (!rgbl_shim::CreateNewMapPoints(matcher, &kf1, neigh, mono, inertial, false, far_points != 0, hdr[6], with_skip ? &skip : nullptr, got, &per)) { printf("drop-in failed\n"); return 1; }
    // only the caller's matcher holds a handle: none was acquired (and handed back to the pool) by the call
    if (rgbl_matcher_pool_size() != idle) { printf("the call changed the pool of idle handles: %d -> %d\n", idle, rgbl_matcher_pool_size()); ++failures; }
    // the transcription
    rgbl_new_points_params prm{8, 1.5f * kf1.mfScaleFactor, far_points, hdr[6], inertial, mono, 1};
    want.clear(); want_per.clear(); geometry.clear();
    rgbl_shim::NewPointsFlat f1;
    for (int i = 0; i < nn; ++i) {
      rgbl_triangulation_params tp;
      rgbl_shim::TriangulationParamsOf(&kf1, neigh[i], false, tp);
      geometry.insert(geometry.end(), tp.F12, tp.F12 + 9); geometry.push_back(tp.epipole[0]); geometry.push_back(tp.epipole[1]);
      const V3 a = kf1.GetCameraCenter(), b = neigh[i]->GetCameraCenter();
      const float d[3] = {b.v[0] - a.v[0], b.v[1] - a.v[1], b.v[2] - a.v[2]};
      float s = d[0] * d[0]; s += d[1] * d[1]; s += d[2] * d[2];
      // :448-460: the baseline test, or (monocular) the caller's median-depth test, which skip[] carries
      if ((with_skip && skip[i]) || (!mono && sqrtf(s) < neigh[i]->mb)) { want_per.push_back(-1); continue; }
      std::vector<std::pair<size_t, size_t> > pairs;
      want_per.push_back(matcher.SearchForTriangulation(static_cast<KeyFrame*>(&kf1), static_cast<KeyFrame*>(neigh[i]), pairs, false, false));
      rgbl_shim::NewPointsFlat f2;
      f1.Fill(&kf1); f2.Fill(neigh[i]);
      std::vector<int32_t> i1, i2;
      for (auto& p : pairs) { i1.push_back((int32_t)p.first); i2.push_back((int32_t)p.second); }
      std::vector<rgbl_new_point> r(pairs.size() + 1);
      f1.kf.view.device = nullptr; f2.kf.view.device = nullptr;   // the host build reads host arrays
      if (rgbl_triangulate_matches_host(&f1.kf, &f2.kf, &prm, (int)pairs.size(), i1.data(), i2.data(), r.data()) != RGBL_OK) { printf("host block: %s\n", rgbl_last_error()); return 1; }
      for (size_t k = 0; k < pairs.size(); ++k) {
        if (r[k].status < 1 || r[k].status > 3) continue;
        r[k].neighbour = i;
        want.push_back(r[k]);
        kf1.mvpMapPoints[r[k].idx1] = some;   // mpCurrentKeyFrame->AddMapPoint(pMP, idx1), :701
      }
    }
    const char* what = mono ? "monocular" : inertial ? "inertial" : with_skip ? (resident ? "resident" : "host arrays") : "no skip list";
    if (got.size() != want.size()) { printf("%s: %zu new points, transcription %zu\n", what, got.size(), want.size()); ++failures; }
    for (size_t k = 0; k < got.size() && k < want.size(); ++k) {
      const bool same = got[k].pKF2 == neigh[want[k].neighbour] && got[k].idx1 == want[k].idx1 && got[k].idx2 == want[k].idx2 &&
                        memcmp(got[k].x3D, want[k].x3D, 12) == 0 && got[k].stereo == (want[k].status != 1);
      if (!same && failures++ < 5) printf("%s: new point %zu differs\n", what, k);
    }
    for (int i = 0; i < nn; ++i) if (per[i] != want_per[i]) { printf("%s: neighbour %d: %d matches, transcription %d\n", what, i, per[i], want_per[i]); ++failures; }
    // a rig key frame among the neighbours (NLeft != -1) or as the current one is refused: false, nothing returned, nothing launched
    if (nn > 0 && !mono && !inertial && with_skip && !resident) {
      neigh[nn - 1]->NLeft = 0;
      if (rgbl_shim::CreateNewMapPoints(matcher, &kf1, neigh, false, false, false, false, 0.f, &skip, got) || !got.empty()) { printf("a rig neighbour was not refused\n"); ++failures; }
      neigh[nn - 1]->NLeft = -1;
      Camera second = *cam;
      kf1.mpCamera2 = &second;
      if (rgbl_shim::CreateNewMapPoints(matcher, &kf1, neigh, false, false, false, false, 0.f, nullptr, got) || !got.empty()) { printf("a rig key frame was not refused\n"); ++failures; }
      kf1.mpCamera2 = nullptr;
    }
  }
  for (auto& k : kfs) if (k.own) rgbl_device_frame_destroy(k.own);
  if (kf1.own) rgbl_device_frame_destroy(kf1.own);
  return failures;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int nn = 0, far_points = 0;
  float hdr[8];   // K[4], mb, mbf, th_far_points, unused
  rd(f, &nn, 1); rd(f, &far_points, 1); rd(f, hdr, 8);
  Camera cam{{hdr[0], hdr[1], hdr[2], hdr[3]}};
  MapPoint some;
  std::vector<unsigned char> skip((size_t)nn);
  rd(f, skip.data(), nn);
  const long start = 8 + 32 + nn;
  int failures = 0;
  std::vector<rgbl_new_point> first, want;
  std::vector<int> want_per;
  std::vector<float> geometry;
  size_t counts[5] = {0, 0, 0, 0, 0};
  // host arrays, resident frames, without a skip list, monocular (no baseline test, skip[] decides), inertial (0.9996)
  const bool modes[5][4] = {{false, false, false, true}, {true, false, false, true}, {false, false, false, false}, {false, true, false, true},
                            {true, false, true, true}};
  for (int m = 0; m < 5; ++m) {
    const int r = run(f, start, nn, hdr, far_points, &cam, &some, skip, modes[m][0], modes[m][1], modes[m][2], modes[m][3], want, want_per, geometry);
    if (r < 0) return 2;
    failures += r;
    counts[m] = want.size();
    if (m == 0) {
      first = want;
      FILE* o = fopen(argv[2], "wb");
      if (!o) return 2;
      const int n = (int)want.size();
      wr(o, &n, 1); wr(o, want_per.data(), nn); wr(o, geometry.data(), geometry.size()); wr(o, want.data(), want.size());
      fclose(o);
    } else if (m == 1 && (first.size() != want.size() || (want.size() && memcmp(first.data(), want.data(), want.size() * sizeof(rgbl_new_point)) != 0))) {
      printf("host arrays and resident frames differ\n"); ++failures;
    }
  }
  // the variants are variants: another neighbour set without the skip list and without the baseline test
  if (counts[2] == counts[0] || counts[3] == counts[0]) { printf("the skip list or the monocular flag changed nothing (%zu %zu %zu)\n", counts[0], counts[2], counts[3]); ++failures; }
  fclose(f);
  if (failures) return 1;
  printf("NEW_POINTS_SHIM_OK %zu\n", first.size());
  return 0;
}
