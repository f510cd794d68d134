// lba_ref_types.h — stand-in declarations for the lines src/Optimizer.cc:1116-1498 of the reference
// (Optimizer::LocalBundleAdjustment), which tests/lba_golden.py copies at test time into the build directory and
// tests/lba_ref_glue.cpp compiles unmodified.  Only the members those lines touch.  TEST INFRASTRUCTURE.
//
// This tier pins the reference's control flow: the three lists (:1118-1178), num_fixedKF and the return at :1182, the vertex ids
// and which vertices are fixed, the monocular / stereo split and the edge order (:1282-1403), num_edges, the stop return at
// :1406, the erase list and its order (:1413-1460), the calls under the map's mutex and the write-back (:1464-1497).
// It does NOT pin g2o's arithmetic: SparseOptimizer::optimize hands the recorded vertices and edges to
// rgbl_local_bundle_adjustment_host (cameras in addVertex order, fixed ones flagged; points and edges in the order added), and
// chi2() / isDepthPositive() afterwards read that call's outputs.  The rig edge (EdgeSE3ProjectXYZToBody) is declared so that the
// lines compile; a scene that reaches it aborts.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <iostream>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../include/rgbl_frontend.h"

namespace Eigen {
struct Vector3f;
struct Vector3d {
  double v[3] = {0, 0, 0};
  double operator()(int i) const { return v[i]; }
  template <class T> Vector3f cast() const;
};
struct Vector3f {
  float v[3] = {0, 0, 0};
  float operator()(int i) const { return v[i]; }
  template <class T> Vector3d cast() const { Vector3d r; for (int i = 0; i < 3; ++i) r.v[i] = (T)v[i]; return r; }
};
template <class T> Vector3f Vector3d::cast() const { Vector3f r; for (int i = 0; i < 3; ++i) r.v[i] = (T)v[i]; return r; }
struct Quaternionf;
struct Quaterniond {
  double c[4] = {0, 0, 0, 1};   // x y z w
  template <class T> Quaternionf cast() const;
};
struct Quaternionf {
  float c[4] = {0, 0, 0, 1};
  template <class T> Quaterniond cast() const { Quaterniond r; for (int i = 0; i < 4; ++i) r.c[i] = (T)c[i]; return r; }
};
template <class T> Quaternionf Quaterniond::cast() const { Quaternionf r; for (int i = 0; i < 4; ++i) r.c[i] = (T)c[i]; return r; }
struct Matrix2d {
  double d = 0.0;   // a multiple of the identity is all the lines build
  static Matrix2d Identity() { Matrix2d r; r.d = 1.0; return r; }
  Matrix2d operator*(float s) const { Matrix2d r; r.d = d * (double)s; return r; }
};
struct Matrix3d {
  double d = 0.0;
  static Matrix3d Identity() { Matrix3d r; r.d = 1.0; return r; }
  Matrix3d operator*(float s) const { Matrix3d r; r.d = d * (double)s; return r; }
};
template <class T, int R, int C> struct Matrix {
  T v[R * C] = {};
  struct Comma {
    Matrix* m; int k;
    Comma operator,(T x) { m->v[k] = x; return Comma{m, k + 1}; }
  };
  Comma operator<<(T x) { v[0] = x; return Comma{this, 1}; }
};
}  // namespace Eigen

namespace Sophus {
template <class T> struct SE3;
template <> struct SE3<float> {
  Eigen::Quaternionf q; Eigen::Vector3f t;
  SE3() {}
  SE3(const Eigen::Quaternionf& qq, const Eigen::Vector3f& tt) : q(qq), t(tt) {}
  Eigen::Quaternionf unit_quaternion() const { return q; }
  Eigen::Vector3f translation() const { return t; }
};
typedef SE3<float> SE3f;
}  // namespace Sophus

namespace cv {
struct Point2f { float x = 0, y = 0; };
struct KeyPoint { Point2f pt; float size = 0, angle = -1, response = 0; int octave = 0, class_id = -1; };
}  // namespace cv

namespace ORB_SLAM3 { struct GeometricCamera { float K[4] = {0, 0, 0, 0}; }; }

namespace g2o {
struct SE3Quat {
  Eigen::Quaterniond r; Eigen::Vector3d t;
  SE3Quat() {}
  SE3Quat(const Eigen::Quaterniond& q, const Eigen::Vector3d& tt) : r(q), t(tt) {}
  const Eigen::Quaterniond& rotation() const { return r; }
  const Eigen::Vector3d& translation() const { return t; }
};
struct RobustKernelHuber {
  double delta = 1.0;
  void setDelta(double d) { delta = d; }
};
struct OptimizableGraph {
  struct Vertex {
    int id = -1;
    bool fixed = false, marginalized = false;
    virtual ~Vertex() {}
    void setId(int i) { id = i; }
    void setFixed(bool f) { fixed = f; }
    void setMarginalized(bool m) { marginalized = m; }
  };
};
struct VertexSBAPointXYZ : OptimizableGraph::Vertex {
  Eigen::Vector3d X;
  void setEstimate(const Eigen::Vector3d& x) { X = x; }
  const Eigen::Vector3d& estimate() const { return X; }
};
struct VertexSE3Expmap : OptimizableGraph::Vertex {
  SE3Quat est;
  void setEstimate(const SE3Quat& s) { est = s; }
  const SE3Quat& estimate() const { return est; }
};
// one edge as the lines set it; chi2 and the depth sign come back from the optimisation
struct RefEdge {
  virtual ~RefEdge() {}
  OptimizableGraph::Vertex* v[2] = {nullptr, nullptr};
  double obs[3] = {0, 0, -1};
  double info = 0.0;
  RobustKernelHuber* kernel = nullptr;
  int type = 0;   // 0 monocular, 1 stereo, 2 the rig's
  double chi = 0.0;
  bool depth_positive = true;
  void setVertex(int i, OptimizableGraph::Vertex* p) { v[i] = p; }
  void setRobustKernel(RobustKernelHuber* k) { kernel = k; }
  double chi2() const { return chi; }
  bool isDepthPositive() { return depth_positive; }
};
struct EdgeStereoSE3ProjectXYZ : RefEdge {
  double fx = 0, fy = 0, cx = 0, cy = 0, bf = 0;
  EdgeStereoSE3ProjectXYZ() { type = 1; }
  void setMeasurement(const Eigen::Matrix<double, 3, 1>& o) { for (int i = 0; i < 3; ++i) obs[i] = o.v[i]; }
  void setInformation(const Eigen::Matrix3d& m) { info = m.d; }
};
struct BlockSolver_6_3 {
  struct LinearSolverType { virtual ~LinearSolverType() {} };
  struct PoseMatrixType {};
  explicit BlockSolver_6_3(LinearSolverType*) {}
};
template <class M> struct LinearSolverEigen : BlockSolver_6_3::LinearSolverType {};
struct OptimizationAlgorithmLevenberg {
  double user_lambda_init = 0.0;
  explicit OptimizationAlgorithmLevenberg(BlockSolver_6_3*) {}
  void setUserLambdaInit(double v) { user_lambda_init = v; }
};
}  // namespace g2o

namespace ORB_SLAM3 {
using namespace std;

struct Verbose {
  enum eLevel { VERBOSITY_QUIET = 0, VERBOSITY_NORMAL = 1, VERBOSITY_VERBOSE = 2, VERBOSITY_VERY_VERBOSE = 3, VERBOSITY_DEBUG = 4 };
  static void PrintMess(const std::string&, eLevel) {}
};
struct EdgeSE3ProjectXYZ : g2o::RefEdge {
  GeometricCamera* pCamera = nullptr;
  void setMeasurement(const Eigen::Matrix<double, 2, 1>& o) { obs[0] = o.v[0]; obs[1] = o.v[1]; obs[2] = -1.0; }
  void setInformation(const Eigen::Matrix2d& m) { info = m.d; }
};
struct EdgeSE3ProjectXYZToBody : EdgeSE3ProjectXYZ {
  g2o::SE3Quat mTrl;
  EdgeSE3ProjectXYZToBody() { type = 2; }
};
struct Map {
  long unsigned init_id = 0;
  bool inertial = false;
  int change = 0;
  std::mutex mMutexMapUpdate;
  std::set<long unsigned> msOptKFs, msFixedKFs;
  long unsigned GetInitKFid() { return init_id; }
  bool IsInertial() { return inertial; }
  void IncreaseChangeIndex() { ++change; }
};
struct KeyFrame;
struct CallLog { std::vector<int> calls; bool mutex_held_at_every_call = true; };
struct MapPoint {
  int idx = 0;
  long unsigned mnId = 0, mnBALocalForKF = 0;
  Eigen::Vector3f pos;
  bool bad = false;
  Map* map = nullptr;
  std::map<KeyFrame*, std::tuple<int, int>> obs;
  int set_pos = 0, updated = 0;
  CallLog* log = nullptr;
  bool isBad() { return bad; }
  Map* GetMap() { return map; }
  Eigen::Vector3f GetWorldPos() { return pos; }
  void SetWorldPos(const Eigen::Vector3f& p) { pos = p; ++set_pos; }
  void UpdateNormalAndDepth() { ++updated; }
  std::map<KeyFrame*, std::tuple<int, int>> GetObservations() { return obs; }
  void EraseObservation(KeyFrame* kf);
};
struct KeyFrame {
  int idx = 0;
  long unsigned mnId = 0, mnBALocalForKF = 0, mnBAFixedForKF = 0;
  bool bad = false;
  Map* map = nullptr;
  Sophus::SE3f pose;
  int set_pose = 0;
  GeometricCamera cam;
  GeometricCamera* mpCamera = &cam;
  GeometricCamera* mpCamera2 = nullptr;
  int NLeft = -1;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  std::vector<cv::KeyPoint> mvKeysUn, mvKeysRight;
  std::vector<float> mvuRight, mvInvLevelSigma2;
  std::vector<MapPoint*> mps;
  std::vector<KeyFrame*> covisible;
  CallLog* log = nullptr;
  bool isBad() { return bad; }
  Map* GetMap() { return map; }
  Sophus::SE3f GetPose() { return pose; }
  Sophus::SE3f GetRelativePoseTrl() { return Sophus::SE3f(); }
  void SetPose(const Sophus::SE3f& T) { pose = T; ++set_pose; }
  std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return covisible; }
  std::vector<MapPoint*> GetMapPointMatches() { return mps; }
  void EraseMapPointMatch(MapPoint* mp) {
    if (map->mMutexMapUpdate.try_lock()) { map->mMutexMapUpdate.unlock(); log->mutex_held_at_every_call = false; }
    log->calls.push_back(0); log->calls.push_back(idx); log->calls.push_back(mp->idx);
  }
};
inline void MapPoint::EraseObservation(KeyFrame* kf) { log->calls.push_back(1); log->calls.push_back(kf->idx); log->calls.push_back(idx); }
}  // namespace ORB_SLAM3

namespace g2o {
struct SparseOptimizer {
  std::map<int, OptimizableGraph::Vertex*> vertices;
  std::vector<VertexSE3Expmap*> cams;        // in addVertex order
  std::vector<VertexSBAPointXYZ*> points;
  std::vector<RefEdge*> edges;               // in addEdge order
  OptimizationAlgorithmLevenberg* algorithm = nullptr;
  bool* stop = nullptr;
  struct Record {
    std::vector<int> vertex;   // id, kind (0 camera, 1 point), fixed, marginalized per vertex in the order added
    std::vector<int> edge;     // type, id of vertex 0, id of vertex 1 per edge in the order added
    int optimize_calls = 0, max_iterations = -1, iterations = -1, trials = -1, ran = -1;
    double user_lambda_init = 0.0, delta[2] = {0, 0};
  };
  static Record& record() { static Record r; return r; }

  void setAlgorithm(OptimizationAlgorithmLevenberg* a) { algorithm = a; }
  void setVerbose(bool) {}
  void setForceStopFlag(bool* f) { stop = f; }
  bool addVertex(VertexSE3Expmap* v) { vertices[v->id] = v; cams.push_back(v); note(v, 0); return true; }
  bool addVertex(VertexSBAPointXYZ* v) { vertices[v->id] = v; points.push_back(v); note(v, 1); return true; }
  void note(OptimizableGraph::Vertex* v, int kind) { for (int x : {v->id, kind, (int)v->fixed, (int)v->marginalized}) record().vertex.push_back(x); }
  OptimizableGraph::Vertex* vertex(int id) { auto it = vertices.find(id); return it == vertices.end() ? nullptr : it->second; }
  bool addEdge(RefEdge* e) {
    if (!e->v[0] || !e->v[1] || e->type == 2) { std::cerr << "an edge without a vertex, or the rig's edge" << std::endl; abort(); }
    edges.push_back(e);
    for (int x : {e->type, e->v[0]->id, e->v[1]->id}) record().edge.push_back(x);
    return true;
  }
  void initializeOptimization() {}
  int optimize(int iterations) {
    const int nC = (int)cams.size(), nP = (int)points.size(), nE = (int)edges.size();
    std::map<OptimizableGraph::Vertex*, int> cam_index, point_index;
    std::vector<uint8_t> fixed((size_t)nC);
    std::vector<float> q(4 * (size_t)nC), t(3 * (size_t)nC), K(4 * (size_t)nC, 0.0f), bf((size_t)nC, 0.0f), pos(3 * (size_t)nP), obs(3 * (size_t)nE), info((size_t)nE);
    std::vector<uint8_t> have_K((size_t)nC, 0);
    for (int c = 0; c < nC; ++c) {
      cam_index[cams[c]] = c;
      fixed[c] = cams[c]->fixed ? 1 : 0;
      for (int i = 0; i < 4; ++i) q[4 * c + i] = (float)cams[c]->est.r.c[i];
      for (int i = 0; i < 3; ++i) t[3 * c + i] = (float)cams[c]->est.t.v[i];
    }
    for (int p = 0; p < nP; ++p) {
      point_index[points[p]] = p;
      for (int i = 0; i < 3; ++i) pos[3 * p + i] = (float)points[p]->X.v[i];
    }
    std::vector<int32_t> ep((size_t)nE), ec((size_t)nE);
    for (int k = 0; k < nE; ++k) {
      RefEdge* e = edges[k];
      ep[k] = point_index.at(e->v[0]); ec[k] = cam_index.at(e->v[1]);
      float Ke[4], bfe = 0.0f;
      if (e->type == 1) {
        auto* s = static_cast<EdgeStereoSE3ProjectXYZ*>(e);
        Ke[0] = (float)s->fx; Ke[1] = (float)s->fy; Ke[2] = (float)s->cx; Ke[3] = (float)s->cy; bfe = (float)s->bf;
      } else {
        auto* m = static_cast<ORB_SLAM3::EdgeSE3ProjectXYZ*>(e);
        for (int i = 0; i < 4; ++i) Ke[i] = m->pCamera->K[i];
      }
      const int c = ec[k];
      for (int i = 0; i < 4; ++i) {
        if (have_K[c] && K[4 * c + i] != Ke[i]) { std::cerr << "a camera with two sets of intrinsics" << std::endl; abort(); }
        K[4 * c + i] = Ke[i];
      }
      have_K[c] = 1;
      if (e->type == 1) bf[c] = bfe;
      for (int i = 0; i < 3; ++i) obs[3 * k + i] = (float)e->obs[i];
      info[k] = (float)e->info;
      if (e->kernel) record().delta[e->type] = e->kernel->delta;
    }
    for (int c = 0; c < nC; ++c)
      if (!have_K[c]) { K[4 * c] = K[4 * c + 1] = 1.0f; }
    rgbl_lba_input in;
    rgbl_lba_output out;
    memset(&in, 0, sizeof(in));
    memset(&out, 0, sizeof(out));
    in.n_free = nC; in.n_fixed = 0; in.free_is_fixed = fixed.data();
    in.cam_q = q.data(); in.cam_t = t.data(); in.cam_K = K.data(); in.cam_bf = bf.data();
    in.n_points = nP; in.world_pos = pos.data();
    in.n_edges = nE; in.edge_point = ep.data(); in.edge_cam = ec.data(); in.edge_obs = obs.data(); in.edge_inv_sigma2 = info.data();
    in.max_iterations = iterations;
    in.user_lambda_init = algorithm ? algorithm->user_lambda_init : 0.0;
    in.stop_byte = reinterpret_cast<const volatile uint8_t*>(stop);
    std::vector<double> dq(4 * (size_t)nC), dt(3 * (size_t)nC), dp(3 * (size_t)nP), chi((size_t)nE);
    std::vector<uint8_t> flags((size_t)nE);
    out.chi2 = chi.data(); out.flags = flags.data();
    out.diag.cam_q = dq.data(); out.diag.cam_t = dt.data(); out.diag.point = dp.data();
    if (rgbl_local_bundle_adjustment_host(&in, &out) != RGBL_OK) { std::cerr << rgbl_last_error() << std::endl; abort(); }
    Record& R = record();
    ++R.optimize_calls; R.max_iterations = iterations; R.ran = out.diag.ran; R.iterations = out.diag.iterations; R.trials = out.diag.trials;
    R.user_lambda_init = in.user_lambda_init;
    if (!out.diag.ran) return 0;
    for (int c = 0; c < nC; ++c) {
      for (int i = 0; i < 4; ++i) cams[c]->est.r.c[i] = dq[4 * c + i];
      for (int i = 0; i < 3; ++i) cams[c]->est.t.v[i] = dt[3 * c + i];
    }
    for (int p = 0; p < nP; ++p)
      for (int i = 0; i < 3; ++i) points[p]->X.v[i] = dp[3 * p + i];
    for (int k = 0; k < nE; ++k) { edges[k]->chi = chi[k]; edges[k]->depth_positive = !(flags[k] & 2); }
    return out.diag.iterations;
  }
};
}  // namespace g2o

namespace ORB_SLAM3 {
class Optimizer {
 public:
  void static LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges);
};
}  // namespace ORB_SLAM3
