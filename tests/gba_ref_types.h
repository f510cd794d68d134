// gba_ref_types.h — stand-in declarations for the lines src/Optimizer.cc:60-390 of the reference (Optimizer::BundleAdjustment),
// which tests/gba_golden.py copies at test time into the build directory and tests/gba_ref_glue.cpp compiles unmodified.  Only
// the members those lines touch.  TEST INFRASTRUCTURE.
//
// This tier pins the reference's control flow and constants: which key frames and points get a vertex, the vertex ids, the fixed
// flag (:125), maxKFid and the skips at :154 / :156, the monocular / stereo split and the edge order (:147-262), bRobust and both
// Huber deltas (:131-132), removeVertex for a point without observations (:266-270), nIterations, and both write-back branches
// (:285-389).  It does NOT pin g2o's arithmetic: SparseOptimizer::optimize hands the recorded vertices and edges to
// rgbl_bundle_adjustment_host (cameras in addVertex order, fixed ones flagged; the points that were not removed, and the edges,
// in the order added), and chi2() afterwards reads that call's output.  The rig edge (EdgeSE3ProjectXYZToBody) is declared so
// that the lines compile; a scene that reaches it aborts.  GetPoseInverse() is the identity and SE3f * SE3f returns its left
// operand: the block :306-363 they feed only fills locals (it runs for every key frame further than 1 from the origin).
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
  float norm() const { return sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
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
  SE3 operator*(const SE3&) const { return *this; }
};
template <> struct SE3<double> {
  Eigen::Quaterniond q; Eigen::Vector3d t;
  SE3(const Eigen::Quaterniond& qq, const Eigen::Vector3d& tt) : q(qq), t(tt) {}
  template <class T> SE3<float> cast() const { return SE3<float>(q.cast<T>(), t.cast<T>()); }
};
typedef SE3<float> SE3f;
typedef SE3<double> SE3d;
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
struct RefEdge {
  virtual ~RefEdge() {}
  OptimizableGraph::Vertex* v[2] = {nullptr, nullptr};
  double obs[3] = {0, 0, -1};
  double info = 0.0;
  RobustKernelHuber* kernel = nullptr;
  int type = 0;   // 0 monocular, 1 stereo, 2 the rig's
  double chi = 0.0;
  void setVertex(int i, OptimizableGraph::Vertex* p) { v[i] = p; }
  void setRobustKernel(RobustKernelHuber* k) { kernel = k; }
  double chi2() const { return chi; }
  bool isDepthPositive() { return true; }
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
  explicit OptimizationAlgorithmLevenberg(BlockSolver_6_3*) {}
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
struct KeyFrame;
struct Map {
  long unsigned init_id = 0;
  KeyFrame* origin = nullptr;
  long unsigned GetInitKFid() { return init_id; }
  KeyFrame* GetOriginKF() { return origin; }
};
struct MapPoint {
  long unsigned mnId = 0, mnBAGlobalForKF = 0;
  Eigen::Vector3f pos, mPosGBA;
  bool bad = false;
  std::map<KeyFrame*, std::tuple<int, int>> obs;
  int set_pos = 0, updated = 0;
  bool isBad() { return bad; }
  Eigen::Vector3f GetWorldPos() { return pos; }
  void SetWorldPos(const Eigen::Vector3f& p) { pos = p; ++set_pos; }
  void UpdateNormalAndDepth() { ++updated; }
  std::map<KeyFrame*, std::tuple<int, int>> GetObservations() { return obs; }
};
struct KeyFrame {
  long unsigned mnId = 0, mnBAGlobalForKF = 0;
  bool bad = false;
  Map* map = nullptr;
  Sophus::SE3f pose, mTcwGBA;
  int set_pose = 0;
  GeometricCamera cam;
  GeometricCamera* mpCamera = &cam;
  GeometricCamera* mpCamera2 = nullptr;
  int NLeft = -1;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  std::vector<cv::KeyPoint> mvKeysUn, mvKeysRight;
  std::vector<float> mvuRight, mvInvLevelSigma2;
  bool isBad() { return bad; }
  Map* GetMap() { return map; }
  Sophus::SE3f GetPose() { return pose; }
  Sophus::SE3f GetPoseInverse() { return Sophus::SE3f(); }
  Sophus::SE3f GetRelativePoseTrl() { return Sophus::SE3f(); }
  void SetPose(const Sophus::SE3f& T) { pose = T; ++set_pose; }
};
}  // namespace ORB_SLAM3

namespace g2o {
struct SparseOptimizer {
  std::map<int, OptimizableGraph::Vertex*> vertices;
  std::vector<VertexSE3Expmap*> cams;        // in addVertex order
  std::vector<VertexSBAPointXYZ*> points;    // in addVertex order, without the removed ones
  std::vector<RefEdge*> edges;               // in addEdge order
  bool* stop = nullptr;
  struct Record {
    std::vector<int> vertex;    // id, kind (0 camera, 1 point), fixed, marginalized per vertex in the order added
    std::vector<int> edge;      // type, id of vertex 0, id of vertex 1 per edge in the order added
    std::vector<int> removed;   // ids handed to removeVertex, in order
    int optimize_calls = 0, max_iterations = -1, iterations = -1, trials = -1, robust = -1, polls = -1;
    double delta[2] = {0, 0};
  };
  static Record& record() { static Record r; return r; }

  void setAlgorithm(OptimizationAlgorithmLevenberg*) {}
  void setVerbose(bool) {}
  void setForceStopFlag(bool* f) { stop = f; }
  bool addVertex(VertexSE3Expmap* v) { vertices[v->id] = v; cams.push_back(v); note(v, 0); return true; }
  bool addVertex(VertexSBAPointXYZ* v) { vertices[v->id] = v; points.push_back(v); note(v, 1); return true; }
  void note(OptimizableGraph::Vertex* v, int kind) { for (int x : {v->id, kind, (int)v->fixed, (int)v->marginalized}) record().vertex.push_back(x); }
  OptimizableGraph::Vertex* vertex(int id) { auto it = vertices.find(id); return it == vertices.end() ? nullptr : it->second; }
  bool removeVertex(VertexSBAPointXYZ* v) {
    for (RefEdge* e : edges)
      if (e->v[0] == v) { std::cerr << "removeVertex of a point with an edge" << std::endl; abort(); }
    vertices.erase(v->id);
    for (size_t i = 0; i < points.size(); ++i)
      if (points[i] == v) { points.erase(points.begin() + (long)i); break; }
    record().removed.push_back(v->id);
    return true;
  }
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
    int with_kernel = 0;
    Record& R = record();
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
      if (e->kernel) {
        ++with_kernel;
        if (R.delta[e->type] != 0.0 && R.delta[e->type] != e->kernel->delta) { std::cerr << "two deltas for one edge type" << std::endl; abort(); }
        R.delta[e->type] = e->kernel->delta;
      }
    }
    if (with_kernel != 0 && with_kernel != nE) { std::cerr << "some edges with a kernel, some without" << std::endl; abort(); }
    for (int c = 0; c < nC; ++c)
      if (!have_K[c]) { K[4 * c] = K[4 * c + 1] = 1.0f; }
    rgbl_ba_input in;
    rgbl_ba_output out;
    memset(&in, 0, sizeof(in));
    memset(&out, 0, sizeof(out));
    in.n_cams = nC; in.cam_is_fixed = fixed.data();
    in.cam_q = q.data(); in.cam_t = t.data(); in.cam_K = K.data(); in.cam_bf = bf.data();
    in.n_points = nP; in.world_pos = pos.data();
    in.n_edges = nE; in.edge_point = ep.data(); in.edge_cam = ec.data(); in.edge_obs = obs.data(); in.edge_inv_sigma2 = info.data();
    in.robust = with_kernel ? 1 : 0;
    in.max_iterations = iterations;
    in.stop_byte = reinterpret_cast<const volatile uint8_t*>(stop);
    std::vector<double> dq(4 * (size_t)nC), dt(3 * (size_t)nC), dp(3 * (size_t)nP), chi((size_t)nE);
    out.chi2 = chi.data();
    out.diag.cam_q = dq.data(); out.diag.cam_t = dt.data(); out.diag.point = dp.data();
    if (rgbl_bundle_adjustment_host(&in, &out) != RGBL_OK) { std::cerr << rgbl_last_error() << std::endl; abort(); }
    ++R.optimize_calls; R.max_iterations = iterations; R.iterations = out.diag.iterations; R.trials = out.diag.trials;
    R.robust = in.robust; R.polls = out.diag.polls;
    for (int c = 0; c < nC; ++c) {
      for (int i = 0; i < 4; ++i) cams[c]->est.r.c[i] = dq[4 * c + i];
      for (int i = 0; i < 3; ++i) cams[c]->est.t.v[i] = dt[3 * c + i];
    }
    for (int p = 0; p < nP; ++p)
      for (int i = 0; i < 3; ++i) points[p]->X.v[i] = dp[3 * p + i];
    for (int k = 0; k < nE; ++k) edges[k]->chi = chi[k];
    return out.diag.iterations;
  }
};
}  // namespace g2o

namespace ORB_SLAM3 {
class Optimizer {
 public:
  void static BundleAdjustment(const std::vector<KeyFrame*>& vpKF, const std::vector<MapPoint*>& vpMP, int nIterations = 5, bool* pbStopFlag = NULL,
                               const unsigned long nLoopKF = 0, const bool bRobust = true);
};
}  // namespace ORB_SLAM3
