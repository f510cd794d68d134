// sim3_opt_ref_types.h — stand-in declarations for the lines src/Optimizer.cc:2115-2381 of the reference (Optimizer::OptimizeSim3),
// which tests/sim3_opt_golden.py copies at test time into the build directory and tests/sim3_opt_ref_glue.cpp compiles
// unmodified.  Only the members those lines touch.  TEST INFRASTRUCTURE.
//
// This tier pins the reference's control flow: the set-up loop (:2167-2304: which features get an edge pair, the float
// P3D1c / P3D2c and the float depth test, obs1, obs2 from mvKeysUn[i2] or the normalised point, both informations), deltaHuber,
// optimize(5), which pairs :2313-2340 drops and which lose their kernel, nMoreIterations, the return at :2349, the second
// optimize(), the final loop and what is written to vpMatches1, g2oS12 and mAcumHessian.
// cv::KeyPoint has OpenCV's constructor (pt, size, angle, response, octave, class_id): :2280 therefore leaves octave 0 for a
// match that is not observed in pKF2, as it does with OpenCV.
// It does NOT pin g2o's arithmetic: SparseOptimizer::optimize hands the graph to csrc/sim3opt_math.h's so_levenberg, chi2()
// and computeError() are the header's so_error, g2o::Sim3 is the header's SoSim3.  Eigen's R * X + t is written in the order
// of csrc/sim3_math.h (s3_transform).
#pragma once
#include <math.h>
#include <stdint.h>

#include <cmath>
#include <iostream>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../orb_slam3_rgbl_amd/csrc/sim3opt_math.h"

namespace Eigen {
struct Vector3d {
  double v[3] = {0, 0, 0};
  double operator()(int i) const { return v[i]; }
};
struct Vector3f {
  float v[3] = {0, 0, 0};
  float& operator()(int i) { return v[i]; }
  float operator()(int i) const { return v[i]; }
  Vector3f operator+(const Vector3f& o) const { Vector3f r; for (int i = 0; i < 3; ++i) r.v[i] = v[i] + o.v[i]; return r; }
  template <class T> Vector3d cast() const { Vector3d r; for (int i = 0; i < 3; ++i) r.v[i] = (T)v[i]; return r; }
};
struct Matrix3f {
  float m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  Vector3f operator*(const Vector3f& x) const {   // the products of s3_transform; the caller adds t
    Vector3f r;
    for (int i = 0; i < 3; ++i) r.v[i] = rgbl::fr_row_times(m + 3 * i, x.v[0], x.v[1], x.v[2]);
    return r;
  }
};
struct Matrix2d {
  double d = 0.0;   // a multiple of the identity is all the lines build
  static Matrix2d Identity() { Matrix2d r; r.d = 1.0; return r; }
  Matrix2d operator*(float s) const { Matrix2d r; r.d = d * (double)s; return r; }
};
struct MatrixXd {
  static MatrixXd Zero(int, int) { return MatrixXd(); }
};
template <class T, int R, int C> struct Matrix;
template <> struct Matrix<double, 2, 1> {
  double v[2] = {0, 0};
  struct Comma {
    Matrix* m; int k;
    Comma operator,(double x) { m->v[k] = x; return Comma{m, k + 1}; }
  };
  Comma operator<<(double x) { v[0] = x; return Comma{this, 1}; }
};
template <> struct Matrix<double, 7, 7> {
  double m[49];
  Matrix() { for (double& x : m) x = 3.0; }   // what the caller's matrix holds before the call
  Matrix& operator=(const MatrixXd&) { for (double& x : m) x = 0.0; return *this; }
  double largest() const { double a = 0; for (double x : m) a = fabs(x) > a ? fabs(x) : a; return a; }
};
}  // namespace Eigen

namespace cv {
struct Point2f {
  float x = 0, y = 0;
  Point2f() {}
  Point2f(float a, float b) : x(a), y(b) {}
};
struct KeyPoint {   // OpenCV's: KeyPoint(Point2f pt, float size, float angle = -1, float response = 0, int octave = 0, int class_id = -1)
  Point2f pt;
  float size = 0, angle = -1, response = 0;
  int octave = 0, class_id = -1;
  KeyPoint() {}
  KeyPoint(Point2f p, float size_, float angle_ = -1, float response_ = 0, int octave_ = 0, int class_id_ = -1)
      : pt(p), size(size_), angle(angle_), response(response_), octave(octave_), class_id(class_id_) {}
};
}  // namespace cv

namespace g2o {
struct Sim3 { rgbl::SoSim3 S = {{0, 0, 0, 1}, {0, 0, 0}, 1.0}; };

struct RobustKernelHuber {
  double delta = 1.0;
  void setDelta(double d) { delta = d; }
};
struct OptimizableGraph {
  struct Vertex {
    int id = -1;
    bool fixed = false;
    virtual ~Vertex() {}
    void setId(int i) { id = i; }
    void setFixed(bool f) { fixed = f; }
  };
};
struct VertexSBAPointXYZ : OptimizableGraph::Vertex {
  Eigen::Vector3d X;
  void setEstimate(const Eigen::Vector3d& x) { X = x; }
};
struct VertexSim3Expmap : OptimizableGraph::Vertex {
  Sim3 est;
  void setEstimate(const Sim3& s) { est = s; }
  const Sim3& estimate() const { return est; }
};
struct BlockSolverX {
  struct LinearSolverType { virtual ~LinearSolverType() {} };
  struct PoseMatrixType {};
  explicit BlockSolverX(LinearSolverType*) {}
};
template <class M> struct LinearSolverDense : BlockSolverX::LinearSolverType {};
struct OptimizationAlgorithmLevenberg { explicit OptimizationAlgorithmLevenberg(BlockSolverX*) {} };
}  // namespace g2o

namespace ORB_SLAM3 {
using namespace std;

struct Verbose {
  enum eLevel { VERBOSITY_QUIET = 0, VERBOSITY_NORMAL = 1, VERBOSITY_VERBOSE = 2, VERBOSITY_VERY_VERBOSE = 3, VERBOSITY_DEBUG = 4 };
  static void PrintMess(const std::string&, eLevel) {}
};
struct GeometricCamera { float K[4] = {0, 0, 0, 0}; };
struct KeyFrame;
struct MapPoint {
  Eigen::Vector3f pos;
  bool bad = false;
  int mnTrackScaleLevel = -1;   // Frame.cc:668 leaves -1 outside the frustum
  KeyFrame* seen_in = nullptr;
  int index_there = -1;
  bool isBad() { return bad; }
  Eigen::Vector3f GetWorldPos() { return pos; }
  std::tuple<int, int> GetIndexInKeyFrame(KeyFrame* pKF) { return pKF == seen_in ? std::make_tuple(index_there, -1) : std::make_tuple(-1, -1); }
};
struct KeyFrame {
  Eigen::Matrix3f R; Eigen::Vector3f t;
  GeometricCamera* mpCamera = nullptr;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<float> mvInvLevelSigma2;
  std::vector<MapPoint*> mps;
  Eigen::Matrix3f GetRotation() { return R; }
  Eigen::Vector3f GetTranslation() { return t; }
  std::vector<MapPoint*> GetMapPointMatches() { return mps; }
};

struct VertexSim3Expmap : g2o::VertexSim3Expmap {   // :2377 reads the ORB_SLAM3 vertex through g2o's class
  bool _fix_scale = false;
  GeometricCamera *pCamera1 = nullptr, *pCamera2 = nullptr;
};

// one edge of a pair: what the lines set, and the chi2 of the error computed last
struct Sim3Edge {
  virtual ~Sim3Edge() {}
  g2o::OptimizableGraph::Vertex* v[2] = {nullptr, nullptr};
  Eigen::Matrix<double, 2, 1> obs;
  Eigen::Matrix2d info;
  g2o::RobustKernelHuber* kernel = nullptr;
  double chi = 0.0;
  bool inverse = false;
  void setVertex(int i, g2o::OptimizableGraph::Vertex* p) { v[i] = p; }
  void setMeasurement(const Eigen::Matrix<double, 2, 1>& o) { obs = o; }
  void setInformation(const Eigen::Matrix2d& m) { info = m; }
  void setRobustKernel(g2o::RobustKernelHuber* k) { kernel = k; }
  double chi2() const { return chi; }
  void computeError() {
    const VertexSim3Expmap* s = static_cast<const VertexSim3Expmap*>(v[1]);
    const g2o::VertexSBAPointXYZ* p = static_cast<const g2o::VertexSBAPointXYZ*>(v[0]);
    const GeometricCamera* c = inverse ? s->pCamera2 : s->pCamera1;
    const rgbl::SoCam C = {(double)c->K[0], (double)c->K[1], (double)c->K[2], (double)c->K[3]};
    const float o[2] = {(float)obs.v[0], (float)obs.v[1]}, X[3] = {(float)p->X.v[0], (float)p->X.v[1], (float)p->X.v[2]};
    double err[2];
    chi = rgbl::so_error(o, X, info.d, C, inverse ? rgbl::so_inverse(s->est.S) : s->est.S, err);
  }
};
struct EdgeSim3ProjectXYZ : Sim3Edge {};
struct EdgeInverseSim3ProjectXYZ : Sim3Edge { EdgeInverseSim3ProjectXYZ() { inverse = true; } };
}  // namespace ORB_SLAM3

namespace g2o {
// what the glue records of every optimize()
struct OptimizeCall { int max_iterations, pairs, robust_edges, iterations; };

struct SparseOptimizer {
  std::map<int, OptimizableGraph::Vertex*> vertices;
  std::vector<ORB_SLAM3::Sim3Edge*> added;    // in the order of addEdge: e12, e21 of pair 0, of pair 1, ...
  std::set<ORB_SLAM3::Sim3Edge*> removed;
  double x[7] = {0, 0, 0, 0, 0, 0, 0};
  static std::vector<OptimizeCall>& calls() { static std::vector<OptimizeCall> c; return c; }
  static std::vector<ORB_SLAM3::Sim3Edge*>& all_edges() { static std::vector<ORB_SLAM3::Sim3Edge*> e; return e; }

  void setAlgorithm(OptimizationAlgorithmLevenberg*) {}
  bool addVertex(OptimizableGraph::Vertex* v) { vertices[v->id] = v; return true; }
  OptimizableGraph::Vertex* vertex(int id) { auto it = vertices.find(id); return it == vertices.end() ? nullptr : it->second; }
  bool addEdge(ORB_SLAM3::Sim3Edge* e) { added.push_back(e); all_edges().push_back(e); return true; }
  bool removeEdge(ORB_SLAM3::Sim3Edge* e) { removed.insert(e); return true; }
  void initializeOptimization() {}
  // the graph through csrc/sim3opt_math.h's Levenberg: pair k keeps its lane after other pairs were removed
  int optimize(int iterations) {
    ORB_SLAM3::VertexSim3Expmap* s = static_cast<ORB_SLAM3::VertexSim3Expmap*>(vertex(0));
    const size_t m = added.size() / 2;
    std::vector<rgbl::SoEdge> edges(m);
    int active = 0, robust = 0;
    double delta = 0.0;
    for (size_t k = 0; k < m; ++k) {
      ORB_SLAM3::Sim3Edge *a = added[2 * k], *b = added[2 * k + 1];
      rgbl::SoEdge& e = edges[k];
      const VertexSBAPointXYZ *p2 = static_cast<const VertexSBAPointXYZ*>(a->v[0]), *p1 = static_cast<const VertexSBAPointXYZ*>(b->v[0]);
      for (int c = 0; c < 3; ++c) { e.X1[c] = (float)p1->X.v[c]; e.X2[c] = (float)p2->X.v[c]; }
      for (int c = 0; c < 2; ++c) { e.obs1[c] = (float)a->obs.v[c]; e.obs2[c] = (float)b->obs.v[c]; }
      e.info1 = (float)a->info.d; e.info2 = (float)b->info.d;
      e.gone = removed.count(a) ? 1 : 0; e.cleared = 0;
      e.chi12 = a->chi; e.chi21 = b->chi;
      if (!e.gone) {
        ++active;
        for (ORB_SLAM3::Sim3Edge* q : {a, b})
          if (q->kernel) { ++robust; delta = q->kernel->delta; }
      }
    }
    OptimizeCall call = {iterations, active, robust, 0};
    if (robust != 0 && robust != 2 * active) { std::cerr << "mixed kernels" << std::endl; abort(); }
    if (active > 0) {
      std::vector<rgbl::SoHostLanes> lanes(1, rgbl::SoHostLanes(edges.data(), (int)m));
      const rgbl::SoCam C1 = {(double)s->pCamera1->K[0], (double)s->pCamera1->K[1], (double)s->pCamera1->K[2], (double)s->pCamera1->K[3]};
      const rgbl::SoCam C2 = {(double)s->pCamera2->K[0], (double)s->pCamera2->K[1], (double)s->pCamera2->K[2], (double)s->pCamera2->K[3]};
      double chi = 0.0;
      rgbl::so_levenberg(lanes[0], C1, C2, s->est.S, robust != 0, delta, s->_fix_scale, iterations, x, &call.iterations, &chi);
      for (size_t k = 0; k < m; ++k)
        if (!edges[k].gone) { added[2 * k]->chi = edges[k].chi12; added[2 * k + 1]->chi = edges[k].chi21; }
    }
    calls().push_back(call);
    return call.iterations;
  }
};
}  // namespace g2o

namespace ORB_SLAM3 {
class Optimizer {
 public:
  int static OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
                          const bool bFixScale, Eigen::Matrix<double, 7, 7>& mAcumHessian, const bool bAllPoints = false);
};
}  // namespace ORB_SLAM3
