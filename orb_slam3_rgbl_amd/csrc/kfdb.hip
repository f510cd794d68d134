// kfdb.hip — KeyFrameDatabase on the device (include/rgbl_frontend.h: rgbl_kfdb_*).
//
// The reference keeps an inverted file (one std::list<KeyFrame*> per vocabulary word, src/KeyFrameDatabase.cc:39-45) and
// answers a place-recognition query by walking the lists of the query's words (:615-635, :741-756).  What that walk computes
// per stored key frame is the size of the intersection of two ascending id lists, and the position of a key frame in
// lKFsSharingWords is decided by the first list it is met in and its position inside that list: ascending by (smallest
// common word id, order of add()).  Here every stored BowVector lies in an append-only arena of ascending (id, value) pairs,
// one wave intersects one (query, entry) pair, and the host orders the sharing entries by that key.
//
//   k_kfdb_common   one wave per (query, entry): common words, smallest common word id, per-query atomicMax
//   k_kfdb_score    the entries with more than int(max * 0.8f) common words: L1Scoring::score, terms in ascending word
//                   order added one after another in double (ScoringObject.cpp:23-68) - bit-identical, never tree-reduced
//   k_kfdb_compact  moves the live entries of an arena with more dead than live words into a fresh one
//
// Traffic per query: every live entry's ids once (4 B a word), the values (8 B a word) of the scored entries only.
#include <string.h>

#include <algorithm>
#include <mutex>
#include <unordered_map>

#include "common.h"

namespace rgbl {

constexpr int kKfdbWaves = 4;                  // waves per workgroup; all of them work on the same query
constexpr int kKfdbMaxQueryWords = 15360;      // 60 KiB of query ids in LDS, next to the score kernel's 2 KiB of terms
constexpr int kKfdbScoreHead = kKfdbWaves * kWave + 2;   // doubles in front of the ids: terms [4][64] | flag (16 B)

struct KfdbEntry { uint32_t off; int32_t n; };            // n < 0: tombstone
struct KfdbMove { uint32_t src, dst; int32_t n; };

// position of `id` in the ascending q[0 .. nq), -1 if it is not there
__device__ __forceinline__ int kfdb_find(const uint32_t* q, int nq, uint32_t id) {
  int lo = 0, hi = nq;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (q[mid] < id) lo = mid + 1; else hi = mid;
  }
  return (lo < nq && q[lo] == id) ? lo : -1;
}

// grid = (entry groups, queries), block = 256.  Dynamic LDS: the query's ids.  Every wave takes the entries
// blockIdx.x * 4 + wave, + gridDim.x * 4, ...; lanes take entry words and binary-search the staged ids.
__global__ __launch_bounds__(256) void k_kfdb_common(const KfdbEntry* __restrict__ ent, int n_ent, const uint32_t* __restrict__ arena_id,
                                                     const int32_t* __restrict__ q_off, const uint32_t* __restrict__ q_id,
                                                     const uint8_t* __restrict__ excl, int32_t* __restrict__ count,
                                                     uint32_t* __restrict__ first, int32_t* __restrict__ qmax) {
  RGBL_DYN_SHARED(uint32_t, s_q);
  const int q = (int)blockIdx.y, tid = (int)threadIdx.x, lane = lane_id(), w = wave_id();
  const int q0 = q_off[q], nq = q_off[q + 1] - q0;
  for (int i = tid; i < nq; i += (int)blockDim.x) s_q[i] = q_id[q0 + i];
  __syncthreads();
  const size_t row = (size_t)q * (size_t)n_ent;
  const uint32_t qlo = nq > 0 ? s_q[0] : 1u, qhi = nq > 0 ? s_q[nq - 1] : 0u;
  int wmax = 0;
  for (int e = (int)blockIdx.x * kKfdbWaves + w; e < n_ent; e += (int)gridDim.x * kKfdbWaves) {
    const KfdbEntry E = ent[e];
    int c = 0;
    uint32_t f = 0xffffffffu;
    // excluded entries (spConnectedKF) are no shared entries: they count nothing and never feed the maximum
    if (E.n > 0 && nq > 0 && !(excl && excl[row + e])) {
      for (int base = 0; base < E.n; base += kWave) {   // wave-uniform trip count: every lane reaches the ballot
        const int i = base + lane;
        uint32_t id = 0;
        bool hit = false;
        if (i < E.n) {
          id = arena_id[(size_t)E.off + i];
          hit = id >= qlo && id <= qhi && kfdb_find(s_q, nq, id) >= 0;
        }
        const unsigned long long m = __ballot(hit);
        if (m) {
          if (c == 0) f = __shfl(id, __ffsll((long long)m) - 1);   // ids ascend: the first hit is the smallest common word
          c += __popcll(m);
        }
      }
    }
    if (lane == 0) { count[row + e] = c; first[row + e] = f; }
    wmax = imax(wmax, c);
  }
  if (lane == 0 && wmax > 0) atomicMax(&qmax[q], wmax);   // integer maximum: order-independent
}

// Same grid.  minCommonWords = int(maxCommonWords * 0.8f) (KeyFrameDatabase.cc:648, :769: an int times a float, truncated),
// raised to the caller's floor; entries with count > minCommonWords are scored.  A workgroup none of whose entries passes
// leaves before it stages anything.
__global__ __launch_bounds__(256) void k_kfdb_score(const KfdbEntry* __restrict__ ent, int n_ent, const uint32_t* __restrict__ arena_id,
                                                    const double* __restrict__ arena_val, const int32_t* __restrict__ q_off,
                                                    const uint32_t* __restrict__ q_id, const double* __restrict__ q_val,
                                                    const int32_t* __restrict__ q_floor, const int32_t* __restrict__ count,
                                                    const int32_t* __restrict__ qmax, float* __restrict__ score) {
  RGBL_DYN_SHARED(double, s_mem);
  double* s_terms = s_mem;
  int* s_any = reinterpret_cast<int*>(s_mem + kKfdbWaves * kWave);
  uint32_t* s_q = reinterpret_cast<uint32_t*>(s_mem + kKfdbScoreHead);
  const int q = (int)blockIdx.y, tid = (int)threadIdx.x, lane = lane_id(), w = wave_id();
  const int q0 = q_off[q], nq = q_off[q + 1] - q0;
  const size_t row = (size_t)q * (size_t)n_ent;
  int minc = (int)((float)qmax[q] * 0.8f);
  minc = imax(minc, q_floor[q]);
  if (tid == 0) *s_any = 0;
  __syncthreads();
  bool need = false;
  for (int e = (int)blockIdx.x * kKfdbWaves + w; e < n_ent; e += (int)gridDim.x * kKfdbWaves) need = need || count[row + e] > minc;
  if (need && lane == 0) *s_any = 1;
  __syncthreads();
  if (!*s_any) return;
  for (int i = tid; i < nq; i += (int)blockDim.x) s_q[i] = q_id[q0 + i];
  __syncthreads();
  double* terms = s_terms + w * kWave;
  for (int e = (int)blockIdx.x * kKfdbWaves + w; e < n_ent; e += (int)gridDim.x * kKfdbWaves) {
    if (count[row + e] <= minc) continue;   // wave-uniform
    const KfdbEntry E = ent[e];
    double s = 0.0;
    for (int base = 0; base < E.n; base += kWave) {
      const int i = base + lane;
      bool hit = false;
      double term = 0.0;
      if (i < E.n) {
        const int pos = kfdb_find(s_q, nq, arena_id[(size_t)E.off + i]);
        if (pos >= 0) {
          hit = true;
          const double vi = q_val[q0 + pos], wi = arena_val[(size_t)E.off + i];
          term = fabs(vi - wi) - fabs(vi) - fabs(wi);
        }
      }
      const unsigned long long m = __ballot(hit);
      if (m) {
        if (hit) terms[__popcll(m & lanemask_lt())] = term;   // ascending word order
        wave_sync();
        const int k = __popcll(m);
        for (int j = 0; j < k; ++j) s += terms[j];            // one after another, as the merge loop of L1Scoring::score adds them
        wave_sync();
      }
    }
    if (lane == 0) score[row + e] = (float)(-s / 2.0);
  }
}

// grid = (live entries), block = 256
__global__ __launch_bounds__(256) void k_kfdb_compact(const KfdbMove* __restrict__ moves, const uint32_t* __restrict__ src_id,
                                                      const double* __restrict__ src_val, uint32_t* __restrict__ dst_id,
                                                      double* __restrict__ dst_val) {
  const KfdbMove m = moves[blockIdx.x];
  for (int i = (int)threadIdx.x; i < m.n; i += (int)blockDim.x) {
    dst_id[(size_t)m.dst + i] = src_id[(size_t)m.src + i];
    dst_val[(size_t)m.dst + i] = src_val[(size_t)m.src + i];
  }
}

static inline size_t kfdb_align(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace rgbl

using namespace rgbl;

struct rgbl_kf_database {
  int device = 0, n_vocab = 0;
  std::mutex mu;                      // KeyFrameDatabase::mMutex: add (loop closing), erase (SetBadFlag), query (tracking)
  hipStream_t stream = nullptr;
  // arena of (id, value) pairs
  uint32_t* d_id = nullptr;
  double* d_val = nullptr;
  long long cap = 0, used = 0, dead_words = 0, live_words = 0;
  int n_compactions = 0;
  // entries in add order: the slot index IS the sequence number the order key needs (compaction keeps the relative order,
  // an erased key frame that comes back gets a new slot at the end)
  struct Host { long long kf_id; int32_t map_id; };
  std::vector<Host> host;
  std::vector<KfdbEntry> ent;
  std::unordered_map<long long, int> live;   // kf_id -> slot
  KfdbEntry* d_ent = nullptr;
  size_t ent_cap = 0;
  bool ent_dirty = false;
  // query staging: one page-locked block up, one back
  uint8_t* d_in = nullptr; uint8_t* h_in = nullptr; size_t in_cap = 0;
  uint8_t* d_res = nullptr; uint8_t* h_res = nullptr; size_t res_cap = 0;
  std::vector<int> order;
  KernelTimer timer;
};

static int kfdb_grow_block(uint8_t** d, uint8_t** h, size_t* cap, size_t need) {
  if (need <= *cap) return RGBL_OK;
  size_t n = std::max<size_t>(*cap * 2, 1 << 16);
  while (n < need) n *= 2;
  if (*d) (void)hipFree(*d);
  if (*h) (void)hipHostFree(*h);
  *d = nullptr; *h = nullptr; *cap = 0;
  RGBL_HIP(rgbl::device_alloc(d, n));
  RGBL_HIP(rgbl::pinned_alloc(h, n));
  *cap = n;
  return RGBL_OK;
}

// the arena holds at least `need` words afterwards (doubling; the words in use move along)
static int kfdb_reserve(rgbl_kf_database* db, long long need) {
  if (need <= db->cap) return RGBL_OK;
  long long n = std::max<long long>(db->cap, 1 << 16);
  while (n < need) n *= 2;
  if (n > 0x7fffffffll) { set_error("key-frame database: more than 2^31 words"); return RGBL_ERR_OVERFLOW; }
  uint32_t* nid = nullptr;
  double* nval = nullptr;
  RGBL_HIP(rgbl::device_alloc(&nid, sizeof(uint32_t) * (size_t)n));
  if (rgbl::device_alloc(&nval, sizeof(double) * (size_t)n) != hipSuccess) { (void)hipFree(nid); set_error("hipMalloc of the arena failed"); return RGBL_ERR_HIP; }
  if (db->used > 0) {
    (void)hipMemcpyAsync(nid, db->d_id, sizeof(uint32_t) * (size_t)db->used, hipMemcpyDeviceToDevice, db->stream);
    (void)hipMemcpyAsync(nval, db->d_val, sizeof(double) * (size_t)db->used, hipMemcpyDeviceToDevice, db->stream);
  }
  const hipError_t e = hipStreamSynchronize(db->stream);
  if (e != hipSuccess) { (void)hipFree(nid); (void)hipFree(nval); set_error("arena growth failed: %s", hipGetErrorString(e)); return RGBL_ERR_HIP; }
  if (db->d_id) (void)hipFree(db->d_id);
  if (db->d_val) (void)hipFree(db->d_val);
  db->d_id = nid; db->d_val = nval; db->cap = n;
  return RGBL_OK;
}

// drops the tombstones: live entries move, in order, to the front of a fresh arena
static int kfdb_compact(rgbl_kf_database* db) {
  std::vector<KfdbMove> moves;
  std::vector<rgbl_kf_database::Host> host;
  std::vector<KfdbEntry> ent;
  long long used = 0;
  for (size_t i = 0; i < db->ent.size(); ++i) {
    if (db->ent[i].n < 0) continue;
    moves.push_back(KfdbMove{db->ent[i].off, (uint32_t)used, db->ent[i].n});
    host.push_back(db->host[i]);
    ent.push_back(KfdbEntry{(uint32_t)used, db->ent[i].n});
    used += db->ent[i].n;
  }
  if (!moves.empty() && used > 0) {
    uint32_t* nid = nullptr;
    double* nval = nullptr;
    KfdbMove* d_moves = nullptr;
    RGBL_HIP(rgbl::device_alloc(&nid, sizeof(uint32_t) * (size_t)db->cap));
    if (rgbl::device_alloc(&nval, sizeof(double) * (size_t)db->cap) != hipSuccess || rgbl::device_alloc(&d_moves, sizeof(KfdbMove) * moves.size()) != hipSuccess) {
      (void)hipFree(nid);
      if (nval) (void)hipFree(nval);
      set_error("hipMalloc for the compaction failed");
      return RGBL_ERR_HIP;
    }
    (void)hipMemcpyAsync(d_moves, moves.data(), sizeof(KfdbMove) * moves.size(), hipMemcpyHostToDevice, db->stream);
    hipLaunchKernelGGL(k_kfdb_compact, dim3((unsigned)moves.size()), dim3(256), 0, db->stream, d_moves, db->d_id, db->d_val, nid, nval);
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(db->stream);
    (void)hipFree(d_moves);
    if (e1 != hipSuccess || e2 != hipSuccess) {
      (void)hipFree(nid); (void)hipFree(nval);
      set_error("compaction failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
      return RGBL_ERR_HIP;
    }
    (void)hipFree(db->d_id);
    (void)hipFree(db->d_val);
    db->d_id = nid; db->d_val = nval;
  }
  db->host.swap(host);
  db->ent.swap(ent);
  db->live.clear();
  for (size_t i = 0; i < db->host.size(); ++i) db->live[db->host[i].kf_id] = (int)i;
  db->used = used;
  db->dead_words = 0;
  db->ent_dirty = true;
  ++db->n_compactions;
  return RGBL_OK;
}

static int kfdb_bury(rgbl_kf_database* db, int slot) {
  db->dead_words += db->ent[slot].n;
  db->live_words -= db->ent[slot].n;
  db->ent[slot].n = -1;
  db->live.erase(db->host[slot].kf_id);
  db->ent_dirty = true;
  return RGBL_OK;
}
static int kfdb_maybe_compact(rgbl_kf_database* db) {
  // "more than half of it is dead", in words; a database of nothing but tombstones gives its slots back as well
  if (db->dead_words * 2 > db->used || (db->live.empty() && !db->ent.empty())) return kfdb_compact(db);
  return RGBL_OK;
}

extern "C" {

int rgbl_kfdb_create(int device, int n_vocab_words, rgbl_kf_database** out) {
  if (!out) { set_error("null argument"); return RGBL_ERR_INVALID; }
  *out = nullptr;
  if (n_vocab_words < 1) { set_error("key-frame database: a vocabulary of %d words", n_vocab_words); return RGBL_ERR_INVALID; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_error("no HIP device: librgbl_frontend has no CPU fallback"); return RGBL_ERR_NO_DEVICE; }
  if (device < 0 || device >= ndev) { set_error("device %d out of range", device); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(device));
  rgbl_kf_database* db = new rgbl_kf_database;
  db->device = device;
  db->n_vocab = n_vocab_words;
  if (hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking) != hipSuccess) { delete db; set_error("hipStreamCreate failed"); return RGBL_ERR_HIP; }
  const int rc = kfdb_reserve(db, 1);
  if (rc != RGBL_OK) { rgbl_kfdb_destroy(db); return rc; }
  *out = db;
  return RGBL_OK;
}

void rgbl_kfdb_destroy(rgbl_kf_database* db) {
  if (!db) return;
  (void)hipSetDevice(db->device);
  if (db->stream) (void)hipStreamSynchronize(db->stream);
  db->timer.collect();
  if (db->d_id) (void)hipFree(db->d_id);
  if (db->d_val) (void)hipFree(db->d_val);
  if (db->d_ent) (void)hipFree(db->d_ent);
  if (db->d_in) (void)hipFree(db->d_in);
  if (db->h_in) (void)hipHostFree(db->h_in);
  if (db->d_res) (void)hipFree(db->d_res);
  if (db->h_res) (void)hipHostFree(db->h_res);
  if (db->stream) (void)hipStreamDestroy(db->stream);
  delete db;
}

int rgbl_kfdb_add(rgbl_kf_database* db, int64_t kf_id, int32_t map_id, int n_words, const uint32_t* word_id, const double* word_val) {
  if (!db || n_words < 0 || (n_words > 0 && (!word_id || !word_val))) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  for (int i = 0; i < n_words; ++i) {
    if (word_id[i] >= (uint32_t)db->n_vocab) { set_error("key-frame database: word id %u, the vocabulary has %d words", word_id[i], db->n_vocab); return RGBL_ERR_INVALID; }
    if (i > 0 && word_id[i] <= word_id[i - 1]) { set_error("key-frame database: word ids must ascend (position %d)", i); return RGBL_ERR_INVALID; }
  }
  std::lock_guard<std::mutex> lock(db->mu);
  if (db->live.count(kf_id)) { set_error("key-frame database: key frame %lld is already in the database", (long long)kf_id); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(db->device));
  RGBL_TRY(kfdb_reserve(db, db->used + n_words));
  if (n_words > 0) {
    StreamDrain drain(db->stream);
    RGBL_HIP(hipMemcpyAsync(db->d_id + db->used, word_id, sizeof(uint32_t) * (size_t)n_words, hipMemcpyHostToDevice, db->stream));
    RGBL_HIP(hipMemcpyAsync(db->d_val + db->used, word_val, sizeof(double) * (size_t)n_words, hipMemcpyHostToDevice, db->stream));
  }
  db->live[kf_id] = (int)db->ent.size();
  db->host.push_back(rgbl_kf_database::Host{(long long)kf_id, map_id});
  db->ent.push_back(KfdbEntry{(uint32_t)db->used, n_words});
  db->used += n_words;
  db->live_words += n_words;
  db->ent_dirty = true;
  return RGBL_OK;
}

int rgbl_kfdb_erase(rgbl_kf_database* db, int64_t kf_id) {
  if (!db) { set_error("null handle"); return RGBL_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(db->mu);
  auto it = db->live.find(kf_id);
  if (it == db->live.end()) return RGBL_OK;   // KeyFrameDatabase::erase of a key frame that is in no list changes nothing
  RGBL_HIP(hipSetDevice(db->device));
  kfdb_bury(db, it->second);
  return kfdb_maybe_compact(db);
}

int rgbl_kfdb_clear(rgbl_kf_database* db) {
  if (!db) { set_error("null handle"); return RGBL_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(db->mu);
  db->host.clear(); db->ent.clear(); db->live.clear();
  db->used = db->dead_words = db->live_words = 0;
  db->ent_dirty = true;
  return RGBL_OK;
}

int rgbl_kfdb_clear_map(rgbl_kf_database* db, int32_t map_id) {
  if (!db) { set_error("null handle"); return RGBL_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(db->mu);
  RGBL_HIP(hipSetDevice(db->device));
  for (size_t i = 0; i < db->ent.size(); ++i)
    if (db->ent[i].n >= 0 && db->host[i].map_id == map_id) kfdb_bury(db, (int)i);
  return kfdb_maybe_compact(db);
}

int rgbl_kfdb_set_map(rgbl_kf_database* db, int64_t kf_id, int32_t map_id) {
  if (!db) { set_error("null handle"); return RGBL_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(db->mu);
  auto it = db->live.find(kf_id);
  if (it != db->live.end()) db->host[it->second].map_id = map_id;
  return RGBL_OK;
}

int rgbl_kfdb_size(rgbl_kf_database* db, int* n_alive, long long* n_words) {
  if (!db) { set_error("null handle"); return RGBL_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(db->mu);
  if (n_alive) *n_alive = (int)db->live.size();
  if (n_words) *n_words = db->live_words;
  return RGBL_OK;
}

int rgbl_kfdb_arena_info(rgbl_kf_database* db, long long* used_words, long long* cap_words, int* n_slots, int* n_compactions) {
  if (!db) { set_error("null handle"); return RGBL_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(db->mu);
  if (used_words) *used_words = db->used;
  if (cap_words) *cap_words = db->cap;
  if (n_slots) *n_slots = (int)db->ent.size();
  if (n_compactions) *n_compactions = db->n_compactions;
  return RGBL_OK;
}

int rgbl_kfdb_query_batch(rgbl_kf_database* db, int n_queries, const int32_t* word_off, const uint32_t* word_id, const double* word_val,
                          const int32_t* excl_off, const int64_t* excl_kf, const int32_t* min_words_floor, int cap,
                          int64_t* share_kf, int32_t* share_words, float* share_score, uint8_t* scored, int32_t* n_share,
                          int32_t* max_common_words, int32_t* min_common_words) {
  if (!db || n_queries < 1 || !word_off || !n_share || !max_common_words || !min_common_words || cap < 0 ||
      (cap > 0 && (!share_kf || !share_words || !share_score || !scored)) || word_off[0] != 0) {
    set_error("invalid argument");
    return RGBL_ERR_INVALID;
  }
  if (n_queries > 65535) { set_error("key-frame database: %d queries in one call (at most 65535: one grid row each)", n_queries); return RGBL_ERR_INVALID; }
  const int Q = n_queries;
  for (int q = 0; q < Q; ++q) {
    const int n = word_off[q + 1] - word_off[q];
    if (n < 0 || n > kKfdbMaxQueryWords) { set_error("key-frame database: a query of %d words (at most %d)", n, kKfdbMaxQueryWords); return RGBL_ERR_INVALID; }
    if (excl_off && (excl_off[q + 1] < excl_off[q] || excl_off[0] != 0)) { set_error("key-frame database: exclusion offsets must not descend"); return RGBL_ERR_INVALID; }
  }
  const int W = word_off[Q];
  if (W > 0 && (!word_id || !word_val)) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  if (excl_off && excl_off[Q] > 0 && !excl_kf) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  int max_nq = 0;
  for (int q = 0; q < Q; ++q) {
    max_nq = std::max(max_nq, word_off[q + 1] - word_off[q]);
    for (int i = word_off[q]; i < word_off[q + 1]; ++i) {
      if (word_id[i] >= (uint32_t)db->n_vocab) { set_error("key-frame database: word id %u, the vocabulary has %d words", word_id[i], db->n_vocab); return RGBL_ERR_INVALID; }
      if (i > word_off[q] && word_id[i] <= word_id[i - 1]) { set_error("key-frame database: word ids must ascend (query %d)", q); return RGBL_ERR_INVALID; }
    }
  }
  std::lock_guard<std::mutex> lock(db->mu);
  const int E = (int)db->ent.size();
  for (int q = 0; q < Q; ++q) n_share[q] = max_common_words[q] = min_common_words[q] = 0;
  if (E == 0 || W == 0) {   // lKFsSharingWords.empty()
    for (int q = 0; q < Q; ++q) min_common_words[q] = min_words_floor ? std::max(0, min_words_floor[q]) : 0;
    return RGBL_OK;
  }
  if ((long long)Q * E > 0x3fffffffll) { set_error("key-frame database: %d queries over %d entries in one call", Q, E); return RGBL_ERR_INVALID; }
  RGBL_HIP(hipSetDevice(db->device));

  // one block up: offsets | floors | maxima (zero) | ids | values | exclusion mask
  const bool any_excl = excl_off && excl_off[Q] > 0;
  const size_t o_off = 0, o_floor = kfdb_align(o_off + 4 * ((size_t)Q + 1)), o_max = kfdb_align(o_floor + 4 * (size_t)Q),
               o_id = kfdb_align(o_max + 4 * (size_t)Q), o_val = kfdb_align(o_id + 4 * (size_t)W), o_excl = kfdb_align(o_val + 8 * (size_t)W),
               in_bytes = o_excl + (any_excl ? (size_t)Q * E : 0);
  RGBL_TRY(kfdb_grow_block(&db->d_in, &db->h_in, &db->in_cap, in_bytes));
  const size_t QE = (size_t)Q * E;
  const size_t r_count = 0, r_first = kfdb_align(4 * QE), r_score = r_first + kfdb_align(4 * QE), res_bytes = r_score + kfdb_align(4 * QE);
  RGBL_TRY(kfdb_grow_block(&db->d_res, &db->h_res, &db->res_cap, res_bytes));
  memcpy(db->h_in + o_off, word_off, 4 * ((size_t)Q + 1));
  int32_t* h_floor = reinterpret_cast<int32_t*>(db->h_in + o_floor);
  for (int q = 0; q < Q; ++q) h_floor[q] = min_words_floor ? std::max(0, min_words_floor[q]) : 0;
  memset(db->h_in + o_max, 0, 4 * (size_t)Q);
  memcpy(db->h_in + o_id, word_id, 4 * (size_t)W);
  memcpy(db->h_in + o_val, word_val, 8 * (size_t)W);
  if (any_excl) {
    uint8_t* mask = db->h_in + o_excl;
    memset(mask, 0, QE);
    for (int q = 0; q < Q; ++q)
      for (int i = excl_off[q]; i < excl_off[q + 1]; ++i) {
        auto it = db->live.find((long long)excl_kf[i]);
        if (it != db->live.end()) mask[(size_t)q * E + it->second] = 1;
      }
  }
  {
    StreamDrain drain(db->stream);
    if (db->ent_dirty) {
      if ((size_t)E > db->ent_cap) {
        if (db->d_ent) (void)hipFree(db->d_ent);
        db->d_ent = nullptr; db->ent_cap = 0;
        const size_t n = std::max<size_t>(1024, (size_t)E * 2);
        RGBL_HIP(rgbl::device_alloc(&db->d_ent, sizeof(KfdbEntry) * n));
        db->ent_cap = n;
      }
      RGBL_HIP(hipMemcpyAsync(db->d_ent, db->ent.data(), sizeof(KfdbEntry) * (size_t)E, hipMemcpyHostToDevice, db->stream));
      db->ent_dirty = false;
    }
    RGBL_HIP(hipMemcpyAsync(db->d_in, db->h_in, in_bytes, hipMemcpyHostToDevice, db->stream));
    const int32_t* d_off = reinterpret_cast<const int32_t*>(db->d_in + o_off);
    const int32_t* d_floor = reinterpret_cast<const int32_t*>(db->d_in + o_floor);
    int32_t* d_max = reinterpret_cast<int32_t*>(db->d_in + o_max);
    const uint32_t* d_qid = reinterpret_cast<const uint32_t*>(db->d_in + o_id);
    const double* d_qval = reinterpret_cast<const double*>(db->d_in + o_val);
    const uint8_t* d_excl = any_excl ? db->d_in + o_excl : nullptr;
    int32_t* d_count = reinterpret_cast<int32_t*>(db->d_res + r_count);
    uint32_t* d_first = reinterpret_cast<uint32_t*>(db->d_res + r_first);
    float* d_score = reinterpret_cast<float*>(db->d_res + r_score);
    // enough workgroups to fill the card, few enough that a workgroup's staging of the query is shared by several entries
    const int groups = std::max(1, std::min((E + kKfdbWaves - 1) / kKfdbWaves, std::max(1, 2048 / Q)));
    const dim3 grid((unsigned)groups, (unsigned)Q);
    const size_t lds_ids = kfdb_align(4 * (size_t)std::max(max_nq, 1));
    db->timer.begin("k_kfdb_common", db->stream);
    hipLaunchKernelGGL(k_kfdb_common, grid, dim3(kKfdbWaves * kWave), lds_ids, db->stream, (const KfdbEntry*)db->d_ent, E,
                       (const uint32_t*)db->d_id, d_off, d_qid, d_excl, d_count, d_first, d_max);
    db->timer.end(db->stream);
    RGBL_HIP(hipGetLastError());
    db->timer.begin("k_kfdb_score", db->stream);
    hipLaunchKernelGGL(k_kfdb_score, grid, dim3(kKfdbWaves * kWave), lds_ids + 8 * (size_t)kKfdbScoreHead, db->stream,
                       (const KfdbEntry*)db->d_ent, E, (const uint32_t*)db->d_id, (const double*)db->d_val, d_off, d_qid, d_qval,
                       d_floor, (const int32_t*)d_count, (const int32_t*)d_max, d_score);
    db->timer.end(db->stream);
    RGBL_HIP(hipGetLastError());
    RGBL_HIP(hipMemcpyAsync(db->h_res, db->d_res, res_bytes, hipMemcpyDeviceToHost, db->stream));
    RGBL_HIP(hipStreamSynchronize(db->stream));
  }

  // lKFsSharingWords in the reference's order: ascending (smallest common word, position in that word's list = add order)
  int rc = RGBL_OK;
  for (int q = 0; q < Q; ++q) {
    const int32_t* cnt = reinterpret_cast<const int32_t*>(db->h_res + r_count) + (size_t)q * E;
    const uint32_t* fst = reinterpret_cast<const uint32_t*>(db->h_res + r_first) + (size_t)q * E;
    const float* sc = reinterpret_cast<const float*>(db->h_res + r_score) + (size_t)q * E;
    db->order.clear();
    int mx = 0;
    for (int e = 0; e < E; ++e)
      if (cnt[e] > 0) { db->order.push_back(e); mx = std::max(mx, cnt[e]); }
    std::sort(db->order.begin(), db->order.end(), [&](int a, int b) { return fst[a] != fst[b] ? fst[a] < fst[b] : a < b; });
    int minc = (int)((float)mx * 0.8f);
    minc = std::max(minc, h_floor[q]);
    const int n = (int)db->order.size();
    n_share[q] = n;
    max_common_words[q] = mx;
    min_common_words[q] = minc;
    if (n > cap) {
      set_error("key-frame database: query %d shares words with %d key frames, room for %d", q, n, cap);
      rc = RGBL_ERR_CAPACITY;
      continue;
    }
    for (int i = 0; i < n; ++i) {
      const int e = db->order[i];
      const size_t o = (size_t)q * cap + i;
      share_kf[o] = db->host[e].kf_id;
      share_words[o] = cnt[e];
      scored[o] = cnt[e] > minc;
      if (scored[o]) share_score[o] = sc[e];
    }
  }
  return rc;
}

int rgbl_kfdb_query(rgbl_kf_database* db, const rgbl_kfdb_query_input* in, rgbl_kfdb_query_output* out) {
  if (!db || !in || !out || in->n_words < 0 || in->n_excluded < 0) { set_error("invalid argument"); return RGBL_ERR_INVALID; }
  const int32_t off[2] = {0, in->n_words}, xoff[2] = {0, in->n_excluded};
  return rgbl_kfdb_query_batch(db, 1, off, in->word_id, in->word_val, in->n_excluded > 0 ? xoff : nullptr, in->excluded_kf,
                               &in->min_words_floor, out->cap, out->share_kf, out->share_words, out->share_score, out->scored,
                               &out->n_share, &out->max_common_words, &out->min_common_words);
}

int rgbl_kfdb_profile(rgbl_kf_database* db, int enable) {
  if (!db) { set_error("null handle"); return RGBL_ERR_INVALID; }
  std::lock_guard<std::mutex> lock(db->mu);
  RGBL_HIP(hipStreamSynchronize(db->stream));
  db->timer.reset();
  db->timer.enabled = enable != 0;
  return RGBL_OK;
}

int rgbl_kfdb_profile_read(rgbl_kf_database* db, const char** names, double* total_ms, long* launches, int cap) {
  if (!db) return 0;
  std::lock_guard<std::mutex> lock(db->mu);
  (void)hipStreamSynchronize(db->stream);
  db->timer.collect();
  const int n = (int)db->timer.names.size();
  for (int i = 0; i < n && i < cap; ++i) {
    if (names) names[i] = db->timer.names[i].c_str();
    if (total_ms) total_ms[i] = db->timer.total_ms[i];
    if (launches) launches[i] = db->timer.count[i];
  }
  return n;
}

}  // extern "C"
