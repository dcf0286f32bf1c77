// tiles.cpp -- libvgs_tiles.so: the native tiled driver of include/vgs_tiles.h.  Host C++ over the C-ABI of
// include/vgs.h; the collectives are RCCL calls (ncclAllGather / ncclBroadcast on the caller's communicator) or, for tests
// that run several ranks on one GPU, threads of one process meeting in shared memory.  The Python twin of this file is
// vgs-svgs-segmentation_amd/dist.py (same protocol, same labels); protocol notes live there and in DESIGN.md section 6.
//
// The agreed-status protocol, once.  A rank that fails LOCALLY between two collectives must not leave while its peers are already inside
// the next one (they would wait for ever: ADVICE r3).  So a failing step only records its status (`carry`: TCARRY, inject), the rank
// still joins the next collective with that status in its payload's header, and every rank reads the headers and leaves with the same
// verdict (agreed): the failing rank its own error, the others VGS_E_PEER naming the lowest failing rank.  A failure BEHIND a call's last
// collective is returned and kept in t->pending (behind_collective), and the next collective's header carries it.  The collectives
// after vgs_tiles_run all read: open_collective (guard, carry = pending, injection) -> own records, header filled in -> exchange (ONE
// all_gather_varlen + the scan of the headers) -> check_payloads / fold -> behind_collective(finish on this rank's GPU).
// vgs_tiles_set_points, chain_grid and the boundary exchange of vgs_tiles_run carry the status in payloads of their own shapes and share
// first_bad_rank and agreed.
// The per-segment tables exist for two labellings, the run's own node labels and a caller's per-point labels (Labelling), and each table
// kind has ONE driver that serves both: moment_collective (descriptors), extent_collective (boxes), attribute_collective<Codec> (field
// statistics, class histogram), tiles_compare (scores).  A public entry fills in the Labelling, calls the driver and places the table.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/vgs_tiles.h"

namespace {

// ------------------------------------------------------------------------------------------------ communicators
struct Comm {
  int rank = 0, world = 1;
  std::string err;
  virtual ~Comm() {}
  virtual bool all_gather(const void* send, void* recv, size_t bytes_per_rank) = 0;   // recv: world * bytes_per_rank, rank order
  virtual bool bcast(void* buf, size_t bytes, int root) = 0;
};

// threads of one process (tests: several ranks on one GPU)
struct LocalGroup {
  int world;
  std::mutex m;
  std::condition_variable cv;
  int waiting = 0;
  uint64_t generation = 0;
  bool broken = false;
  std::vector<const void*> slot;
  explicit LocalGroup(int w) : world(w), slot((size_t)w, nullptr) {}
  bool barrier() {
    std::unique_lock<std::mutex> lk(m);
    if (broken) return false;
    const uint64_t g = generation;
    if (++waiting == world) { waiting = 0; ++generation; cv.notify_all(); return true; }
    cv.wait(lk, [&] { return generation != g || broken; });
    return !broken;
  }
  void abort() { std::lock_guard<std::mutex> lk(m); broken = true; cv.notify_all(); }
};

struct LocalComm : Comm {
  LocalGroup* g;
  LocalComm(LocalGroup* grp, int r) : g(grp) { rank = r; world = grp->world; }
  bool all_gather(const void* send, void* recv, size_t bytes) override {
    g->slot[(size_t)rank] = send;
    if (!g->barrier()) { err = "local group aborted"; return false; }
    for (int r = 0; r < world; ++r) std::memcpy((char*)recv + (size_t)r * bytes, g->slot[(size_t)r], bytes);
    if (!g->barrier()) { err = "local group aborted"; return false; }
    return true;
  }
  bool bcast(void* buf, size_t bytes, int root) override {
    if (rank == root) g->slot[(size_t)root] = buf;
    if (!g->barrier()) { err = "local group aborted"; return false; }
    if (rank != root) std::memcpy(buf, g->slot[(size_t)root], bytes);
    if (!g->barrier()) { err = "local group aborted"; return false; }
    return true;
  }
};

// RCCL: payloads are staged through device buffers (the collectives move device memory over xGMI)
struct RcclComm : Comm {
  ncclComm_t comm;
  int device;
  hipStream_t stream = nullptr;
  char *d_send = nullptr, *d_recv = nullptr;
  size_t cap_send = 0, cap_recv = 0;
  RcclComm(ncclComm_t c, int r, int w, int dev) : comm(c), device(dev) { rank = r; world = w; }
  ~RcclComm() override {
    (void)hipSetDevice(device);
    if (d_send) (void)hipFree(d_send);
    if (d_recv) (void)hipFree(d_recv);
    if (stream) (void)hipStreamDestroy(stream);
  }
  bool hip_ok(hipError_t e, const char* what) { if (e != hipSuccess) { err = std::string(what) + ": " + hipGetErrorString(e); return false; } return true; }
  bool nccl_ok(ncclResult_t e, const char* what) { if (e != ncclSuccess) { err = std::string(what) + ": " + ncclGetErrorString(e); return false; } return true; }
  bool ensure(size_t send_bytes, size_t recv_bytes) {
    if (!hip_ok(hipSetDevice(device), "hipSetDevice")) return false;
    if (!stream && !hip_ok(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate")) return false;
    if (send_bytes > cap_send) { if (d_send) (void)hipFree(d_send); d_send = nullptr; if (!hip_ok(hipMalloc((void**)&d_send, send_bytes + 256), "hipMalloc")) return false; cap_send = send_bytes + 256; }
    if (recv_bytes > cap_recv) { if (d_recv) (void)hipFree(d_recv); d_recv = nullptr; if (!hip_ok(hipMalloc((void**)&d_recv, recv_bytes + 256), "hipMalloc")) return false; cap_recv = recv_bytes + 256; }
    return true;
  }
  bool all_gather(const void* send, void* recv, size_t bytes) override {
    if (!ensure(bytes, bytes * (size_t)world)) return false;
    return hip_ok(hipMemcpyAsync(d_send, send, bytes, hipMemcpyHostToDevice, stream), "H2D") &&
           nccl_ok(ncclAllGather(d_send, d_recv, bytes, ncclChar, comm, stream), "ncclAllGather") &&
           hip_ok(hipMemcpyAsync(recv, d_recv, bytes * (size_t)world, hipMemcpyDeviceToHost, stream), "D2H") &&
           hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize");
  }
  bool bcast(void* buf, size_t bytes, int root) override {
    if (!ensure(bytes, bytes)) return false;
    return hip_ok(hipMemcpyAsync(d_send, buf, bytes, hipMemcpyHostToDevice, stream), "H2D") &&
           nccl_ok(ncclBroadcast(d_send, d_recv, bytes, ncclChar, root, comm, stream), "ncclBroadcast") &&
           hip_ok(hipMemcpyAsync(buf, d_recv, bytes, hipMemcpyDeviceToHost, stream), "D2H") &&
           hip_ok(hipStreamSynchronize(stream), "hipStreamSynchronize");
  }
};

// the caller's own transport (MPI, gloo, a test harness): two C callbacks over host buffers
struct CallbackComm : Comm {
  vgs_tiles_callbacks cb;
  CallbackComm(const vgs_tiles_callbacks& c, int r, int w) : cb(c) { rank = r; world = w; }
  bool all_gather(const void* send, void* recv, size_t bytes) override {
    if (cb.all_gather(cb.user, send, recv, (uint64_t)bytes) != 0) { err = "caller's all_gather callback failed"; return false; }
    return true;
  }
  bool bcast(void* buf, size_t bytes, int root) override {
    if (cb.bcast(cb.user, buf, (uint64_t)bytes, root) != 0) { err = "caller's bcast callback failed"; return false; }
    return true;
  }
};

// arrays of different lengths: one size exchange + one padded payload exchange
template <typename T>
bool all_gather_varlen(Comm& c, const std::vector<T>& mine, std::vector<std::vector<T>>& out) {
  std::vector<int64_t> sizes((size_t)c.world);
  const int64_t n = (int64_t)mine.size();
  if (!c.all_gather(&n, sizes.data(), sizeof(int64_t))) return false;
  const int64_t m = std::max<int64_t>(*std::max_element(sizes.begin(), sizes.end()), 1);
  std::vector<T> pad((size_t)m, T()), all((size_t)m * c.world);
  std::copy(mine.begin(), mine.end(), pad.begin());
  if (!c.all_gather(pad.data(), all.data(), (size_t)m * sizeof(T))) return false;
  out.assign((size_t)c.world, {});
  for (int r = 0; r < c.world; ++r) out[(size_t)r].assign(all.begin() + (size_t)r * m, all.begin() + (size_t)r * m + sizes[(size_t)r]);
  return true;
}

// ------------------------------------------------------------------------------------------------ boundary merge
struct RankRecords { std::vector<uint64_t> code; std::vector<int32_t> root, cnt; };

// Global segments from the compact per-rank results (vgs_get_boundary_roots): the same tables on every rank from the same
// gathered inputs.  base[r] + rank-in-root-order labels the components that touch no boundary voxel (on the GPU), the
// components named by records get dense labels behind them, in the order of their first (rank, root) node.
void merge_boundary_compact(const std::vector<RankRecords>& rec, const std::vector<int64_t>& kept_local, int voxels_min,
                            std::vector<int64_t>& base, std::vector<std::vector<int32_t>>& uroot, std::vector<std::vector<int32_t>>& ulabel,
                            int64_t& kept_total) {
  const int world = (int)rec.size();
  base.assign((size_t)world, 0);
  for (int r = 1; r < world; ++r) base[(size_t)r] = base[(size_t)r - 1] + kept_local[(size_t)r - 1];
  int64_t next_label = 0;
  for (int r = 0; r < world; ++r) next_label += kept_local[(size_t)r];
  uroot.assign((size_t)world, {}); ulabel.assign((size_t)world, {});
  std::vector<int64_t> node_cnt, offset((size_t)world + 1, 0);
  std::vector<std::pair<uint64_t, int64_t>> rec_code_node;   // (code, node) of every record
  for (int r = 0; r < world; ++r) {
    const RankRecords& R = rec[(size_t)r];
    std::vector<int32_t>& ur = uroot[(size_t)r];
    ur = R.root;
    std::sort(ur.begin(), ur.end());
    ur.erase(std::unique(ur.begin(), ur.end()), ur.end());
    std::vector<int64_t> cnt_of(ur.size(), -1);
    for (size_t k = 0; k < R.root.size(); ++k) {
      const size_t j = (size_t)(std::lower_bound(ur.begin(), ur.end(), R.root[k]) - ur.begin());
      if (cnt_of[j] < 0) cnt_of[j] = R.cnt[k];   // first record of that root (every record of a root carries the same count)
      rec_code_node.emplace_back(R.code[k], offset[(size_t)r] + (int64_t)j);
    }
    for (int64_t x : cnt_of) node_cnt.push_back(x < 0 ? 0 : x);
    offset[(size_t)r + 1] = offset[(size_t)r] + (int64_t)ur.size();
  }
  const int64_t n = offset[(size_t)world];
  kept_total = next_label;
  if (n == 0) return;
  std::vector<int64_t> parent((size_t)n);
  std::iota(parent.begin(), parent.end(), 0);
  auto find = [&](int64_t x) { while (parent[(size_t)x] != x) { parent[(size_t)x] = parent[(size_t)parent[(size_t)x]]; x = parent[(size_t)x]; } return x; };
  std::stable_sort(rec_code_node.begin(), rec_code_node.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  for (size_t k = 1; k < rec_code_node.size(); ++k)
    if (rec_code_node[k].first == rec_code_node[k - 1].first) {   // records of all ranks that share a code name the same segment
      int64_t a = find(rec_code_node[k - 1].second), b = find(rec_code_node[k].second);
      if (a != b) { if (a < b) parent[(size_t)b] = a; else parent[(size_t)a] = b; }   // the smaller node index is the root = the component's first node
    }
  std::vector<int64_t> total((size_t)n, 0);
  for (int64_t x = 0; x < n; ++x) total[(size_t)find(x)] += node_cnt[(size_t)x];
  std::vector<int64_t> label_of((size_t)n, -1);
  for (int64_t x = 0; x < n; ++x)   // roots in ascending node order = components in the order of their first node
    if (parent[(size_t)x] == x && total[(size_t)x] > voxels_min) label_of[(size_t)x] = next_label++;
  for (int r = 0; r < world; ++r) {
    const size_t m = uroot[(size_t)r].size();
    ulabel[(size_t)r].resize(m);
    for (size_t j = 0; j < m; ++j) ulabel[(size_t)r][j] = (int32_t)label_of[(size_t)find(offset[(size_t)r] + (int64_t)j)];
  }
  kept_total = next_label;
}

// ------------------------------------------------------------------------------------------------ descriptor moments
// One rank's moments of one global label (vgs_get_own_segment_moments); the payload of the descriptor exchange.  Its first entry is the
// header: label = the rank's status word, n_points = its record count.
struct MomentRec {
  int32_t label = 0, n_nodes = 0;
  int64_t n_points = 0;
  float bbox[6] = {0, 0, 0, 0, 0, 0};
  float anchor[3] = {0, 0, 0};
  float pad = 0;
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};
static_assert(sizeof(MomentRec) == 128, "MomentRec is the exchange's wire format");

MomentRec pack_moment(const int32_t* label, const int64_t* n_points, const int32_t* n_nodes, const float* bbox6, const float* anchor3, const double* s9, size_t i) {
  MomentRec m;
  m.label = label[i]; m.n_nodes = n_nodes[i]; m.n_points = n_points[i];
  for (int a = 0; a < 6; ++a) m.bbox[a] = bbox6[6 * i + a];
  for (int a = 0; a < 3; ++a) m.anchor[a] = anchor3[3 * i + a];
  for (int f = 0; f < 9; ++f) m.s[f] = s9[9 * i + f];
  return m;
}

// The moments of every global label 0 .. K-1 from the ranks' records, the same bytes on every rank: per label, ranks in ascending order.
// The anchor is the lowest rank's with own points; another rank's sums move to it by delta = a_r - a (exact in fp64: a float minus a
// float): S1 += S1_r + n_r delta, S2 += S2_r + S1_r delta^T + delta S1_r^T + n_r delta delta^T.  Counts add, boxes take min / max.
// Returns false if a record names a label outside 0 .. K-1.
bool fold_moments(const std::vector<std::vector<MomentRec>>& ranks, int64_t K, std::vector<int64_t>& npts, std::vector<int32_t>& nnodes,
                  std::vector<float>& bbox, std::vector<float>& anchor, std::vector<double>& s9) {
  const float inf = __builtin_huge_valf();
  npts.assign((size_t)K, 0); nnodes.assign((size_t)K, 0); anchor.assign(3 * (size_t)K, 0.0f); s9.assign(9 * (size_t)K, 0.0);
  bbox.assign(6 * (size_t)K, 0.0f);
  for (int64_t k = 0; k < K; ++k) for (int a = 0; a < 3; ++a) { bbox[6 * (size_t)k + a] = inf; bbox[6 * (size_t)k + 3 + a] = -inf; }
  for (const std::vector<MomentRec>& R : ranks)
    for (const MomentRec& m : R) {
      if (m.label < 0 || (int64_t)m.label >= K) return false;
      const size_t k = (size_t)m.label;
      nnodes[k] += m.n_nodes;
      for (int a = 0; a < 3; ++a) { bbox[6 * k + a] = std::min(bbox[6 * k + a], m.bbox[a]); bbox[6 * k + 3 + a] = std::max(bbox[6 * k + 3 + a], m.bbox[3 + a]); }
      if (m.n_points <= 0) continue;
      double* S = s9.data() + 9 * k;
      if (npts[k] == 0) {   // the first rank with points: its anchor, its sums as they are
        for (int a = 0; a < 3; ++a) anchor[3 * k + a] = m.anchor[a];
        for (int f = 0; f < 9; ++f) S[f] = m.s[f];
        npts[k] = m.n_points;
        continue;
      }
      const double n = (double)m.n_points;
      double d[3];
      for (int a = 0; a < 3; ++a) d[a] = (double)m.anchor[a] - (double)anchor[3 * k + a];
      for (int a = 0; a < 3; ++a) S[a] += m.s[a] + n * d[a];
      static const int I[6] = {0, 0, 0, 1, 1, 2}, J[6] = {0, 1, 2, 1, 2, 2};
      for (int f = 0; f < 6; ++f) {
        const int i = I[f], j = J[f];
        S[3 + f] += m.s[3 + f] + m.s[i] * d[j] + d[i] * m.s[j] + n * d[i] * d[j];
      }
      npts[k] += m.n_points;
    }
  return true;
}

// ------------------------------------------------------------------------------------------------ segment graph
// One edge of one rank's partial table (vgs_get_own_segment_graph); the payload of the graph exchange.  Its first entry is the header:
// a = the rank's status word, n_pairs = its record count.
struct EdgeRec {
  int32_t a = 0, b = 0;
  int64_t n_pairs = 0, n_finite = 0;
  int32_t nodes_a = 0, nodes_b = 0;
  double w_sum = 0;
  float w_min = 0, w_max = 0;
};
static_assert(sizeof(EdgeRec) == 48, "EdgeRec is the exchange's wire format");

EdgeRec pack_edge(const int32_t* seg_ab, const int64_t* n_pairs, const int64_t* n_finite, const int32_t* nodes_ab, const double* w_sum, const float* w_min, const float* w_max, size_t i) {
  EdgeRec e;
  e.a = seg_ab[2 * i]; e.b = seg_ab[2 * i + 1]; e.n_pairs = n_pairs[i]; e.n_finite = n_finite[i]; e.nodes_a = nodes_ab[2 * i]; e.nodes_b = nodes_ab[2 * i + 1];
  e.w_sum = w_sum[i]; e.w_min = w_min[i]; e.w_max = w_max[i];
  return e;
}
// the inverse, into the caller's arrays (each may be NULL)
void unpack_edge(const EdgeRec& e, size_t i, int32_t* seg_ab, int64_t* n_pairs, int64_t* n_finite, int32_t* nodes_ab, double* w_sum, float* w_min, float* w_max) {
  if (seg_ab) { seg_ab[2 * i] = e.a; seg_ab[2 * i + 1] = e.b; }
  if (n_pairs) n_pairs[i] = e.n_pairs;
  if (n_finite) n_finite[i] = e.n_finite;
  if (nodes_ab) { nodes_ab[2 * i] = e.nodes_a; nodes_ab[2 * i + 1] = e.nodes_b; }
  if (w_sum) w_sum[i] = e.w_sum;
  if (w_min) w_min[i] = e.w_min;
  if (w_max) w_max[i] = e.w_max;
}

// The edge table of the whole scene from the ranks' partial tables, the same bytes on every rank: the tables are merged by (a, b); per
// edge the ranks are taken in ascending order.  Counts add, w_sum adds in fp64 in that order, w_min / w_max take the smaller / larger of
// the ranks with n_finite > 0 (NaN when there is none).  Returns false for a label outside 0 .. K-1, a >= b, or a rank table that is not
// strictly ascending in (a, b).
bool fold_edges(const std::vector<std::vector<EdgeRec>>& ranks, int64_t K, std::vector<EdgeRec>& out) {
  struct Ref { uint64_t key; int32_t rank; uint32_t idx; };
  std::vector<Ref> refs;
  size_t total = 0;
  for (const std::vector<EdgeRec>& R : ranks) total += R.size();
  refs.reserve(total);
  for (size_t r = 0; r < ranks.size(); ++r) {
    const std::vector<EdgeRec>& R = ranks[r];
    uint64_t prev = 0;
    for (size_t i = 0; i < R.size(); ++i) {
      const EdgeRec& e = R[i];
      if (e.a < 0 || e.b < 0 || (int64_t)e.a >= K || (int64_t)e.b >= K || e.a >= e.b) return false;
      const uint64_t key = (uint64_t)e.a * (uint64_t)K + (uint64_t)e.b;   // K < 2^31: below 2^62
      if (i > 0 && key <= prev) return false;
      prev = key;
      refs.push_back(Ref{key, (int32_t)r, (uint32_t)i});
    }
  }
  std::sort(refs.begin(), refs.end(), [](const Ref& x, const Ref& y) { return x.key != y.key ? x.key < y.key : x.rank < y.rank; });
  out.clear();
  for (size_t k = 0; k < refs.size();) {
    EdgeRec f;
    bool have = false;
    const uint64_t key = refs[k].key;
    for (; k < refs.size() && refs[k].key == key; ++k) {
      const EdgeRec& e = ranks[(size_t)refs[k].rank][refs[k].idx];
      f.a = e.a; f.b = e.b;
      f.n_pairs += e.n_pairs; f.n_finite += e.n_finite; f.nodes_a += e.nodes_a; f.nodes_b += e.nodes_b;
      f.w_sum += e.w_sum;
      if (e.n_finite <= 0) continue;
      if (!have) { f.w_min = e.w_min; f.w_max = e.w_max; have = true; }
      else { if (e.w_min < f.w_min) f.w_min = e.w_min; if (e.w_max > f.w_max) f.w_max = e.w_max; }
    }
    if (!have) { f.w_min = __builtin_nanf(""); f.w_max = __builtin_nanf(""); }
    out.push_back(f);
  }
  return true;
}

// One edge of one rank's partial table of a point labelling's graph (vgs_get_own_point_label_graph): EdgeRec and the shared nodes; the
// payload of that graph's second exchange.  Its first entry is the header, as EdgeRec's.
struct LabelEdgeRec {
  EdgeRec e;
  int64_t n_shared = 0;
};
static_assert(sizeof(LabelEdgeRec) == 56, "LabelEdgeRec is the exchange's wire format");

// fold_edges over the ranks' partial tables of a point labelling; n_shared adds like the other counts
bool fold_label_edges(const std::vector<std::vector<LabelEdgeRec>>& ranks, int64_t K, std::vector<LabelEdgeRec>& out) {
  std::vector<std::vector<EdgeRec>> plain(ranks.size());
  for (size_t r = 0; r < ranks.size(); ++r) { plain[r].reserve(ranks[r].size()); for (const LabelEdgeRec& q : ranks[r]) plain[r].push_back(q.e); }
  std::vector<EdgeRec> folded;
  if (!fold_edges(plain, K, folded)) return false;
  out.assign(folded.size(), LabelEdgeRec());
  for (size_t i = 0; i < folded.size(); ++i) out[i].e = folded[i];
  for (const std::vector<LabelEdgeRec>& R : ranks) {   // both ascending in (a, b): one pass per rank
    size_t j = 0;
    for (const LabelEdgeRec& q : R) {
      while (j < out.size() && (out[j].e.a != q.e.a || out[j].e.b != q.e.b)) ++j;
      if (j == out.size()) return false;
      out[j].n_shared += q.n_shared;
    }
  }
  return true;
}

// ------------------------------------------------------------------------------------------------ pair records of a point labelling
// One head flag of one rank in a voxel that holds points of several ranks (vgs_own_point_label_moments): the voxel's code and the label.
struct PairRec {
  uint64_t code = 0;
  int32_t label = 0, pad = 0;
};
static_assert(sizeof(PairRec) == 16, "PairRec is the exchange's wire format");

// Per label 0 .. K-1 the number of distinct (code, label) pairs among all ranks' records: a voxel that several ranks flagged for the same
// label is one node of that label.  The same integers on every rank whatever the order.  False for a label outside 0 .. K-1.
bool fold_label_pairs(const std::vector<std::vector<PairRec>>& ranks, int64_t K, std::vector<int32_t>& add) {
  add.assign((size_t)K, 0);
  std::vector<std::pair<int32_t, uint64_t>> all;
  for (const std::vector<PairRec>& R : ranks)
    for (const PairRec& p : R) {
      if (p.label < 0 || (int64_t)p.label >= K) return false;
      all.emplace_back(p.label, p.code);
    }
  std::sort(all.begin(), all.end());
  all.erase(std::unique(all.begin(), all.end()), all.end());
  for (const auto& p : all) ++add[(size_t)p.first];
  return true;
}

// ------------------------------------------------------------------------------------------------ box extents
// One rank's extents of one global label (vgs_get_own_segment_extents); the payload of the box exchange.  Its first entry is the header:
// label = the rank's status word, pad = 0, lo[0] = its record count.
struct ExtentRec {
  int32_t label = 0, pad = 0;
  double lo[3] = {0, 0, 0};
  double hi[3] = {0, 0, 0};
};
static_assert(sizeof(ExtentRec) == 56, "ExtentRec is the exchange's wire format");

ExtentRec pack_extent(const int32_t* label, const double* lo3, const double* hi3, size_t i) {
  ExtentRec e;
  e.label = label[i];
  for (int a = 0; a < 3; ++a) { e.lo[a] = lo3[3 * i + a]; e.hi[a] = hi3[3 * i + a]; }
  return e;
}

// The extents of every global label 0 .. K-1 from the ranks' records, the same bytes on every rank: per label, ranks in ascending order,
// lo takes the smaller and hi the larger (of values; a zero bound keeps the sign it met first).  A row no record reaches: +inf / -inf and
// reached = 0.  Returns false if a record names a label outside 0 .. K-1.
bool fold_extents(const std::vector<std::vector<ExtentRec>>& ranks, int64_t K, std::vector<double>& lo, std::vector<double>& hi,
                  std::vector<uint8_t>& reached) {
  const double inf = __builtin_huge_val();
  lo.assign(3 * (size_t)K, inf); hi.assign(3 * (size_t)K, -inf); reached.assign((size_t)K, 0);
  for (const std::vector<ExtentRec>& R : ranks)
    for (const ExtentRec& e : R) {
      if (e.label < 0 || (int64_t)e.label >= K) return false;
      const size_t k = (size_t)e.label;
      for (int a = 0; a < 3; ++a) { if (e.lo[a] < lo[3 * k + a]) lo[3 * k + a] = e.lo[a]; if (e.hi[a] > hi[3 * k + a]) hi[3 * k + a] = e.hi[a]; }
      reached[k] = 1;
    }
  return true;
}

// ------------------------------------------------------------------------------------------------ attribute moments
// One rank's attribute moments (vgs_get_own_segment_field_moments): per record a label and n_channels x (n_valid, anchor, S1, S2, min, max).
// On the wire (words of 8 bytes): a header of status word, record count and n_channels, then per record the label and per channel n_valid,
// anchor, S1, S2 and one word holding min | max (two floats): 1 + 5 n_channels words.
struct FieldRecs {
  std::vector<int32_t> label;
  std::vector<int64_t> n;
  std::vector<double> a, s1, s2;
  std::vector<float> mn, mx;
};

// record i of flat arrays (C channels each) as 1 + 5 C wire words behind w
void pack_field(std::vector<uint64_t>& w, const int32_t* label, const int64_t* n, const double* a, const double* s1, const double* s2, const float* mn, const float* mx, size_t C, size_t i) {
  auto bits = [](double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; };
  w.push_back((uint64_t)(uint32_t)label[i]);
  for (size_t ch = 0; ch < C; ++ch) {
    const size_t j = i * C + ch;
    uint32_t lo, hi;
    std::memcpy(&lo, &mn[j], 4); std::memcpy(&hi, &mx[j], 4);
    w.push_back((uint64_t)n[j]); w.push_back(bits(a[j])); w.push_back(bits(s1[j])); w.push_back(bits(s2[j]));
    w.push_back((uint64_t)lo | ((uint64_t)hi << 32));
  }
}
// the inverse: nr records of wire words
void unpack_fields(const uint64_t* w, size_t nr, size_t C, FieldRecs& R) {
  auto dbl = [](uint64_t u) { double v; std::memcpy(&v, &u, 8); return v; };
  R.label.resize(nr); R.n.resize(nr * C); R.a.resize(nr * C); R.s1.resize(nr * C); R.s2.resize(nr * C); R.mn.resize(nr * C); R.mx.resize(nr * C);
  for (size_t i = 0; i < nr; ++i) {
    R.label[i] = (int32_t)(uint32_t)*w++;
    for (size_t ch = 0; ch < C; ++ch) {
      const size_t j = i * C + ch;
      R.n[j] = (int64_t)w[0]; R.a[j] = dbl(w[1]); R.s1[j] = dbl(w[2]); R.s2[j] = dbl(w[3]);
      const uint32_t lo = (uint32_t)w[4], hi = (uint32_t)(w[4] >> 32);
      std::memcpy(&R.mn[j], &lo, 4); std::memcpy(&R.mx[j], &hi, 4);
      w += 5;
    }
  }
}

// The moments of every (label, channel) from the ranks' records, the same bytes on every rank: per entry, ranks in ascending order.  The
// anchor a is the anchor of the lowest rank with n_valid > 0, whose sums are taken as they are; a later rank's sums move to it by delta =
// a_r - a in fp64: S1 += S1_r + n_r delta, S2 += S2_r + S1_r delta + delta S1_r + n_r delta delta (the association of fold_moments'
// diagonal terms).  n_valid adds, min and max take min and max.  An entry no valid value reaches: n = 0, anchor 0, sums 0, +inf / -inf.
// Returns false if a record names a label outside 0 .. K-1.
bool fold_field_moments(const std::vector<FieldRecs>& ranks, int64_t K, int C, std::vector<int64_t>& n, std::vector<double>& a,
                        std::vector<double>& s1, std::vector<double>& s2, std::vector<float>& mn, std::vector<float>& mx) {
  const size_t kc = (size_t)K * (size_t)C;
  n.assign(kc, 0); a.assign(kc, 0.0); s1.assign(kc, 0.0); s2.assign(kc, 0.0);
  mn.assign(kc, __builtin_huge_valf()); mx.assign(kc, -__builtin_huge_valf());
  for (const FieldRecs& R : ranks)
    for (size_t i = 0; i < R.label.size(); ++i) {
      if (R.label[i] < 0 || (int64_t)R.label[i] >= K) return false;
      for (int ch = 0; ch < C; ++ch) {
        const size_t o = (size_t)R.label[i] * (size_t)C + (size_t)ch, j = i * (size_t)C + (size_t)ch;
        if (R.mn[j] < mn[o]) mn[o] = R.mn[j];
        if (R.mx[j] > mx[o]) mx[o] = R.mx[j];
        if (R.n[j] <= 0) continue;
        if (n[o] == 0) {   // the first rank with a valid value: its anchor, its sums as they are
          a[o] = R.a[j]; s1[o] = R.s1[j]; s2[o] = R.s2[j]; n[o] = R.n[j];
          continue;
        }
        const double nr = (double)R.n[j], d = R.a[j] - a[o];
        s1[o] += R.s1[j] + nr * d;
        s2[o] += R.s2[j] + R.s1[j] * d + d * R.s1[j] + nr * d * d;
        n[o] += R.n[j];
      }
    }
  return true;
}

// One rank's class counts (vgs_get_own_segment_class_counts): per record a label, n_outside and n_classes counts.  On the wire (int64
// words): a header of status word, record count and n_classes, then per record label, n_outside, hist[n_classes].
struct ClassRecs {
  std::vector<int32_t> label;
  std::vector<int64_t> hist, n_outside;
};

// record i of flat arrays as 2 + nc wire words behind w
void pack_class(std::vector<int64_t>& w, const int32_t* label, const int64_t* hist, const int64_t* n_outside, size_t nc, size_t i) {
  w.push_back((int64_t)label[i]); w.push_back(n_outside[i]);
  w.insert(w.end(), hist + i * nc, hist + (i + 1) * nc);
}
// the inverse: nr records of wire words
void unpack_classes(const int64_t* w, size_t nr, size_t nc, ClassRecs& R) {
  R.label.resize(nr); R.n_outside.resize(nr); R.hist.resize(nr * nc);
  for (size_t i = 0; i < nr; ++i, w += 2 + nc) {
    R.label[i] = (int32_t)w[0]; R.n_outside[i] = w[1];
    std::copy(w + 2, w + 2 + nc, R.hist.begin() + (ptrdiff_t)(i * nc));
  }
}

// Integer adds per (label, class), then the majority rule of vgs_segment_class_histogram on the folded table: the lowest class with the
// largest count, -1 and 0 when every count is 0.  Returns false if a record names a label outside 0 .. K-1.
bool fold_class_counts(const std::vector<ClassRecs>& ranks, int64_t K, int nc, std::vector<int64_t>& hist, std::vector<int64_t>& n_outside,
                       std::vector<int32_t>& majority, std::vector<int64_t>& majority_count) {
  hist.assign((size_t)K * (size_t)nc, 0); n_outside.assign((size_t)K, 0); majority.assign((size_t)K, -1); majority_count.assign((size_t)K, 0);
  for (const ClassRecs& R : ranks)
    for (size_t i = 0; i < R.label.size(); ++i) {
      if (R.label[i] < 0 || (int64_t)R.label[i] >= K) return false;
      const size_t k = (size_t)R.label[i];
      n_outside[k] += R.n_outside[i];
      for (int j = 0; j < nc; ++j) hist[k * (size_t)nc + (size_t)j] += R.hist[i * (size_t)nc + (size_t)j];
    }
  for (size_t k = 0; k < (size_t)K; ++k)
    for (int j = 0; j < nc; ++j) {
      const int64_t v = hist[k * (size_t)nc + (size_t)j];
      if (v > majority_count[k]) { majority_count[k] = v; majority[k] = j; }   // a strictly larger count only: the lowest class on a tie
    }
  return true;
}

// ------------------------------------------------------------------------------------------------ label refinement
// One band record of one rank (vgs_get_own_band_labels): the payload of the refinement's exchange.  Its first TWO entries are the header:
// [0] code = the rank's status word, label = fill; [1] code = its record count, label | pad = the bits of patch_radius | switch_ratio.
struct BandRec {
  uint64_t code = 0;
  int32_t label = 0, pad = 0;
};
static_assert(sizeof(BandRec) == 16, "BandRec is the exchange's wire format");

// ------------------------------------------------------------------------------------------------ payload headers
// Every payload of a post-run collective opens with a header that holds the rank's status word and its record count: the first entry of
// a struct payload (status in its first field; the count where the record has a slot wide enough for it), the first three words of a word
// payload (status, count, one word of the collective's own; the attribute records of a point labelling add two).  The moment entries'
// count is read behind the exchange (their header also holds K, the pair count and n_skipped in s); no receiver reads an edge or extent
// payload's count, which stays on the wire.
void set_header(MomentRec& h, vgs_status st, size_t n) { h.label = (int32_t)st; h.n_points = (int64_t)n; }
void set_header(EdgeRec& h, vgs_status st, size_t n) { h.a = (int32_t)st; h.n_pairs = (int64_t)n; }
void set_header(ExtentRec& h, vgs_status st, size_t n) { h.label = (int32_t)st; h.lo[0] = (double)n; }
template <typename W> void set_header(std::vector<W>& w, vgs_status st, int64_t n, int64_t own) { w[0] = (W)(uint32_t)st; w[1] = (W)n; w[2] = (W)own; }
template <typename T> constexpr size_t header_len() { return std::is_integral<T>::value ? 3 : 1; }   // entries of the payload
template <> constexpr size_t header_len<BandRec>() { return 2; }
bool header_ok(const MomentRec& h) { return h.label == 0; }
bool header_ok(const EdgeRec& h) { return h.a == 0; }
bool header_ok(const ExtentRec& h) { return h.label == 0; }
bool header_ok(const BandRec& h) { return h.code == 0; }
bool header_ok(const LabelEdgeRec& h) { return h.e.a == 0; }
bool header_ok(uint64_t word0) { return word0 == 0; }
bool header_ok(int64_t word0) { return word0 == 0; }
template <typename T> void strip_headers(std::vector<std::vector<T>>& gathered) { for (std::vector<T>& g : gathered) g.erase(g.begin()); }

// a table (its first n entries) into a caller's array, which may be NULL
template <typename V, typename D> void put(const V& v, D* dst, size_t n = SIZE_MAX) { if (dst) std::copy(v.begin(), v.begin() + (ptrdiff_t)std::min(n, v.size()), dst); }

// the lowest rank for which bad(rank) holds, -1 when there is none: every rank scans what it gathered in the same order, so all name the same rank
template <typename F> int first_bad_rank(int world, F bad) {
  for (int r = 0; r < world; ++r) if (bad(r)) return r;
  return -1;
}

// Where a rank can be told to fail (tests of the agreed-status protocol: VGS_TILES_FAIL_RANK / VGS_TILES_FAIL_AT=<name>).  points, grid and
// stages: before that phase's collective; upload: behind the last collective of vgs_tiles_set_points; the others: before the exchange of
// a post-run collective, and the name is the phase word of the peers' VGS_E_PEER.  descriptors, boxes, fields, compare: the tables of the
// node labelling (fields: statistics and histogram alike); point_labels: every table of a caller's point labelling -- the moment exchange
// of vgs_tiles_point_label_descriptors / _boxes, the cell exchange of vgs_tiles_compare_point_labels, the record exchange of
// vgs_tiles_point_label_field_stats / _class_histogram; refine: vgs_tiles_refine_point_labels; components: the first exchange of
// vgs_tiles_point_label_components; label_graph: the first exchange of vgs_tiles_point_label_graph.
enum Phase { PH_NONE, PH_GRID, PH_STAGES, PH_POINTS, PH_UPLOAD, PH_DESCRIPTORS, PH_GRAPH, PH_BOXES, PH_FIELDS, PH_COMPARE, PH_REFINE, PH_POINT_LABELS, PH_COMPONENTS, PH_LABEL_GRAPH, PH_COUNT };
const char* const PHASE_NAME[PH_COUNT] = {"", "grid", "stages", "points", "upload", "descriptors", "graph", "boxes", "fields", "compare", "refine", "point_labels", "components", "label_graph"};

// Phase clock of one call: lap(slot) gives the slot the host wall time since the last lap (the start, for the first), total(slot) the
// time from the start to the last lap.  Milliseconds.  vgs_tiles_run stamps t->times as it goes; a post-run collective stamps an array of
// its own and total(slot, dst) publishes all of it at the end, so that a call that fails leaves the last good call's times alone.
struct Stopwatch {
  double* ms;
  double start, last;
  static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  explicit Stopwatch(double* slots) : ms(slots), start(now()), last(start) {}
  void lap(int slot) { const double t = now(); ms[slot] = t - last; last = t; }
  void total(int slot) { ms[slot] = last - start; }
  template <int N> void total(int slot, double (&dst)[N]) { total(slot); std::copy(ms, ms + N, dst); }
};

// the phases of a table's collective: dtimes, btimes, ftimes and ltimes share the five slots
enum { T_OWN, T_EXCHANGE, T_FOLD, T_FINISH, T_TOTAL, T_COUNT };
static_assert(VGS_TILES_D_MOMENTS == T_OWN && VGS_TILES_B_EXTENTS == T_OWN && VGS_TILES_F_OWN == T_OWN && VGS_TILES_L_OWN == T_OWN, "slot 0");
static_assert(VGS_TILES_D_EXCHANGE == T_EXCHANGE && VGS_TILES_B_EXCHANGE == T_EXCHANGE && VGS_TILES_F_EXCHANGE == T_EXCHANGE && VGS_TILES_L_EXCHANGE == T_EXCHANGE, "slot 1");
static_assert(VGS_TILES_D_FOLD == T_FOLD && VGS_TILES_B_FOLD == T_FOLD && VGS_TILES_F_FOLD == T_FOLD && VGS_TILES_L_FOLD == T_FOLD, "slot 2");
static_assert(VGS_TILES_D_ALGEBRA == T_FINISH && VGS_TILES_B_FINISH == T_FINISH && VGS_TILES_F_FINISH == T_FINISH && VGS_TILES_L_FINISH == T_FINISH, "slot 3");
static_assert(VGS_TILES_D_TOTAL == T_TOTAL && VGS_TILES_B_TOTAL == T_TOTAL && VGS_TILES_F_TOTAL == T_TOTAL && VGS_TILES_L_TOTAL == T_TOTAL, "slot 4");
static_assert(VGS_TILES_D_COUNT == T_COUNT && VGS_TILES_B_COUNT == T_COUNT && VGS_TILES_F_COUNT == T_COUNT && VGS_TILES_L_COUNT == T_COUNT, "five slots");

// The labelling a per-segment table is made for, which is all a table's driver is told of it.  Node: the run's own labels, K = kept rows,
// nothing of the caller's.  Point: one label per own point of the caller's, K rows of the caller's, on the host or on the device.
struct Labelling {
  const char* fn;         // the public function that was called, for the guard and the messages
  Phase phase;            // where VGS_TILES_FAIL_AT strikes; PHASE_NAME[phase] is the phase word of VGS_E_PEER
  bool point;
  // Which variant of the public entry was called: a `_device` entry is handed device pointers for EVERY array of the caller's, so this
  // says where the labels live (point) and where the attribute rows of an attribute call live (node and point alike).  The node
  // descriptors and boxes take nothing of the caller's and never read it.
  bool on_device;
  // point: the labels and their number.  (The rows of an attribute are counted by the codec: the node family has rows but no labels;
  // the public point entries take one n for both arrays.)
  const int32_t* labels;
  int64_t n;
  int64_t K;              // rows of the table
  const char* limit;      // what every label stays below, for the bad-label message
};

// the tables the drivers fill: the descriptor rows (n_skipped: of a point labelling, summed over the ranks) and the boxes of one frame
struct DescTable {
  std::vector<int64_t> npts;
  std::vector<int32_t> nnodes;
  std::vector<float> bbox, eig8;
  std::vector<double> cen, cov, eval, evec;
  int64_t n_skipped = 0;
};
struct BoxTable { std::vector<double> center, half, frame, lo, hi; };

}  // namespace

// ------------------------------------------------------------------------------------------------ driver
struct vgs_tiles {
  vgs_params P;
  Comm* comm = nullptr;
  vgs_ctx* ctx = nullptr;
  int tiles_x = 1, tiles_y = 1;
  double pitch = 0, cx = 0, cy = 0;
  double lo[2] = {0, 0}, hi[2] = {0, 0};
  std::vector<float> local;   // tile + halo, packed xyz
  int64_t own_first = 0, n_own = 0, n_outside = 0, n_records = 0, kept = 0;
  int64_t exch_sent = 0, exch_recv = 0; int exch_calls = 0;   // the last run's boundary exchange: bytes this rank sent / received, collectives it took
  double times[VGS_TILES_T_COUNT] = {0};   // last run, milliseconds of host wall time per phase (vgs_tiles_get_times)
  int strict_region = 0;      // VGS_TILES_OPT_STRICT_REGION
  Phase fail_phase = PH_NONE;   // tests: where this rank was told to fail (inject)
  vgs_status pending = VGS_OK;   // a local failure behind a call's last collective: the status word of the next collective carries it
  bool warned_outside = false;
  bool ran = false;              // the last vgs_tiles_run completed here
  // the global descriptor table of the last run (vgs_tiles_get_segment_descriptors), K = kept rows; valid until the next run / set_points
  bool desc_valid = false;
  DescTable desc;
  double dtimes[VGS_TILES_D_COUNT] = {0};   // the last descriptor collective, milliseconds of host wall time per phase
  // what the last run's boundary exchange brought (vgs_tiles_get_segment_graph turns it into the halo labels): every rank's records
  // (code, root) and the global label of every (rank, root)
  std::vector<RankRecords> run_rec;
  std::vector<std::vector<int32_t>> run_uroot, run_ulabel;
  // the global edge table of the last run (vgs_tiles_get_segment_graph); valid until the next run / set_points
  bool graph_valid = false;
  std::vector<EdgeRec> graph;
  double gtimes[VGS_TILES_G_COUNT] = {0};   // the last graph collective, milliseconds of host wall time per phase
  int64_t g_halo = 0, g_own = 0, g_bytes = 0;   // its payload: halo labels handed to the context, own edges, bytes sent
  // the global box table of the last run per frame (vgs_tiles_get_segment_boxes), K = kept rows; valid until the next run / set_points
  bool box_valid[2] = {false, false};
  BoxTable box[2];
  double btimes[VGS_TILES_B_COUNT] = {0};   // the last box collective, milliseconds of host wall time per phase
  // the last attribute collective (field statistics or class histogram, of the node labels or of a caller's point labelling; nothing of
  // it is cached): phases, own records, bytes sent
  double ftimes[VGS_TILES_F_COUNT] = {0};
  int64_t f_own = 0, f_bytes = 0;
  // the last tiled compare (its tables live in the context's cmp_* buffers; nothing of the input is cached): phases, own cells, bytes sent
  bool cmp_valid = false;
  double ctimes[VGS_TILES_C_COUNT] = {0};
  int64_t c_own = 0, c_bytes = 0;
  // label refinement: the band table is in the context (vgs_set_refine_halo_labels) from the first refine after a run until the next run
  // or set_points (band_valid: later calls send the header only); the refined labels are in the context too (rf_valid); the last call's
  // phases, band records and bytes sent
  bool band_valid = false, rf_valid = false;
  double rtimes[VGS_TILES_R_COUNT] = {0};
  int64_t r_band = 0, r_bytes = 0;
  // the last table of a caller's point labelling (nothing of it is cached): phases, own moment records, own pair records, bytes sent
  double ltimes[VGS_TILES_L_COUNT] = {0};
  int64_t l_own = 0, l_pairs = 0, l_bytes = 0;
  // the connected parts of the last labelling (vgs_tiles_point_label_components): the global tables, K = cc_K; the part ids of the own
  // points are in the context.  Valid until the next call, the next run or set_points.  Phases, band records, parts, links, bytes sent
  bool cc_valid = false;
  int64_t cc_K = 0;
  std::vector<int32_t> cc_label, cc_nodes, cc_largest;
  std::vector<int64_t> cc_points, cc_first;
  std::vector<uint64_t> cc_code;
  double cctimes[VGS_TILES_CC_COUNT] = {0};
  int64_t cc_band = 0, cc_parts = 0, cc_links = 0, cc_bytes = 0;
  // the adjacency graph of the last labelling (vgs_tiles_point_label_graph): the global table.  Valid until the next call, the next run
  // or set_points.  Phases, band records, foreign records found, own edges, bytes sent
  bool lg_valid = false;
  std::vector<LabelEdgeRec> lgraph;
  double lgtimes[VGS_TILES_LG_COUNT] = {0};
  int64_t lg_band = 0, lg_hits = 0, lg_own = 0, lg_bytes = 0;
  std::string err;
};

static vgs_status tfail(vgs_tiles* t, vgs_status s, const std::string& msg) { t->err = msg; return s; }
#define TCTX(call) do { vgs_status s_ = (call); if (s_ != VGS_OK) return tfail(t, s_, std::string(#call) + ": " + vgs_last_error_string(t->ctx)); } while (0)
#define TCOMM(call) do { if (!(call)) return tfail(t, VGS_E_HIP, std::string("collective failed: ") + t->comm->err); } while (0)
#define TRY(call) do { vgs_status s_ = (call); if (s_ != VGS_OK) return s_; } while (0)   // (the callee has set t->err)
// The pieces of the agreed-status protocol (the head of this file), in the order a collective meets them.
// A step between two collectives runs only while nothing has failed here; its failure is recorded in `carry`, never returned.  TCARRY_AS:
// the call goes through a pointer chosen at run time, `name` is the function it points to -- the text is that of TCARRY on the call itself.
#define TCARRY_AS(fn, name, ...) do { if (carry == VGS_OK) { vgs_status s_ = (fn)(__VA_ARGS__); if (s_ != VGS_OK) { carry = s_; t->err = std::string(name) + "(" #__VA_ARGS__ "): " + vgs_last_error_string(t->ctx); } } } while (0)
#define TCARRY(call) do { if (carry == VGS_OK) { vgs_status s_ = (call); if (s_ != VGS_OK) { carry = s_; t->err = std::string(#call) + ": " + vgs_last_error_string(t->ctx); } } } while (0)

// failure injection: a rank told to fail at `ph` records that as its local failure there, unless a real one came first
static void inject(vgs_tiles* t, Phase ph, vgs_status& carry) {
  if (t->fail_phase == ph && carry == VGS_OK) { carry = VGS_E_STATE; t->err = std::string("failure requested by VGS_TILES_FAIL_RANK / VGS_TILES_FAIL_AT=") + PHASE_NAME[ph]; }
}

// opening of a collective after vgs_tiles_run: a rank that never ran and keeps no failure makes no collective (nor do its peers, in the same state)
static vgs_status open_collective(vgs_tiles* t, const std::string& fn, Phase ph, vgs_status& carry) {
  if (!t->ran && t->pending == VGS_OK) return tfail(t, VGS_E_STATE, fn + ": vgs_tiles_run first");
  carry = t->pending;
  inject(t, ph, carry);
  return VGS_OK;
}

// the verdict, the same on every rank from the same gathered status words
static vgs_status agreed(vgs_tiles* t, vgs_status mine, int bad_rank, const char* phase) {
  if (mine != VGS_OK) return mine;   // t->err already says what failed here
  if (bad_rank >= 0) return tfail(t, VGS_E_PEER, std::string("rank ") + std::to_string(bad_rank) + " failed in the " + phase + " phase; this rank stops with it");
  return VGS_OK;
}

// The exchange of a post-run collective: the payload, its header filled in (set_header; `carry` is the status in it), goes through ONE
// all_gather_varlen whatever `carry` is -- no path leads round it.  A payload too short to hold a header counts as a failed rank.
// VGS_OK: every gathered[r] opens with a header of status 0, still in place.
template <typename T>
static vgs_status exchange(vgs_tiles* t, vgs_status carry, const std::vector<T>& payload, const char* phase, Stopwatch& sw, int slot, std::vector<std::vector<T>>& gathered) {
  TCOMM(all_gather_varlen(*t->comm, payload, gathered));
  sw.lap(slot);
  const int bad = first_bad_rank(t->comm->world, [&](int r) { return gathered[(size_t)r].size() < header_len<T>() || !header_ok(gathered[(size_t)r][0]); });
  return agreed(t, carry, bad, phase);
}

// The two verdicts behind an exchange in which every rank was valid on its own, the same on every rank from the same gathered words: the
// ranks do not describe the same table (`what`: an argument of the call that must be the same everywhere), or a payload is not as long as
// its header says.
static vgs_status disagree(vgs_tiles* t, const char* fn, size_t r, const char* what, int64_t vr, int64_t v0) {
  return tfail(t, VGS_E_ARG, std::string(fn) + ": rank " + std::to_string(r) + " passed " + what + " = " + std::to_string(vr) + ", rank 0 passed " + std::to_string(v0));
}
static vgs_status wrong_size(vgs_tiles* t, const char* fn, size_t r) { return tfail(t, VGS_E_STATE, std::string(fn) + ": rank " + std::to_string(r) + " sent a payload of the wrong size"); }

// Behind the exchange of a word payload: a header of `header` words (status, record count, then the collective's own), `per` words a
// record.  The header words named in `same` are arguments of the call and must agree over the ranks, in that order of precedence.
struct AgreedWord { size_t at; const char* name; };
constexpr size_t LF_HEADER = 5;   // header words of a point labelling's attribute records: status, record count, n_channels or n_classes, K, own n_skipped
template <typename W>
static vgs_status check_payloads(vgs_tiles* t, const char* fn, const std::vector<std::vector<W>>& gathered, size_t header, size_t per, const std::vector<AgreedWord>& same) {
  auto word = [&](size_t r, size_t i) { return (int64_t)gathered[r][i]; };
  for (size_t r = 0; r < gathered.size(); ++r) if (gathered[r].size() < header) return wrong_size(t, fn, r);
  for (size_t r = 1; r < gathered.size(); ++r)
    for (const AgreedWord& a : same) if (word(r, a.at) != word(0, a.at)) return disagree(t, fn, r, a.name, word(r, a.at), word(0, a.at));
  for (size_t r = 0; r < gathered.size(); ++r)
    if (word(r, 1) < 0 || gathered[r].size() != header + (size_t)word(r, 1) * per) return wrong_size(t, fn, r);
  return VGS_OK;
}

// closing: the local step behind a call's last collective; its error is returned AND kept for the next collective's header (open_collective)
static vgs_status behind_collective(vgs_tiles* t, vgs_status s, const char* what) {
  if (s == VGS_OK) return VGS_OK;
  t->pending = s;
  return tfail(t, s, std::string(what) + ": " + vgs_last_error_string(t->ctx));
}

// what a new cloud or a new run makes stale: the run itself and every table cached from it
static void invalidate(vgs_tiles* t) { t->ran = false; t->desc_valid = false; t->graph_valid = false; t->box_valid[0] = t->box_valid[1] = false; t->cmp_valid = false; t->band_valid = false; t->rf_valid = false; t->cc_valid = false; t->lg_valid = false; }

template <int N> static vgs_status get_times(vgs_tiles* t, double (vgs_tiles::*slots)[N], double* ms, int32_t n) {
  if (!t || !ms || n < 0 || n > N) return VGS_E_ARG;
  std::copy(t->*slots, t->*slots + n, ms);
  return VGS_OK;
}

// ------------------------------------------------------------------------------------------------ descriptors and boxes: the drivers
static Labelling node_labelling(const vgs_tiles* t, const char* fn, Phase ph, bool on_device = false) { return Labelling{fn, ph, false, on_device, nullptr, 0, t->kept, "kept_global"}; }
static Labelling point_labelling(const char* fn, bool on_device, const int32_t* labels, int64_t n, int64_t K) { return Labelling{fn, PH_POINT_LABELS, true, on_device, labels, n, K, "K"}; }
static vgs_status bad_label(vgs_tiles* t, const Labelling& L) { return tfail(t, VGS_E_STATE, std::string(L.fn) + ": a rank sent a label >= " + L.limit); }

namespace {
constexpr size_t PAIRS_PER_ENTRY = sizeof(MomentRec) / sizeof(PairRec);
struct MomentSent { int64_t own = 0, pairs = 0, bytes = 0; };   // this rank's payload: moment records, pair records, bytes
}  // namespace

// The moment collective: the descriptors of either labelling.  No point, label or id travels, every point is handled by the rank that
// loaded it.  This rank's moment records of its own points (one small pipeline on its GPU; a point labelling also has pair records, the
// head flags of the voxels that hold points of several ranks) -> ONE all_gather_varlen of 128-byte entries: a header (status word,
// moment-record count; K, pair-record count and own n_skipped as int64 in the first three slots of s), the moment records, then the
// 16-byte pair records, eight to an entry -> fold_moments and fold_label_pairs, the same on every rank -> n_nodes = folded n_nodes +
// distinct pairs -> the per-segment algebra on this rank's GPU.  Same bytes on every rank: the folds' inputs and order are the same
// everywhere, and the algebra is one deterministic device function of its inputs.  Everything a rank can get wrong on its own is found by
// the context call and travels in the status word; ranks that are each valid but pass different K all leave with VGS_E_ARG behind the
// exchange.  The caller has opened the collective (`carry`) and places the table, the times and the payload figures.
static vgs_status moment_collective(vgs_tiles* t, const Labelling& L, vgs_status carry, double (&ms)[T_COUNT], DescTable& D, MomentSent& sent) {
  const int64_t K = L.K;
  Stopwatch sw(ms);
  int64_t n_rec = 0, n_pairs = 0, n_skip = 0;
  std::vector<MomentRec> payload(1);
  {   // (the staging arrays are gone before the fold asks for its tables)
    std::vector<int32_t> lab, nn, pl;
    std::vector<int64_t> pts;
    std::vector<float> bb, an;
    std::vector<double> sm;
    std::vector<uint64_t> pc;
    auto room = [&](size_t nr, size_t np) {
      lab.resize(nr + 1); nn.resize(nr + 1); pts.resize(nr + 1); bb.resize(6 * nr + 1); an.resize(3 * nr + 1); sm.resize(9 * nr + 1); pc.resize(np + 1); pl.resize(np + 1);
    };
    if (L.point) {   // count, then fetch; K = 0 included (nothing is cached and the ranks still agree on n_skipped)
      TCARRY_AS(L.on_device ? vgs_own_point_label_moments_device : vgs_own_point_label_moments,
                L.on_device ? "vgs_own_point_label_moments_device" : "vgs_own_point_label_moments", t->ctx, K, L.labels, L.n, &n_rec, &n_pairs, &n_skip);
      if (carry == VGS_OK) room((size_t)n_rec, (size_t)n_pairs);
      TCARRY(vgs_get_own_point_label_moments(t->ctx, lab.data(), pts.data(), nn.data(), bb.data(), an.data(), sm.data(), pc.data(), pl.data()));
    } else if (K > 0) {   // at most one record per kept segment and no pair record: a node lies in one rank's region
      room((size_t)K, 0);
      TCARRY(vgs_get_own_segment_moments(t->ctx, K, &n_rec, lab.data(), pts.data(), nn.data(), bb.data(), an.data(), sm.data()));
    }
    if (carry != VGS_OK) { n_rec = 0; n_pairs = 0; n_skip = 0; }
    const size_t nr = (size_t)n_rec, np = (size_t)n_pairs;
    payload.resize(1 + nr + (np + PAIRS_PER_ENTRY - 1) / PAIRS_PER_ENTRY);
    for (size_t i = 0; i < nr; ++i) payload[1 + i] = pack_moment(lab.data(), pts.data(), nn.data(), bb.data(), an.data(), sm.data(), i);
    PairRec* pr = reinterpret_cast<PairRec*>(payload.data() + 1 + nr);
    for (size_t i = 0; i < np; ++i) { pr[i].code = pc[i]; pr[i].label = pl[i]; pr[i].pad = 0; }
  }
  const size_t k1 = (size_t)K;
  set_header(payload[0], carry, (size_t)n_rec);
  const int64_t own_words[3] = {K, n_pairs, n_skip};
  std::memcpy(payload[0].s, own_words, sizeof(own_words));
  sw.lap(T_OWN);
  std::vector<std::vector<MomentRec>> gathered;
  TRY(exchange(t, carry, payload, PHASE_NAME[L.phase], sw, T_EXCHANGE, gathered));
  // every rank was valid on its own: do they describe the same table, and is every payload as long as its header says?
  const size_t world = gathered.size();
  std::vector<int64_t> hk(world), hp(world), hr(world);
  D.n_skipped = 0;
  for (size_t r = 0; r < world; ++r) {
    int64_t w[3];
    std::memcpy(w, gathered[r][0].s, sizeof(w));
    hk[r] = w[0]; hp[r] = w[1]; D.n_skipped += w[2]; hr[r] = gathered[r][0].n_points;
  }
  for (size_t r = 1; r < world; ++r) if (hk[r] != hk[0]) return disagree(t, L.fn, r, "K", hk[r], hk[0]);
  for (size_t r = 0; r < world; ++r)
    if (hr[r] < 0 || hp[r] < 0 || gathered[r].size() != 1 + (size_t)hr[r] + ((size_t)hp[r] + PAIRS_PER_ENTRY - 1) / PAIRS_PER_ENTRY) return wrong_size(t, L.fn, r);
  std::vector<std::vector<MomentRec>> recs(world);
  std::vector<std::vector<PairRec>> pairs(world);
  for (size_t r = 0; r < world; ++r) {
    recs[r].assign(gathered[r].begin() + 1, gathered[r].begin() + 1 + (ptrdiff_t)hr[r]);
    pairs[r].resize((size_t)hp[r]);
    if (hp[r] > 0) std::memcpy(pairs[r].data(), gathered[r].data() + 1 + hr[r], (size_t)hp[r] * sizeof(PairRec));
  }
  std::vector<int64_t> npts;
  std::vector<int32_t> nnodes, add;
  std::vector<float> bbox, anchor;
  std::vector<double> s9;
  if (!fold_moments(recs, K, npts, nnodes, bbox, anchor, s9) || !fold_label_pairs(pairs, K, add)) return bad_label(t, L);
  for (size_t k = 0; k < k1; ++k) nnodes[k] += add[k];
  sw.lap(T_FOLD);
  D.npts.resize(k1); D.nnodes.resize(k1); D.bbox.resize(6 * k1); D.cen.resize(3 * k1); D.cov.resize(6 * k1); D.eval.resize(3 * k1); D.evec.resize(9 * k1);
  D.eig8.resize(8 * k1);
  TRY(behind_collective(t, vgs_segment_descriptors_from_moments(t->ctx, K, npts.data(), nnodes.data(), bbox.data(), anchor.data(), s9.data(), D.npts.data(), D.nnodes.data(),
                                                                D.bbox.data(), D.cen.data(), D.cov.data(), D.eval.data(), D.evec.data(), D.eig8.data()),
                        "vgs_segment_descriptors_from_moments"));
  sw.lap(T_FINISH);
  sw.total(T_TOTAL);
  sent.own = n_rec; sent.pairs = n_pairs; sent.bytes = (int64_t)(payload.size() * sizeof(MomentRec));
  return VGS_OK;
}

// The extent collective: the boxes of either labelling about the rows `D` of its descriptor table.  This rank's extents of its own points
// about the global centroids, in the frames made from the global rows (one small pipeline on its GPU) -> ONE all_gather_varlen of 56-byte
// records behind a header of status word and record count -> the same host fold on every rank (min / max) -> half and centre on this
// rank's GPU.  Same bytes on every rank: min and max do not depend on the order, and the finish is one device function of its inputs.
// The caller has made the table `D` and opened the collective (`carry`); it places the boxes, the times and the bytes sent.
static vgs_status extent_collective(vgs_tiles* t, const Labelling& L, int32_t frame, vgs_status carry, const DescTable& D, double (&ms)[T_COUNT], BoxTable& B, int64_t& bytes) {
  const int64_t K = L.K;
  const size_t k1 = (size_t)K;
  Stopwatch sw(ms);
  std::vector<ExtentRec> payload(1);
  if (carry == VGS_OK && K > 0) {
    std::vector<int32_t> lab(k1);
    std::vector<double> lo(3 * k1), hi(3 * k1);
    int64_t n = 0;
    if (L.point)
      TCARRY_AS(L.on_device ? vgs_get_own_point_label_extents_device : vgs_get_own_point_label_extents,
                L.on_device ? "vgs_get_own_point_label_extents_device" : "vgs_get_own_point_label_extents", t->ctx, K, frame, L.labels, L.n, D.cen.data(), D.cov.data(),
                D.evec.data(), &n, lab.data(), lo.data(), hi.data());
    else
      TCARRY(vgs_get_own_segment_extents(t->ctx, K, frame, D.cen.data(), D.cov.data(), D.evec.data(), &n, lab.data(), lo.data(), hi.data()));
    if (carry == VGS_OK) payload.reserve(1 + (size_t)n);
    if (carry == VGS_OK) for (size_t i = 0; i < (size_t)n; ++i) payload.push_back(pack_extent(lab.data(), lo.data(), hi.data(), i));
  }
  set_header(payload[0], carry, payload.size() - 1);
  sw.lap(T_OWN);
  std::vector<std::vector<ExtentRec>> gathered;
  TRY(exchange(t, carry, payload, PHASE_NAME[L.phase], sw, T_EXCHANGE, gathered));
  strip_headers(gathered);
  std::vector<double> lo, hi;
  std::vector<uint8_t> reached;
  if (!fold_extents(gathered, K, lo, hi, reached)) return bad_label(t, L);
  // a row no record reaches (no labelled point anywhere, n_points = 0 in the descriptor table): lo = hi = 0, so half = 0 and centre = centroid
  for (size_t k = 0; k < k1; ++k) if (!reached[k]) for (int a = 0; a < 3; ++a) { lo[3 * k + a] = 0.0; hi[3 * k + a] = 0.0; }
  sw.lap(T_FOLD);
  std::vector<double> ce(3 * k1), ha(3 * k1), fr(9 * k1);
  TRY(behind_collective(t, vgs_segment_boxes_from_extents(t->ctx, K, frame, D.cen.data(), D.cov.data(), D.evec.data(), lo.data(), hi.data(), ce.data(), ha.data(), fr.data()),
                        "vgs_segment_boxes_from_extents"));
  sw.lap(T_FINISH);
  sw.total(T_TOTAL);
  B.center.swap(ce); B.half.swap(ha); B.frame.swap(fr); B.lo.swap(lo); B.hi.swap(hi);
  bytes = (int64_t)(payload.size() * sizeof(ExtentRec));
  return VGS_OK;
}

// The first of a call's two collectives (the descriptors a box call needs) ends the call on every rank alike when a status word in it says
// so.  A failure of this rank BEHIND that collective (it newly sets t->pending; the peers' tables are complete and they go on) does not:
// it travels in the second exchange's status word, which the caller takes from t->pending.
template <typename Step> static vgs_status first_of_two(vgs_tiles* t, Step step) {
  const vgs_status before = t->pending;
  const vgs_status s = step();
  return s != VGS_OK && before == VGS_OK && t->pending != VGS_OK ? VGS_OK : s;
}

static bool bad_frame(vgs_tiles* t, const char* fn, int32_t frame) {
  if (frame == VGS_BOX_PRINCIPAL || frame == VGS_BOX_UPRIGHT) return false;
  t->err = std::string(fn) + ": frame must be VGS_BOX_PRINCIPAL (0) or VGS_BOX_UPRIGHT (1)";
  return true;
}

static void put_descriptors(const DescTable& D, int64_t* n_points, int32_t* n_nodes, float* bbox6, double* centroid3, double* cov6, double* evals3, double* evecs9, float* eigen8) {
  put(D.npts, n_points); put(D.nnodes, n_nodes); put(D.bbox, bbox6); put(D.cen, centroid3); put(D.cov, cov6); put(D.eval, evals3); put(D.evec, evecs9); put(D.eig8, eigen8);
}
static void put_boxes(const BoxTable& B, double* center3, double* half3, double* frame9, double* lo3, double* hi3) {
  put(B.center, center3); put(B.half, half3); put(B.frame, frame9); put(B.lo, lo3); put(B.hi, hi3);
}

// ------------------------------------------------------------------------------------------------ attribute statistics: the driver
// The attribute collective: field statistics and class histograms of either labelling.  No attribute travels, every point is counted once,
// by the rank that loaded it (so a voxel shared by ranks needs no pair records here).  This rank's records of its own rows (one small
// pipeline on its GPU) -> ONE all_gather_varlen of 8-byte words: a header, then the records in the codec's wire format -> the same host
// fold on every rank -> (fields) mean, var, min and max on this rank's GPU.  The header: status word, record count, n_channels or
// n_classes; a point labelling adds K and this rank's own n_skipped (LF_HEADER words in all).  Nothing is cached (the input is the
// caller's), so every call is collective, K = 0 included.  Everything a rank can get wrong on its own -- n, a NULL input, the channel and
// stride values, a failing context call -- is found by the context call and travels in the status word; ranks that are each valid but
// disagree on K or on n_channels / n_classes all leave with VGS_E_ARG behind the exchange.
namespace {
// the records a rank can have: one per kept segment, or per label with an own point; 0 where the context refuses the call before it
// writes (K x per_label counters bound both tables of a point labelling and the histogram of the node labelling)
size_t record_cap(const vgs_tiles* t, const Labelling& L, int64_t per_label, bool per_ok, bool node_limit) {
  if (!per_ok || L.K < 0 || L.K > (int64_t)0x7fffffff || ((L.point || node_limit) && L.K * per_label > ((int64_t)1 << 27))) return 0;
  return (size_t)(L.point ? std::min(L.K, std::max<int64_t>(t->n_own, 0)) : L.K);
}

// What the collective is told of a table kind: the wire word and the words of a record, the own records (the context call, packed
// behind the header; no record where the call fails or the context refuses it), unpack, the fold, the finish on the device (FINISH: its
// name; none for the histogram, whose majority rule is integer work inside the fold) and the caller's arrays.  One object per call: it
// holds the folded table.
struct FieldCodec {
  using Word = uint64_t;
  using Recs = FieldRecs;
  static constexpr const char* ARG = "n_channels";
  static constexpr const char* FINISH = "vgs_segment_field_stats_from_moments";
  static constexpr bool NODE_LIMIT = false;
  const float* field; int64_t n; int32_t count; int64_t stride_bytes;
  int64_t* o_n; double *o_anchor, *o_mean, *o_var; float *o_min, *o_max;
  std::vector<int64_t> fn;
  std::vector<double> fa, f1, f2, me, va;
  std::vector<float> fmn, fmx, omn, omx;
  FieldCodec(const float* field_, int64_t n_, int32_t n_channels, int64_t stride, int64_t* n_valid, double* anchor, double* mean, double* var, float* vmin, float* vmax)
      : field(field_), n(n_), count(n_channels), stride_bytes(stride), o_n(n_valid), o_anchor(anchor), o_mean(mean), o_var(var), o_min(vmin), o_max(vmax) {}
  bool ok() const { return count >= 1 && count <= 64; }
  size_t C() const { return ok() ? (size_t)count : 0; }
  size_t words() const { return 1 + 5 * C(); }
  int64_t header() const { return (int64_t)(uint32_t)count; }
  void own(vgs_tiles* t, const Labelling& L, size_t cap, vgs_status& carry, int64_t& n_rec, int64_t& n_skip, std::vector<Word>& payload) const {
    const size_t c = cap * C() + 1;
    std::vector<int32_t> lab(cap + 1);
    std::vector<int64_t> nv(c);
    std::vector<double> an(c), m1(c), m2(c);
    std::vector<float> mn(c), mx(c);
    auto p = [cap](auto& v) { return cap > 0 ? v.data() : nullptr; };   // (a call the context refuses writes nothing; so does one without a record)
    if (L.point)
      TCARRY_AS(L.on_device ? vgs_own_point_label_field_moments_device : vgs_own_point_label_field_moments,
                L.on_device ? "vgs_own_point_label_field_moments_device" : "vgs_own_point_label_field_moments", t->ctx, L.K, L.labels, field, n, count, stride_bytes,
                &n_rec, &n_skip, p(lab), p(nv), p(an), p(m1), p(m2), p(mn), p(mx));
    else
      TCARRY_AS(L.on_device ? vgs_get_own_segment_field_moments_device : vgs_get_own_segment_field_moments,
                L.on_device ? "vgs_get_own_segment_field_moments_device" : "vgs_get_own_segment_field_moments", t->ctx, L.K, field, n, count, stride_bytes, &n_rec,
                p(lab), p(nv), p(an), p(m1), p(m2), p(mn), p(mx));
    if (carry != VGS_OK || cap == 0) n_rec = 0;
    payload.reserve(payload.size() + (size_t)n_rec * words());
    for (size_t i = 0; i < (size_t)n_rec; ++i) pack_field(payload, lab.data(), nv.data(), an.data(), m1.data(), m2.data(), mn.data(), mx.data(), C(), i);
  }
  void unpack(const Word* w, size_t nr, Recs& R) const { unpack_fields(w, nr, C(), R); }
  bool fold(const std::vector<Recs>& ranks, int64_t K) { return fold_field_moments(ranks, K, (int)C(), fn, fa, f1, f2, fmn, fmx); }
  vgs_status finish(vgs_ctx* ctx, int64_t K) {
    const size_t kc = (size_t)K * C() + 1;
    me.resize(kc); va.resize(kc); omn.resize(kc); omx.resize(kc);
    return vgs_segment_field_stats_from_moments(ctx, K, count, fn.data(), fa.data(), f1.data(), f2.data(), fmn.data(), fmx.data(), me.data(), va.data(), omn.data(), omx.data());
  }
  void place(int64_t K) const {
    const size_t kc = (size_t)K * C();
    put(fn, o_n); put(fa, o_anchor); put(me, o_mean, kc); put(va, o_var, kc); put(omn, o_min, kc); put(omx, o_max, kc);
  }
};

struct ClassCodec {
  using Word = int64_t;
  using Recs = ClassRecs;
  static constexpr const char* ARG = "n_classes";
  static constexpr const char* FINISH = nullptr;
  static constexpr bool NODE_LIMIT = true;
  const int32_t* cls; int64_t n; int32_t count;
  int64_t *o_hist, *o_outside; int32_t* o_majority; int64_t* o_count;
  std::vector<int32_t> fm;
  std::vector<int64_t> fh, fo, fc;
  ClassCodec(const int32_t* cls_, int64_t n_, int32_t n_classes, int64_t* hist, int64_t* n_outside, int32_t* majority, int64_t* majority_count)
      : cls(cls_), n(n_), count(n_classes), o_hist(hist), o_outside(n_outside), o_majority(majority), o_count(majority_count) {}
  bool ok() const { return count >= 1 && count <= 1024; }
  size_t nc() const { return ok() ? (size_t)count : 0; }
  size_t words() const { return 2 + nc(); }
  int64_t header() const { return (int64_t)count; }
  void own(vgs_tiles* t, const Labelling& L, size_t cap, vgs_status& carry, int64_t& n_rec, int64_t& n_skip, std::vector<Word>& payload) const {
    std::vector<int32_t> lab(cap + 1);
    std::vector<int64_t> hi(cap * nc() + 1), no(cap + 1);
    auto p = [cap](auto& v) { return cap > 0 ? v.data() : nullptr; };
    if (L.point)
      TCARRY_AS(L.on_device ? vgs_own_point_label_class_counts_device : vgs_own_point_label_class_counts,
                L.on_device ? "vgs_own_point_label_class_counts_device" : "vgs_own_point_label_class_counts", t->ctx, L.K, L.labels, cls, n, count, &n_rec, &n_skip,
                p(lab), p(hi), p(no));
    else
      TCARRY_AS(L.on_device ? vgs_get_own_segment_class_counts_device : vgs_get_own_segment_class_counts,
                L.on_device ? "vgs_get_own_segment_class_counts_device" : "vgs_get_own_segment_class_counts", t->ctx, L.K, cls, n, count, &n_rec, p(lab), p(hi), p(no));
    if (carry != VGS_OK || cap == 0) n_rec = 0;
    payload.reserve(payload.size() + (size_t)n_rec * words());
    for (size_t i = 0; i < (size_t)n_rec; ++i) pack_class(payload, lab.data(), hi.data(), no.data(), nc(), i);
  }
  void unpack(const Word* w, size_t nr, Recs& R) const { unpack_classes(w, nr, nc(), R); }
  bool fold(const std::vector<Recs>& ranks, int64_t K) { return fold_class_counts(ranks, K, (int)nc(), fh, fo, fm, fc); }
  vgs_status finish(vgs_ctx*, int64_t) { return VGS_OK; }
  void place(int64_t) const { put(fh, o_hist); put(fo, o_outside); put(fm, o_majority); put(fc, o_count); }
};
}  // namespace

template <typename Codec>
static vgs_status attribute_collective(vgs_tiles* t, const Labelling& L, Codec A, int64_t* n_skipped) {
  using W = typename Codec::Word;
  vgs_status carry;
  TRY(open_collective(t, L.fn, L.phase, carry));
  double ms[T_COUNT] = {0};
  Stopwatch sw(ms);
  const size_t header = L.point ? LF_HEADER : 3, per = A.words();
  std::vector<W> payload(header, 0);
  int64_t n_rec = 0, n_skip = 0;
  if (carry == VGS_OK) {
    const size_t cap = record_cap(t, L, A.count, A.ok(), Codec::NODE_LIMIT);
    A.own(t, L, cap, carry, n_rec, n_skip, payload);   // (its staging arrays are gone before the fold asks for its tables)
    if (carry != VGS_OK) n_skip = 0;
  }
  set_header(payload, carry, n_rec, A.header());
  if (L.point) { payload[3] = (W)L.K; payload[4] = (W)n_skip; }
  sw.lap(T_OWN);
  std::vector<std::vector<W>> gathered;
  TRY(exchange(t, carry, payload, PHASE_NAME[L.phase], sw, T_EXCHANGE, gathered));
  // every rank was valid on its own: do they describe the same table, and is every payload as long as its header says?
  std::vector<AgreedWord> same;
  if (L.point) same.push_back({3, "K"});
  same.push_back({2, Codec::ARG});
  TRY(check_payloads(t, L.fn, gathered, header, per, same));
  std::vector<typename Codec::Recs> recs(gathered.size());
  int64_t skipped = 0;
  for (size_t r = 0; r < gathered.size(); ++r) {
    A.unpack(gathered[r].data() + header, (size_t)gathered[r][1], recs[r]);
    if (L.point) skipped += (int64_t)gathered[r][4];
  }
  if (!A.fold(recs, L.K)) return bad_label(t, L);
  sw.lap(T_FOLD);
  if constexpr (Codec::FINISH != nullptr) {   // (the histogram's VGS_TILES_F_FINISH stays 0)
    TRY(behind_collective(t, A.finish(t->ctx, L.K), Codec::FINISH));
    sw.lap(T_FINISH);
  }
  sw.total(T_TOTAL, t->ftimes);
  if (n_skipped) *n_skipped = skipped;
  A.place(L.K);
  t->f_own = n_rec; t->f_bytes = (int64_t)(payload.size() * sizeof(W));
  return VGS_OK;
}

extern "C" {

vgs_status vgs_tiles_local_group_create(int world, void** group) {
  if (world < 1 || !group) return VGS_E_ARG;
  *group = new LocalGroup(world);
  return VGS_OK;
}
void vgs_tiles_local_group_destroy(void* group) { delete (LocalGroup*)group; }
void vgs_tiles_local_group_abort(void* group) { if (group) ((LocalGroup*)group)->abort(); }

vgs_status vgs_tiles_create(const vgs_params* p, int comm_kind, void* comm_handle, int rank, int world, int tiles_x, int tiles_y, double pitch,
                            double center_x, double center_y, vgs_tiles** out) {
  if (!p || !out || !comm_handle || world < 1 || rank < 0 || rank >= world || tiles_x < 1 || tiles_y < 1 || tiles_x * tiles_y != world) return VGS_E_ARG;
  if (p->method != 2) return VGS_E_UNSUPPORTED;   // the tiled path is VGS (BASELINE.json configs[4])
  *out = nullptr;
  vgs_tiles* t = new vgs_tiles();
  t->P = *p;
  t->tiles_x = tiles_x; t->tiles_y = tiles_y; t->pitch = pitch; t->cx = center_x; t->cy = center_y;
  if (comm_kind == VGS_TILES_COMM_LOCAL) t->comm = new LocalComm((LocalGroup*)comm_handle, rank);
  else if (comm_kind == VGS_TILES_COMM_RCCL) t->comm = new RcclComm((ncclComm_t)comm_handle, rank, world, p->device);
  else if (comm_kind == VGS_TILES_COMM_CALLBACKS) {
    const vgs_tiles_callbacks* cb = (const vgs_tiles_callbacks*)comm_handle;
    if (!cb->all_gather || !cb->bcast) { delete t; return VGS_E_ARG; }
    t->comm = new CallbackComm(*cb, rank, world);
  } else { delete t; return VGS_E_ARG; }
  {
    // failure injection for the tests of the agreed-status protocol; read once, here
    const char* fr = std::getenv("VGS_TILES_FAIL_RANK");
    const char* fa = std::getenv("VGS_TILES_FAIL_AT");
    if (fr && fa && std::atoi(fr) == rank)
      for (int ph = PH_NONE + 1; ph < PH_COUNT; ++ph) if (!std::strcmp(fa, PHASE_NAME[ph])) t->fail_phase = (Phase)ph;
  }
  vgs_status s = vgs_create(p, &t->ctx);
  if (s != VGS_OK) { delete t->comm; delete t; return s; }
  *out = t;
  return VGS_OK;
}

void vgs_tiles_destroy(vgs_tiles* t) {
  if (!t) return;
  if (t->ctx) vgs_destroy(t->ctx);
  delete t->comm;
  delete t;
}

const char* vgs_tiles_last_error_string(const vgs_tiles* t) { return t ? t->err.c_str() : "null handle"; }
vgs_ctx* vgs_tiles_context(vgs_tiles* t) { return t ? t->ctx : nullptr; }

vgs_status vgs_tiles_set_option(vgs_tiles* t, int32_t option, int64_t value) {
  if (!t) return VGS_E_ARG;
  if (option == VGS_TILES_OPT_STRICT_REGION) { t->strict_region = value != 0; return VGS_OK; }
  return tfail(t, VGS_E_ARG, "unknown option");
}

vgs_status vgs_tiles_get_times(vgs_tiles* t, double* ms, int32_t n) { return get_times(t, &vgs_tiles::times, ms, n); }

vgs_status vgs_tiles_set_points(vgs_tiles* t, const float* xyz, int64_t n, int32_t stride_bytes) {
  if (!t || (!xyz && n > 0) || n < 0 || (stride_bytes != 12 && stride_bytes != 16)) return VGS_E_ARG;
  Comm& c = *t->comm;
  invalidate(t);
  const int sf = stride_bytes / 4;
  if (!(t->pitch > 0)) {   // the largest x-extent over the ranks
    float mn = 3.0e38f, mx = -3.0e38f;
    for (int64_t i = 0; i < n; ++i) { const float x = xyz[i * sf]; if (x == x) { mn = std::min(mn, x); mx = std::max(mx, x); } }
    double ext = n > 0 ? (double)(mx - mn) : 0.0;
    std::vector<double> all((size_t)c.world);
    TCOMM(c.all_gather(&ext, all.data(), sizeof(double)));
    t->pitch = *std::max_element(all.begin(), all.end());
  }
  // ownership rectangle [lo, hi): outer edges are open ended
  const double big = 1.0e30;
  const int i = c.rank % t->tiles_x, j = c.rank / t->tiles_x;
  const double x0 = t->cx + (i - t->tiles_x / 2.0) * t->pitch, y0 = t->cy + (j - t->tiles_y / 2.0) * t->pitch;
  t->lo[0] = i > 0 ? x0 : -big; t->lo[1] = j > 0 ? y0 : -big;
  t->hi[0] = i < t->tiles_x - 1 ? x0 + t->pitch : big; t->hi[1] = j < t->tiles_y - 1 ? y0 + t->pitch : big;
  const double h = 2.0 * (double)t->P.graph_size + (double)t->P.voxel_size;
  // border strips of this rank's cloud, all-gathered; every rank keeps what falls into its own rectangle widened by the halo
  std::vector<float> strip;
  t->n_outside = 0;
  for (int64_t k = 0; k < n; ++k) {
    const double x = (double)xyz[k * sf], y = (double)xyz[k * sf + 1];
    if (x < t->lo[0] || x >= t->hi[0] || y < t->lo[1] || y >= t->hi[1]) ++t->n_outside;
    if (x < t->lo[0] + h || x >= t->hi[0] - h || y < t->lo[1] + h || y >= t->hi[1] - h) { strip.push_back(xyz[k * sf]); strip.push_back(xyz[k * sf + 1]); strip.push_back(xyz[k * sf + 2]); }
  }
  // Points a rank holds beyond its own region may come back unlabelled (their voxels are owned, and cut, elsewhere; found by
  // tools/fuzz_tiles.py): a caller with an arbitrary partition is told so once -- or, with VGS_TILES_OPT_STRICT_REGION, every
  // rank refuses the cloud (the count travels in the strips' size exchange below, so the ranks agree on it)
  if (t->n_outside > 0 && !t->strict_region && !t->warned_outside) {
    t->warned_outside = true;
    std::fprintf(stderr, "[vgs_tiles] rank %d: %lld of %lld points lie outside this rank's region; they may come back unlabelled (-1). "
                         "Load points by region, or set VGS_TILES_OPT_STRICT_REGION to make this an error.\n", c.rank, (long long)t->n_outside, (long long)n);
  }
  // a failure behind the last collective of the previous call (the label write-back at the end of vgs_tiles_run) has reached nobody
  // yet: it travels in this call's status word (it used to be cleared below and never arrived)
  vgs_status carry = t->pending;
  inject(t, PH_POINTS, carry);
  if (t->strict_region && t->n_outside > 0 && carry == VGS_OK) {
    carry = VGS_E_ARG;
    t->err = std::to_string(t->n_outside) + " points lie outside this rank's region (VGS_TILES_OPT_STRICT_REGION)";
  }
  {
    // agreed status before the payload: one word per rank
    const int64_t st = (int64_t)carry;
    std::vector<int64_t> all((size_t)c.world);
    TCOMM(c.all_gather(&st, all.data(), sizeof(int64_t)));
    TRY(agreed(t, carry, first_bad_rank(c.world, [&](int r) { return all[(size_t)r] != 0; }), "point loading"));
  }
  std::vector<std::vector<float>> strips;
  TCOMM(all_gather_varlen(c, strip, strips));
  // the local cloud in RANK ORDER: strips of lower ranks, own points, strips of higher ranks -- the order in which one process
  // would have inserted the points (a voxel's attributes depend on the order of its points; see dist.py)
  t->local.clear();
  auto take_strip = [&](int r) {
    const std::vector<float>& s = strips[(size_t)r];
    for (size_t k = 0; k + 2 < s.size(); k += 3) {
      const double x = (double)s[k], y = (double)s[k + 1];
      if (x >= t->lo[0] - h && x < t->hi[0] + h && y >= t->lo[1] - h && y < t->hi[1] + h) { t->local.push_back(s[k]); t->local.push_back(s[k + 1]); t->local.push_back(s[k + 2]); }
    }
  };
  for (int r = 0; r < c.rank; ++r) take_strip(r);
  t->own_first = (int64_t)(t->local.size() / 3);
  for (int64_t k = 0; k < n; ++k) { t->local.push_back(xyz[k * sf]); t->local.push_back(xyz[k * sf + 1]); t->local.push_back(xyz[k * sf + 2]); }
  for (int r = c.rank + 1; r < c.world; ++r) take_strip(r);
  t->n_own = n;
  // failures from here on are local and no collective follows inside this call: the rank returns its error AND keeps it
  // (t->pending), so that a caller who goes on to vgs_tiles_run all the same joins the grid's collective with that status in its
  // word instead of leaving its peers inside it
  t->pending = VGS_OK;
  auto local_step = [&](vgs_status s, const char* what) {
    if (s != VGS_OK && t->pending == VGS_OK) { t->pending = s; t->err = std::string(what) + ": " + vgs_last_error_string(t->ctx); }
  };
  inject(t, PH_UPLOAD, t->pending);
  if (t->pending == VGS_OK) local_step(vgs_set_points(t->ctx, t->local.data(), (int64_t)(t->local.size() / 3), 12), "vgs_set_points");
  if (t->pending == VGS_OK) local_step(vgs_set_owned_region(t->ctx, t->lo, t->hi), "vgs_set_owned_region");
  if (t->pending == VGS_OK) local_step(vgs_set_own_point_range(t->ctx, t->own_first, t->n_own), "vgs_set_own_point_range");
  return t->pending;
}

// The shared grid: what inserting the ranks' clouds one after the other does to the octree box.  One all-gather
// of the clouds' bounding boxes lets every rank replay the growth on the host wherever the box alone decides it
// (vgs_grid_advance_bbox); only a rank whose cloud leaves the step open scans its points on the GPU and broadcasts the state --
// except rank 0, whose box starts at its first point: it scans first and its state travels with its bounding box.
// `carry`: see TCARRY -- a local failure travels as a status word of the next collective.
static vgs_status chain_grid(vgs_tiles* t, vgs_status& carry) {
  Comm& c = *t->comm;
  float bb[6] = {0, 0, 0, 0, 0, 0};
  int64_t nf = 0;
  if (t->fail_phase == PH_GRID) carry = VGS_OK;   // (at this one site the injected failure has always replaced a kept one)
  inject(t, PH_GRID, carry);
  TCARRY(vgs_points_bbox(t->ctx, bb, &nf));
  auto pack = [](const vgs_grid_state& g, double* v) { for (int a = 0; a < 3; ++a) { v[a] = g.min[a]; v[3 + a] = (double)g.shift[a]; } v[6] = g.depth; v[7] = g.defined; };
  auto unpack = [](vgs_grid_state& g, const double* v) { for (int a = 0; a < 3; ++a) { g.min[a] = v[a]; g.shift[a] = (uint64_t)v[3 + a]; } g.depth = (int32_t)v[6]; g.defined = (int32_t)v[7]; };
  vgs_grid_state g0;
  vgs_grid_state_init(&g0);
  if (c.rank == 0 && nf > 0) TCARRY(vgs_grid_advance(t->ctx, &g0));
  double mine[16];
  for (int a = 0; a < 6; ++a) mine[a] = (double)bb[a];
  mine[6] = (double)nf;
  pack(g0, mine + 7);
  mine[15] = (double)carry;   // status word
  std::vector<double> all((size_t)16 * c.world);
  TCOMM(c.all_gather(mine, all.data(), sizeof(mine)));
  TRY(agreed(t, carry, first_bad_rank(c.world, [&](int r) { return all[(size_t)16 * r + 15] != 0.0; }), "grid"));
  vgs_grid_state g;
  vgs_grid_state_init(&g);
  for (int r = 0; r < c.world; ++r) {
    const double* v = all.data() + (size_t)16 * r;
    if (v[6] == 0) continue;   // no finite point: the cloud changes nothing
    if (r == 0) { unpack(g, v + 7); continue; }
    float box[6];
    for (int a = 0; a < 6; ++a) box[a] = (float)v[a];   // float values, exactly as gathered
    int32_t need = 0;
    vgs_status s = vgs_grid_advance_bbox(&g, (double)t->P.voxel_size, box, &need);   // host arithmetic on gathered values: fails on every rank alike
    if (s != VGS_OK) return tfail(t, s, "vgs_grid_advance_bbox");
    if (!need) continue;
    double buf[9] = {0};
    if (c.rank == r) { TCARRY(vgs_grid_advance(t->ctx, &g)); pack(g, buf); buf[8] = (double)carry; }
    TCOMM(c.bcast(buf, sizeof(buf), r));
    if (buf[8] != 0.0) return agreed(t, carry, r, "grid");
    unpack(g, buf);
  }
  TCARRY(vgs_set_grid_covering(t->ctx, &g));   // (every rank's cloud went into g, scanned or by its bounding box) a failure here travels with the boundary records
  return VGS_OK;
}

vgs_status vgs_tiles_run(vgs_tiles* t) {
  if (!t) return VGS_E_ARG;
  Comm& c = *t->comm;
  vgs_status carry = t->pending;   // a local failure behind the last collective of the previous call (upload, label write-back) travels now
  invalidate(t);
  Stopwatch sw(t->times);
  TRY(chain_grid(t, carry));
  sw.lap(VGS_TILES_T_GRID);
  inject(t, PH_STAGES, carry);
  TCARRY(vgs_voxelize(t->ctx)); TCARRY(vgs_features(t->ctx)); TCARRY(vgs_adjacency(t->ctx)); TCARRY(vgs_segment(t->ctx));
  sw.lap(VGS_TILES_T_STAGES);
  // only the border leaves the GPU: unique boundary voxels (code, local root, owned voxels of that root) and the number of
  // components that are local to this tile
  int64_t n = 0, nkl = 0;
  TCARRY(vgs_get_boundary_roots(t->ctx, &n, nullptr, nullptr, nullptr, &nkl));
  if (carry != VGS_OK) { n = 0; nkl = 0; }
  RankRecords mine;
  mine.code.resize((size_t)std::max<int64_t>(n, 1)); mine.root.resize(mine.code.size()); mine.cnt.resize(mine.code.size());
  if (n > 0) TCARRY(vgs_get_boundary_roots(t->ctx, &n, mine.code.data(), mine.root.data(), mine.cnt.data(), &nkl));
  if (carry != VGS_OK) { n = 0; nkl = 0; }
  mine.code.resize((size_t)n); mine.root.resize((size_t)n); mine.cnt.resize((size_t)n);
  t->n_records = n;
  sw.lap(VGS_TILES_T_RECORDS);
  // the one data-path exchange: header (record count, local segment count, this rank's status) + records, 3 words each
  constexpr size_t HDR = 3;
  std::vector<int64_t> payload(HDR + 3 * (size_t)n);
  payload[0] = n; payload[1] = nkl; payload[2] = (int64_t)carry;
  for (int64_t k = 0; k < n; ++k) { payload[HDR + (size_t)k] = (int64_t)mine.code[(size_t)k]; payload[HDR + (size_t)(n + k)] = mine.root[(size_t)k]; payload[HDR + (size_t)(2 * n + k)] = mine.cnt[(size_t)k]; }
  // one collective of a fixed size when every rank's payload fits; the gathered headers tell every rank alike when not
  const size_t cap = 3 * 8192 + HDR;
  std::vector<std::vector<int64_t>> gathered((size_t)c.world);
  {
    std::vector<int64_t> fixed(cap, 0), all(cap * (size_t)c.world);
    std::copy(payload.begin(), payload.begin() + (ptrdiff_t)std::min(payload.size(), cap), fixed.begin());
    TCOMM(c.all_gather(fixed.data(), all.data(), cap * sizeof(int64_t)));
    TRY(agreed(t, carry, first_bad_rank(c.world, [&](int r) { return all[cap * (size_t)r + 2] != 0; }), "stages"));
    bool fits = true;
    for (int r = 0; r < c.world; ++r) fits = fits && (HDR + 3 * (size_t)all[cap * (size_t)r]) <= cap;
    t->exch_sent = (int64_t)(cap * sizeof(int64_t)); t->exch_recv = t->exch_sent * c.world; t->exch_calls = 1;
    if (fits) for (int r = 0; r < c.world; ++r) gathered[(size_t)r].assign(all.begin() + (ptrdiff_t)(cap * (size_t)r), all.begin() + (ptrdiff_t)(cap * (size_t)r + HDR + 3 * (size_t)all[cap * (size_t)r]));
    else {
      // (a rank with more than 8192 boundary voxels -- a 10 M-point tile has 10^4 to 10^5: the sizes are known from the headers, but the
      // helper's own size word keeps the code path one; the payload is padded to the largest rank's)
      int64_t mx = 0;
      for (int r = 0; r < c.world; ++r) mx = std::max<int64_t>(mx, (int64_t)(HDR + 3 * (size_t)all[cap * (size_t)r]));
      TCOMM(all_gather_varlen(c, payload, gathered));
      t->exch_sent += (int64_t)sizeof(int64_t) * (1 + mx); t->exch_recv += (int64_t)sizeof(int64_t) * (1 + mx) * c.world; t->exch_calls += 2;
    }
  }
  sw.lap(VGS_TILES_T_EXCHANGE);
  std::vector<RankRecords> rec((size_t)c.world);
  std::vector<int64_t> kept_local((size_t)c.world);
  for (int r = 0; r < c.world; ++r) {
    const std::vector<int64_t>& gr = gathered[(size_t)r];
    const int64_t m = gr[0];
    kept_local[(size_t)r] = gr[1];
    RankRecords& R = rec[(size_t)r];
    R.code.resize((size_t)m); R.root.resize((size_t)m); R.cnt.resize((size_t)m);
    for (int64_t k = 0; k < m; ++k) { R.code[(size_t)k] = (uint64_t)gr[HDR + (size_t)k]; R.root[(size_t)k] = (int32_t)gr[HDR + (size_t)(m + k)]; R.cnt[(size_t)k] = (int32_t)gr[HDR + (size_t)(2 * m + k)]; }
  }
  std::vector<int64_t> base;
  std::vector<std::vector<int32_t>> uroot, ulabel;
  merge_boundary_compact(rec, kept_local, t->P.voxels_min, base, uroot, ulabel, t->kept);
  sw.lap(VGS_TILES_T_MERGE);
  std::vector<int32_t>& br = uroot[(size_t)c.rank];
  std::vector<int32_t>& bl = ulabel[(size_t)c.rank];
  int32_t dummy = 0;
  // (the run's last collective is behind us: the peers -- whose results are complete -- see a failure here in the status word of the
  // next collective, or at the launcher)
  TRY(behind_collective(t, vgs_apply_tile_labels(t->ctx, (int32_t)base[(size_t)c.rank], br.empty() ? &dummy : br.data(), bl.empty() ? &dummy : bl.data(), (int64_t)br.size()),
                        "vgs_apply_tile_labels"));
  sw.lap(VGS_TILES_T_LABELS);
  sw.total(VGS_TILES_T_TOTAL);
  for (RankRecords& R : rec) { R.cnt.clear(); R.cnt.shrink_to_fit(); }
  t->run_rec.swap(rec); t->run_uroot.swap(uroot); t->run_ulabel.swap(ulabel);   // (kept for the segment graph's halo labels; nothing is copied)
  t->ran = true;
  return VGS_OK;
}

// ------------------------------------------------------------------------------------------------ tables of the node labelling
// The table into t->desc: the moment collective when it is not cached (vgs_tiles_get_segment_boxes takes the table through here too).
static vgs_status ensure_descriptors(vgs_tiles* t, const char* fn) {   // fn: the public function that was called, for the guard's message
  if (t->desc_valid) return VGS_OK;
  const Labelling L = node_labelling(t, fn, PH_DESCRIPTORS);
  vgs_status carry;
  TRY(open_collective(t, fn, L.phase, carry));
  double ms[T_COUNT] = {0};
  MomentSent sent;
  TRY(moment_collective(t, L, carry, ms, t->desc, sent));
  std::copy(ms, ms + T_COUNT, t->dtimes);
  t->desc_valid = true;
  return VGS_OK;
}

vgs_status vgs_tiles_get_segment_descriptors(vgs_tiles* t, int64_t* K, int64_t* n_points, int32_t* n_nodes, float* bbox6, double* centroid3,
                                             double* cov6, double* evals3, double* evecs9, float* eigen8) {
  if (!t) return VGS_E_ARG;
  if (K) *K = t->kept;
  if (!n_points && !n_nodes && !bbox6 && !centroid3 && !cov6 && !evals3 && !evecs9 && !eigen8) return VGS_OK;   // size query: no collective
  TRY(ensure_descriptors(t, "vgs_tiles_get_segment_descriptors"));
  put_descriptors(t->desc, n_points, n_nodes, bbox6, centroid3, cov6, evals3, evecs9, eigen8);
  return VGS_OK;
}

vgs_status vgs_tiles_get_descriptor_times(vgs_tiles* t, double* ms, int32_t n) { return get_times(t, &vgs_tiles::dtimes, ms, n); }

// ------------------------------------------------------------------------------------------------ tables of a caller's point labelling
// Descriptors: the moment collective of THIS labelling.  Nothing is cached (the input is the caller's), so every call is collective.
static vgs_status tiles_label_descriptors(vgs_tiles* t, const Labelling& L, int64_t* n_skipped, int64_t* n_points, int32_t* n_nodes, float* bbox6,
                                          double* centroid3, double* cov6, double* evals3, double* evecs9, float* eigen8) {
  vgs_status carry;
  TRY(open_collective(t, L.fn, L.phase, carry));
  double ms[T_COUNT] = {0};
  DescTable D;
  MomentSent sent;
  TRY(moment_collective(t, L, carry, ms, D, sent));
  std::copy(ms, ms + T_COUNT, t->ltimes);
  t->l_own = sent.own; t->l_pairs = sent.pairs; t->l_bytes = sent.bytes;
  if (n_skipped) *n_skipped = D.n_skipped;
  put_descriptors(D, n_points, n_nodes, bbox6, centroid3, cov6, evals3, evecs9, eigen8);
  return VGS_OK;
}

vgs_status vgs_tiles_point_label_descriptors(vgs_tiles* t, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_skipped, int64_t* n_points,
                                             int32_t* n_nodes, float* bbox6, double* centroid3, double* cov6, double* evals3, double* evecs9,
                                             float* eigen8) {
  if (!t) return VGS_E_ARG;
  return tiles_label_descriptors(t, point_labelling("vgs_tiles_point_label_descriptors", false, labels_host, n, K), n_skipped, n_points, n_nodes, bbox6, centroid3,
                                 cov6, evals3, evecs9, eigen8);
}

vgs_status vgs_tiles_point_label_descriptors_device(vgs_tiles* t, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_skipped, int64_t* n_points,
                                                    int32_t* n_nodes, float* bbox6, double* centroid3, double* cov6, double* evals3, double* evecs9,
                                                    float* eigen8) {
  if (!t) return VGS_E_ARG;
  return tiles_label_descriptors(t, point_labelling("vgs_tiles_point_label_descriptors_device", true, labels_dev, n, K), n_skipped, n_points, n_nodes, bbox6,
                                 centroid3, cov6, evals3, evecs9, eigen8);
}

// Boxes: TWO collectives -- the moment collective of THIS labelling, then the extent collective about its rows.  A bad frame travels in the
// first status word.  Nothing outlives the call; the times are the sums over both collectives, the bytes too.
static vgs_status tiles_label_boxes(vgs_tiles* t, const Labelling& L, int32_t frame, double* center3, double* half3, double* frame9, double* lo3, double* hi3) {
  vgs_status carry;
  TRY(open_collective(t, L.fn, L.phase, carry));
  if (carry == VGS_OK && bad_frame(t, L.fn, frame)) carry = VGS_E_ARG;
  double ms[T_COUNT] = {0}, ms2[T_COUNT] = {0};
  DescTable D;
  MomentSent sent;
  TRY(first_of_two(t, [&] { return moment_collective(t, L, carry, ms, D, sent); }));
  BoxTable B;
  int64_t bytes = 0;
  TRY(extent_collective(t, L, frame, t->pending, D, ms2, B, bytes));
  for (int i = 0; i < T_COUNT; ++i) t->ltimes[i] = ms[i] + ms2[i];
  t->l_own = sent.own; t->l_pairs = sent.pairs; t->l_bytes = sent.bytes + bytes;
  put_boxes(B, center3, half3, frame9, lo3, hi3);
  return VGS_OK;
}

vgs_status vgs_tiles_point_label_boxes(vgs_tiles* t, const int32_t* labels_host, int64_t n, int64_t K, int32_t frame, double* center3, double* half3,
                                       double* frame9, double* lo3, double* hi3) {
  if (!t) return VGS_E_ARG;
  return tiles_label_boxes(t, point_labelling("vgs_tiles_point_label_boxes", false, labels_host, n, K), frame, center3, half3, frame9, lo3, hi3);
}

vgs_status vgs_tiles_point_label_boxes_device(vgs_tiles* t, const int32_t* labels_dev, int64_t n, int64_t K, int32_t frame, double* center3,
                                              double* half3, double* frame9, double* lo3, double* hi3) {
  if (!t) return VGS_E_ARG;
  return tiles_label_boxes(t, point_labelling("vgs_tiles_point_label_boxes_device", true, labels_dev, n, K), frame, center3, half3, frame9, lo3, hi3);
}

vgs_status vgs_tiles_get_point_label_times(vgs_tiles* t, double* ms, int32_t n) { return get_times(t, &vgs_tiles::ltimes, ms, n); }

vgs_status vgs_tiles_get_point_label_payload(vgs_tiles* t, int64_t* own_records, int64_t* own_pairs, int64_t* bytes_sent) {
  if (!t) return VGS_E_ARG;
  if (own_records) *own_records = t->l_own;
  if (own_pairs) *own_pairs = t->l_pairs;
  if (bytes_sent) *bytes_sent = t->l_bytes;
  return VGS_OK;
}

// host arithmetic only (tests): the pair fold on flattened per-rank records
vgs_status vgs_tiles_fold_label_pairs(int world, const int64_t* rec_off, const uint64_t* code, const int32_t* label, int64_t K, int32_t* n_nodes_add) {
  if (world < 1 || !rec_off || K < 0 || (K > 0 && !n_nodes_add)) return VGS_E_ARG;
  if (rec_off[world] > 0 && (!code || !label)) return VGS_E_ARG;
  std::vector<std::vector<PairRec>> ranks((size_t)world);
  for (int r = 0; r < world; ++r) {
    if (rec_off[r + 1] < rec_off[r]) return VGS_E_ARG;
    for (int64_t i = rec_off[r]; i < rec_off[r + 1]; ++i) { PairRec p; p.code = code[i]; p.label = label[i]; ranks[(size_t)r].push_back(p); }
  }
  std::vector<int32_t> add;
  if (!fold_label_pairs(ranks, K, add)) return VGS_E_ARG;
  std::copy(add.begin(), add.end(), n_nodes_add);
  return VGS_OK;
}

// Boxes of the node labelling: the global descriptor table (its own collective when it is not cached; its guard is this call's), then the
// extent collective about its rows; cached per frame.  A bad frame is refused here, before any collective.
vgs_status vgs_tiles_get_segment_boxes(vgs_tiles* t, int32_t frame, int64_t* K, double* center3, double* half3, double* frame9, double* lo3,
                                       double* hi3) {
  const char* fn = "vgs_tiles_get_segment_boxes";
  if (!t) return VGS_E_ARG;
  if (bad_frame(t, fn, frame)) return VGS_E_ARG;
  if (K) *K = t->kept;
  if (!center3 && !half3 && !frame9 && !lo3 && !hi3) return VGS_OK;   // size query: no collective
  if (!t->box_valid[frame]) {
    TRY(first_of_two(t, [&] { return ensure_descriptors(t, fn); }));
    const Labelling L = node_labelling(t, fn, PH_BOXES);
    vgs_status carry;
    TRY(open_collective(t, fn, L.phase, carry));   // (takes up a failure behind the descriptor collective)
    double ms[T_COUNT] = {0};
    int64_t bytes = 0;
    TRY(extent_collective(t, L, frame, carry, t->desc, ms, t->box[frame], bytes));
    std::copy(ms, ms + T_COUNT, t->btimes);
    t->box_valid[frame] = true;
  }
  put_boxes(t->box[frame], center3, half3, frame9, lo3, hi3);
  return VGS_OK;
}

vgs_status vgs_tiles_get_box_times(vgs_tiles* t, double* ms, int32_t n) { return get_times(t, &vgs_tiles::btimes, ms, n); }

// host arithmetic only (tests): the extent fold on flattened per-rank records
vgs_status vgs_tiles_fold_extents(int world, const int64_t* rec_off, const int32_t* label, const double* lo3, const double* hi3, int64_t K,
                                  double* lo3_out, double* hi3_out, uint8_t* reached_out) {
  if (world < 1 || !rec_off || K < 0 || (K > 0 && (!lo3_out || !hi3_out || !reached_out))) return VGS_E_ARG;
  if (rec_off[world] > 0 && (!label || !lo3 || !hi3)) return VGS_E_ARG;
  std::vector<std::vector<ExtentRec>> ranks((size_t)world);
  for (int r = 0; r < world; ++r) {
    if (rec_off[r + 1] < rec_off[r]) return VGS_E_ARG;
    for (int64_t i = rec_off[r]; i < rec_off[r + 1]; ++i) ranks[(size_t)r].push_back(pack_extent(label, lo3, hi3, (size_t)i));
  }
  std::vector<double> lo, hi;
  std::vector<uint8_t> reached;
  if (!fold_extents(ranks, K, lo, hi, reached)) return VGS_E_ARG;
  std::copy(lo.begin(), lo.end(), lo3_out); std::copy(hi.begin(), hi.end(), hi3_out); std::copy(reached.begin(), reached.end(), reached_out);
  return VGS_OK;
}

// ------------------------------------------------------------------------------------------------ attribute statistics
// the node labelling: row k covers the points that the run labels k, K = kept rows
vgs_status vgs_tiles_segment_field_stats(vgs_tiles* t, const float* field_host, int64_t n, int32_t n_channels, int64_t stride_bytes, int64_t* K,
                                         int64_t* n_valid, double* anchor, double* mean, double* var, float* vmin, float* vmax) {
  if (!t) return VGS_E_ARG;
  if (K) *K = t->kept;
  return attribute_collective(t, node_labelling(t, "vgs_tiles_segment_field_stats", PH_FIELDS), FieldCodec(field_host, n, n_channels, stride_bytes, n_valid, anchor, mean, var, vmin, vmax), nullptr);
}

vgs_status vgs_tiles_segment_field_stats_device(vgs_tiles* t, const float* field_dev, int64_t n, int32_t n_channels, int64_t stride_bytes, int64_t* K,
                                                int64_t* n_valid, double* anchor, double* mean, double* var, float* vmin, float* vmax) {
  if (!t) return VGS_E_ARG;
  if (K) *K = t->kept;
  return attribute_collective(t, node_labelling(t, "vgs_tiles_segment_field_stats_device", PH_FIELDS, true), FieldCodec(field_dev, n, n_channels, stride_bytes, n_valid, anchor, mean, var, vmin, vmax), nullptr);
}

vgs_status vgs_tiles_segment_class_histogram(vgs_tiles* t, const int32_t* cls_host, int64_t n, int32_t n_classes, int64_t* K, int64_t* hist,
                                             int64_t* n_outside, int32_t* majority, int64_t* majority_count) {
  if (!t) return VGS_E_ARG;
  if (K) *K = t->kept;
  return attribute_collective(t, node_labelling(t, "vgs_tiles_segment_class_histogram", PH_FIELDS), ClassCodec(cls_host, n, n_classes, hist, n_outside, majority, majority_count), nullptr);
}

vgs_status vgs_tiles_segment_class_histogram_device(vgs_tiles* t, const int32_t* cls_dev, int64_t n, int32_t n_classes, int64_t* K, int64_t* hist,
                                                    int64_t* n_outside, int32_t* majority, int64_t* majority_count) {
  if (!t) return VGS_E_ARG;
  if (K) *K = t->kept;
  return attribute_collective(t, node_labelling(t, "vgs_tiles_segment_class_histogram_device", PH_FIELDS, true), ClassCodec(cls_dev, n, n_classes, hist, n_outside, majority, majority_count), nullptr);
}

// a caller's point labelling: row k covers the own points, over all ranks, that the caller labels k, K rows of the caller's
vgs_status vgs_tiles_point_label_field_stats(vgs_tiles* t, const int32_t* labels_host, int64_t K, const float* field_host, int64_t n, int32_t n_channels,
                                             int64_t stride_bytes, int64_t* n_skipped, int64_t* n_valid, double* anchor, double* mean, double* var,
                                             float* vmin, float* vmax) {
  if (!t) return VGS_E_ARG;
  return attribute_collective(t, point_labelling("vgs_tiles_point_label_field_stats", false, labels_host, n, K), FieldCodec(field_host, n, n_channels, stride_bytes, n_valid, anchor, mean, var, vmin, vmax), n_skipped);
}

vgs_status vgs_tiles_point_label_field_stats_device(vgs_tiles* t, const int32_t* labels_dev, int64_t K, const float* field_dev, int64_t n,
                                                    int32_t n_channels, int64_t stride_bytes, int64_t* n_skipped, int64_t* n_valid, double* anchor,
                                                    double* mean, double* var, float* vmin, float* vmax) {
  if (!t) return VGS_E_ARG;
  return attribute_collective(t, point_labelling("vgs_tiles_point_label_field_stats_device", true, labels_dev, n, K), FieldCodec(field_dev, n, n_channels, stride_bytes, n_valid, anchor, mean, var, vmin, vmax), n_skipped);
}

vgs_status vgs_tiles_point_label_class_histogram(vgs_tiles* t, const int32_t* labels_host, int64_t K, const int32_t* cls_host, int64_t n, int32_t n_classes,
                                                 int64_t* n_skipped, int64_t* hist, int64_t* n_outside, int32_t* majority, int64_t* majority_count) {
  if (!t) return VGS_E_ARG;
  return attribute_collective(t, point_labelling("vgs_tiles_point_label_class_histogram", false, labels_host, n, K), ClassCodec(cls_host, n, n_classes, hist, n_outside, majority, majority_count), n_skipped);
}

vgs_status vgs_tiles_point_label_class_histogram_device(vgs_tiles* t, const int32_t* labels_dev, int64_t K, const int32_t* cls_dev, int64_t n,
                                                        int32_t n_classes, int64_t* n_skipped, int64_t* hist, int64_t* n_outside, int32_t* majority,
                                                        int64_t* majority_count) {
  if (!t) return VGS_E_ARG;
  return attribute_collective(t, point_labelling("vgs_tiles_point_label_class_histogram_device", true, labels_dev, n, K), ClassCodec(cls_dev, n, n_classes, hist, n_outside, majority, majority_count), n_skipped);
}

vgs_status vgs_tiles_get_field_times(vgs_tiles* t, double* ms, int32_t n) { return get_times(t, &vgs_tiles::ftimes, ms, n); }

vgs_status vgs_tiles_get_field_payload(vgs_tiles* t, int64_t* own_records, int64_t* bytes_sent) {
  if (!t) return VGS_E_ARG;
  if (own_records) *own_records = t->f_own;
  if (bytes_sent) *bytes_sent = t->f_bytes;
  return VGS_OK;
}

// ------------------------------------------------------------------------------------------------ score against reference labels
// The comparison over the ranks: no label and no reference id travels, every point is counted by the rank that loaded it.  This rank's
// cells over its own points (one small pipeline on its GPU) -> ONE all_gather_varlen of int64 words: a header of status word, own cell
// count and own unannotated count, then per cell (L + 1) << 32 | g and the count -> the lists in rank order into
// vgs_label_comparison_from_cells on this rank's context, which merges them and builds the tables on the GPU: there is no host fold.
// Nothing is cached (the input is the caller's), so every call is collective.  Everything a rank can get wrong on its own -- n, a NULL
// input, a failing context call -- is found by the context call and travels in the status word.
// POINT (vgs_tiles_compare_point_labels): the cells pair a labelling of the caller's (seg, K_in rows; vgs_own_point_label_cells) with ref
// instead of the run's labels; K_in travels as one more word behind the cells, and ranks that pass different K all leave with VGS_E_ARG.
static vgs_status tiles_compare(vgs_tiles* t, const char* fn, bool on_device, const int32_t* ref, int64_t n, int64_t* K, int64_t* n_cells,
                                int64_t* n_refs, int64_t* summary, bool point = false, const int32_t* seg = nullptr, int64_t K_in = 0) {
  if (!t) return VGS_E_ARG;
  if (K) *K = t->kept;
  vgs_status carry;
  TRY(open_collective(t, fn, point ? PH_POINT_LABELS : PH_COMPARE, carry));
  const int64_t Kg = point ? K_in : t->kept;
  t->cmp_valid = false;
  double ms[VGS_TILES_C_COUNT] = {0};
  Stopwatch sw(ms);
  std::vector<int64_t> payload(3, 0);
  int64_t n_own_cells = 0, n_unann = 0;
  if (carry == VGS_OK) {
    if (point)
      TCARRY_AS(on_device ? vgs_own_point_label_cells_device : vgs_own_point_label_cells,
                on_device ? "vgs_own_point_label_cells_device" : "vgs_own_point_label_cells", t->ctx, Kg, seg, ref, n, &n_own_cells, &n_unann);
    else
      TCARRY_AS(on_device ? vgs_own_label_cells_device : vgs_own_label_cells, on_device ? "vgs_own_label_cells_device" : "vgs_own_label_cells", t->ctx, Kg, ref, n, &n_own_cells, &n_unann);
    std::vector<int32_t> cs((size_t)n_own_cells + 1), cr((size_t)n_own_cells + 1);
    std::vector<int64_t> cn((size_t)n_own_cells + 1);
    if (carry == VGS_OK) TCARRY(vgs_get_own_label_cells(t->ctx, cs.data(), cr.data(), cn.data()));
    if (carry == VGS_OK) {
      payload.resize(3 + 2 * (size_t)n_own_cells);
      for (size_t i = 0; i < (size_t)n_own_cells; ++i) {
        payload[3 + 2 * i] = (int64_t)(((uint64_t)(uint32_t)(cs[i] + 1) << 32) | (uint64_t)(uint32_t)cr[i]);
        payload[4 + 2 * i] = cn[i];
      }
    } else { n_own_cells = 0; n_unann = 0; }
  }
  set_header(payload, carry, n_own_cells, n_unann);
  if (point) payload.push_back(Kg);
  sw.lap(VGS_TILES_C_OWN);
  std::vector<std::vector<int64_t>> gathered;
  TRY(exchange(t, carry, payload, point ? "point_labels" : "compare", sw, VGS_TILES_C_EXCHANGE, gathered));
  if (point) {
    for (size_t r = 1; r < gathered.size(); ++r)
      if (gathered[r].back() != gathered[0].back()) return disagree(t, fn, r, "K", gathered[r].back(), gathered[0].back());
    for (std::vector<int64_t>& g : gathered) g.pop_back();
  }
  TRY(check_payloads(t, fn, gathered, 3, 2, {}));   // (the third header word is the rank's own figure: nothing to agree on)
  size_t n_in = 0;
  int64_t unann = 0;
  for (const std::vector<int64_t>& g : gathered) { n_in += (size_t)g[1]; unann += g[2]; }
  std::vector<int32_t> as(n_in + 1), ar(n_in + 1);
  std::vector<int64_t> an(n_in + 1);
  size_t o = 0;
  for (const std::vector<int64_t>& g : gathered) {
    for (size_t i = 0; i < (size_t)g[1]; ++i, ++o) {
      const uint64_t w = (uint64_t)g[3 + 2 * i];
      as[o] = (int32_t)(uint32_t)(w >> 32) - 1; ar[o] = (int32_t)(uint32_t)w; an[o] = g[4 + 2 * i];
    }
  }
  TRY(behind_collective(t, vgs_label_comparison_from_cells(t->ctx, Kg, (int64_t)n_in, as.data(), ar.data(), an.data(), unann, n_cells, n_refs, summary), "vgs_label_comparison_from_cells"));
  sw.lap(VGS_TILES_C_TABLES);
  sw.total(VGS_TILES_C_TOTAL, t->ctimes);
  t->c_own = n_own_cells; t->c_bytes = (int64_t)(payload.size() * sizeof(int64_t));
  t->cmp_valid = true;
  return VGS_OK;
}

vgs_status vgs_tiles_compare_labels(vgs_tiles* t, const int32_t* ref_host, int64_t n, int64_t* K, int64_t* n_cells, int64_t* n_refs, int64_t* summary) {
  return tiles_compare(t, "vgs_tiles_compare_labels", false, ref_host, n, K, n_cells, n_refs, summary);
}

vgs_status vgs_tiles_compare_labels_device(vgs_tiles* t, const int32_t* ref_dev, int64_t n, int64_t* K, int64_t* n_cells, int64_t* n_refs,
                                           int64_t* summary) {
  return tiles_compare(t, "vgs_tiles_compare_labels_device", true, ref_dev, n, K, n_cells, n_refs, summary);
}

vgs_status vgs_tiles_compare_point_labels(vgs_tiles* t, const int32_t* seg_labels_host, int64_t K, const int32_t* ref_host, int64_t n, int64_t* n_cells,
                                          int64_t* n_refs, int64_t* summary) {
  return tiles_compare(t, "vgs_tiles_compare_point_labels", false, ref_host, n, nullptr, n_cells, n_refs, summary, true, seg_labels_host, K);
}

vgs_status vgs_tiles_compare_point_labels_device(vgs_tiles* t, const int32_t* seg_labels_dev, int64_t K, const int32_t* ref_dev, int64_t n,
                                                 int64_t* n_cells, int64_t* n_refs, int64_t* summary) {
  return tiles_compare(t, "vgs_tiles_compare_point_labels_device", true, ref_dev, n, nullptr, n_cells, n_refs, summary, true, seg_labels_dev, K);
}

vgs_status vgs_tiles_get_label_comparison(vgs_tiles* t, int32_t* cell_seg, int32_t* cell_ref, int64_t* cell_n, int32_t* ref_id, int64_t* ref_points,
                                          int64_t* ref_dropped, int32_t* ref_best_seg, int64_t* ref_best_n, double* ref_best_iou,
                                          int64_t* seg_annotated, int32_t* seg_refs, int32_t* seg_best_ref, int64_t* seg_best_n, double* seg_best_iou) {
  if (!t) return VGS_E_ARG;
  if (!t->ran || !t->cmp_valid)
    return tfail(t, VGS_E_STATE, "vgs_tiles_get_label_comparison: no comparison since the last run or the last vgs_tiles_set_points (vgs_tiles_compare_labels first)");
  TCTX(vgs_get_label_comparison(t->ctx, cell_seg, cell_ref, cell_n, ref_id, ref_points, ref_dropped, ref_best_seg, ref_best_n, ref_best_iou, seg_annotated,
                                seg_refs, seg_best_ref, seg_best_n, seg_best_iou));
  return VGS_OK;
}

vgs_status vgs_tiles_get_compare_times(vgs_tiles* t, double* ms, int32_t n) { return get_times(t, &vgs_tiles::ctimes, ms, n); }

vgs_status vgs_tiles_get_compare_payload(vgs_tiles* t, int64_t* own_cells, int64_t* bytes_sent) {
  if (!t) return VGS_E_ARG;
  if (own_cells) *own_cells = t->c_own;
  if (bytes_sent) *bytes_sent = t->c_bytes;
  return VGS_OK;
}

// ------------------------------------------------------------------------------------------------ point-level label refinement
// The refinement over the ranks (include/vgs_tiles.h): this rank's band records, compacted on its GPU (first call after a run only) -> ONE
// all_gather_varlen of 16-byte records behind a header of status word, record count and the three parameters -> the halo table of the
// refinement in the context: the band records of the other ranks and, for the codes they do not name, the run's boundary records as the
// segment graph uses them -> this rank's share of the rule on its GPU (vgs_refine_own_point_labels).  No label of a point travels.
vgs_status vgs_tiles_refine_point_labels(vgs_tiles* t, const vgs_refine_params* rp_in, int64_t* counts) {
  if (!t) return VGS_E_ARG;
  vgs_status carry;
  TRY(open_collective(t, "vgs_tiles_refine_point_labels", PH_REFINE, carry));
  Comm& c = *t->comm;
  t->rf_valid = false;
  double ms[VGS_TILES_R_COUNT] = {0};
  Stopwatch sw(ms);
  vgs_refine_params rp;
  if (rp_in) rp = *rp_in;
  else TCARRY(vgs_refine_params_default(t->ctx, &rp));
  if (carry != VGS_OK && !rp_in) { rp.patch_radius = 0.f; rp.switch_ratio = 0.f; rp.fill = 0; }
  rp.fill = rp.fill ? 1 : 0;
  // what a rank can get wrong on its own travels in the status word (the context would refuse the same values behind the exchange)
  if (carry == VGS_OK && (!(rp.patch_radius >= 0.f) || !std::isfinite(rp.patch_radius))) { carry = VGS_E_ARG; t->err = "vgs_tiles_refine_point_labels: patch_radius must be finite and not negative"; }
  if (carry == VGS_OK && !(rp.switch_ratio >= 0.f && rp.switch_ratio <= 1.f)) { carry = VGS_E_ARG; t->err = "vgs_tiles_refine_point_labels: switch_ratio must lie in [0, 1]"; }
  const bool send_band = !t->band_valid;   // (the same on every rank: set behind an exchange every rank saw succeed, dropped by run / set_points)
  std::vector<BandRec> payload(2);
  if (send_band && carry == VGS_OK) {
    int64_t n = 0;
    TCARRY(vgs_get_own_band_labels(t->ctx, &n, nullptr, nullptr));
    if (carry == VGS_OK && n > 0) {
      std::vector<uint64_t> code((size_t)n);
      std::vector<int32_t> lab((size_t)n);
      TCARRY(vgs_get_own_band_labels(t->ctx, &n, code.data(), lab.data()));
      if (carry == VGS_OK) {
        payload.resize(2 + (size_t)n);
        for (size_t i = 0; i < (size_t)n; ++i) { payload[2 + i].code = code[i]; payload[2 + i].label = lab[i]; }
      }
    }
  }
  payload[0].code = (uint64_t)(uint32_t)carry; payload[0].label = rp.fill;
  payload[1].code = (uint64_t)(payload.size() - 2);
  std::memcpy(&payload[1].label, &rp.patch_radius, 4); std::memcpy(&payload[1].pad, &rp.switch_ratio, 4);
  sw.lap(VGS_TILES_R_BAND);
  std::vector<std::vector<BandRec>> gathered;
  TRY(exchange(t, carry, payload, "refine", sw, VGS_TILES_R_EXCHANGE, gathered));
  for (size_t r = 0; r < gathered.size(); ++r)
    if (gathered[r].size() != 2 + (size_t)gathered[r][1].code) return tfail(t, VGS_E_STATE, "vgs_tiles_refine_point_labels: rank " + std::to_string(r) + " sent a payload of the wrong size");
  // every rank was valid on its own; they must also describe the same refinement (the precedent of n_channels)
  vgs_status verdict = VGS_OK;
  for (size_t r = 1; r < gathered.size() && verdict == VGS_OK; ++r) {
    const BandRec *a = gathered[r].data(), *b = gathered[0].data();
    float pr[2], sr[2];
    std::memcpy(&pr[0], &a[1].label, 4); std::memcpy(&pr[1], &b[1].label, 4); std::memcpy(&sr[0], &a[1].pad, 4); std::memcpy(&sr[1], &b[1].pad, 4);
    if (a[0].label != b[0].label || pr[0] != pr[1] || sr[0] != sr[1]) {   // as values: 0.0 and -0.0 agree (no NaN gets here: it fails its own rank)
      verdict = tfail(t, VGS_E_ARG, "vgs_tiles_refine_point_labels: rank " + std::to_string(r) + " passed (patch_radius, switch_ratio, fill) = (" + std::to_string(pr[0]) + ", " +
                                        std::to_string(sr[0]) + ", " + std::to_string(a[0].label) + "), rank 0 passed (" + std::to_string(pr[1]) + ", " + std::to_string(sr[1]) + ", " +
                                        std::to_string(b[0].label) + ")");
    }
  }
  if (send_band) {
    // The band has travelled on every rank alike: the flag follows that verdict, not this rank's upload below.  A rank whose upload fails
    // returns its error, keeps it pending, and holds no table until the next run (its context answers VGS_E_STATE); it does not send its
    // band a second time into headers-only peers.
    t->band_valid = true;
    // The halo table: the owners' band records first; a boundary record of the run adds a code that no band record names (a voxel whose
    // cube crosses the border lies in the band, so these are voxels beyond it that the graph's rows reach).  One entry per code.
    std::vector<uint64_t> hcode;
    std::vector<int32_t> hlab;
    for (int r = 0; r < c.world; ++r) {
      if (r == c.rank) continue;
      for (size_t i = 2; i < gathered[(size_t)r].size(); ++i) { hcode.push_back(gathered[(size_t)r][i].code); hlab.push_back(gathered[(size_t)r][i].label); }
    }
    std::vector<uint64_t> named(hcode);
    std::sort(named.begin(), named.end());
    if (t->run_rec.size() == (size_t)c.world) {
      std::vector<std::pair<uint64_t, int32_t>> extra;
      for (int r = 0; r < c.world; ++r) {
        if (r == c.rank) continue;
        const RankRecords& R = t->run_rec[(size_t)r];
        const std::vector<int32_t>& ur = t->run_uroot[(size_t)r];
        const std::vector<int32_t>& ul = t->run_ulabel[(size_t)r];
        for (size_t k = 0; k < R.code.size(); ++k) {
          if (std::binary_search(named.begin(), named.end(), R.code[k])) continue;
          extra.emplace_back(R.code[k], ul[(size_t)(std::lower_bound(ur.begin(), ur.end(), R.root[k]) - ur.begin())]);
        }
      }
      std::stable_sort(extra.begin(), extra.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
      for (size_t k = 0; k < extra.size(); ++k)
        if (k == 0 || extra[k].first != extra[k - 1].first) { hcode.push_back(extra[k].first); hlab.push_back(extra[k].second); }   // (the lowest rank's record of a code)
    }
    const uint64_t no_code = 0;
    const int32_t no_lab = 0;
    TRY(behind_collective(t, vgs_set_refine_halo_labels(t->ctx, hcode.empty() ? &no_code : hcode.data(), hlab.empty() ? &no_lab : hlab.data(), (int64_t)hcode.size()),
                          "vgs_set_refine_halo_labels"));
  }
  sw.lap(VGS_TILES_R_TABLE);
  if (verdict != VGS_OK) return verdict;
  int64_t cnt[5] = {0, 0, 0, 0, 0};
  TRY(behind_collective(t, vgs_refine_own_point_labels(t->ctx, &rp, cnt), "vgs_refine_own_point_labels"));
  sw.lap(VGS_TILES_R_REFINE);
  sw.total(VGS_TILES_R_TOTAL, t->rtimes);
  if (counts) std::copy(cnt, cnt + 5, counts);
  t->r_band = (int64_t)payload.size() - 2; t->r_bytes = (int64_t)(payload.size() * sizeof(BandRec));
  t->rf_valid = true;
  return VGS_OK;
}

vgs_status vgs_tiles_get_refined_labels(vgs_tiles* t, int32_t* labels) {
  if (!t || (!labels && t->n_own > 0)) return VGS_E_ARG;
  if (!t->ran || !t->rf_valid)
    return tfail(t, VGS_E_STATE, "vgs_tiles_get_refined_labels: no refinement since the last run or the last vgs_tiles_set_points (vgs_tiles_refine_point_labels first)");
  const int32_t* dev = nullptr;
  TCTX(vgs_get_refined_labels_device(t->ctx, &dev));
  // the own range only: the rest of the context's cloud belongs to other ranks (the refine call has waited for its kernels)
  if (t->n_own > 0) {
    hipError_t e = hipSetDevice(t->P.device);
    if (e == hipSuccess) e = hipMemcpy(labels, dev + t->own_first, (size_t)t->n_own * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return tfail(t, VGS_E_HIP, std::string("vgs_tiles_get_refined_labels: ") + hipGetErrorString(e));
  }
  return VGS_OK;
}

vgs_status vgs_tiles_get_refine_times(vgs_tiles* t, double* ms, int32_t n) { return get_times(t, &vgs_tiles::rtimes, ms, n); }

vgs_status vgs_tiles_get_refine_payload(vgs_tiles* t, int64_t* band_records, int64_t* bytes_sent) {
  if (!t) return VGS_E_ARG;
  if (band_records) *band_records = t->r_band;
  if (bytes_sent) *bytes_sent = t->r_bytes;
  return VGS_OK;
}

// ------------------------------------------------------------------------------------------------ parts of a labelling
// The fold of vgs_tiles_point_label_components, the same on every rank (include/vgs_tiles.h): a union-find over (rank, local part) --
// unite along the links, unite along EQUAL (code, label) keys among the band records of different ranks (the shared voxel; a key with m
// records is one node, m - 1 comes off the merged part's node count) -- then label, points (sum), nodes (sum - surplus) and first code
// (max) of every part, sorted by (label ascending, first code descending).  Flat arrays, rank r's entries being off[r] .. off[r + 1].
namespace {
struct PartsIn {
  int world; int64_t K;
  const int64_t* p_off; const int32_t* p_label; const int64_t* p_points; const int32_t* p_nodes; const uint64_t* p_code;
  const int64_t* b_off; const uint64_t* b_code; const int32_t* b_label; const int32_t* b_part;
  const int64_t* l_off; const int32_t* l_own; const int32_t* l_rank; const int32_t* l_part;
};
struct PartsOut {
  std::vector<int32_t> map, label, nodes, largest;
  std::vector<int64_t> points, first;
  std::vector<uint64_t> code;
};
// false: `why` says what the records got wrong
bool fold_label_parts(const PartsIn& I, PartsOut& O, std::string& why) {
  const int world = I.world;
  const int64_t K = I.K;
  for (int r = 0; r < world; ++r)
    if (I.p_off[r + 1] < I.p_off[r] || I.b_off[r + 1] < I.b_off[r] || I.l_off[r + 1] < I.l_off[r]) { why = "offsets must not decrease"; return false; }
  if (I.p_off[0] != 0 || I.b_off[0] != 0 || I.l_off[0] != 0) { why = "offsets must start at 0"; return false; }
  const size_t P = (size_t)I.p_off[world];
  if (P > (size_t)0x7fffffff) { why = "more than 2^31 - 1 local parts"; return false; }
  for (size_t p = 0; p < P; ++p)
    if (I.p_label[p] < 0 || (int64_t)I.p_label[p] >= K) { why = "part " + std::to_string(p) + " carries label " + std::to_string(I.p_label[p]) + ", outside 0 .. K-1"; return false; }
  std::vector<uint32_t> parent(P);
  for (size_t p = 0; p < P; ++p) parent[p] = (uint32_t)p;
  auto find = [&](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
  auto unite = [&](uint32_t a, uint32_t b) { a = find(a); b = find(b); if (a != b) { if (a < b) parent[b] = a; else parent[a] = b; } };
  for (int r = 0; r < world; ++r) {
    const int64_t np = I.p_off[r + 1] - I.p_off[r];
    for (int64_t i = I.l_off[r]; i < I.l_off[r + 1]; ++i) {
      const int32_t s = I.l_rank[i];
      if (I.l_own[i] < 0 || (int64_t)I.l_own[i] >= np || s < 0 || s >= world || I.l_part[i] < 0 || (int64_t)I.l_part[i] >= I.p_off[s + 1] - I.p_off[s])
        { why = "link " + std::to_string(i - I.l_off[r]) + " of rank " + std::to_string(r) + " names a part that does not exist"; return false; }
      const uint32_t a = (uint32_t)(I.p_off[r] + I.l_own[i]), b = (uint32_t)(I.p_off[s] + I.l_part[i]);
      if (I.p_label[a] != I.p_label[b]) { why = "link " + std::to_string(i - I.l_off[r]) + " of rank " + std::to_string(r) + " joins parts of different labels"; return false; }
      unite(a, b);
    }
  }
  // the shared voxels: equal (code, label) among the band records
  struct Key { uint64_t code; int32_t label; uint32_t part; };
  std::vector<Key> keys;
  keys.reserve((size_t)I.b_off[world]);
  for (int r = 0; r < world; ++r) {
    const int64_t np = I.p_off[r + 1] - I.p_off[r];
    for (int64_t i = I.b_off[r]; i < I.b_off[r + 1]; ++i) {
      if (I.b_part[i] < 0 || (int64_t)I.b_part[i] >= np) { why = "band record " + std::to_string(i - I.b_off[r]) + " of rank " + std::to_string(r) + " names a part that does not exist"; return false; }
      const uint32_t g = (uint32_t)(I.p_off[r] + I.b_part[i]);
      if (I.p_label[g] != I.b_label[i]) { why = "band record " + std::to_string(i - I.b_off[r]) + " of rank " + std::to_string(r) + " and its part carry different labels"; return false; }
      keys.push_back(Key{I.b_code[i], I.b_label[i], g});
    }
  }
  std::sort(keys.begin(), keys.end(), [](const Key& x, const Key& y) { return x.code != y.code ? x.code < y.code : x.label != y.label ? x.label < y.label : x.part < y.part; });
  std::vector<int64_t> surplus(P, 0);
  for (size_t i = 1; i < keys.size(); ++i)
    if (keys[i].code == keys[i - 1].code && keys[i].label == keys[i - 1].label) { unite(keys[i].part, keys[i - 1].part); ++surplus[keys[i].part]; }
  // the merged parts
  std::vector<int64_t> pts(P, 0), nds(P, 0);
  std::vector<uint64_t> code(P, 0);
  std::vector<uint32_t> roots;
  for (size_t p = 0; p < P; ++p) {
    const uint32_t r = find((uint32_t)p);
    if (r == (uint32_t)p) roots.push_back(r);
    pts[r] += I.p_points[p]; nds[r] += (int64_t)I.p_nodes[p] - surplus[p]; code[r] = std::max(code[r], I.p_code[p]);
  }
  std::sort(roots.begin(), roots.end(), [&](uint32_t a, uint32_t b) {
    return I.p_label[a] != I.p_label[b] ? I.p_label[a] < I.p_label[b] : code[a] != code[b] ? code[a] > code[b] : a < b; });
  const size_t C = roots.size();
  std::vector<int32_t> id_of(P, -1);
  O.label.resize(C); O.nodes.resize(C); O.points.resize(C); O.code.resize(C);
  for (size_t g = 0; g < C; ++g) {
    const uint32_t r = roots[g];
    id_of[r] = (int32_t)g; O.label[g] = I.p_label[r]; O.points[g] = pts[r]; O.nodes[g] = (int32_t)nds[r]; O.code[g] = code[r];
  }
  O.map.resize(P);
  for (size_t p = 0; p < P; ++p) O.map[p] = id_of[find((uint32_t)p)];
  O.first.assign((size_t)K + 1, 0); O.largest.assign((size_t)K, -1);
  for (size_t g = 0; g < C; ++g) ++O.first[(size_t)O.label[g] + 1];
  for (size_t k = 0; k < (size_t)K; ++k) O.first[k + 1] += O.first[k];   // the parts of label k: first[k] .. first[k + 1] - 1
  for (size_t g = 0; g < C; ++g) {
    int32_t& best = O.largest[(size_t)O.label[g]];
    if (best < 0 || O.points[g] > O.points[(size_t)best]) best = (int32_t)g;   // a strictly larger count only: the lowest id on a tie
  }
  return true;
}
}  // namespace

vgs_status vgs_tiles_fold_label_parts(int world, int64_t K, const int64_t* part_off, const int32_t* part_label, const int64_t* part_points,
                                      const int32_t* part_nodes, const uint64_t* part_first_code, const int64_t* band_off, const uint64_t* band_code,
                                      const int32_t* band_label, const int32_t* band_part, const int64_t* link_off, const int32_t* link_own,
                                      const int32_t* link_rank, const int32_t* link_part, int64_t* n_parts, int32_t* map, int32_t* out_label,
                                      int64_t* out_points, int32_t* out_nodes, uint64_t* out_first_code, int64_t* label_first, int32_t* label_largest) {
  if (world < 1 || K < 0 || K > (int64_t)0x7fffffff || !part_off || !band_off || !link_off) return VGS_E_ARG;
  if (part_off[world] > 0 && (!part_label || !part_points || !part_nodes || !part_first_code)) return VGS_E_ARG;
  if (band_off[world] > 0 && (!band_code || !band_label || !band_part)) return VGS_E_ARG;
  if (link_off[world] > 0 && (!link_own || !link_rank || !link_part)) return VGS_E_ARG;
  const PartsIn I{world, K, part_off, part_label, part_points, part_nodes, part_first_code, band_off, band_code, band_label, band_part, link_off, link_own, link_rank, link_part};
  PartsOut O;
  std::string why;
  if (!fold_label_parts(I, O, why)) return VGS_E_ARG;
  if (n_parts) *n_parts = (int64_t)O.label.size();
  put(O.map, map); put(O.label, out_label); put(O.points, out_points); put(O.nodes, out_nodes); put(O.code, out_first_code);
  put(O.first, label_first); put(O.largest, label_largest);
  return VGS_OK;
}

// The connected parts of a caller's point labelling over the ranks (include/vgs_tiles.h states the definition, the band argument and the
// shared-voxel rule).  TWO all_gather_varlen of 8-byte words per call, nothing cached:
//   own parts on this rank's GPU (vgs_own_point_label_parts) -> exchange 1: a header of four words (status, band count, K, own n_skipped)
//   and two words a band record (code; label << 32 | local part) -> cross links on this rank's GPU over the other ranks' records
//   (vgs_link_point_label_parts) -> exchange 2: a header of four words (status -- a failure of the link step travels here --, part count,
//   link count, K), three words a local part (label << 32 | nodes; points; first code), two words a link (own part << 32 | rank; part)
//   -> fold_label_parts, the same on every rank -> the part ids of the own points through this rank's map (vgs_apply_point_label_part_ids).
constexpr size_t CC_HEADER = 4;
static vgs_status tiles_label_components(vgs_tiles* t, const char* fn, bool on_device, const int32_t* labels, int64_t n, int64_t K, int64_t* n_parts,
                                         int64_t* n_skipped) {
  if (!t) return VGS_E_ARG;
  if (n_parts) *n_parts = 0;
  if (n_skipped) *n_skipped = 0;
  vgs_status carry;
  TRY(open_collective(t, fn, PH_COMPONENTS, carry));
  Comm& c = *t->comm;
  const size_t world = (size_t)c.world;
  t->cc_valid = false;
  double ms[VGS_TILES_CC_COUNT] = {0};
  Stopwatch sw(ms);
  // step 1: own parts and band records
  int64_t n_own_parts = 0, n_band = 0, n_skip = 0;
  TCARRY_AS(on_device ? vgs_own_point_label_parts_device : vgs_own_point_label_parts, on_device ? "vgs_own_point_label_parts_device" : "vgs_own_point_label_parts",
            t->ctx, labels, n, K, &n_own_parts, &n_band, &n_skip);
  if (carry != VGS_OK) { n_own_parts = 0; n_band = 0; n_skip = 0; }
  std::vector<int32_t> p_label((size_t)n_own_parts + 1), p_nodes((size_t)n_own_parts + 1), b_label((size_t)n_band + 1), b_part((size_t)n_band + 1);
  std::vector<int64_t> p_points((size_t)n_own_parts + 1);
  std::vector<uint64_t> p_code((size_t)n_own_parts + 1), b_code((size_t)n_band + 1);
  TCARRY(vgs_get_own_point_label_parts(t->ctx, p_label.data(), p_points.data(), p_nodes.data(), p_code.data(), b_code.data(), b_label.data(), b_part.data()));
  if (carry != VGS_OK) { n_own_parts = 0; n_band = 0; n_skip = 0; }
  std::vector<uint64_t> pay1(CC_HEADER + 2 * (size_t)n_band);
  pay1[0] = (uint64_t)(uint32_t)carry; pay1[1] = (uint64_t)n_band; pay1[2] = (uint64_t)K; pay1[3] = (uint64_t)n_skip;
  for (size_t i = 0; i < (size_t)n_band; ++i) {
    pay1[CC_HEADER + 2 * i] = b_code[i];
    pay1[CC_HEADER + 2 * i + 1] = ((uint64_t)(uint32_t)b_label[i] << 32) | (uint64_t)(uint32_t)b_part[i];
  }
  sw.lap(VGS_TILES_CC_OWN);
  std::vector<std::vector<uint64_t>> g1;
  TRY(exchange(t, carry, pay1, "components", sw, VGS_TILES_CC_EXCHANGE1, g1));
  // every rank was valid on its own: do they describe the same table, and is every payload as long as its header says?
  for (size_t r = 0; r < world; ++r)
    if (g1[r].size() < CC_HEADER || g1[r].size() != CC_HEADER + 2 * (size_t)g1[r][1]) return tfail(t, VGS_E_STATE, std::string(fn) + ": rank " + std::to_string(r) + " sent a payload of the wrong size");
  for (size_t r = 1; r < world; ++r)
    if (g1[r][2] != g1[0][2])
      return tfail(t, VGS_E_ARG, std::string(fn) + ": rank " + std::to_string(r) + " passed K = " + std::to_string((int64_t)g1[r][2]) + ", rank 0 passed " + std::to_string((int64_t)g1[0][2]));
  int64_t skipped = 0;
  for (size_t r = 0; r < world; ++r) skipped += (int64_t)g1[r][3];
  // step 3: the cross links over the other ranks' band records
  std::vector<uint64_t> f_code;
  std::vector<int32_t> f_label, f_rank, f_part;
  for (size_t r = 0; r < world; ++r) {
    if ((int)r == c.rank) continue;
    for (size_t i = 0; i < (size_t)g1[r][1]; ++i) {
      const uint64_t w = g1[r][CC_HEADER + 2 * i + 1];
      f_code.push_back(g1[r][CC_HEADER + 2 * i]); f_label.push_back((int32_t)(uint32_t)(w >> 32)); f_rank.push_back((int32_t)r); f_part.push_back((int32_t)(uint32_t)w);
    }
  }
  int64_t n_links = 0;
  TCARRY(vgs_link_point_label_parts(t->ctx, f_code.data(), f_label.data(), f_rank.data(), f_part.data(), (int64_t)f_code.size(), &n_links));
  if (carry != VGS_OK) n_links = 0;
  std::vector<int32_t> l_own((size_t)n_links + 1), l_rank((size_t)n_links + 1), l_part((size_t)n_links + 1);
  TCARRY(vgs_get_point_label_part_links(t->ctx, l_own.data(), l_rank.data(), l_part.data()));
  if (carry != VGS_OK) n_links = 0;
  const size_t np = carry == VGS_OK ? (size_t)n_own_parts : 0, nl = (size_t)n_links;
  std::vector<uint64_t> pay2(CC_HEADER + 3 * np + 2 * nl);
  pay2[0] = (uint64_t)(uint32_t)carry; pay2[1] = (uint64_t)np; pay2[2] = (uint64_t)nl; pay2[3] = (uint64_t)K;
  for (size_t i = 0; i < np; ++i) {
    uint64_t* w = pay2.data() + CC_HEADER + 3 * i;
    w[0] = ((uint64_t)(uint32_t)p_label[i] << 32) | (uint64_t)(uint32_t)p_nodes[i]; w[1] = (uint64_t)p_points[i]; w[2] = p_code[i];
  }
  for (size_t i = 0; i < nl; ++i) {
    uint64_t* w = pay2.data() + CC_HEADER + 3 * np + 2 * i;
    w[0] = ((uint64_t)(uint32_t)l_own[i] << 32) | (uint64_t)(uint32_t)l_rank[i]; w[1] = (uint64_t)(uint32_t)l_part[i];
  }
  sw.lap(VGS_TILES_CC_LINK);
  std::vector<std::vector<uint64_t>> g2;
  TRY(exchange(t, carry, pay2, "components", sw, VGS_TILES_CC_EXCHANGE2, g2));
  for (size_t r = 0; r < world; ++r)
    if (g2[r].size() < CC_HEADER || g2[r].size() != CC_HEADER + 3 * (size_t)g2[r][1] + 2 * (size_t)g2[r][2])
      return tfail(t, VGS_E_STATE, std::string(fn) + ": rank " + std::to_string(r) + " sent a payload of the wrong size");
  // step 5: the fold
  std::vector<int64_t> p_off(world + 1, 0), b_off(world + 1, 0), l_off(world + 1, 0);
  for (size_t r = 0; r < world; ++r) { p_off[r + 1] = p_off[r] + (int64_t)g2[r][1]; b_off[r + 1] = b_off[r] + (int64_t)g1[r][1]; l_off[r + 1] = l_off[r] + (int64_t)g2[r][2]; }
  std::vector<int32_t> ap_label((size_t)p_off[world]), ap_nodes((size_t)p_off[world]), ab_label((size_t)b_off[world]), ab_part((size_t)b_off[world]);
  std::vector<int32_t> al_own((size_t)l_off[world]), al_rank((size_t)l_off[world]), al_part((size_t)l_off[world]);
  std::vector<int64_t> ap_points((size_t)p_off[world]);
  std::vector<uint64_t> ap_code((size_t)p_off[world]), ab_code((size_t)b_off[world]);
  for (size_t r = 0; r < world; ++r) {
    const size_t rp = (size_t)g2[r][1];
    for (size_t i = 0; i < rp; ++i) {
      const uint64_t* w = g2[r].data() + CC_HEADER + 3 * i;
      const size_t o = (size_t)p_off[r] + i;
      ap_label[o] = (int32_t)(uint32_t)(w[0] >> 32); ap_nodes[o] = (int32_t)(uint32_t)w[0]; ap_points[o] = (int64_t)w[1]; ap_code[o] = w[2];
    }
    for (size_t i = 0; i < (size_t)g2[r][2]; ++i) {
      const uint64_t* w = g2[r].data() + CC_HEADER + 3 * rp + 2 * i;
      const size_t o = (size_t)l_off[r] + i;
      al_own[o] = (int32_t)(uint32_t)(w[0] >> 32); al_rank[o] = (int32_t)(uint32_t)w[0]; al_part[o] = (int32_t)(uint32_t)w[1];
    }
    for (size_t i = 0; i < (size_t)g1[r][1]; ++i) {
      const uint64_t w = g1[r][CC_HEADER + 2 * i + 1];
      const size_t o = (size_t)b_off[r] + i;
      ab_code[o] = g1[r][CC_HEADER + 2 * i]; ab_label[o] = (int32_t)(uint32_t)(w >> 32); ab_part[o] = (int32_t)(uint32_t)w;
    }
  }
  const PartsIn I{(int)world, K, p_off.data(), ap_label.data(), ap_points.data(), ap_nodes.data(), ap_code.data(), b_off.data(), ab_code.data(), ab_label.data(),
                  ab_part.data(), l_off.data(), al_own.data(), al_rank.data(), al_part.data()};
  PartsOut O;
  std::string bad;
  if (!fold_label_parts(I, O, bad)) return tfail(t, VGS_E_ARG, std::string(fn) + ": " + bad);
  sw.lap(VGS_TILES_CC_FOLD);
  // step 6: the part ids of the own points
  const int32_t none = 0;
  const int64_t mine = p_off[(size_t)c.rank + 1] - p_off[(size_t)c.rank];
  TRY(behind_collective(t, vgs_apply_point_label_part_ids(t->ctx, mine > 0 ? O.map.data() + p_off[(size_t)c.rank] : &none, mine), "vgs_apply_point_label_part_ids"));
  sw.lap(VGS_TILES_CC_APPLY);
  sw.total(VGS_TILES_CC_TOTAL, t->cctimes);
  t->cc_label.swap(O.label); t->cc_nodes.swap(O.nodes); t->cc_points.swap(O.points); t->cc_code.swap(O.code); t->cc_first.swap(O.first); t->cc_largest.swap(O.largest);
  t->cc_K = K; t->cc_valid = true;
  t->cc_band = n_band; t->cc_parts = (int64_t)np; t->cc_links = (int64_t)nl; t->cc_bytes = (int64_t)((pay1.size() + pay2.size()) * sizeof(uint64_t));
  if (n_parts) *n_parts = (int64_t)t->cc_label.size();
  if (n_skipped) *n_skipped = skipped;
  return VGS_OK;
}

vgs_status vgs_tiles_point_label_components(vgs_tiles* t, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_parts, int64_t* n_skipped) {
  return tiles_label_components(t, "vgs_tiles_point_label_components", false, labels_host, n, K, n_parts, n_skipped);
}
vgs_status vgs_tiles_point_label_components_device(vgs_tiles* t, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_parts, int64_t* n_skipped) {
  return tiles_label_components(t, "vgs_tiles_point_label_components_device", true, labels_dev, n, K, n_parts, n_skipped);
}

vgs_status vgs_tiles_get_point_label_components(vgs_tiles* t, int32_t* part_of_point, int32_t* part_label, int64_t* part_points, int32_t* part_nodes,
                                                uint64_t* part_first_code, int64_t* label_first, int32_t* label_largest) {
  if (!t) return VGS_E_ARG;
  if (!t->ran || !t->cc_valid)
    return tfail(t, VGS_E_STATE, "vgs_tiles_get_point_label_components: no label components since the last run or the last vgs_tiles_set_points (vgs_tiles_point_label_components first)");
  if (part_of_point && t->n_own > 0) TCTX(vgs_get_point_label_part_ids(t->ctx, part_of_point, t->n_own));
  put(t->cc_label, part_label); put(t->cc_points, part_points); put(t->cc_nodes, part_nodes); put(t->cc_code, part_first_code);
  put(t->cc_first, label_first); put(t->cc_largest, label_largest);
  return VGS_OK;
}

vgs_status vgs_tiles_get_point_label_component_times(vgs_tiles* t, double* ms, int32_t n) { return get_times(t, &vgs_tiles::cctimes, ms, n); }

vgs_status vgs_tiles_get_point_label_component_payload(vgs_tiles* t, int64_t* band_records, int64_t* parts, int64_t* links, int64_t* bytes_sent) {
  if (!t) return VGS_E_ARG;
  if (band_records) *band_records = t->cc_band;
  if (parts) *parts = t->cc_parts;
  if (links) *links = t->cc_links;
  if (bytes_sent) *bytes_sent = t->cc_bytes;
  return VGS_OK;
}

// The adjacency graph of a caller's point labelling over the ranks (include/vgs_tiles.h states the counting rule).  TWO all_gather_varlen
// per call, nothing cached:
//   own vertices and band records on this rank's GPU (vgs_own_point_label_band) -> exchange 1: BandRec, a header of two entries ([0]
//   code = status word, label = K; [1] code = band count, label | pad = own n_skipped), then (code, label) -> the merged vertices, the
//   tile walk and the pipeline on this rank's GPU over the other ranks' records (vgs_own_point_label_graph) -> exchange 2: LabelEdgeRec,
//   a header entry (a = status word -- a failure of the GPU step travels here --, n_pairs = record count), then the partial table ->
//   fold_label_edges, the same on every rank.
static vgs_status tiles_label_graph(vgs_tiles* t, const char* fn, bool on_device, const int32_t* labels, int64_t n, int64_t K, int64_t* n_edges,
                                    int64_t* n_skipped) {
  if (!t) return VGS_E_ARG;
  if (n_edges) *n_edges = 0;
  if (n_skipped) *n_skipped = 0;
  vgs_status carry;
  TRY(open_collective(t, fn, PH_LABEL_GRAPH, carry));
  Comm& c = *t->comm;
  const size_t world = (size_t)c.world;
  t->lg_valid = false;
  t->cc_valid = false;   // (the own pass overwrites the vertex arrays of the parts pass: its part ids in the context go with them)
  double ms[VGS_TILES_LG_COUNT] = {0};
  Stopwatch sw(ms);
  // step 1: own vertices and band records
  int64_t n_band = 0, n_skip = 0;
  TCARRY_AS(on_device ? vgs_own_point_label_band_device : vgs_own_point_label_band, on_device ? "vgs_own_point_label_band_device" : "vgs_own_point_label_band",
            t->ctx, labels, n, K, &n_band, &n_skip);
  if (carry != VGS_OK) { n_band = 0; n_skip = 0; }
  std::vector<uint64_t> b_code((size_t)n_band + 1);
  std::vector<int32_t> b_label((size_t)n_band + 1);
  TCARRY(vgs_get_own_point_label_band(t->ctx, b_code.data(), b_label.data()));
  if (carry != VGS_OK) { n_band = 0; n_skip = 0; }
  std::vector<BandRec> pay1(2 + (size_t)n_band);
  pay1[0].code = (uint64_t)(uint32_t)carry; pay1[0].label = (int32_t)K;   // (K outside int32 has failed above: nobody compares it)
  pay1[1].code = (uint64_t)n_band; pay1[1].label = (int32_t)(uint32_t)((uint64_t)n_skip & 0xffffffffull); pay1[1].pad = (int32_t)(uint32_t)((uint64_t)n_skip >> 32);
  for (size_t i = 0; i < (size_t)n_band; ++i) { pay1[2 + i].code = b_code[i]; pay1[2 + i].label = b_label[i]; }
  sw.lap(VGS_TILES_LG_OWN);
  std::vector<std::vector<BandRec>> g1;
  TRY(exchange(t, carry, pay1, "label_graph", sw, VGS_TILES_LG_EXCHANGE1, g1));
  for (size_t r = 0; r < world; ++r) if (g1[r].size() != 2 + (size_t)g1[r][1].code) return wrong_size(t, fn, r);
  for (size_t r = 1; r < world; ++r) if (g1[r][0].label != g1[0][0].label) return disagree(t, fn, r, "K", g1[r][0].label, g1[0][0].label);
  int64_t skipped = 0;
  for (size_t r = 0; r < world; ++r) skipped += (int64_t)(((uint64_t)(uint32_t)g1[r][1].pad << 32) | (uint64_t)(uint32_t)g1[r][1].label);
  // steps 3 and 4: the other ranks' records, the merged vertices, the walk, the partial table
  std::vector<uint64_t> f_code;
  std::vector<int32_t> f_label;
  for (size_t r = 0; r < world; ++r) {
    if ((int)r == c.rank) continue;
    for (size_t i = 2; i < g1[r].size(); ++i) { f_code.push_back(g1[r][i].code); f_label.push_back(g1[r][i].label); }
  }
  int64_t E = 0, hits = 0;
  TCARRY(vgs_own_point_label_graph(t->ctx, f_code.data(), f_label.data(), (int64_t)f_code.size(), &E));
  if (carry != VGS_OK) E = 0;
  const size_t e1 = (size_t)E;
  std::vector<int32_t> ab(2 * e1 + 2), nd(2 * e1 + 2);
  std::vector<int64_t> ns(e1 + 1), np(e1 + 1), nf(e1 + 1);
  std::vector<double> ws(e1 + 1);
  std::vector<float> mn(e1 + 1), mx(e1 + 1);
  TCARRY(vgs_get_own_point_label_graph(t->ctx, ab.data(), ns.data(), np.data(), nf.data(), nd.data(), ws.data(), mn.data(), mx.data()));
  TCARRY(vgs_get_own_point_label_graph_counts(t->ctx, nullptr, &hits, nullptr));
  std::vector<LabelEdgeRec> pay2(1);
  if (carry == VGS_OK) {
    pay2.reserve(1 + e1);
    for (size_t i = 0; i < e1; ++i) {
      LabelEdgeRec q;
      q.e = pack_edge(ab.data(), np.data(), nf.data(), nd.data(), ws.data(), mn.data(), mx.data(), i);
      q.n_shared = ns[i];
      pay2.push_back(q);
    }
  }
  set_header(pay2[0].e, carry, pay2.size() - 1);
  sw.lap(VGS_TILES_LG_TABLE);
  std::vector<std::vector<LabelEdgeRec>> g2;
  TRY(exchange(t, carry, pay2, "label_graph", sw, VGS_TILES_LG_EXCHANGE2, g2));
  for (size_t r = 0; r < world; ++r) if (g2[r][0].e.n_pairs < 0 || g2[r].size() != 1 + (size_t)g2[r][0].e.n_pairs) return wrong_size(t, fn, r);
  strip_headers(g2);
  // step 6: the fold
  if (!fold_label_edges(g2, std::max<int64_t>(K, 0), t->lgraph)) return tfail(t, VGS_E_ARG, std::string(fn) + ": a rank sent a table that is not sorted or names a label outside 0 .. K-1");
  sw.lap(VGS_TILES_LG_FOLD);
  sw.total(VGS_TILES_LG_TOTAL, t->lgtimes);
  t->lg_valid = true;
  t->lg_band = n_band; t->lg_hits = hits; t->lg_own = (int64_t)pay2.size() - 1;
  t->lg_bytes = (int64_t)(pay1.size() * sizeof(BandRec) + pay2.size() * sizeof(LabelEdgeRec));
  if (n_edges) *n_edges = (int64_t)t->lgraph.size();
  if (n_skipped) *n_skipped = skipped;
  return VGS_OK;
}

vgs_status vgs_tiles_point_label_graph(vgs_tiles* t, const int32_t* labels_host, int64_t n, int64_t K, int64_t* n_edges, int64_t* n_skipped) {
  return tiles_label_graph(t, "vgs_tiles_point_label_graph", false, labels_host, n, K, n_edges, n_skipped);
}
vgs_status vgs_tiles_point_label_graph_device(vgs_tiles* t, const int32_t* labels_dev, int64_t n, int64_t K, int64_t* n_edges, int64_t* n_skipped) {
  return tiles_label_graph(t, "vgs_tiles_point_label_graph_device", true, labels_dev, n, K, n_edges, n_skipped);
}

vgs_status vgs_tiles_get_point_label_graph(vgs_tiles* t, int32_t* seg_ab, int64_t* n_shared, int64_t* n_pairs, int64_t* n_finite, int32_t* nodes_ab,
                                           double* w_sum, float* w_min, float* w_max) {
  if (!t) return VGS_E_ARG;
  if (!t->ran || !t->lg_valid)
    return tfail(t, VGS_E_STATE, "vgs_tiles_get_point_label_graph: no label graph since the last run or the last vgs_tiles_set_points (vgs_tiles_point_label_graph first)");
  for (size_t i = 0; i < t->lgraph.size(); ++i) {
    unpack_edge(t->lgraph[i].e, i, seg_ab, n_pairs, n_finite, nodes_ab, w_sum, w_min, w_max);
    if (n_shared) n_shared[i] = t->lgraph[i].n_shared;
  }
  return VGS_OK;
}

vgs_status vgs_tiles_get_label_graph_times(vgs_tiles* t, double* ms, int32_t n) { return get_times(t, &vgs_tiles::lgtimes, ms, n); }

vgs_status vgs_tiles_get_label_graph_payload(vgs_tiles* t, int64_t* band_records, int64_t* foreign_hits, int64_t* own_edges, int64_t* bytes_sent) {
  if (!t) return VGS_E_ARG;
  if (band_records) *band_records = t->lg_band;
  if (foreign_hits) *foreign_hits = t->lg_hits;
  if (own_edges) *own_edges = t->lg_own;
  if (bytes_sent) *bytes_sent = t->lg_bytes;
  return VGS_OK;
}

// host arithmetic only (tests): the label-graph fold on flattened per-rank partial tables
vgs_status vgs_tiles_fold_label_edges(int world, int64_t K, const int64_t* rec_off, const int32_t* seg_ab, const int64_t* n_shared, const int64_t* n_pairs,
                                      const int64_t* n_finite, const int32_t* nodes_ab, const double* w_sum, const float* w_min, const float* w_max,
                                      int64_t* n_edges, int32_t* seg_ab_out, int64_t* n_shared_out, int64_t* n_pairs_out, int64_t* n_finite_out,
                                      int32_t* nodes_ab_out, double* w_sum_out, float* w_min_out, float* w_max_out) {
  if (world < 1 || !rec_off || K < 0 || K > (int64_t)0x7fffffffLL || !n_edges) return VGS_E_ARG;
  *n_edges = 0;
  if (rec_off[0] != 0) return VGS_E_ARG;
  for (int r = 0; r < world; ++r) if (rec_off[r + 1] < rec_off[r]) return VGS_E_ARG;
  if (rec_off[world] > 0 && (!seg_ab || !n_shared || !n_pairs || !n_finite || !nodes_ab || !w_sum || !w_min || !w_max)) return VGS_E_ARG;
  std::vector<std::vector<LabelEdgeRec>> ranks((size_t)world);
  for (int r = 0; r < world; ++r)
    for (int64_t i = rec_off[r]; i < rec_off[r + 1]; ++i) {
      LabelEdgeRec q;
      q.e = pack_edge(seg_ab, n_pairs, n_finite, nodes_ab, w_sum, w_min, w_max, (size_t)i);
      q.n_shared = n_shared[i];
      ranks[(size_t)r].push_back(q);
    }
  std::vector<LabelEdgeRec> out;
  if (!fold_label_edges(ranks, K, out)) return VGS_E_ARG;
  *n_edges = (int64_t)out.size();
  for (size_t i = 0; i < out.size(); ++i) {
    unpack_edge(out[i].e, i, seg_ab_out, n_pairs_out, n_finite_out, nodes_ab_out, w_sum_out, w_min_out, w_max_out);
    if (n_shared_out) n_shared_out[i] = out[i].n_shared;
  }
  return VGS_OK;
}

// host arithmetic only (tests): the attribute folds on flattened per-rank records
vgs_status vgs_tiles_fold_field_moments(int world, const int64_t* rec_off, const int32_t* label, int32_t n_channels, const int64_t* n_valid,
                                        const double* anchor, const double* s1, const double* s2, const float* vmin, const float* vmax, int64_t K,
                                        int64_t* n_valid_out, double* anchor_out, double* s1_out, double* s2_out, float* vmin_out, float* vmax_out) {
  if (world < 1 || !rec_off || K < 0 || n_channels < 1 || n_channels > 64) return VGS_E_ARG;
  if (K > 0 && (!n_valid_out || !anchor_out || !s1_out || !s2_out || !vmin_out || !vmax_out)) return VGS_E_ARG;
  if (rec_off[world] > 0 && (!label || !n_valid || !anchor || !s1 || !s2 || !vmin || !vmax)) return VGS_E_ARG;
  const size_t C = (size_t)n_channels;
  std::vector<FieldRecs> ranks((size_t)world);
  for (int r = 0; r < world; ++r) {
    if (rec_off[r + 1] < rec_off[r]) return VGS_E_ARG;
    std::vector<uint64_t> w;   // through the wire words, as in the collective
    for (int64_t i = rec_off[r]; i < rec_off[r + 1]; ++i) pack_field(w, label, n_valid, anchor, s1, s2, vmin, vmax, C, (size_t)i);
    unpack_fields(w.data(), (size_t)(rec_off[r + 1] - rec_off[r]), C, ranks[(size_t)r]);
  }
  std::vector<int64_t> n;
  std::vector<double> a, m1, m2;
  std::vector<float> mn, mx;
  if (!fold_field_moments(ranks, K, n_channels, n, a, m1, m2, mn, mx)) return VGS_E_ARG;
  std::copy(n.begin(), n.end(), n_valid_out); std::copy(a.begin(), a.end(), anchor_out); std::copy(m1.begin(), m1.end(), s1_out);
  std::copy(m2.begin(), m2.end(), s2_out); std::copy(mn.begin(), mn.end(), vmin_out); std::copy(mx.begin(), mx.end(), vmax_out);
  return VGS_OK;
}

vgs_status vgs_tiles_fold_class_counts(int world, const int64_t* rec_off, const int32_t* label, int32_t n_classes, const int64_t* hist,
                                       const int64_t* n_outside, int64_t K, int64_t* hist_out, int64_t* n_outside_out, int32_t* majority_out,
                                       int64_t* majority_count_out) {
  if (world < 1 || !rec_off || K < 0 || n_classes < 1 || n_classes > 1024) return VGS_E_ARG;
  if (K > 0 && (!hist_out || !n_outside_out || !majority_out || !majority_count_out)) return VGS_E_ARG;
  if (rec_off[world] > 0 && (!label || !hist || !n_outside)) return VGS_E_ARG;
  const size_t nc = (size_t)n_classes;
  std::vector<ClassRecs> ranks((size_t)world);
  for (int r = 0; r < world; ++r) {
    if (rec_off[r + 1] < rec_off[r]) return VGS_E_ARG;
    std::vector<int64_t> w;   // through the wire words, as in the collective
    for (int64_t i = rec_off[r]; i < rec_off[r + 1]; ++i) pack_class(w, label, hist, n_outside, nc, (size_t)i);
    unpack_classes(w.data(), (size_t)(rec_off[r + 1] - rec_off[r]), nc, ranks[(size_t)r]);
  }
  std::vector<int64_t> h, o, mc;
  std::vector<int32_t> m;
  if (!fold_class_counts(ranks, K, n_classes, h, o, m, mc)) return VGS_E_ARG;
  std::copy(h.begin(), h.end(), hist_out); std::copy(o.begin(), o.end(), n_outside_out);
  std::copy(m.begin(), m.end(), majority_out); std::copy(mc.begin(), mc.end(), majority_count_out);
  return VGS_OK;
}

// The segment graph over the ranks: the halo labels from the run's own boundary records -> this rank's partial table (one small pipeline
// on its GPU over the rows of its owned voxels) -> ONE all_gather_varlen of the edge records with a header of record count and status word
// -> the same host fold on every rank.
vgs_status vgs_tiles_get_segment_graph(vgs_tiles* t, int64_t* n_edges, int32_t* seg_ab, int64_t* n_pairs, int64_t* n_finite, int32_t* nodes_ab,
                                       double* w_sum, float* w_min, float* w_max) {
  if (!t || !n_edges) return VGS_E_ARG;
  *n_edges = 0;
  if (!t->graph_valid) {
    vgs_status carry;
    TRY(open_collective(t, "vgs_tiles_get_segment_graph", PH_GRAPH, carry));
    Comm& c = *t->comm;
    const int64_t Kg = t->kept;
    double ms[VGS_TILES_G_COUNT] = {0};
    Stopwatch sw(ms);
    // (code, global label) of every boundary record of the other ranks: a voxel this rank holds in its halo and counts pairs with has one
    std::vector<uint64_t> hcode;
    std::vector<int32_t> hlab;
    if (carry == VGS_OK && t->run_rec.size() == (size_t)c.world) {
      for (int r = 0; r < c.world; ++r) {
        if (r == c.rank) continue;
        const RankRecords& R = t->run_rec[(size_t)r];
        const std::vector<int32_t>& ur = t->run_uroot[(size_t)r];
        const std::vector<int32_t>& ul = t->run_ulabel[(size_t)r];
        for (size_t k = 0; k < R.code.size(); ++k) {
          const size_t j = (size_t)(std::lower_bound(ur.begin(), ur.end(), R.root[k]) - ur.begin());
          hcode.push_back(R.code[k]);
          hlab.push_back(ul[j]);
        }
      }
    }
    const uint64_t no_code = 0;
    const int32_t no_lab = 0;
    TCARRY(vgs_set_halo_labels(t->ctx, hcode.empty() ? &no_code : hcode.data(), hlab.empty() ? &no_lab : hlab.data(), (int64_t)hcode.size()));
    sw.lap(VGS_TILES_G_HALO);
    std::vector<EdgeRec> payload(1);
    if (carry == VGS_OK) {
      int64_t E = 0;
      TCARRY(vgs_get_own_segment_graph(t->ctx, Kg, &E, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
      if (carry == VGS_OK && E > 0) {
        const size_t e1 = (size_t)E;
        std::vector<int32_t> ab(2 * e1), nd(2 * e1);
        std::vector<int64_t> np(e1), nf(e1);
        std::vector<double> ws(e1);
        std::vector<float> mn(e1), mx(e1);
        TCARRY(vgs_get_own_segment_graph(t->ctx, Kg, &E, ab.data(), np.data(), nf.data(), nd.data(), ws.data(), mn.data(), mx.data()));
        if (carry == VGS_OK) payload.reserve(1 + e1);
        if (carry == VGS_OK) for (size_t i = 0; i < e1; ++i) payload.push_back(pack_edge(ab.data(), np.data(), nf.data(), nd.data(), ws.data(), mn.data(), mx.data(), i));
      }
    }
    set_header(payload[0], carry, payload.size() - 1);
    sw.lap(VGS_TILES_G_OWN);
    std::vector<std::vector<EdgeRec>> gathered;
    TRY(exchange(t, carry, payload, "graph", sw, VGS_TILES_G_EXCHANGE, gathered));
    strip_headers(gathered);
    if (!fold_edges(gathered, Kg, t->graph)) return tfail(t, VGS_E_STATE, "vgs_tiles_get_segment_graph: a rank sent a table that is not sorted or names a label >= kept_global");
    sw.lap(VGS_TILES_G_FOLD);
    sw.total(VGS_TILES_G_TOTAL, t->gtimes);
    t->g_halo = (int64_t)hcode.size(); t->g_own = (int64_t)payload.size() - 1; t->g_bytes = (int64_t)(payload.size() * sizeof(EdgeRec));
    t->graph_valid = true;
  }
  const size_t E = t->graph.size();
  *n_edges = (int64_t)E;
  for (size_t i = 0; i < E; ++i) unpack_edge(t->graph[i], i, seg_ab, n_pairs, n_finite, nodes_ab, w_sum, w_min, w_max);
  return VGS_OK;
}

vgs_status vgs_tiles_get_graph_times(vgs_tiles* t, double* ms, int32_t n) { return get_times(t, &vgs_tiles::gtimes, ms, n); }

vgs_status vgs_tiles_get_graph_payload(vgs_tiles* t, int64_t* halo_labels, int64_t* own_edges, int64_t* bytes_sent) {
  if (!t) return VGS_E_ARG;
  if (halo_labels) *halo_labels = t->g_halo;
  if (own_edges) *own_edges = t->g_own;
  if (bytes_sent) *bytes_sent = t->g_bytes;
  return VGS_OK;
}

// host arithmetic only (tests): the edge fold on flattened per-rank tables
vgs_status vgs_tiles_fold_edges(int world, const int64_t* rec_off, const int32_t* seg_ab, const int64_t* n_pairs, const int64_t* n_finite,
                                const int32_t* nodes_ab, const double* w_sum, const float* w_min, const float* w_max, int64_t K,
                                int64_t* n_edges, int32_t* seg_ab_out, int64_t* n_pairs_out, int64_t* n_finite_out, int32_t* nodes_ab_out,
                                double* w_sum_out, float* w_min_out, float* w_max_out) {
  if (world < 1 || !rec_off || K < 0 || K >= (int64_t)0x7fffffffLL || !n_edges) return VGS_E_ARG;
  *n_edges = 0;
  if (rec_off[0] != 0) return VGS_E_ARG;
  for (int r = 0; r < world; ++r) if (rec_off[r + 1] < rec_off[r]) return VGS_E_ARG;
  if (rec_off[world] > 0 && (!seg_ab || !n_pairs || !n_finite || !nodes_ab || !w_sum || !w_min || !w_max)) return VGS_E_ARG;
  std::vector<std::vector<EdgeRec>> ranks((size_t)world);
  for (int r = 0; r < world; ++r)
    for (int64_t i = rec_off[r]; i < rec_off[r + 1]; ++i) ranks[(size_t)r].push_back(pack_edge(seg_ab, n_pairs, n_finite, nodes_ab, w_sum, w_min, w_max, (size_t)i));
  std::vector<EdgeRec> out;
  if (!fold_edges(ranks, K, out)) return VGS_E_ARG;
  *n_edges = (int64_t)out.size();
  for (size_t i = 0; i < out.size(); ++i) unpack_edge(out[i], i, seg_ab_out, n_pairs_out, n_finite_out, nodes_ab_out, w_sum_out, w_min_out, w_max_out);
  return VGS_OK;
}

// host arithmetic only (tests): the descriptor fold on flattened per-rank records
vgs_status vgs_tiles_fold_moments(int world, const int64_t* rec_off, const int32_t* label, const int64_t* n_points, const int32_t* n_nodes,
                                  const float* bbox6, const float* anchor3, const double* s9, int64_t K, int64_t* n_points_out,
                                  int32_t* n_nodes_out, float* bbox6_out, float* anchor3_out, double* s9_out) {
  if (world < 1 || !rec_off || K < 0 || !n_points_out || !n_nodes_out || !bbox6_out || !anchor3_out || !s9_out) return VGS_E_ARG;
  if (rec_off[world] > 0 && (!label || !n_points || !n_nodes || !bbox6 || !anchor3 || !s9)) return VGS_E_ARG;
  std::vector<std::vector<MomentRec>> ranks((size_t)world);
  for (int r = 0; r < world; ++r) {
    if (rec_off[r + 1] < rec_off[r]) return VGS_E_ARG;
    for (int64_t i = rec_off[r]; i < rec_off[r + 1]; ++i) ranks[(size_t)r].push_back(pack_moment(label, n_points, n_nodes, bbox6, anchor3, s9, (size_t)i));
  }
  std::vector<int64_t> np;
  std::vector<int32_t> nn;
  std::vector<float> bb, an;
  std::vector<double> sm;
  if (!fold_moments(ranks, K, np, nn, bb, an, sm)) return VGS_E_ARG;
  std::copy(np.begin(), np.end(), n_points_out); std::copy(nn.begin(), nn.end(), n_nodes_out);
  std::copy(bb.begin(), bb.end(), bbox6_out); std::copy(an.begin(), an.end(), anchor3_out); std::copy(sm.begin(), sm.end(), s9_out);
  return VGS_OK;
}

vgs_status vgs_tiles_get_point_labels(vgs_tiles* t, int32_t* labels, int64_t* kept_global) {
  if (!t || (!labels && t->n_own > 0)) return VGS_E_ARG;
  std::vector<int32_t> all(t->local.size() / 3 + 1);
  TCTX(vgs_get_point_labels(t->ctx, all.data()));
  std::copy(all.begin() + (ptrdiff_t)t->own_first, all.begin() + (ptrdiff_t)(t->own_first + t->n_own), labels);   // halo points belong to other ranks
  if (kept_global) *kept_global = t->kept;
  return VGS_OK;
}

// host arithmetic only (tests): the boundary merge on flattened per-rank records
vgs_status vgs_tiles_merge_boundary(int world, const int64_t* rec_off, const uint64_t* code, const int32_t* root, const int32_t* cnt,
                                    const int64_t* kept_local, int voxels_min, int64_t* base, int64_t* uoff, int32_t* uroot, int32_t* ulabel,
                                    int64_t* kept_total) {
  if (world < 1 || !rec_off || !kept_local || !base || !uoff || !kept_total) return VGS_E_ARG;
  std::vector<RankRecords> rec((size_t)world);
  std::vector<int64_t> kl(kept_local, kept_local + world);
  for (int r = 0; r < world; ++r) {
    rec[(size_t)r].code.assign(code + rec_off[r], code + rec_off[r + 1]);
    rec[(size_t)r].root.assign(root + rec_off[r], root + rec_off[r + 1]);
    rec[(size_t)r].cnt.assign(cnt + rec_off[r], cnt + rec_off[r + 1]);
  }
  std::vector<int64_t> b;
  std::vector<std::vector<int32_t>> ur, ul;
  merge_boundary_compact(rec, kl, voxels_min, b, ur, ul, *kept_total);
  uoff[0] = 0;
  for (int r = 0; r < world; ++r) {
    base[r] = b[(size_t)r];
    uoff[r + 1] = uoff[r] + (int64_t)ur[(size_t)r].size();
    if (uroot) std::copy(ur[(size_t)r].begin(), ur[(size_t)r].end(), uroot + uoff[r]);
    if (ulabel) std::copy(ul[(size_t)r].begin(), ul[(size_t)r].end(), ulabel + uoff[r]);
  }
  return VGS_OK;
}

vgs_status vgs_tiles_get_exchange(vgs_tiles* t, int64_t* bytes_sent, int64_t* bytes_received, int32_t* collectives) {
  if (!t) return VGS_E_ARG;
  if (bytes_sent) *bytes_sent = t->exch_sent;
  if (bytes_received) *bytes_received = t->exch_recv;
  if (collectives) *collectives = t->exch_calls;
  return VGS_OK;
}

vgs_status vgs_tiles_get_info(vgs_tiles* t, int64_t* n_outside, int64_t* n_local, int64_t* n_boundary_records) {
  if (!t) return VGS_E_ARG;
  if (n_outside) *n_outside = t->n_outside;
  if (n_local) *n_local = (int64_t)(t->local.size() / 3);
  if (n_boundary_records) *n_boundary_records = t->n_records;
  return VGS_OK;
}

}  // extern "C"
