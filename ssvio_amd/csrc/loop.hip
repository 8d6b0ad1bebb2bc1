// ssvio_amd/csrc/loop.hip -- the keyframe database of loop closing, resident on the device.
//
// LoopClosing keeps every keyframe it has seen in key_frame_database_ (a std::map by keyframe id,
// src/ssvio/loopclosing.cpp:646-649), scans it for the best bag-of-words score on every new keyframe
// (DetectLoop, :72-103) and brute-force matches the winner's descriptors against the current ones (MatchFeatures,
// :105-145).  Here the database lives in HBM:
//
//   arena   one blob per keyframe, 32-byte aligned:  ids int32[n_bow] | values double[n_bow] | class_id int32[n_desc] |
//           descriptors uint8[n_desc][32]
//   table   KfRow[n]: where a keyframe's blob starts and its two counts
//
// Both grow geometrically with a device-to-device copy.  ssx_kfdb_add stages the blob and its row once and copies
// them up; it launches nothing.
//
// k_kfdb_score   one wavefront per stored keyframe.  The query's (id, value) pairs are in LDS when they fit (4096
//                words), else they are read from global memory.  A lane takes the row's entries lane + 64 k (four
//                chunks in flight), finds the word in the query by binary search and forms |q - e| - |q| - |e|.  L1Scoring::score
//                (ScoringObject.cpp:23-68) adds these terms in ascending word order, and a double sum depends on its
//                order, so the hits of a chunk are taken lane by lane (ballot, lowest set bit first) into ONE chain;
//                a miss adds nothing.  The chain is as long as the common words (tens to hundreds), not the row.
//                The winner of DetectLoop is the arg-max of the scores narrowed to float with the lowest index on a
//                tie: floats > 0 order like their bit patterns, so it is one 64-bit atomicMax of
//                (float bits << 32) | ~index per workgroup.
// k_kfdb_pairs   one workgroup after k_bf_match: minimum distance, the screen dist <= max(2 min, 30), the kept pairs
//                (current class_id, loop class_id) packed into order-preserving 64-bit keys, a bitonic sort (in LDS up
//                to 4096 keys, else in a global scratch), and the unique keys written in order = the std::set.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "orb_ws.hpp"

namespace {

struct KfRow {
  int64_t off;      // byte offset of the blob in the arena
  int32_t n_bow;    // BowVector entries
  int32_t n_desc;   // descriptors; -1: the keyframe was added without any
};

constexpr int kQueryLds = 4096;     // query words staged in LDS (12 bytes each)
constexpr int kSortLds = 4096;      // keys sorted in LDS (8 bytes each)
constexpr int kPairsThreads = 1024;
constexpr int kChunks = 4;          // 64-entry chunks of a row a wavefront has in flight

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
__host__ __device__ inline size_t blob_vals(int n_bow) { return ((size_t)n_bow * 4 + 7) & ~size_t(7); }
__host__ __device__ inline size_t blob_class(int n_bow) { return blob_vals(n_bow) + (size_t)n_bow * 8; }
__host__ __device__ inline size_t blob_desc(int n_bow, int n_desc) { return (blob_class(n_bow) + (size_t)n_desc * 4 + 31) & ~size_t(31); }
__host__ __device__ inline size_t blob_bytes(int n_bow, int n_desc) { return (blob_desc(n_bow, n_desc) + (size_t)n_desc * 32 + 31) & ~size_t(31); }

__device__ __forceinline__ double readlane_f64(double v, int l)
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// scores[row] = L1Scoring::score(query, row) for the first n_rows keyframes; *best = max over rows of (float bits << 32) | ~row
template <bool LDS>
__global__ __launch_bounds__(256) void k_kfdb_score(const char* arena, const KfRow* rows, int n_rows, const int32_t* q_ids, const double* q_vals, int nq,
                                                    double* scores, unsigned long long* best)
{
  extern __shared__ double smem[];                            // [nq] values, then [nq] ids
  const int32_t* qi = q_ids;
  const double* qv = q_vals;
  if (LDS) {
    int32_t* si = reinterpret_cast<int32_t*>(smem + nq);
    for (int k = threadIdx.x; k < nq; k += blockDim.x) { smem[k] = q_vals[k]; si[k] = q_ids[k]; }
    __syncthreads();
    qi = si; qv = smem;
  }
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int top = nq > 0 ? 1 << (31 - __clz(nq)) : 0;          // the largest power of two <= nq
  unsigned long long best_key = 0;
  for (int row = blockIdx.x * 4 + wave; row < n_rows; row += gridDim.x * 4) {
    const KfRow r = rows[row];
    const int32_t* ids = reinterpret_cast<const int32_t*>(arena + r.off);
    const double* vals = reinterpret_cast<const double*>(arena + r.off + blob_vals(r.n_bow));
    double s = 0.0;                                           // the same value in every lane
    for (int base = 0; base < r.n_bow; base += 64 * kChunks) {
      // kChunks chunks of 64 entries at once: their loads and their searches are independent, only the additions are ordered
      int32_t x[kChunks];
      double e[kChunks];
      int lo[kChunks];
      bool act[kChunks];
#pragma unroll
      for (int u = 0; u < kChunks; ++u) {
        const int k = base + 64 * u + lane;
        act[u] = k < r.n_bow;
        x[u] = act[u] ? ids[k] : 0;
        e[u] = act[u] ? vals[k] : 0.0;
        lo[u] = 0;
      }
      for (int step = top; step > 0; step >>= 1) {            // lo = number of query ids below x, one bit per step
#pragma unroll
        for (int u = 0; u < kChunks; ++u) {
          const int m = lo[u] + step;
          if (m <= nq && qi[m - 1] < x[u]) lo[u] = m;
        }
      }
#pragma unroll
      for (int u = 0; u < kChunks; ++u) {
        const bool hit = act[u] && lo[u] < nq && qi[lo[u]] == x[u];
        double term = 0.0;
        if (hit) {
          const double q = qv[lo[u]];
          term = fabs(q - e[u]) - fabs(q) - fabs(e[u]);
        }
        unsigned long long m = __ballot(hit);
        while (m) {                                           // ascending lane = ascending word id: the reference's order of additions
          const int l = __ffsll((long long)m) - 1;
          m &= m - 1;
          s += readlane_f64(term, l);
        }
      }
    }
    const double score = (nq > 0 && r.n_bow > 0) ? -s / 2.0 : 0.0;   // an empty vector on either side is skipped (loopclosing.cpp:81)
    const float f = (float)score;
    if (lane == 0) scores[row] = score;
    if (f > 0.f) best_key = max(best_key, ((unsigned long long)__float_as_uint(f) << 32) | (unsigned)~row);
  }
  // one atomic per workgroup, and none when the word already holds a larger key (it only ever grows): thousands of wavefronts
  // hitting one address otherwise queue up behind each other
  __shared__ unsigned long long s_best[4];
  if (lane == 0) s_best[wave] = best_key;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long k = max(max(s_best[0], s_best[1]), max(s_best[2], s_best[3]));
    if (k > *reinterpret_cast<volatile unsigned long long*>(best)) atomicMax(best, k);
  }
}

__device__ __forceinline__ unsigned long long pair_key(int cur, int loop)
{
  return ((unsigned long long)((unsigned)cur ^ 0x80000000u) << 32) | ((unsigned)loop ^ 0x80000000u);   // unsigned order == (int, int) order
}

// block-wide exclusive sum of one int per thread (1024 threads); every thread also gets the total
__device__ __forceinline__ int block_scan_excl(int v, int* wave_sums, int* total)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  __syncthreads();                                            // wave_sums may still be read from a previous call
  if (lane == 63) wave_sums[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < kPairsThreads / 64; ++w) {
    const int t = wave_sums[w];
    before += w < wave ? t : 0;
    all += t;
  }
  *total = all;
  return before + inc - v;
}

// The kept pairs as keys into `keys`, sorted, the first of every run written out.  Called once with the LDS array and once with the
// global scratch, so that after inlining each copy addresses one known memory (no flat pointer to LDS).
__device__ __forceinline__ void sort_unique_pairs(unsigned long long* keys, int n_valid, int npad, int thr, const int* idx, const int* dist, int n_loop,
                                                  const int32_t* loop_class, const int32_t* cur_class, int* s_fill, int* wave_sums, int32_t* hdr,
                                                  int32_t* pairs, int min_d)
{
  const int tid = threadIdx.x;
  for (int i = tid; i < n_loop; i += kPairsThreads)
    if (dist[i] <= thr) keys[atomicAdd(s_fill, 1)] = pair_key(cur_class[idx[i]], loop_class[i]);   // any order: sorted next
  for (int i = n_valid + tid; i < npad; i += kPairsThreads) keys[i] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1) {                       // bitonic sort of npad = 2^m keys
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (npad >> 1); t += kPairsThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const unsigned long long a = keys[i], b = keys[i | j];
        if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[i | j] = a; }
      }
      __syncthreads();
    }
  }
  // the first n_valid keys are the kept pairs in order (padding sorts last); a thread takes a contiguous piece and keeps the first of every run
  const int seg = (n_valid + kPairsThreads - 1) / kPairsThreads;
  const int i0 = min(tid * seg, n_valid), i1 = min(i0 + seg, n_valid);
  const unsigned long long before = i0 > 0 ? keys[i0 - 1] : 0;
  unsigned long long prev = before;
  int uniq = 0;
  for (int i = i0; i < i1; ++i) {
    const unsigned long long key = keys[i];
    uniq += (i == 0 || key != prev) ? 1 : 0;
    prev = key;
  }
  int n_pairs = 0;
  int pos = block_scan_excl(uniq, wave_sums, &n_pairs);
  prev = before;
  for (int i = i0; i < i1; ++i) {
    const unsigned long long key = keys[i];
    if (i == 0 || key != prev) {
      pairs[2 * pos] = (int32_t)((unsigned)(key >> 32) ^ 0x80000000u);
      pairs[2 * pos + 1] = (int32_t)((unsigned)key ^ 0x80000000u);
      ++pos;
    }
    prev = key;
  }
  if (tid == 0) { hdr[0] = n_pairs; hdr[1] = min_d; }
}

// hdr[0] = number of unique pairs, hdr[1] = minimum distance; pairs[2 k], pairs[2 k + 1] = (current class_id, loop class_id) ascending
__global__ __launch_bounds__(kPairsThreads) void k_kfdb_pairs(const int* idx, const int* dist, int n_loop, const int32_t* loop_class, const int32_t* cur_class,
                                                              unsigned long long* gkeys, int32_t* hdr, int32_t* pairs)
{
  __shared__ unsigned long long skeys[kSortLds];
  __shared__ int wave_sums[kPairsThreads / 64];
  __shared__ int s_min, s_fill;
  const int tid = threadIdx.x;
  if (tid == 0) { s_min = 0x7fffffff; s_fill = 0; }
  __syncthreads();
  int mn = 0x7fffffff;
  for (int i = tid; i < n_loop; i += kPairsThreads) mn = min(mn, dist[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = min(mn, __shfl_xor(mn, o));
  if ((tid & 63) == 0) atomicMin(&s_min, mn);
  __syncthreads();
  const int min_d = s_min;
  const int thr = max(2 * min_d, 30);                         // dist <= max(2 * min_distance, 30.0), loopclosing.cpp:120
  int mine = 0;
  for (int i = tid; i < n_loop; i += kPairsThreads) mine += dist[i] <= thr ? 1 : 0;
  int n_valid = 0;
  block_scan_excl(mine, wave_sums, &n_valid);
  int npad = 1;
  while (npad < n_valid) npad <<= 1;
  if (npad <= kSortLds)
    sort_unique_pairs(skeys, n_valid, npad, thr, idx, dist, n_loop, loop_class, cur_class, &s_fill, wave_sums, hdr, pairs, min_d);
  else                                                        // gkeys holds the next power of two of n_loop keys
    sort_unique_pairs(gkeys, n_valid, npad, thr, idx, dist, n_loop, loop_class, cur_class, &s_fill, wave_sums, hdr, pairs, min_d);
}

}  // namespace

struct ssx_kf_database {
  ssx_ctx* ctx = nullptr;
  std::vector<int64_t> ids;       // keyframe ids, ascending
  std::vector<KfRow> rows;        // host mirror of the table
  DevBuf arena, table, io;
  HostBuf stage;
  size_t used = 0;                // bytes of the arena in use
  int64_t n_bow = 0, n_desc = 0;
};

namespace {

// DevBuf::reserve drops the contents: grow to at least `need` bytes keeping the first `keep`
hipError_t grow_keep(ssx_ctx* ctx, DevBuf& b, size_t keep, size_t need)
{
  if (need <= b.cap) return hipSuccess;
  size_t want = std::max<size_t>(b.cap, 4096);
  while (want < need) want *= 2;
  void* np = nullptr;
  hipError_t e = hipMalloc(&np, want);
  if (e != hipSuccess) return e;
  if (keep) e = hipMemcpyAsync(np, b.p, keep, hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { (void)hipFree(np); return e; }
  if (b.p) (void)hipFree(b.p);
  b.p = np; b.cap = want;
  return hipSuccess;
}

}  // namespace

extern "C" {

ssx_status ssx_kfdb_create(ssx_ctx* ctx, int32_t keyframes_hint, ssx_kf_database** out)
{
  if (!ctx || !out || keyframes_hint < 0) return SSX_ERR_INVALID_ARG;
  *out = nullptr;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  ssx_kf_database* db = new ssx_kf_database();
  db->ctx = ctx;
  const size_t hint = (size_t)std::max(keyframes_hint, 1);
  // a keyframe of the reference has about 1000 words and 1000 pyramid descriptors: 48 KB
  hipError_t e = grow_keep(ctx, db->table, 0, hint * sizeof(KfRow));
  if (e == hipSuccess) e = grow_keep(ctx, db->arena, 0, hint * 49152);
  if (e != hipSuccess) {
    db->table.release(); db->arena.release();
    delete db;
    ctx->set_error("ssx_kfdb_create: device allocation failed: %s", hipGetErrorString(e));
    return SSX_ERR_HIP;
  }
  db->ids.reserve(hint); db->rows.reserve(hint);
  *out = db;
  return SSX_OK;
}

void ssx_kfdb_destroy(ssx_kf_database* db)
{
  if (!db) return;
  db->arena.release(); db->table.release(); db->io.release(); db->stage.release();
  delete db;
}

ssx_status ssx_kfdb_size(const ssx_kf_database* db, int32_t* n_keyframes, int64_t* n_bow_entries, int64_t* n_descriptors)
{
  if (!db) return SSX_ERR_INVALID_ARG;
  if (n_keyframes) *n_keyframes = (int32_t)db->ids.size();
  if (n_bow_entries) *n_bow_entries = db->n_bow;
  if (n_descriptors) *n_descriptors = db->n_desc;
  return SSX_OK;
}

ssx_status ssx_kfdb_add(ssx_kf_database* db, int64_t kf_id, int32_t n_bow, const int32_t* ids, const double* vals, int32_t n_desc,
                        const uint8_t* desc, const int32_t* class_id)
{
  if (!db || n_bow < 0 || n_desc < 0 || (n_bow > 0 && (!ids || !vals)) || (n_desc > 0 && (!desc || !class_id))) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = db->ctx;
  if (!db->ids.empty() && kf_id <= db->ids.back()) {
    ctx->set_error("ssx_kfdb_add: keyframe id %lld after %lld (ids must ascend)", (long long)kf_id, (long long)db->ids.back());
    return SSX_ERR_INVALID_ARG;
  }
  for (int32_t i = 1; i < n_bow; ++i)
    if (ids[i] <= ids[i - 1]) { ctx->set_error("ssx_kfdb_add: word ids must ascend (entry %d)", i); return SSX_ERR_INVALID_ARG; }
  if (db->ids.size() >= (size_t)0x7fffffff) { ctx->set_error("ssx_kfdb_add: the database is full"); return SSX_ERR_CAPACITY; }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool with_desc = desc != nullptr;
  const size_t bytes = blob_bytes(n_bow, n_desc), n = db->ids.size();
  SSX_HIP_TRY(ctx, grow_keep(ctx, db->arena, db->used, db->used + bytes));
  SSX_HIP_TRY(ctx, grow_keep(ctx, db->table, n * sizeof(KfRow), (n + 1) * sizeof(KfRow)));
  SSX_HIP_TRY(ctx, db->stage.reserve(bytes + sizeof(KfRow)));
  char* hs = db->stage.as<char>();
  memset(hs, 0, bytes);
  if (n_bow) { memcpy(hs, ids, (size_t)n_bow * 4); memcpy(hs + blob_vals(n_bow), vals, (size_t)n_bow * 8); }
  if (n_desc) { memcpy(hs + blob_class(n_bow), class_id, (size_t)n_desc * 4); memcpy(hs + blob_desc(n_bow, n_desc), desc, (size_t)n_desc * 32); }
  const KfRow row{(int64_t)db->used, n_bow, with_desc ? n_desc : -1};
  memcpy(hs + bytes, &row, sizeof(KfRow));
  if (bytes) SSX_HIP_TRY(ctx, hipMemcpyAsync(db->arena.as<char>() + db->used, hs, bytes, hipMemcpyHostToDevice, ctx->stream));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(db->table.as<KfRow>() + n, hs + bytes, sizeof(KfRow), hipMemcpyHostToDevice, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));       // the staging buffer is free again, and a failed copy is reported here
  db->ids.push_back(kf_id); db->rows.push_back(row);
  db->used += bytes; db->n_bow += n_bow; db->n_desc += n_desc;
  return SSX_OK;
}

ssx_status ssx_kfdb_detect_loop(ssx_kf_database* db, int64_t query_kf_id, int32_t n_bow, const int32_t* ids, const double* vals, int32_t min_id_gap,
                                float threshold, int32_t* found, int64_t* best_kf_id, float* best_score, int32_t scores_cap, double* scores_out,
                                int32_t* n_scored)
{
  if (!db || n_bow < 0 || (n_bow > 0 && (!ids || !vals)) || !found || scores_cap < 0) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = db->ctx;
  *found = 0;
  // the map is walked in id order and left at the first keyframe that is too recent (loopclosing.cpp:79): a prefix
  const int n_elig = (int)(std::upper_bound(db->ids.begin(), db->ids.end(), query_kf_id - (int64_t)min_id_gap) - db->ids.begin());
  if (n_scored) *n_scored = n_elig;
  if (scores_out && scores_cap < n_elig) {
    ctx->set_error("ssx_kfdb_detect_loop: %d scores but capacity %d", n_elig, scores_cap);
    return SSX_ERR_CAPACITY;
  }
  if (n_elig == 0 || n_bow == 0) {                            // nothing to score, or every entry skipped
    if (scores_out) std::fill(scores_out, scores_out + n_elig, 0.0);
    return SSX_OK;
  }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  Layout lay;
  const size_t o_v = lay.take((size_t)n_bow * 8), o_i = lay.take((size_t)n_bow * 4), o_best = lay.take(8);
  const size_t in_bytes = lay.off;
  const size_t o_s = lay.take((size_t)n_elig * 8);
  SSX_HIP_TRY(ctx, db->io.reserve(lay.off));
  SSX_HIP_TRY(ctx, db->stage.reserve(lay.off));
  char* hs = db->stage.as<char>();
  char* base = db->io.as<char>();
  memcpy(hs + o_v, vals, (size_t)n_bow * 8);
  memcpy(hs + o_i, ids, (size_t)n_bow * 4);
  memset(hs + o_best, 0, 8);
  SSX_HIP_TRY(ctx, hipMemcpyAsync(base, hs, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  const int blocks = std::min((n_elig + 3) / 4, 1024);   // four workgroups per CU; a wavefront takes every 4096th row
  const char* arena = db->arena.as<char>();
  const KfRow* rows = db->table.as<KfRow>();
  const int32_t* q_ids = (const int32_t*)(base + o_i);
  const double* q_vals = (const double*)(base + o_v);
  double* scores = (double*)(base + o_s);
  unsigned long long* best = (unsigned long long*)(base + o_best);
  if (n_bow <= kQueryLds)
    SSX_PROF(ctx, KID_LOOP_SCORE, hipLaunchKernelGGL(k_kfdb_score<true>, dim3(blocks), dim3(256), (size_t)n_bow * 12, ctx->stream, arena, rows, n_elig,
                                                     q_ids, q_vals, n_bow, scores, best));
  else
    SSX_PROF(ctx, KID_LOOP_SCORE, hipLaunchKernelGGL(k_kfdb_score<false>, dim3(blocks), dim3(256), 0, ctx->stream, arena, rows, n_elig, q_ids, q_vals,
                                                     n_bow, scores, best));
  SSX_HIP_TRY(ctx, hipGetLastError());
  // the winner's key and, when asked for, the scores right behind it: one copy, one synchronisation
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + o_best, base + o_best, scores_out ? lay.off - o_best : 8, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (scores_out) memcpy(scores_out, hs + o_s, (size_t)n_elig * 8);
  unsigned long long key = 0;
  memcpy(&key, hs + o_best, 8);
  if (key == 0) return SSX_OK;                                // no score above 0: max_score stays 0 (loopclosing.cpp:74,85)
  const uint32_t bits = (uint32_t)(key >> 32), row = ~(uint32_t)key;
  float f = 0.f;
  memcpy(&f, &bits, 4);
  if (f < threshold) return SSX_OK;                           // loopclosing.cpp:93
  *found = 1;
  if (best_kf_id) *best_kf_id = db->ids[row];
  if (best_score) *best_score = f;
  return SSX_OK;
}

ssx_status ssx_kfdb_match_features(ssx_kf_database* db, int64_t loop_kf_id, int32_t n_cur, const uint8_t* cur_desc, const int32_t* cur_class_id,
                                   int32_t cap, int32_t* pairs_out, int32_t* n_pairs, int32_t* min_distance)
{
  if (!db || n_cur < 0 || (n_cur > 0 && (!cur_desc || !cur_class_id)) || cap < 0 || (cap > 0 && !pairs_out) || !n_pairs) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = db->ctx;
  *n_pairs = 0;
  if (min_distance) *min_distance = -1;
  const auto it = std::lower_bound(db->ids.begin(), db->ids.end(), loop_kf_id);
  if (it == db->ids.end() || *it != loop_kf_id) { ctx->set_error("ssx_kfdb_match_features: keyframe %lld is not in the database", (long long)loop_kf_id); return SSX_ERR_INVALID_ARG; }
  const KfRow row = db->rows[it - db->ids.begin()];
  if (row.n_desc < 0) { ctx->set_error("ssx_kfdb_match_features: keyframe %lld was added without descriptors", (long long)loop_kf_id); return SSX_ERR_INVALID_ARG; }
  if (n_cur > 65535) { ctx->set_error("ssx_kfdb_match_features: more than 65535 current descriptors"); return SSX_ERR_UNSUPPORTED; }
  const int nl = row.n_desc;
  if (nl == 0 || n_cur == 0) return SSX_OK;                   // no match exists: no pairs (the reference dereferences end() here)
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  size_t npad = 1;
  while (npad < (size_t)nl) npad *= 2;
  const int n_down = std::min(nl, cap);
  Layout lay;
  const size_t o_d = lay.take((size_t)n_cur * 32), o_c = lay.take((size_t)n_cur * 4);
  const size_t in_bytes = lay.off;
  const size_t o_idx = lay.take((size_t)nl * 4), o_dist = lay.take((size_t)nl * 4), o_keys = lay.take(nl > kSortLds ? npad * 8 : 0);
  const size_t o_hdr = lay.take(8), o_pairs = lay.take((size_t)nl * 8);
  SSX_HIP_TRY(ctx, db->io.reserve(lay.off));
  SSX_HIP_TRY(ctx, db->stage.reserve(lay.off));
  char* hs = db->stage.as<char>();
  char* base = db->io.as<char>();
  memcpy(hs + o_d, cur_desc, (size_t)n_cur * 32);
  memcpy(hs + o_c, cur_class_id, (size_t)n_cur * 4);
  SSX_HIP_TRY(ctx, hipMemcpyAsync(base, hs, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  const char* blob = db->arena.as<char>() + row.off;
  // cv::BFMatcher::match(loop, current): query = the resident loop descriptors, train = the current ones
  SSX_PROF(ctx, KID_LOOP_MATCH, ssxorb::launch_bf_match(ctx->stream, (const uint8_t*)(blob + blob_desc(row.n_bow, nl)), nl, (const uint8_t*)(base + o_d), n_cur,
                                                        (int*)(base + o_idx), (int*)(base + o_dist)));
  SSX_HIP_TRY(ctx, hipGetLastError());
  SSX_PROF(ctx, KID_LOOP_PAIRS, hipLaunchKernelGGL(k_kfdb_pairs, dim3(1), dim3(kPairsThreads), 0, ctx->stream, (const int*)(base + o_idx), (const int*)(base + o_dist),
                                                   nl, (const int32_t*)(blob + blob_class(row.n_bow)), (const int32_t*)(base + o_c),
                                                   (unsigned long long*)(base + o_keys), (int32_t*)(base + o_hdr), (int32_t*)(base + o_pairs)));
  SSX_HIP_TRY(ctx, hipGetLastError());
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + o_hdr, base + o_hdr, (o_pairs - o_hdr) + (size_t)n_down * 8, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  int32_t hdr[2];
  memcpy(hdr, hs + o_hdr, 8);
  *n_pairs = hdr[0];
  if (min_distance) *min_distance = hdr[1];
  if (cap > 0) memcpy(pairs_out, hs + o_pairs, (size_t)std::min(hdr[0], cap) * 8);
  if (hdr[0] > cap) { ctx->set_error("ssx_kfdb_match_features: %d pairs but capacity %d", hdr[0], cap); return SSX_ERR_CAPACITY; }
  return SSX_OK;
}

}  // extern "C"
