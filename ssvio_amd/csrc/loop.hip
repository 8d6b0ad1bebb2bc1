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
// Both grow geometrically with a device-to-device copy.  ssx_kfdb_add stages the blob and its row once and copies them up; it launches nothing.
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
// k_kfdb_pairs   one workgroup after k_bf_match_jobs (stereo.hip): minimum distance, the screen dist <= max(2 min, 30), the kept
//                pairs (current class_id, loop class_id) packed into order-preserving 64-bit keys, a bitonic sort (in LDS up
//                to 4096 keys, else in a global scratch), and the unique keys written in order = the std::set.
// k_kf_compact   one workgroup: the kept pyramid keypoints, their descriptors and class ids in push_back order (orbextractor.cpp:893)
//                by a prefix sum over the keep flags; the count to device memory.
// k_kf_bow       one workgroup: the BowVector of the per-feature (word, weight) exactly as voc.hip builds it on the host.  The keys
//                (word << 32) | feature are unique, so a bitonic sort orders every word's features; the head of a run adds its run's weights
//                in feature order (TF_IDF, TF) or keeps the first (IDF, BINARY); the L1 norm is ONE chain over the words in ascending order,
//                lane by lane over 64-entry chunks like the chain of k_kfdb_score.  Both sums are doubles whose value depends on the order
//                of the additions, so neither is a tree.
// k_kfdb_commit  the pending arrays into a blob of the arena and its row into the table.
// k_kfdb_topk    one workgroup per job: the K <= 8 largest keys (float bits << 32) | ~row of the scores -- per thread in registers, merged in K
//                rounds of a block-wide maximum -- screened by the threshold and by a share of the best, and the match job of every
//                candidate filled on the device, so that the match kernels run for all K behind it without a round trip.
// One entry per stage: pairs, compact, bow, commit and topk take (jobs, one) -- a workgroup or a grid row per job of a device table (kf_batch.hpp),
// or with jobs == null the one job as a kernel argument -- and read their counts from the job's StepHdr in device memory.  The score kernel
// alone keeps k_kfdb_score<LDS> for one query and k_kfdb_score_jobs for a table: merged it was measurably slower (launch_score).
//
// The host side is ONE chain, describe (orb.hip) -> [k_kfdb_commit] -> k_kf_compact -> k_voc_words (voc.hip) -> k_kf_bow -> [k_kfdb_score]
// (chain_reserve, chain_enqueue), a verdict (step_verdict) and a match phase k_bf_match_jobs -> k_kfdb_pairs (match_phase).  Its callers:
//   ssx_kfdb_process_keyframe        the per-keyframe step of the loop-closing thread (ProcessNewKeyframe, DetectLoop, MatchFeatures of
//       loopclosing.cpp:596-634, :72-103, :105-145): the chain with one job by value, the verdict, the match phase with one entry.  It leaves
//       the keyframe in the PENDING slot: kps | descriptors | class ids | BowVector ids | values, each at the capacity n_features *
//       pyramid_levels, the two counts known to the host.  ssx_kfdb_add_pending moves it into the arena: k_kfdb_commit, one job by value.
//   ssx_kfdb_process_keyframe_batch  that step for one keyframe of each of n databases of one context (the streams of a batched cohort): the
//       chain over a job table that goes up with the describe block, a job's commit of its previous pending keyframe inside it, n verdicts,
//       the match phase with the found jobs.
//   ssx_kfdb_relocalize_query        the query of a frame that lost tracking: the chain with one job by value into scratch of
//       its own and over EVERY stored keyframe, k_kfdb_topk, the match kernels over the table it filled, ONE synchronisation.  The database
//       and its pending keyframe are only read.
//   ssx_kfdb_relocalize_query_batch  that query for one frame of each of n databases of one context (the lost streams of a batched cohort):
//       the chain over a job table into scratch of the call, a job's commit of its pending keyframe inside it, k_kfdb_topk with a workgroup
//       per job, the match kernels once over the n x K table, ONE copy of the n result blocks and ONE synchronisation.
//   ssx_kfdb_detect_loop / ssx_kfdb_match_features / ssx_kfdb_debug_bow   one stage on a caller's arrays: the score launch, the match
//       launch and the words + BowVector launch of the chain, each with one job by value.
//   ssx_kfdb_guided_search / ssx_kfdb_project_match   the second step of relocalisation, in loop_guided.inc: the describe and
//       k_kfdb_project -> k_kfdb_claim x 2, ONE synchronisation; the database and its pending keyframe are only read.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "kf_batch.hpp"
#include "orb_ws.hpp"
#include "voc.hpp"
#include "../../include/ssx_test_hooks.h"

namespace {

struct KfRow {
  int64_t off;      // byte offset of the blob in the arena
  int32_t n_bow;    // BowVector entries
  int32_t n_desc;   // descriptors; -1: the keyframe was added without any
};
// The counts of one job of the chain, in device memory: k_kf_compact writes n_pyr, k_kf_bow reads it and writes n_bow (and zeroes best),
// k_kfdb_score reads n_bow and raises best.  It is what the first synchronisation brings down, per keyframe step.
struct StepHdr { int32_t n_pyr, n_bow; unsigned long long best; };

constexpr int kQueryLds = 4096;     // query words staged in LDS (12 bytes each)
constexpr int kSortLds = 4096;      // keys sorted in LDS (8 bytes each)
constexpr int kPairsThreads = 1024;
constexpr int kChunks = 4;          // 64-entry chunks of a row a wavefront has in flight

__host__ __device__ inline size_t blob_vals(int n_bow) { return ((size_t)n_bow * 4 + 7) & ~size_t(7); }
__host__ __device__ inline size_t blob_class(int n_bow) { return blob_vals(n_bow) + (size_t)n_bow * 8; }
__host__ __device__ inline size_t blob_desc(int n_bow, int n_desc) { return (blob_class(n_bow) + (size_t)n_desc * 4 + 31) & ~size_t(31); }
__host__ __device__ inline size_t blob_bytes(int n_bow, int n_desc) { return (blob_desc(n_bow, n_desc) + (size_t)n_desc * 32 + 31) & ~size_t(31); }

__device__ __forceinline__ double readlane_f64(double v, int l)
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// The rows blockIdx.x * 4 + wave + gridDim.x * 4 k of the first n_rows keyframes against the query (qi, qv) of nq words.  Called once with
// the query in LDS and once with it in global memory, so that after inlining each copy addresses one known memory.
__device__ __forceinline__ void score_rows(const char* arena, const KfRow* rows, int n_rows, const int32_t* qi, const double* qv, int nq, double* scores,
                                           unsigned long long* best)
{
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

// the query into LDS: [nq] values, then [nq] ids
__device__ __forceinline__ void stage_query(double* smem, const int32_t* q_ids, const double* q_vals, int nq)
{
  int32_t* si = reinterpret_cast<int32_t*>(smem + nq);
  for (int k = threadIdx.x; k < nq; k += blockDim.x) { smem[k] = q_vals[k]; si[k] = q_ids[k]; }
  __syncthreads();
}

// (jobs, one): with jobs == null the one job of the launch is `one`, a kernel argument, and no workgroup reads a table.  The body is called
// once with either, so that each copy reads the job from one known memory with scalar loads (behind a chosen pointer, a flat one, its fields land in VGPRs).
template <class Body> __device__ __forceinline__ void with_job(const KfJobDev* jobs, const KfJobDev& one, unsigned i, Body&& body) { if (jobs) body(jobs[i]); else body(one); }

// The score kernel alone keeps a form per caller (launch_score says why).  The single calls: scores[row] = L1Scoring::score(query, row)
// for the first n_rows keyframes; *best = max over rows of (float bits << 32) | ~row
template <bool LDS>
__global__ __launch_bounds__(256) void k_kfdb_score(const char* arena, const KfRow* rows, int n_rows, const int32_t* q_ids, const double* q_vals, int nq,
                                                    const int32_t* nq_dev, double* scores, unsigned long long* best)
{
  extern __shared__ double smem[];                            // [nq] values, then [nq] ids
  if (nq_dev) nq = *nq_dev;                                   // the query was built on the device: `nq` was its bound (it sized the LDS)
  if (LDS) {
    stage_query(smem, q_ids, q_vals, nq);
    score_rows(arena, rows, n_rows, reinterpret_cast<const int32_t*>(smem + nq), smem, nq, scores, best);
  } else {
    score_rows(arena, rows, n_rows, q_ids, q_vals, nq, scores, best);
  }
}

// grid (blocks, job): every job scores its own eligible prefix of its own database against the BowVector in its pending arrays.  The dynamic
// LDS holds lds_cap query words (the call's largest bound, at most kQueryLds); a longer query is searched in global memory.
__global__ __launch_bounds__(256) void k_kfdb_score_jobs(const KfJobDev* jobs, StepHdr* hdr, int lds_cap)
{
  extern __shared__ double smem[];
  const KfJobDev& j = jobs[blockIdx.y];
  const int n_rows = j.n_elig;
  if ((int)blockIdx.x * 4 >= n_rows) return;                  // nothing eligible, or fewer rows than the largest job has
  StepHdr* h = hdr + blockIdx.y;
  const int nq = h->n_bow;
  const char* arena = j.arena;
  const KfRow* rows = static_cast<const KfRow*>(j.rows);
  if (nq <= lds_cap) {
    stage_query(smem, j.p_ids, j.p_vals, nq);
    score_rows(arena, rows, n_rows, reinterpret_cast<const int32_t*>(smem + nq), smem, nq, j.scores, &h->best);
  } else {
    score_rows(arena, rows, n_rows, j.p_ids, j.p_vals, nq, j.scores, &h->best);
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

// keys[0, n_valid) ascending by a bitonic sort of npad = 2^m >= n_valid keys, the tail padded with ~0 (it sorts last).  Its callers are
// each called once with the LDS array and once with the global scratch, so that after inlining each copy addresses one known memory (no
// flat pointer to LDS).
__device__ __forceinline__ void bitonic_sort_padded(unsigned long long* keys, int n_valid, int npad)
{
  const int tid = threadIdx.x;
  for (int i = n_valid + tid; i < npad; i += kPairsThreads) keys[i] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (npad >> 1); t += kPairsThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const unsigned long long a = keys[i], b = keys[i | j];
        if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[i | j] = a; }
      }
      __syncthreads();
    }
  }
}

// The kept pairs as keys into `keys`, sorted, the first of every run written out.  Called once with the LDS array and once with the
// global scratch (bitonic_sort_padded).
__device__ __forceinline__ void sort_unique_pairs(unsigned long long* keys, int n_valid, int npad, int thr, const int* idx, const int* dist, int n_loop,
                                                  const int32_t* loop_class, const int32_t* cur_class, int* s_fill, int* wave_sums, int32_t* hdr,
                                                  int32_t* pairs, int min_d)
{
  const int tid = threadIdx.x;
  for (int i = tid; i < n_loop; i += kPairsThreads)
    if (dist[i] <= thr) keys[atomicAdd(s_fill, 1)] = pair_key(cur_class[idx[i]], loop_class[i]);   // any order: sorted next
  bitonic_sort_padded(keys, n_valid, npad);
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
__device__ __forceinline__ void pairs_block(const int* idx, const int* dist, int n_loop, const int32_t* loop_class, const int32_t* cur_class,
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

// one workgroup per match job, behind k_bf_match_jobs (stereo.hip) over the same jobs
__global__ __launch_bounds__(kPairsThreads) void k_kfdb_pairs(const KfMatchJob* jobs, KfMatchJob one)
{
  const KfMatchJob j = jobs ? jobs[blockIdx.x] : one;
  if (j.nl <= 0) return;                                      // a table filled on the device (k_kfdb_topk) has empty entries: their header stays (0, -1)
  pairs_block(j.idx, j.dist, j.nl, j.loop_cls, j.cur_cls, j.keys, j.hdr, j.pairs);
}


// the kept keypoints of k_describe_at, their descriptors and class ids, in input order; *count = how many
__device__ __forceinline__ void compact_block(const ssx_keypoint* kps, const uint8_t* desc, const uint8_t* keep, int n, ssx_keypoint* okps,
                                              uint8_t* odesc, int32_t* ocls, int32_t* count)
{
  __shared__ int wave_sums[kPairsThreads / 64];
  const int tid = threadIdx.x;
  const int seg = (n + kPairsThreads - 1) / kPairsThreads;    // a thread takes a contiguous piece
  const int i0 = min(tid * seg, n), i1 = min(i0 + seg, n);
  int mine = 0;
  for (int i = i0; i < i1; ++i) mine += keep[i] ? 1 : 0;
  int total = 0;
  int pos = block_scan_excl(mine, wave_sums, &total);
  for (int i = i0; i < i1; ++i) {
    if (!keep[i]) continue;
    const ssx_keypoint kp = kps[i];
    const uint4* d4 = reinterpret_cast<const uint4*>(desc + (size_t)32 * i);
    uint4* o4 = reinterpret_cast<uint4*>(odesc + (size_t)32 * pos);
    okps[pos] = kp;
    o4[0] = d4[0]; o4[1] = d4[1];
    ocls[pos] = kp.class_id;
    ++pos;
  }
  if (tid == 0) *count = total;
}

// one workgroup per job: the describe kernel's outputs of the job (entries kp0 .. kp0 + n_in of the concatenated arrays) into its pending
// arrays, the count into its header
__global__ __launch_bounds__(kPairsThreads) void k_kf_compact(const KfJobDev* jobs, KfJobDev one, const ssx_keypoint* kps, const uint8_t* desc, const uint8_t* keep,
                                                              StepHdr* hdr)
{
  with_job(jobs, one, blockIdx.x, [&](const KfJobDev& j) __attribute__((always_inline)) {
    compact_block(kps + j.kp0, desc + (size_t)32 * j.kp0, keep + j.kp0, j.n_in, j.p_kps, j.p_desc, j.p_cls, &hdr[blockIdx.x].n_pyr); });
}

// The BowVector of n features from their (word, weight), as ssx_voc_transform assembles it (TemplatedVocabulary.h:1083-1124,
// BowVector.cpp:62-84).  Called once with the LDS array and once with the global scratch, like sort_unique_pairs.
__device__ __forceinline__ void bow_assemble(unsigned long long* keys, int n, int n_valid, int npad, const int32_t* word, const double* weight, bool add,
                                             int* s_fill, int* wave_sums, double* s_norm, int32_t* ids, double* vals, int32_t* n_bow_out)
{
  const int tid = threadIdx.x;
  for (int f = tid; f < n; f += kPairsThreads)
    if (word[f] >= 0 && weight[f] > 0) keys[atomicAdd(s_fill, 1)] = ((unsigned long long)(unsigned)word[f] << 32) | (unsigned)f;   // any order: sorted next
  bitonic_sort_padded(keys, n_valid, npad);                   // (these keys are unique)
  // keys [0, n_valid): ascending word, and inside a word ascending feature.  A thread takes a contiguous piece; the head of a run is an entry
  const int seg = (n_valid + kPairsThreads - 1) / kPairsThreads;
  const int i0 = min(tid * seg, n_valid), i1 = min(i0 + seg, n_valid);
  int heads = 0;
  for (int i = i0; i < i1; ++i) heads += (i == 0 || (keys[i] >> 32) != (keys[i - 1] >> 32)) ? 1 : 0;
  int n_bow = 0;
  int pos = block_scan_excl(heads, wave_sums, &n_bow);
  for (int i = i0; i < i1; ++i) {
    const unsigned long long key = keys[i];
    const unsigned w = (unsigned)(key >> 32);
    if (i > 0 && (unsigned)(keys[i - 1] >> 32) == w) continue;
    double v = weight[(unsigned)key];                         // the first occurrence inserts its weight ...
    if (add)                                                  // ... and TF_IDF / TF add the later ones in feature order: one chain per word
      for (int j = i + 1; j < n_valid && (unsigned)(keys[j] >> 32) == w; ++j) v += weight[(unsigned)keys[j]];
    ids[pos] = (int32_t)w;
    vals[pos] = v;
    ++pos;
  }
  __syncthreads();
  if (tid < 64) {                                             // the L1 norm: sum of fabs in ascending word order, ONE chain
    double s = 0.0;
    for (int base = 0; base < n_bow; base += 64) {
      const int k = base + tid;
      const double v = k < n_bow ? fabs(vals[k]) : 0.0;
      const int cnt = min(64, n_bow - base);
      for (int l = 0; l < cnt; ++l) s += readlane_f64(v, l);
    }
    if (tid == 0) *s_norm = s;
  }
  __syncthreads();
  const double norm = *s_norm;
  if (norm > 0.0)
    for (int k = tid; k < n_bow; k += kPairsThreads) vals[k] /= norm;
  if (tid == 0) *n_bow_out = n_bow;
}

// ids / vals / *n_bow = the BowVector of the first *n_dev features; *best_zero = 0 for the k_kfdb_score that follows
__device__ __forceinline__ void bow_block(const int32_t* word, const double* weight, const int32_t* n_dev, int weighting, unsigned long long* gkeys,
                                          int32_t* ids, double* vals, int32_t* n_bow, unsigned long long* best_zero)
{
  __shared__ unsigned long long skeys[kSortLds];
  __shared__ int wave_sums[kPairsThreads / 64];
  __shared__ int s_fill;
  __shared__ double s_norm;
  const int tid = threadIdx.x;
  const int n = *n_dev;
  if (tid == 0) { s_fill = 0; s_norm = 0.0; if (best_zero) *best_zero = 0; }
  int mine = 0;
  for (int f = tid; f < n; f += kPairsThreads) mine += (word[f] >= 0 && weight[f] > 0) ? 1 : 0;   // stopped words (weight 0) are skipped
  int n_valid = 0;
  block_scan_excl(mine, wave_sums, &n_valid);                 // (its barriers publish s_fill)
  int npad = 1;
  while (npad < n_valid) npad <<= 1;
  const bool add = weighting == 0 || weighting == 1;          // TF_IDF, TF
  if (npad <= kSortLds)
    bow_assemble(skeys, n, n_valid, npad, word, weight, add, &s_fill, wave_sums, &s_norm, ids, vals, n_bow);
  else                                                        // gkeys holds the next power of two of the feature bound
    bow_assemble(gkeys, n, n_valid, npad, word, weight, add, &s_fill, wave_sums, &s_norm, ids, vals, n_bow);
}

// one workgroup per job: its BowVector from its slice of the concatenated words and weights, the count read from its header
__global__ __launch_bounds__(kPairsThreads) void k_kf_bow(const KfJobDev* jobs, KfJobDev one, const int32_t* word, const double* weight, int weighting, StepHdr* hdr)
{
  StepHdr* h = hdr + blockIdx.x;
  with_job(jobs, one, blockIdx.x, [&](const KfJobDev& j) __attribute__((always_inline)) {
    bow_block(word + j.kp0, weight + j.kp0, &h->n_pyr, weighting, j.bow_keys, j.p_ids, j.p_vals, &h->n_bow, &h->best); });
}

// the pending keyframe into its blob (layout at the top of the file, padding zeroed) and its row into the table
__device__ __forceinline__ void commit_blob(char* blob, const int32_t* ids, const double* vals, const int32_t* cls, const uint8_t* desc, int n_bow, int n_desc,
                                            KfRow* row_out, KfRow row)
{
  const size_t o_v = blob_vals(n_bow), o_c = blob_class(n_bow), o_d = blob_desc(n_bow, n_desc), words = blob_bytes(n_bow, n_desc) / 4;
  const uint32_t* v32 = reinterpret_cast<const uint32_t*>(vals);
  const uint32_t* d32 = reinterpret_cast<const uint32_t*>(desc);
  uint32_t* out = reinterpret_cast<uint32_t*>(blob);
  for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (size_t)gridDim.x * blockDim.x) {
    const size_t off = w * 4;
    uint32_t x = 0;
    if (off < (size_t)n_bow * 4) x = (uint32_t)ids[w];
    else if (off >= o_v && off < o_c) x = v32[(off - o_v) / 4];
    else if (off >= o_c && off < o_c + (size_t)n_desc * 4) x = (uint32_t)cls[(off - o_c) / 4];
    else if (off >= o_d && off < o_d + (size_t)n_desc * 32) x = d32[(off - o_d) / 4];
    out[w] = x;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *row_out = row;
}

// grid (blocks, job): the jobs that commit move their previous pending keyframe into its blob, before anything overwrites it
__global__ __launch_bounds__(256) void k_kfdb_commit(const KfJobDev* jobs, KfJobDev one)
{
  with_job(jobs, one, blockIdx.y, [&](const KfJobDev& j) __attribute__((always_inline)) {
    if (!j.commit) return;
    commit_blob(j.c_blob, j.c_ids, j.c_vals, j.c_cls, j.c_desc, j.c_n_bow, j.c_n_desc, static_cast<KfRow*>(j.c_row_out), KfRow{j.c_off, j.c_n_bow, j.c_n_desc});
  });
}

// ---- the candidate query of relocalisation (ssx_kfdb_relocalize_query; the rule: tools/reloc_model.py) ----
constexpr int kTopK = SSX_RELOC_MAX_CANDIDATES;
struct RelocDev {                    // what the query's one synchronisation brings down
  StepHdr h;
  int32_t n_cand, pad;
  int32_t row[kTopK];                // the candidates in order; -1 behind the last
  uint32_t fbits[kTopK];             // their float scores
};
// where candidate c's match job finds the frame's side and its slices of the scratch and of the mapped pinned output
struct RelocMatch {
  const uint8_t* cur_desc; const int32_t* cur_cls;
  int* idx; int* dist; unsigned long long* keys;   // c * max_nl, c * max_nl, c * keys_stride (keys null: every sort fits the LDS)
  char* out; size_t out_stride;                    // c * out_stride: the candidate's block of the mapped pinned output (match_out)
  int max_nl; size_t keys_stride;
};
constexpr size_t kMatchPairsOff = 256;             // a block of the match output: (pair count, minimum distance), and the pairs this far behind

// One workgroup after k_kfdb_score: the kTopK largest keys (float bits << 32) | ~row of the scores, i.e. f descending and then row
// ascending.  A thread keeps the kTopK largest of rows tid + 1024 k in registers, sorted; kTopK rounds then take the block-wide maximum
// of the threads' heads through LDS, and the thread that held it moves on to its next (keys of rows are unique, 0 = none).  No
// floating-point arithmetic but the narrowing and the one product ratio * f_best, no atomics: a pure function of the scores.
// Threads 0 .. max_cand - 1 then screen their candidate (f >= threshold, f >= ratio * f_best: both hold for a prefix of the order)
// and fill its match job, with nl = 0 where there is nothing to match (no candidate, no descriptors on either side).
__device__ __forceinline__ void topk_block(const double* scores, int n_rows, const char* arena, const KfRow* rows, int max_cand, float threshold, float ratio,
                                           RelocDev* out, const StepHdr* hdr, KfMatchJob* jobs, const RelocMatch& mb)
{
  __shared__ unsigned long long s_wave[kPairsThreads / 64];
  __shared__ unsigned long long s_top[kTopK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long top[kTopK];
#pragma unroll
  for (int k = 0; k < kTopK; ++k) top[k] = 0;
  for (int row = tid; row < n_rows; row += kPairsThreads) {
    const float f = (float)scores[row];
    if (!(f > 0.f)) continue;
    const unsigned long long key = ((unsigned long long)__float_as_uint(f) << 32) | (unsigned)~row;
    if (key <= top[kTopK - 1]) continue;
    top[kTopK - 1] = key;
#pragma unroll
    for (int k = kTopK - 1; k > 0; --k) {                     // one pass of a bubble: the array stays sorted descending
      const unsigned long long a = top[k - 1], b = top[k];
      top[k - 1] = max(a, b); top[k] = min(a, b);
    }
  }
#pragma unroll
  for (int r = 0; r < kTopK; ++r) {
    unsigned long long m = top[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned long long)__shfl_xor((long long)m, o));
    if (lane == 0) s_wave[wave] = m;
    __syncthreads();
    unsigned long long win = 0;
#pragma unroll
    for (int w = 0; w < kPairsThreads / 64; ++w) win = max(win, s_wave[w]);
    if (tid == 0) s_top[r] = win;
    if (win != 0 && top[0] == win) {                          // exactly one thread: it moves on to its next key
#pragma unroll
      for (int k = 0; k + 1 < kTopK; ++k) top[k] = top[k + 1];
      top[kTopK - 1] = 0;
    }
    __syncthreads();                                          // s_wave is rewritten by the next round; s_top is read below
  }
  if (tid >= 64) return;
  const int c = tid;
  const unsigned long long key = c < kTopK ? s_top[c] : 0;
  const float f = __uint_as_float((unsigned)(key >> 32)), f_best = __uint_as_float((unsigned)(s_top[0] >> 32));
  const bool ok = c < max_cand && key != 0 && f >= threshold && f >= ratio * f_best;
  const int n_cand = __popcll(__ballot(ok));
  if (c == 0) { out->n_cand = n_cand; out->pad = 0; }
  if (hdr && c == 0) { out->h.n_pyr = hdr->n_pyr; out->h.n_bow = hdr->n_bow; out->h.best = hdr->best; }   // a table's block takes its job's header along: one copy brings both down
  if (c >= kTopK) return;
  const int row = (int)~(unsigned)key;
  out->row[c] = ok ? row : -1;
  out->fbits[c] = ok ? (unsigned)(key >> 32) : 0u;
  if (c >= max_cand) return;
  const int n_cur = hdr ? hdr->n_pyr : out->h.n_pyr;          // (k_kf_compact's count, an earlier launch)
  KfMatchJob j{};
  j.cur_desc = mb.cur_desc; j.cur_cls = mb.cur_cls;
  j.idx = mb.idx + (size_t)c * mb.max_nl; j.dist = mb.dist + (size_t)c * mb.max_nl;
  j.keys = mb.keys ? mb.keys + (size_t)c * mb.keys_stride : nullptr;
  j.hdr = reinterpret_cast<int32_t*>(mb.out + (size_t)c * mb.out_stride); j.pairs = j.hdr + kMatchPairsOff / 4;
  j.n_cur = n_cur;
  if (ok) {
    const KfRow r = rows[row];
    if (r.n_desc > 0 && r.n_desc <= mb.max_nl && n_cur > 0) { // (n_desc <= max_nl by construction: the scratch is sized by the host mirror's largest)
      const char* blob = arena + r.off;
      j.loop_desc = (const uint8_t*)(blob + blob_desc(r.n_bow, r.n_desc)); j.loop_cls = (const int32_t*)(blob + blob_class(r.n_bow));
      j.nl = r.n_desc;
    }
  }
  jobs[c] = j;
}

// One workgroup per job.  The single query: the job `one` and its RelocMatch `mb1` by value, its result block `out` for a header, `jobs`
// its max_cand match jobs.  A table: job i scores j.n_elig rows of its own database, reads header i of `hdr`, writes block i of `out`
// and slice i of `jobs`, and finds its slices of the scratch and of the mapped output in entry i of `mbs`.
__global__ __launch_bounds__(kPairsThreads) void k_kfdb_topk(const KfJobDev* tab, KfJobDev one, const RelocMatch* mbs, RelocMatch mb1, int max_cand, float threshold,
                                                             float ratio, RelocDev* out, const StepHdr* hdr, KfMatchJob* jobs)
{
  const unsigned i = blockIdx.x;
  with_job(tab, one, i, [&](const KfJobDev& j) __attribute__((always_inline)) {
    if (tab) topk_block(j.scores, j.n_elig, j.arena, static_cast<const KfRow*>(j.rows), max_cand, threshold, ratio, out + i, hdr + i, jobs + (size_t)i * max_cand, mbs[i]);
    else topk_block(j.scores, j.n_elig, j.arena, static_cast<const KfRow*>(j.rows), max_cand, threshold, ratio, out, nullptr, jobs, mb1);
  });
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
  // the pending keyframe: arrays of capacity `cap` entries each in `pend` (pend_arrays), the counts known to the host
  DevBuf pend;
  struct Pending { bool valid = false; int64_t kf_id = 0; int cap = 0, n_pyr = 0, n_bow = 0; } pending;
  KfChainStats last;              // what the last ssx_kfdb_process_keyframe / ssx_kfdb_relocalize_query issued (ssx_kfdb_debug_last_step)
};

namespace {

struct PendArrays { ssx_keypoint* kps; uint8_t* desc; int32_t* cls; int32_t* ids; double* vals; };
// the pending slot for `cap` pyramid keypoints; base null: the bytes only
size_t pend_arrays(char* base, int cap, PendArrays& a)
{
  return carve(base, [&](auto&& f) {
    f(a.kps, sizeof(ssx_keypoint) * (size_t)cap); f(a.desc, (size_t)32 * cap); f(a.cls, (size_t)4 * cap); f(a.ids, (size_t)4 * cap); f(a.vals, (size_t)8 * cap);
  });
}

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

// "job 3: " in the messages of a batch, nothing in those of a single call (job < 0)
struct JobTag { char s[24] = ""; explicit JobTag(int job) { if (job >= 0) snprintf(s, sizeof s, "job %d: ", job); } };

// the global scratch of a bitonic sort of up to `bound` keys: none while they fit the LDS
size_t sort_scratch_bytes(int bound)
{
  size_t npad = 1;
  while (npad < (size_t)bound) npad *= 2;
  return bound > kSortLds ? npad * 8 : 0;
}

// ---- the commit: a keyframe into the arena and the table (AddToKeyframeDatabase) --------------------------------------------------------
// ids ascend (the std::map of the reference is walked as a prefix, loopclosing.cpp:79) and the table has room
ssx_status check_commit(const ssx_kf_database* db, const char* who, int job, int64_t kf_id)
{
  if (!db->ids.empty() && kf_id <= db->ids.back()) {
    db->ctx->set_error("%s: keyframe id %lld after %lld (ids must ascend)", who, (long long)kf_id, (long long)db->ids.back());
    return SSX_ERR_INVALID_ARG;
  }
  if (db->ids.size() >= (size_t)0x7fffffff) { db->ctx->set_error("%s: %sthe database is full", who, JobTag(job).s); return SSX_ERR_CAPACITY; }
  return SSX_OK;
}
// room for one more blob and one more row; *moved = the buffers that had to move (each with a synchronisation of its own)
hipError_t grow_for_commit(ssx_kf_database* db, size_t blob, int* moved = nullptr)
{
  const size_t cap_a = db->arena.cap, cap_t = db->table.cap, n = db->ids.size();
  hipError_t e = grow_keep(db->ctx, db->arena, db->used, db->used + blob);
  if (e == hipSuccess) e = grow_keep(db->ctx, db->table, n * sizeof(KfRow), (n + 1) * sizeof(KfRow));
  if (moved) *moved = (db->arena.cap != cap_a ? 1 : 0) + (db->table.cap != cap_t ? 1 : 0);
  return e;
}
// the host mirrors follow a commit that has happened on the device
void commit_mirror(ssx_kf_database* db, int64_t kf_id, const KfRow& row, size_t blob)
{
  db->ids.push_back(kf_id); db->rows.push_back(row);
  db->used += blob; db->n_bow += row.n_bow; db->n_desc += std::max(row.n_desc, 0);
}
// the commit of the pending keyframe as k_kfdb_commit reads it from a job (after grow_for_commit: the blob and the row lie where they stay)
void commit_job(KfJobDev& t, const ssx_kf_database* db)
{
  const ssx_kf_database::Pending& pe = db->pending;
  PendArrays old{};
  pend_arrays(db->pend.as<char>(), pe.cap, old);              // (cap == 0: an empty keyframe, nothing is read)
  t.commit = 1;
  t.c_ids = old.ids; t.c_vals = old.vals; t.c_cls = old.cls; t.c_desc = old.desc;
  t.c_blob = db->arena.as<char>() + db->used; t.c_row_out = db->table.as<KfRow>() + db->ids.size();
  t.c_off = (int64_t)db->used; t.c_n_bow = pe.n_bow; t.c_n_desc = pe.n_pyr;
}

// ---- the chain: [commit] -> compact -> words -> BowVector -> [score], for n jobs --------------------------------------------------------
// The frame arguments of a keyframe step or a query.  Two checks: every caller has one of its own between them (the contexts of its
// handles), and their order decides the error code of a call that is wrong twice.
struct FrameArgs {
  const uint8_t* img; int32_t stride, rows, cols; const ssx_orb_params* prm; int32_t n_features; const ssx_keypoint* features; int32_t pyramid_levels, pairs_cap; const int32_t* pairs_out;
};
bool frame_args_ok(const FrameArgs& a)
{
  return a.prm && a.img && a.rows > 0 && a.cols > 0 && a.stride >= a.cols && a.n_features >= 0 && (a.n_features == 0 || a.features) && a.pyramid_levels >= 1 &&
         a.pyramid_levels <= ssxorb::MAX_LEVELS && a.pairs_cap >= 0 && (a.pairs_cap == 0 || a.pairs_out);
}
// (k_bf_match packs a train index into 16 bits, and the pyramid keypoints of a frame are the train side of its match)
ssx_status check_pyramid_bound(ssx_ctx* ctx, const char* who, int job, const FrameArgs& a)
{
  if ((int64_t)a.n_features * a.pyramid_levels <= 65535) return SSX_OK;
  ctx->set_error("%s: %s%d features x %d levels: more than 65535 pyramid keypoints", who, JobTag(job).s, a.n_features, a.pyramid_levels);
  return SSX_ERR_UNSUPPORTED;
}

// One enqueue of the chain.  The caller states n, the jobs (n_in, n_elig, the pending arrays, the database, a commit), the describe outputs, the bound.
struct Chain {
  int n = 0; KfJobDev* jobs = nullptr;  // on the host: the table that goes up with the describe block, or the one job
  const KfJobDev* dev_jobs = nullptr;   // the table on the device; null: jobs[0] travels as a kernel argument
  const ssx_keypoint* kps = nullptr; const uint8_t* desc = nullptr; const uint8_t* keep = nullptr;   // the describe outputs, concatenated over the jobs
  int bound = 0;                        // the query's bound, or the largest of the table's (launch_score)
  StepHdr* hdr = nullptr; int32_t* word = nullptr; double* weight = nullptr; int total = 0;        // chain_reserve
};

// The device scratch of the chain in `io`: [header block | words | weights | per job: the BowVector's global sort scratch, the scores],
// then what the caller adds to the same buffer (`more`, the carve idiom).  The header block is a StepHdr per job, or a caller's larger
// block that begins with one.  `stage` takes the headers when they come down.
template <class More>
hipError_t chain_reserve(DevBuf& io, HostBuf& stage, Chain& c, size_t hdr_bytes, More&& more)
{
  c.total = 0;
  for (int j = 0; j < c.n; ++j) c.total += c.jobs[j].n_in;
  auto scratch = [&](auto&& f) {
    f(c.hdr, hdr_bytes); f(c.word, (size_t)4 * c.total); f(c.weight, (size_t)8 * c.total);
    for (int j = 0; j < c.n; ++j) { f(c.jobs[j].bow_keys, sort_scratch_bytes(c.jobs[j].n_in)); f(c.jobs[j].scores, (size_t)c.jobs[j].n_elig * 8); }
    more(f);
  };
  hipError_t e = io.reserve(carve(nullptr, scratch));
  if (e == hipSuccess) e = stage.reserve(sizeof(StepHdr) * (size_t)c.n + 256);
  if (e == hipSuccess) carve(io.as<char>(), scratch);
  return e;
}
const auto nothing_more = [](auto&&) {};
// the frame side and the database of a job
void job_arrays(KfJobDev& t, const PendArrays& pa, const ssx_kf_database* db)
{
  t.p_kps = pa.kps; t.p_desc = pa.desc; t.p_cls = pa.cls; t.p_ids = pa.ids; t.p_vals = pa.vals;
  t.arena = db->arena.as<char>(); t.rows = db->table.p;
}

// k_voc_words + k_kf_bow: n_pyr descriptors of every job (its p_desc) into its BowVector (p_ids, p_vals, n_bow of its header)
void launch_words_bow(ssx_ctx* ctx, const ssx_vocabulary* voc, const KfJobDev* tab, const KfJobDev& one, int n, int total, StepHdr* hdr, int32_t* word, double* weight)
{
  hipStream_t s = ctx->stream;
  if (tab)
    SSX_PROF(ctx, KID_LOOP_WORDS, ssxvoc::launch_words_jobs(s, voc, tab, n, &hdr->n_pyr, (int)(sizeof(StepHdr) / 4), total, word, weight));
  else
    SSX_PROF(ctx, KID_LOOP_WORDS, ssxvoc::launch_words(s, voc, one.p_desc, one.n_in, &hdr->n_pyr, word, weight));
  SSX_PROF(ctx, KID_LOOP_BOW, hipLaunchKernelGGL(k_kf_bow, dim3(n), dim3(kPairsThreads), 0, s, tab, one, word, weight, voc->weighting, hdr));
}

// The scores of n jobs, the largest of max_elig stored keyframes.  The query is staged in LDS or searched in global memory, and the
// single calls and the batch choose differently: a single call stages by its BOUND (all of it when it fits kQueryLds, else nothing: such
// a query is searched in global memory however short it came out), the batch stages by each job's LENGTH against the call's cap
// min(largest bound, kQueryLds).  The scores are the same bits either way, the speed is not; making the two alike is a change of
// behaviour that wants a measurement of its own.
// This stage alone keeps the kernel of each: one kernel with both paths behind a job took 55.3 us where k_kfdb_score<true> takes 53.0 us
// (a step against 100 keyframes of 1000 words, MI355X), at the same occupancy and without scratch.  `bound`: the query's bound (a single
// call; its length is read from the header when `on_device`) or the largest bound of the call (a table).
void launch_score(ssx_ctx* ctx, const KfJobDev* tab, const KfJobDev& one, int n, int max_elig, StepHdr* hdr, int bound, bool on_device)
{
  const int blocks = std::min((max_elig + 3) / 4, 1024), lds_cap = std::min(bound, kQueryLds);   // four workgroups per CU; a wavefront takes every 4096th row
  const auto single = bound <= kQueryLds ? k_kfdb_score<true> : k_kfdb_score<false>;
  if (tab)
    SSX_PROF(ctx, KID_LOOP_SCORE, hipLaunchKernelGGL(k_kfdb_score_jobs, dim3(blocks, n), dim3(256), (size_t)lds_cap * 12, ctx->stream, tab, hdr, lds_cap));
  else
    SSX_PROF(ctx, KID_LOOP_SCORE, hipLaunchKernelGGL(single, dim3(blocks), dim3(256), bound <= kQueryLds ? (size_t)bound * 12 : 0, ctx->stream, one.arena,
                                                     static_cast<const KfRow*>(one.rows), one.n_elig, one.p_ids, one.p_vals, bound, on_device ? &hdr->n_bow : nullptr,
                                                     one.scores, &hdr->best));
}
int commit_blocks(size_t blob) { return (int)std::min<size_t>(std::max<size_t>((blob / 4 + 255) / 256, 1), 1024); }

// `down`: the headers of the n jobs come down behind the chain, which is the first synchronisation of a step
hipError_t chain_enqueue(ssx_ctx* ctx, const ssx_vocabulary* voc, HostBuf& stage, const Chain& c, StepHdr* down, KfChainStats& st)
{
  const KfJobDev* tab = c.dev_jobs; const KfJobDev& one = c.jobs[0];
  bool any_commit = false; size_t most = 0, bytes = sizeof(StepHdr) * (size_t)c.n;
  int max_elig = 0;
  for (int j = 0; j < c.n; ++j) {
    const KfJobDev& t = c.jobs[j];
    if (t.commit) { any_commit = true; most = std::max(most, blob_bytes(t.c_n_bow, t.c_n_desc)); }
    max_elig = std::max(max_elig, t.n_elig);
  }
  if (any_commit) {
    SSX_PROF(ctx, KID_LOOP_COMMIT, hipLaunchKernelGGL(k_kfdb_commit, dim3(commit_blocks(most), c.n), dim3(256), 0, ctx->stream, tab, one));
    ++st.launches;
  }
  SSX_PROF(ctx, KID_LOOP_COMPACT, hipLaunchKernelGGL(k_kf_compact, dim3(c.n), dim3(kPairsThreads), 0, ctx->stream, tab, one, c.kps, c.desc, c.keep, c.hdr));
  launch_words_bow(ctx, voc, tab, one, c.n, c.total, c.hdr, c.word, c.weight);
  st.launches += 3;
  if (max_elig > 0) {                                         // the queries where k_kf_bow left them, their lengths read on the device
    launch_score(ctx, tab, one, c.n, max_elig, c.hdr, c.bound, true);
    ++st.launches;
  }
  hipError_t e = hipGetLastError();
  if (!down || e != hipSuccess) return e;
  e = hipMemcpyAsync(stage.p, c.hdr, bytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return e;
  ++st.syncs; st.bytes_down += (int64_t)bytes;
  memcpy(down, stage.p, bytes);
  return hipSuccess;
}

// DetectLoop's verdict from the key k_kfdb_score left: no score above 0 keeps max_score 0 (loopclosing.cpp:74,85); below the threshold: none (:93)
bool winner_of(unsigned long long key, float threshold, uint32_t* row, float* score)
{
  if (key == 0) return false;
  const uint32_t bits = (uint32_t)(key >> 32);
  float f = 0.f;
  memcpy(&f, &bits, 4);
  if (f < threshold) return false;
  *row = ~(uint32_t)key; *score = f;
  return true;
}
ssx_status no_descriptors(ssx_ctx* ctx, const char* who, int job, const char* which, int64_t kf_id)
{
  ctx->set_error("%s: %s%skeyframe %lld was added without descriptors", who, JobTag(job).s, which, (long long)kf_id);
  return SSX_ERR_INVALID_ARG;
}
// the verdict of a keyframe step whose header came down (`scored`: k_kfdb_score ran for it) into found / score / loop_kf_id of its
// result; *match: the winner `row` and the keyframe both have descriptors, so MatchFeatures follows (else no match exists: no pairs)
ssx_status step_verdict(const ssx_kf_database* db, const char* who, int job, const StepHdr& h, bool scored, float threshold, ssx_kfdb_step_result* res, KfRow* row, bool* match)
{
  *match = false;
  uint32_t row_i = 0; float f = 0.f;
  if (!scored || !winner_of(h.best, threshold, &row_i, &f)) return SSX_OK;
  res->found = 1; res->score = f; res->loop_kf_id = db->ids[row_i];
  *row = db->rows[row_i];
  if (row->n_desc < 0) return no_descriptors(db->ctx, who, job, "the loop ", db->ids[row_i]);
  *match = row->n_desc > 0 && h.n_pyr > 0;
  return SSX_OK;
}

// ---- the match phase: MatchFeatures ---------------------------------------------------------------------------------------------------
// cv::BFMatcher::match(loop, current) + the screen and the set: query = the resident descriptors of `row`, train = the n_cur current ones
// on the device.  The job but for its scratch (match_scratch) and for where its result goes.
KfMatchJob match_job(const ssx_kf_database* db, const KfRow& row, const uint8_t* cur_desc, const int32_t* cur_cls, int n_cur)
{
  const char* blob = db->arena.as<char>() + row.off;
  KfMatchJob t{};
  t.loop_desc = (const uint8_t*)(blob + blob_desc(row.n_bow, row.n_desc)); t.loop_cls = (const int32_t*)(blob + blob_class(row.n_bow));
  t.cur_desc = cur_desc; t.cur_cls = cur_cls; t.nl = row.n_desc; t.n_cur = n_cur;
  return t;
}
template <class F> void match_scratch(F&& f, KfMatchJob& t) { f(t.idx, (size_t)t.nl * 4); f(t.dist, (size_t)t.nl * 4); f(t.keys, sort_scratch_bytes(t.nl)); }
// k_bf_match_jobs + k_kfdb_pairs over n jobs, the largest of max_nl stored descriptors; tab null (n == 1): the job is `one`
hipError_t launch_match_jobs(ssx_ctx* ctx, const KfMatchJob* tab, const KfMatchJob& one, int n, int max_nl)
{
  SSX_PROF(ctx, KID_LOOP_MATCH, ssxorb::launch_bf_match_jobs(ctx->stream, tab, one, n, max_nl));
  SSX_PROF(ctx, KID_LOOP_PAIRS, hipLaunchKernelGGL(k_kfdb_pairs, dim3(n), dim3(kPairsThreads), 0, ctx->stream, tab, one));
  return hipGetLastError();
}
// A job's result in pinned memory that is mapped into the device's address space: (pair count, minimum distance), and kMatchPairsOff
// bytes behind them the pairs, written by k_kfdb_pairs straight from the device: what crosses is the 8-byte header and 8 bytes per pair.
size_t match_out_bytes(int nl) { return kMatchPairsOff + (size_t)nl * 8; }
void match_out_preset(int32_t* o) { o[0] = 0; o[1] = -1; }    // what a job that no workgroup runs for reads as
struct MatchResult { int n_pairs, min_distance; const int32_t* pairs; };
MatchResult match_out_read(const int32_t* o) { return MatchResult{o[0], o[1], o + kMatchPairsOff / 4}; }
int64_t match_out_crossed(const MatchResult& r) { return 8 + (int64_t)r.n_pairs * 8; }
void copy_pairs(const MatchResult& r, int32_t cap, int32_t* pairs_out) { if (cap > 0) memcpy(pairs_out, r.pairs, (size_t)std::min(r.n_pairs, cap) * 8); }

// One entry of the match phase: a winner's row of its database against a current side on the device; `r` holds until `stage` is used again
struct MatchEntry {
  const ssx_kf_database* db; KfRow row; const uint8_t* cur_desc; const int32_t* cur_cls; int n_cur; int tag;   // (tag: the caller's, its job)
  int32_t* out = nullptr; MatchResult r{0, -1, nullptr};
};

// MatchFeatures of n entries: two launches, one synchronisation.  The scratch in `io` (its contents are dropped), table and results in `stage`.
hipError_t match_phase(ssx_ctx* ctx, DevBuf& io, HostBuf& stage, MatchEntry* e, int n, KfChainStats& st)
{
  KfMatchJob* mt;
  auto pinned = [&](auto&& g) { g(mt, sizeof(KfMatchJob) * (size_t)n); for (int k = 0; k < n; ++k) g(e[k].out, match_out_bytes(e[k].row.n_desc)); };
  hipError_t err = stage.reserve(carve(nullptr, pinned));
  if (err != hipSuccess) return err;
  char* hp = stage.as<char>();
  carve(hp, pinned);
  void* dp = nullptr;
  if ((err = hipHostGetDevicePointer(&dp, hp, 0)) != hipSuccess) return err;
  auto on_device = [&](void* host) { return (char*)dp + ((char*)host - hp); };
  int max_nl = 0;
  for (int k = 0; k < n; ++k) {
    mt[k] = match_job(e[k].db, e[k].row, e[k].cur_desc, e[k].cur_cls, e[k].n_cur);
    match_out_preset(e[k].out);
    mt[k].hdr = (int32_t*)on_device(e[k].out); mt[k].pairs = mt[k].hdr + kMatchPairsOff / 4;
    max_nl = std::max(max_nl, mt[k].nl);
  }
  auto scratch = [&](auto&& g) { for (int k = 0; k < n; ++k) match_scratch(g, mt[k]); };
  if ((err = io.reserve(carve(nullptr, scratch))) != hipSuccess) return err;
  carve(io.as<char>(), scratch);
  // (one entry: it travels as a kernel argument, and no workgroup reads host memory for it)
  err = launch_match_jobs(ctx, n > 1 ? (const KfMatchJob*)on_device(mt) : nullptr, mt[0], n, max_nl);
  if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
  if (err != hipSuccess) return err;
  st.launches += 2; ++st.syncs;
  for (int k = 0; k < n; ++k) { e[k].r = match_out_read(e[k].out); st.bytes_down += match_out_crossed(e[k].r); }
  return hipSuccess;
}

// A query's result block `hh` (`ran`: k_kfdb_topk wrote it) and its K match results in the mapped output `ho` into *res and pairs_out, against
// the host mirror of its database.  SSX_ERR_CAPACITY: some candidate has more than pairs_cap pairs (every count true, the first pairs_cap written).
ssx_status reloc_result(const ssx_kf_database* db, const char* who, int job, const RelocDev& hh, bool ran, int K, const char* ho, size_t out_stride, int32_t pairs_cap,
                        int32_t* pairs_out, ssx_reloc_query_result* res, KfChainStats& st)
{
  ssx_ctx* ctx = db->ctx;
  const int n_db = (int)db->ids.size();
  res->n_pyramid = hh.h.n_pyr; res->n_bow = hh.h.n_bow;
  const int n_cand = ran ? std::min(std::max(hh.n_cand, 0), K) : 0;
  res->n_candidates = n_cand;
  int over = -1;
  for (int k = 0; k < n_cand; ++k) {
    ssx_reloc_candidate& q = res->cand[k];
    const int row = hh.row[k];
    if (row < 0 || row >= n_db) { ctx->set_error("%s: %scandidate %d names row %d of %d", who, JobTag(job).s, k, row, n_db); return SSX_ERR_HIP; }
    q.row = row; q.kf_id = db->ids[row];
    memcpy(&q.score, &hh.fbits[k], 4);
    q.no_descriptors = db->rows[row].n_desc < 0 ? 1 : 0;
    const MatchResult r = match_out_read((const int32_t*)(ho + out_stride * (size_t)k));
    q.n_pairs = r.n_pairs; q.min_distance = r.min_distance; st.bytes_down += match_out_crossed(r);
    copy_pairs(r, pairs_cap, pairs_out + (size_t)2 * k * pairs_cap);
    if (q.n_pairs > pairs_cap && over < 0) over = k;
  }
  if (over >= 0) {
    ctx->set_error("%s: %scandidate %d has %d pairs but capacity %d", who, JobTag(job).s, over, res->cand[over].n_pairs, pairs_cap);
    return SSX_ERR_CAPACITY;
  }
  return SSX_OK;
}

void report_stats(const KfChainStats& s,int32_t* launches, int32_t* synchronisations, int64_t* bytes_up, int64_t* bytes_down)
{
  if (launches) *launches = s.launches; if (synchronisations) *synchronisations = s.syncs;
  if (bytes_up) *bytes_up = s.bytes_up; if (bytes_down) *bytes_down = s.bytes_down;
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
  db->arena.release(); db->table.release(); db->io.release(); db->pend.release(); db->stage.release();
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
  if (ssx_status st = check_commit(db, "ssx_kfdb_add", -1, kf_id)) return st;
  for (int32_t i = 1; i < n_bow; ++i)
    if (ids[i] <= ids[i - 1]) { ctx->set_error("ssx_kfdb_add: word ids must ascend (entry %d)", i); return SSX_ERR_INVALID_ARG; }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool with_desc = desc != nullptr;
  const size_t bytes = blob_bytes(n_bow, n_desc), n = db->ids.size();
  SSX_HIP_TRY(ctx, grow_for_commit(db, bytes));
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
  commit_mirror(db, kf_id, row, bytes);
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
  // one block, on the device and (pinned) on the host: [values | ids | header] go up, [header | scores] come back
  Layout lay;
  const size_t o_v = lay.take((size_t)n_bow * 8), o_i = lay.take((size_t)n_bow * 4), o_hdr = lay.take(sizeof(StepHdr));
  const size_t in_bytes = lay.off;
  const size_t o_s = lay.take((size_t)n_elig * 8);
  SSX_HIP_TRY(ctx, db->io.reserve(lay.off));
  SSX_HIP_TRY(ctx, db->stage.reserve(lay.off));
  char* hs = db->stage.as<char>();
  char* base = db->io.as<char>();
  memcpy(hs + o_v, vals, (size_t)n_bow * 8);
  memcpy(hs + o_i, ids, (size_t)n_bow * 4);
  StepHdr hdr{0, n_bow, 0};
  memcpy(hs + o_hdr, &hdr, sizeof(StepHdr));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(base, hs, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  KfJobDev one{};
  one.n_elig = n_elig; one.arena = db->arena.as<char>(); one.rows = db->table.p;
  one.p_ids = (int32_t*)(base + o_i); one.p_vals = (double*)(base + o_v); one.scores = (double*)(base + o_s);
  launch_score(ctx, nullptr, one, 1, n_elig, (StepHdr*)(base + o_hdr), n_bow, false);
  SSX_HIP_TRY(ctx, hipGetLastError());
  // the header with the winner's key and, when asked for, the scores right behind it: one copy, one synchronisation
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + o_hdr, base + o_hdr, scores_out ? lay.off - o_hdr : sizeof(StepHdr), hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (scores_out) memcpy(scores_out, hs + o_s, (size_t)n_elig * 8);
  memcpy(&hdr, hs + o_hdr, sizeof(StepHdr));
  uint32_t row = 0; float f = 0.f;
  if (!winner_of(hdr.best, threshold, &row, &f)) return SSX_OK;
  *found = 1;
  if (best_kf_id) *best_kf_id = db->ids[row];
  if (best_score) *best_score = f;
  return SSX_OK;
}

// (the current side is uploaded and the result copied back; a keyframe step matches its pending arrays where they lie: match_phase)
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
  if (row.n_desc < 0) return no_descriptors(ctx, "ssx_kfdb_match_features", -1, "", loop_kf_id);
  if (n_cur > 65535) { ctx->set_error("ssx_kfdb_match_features: more than 65535 current descriptors"); return SSX_ERR_UNSUPPORTED; }
  const int nl = row.n_desc;
  if (nl == 0 || n_cur == 0) return SSX_OK;                   // no match exists: no pairs (the reference dereferences end() here)
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // one block, on the device and (pinned) on the host: [descriptors | class ids] go up, [header | pairs] come back
  uint8_t* d_desc; int32_t* d_cls; int32_t* d_out;
  KfMatchJob t = match_job(db, row, nullptr, nullptr, n_cur);
  auto bufs = [&](auto&& f) { f(d_desc, (size_t)n_cur * 32); f(d_cls, (size_t)n_cur * 4); match_scratch(f, t); f(d_out, match_out_bytes(nl)); };
  const size_t total = carve(nullptr, bufs);
  SSX_HIP_TRY(ctx, db->io.reserve(total));
  SSX_HIP_TRY(ctx, db->stage.reserve(total));
  char* hs = db->stage.as<char>();
  char* base = db->io.as<char>();
  carve(base, bufs);
  const size_t in_bytes = (size_t)((char*)t.idx - base), o_cls = (size_t)((char*)d_cls - base), o_out = (size_t)((char*)d_out - base);
  t.cur_desc = d_desc; t.cur_cls = d_cls; t.hdr = d_out; t.pairs = d_out + kMatchPairsOff / 4;
  memcpy(hs, cur_desc, (size_t)n_cur * 32);
  memcpy(hs + o_cls, cur_class_id, (size_t)n_cur * 4);
  SSX_HIP_TRY(ctx, hipMemcpyAsync(base, hs, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  SSX_HIP_TRY(ctx, launch_match_jobs(ctx, nullptr, t, 1, nl));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + o_out, d_out, kMatchPairsOff + (size_t)std::min(nl, cap) * 8, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const MatchResult r = match_out_read((const int32_t*)(hs + o_out));
  *n_pairs = r.n_pairs;
  if (min_distance) *min_distance = r.min_distance;
  copy_pairs(r, cap, pairs_out);
  if (r.n_pairs > cap) { ctx->set_error("ssx_kfdb_match_features: %d pairs but capacity %d", r.n_pairs, cap); return SSX_ERR_CAPACITY; }
  return SSX_OK;
}

ssx_status ssx_kfdb_process_keyframe(ssx_kf_database* db, ssx_vocabulary* voc, int64_t kf_id, const uint8_t* img, int32_t stride, int32_t rows, int32_t cols,
                                     const ssx_orb_params* prm, int32_t n_features, const ssx_keypoint* features, int32_t pyramid_levels, int32_t min_db_size,
                                     int32_t min_id_gap, float threshold, int32_t pairs_cap, int32_t* pairs_out, ssx_kfdb_step_result* res)
{
  static const char* const who = "ssx_kfdb_process_keyframe";
  if (!db) return SSX_ERR_INVALID_ARG;
  db->pending.valid = false;                                  // a call that fails leaves nothing pending
  db->last = KfChainStats{};
  const FrameArgs fa{img, stride, rows, cols, prm, n_features, features, pyramid_levels, pairs_cap, pairs_out};
  if (!voc || !res || !frame_args_ok(fa)) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = db->ctx;
  if (voc->ctx != ctx) { ctx->set_error("%s: the vocabulary belongs to another context", who); return SSX_ERR_INVALID_ARG; }
  if (ssx_status s = check_pyramid_bound(ctx, who, -1, fa)) return s;
  *res = ssx_kfdb_step_result{};
  res->min_distance = -1;
  const int N = n_features * pyramid_levels;
  // DetectLoop runs when enough keyframes are stored (loopclosing.cpp:48) and scores the prefix that is old enough (:79)
  const bool detect = (int64_t)db->ids.size() > (int64_t)min_db_size;
  const int n_elig = detect ? (int)(std::upper_bound(db->ids.begin(), db->ids.end(), kf_id - (int64_t)min_id_gap) - db->ids.begin()) : 0;
  res->detect_ran = detect ? 1 : 0;
  res->n_scored = n_elig;
  KfChainStats st{}; StepHdr hdr{0, 0, 0}; PendArrays pa{};
  if (N > 0) {
    SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ssxorb::Described d;
    if (ssx_status s = ssxorb::describe_enqueue(ctx, img, stride, rows, cols, *prm, features, n_features, pyramid_levels, &d)) return s;
    st.launches += d.launches; st.syncs += d.syncs; st.bytes_up += (int64_t)d.bytes_up;
    SSX_HIP_TRY(ctx, db->pend.reserve(pend_arrays(nullptr, N, pa)));
    pend_arrays(db->pend.as<char>(), N, pa);
    KfJobDev one{}; one.n_in = N; one.n_elig = n_elig;
    job_arrays(one, pa, db);
    Chain c; c.n = 1; c.jobs = &one; c.kps = d.kps; c.desc = d.desc; c.keep = d.keep; c.bound = N;
    SSX_HIP_TRY(ctx, chain_reserve(db->io, db->stage, c, sizeof(StepHdr), nothing_more));
    SSX_HIP_TRY(ctx, chain_enqueue(ctx, voc, db->stage, c, &hdr, st));
  }
  res->n_pyramid = hdr.n_pyr; res->n_bow = hdr.n_bow;
  MatchEntry m{db, KfRow{}, pa.desc, pa.cls, hdr.n_pyr, 0};
  bool match = false;
  if (ssx_status s = step_verdict(db, who, -1, hdr, n_elig > 0, threshold, res, &m.row, &match)) return s;
  if (match) {                                                // MatchFeatures: the pending descriptors and class ids are the current side
    SSX_HIP_TRY(ctx, match_phase(ctx, db->io, db->stage, &m, 1, st));
    res->min_distance = m.r.min_distance;
    copy_pairs(m.r, pairs_cap, pairs_out);
  }
  const int n_pairs = res->n_pairs = m.r.n_pairs;
  // every synchronisation has succeeded: the keyframe is pending
  db->pending.valid = true; db->pending.kf_id = kf_id; db->pending.cap = N; db->pending.n_pyr = hdr.n_pyr; db->pending.n_bow = hdr.n_bow;
  db->last = st;
  if (n_pairs > pairs_cap) { ctx->set_error("%s: %d pairs but capacity %d", who, n_pairs, pairs_cap); return SSX_ERR_CAPACITY; }
  return SSX_OK;
}

ssx_status ssx_kfdb_add_pending(ssx_kf_database* db)
{
  if (!db) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = db->ctx;
  if (!db->pending.valid) { ctx->set_error("ssx_kfdb_add_pending: no keyframe is pending"); return SSX_ERR_INVALID_ARG; }
  const ssx_kf_database::Pending pe = db->pending;
  if (ssx_status st = check_commit(db, "ssx_kfdb_add_pending", -1, pe.kf_id)) return st;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t bytes = blob_bytes(pe.n_bow, pe.n_pyr);
  SSX_HIP_TRY(ctx, grow_for_commit(db, bytes));
  KfJobDev one{};
  commit_job(one, db);
  SSX_PROF(ctx, KID_LOOP_COMMIT, hipLaunchKernelGGL(k_kfdb_commit, dim3(commit_blocks(bytes), 1), dim3(256), 0, ctx->stream, (const KfJobDev*)nullptr, one));
  SSX_HIP_TRY(ctx, hipGetLastError());
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  commit_mirror(db, pe.kf_id, KfRow{one.c_off, pe.n_bow, pe.n_pyr}, bytes);
  db->pending.valid = false;                                  // a keyframe is committed once
  return SSX_OK;
}

ssx_status ssx_kfdb_pending(ssx_kf_database* db, int64_t* kf_id, int32_t kps_cap, ssx_keypoint* kps_out, uint8_t* desc_out, int32_t* class_id_out,
                            int32_t* n_pyramid, int32_t bow_cap, int32_t* ids_out, double* vals_out, int32_t* n_bow)
{
  if (!db || kps_cap < 0 || bow_cap < 0) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = db->ctx;
  if (!db->pending.valid) { ctx->set_error("ssx_kfdb_pending: no keyframe is pending"); return SSX_ERR_INVALID_ARG; }
  const ssx_kf_database::Pending pe = db->pending;
  if (kf_id) *kf_id = pe.kf_id;
  if (n_pyramid) *n_pyramid = pe.n_pyr;
  if (n_bow) *n_bow = pe.n_bow;
  const bool want_kps = kps_out || desc_out || class_id_out, want_bow = ids_out || vals_out;
  if ((want_kps && kps_cap < pe.n_pyr) || (want_bow && bow_cap < pe.n_bow)) {
    ctx->set_error("ssx_kfdb_pending: %d keypoints and %d words but capacities %d and %d", pe.n_pyr, pe.n_bow, kps_cap, bow_cap);
    return SSX_ERR_CAPACITY;
  }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  PendArrays pa{};
  pend_arrays(db->pend.as<char>(), pe.cap, pa);
  hipStream_t s = ctx->stream;
  if (pe.n_pyr > 0) {
    if (kps_out) SSX_HIP_TRY(ctx, hipMemcpyAsync(kps_out, pa.kps, sizeof(ssx_keypoint) * (size_t)pe.n_pyr, hipMemcpyDeviceToHost, s));
    if (desc_out) SSX_HIP_TRY(ctx, hipMemcpyAsync(desc_out, pa.desc, (size_t)32 * pe.n_pyr, hipMemcpyDeviceToHost, s));
    if (class_id_out) SSX_HIP_TRY(ctx, hipMemcpyAsync(class_id_out, pa.cls, (size_t)4 * pe.n_pyr, hipMemcpyDeviceToHost, s));
  }
  if (pe.n_bow > 0) {
    if (ids_out) SSX_HIP_TRY(ctx, hipMemcpyAsync(ids_out, pa.ids, (size_t)4 * pe.n_bow, hipMemcpyDeviceToHost, s));
    if (vals_out) SSX_HIP_TRY(ctx, hipMemcpyAsync(vals_out, pa.vals, (size_t)8 * pe.n_bow, hipMemcpyDeviceToHost, s));
  }
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  return SSX_OK;
}

// The candidate query of relocalisation: the chain with n = 1 over EVERY stored keyframe -> k_kfdb_topk (the candidates and their match
// jobs, on the device) -> k_bf_match_jobs + k_kfdb_pairs with one job per candidate slot, then ONE synchronisation.  The match grid and
// the scratch are sized by the host mirror's largest n_desc, so nothing has to come down before the match is enqueued; a job without a
// candidate exits.  The frame's compacted arrays live in db->io, never in db->pend.
ssx_status ssx_kfdb_relocalize_query(ssx_kf_database* db, ssx_vocabulary* voc, const uint8_t* img, int32_t stride, int32_t rows, int32_t cols,
                                     const ssx_orb_params* prm, int32_t n_features, const ssx_keypoint* features, int32_t pyramid_levels, int32_t max_candidates,
                                     float threshold, float ratio, int32_t pairs_cap, int32_t* pairs_out, ssx_reloc_query_result* res)
{
  static const char* const who = "ssx_kfdb_relocalize_query";
  const FrameArgs fa{img, stride, rows, cols, prm, n_features, features, pyramid_levels, pairs_cap, pairs_out};
  if (!db || !voc || !res || !frame_args_ok(fa) || max_candidates < 1 || max_candidates > kTopK || !std::isfinite(ratio) || ratio < 0.f || ratio > 1.f ||
      !(threshold >= 0.f))
    return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = db->ctx;
  if (voc->ctx != ctx) { ctx->set_error("%s: the vocabulary belongs to another context", who); return SSX_ERR_INVALID_ARG; }
  if (ssx_status s = check_pyramid_bound(ctx, who, -1, fa)) return s;
  db->last = KfChainStats{};
  *res = ssx_reloc_query_result{};
  for (int c = 0; c < kTopK; ++c) { res->cand[c].kf_id = -1; res->cand[c].row = -1; res->cand[c].min_distance = -1; }
  const int N = n_features * pyramid_levels, K = max_candidates, n_db = (int)db->ids.size();
  res->n_scored = n_db;
  if (N == 0) return SSX_OK;
  int max_nl = 0;
  for (const KfRow& r : db->rows) max_nl = std::max(max_nl, r.n_desc);
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  KfChainStats st{};
  ssxorb::Described d;
  if (ssx_status s = ssxorb::describe_enqueue(ctx, img, stride, rows, cols, *prm, features, n_features, pyramid_levels, &d)) return s;
  st.launches += d.launches; st.syncs += d.syncs; st.bytes_up += (int64_t)d.bytes_up;
  // the device scratch: the chain's with the result block as its header, then the frame's compacted arrays, the match table and its jobs' scratch
  static_assert(offsetof(RelocDev, h) == 0, "the chain's kernels take the result block for a step header");
  const size_t keys_stride = sort_scratch_bytes(max_nl) / 8;
  PendArrays pa{}; KfMatchJob* jobs; RelocMatch mb{}; char* frame;
  KfJobDev one{}; one.n_in = N; one.n_elig = n_db;
  Chain c; c.n = 1; c.jobs = &one; c.kps = d.kps; c.desc = d.desc; c.keep = d.keep; c.bound = N;
  SSX_HIP_TRY(ctx, chain_reserve(db->io, db->stage, c, sizeof(RelocDev), [&](auto&& f) {
    f(frame, pend_arrays(nullptr, N, pa)); f(jobs, sizeof(KfMatchJob) * (size_t)K);
    f(mb.idx, (size_t)4 * K * max_nl); f(mb.dist, (size_t)4 * K * max_nl); f(mb.keys, (size_t)8 * K * keys_stride);
  }));
  RelocDev* dh = reinterpret_cast<RelocDev*>(c.hdr);
  pend_arrays(frame, N, pa); job_arrays(one, pa, db);
  // the mapped pinned block: [the result block's copy | a match result per candidate slot, each for max_nl pairs]
  const size_t out_stride = (match_out_bytes(max_nl) + 255) & ~size_t(255);
  RelocDev* hh; char* ho;
  auto pinned = [&](auto&& f) { f(hh, sizeof(RelocDev)); f(ho, out_stride * (size_t)K); };
  SSX_HIP_TRY(ctx, db->stage.reserve(carve(nullptr, pinned)));
  char* hs = db->stage.as<char>();
  carve(hs, pinned);
  for (int k = 0; k < K; ++k) match_out_preset((int32_t*)(ho + out_stride * (size_t)k));
  void* dp = nullptr;
  SSX_HIP_TRY(ctx, hipHostGetDevicePointer(&dp, hs, 0));
  mb.cur_desc = pa.desc; mb.cur_cls = pa.cls; mb.max_nl = max_nl; mb.keys_stride = keys_stride;
  if (keys_stride == 0) mb.keys = nullptr;
  mb.out = (char*)dp + (ho - hs); mb.out_stride = out_stride;
  hipStream_t s = ctx->stream;
  SSX_HIP_TRY(ctx, chain_enqueue(ctx, voc, db->stage, c, nullptr, st));
  if (n_db > 0) {
    SSX_PROF(ctx, KID_LOOP_TOPK, hipLaunchKernelGGL(k_kfdb_topk, dim3(1), dim3(kPairsThreads), 0, s, (const KfJobDev*)nullptr, one, (const RelocMatch*)nullptr, mb, K,
                                                    threshold, ratio, dh, (const StepHdr*)nullptr, jobs));
    SSX_HIP_TRY(ctx, hipGetLastError());
    ++st.launches;
    if (max_nl > 0) {                                         // (else no stored keyframe has a descriptor: nothing can match)
      SSX_HIP_TRY(ctx, launch_match_jobs(ctx, jobs, KfMatchJob{}, K, max_nl));
      st.launches += 2;
    }
  }
  // (n_db == 0: k_kfdb_topk did not run and n_cand, row and fbits of the block are not written; the host does not read them then)
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hh, dh, sizeof(RelocDev), hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  ++st.syncs; st.bytes_down += (int64_t)sizeof(RelocDev);
  const ssx_status rs = reloc_result(db, who, -1, *hh, n_db > 0, K, ho, out_stride, pairs_cap, pairs_out, res, st);
  if (rs != SSX_ERR_HIP) db->last = st;
  return rs;
}

// The candidate query for one frame of each of n databases of one context (the lost streams of a batched cohort) as ONE enqueue: the
// chain over a job table as ssx_kfdb_process_keyframe_batch issues it -- a job's commit of its pending keyframe inside it, so that the
// keyframe is scored and matched like any stored one -- into scratch of the call (voc->io: no database's pending arrays are written),
// k_kfdb_topk with a workgroup per job, the match kernels once over the n x max_candidates table it filled, ONE copy of the n result
// blocks and ONE synchronisation.  Each job's scratch and its slice of the mapped output are sized by its own host mirror's largest
// n_desc (the keyframe it commits included), the match grid by the largest of all.
ssx_status ssx_kfdb_relocalize_query_batch(ssx_vocabulary* voc, int32_t n, const ssx_reloc_query_job* jobs, int32_t rows, int32_t cols, const ssx_orb_params* prm,
                                           int32_t pyramid_levels, int32_t max_candidates, float threshold, float ratio, int32_t images_on_device)
{
  static const char* const who = "ssx_kfdb_relocalize_query_batch";
  if (n < 0) return SSX_ERR_INVALID_ARG;
  if (n == 0) return SSX_OK;
  if (!voc || !jobs || !prm || rows <= 0 || cols <= 0 || pyramid_levels < 1 || pyramid_levels > ssxorb::MAX_LEVELS || max_candidates < 1 || max_candidates > kTopK ||
      !std::isfinite(ratio) || ratio < 0.f || ratio > 1.f || !(threshold >= 0.f))
    return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = voc->ctx;
  const int K = max_candidates;
  // ---- nothing is touched before every job has passed ----
  std::vector<const ssx_kf_database*> seen;
  for (int j = 0; j < n; ++j) {
    const ssx_reloc_query_job& q = jobs[j];
    const FrameArgs fa{q.img, q.stride, rows, cols, prm, q.n_features, q.features, pyramid_levels, q.pairs_cap, q.pairs_out};
    if (!q.db || !q.res || !q.status_out || !frame_args_ok(fa)) {
      ctx->set_error("%s: job %d: a missing database / result / status / image / array, a stride below the width or a negative count", who, j);
      return SSX_ERR_INVALID_ARG;
    }
    if (q.db->ctx != ctx) { ctx->set_error("%s: job %d: the database and the vocabulary belong to different contexts", who, j); return SSX_ERR_INVALID_ARG; }
    if (q.stride != jobs[0].stride) { ctx->set_error("%s: the images of a call share one stride", who); return SSX_ERR_INVALID_ARG; }
    if (std::find(seen.begin(), seen.end(), q.db) != seen.end()) { ctx->set_error("%s: job %d names the database of an earlier job", who, j); return SSX_ERR_INVALID_ARG; }
    seen.push_back(q.db);
    if (ssx_status s = check_pyramid_bound(ctx, who, j, fa)) return s;
    if (q.commit_pending) {
      if (!q.db->pending.valid) { ctx->set_error("%s: job %d: commit_pending but no keyframe is pending", who, j); return SSX_ERR_INVALID_ARG; }
      if (ssx_status s = check_commit(q.db, who, j, q.db->pending.kf_id)) return s;
    }
  }
  if ((int64_t)n * K > 65535) { ctx->set_error("%s: %d jobs x %d candidates: more than 65535 match jobs", who, n, K); return SSX_ERR_UNSUPPORTED; }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  KfChainStats st{};
  ctx->kf_batch = st;
  // ---- what every job is, as if its commit had happened ----
  struct Job { ssx_kf_database::Pending pe; bool commit; int N, n_db, max_nl; size_t blob, keys_stride, out_stride; char* out; };
  std::vector<Job> J(n);
  int max_N = 0, max_nl = 0;
  for (int j = 0; j < n; ++j) {
    const ssx_reloc_query_job& q = jobs[j];
    ssx_kf_database* db = q.db;
    Job& a = J[j];
    a.commit = q.commit_pending != 0; a.pe = db->pending; a.N = q.n_features * pyramid_levels;
    a.blob = a.commit ? blob_bytes(a.pe.n_bow, a.pe.n_pyr) : 0;
    a.n_db = (int)db->ids.size() + (a.commit ? 1 : 0);
    a.max_nl = a.commit ? a.pe.n_pyr : 0;
    for (const KfRow& r : db->rows) a.max_nl = std::max(a.max_nl, r.n_desc);
    a.keys_stride = sort_scratch_bytes(a.max_nl) / 8;
    a.out_stride = (match_out_bytes(a.max_nl) + 255) & ~size_t(255);
    max_N = std::max(max_N, a.N); max_nl = std::max(max_nl, a.max_nl);
    if (a.commit) {                                           // the growth a commit needs, with its own synchronisation as in ssx_kfdb_add_pending
      int moved = 0;
      SSX_HIP_TRY(ctx, grow_for_commit(db, a.blob, &moved));
      st.syncs += moved;
    }
  }
  // ---- the describe block (the job table and the jobs' RelocMatch at its head), the scratch, the pinned block: every allocation before the first enqueue ----
  std::vector<ssxorb::DescribeJob> dj(n);
  for (int j = 0; j < n; ++j) dj[j] = ssxorb::DescribeJob{jobs[j].img, jobs[j].features, jobs[j].n_features};
  ssxorb::DescribedBatch d;
  static_assert(sizeof(KfJobDev) % 8 == 0, "the RelocMatch table follows the job table");
  const size_t o_mb = sizeof(KfJobDev) * (size_t)n;
  if (ssx_status s = ssxorb::describe_batch_prepare(ctx, n, dj.data(), jobs[0].stride, rows, cols, *prm, pyramid_levels, images_on_device != 0,
                                                    o_mb + sizeof(RelocMatch) * (size_t)n, &d))
    return s;
  st.syncs += d.syncs;
  KfJobDev* tab = reinterpret_cast<KfJobDev*>(d.host_extra);
  RelocMatch* mbs = reinterpret_cast<RelocMatch*>(d.host_extra + o_mb);
  for (int j = 0, kp0 = 0; j < n; kp0 += J[j].N, ++j) {
    tab[j] = KfJobDev{}; mbs[j] = RelocMatch{};
    tab[j].kp0 = kp0; tab[j].n_in = J[j].N; tab[j].n_elig = J[j].N > 0 ? J[j].n_db : 0;   // (no features: nothing is scored, no candidate)
  }
  Chain c; c.n = n; c.jobs = tab; c.dev_jobs = reinterpret_cast<const KfJobDev*>(d.dev_extra); c.bound = max_N;
  RelocDev* dh; KfMatchJob* mt; std::vector<char*> frame(n);
  SSX_HIP_TRY(ctx, chain_reserve(voc->io, voc->stage, c, sizeof(StepHdr) * (size_t)n, [&](auto&& f) {
    f(dh, sizeof(RelocDev) * (size_t)n); f(mt, sizeof(KfMatchJob) * (size_t)n * K);
    for (int j = 0; j < n; ++j) {
      PendArrays pa{};
      f(frame[j], pend_arrays(nullptr, J[j].N, pa));
      f(mbs[j].idx, (size_t)4 * K * J[j].max_nl); f(mbs[j].dist, (size_t)4 * K * J[j].max_nl); f(mbs[j].keys, (size_t)8 * K * J[j].keys_stride);
    }
  }));
  // the mapped pinned block: [the n result blocks' copy | per job: a match result per candidate slot, each for the job's max_nl pairs]
  RelocDev* hh;
  auto pinned = [&](auto&& f) { f(hh, sizeof(RelocDev) * (size_t)n); for (int j = 0; j < n; ++j) f(J[j].out, J[j].out_stride * (size_t)K); };
  SSX_HIP_TRY(ctx, voc->stage.reserve(carve(nullptr, pinned)));
  char* hs = voc->stage.as<char>();
  carve(hs, pinned);
  void* dp = nullptr;
  SSX_HIP_TRY(ctx, hipHostGetDevicePointer(&dp, hs, 0));
  for (int j = 0; j < n; ++j) {
    const ssx_reloc_query_job& q = jobs[j];
    const Job& a = J[j];
    if (a.commit) commit_job(tab[j], q.db);
    PendArrays pa{};
    pend_arrays(frame[j], a.N, pa); job_arrays(tab[j], pa, q.db);
    RelocMatch& mb = mbs[j];
    mb.cur_desc = pa.desc; mb.cur_cls = pa.cls; mb.max_nl = a.max_nl; mb.keys_stride = a.keys_stride;
    if (a.keys_stride == 0) mb.keys = nullptr;
    mb.out = (char*)dp + (a.out - hs); mb.out_stride = a.out_stride;
    for (int k = 0; k < K; ++k) match_out_preset((int32_t*)(a.out + a.out_stride * (size_t)k));
    *q.res = ssx_reloc_query_result{};
    for (int k = 0; k < kTopK; ++k) { q.res->cand[k].kf_id = -1; q.res->cand[k].row = -1; q.res->cand[k].min_distance = -1; }
    q.res->n_scored = a.n_db;
    *q.status_out = SSX_OK;
  }
  // ---- one enqueue for all jobs, one copy, one synchronisation ----
  hipStream_t s = ctx->stream;
  if (ssx_status e = ssxorb::describe_batch_launch(ctx, n, c.dev_jobs, max_N, &d)) return e;
  st.launches += d.launches; st.bytes_up += (int64_t)d.bytes_up;
  c.kps = d.kps; c.desc = d.desc; c.keep = d.keep;
  SSX_HIP_TRY(ctx, chain_enqueue(ctx, voc, voc->stage, c, nullptr, st));
  SSX_PROF(ctx, KID_LOOP_TOPK, hipLaunchKernelGGL(k_kfdb_topk, dim3(n), dim3(kPairsThreads), 0, s, c.dev_jobs, KfJobDev{}, reinterpret_cast<const RelocMatch*>(d.dev_extra + o_mb),
                                                  RelocMatch{}, K, threshold, ratio, dh, c.hdr, mt));
  SSX_HIP_TRY(ctx, hipGetLastError());
  ++st.launches;
  if (max_nl > 0) {                                           // (else no keyframe of any job has a descriptor: nothing can match)
    SSX_HIP_TRY(ctx, launch_match_jobs(ctx, mt, KfMatchJob{}, n * K, max_nl));
    st.launches += 2;
  }
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hh, dh, sizeof(RelocDev) * (size_t)n, hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  ++st.syncs; st.bytes_down += (int64_t)(sizeof(RelocDev) * (size_t)n);
  // ---- the commits have happened: the host mirrors follow, and nothing is pending there ----
  for (int j = 0; j < n; ++j)
    if (J[j].commit) {
      commit_mirror(jobs[j].db, J[j].pe.kf_id, KfRow{tab[j].c_off, J[j].pe.n_bow, J[j].pe.n_pyr}, J[j].blob);
      jobs[j].db->pending.valid = false;
    }
  ssx_status first = SSX_OK;
  for (int j = 0; j < n; ++j) {
    const ssx_reloc_query_job& q = jobs[j];
    const ssx_status rs = reloc_result(q.db, who, j, hh[j], true, K, J[j].out, J[j].out_stride, q.pairs_cap, q.pairs_out, q.res, st);
    *q.status_out = rs;
    if (rs != SSX_OK && first == SSX_OK) first = rs;
  }
  ctx->kf_batch = st;
  return first;
}

// The keyframe steps of n databases of one context as ONE enqueue of the chain (and the job-indexed kernels of orb.hip / voc.hip /
// stereo.hip): validate everything, grow what the commits need, enqueue phase 1 for all jobs, one synchronisation, and phase 2 (match and
// pairs of the found jobs) behind a second one.  The host mirrors of the databases change only after the first synchronisation succeeded.
ssx_status ssx_kfdb_process_keyframe_batch(ssx_vocabulary* voc, int32_t n, const ssx_kfdb_step_job* jobs, int32_t rows, int32_t cols, const ssx_orb_params* prm,
                                           int32_t pyramid_levels, int32_t min_db_size, int32_t min_id_gap, float threshold, int32_t images_on_device)
{
  static const char* const who = "ssx_kfdb_process_keyframe_batch";
  if (n < 0) return SSX_ERR_INVALID_ARG;
  if (n == 0) return SSX_OK;
  if (!voc || !jobs || !prm || rows <= 0 || cols <= 0 || pyramid_levels < 1 || pyramid_levels > ssxorb::MAX_LEVELS) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = voc->ctx;
  // ---- nothing is touched before every job has passed ----
  std::vector<const ssx_kf_database*> seen;
  for (int j = 0; j < n; ++j) {
    const ssx_kfdb_step_job& q = jobs[j];
    const FrameArgs fa{q.img, q.stride, rows, cols, prm, q.n_features, q.features, pyramid_levels, q.pairs_cap, q.pairs_out};
    if (!q.db || !q.res || !q.status_out || !frame_args_ok(fa)) {
      ctx->set_error("%s: job %d: a missing database / result / status / image / array, a stride below the width or a negative count", who, j);
      return SSX_ERR_INVALID_ARG;
    }
    if (q.db->ctx != ctx) { ctx->set_error("%s: job %d: the database and the vocabulary belong to different contexts", who, j); return SSX_ERR_INVALID_ARG; }
    if (q.stride != jobs[0].stride) { ctx->set_error("%s: the images of a call share one stride", who); return SSX_ERR_INVALID_ARG; }
    if (std::find(seen.begin(), seen.end(), q.db) != seen.end()) { ctx->set_error("%s: job %d names the database of an earlier job", who, j); return SSX_ERR_INVALID_ARG; }
    seen.push_back(q.db);
    if (ssx_status s = check_pyramid_bound(ctx, who, j, fa)) return s;
    if (q.commit_pending) {
      if (!q.db->pending.valid) { ctx->set_error("%s: job %d: commit_pending but no keyframe is pending", who, j); return SSX_ERR_INVALID_ARG; }
      if (ssx_status s = check_commit(q.db, who, j, q.db->pending.kf_id)) return s;
    }
  }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  KfChainStats st{};
  ctx->kf_batch = st;
  // ---- what every job is, as if its commit had happened ----
  struct Job { ssx_kf_database::Pending pe; bool commit; int N, n_elig; size_t blob; bool detect; };
  std::vector<Job> J(n);
  int max_N = 0;
  for (int j = 0; j < n; ++j) {
    const ssx_kfdb_step_job& q = jobs[j];
    ssx_kf_database* db = q.db;
    Job& a = J[j];
    a.commit = q.commit_pending != 0; a.pe = db->pending; a.N = q.n_features * pyramid_levels;
    a.blob = a.commit ? blob_bytes(a.pe.n_bow, a.pe.n_pyr) : 0;
    const size_t stored = db->ids.size() + (a.commit ? 1 : 0);
    a.detect = (int64_t)stored > (int64_t)min_db_size;       // loopclosing.cpp:48
    const int64_t newest = q.kf_id - (int64_t)min_id_gap;    // the prefix that is old enough (:79); the committed keyframe is the last of the map
    a.n_elig = a.detect ? (int)(std::upper_bound(db->ids.begin(), db->ids.end(), newest) - db->ids.begin()) + ((a.commit && a.pe.kf_id <= newest) ? 1 : 0) : 0;
    max_N = std::max(max_N, a.N);
    if (a.commit) {                                           // the growth a commit needs, with its own synchronisation as in ssx_kfdb_add_pending
      int moved = 0;                                          // (counted: the batch's synchronisations stay exact)
      SSX_HIP_TRY(ctx, grow_for_commit(db, a.blob, &moved));
      st.syncs += moved;
    }
  }
  // ---- the describe block (the job table at its head), the scratch, the pending buffers: every allocation before the first enqueue ----
  std::vector<ssxorb::DescribeJob> dj(n);
  for (int j = 0; j < n; ++j) dj[j] = ssxorb::DescribeJob{jobs[j].img, jobs[j].features, jobs[j].n_features};
  ssxorb::DescribedBatch d;
  if (ssx_status s = ssxorb::describe_batch_prepare(ctx, n, dj.data(), jobs[0].stride, rows, cols, *prm, pyramid_levels, images_on_device != 0,
                                                    sizeof(KfJobDev) * (size_t)n, &d))
    return s;
  st.syncs += d.syncs;
  KfJobDev* tab = reinterpret_cast<KfJobDev*>(d.host_extra);
  for (int j = 0, kp0 = 0; j < n; kp0 += J[j].N, ++j) {
    tab[j] = KfJobDev{};
    tab[j].kp0 = kp0; tab[j].n_in = J[j].N; tab[j].n_elig = J[j].N > 0 ? J[j].n_elig : 0;
  }
  Chain c; c.n = n; c.jobs = tab; c.dev_jobs = reinterpret_cast<const KfJobDev*>(d.dev_extra); c.bound = max_N;
  SSX_HIP_TRY(ctx, chain_reserve(voc->io, voc->stage, c, sizeof(StepHdr) * (size_t)n, nothing_more));
  // A job that commits reads its previous pending arrays in the chain below: a buffer that has to grow is replaced, and the old one is
  // freed only after the synchronisation (DevBuf::reserve would free it now)
  struct Retired { std::vector<void*> p; ~Retired() { for (void* q : p) (void)hipFree(q); } } retired;
  // from here on the databases are touched: whatever way the call fails, nothing is left pending
  struct DropPending {
    const ssx_kfdb_step_job* jobs; int n; bool armed;
    ~DropPending() { if (armed) for (int j = 0; j < n; ++j) jobs[j].db->pending.valid = false; }
  } drop{jobs, n, true};
  for (int j = 0; j < n; ++j) {
    const ssx_kfdb_step_job& q = jobs[j];
    ssx_kf_database* db = q.db;
    const Job& a = J[j];
    if (a.commit) commit_job(tab[j], db);                               // (the arrays where they lie now, before the buffer is replaced)
    PendArrays pa{};
    if (a.N > 0) {
      const size_t need = pend_arrays(nullptr, a.N, pa);
      if (a.commit && need > db->pend.cap) {
        const size_t want = (size_t)((double)need * 1.25) + 256;
        void* np = nullptr;
        SSX_HIP_TRY(ctx, hipMalloc(&np, want));
        if (db->pend.p) retired.p.push_back(db->pend.p);
        db->pend.p = np; db->pend.cap = want;
      } else {
        SSX_HIP_TRY(ctx, db->pend.reserve(need));
      }
      pend_arrays(db->pend.as<char>(), a.N, pa);
    }
    db->pending.valid = false;                                          // a call that fails from here on leaves nothing pending
    db->last = KfChainStats{};
    job_arrays(tab[j], pa, db);
    *q.res = ssx_kfdb_step_result{};
    q.res->min_distance = -1; q.res->detect_ran = a.detect ? 1 : 0; q.res->n_scored = a.n_elig;
    *q.status_out = SSX_OK;
  }
  // ---- phase 1: one enqueue for all jobs ----
  if (ssx_status e = ssxorb::describe_batch_launch(ctx, n, c.dev_jobs, max_N, &d)) return e;
  st.launches += d.launches; st.bytes_up += (int64_t)d.bytes_up;
  c.kps = d.kps; c.desc = d.desc; c.keep = d.keep;
  std::vector<StepHdr> hdr(n);
  SSX_HIP_TRY(ctx, chain_enqueue(ctx, voc, voc->stage, c, hdr.data(), st));
  // ---- the commits have happened: the host mirrors follow ----
  for (int j = 0; j < n; ++j)
    if (J[j].commit) commit_mirror(jobs[j].db, J[j].pe.kf_id, KfRow{tab[j].c_off, J[j].pe.n_bow, J[j].pe.n_pyr}, J[j].blob);
  // ---- DetectLoop's verdicts; the jobs whose winner has something to match go to phase 2 ----
  ssx_status first = SSX_OK;
  auto fail = [&](int j, ssx_status e) { *jobs[j].status_out = e; if (first == SSX_OK) first = e; };
  std::vector<MatchEntry> found;
  for (int j = 0; j < n; ++j) {
    const ssx_kfdb_step_job& q = jobs[j];
    ssx_kf_database* db = q.db;
    q.res->n_pyramid = hdr[j].n_pyr; q.res->n_bow = hdr[j].n_bow;
    MatchEntry m{db, KfRow{}, tab[j].p_desc, tab[j].p_cls, hdr[j].n_pyr, j};
    bool match = false;
    if (ssx_status s = step_verdict(db, who, j, hdr[j], tab[j].n_elig > 0, threshold, q.res, &m.row, &match)) {
      fail(j, s);
      continue;                                               // (nothing pending, as the single call leaves it)
    }
    if (match) found.push_back(m);
    db->pending.valid = true; db->pending.kf_id = q.kf_id; db->pending.cap = J[j].N; db->pending.n_pyr = hdr[j].n_pyr; db->pending.n_bow = hdr[j].n_bow;
  }
  if (!found.empty()) {
    // ---- phase 2: MatchFeatures of the found jobs.  Their table lies in mapped pinned memory and is read from there ----
    const int nf = (int)found.size();
    if (hipError_t e = match_phase(ctx, voc->io, voc->stage, found.data(), nf, st)) {
      ctx->set_error("%s: the match phase failed: %s", who, hipGetErrorString(e));
      return SSX_ERR_HIP;
    }
    st.bytes_up += (int64_t)(sizeof(KfMatchJob) * (size_t)nf);   // (nf == 1: as kernel arguments; the single step does not count its one)
    for (const MatchEntry& m : found) {
      const ssx_kfdb_step_job& q = jobs[m.tag];
      q.res->n_pairs = m.r.n_pairs; q.res->min_distance = m.r.min_distance;
      copy_pairs(m.r, q.pairs_cap, q.pairs_out);
      if (m.r.n_pairs > q.pairs_cap) {
        ctx->set_error("%s: job %d: %d pairs but capacity %d", who, m.tag, m.r.n_pairs, q.pairs_cap);
        fail(m.tag, SSX_ERR_CAPACITY);
      }
    }
  }
  ctx->kf_batch = st;
  drop.armed = false;                                         // the call ran: every job's keyframe is pending (but for a winner without descriptors)
  return first;
}

#ifndef SSX_NO_TEST_HOOKS   // include/ssx_test_hooks.h
ssx_status ssx_kfdb_debug_last_batch(ssx_ctx* ctx, int32_t* launches, int32_t* synchronisations, int64_t* bytes_up, int64_t* bytes_down)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  report_stats(ctx->kf_batch, launches, synchronisations, bytes_up, bytes_down);
  return SSX_OK;
}

ssx_status ssx_kfdb_debug_last_step(const ssx_kf_database* db, int32_t* launches, int32_t* synchronisations, int64_t* bytes_up, int64_t* bytes_down)
{
  if (!db) return SSX_ERR_INVALID_ARG;
  report_stats(db->last, launches, synchronisations, bytes_up, bytes_down);
  return SSX_OK;
}

// steps 3-4 of the chain alone, on a caller's descriptors
ssx_status ssx_kfdb_debug_bow(ssx_vocabulary* voc, const uint8_t* desc, int32_t n, int32_t cap, int32_t* ids_out, double* vals_out, int32_t* n_entries)
{
  if (!voc || n < 0 || (n > 0 && !desc) || cap < 0 || (cap > 0 && (!ids_out || !vals_out)) || !n_entries) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = voc->ctx;
  *n_entries = 0;
  if (n == 0) return SSX_OK;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  StepHdr* dh; int32_t* word; double* weight;
  KfJobDev one{}; one.n_in = n;
  // one block, on the device and (pinned) on the host: [descriptors | header: count in, count out] go up, [ids | values] and the header come back
  auto bufs = [&](auto&& f) {
    f(one.p_desc, (size_t)32 * n); f(dh, sizeof(StepHdr)); f(word, (size_t)4 * n); f(weight, (size_t)8 * n); f(one.bow_keys, sort_scratch_bytes(n));
    f(one.p_ids, (size_t)4 * n); f(one.p_vals, (size_t)8 * n);
  };
  const size_t total = carve(nullptr, bufs);
  SSX_HIP_TRY(ctx, voc->io.reserve(total));
  SSX_HIP_TRY(ctx, voc->stage.reserve(total));
  char* base = voc->io.as<char>();
  carve(base, bufs);
  const size_t o_hdr = (size_t)((char*)dh - base), o_in = (size_t)((char*)word - base), o_ids = (size_t)((char*)one.p_ids - base),
               o_vals = (size_t)((char*)one.p_vals - base);
  char* hs = voc->stage.as<char>();
  memcpy(hs, desc, (size_t)32 * n);
  StepHdr hdr{n, 0, 0};
  memcpy(hs + o_hdr, &hdr, sizeof(StepHdr));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(base, hs, o_in, hipMemcpyHostToDevice, ctx->stream));
  launch_words_bow(ctx, voc, nullptr, one, 1, n, dh, word, weight);
  SSX_HIP_TRY(ctx, hipGetLastError());
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + o_hdr, dh, sizeof(StepHdr), hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + o_ids, base + o_ids, total - o_ids, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(&hdr, hs + o_hdr, sizeof(StepHdr));
  *n_entries = hdr.n_bow;
  if (hdr.n_bow > cap) { ctx->set_error("ssx_kfdb_debug_bow: %d words but capacity %d", hdr.n_bow, cap); return SSX_ERR_CAPACITY; }
  if (hdr.n_bow > 0) {
    memcpy(ids_out, hs + o_ids, (size_t)4 * hdr.n_bow);
    memcpy(vals_out, hs + o_vals, (size_t)8 * hdr.n_bow);
  }
  return SSX_OK;
}
#endif

}  // extern "C"

#include "loop_guided.inc"   // ssx_kfdb_project_match, ssx_kfdb_guided_search: k_kfdb_project, k_kfdb_claim
