// ssvio_amd/csrc/ba.hip -- local bundle adjustment on gfx950 (ssx_ba_solve / ssx_ba_linearize).
//
// Replaces the arithmetic behind Backend::OptimizeActiveMap (/root/reference/src/ssvio/backend.cpp:78-245):
// g2o's SparseOptimizer + BlockSolver<6,3> + OptimizationAlgorithmLevenberg over ssvio's
// VertexPose / VertexXYZ / EdgeProjection (include/ssvio/g2otypes.hpp).  No g2o, no Eigen: the normal
// equations are built, Schur-reduced, solved and applied by the kernels below, and the LM accept/reject
// logic runs on the device too (lm_step): the host enqueues a whole optimize(iters) and synchronises once.
//
// Data layout in HBM (one arena per ctx, grow-only):
//   edges are SORTED BY LANDMARK (then by pose inside a landmark) on upload so that all observations of
//   a landmark are contiguous; landmarks are grouped into CHUNKS of whole landmarks with <= 255 edges.
//   One 256-thread workgroup (4 waves) owns one chunk in every per-edge / per-landmark kernel, so every
//   per-landmark reduction (Hll, bl, Schur terms, back-substitution) happens in LDS without atomics.
//   Per-edge arrays are structure-of-arrays (W[k][E], uv[2][E] ...) so that lane i touches element i.
//   Two small index lists per chunk are prepared on the host together with the sort:
//     - the chunk's edges grouped by pose           (pose block accumulation walks only its own edges)
//     - the chunk's (edge, edge) pairs grouped by reduced-system block (Schur accumulation likewise)
//
// Determinism: no floating-point atomics anywhere.  Cross-edge sums inside a chunk are done by
// "owned entries" (each thread owns a few output scalars and adds its contributions in list order);
// cross-chunk sums are done by reduction kernels with a fixed tree.  Two runs give identical bits.
//
// Kernels (small-window path, free poses <= SSX_BA_SMALL_P = 16; the local window of ssvio is 12):
//   k_linearize<JAC>      per LM iteration : residuals, Jacobians, Huber weights, W_e = Ji^T w Jj,
//                                            Hll/bl per landmark, Hpp/bp slab per chunk, chi2 slab
//   k_reduce_lin          per LM iteration : slabs -> Hpp, bp, chi2, max|diag| (+ lambda_0)
//   k_schur               per LM trial     : (Hll+lambda I)^-1, W D^-1 W^T and W D^-1 bl slabs per chunk
//   k_reduce_schur        per LM trial     : slabs -> dense reduced system S (without lambda), b_s
//   k_solve               per LM trial     : (S + lambda I) x = b_s by LDL^T, register-tiled over 256 threads
//                                            with the right-hand side carried as an extra row; exp(x) * T
//   k_backsub_residual    per LM trial     : x_l = D^-1 (bl - W^T x_p), new points, new residuals, chi2 slab
//   k_reduce_trial        per LM trial     : slabs -> tempChi, scale, outlier count
//
// Multi-GPU (landmark-sharded): every rank holds all poses and the edges of its
// landmarks; three buffers are sum-all-reduced through the ssx_allreduce_fn hook (RCCL over xGMI when the
// caller wires torch.distributed / rccl to it): [Hpp | bp | chi2 | per-rank max-diagonal slots] once per
// iteration, [S | b_s] once per trial before the (replicated, deterministic) solve, [chi2', scale, #outliers]
// once per trial after the residual pass.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <limits>
#include <map>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <numeric>
#include <thread>
#include <unordered_map>
#include <vector>

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include "ctx.hpp"
#include "se3.hpp"
#include "../../include/ssx_test_hooks.h"

int ssx_comm_allreduce_f64(void* user, double* buf_dev, size_t count, void* stream);   // comm.hip

namespace {

using ssx::Cam;

constexpr int CH = 256;            // threads per chunk workgroup
// (tools/build_variant.py experiments: smaller chunks -> less LDS per workgroup -> more workgroups per CU; profiles/r06/lin_schur_residency.md)
#ifndef SSX_CHUNK_E
#define SSX_CHUNK_E 255
#endif
#ifndef SSX_CHUNK_L
#define SSX_CHUNK_L 128
#endif
#ifndef SSX_LIN_VA
#define SSX_LIN_VA 14
#endif
#ifndef SSX_LS_WGS
#define SSX_LS_WGS 3
#endif
constexpr int CH_E = SSX_CHUNK_E;  // max edges per chunk (chunk-local edge indices fit a byte)
constexpr int PW = CH_E + 2;       // padded (odd) LDS pitch (doubles) of [component][edge] tiles
constexpr int CH_L = SSX_CHUNK_L;  // max landmarks per chunk (per-landmark LDS arrays of k_schur)
constexpr int PL = CH_L + 1;       // their padded pitch
constexpr int SSX_BA_SMALL_P = 16; // free poses handled by the owned-entry (deterministic LDS) path
constexpr int UPPER6 = 21;
constexpr int TOUCH_WORDS = (SSX_BA_SMALL_P * (SSX_BA_SMALL_P + 1) / 2 + SSX_BA_SMALL_P + 31) / 32;   // 5: bits of a chunk's touch mask
constexpr int BSEG_PARTS = 4;      // a block's pair list is cut into at most this many parts (k_schur's block phase) ...
constexpr int BSEG_MIN = 8;        // ... of at least this many pairs
constexpr int MAX_PAIRS = CH_E * (SSX_BA_SMALL_P + 1) / 2 + 8;       // leader pairs of one chunk (sum k(k+1)/2, k <= 16)

// A pointer into device GLOBAL memory as a struct member.  The batched kernels read their window descriptor through a
// reference into a device array, so its pointer members are values LOADED from memory: the compiler cannot know their
// address space and emitted flat_load / flat_store / flat_atomic for every access through them (133 + 53 + 24 in
// k_lin_schur_b) -- and a FLAT access counts on lgkmcnt as well as vmcnt, so every `s_waitcnt lgkmcnt(0)` in front of an LDS
// read also waited for the global loads / stores / atomics in flight.  On the device the member converts to a pointer INTO
// address space 1, so indexing it is a global_* access; code that carries such a pointer around keeps the type (gdouble_p).
template <class T>
struct GPtr {
  T* p;
#if defined(__HIP_DEVICE_COMPILE__)
  using G = __attribute__((address_space(1))) T*;          // device code sees a pointer into the GLOBAL address space
#else
  using G = T*;
#endif
  __host__ __device__ __forceinline__ GPtr& operator=(T* q) { p = q; return *this; }
  __host__ __device__ __forceinline__ operator G() const { return (G)p; }
  __host__ __device__ __forceinline__ G get() const { return (G)p; }
};
#if defined(__HIP_DEVICE_COMPILE__)
using gdouble_p = __attribute__((address_space(1))) double*;
using gcdouble_p = __attribute__((address_space(1))) const double*;
#else
using gdouble_p = double*;
using gcdouble_p = const double*;
#endif


struct BaDev {
  // problem (uploaded once per ssx_ba_solve)
  int P, L, E, nP, nLm, nCh, nBlk, world, rank;
  int big;                  // large-window path (free poses > SSX_BA_SMALL_P): pose blocks / Schur / solve in ba_big.inc
  int store_w;              // 1: k_linearize stores W = Ji^T w Jj (144 B per edge) for the later kernels (large windows, numeric
                            // Jacobians, the linearize hook); 0: small windows with analytic Jacobians RECOMPUTE it where needed --
                            // 150 flops per edge instead of one 144-byte write and two reads
  int lin_stride;           // doubles per chunk in lin_slab: nP*27 + 2 (small) or 2 (big)
  int dense_slabs;          // 1: every chunk writes every entry of its slabs (zeros for blocks / poses it does not touch) and the
                            // reductions read all of them: round 3's traffic, kept as the cross-check of the sparse form (same bits)
  GPtr<unsigned int> touch; // nCh x TOUCH_WORDS: bit b < nBlk = the chunk's landmarks contribute to block b of the reduced system,
                            // bit nBlk + p = the chunk holds edges of free pose p.  A chunk WRITES only those parts of its slabs, the
                            // reductions READ only those (a C3 chunk of 51 landmarks sorted by first keyframe touches 15-25 of the
                            // 55 blocks and 5-7 of the 10 poses)
  GPtr<const int> pose_free;     // P: free index or -1
  GPtr<const uint8_t> lm_fixed;  // nLm (compact landmarks = landmarks that have edges)
  GPtr<const int> lm_id;         // nLm -> original landmark
  GPtr<const int> lm_ptr;        // nLm+1 -> first sorted edge
  GPtr<const int> ch_lm;         // nCh+1 -> first compact landmark
  GPtr<const int> e_pose;        // E (sorted)
  GPtr<const int> e_lmc;         // E compact landmark index
  GPtr<const uint8_t> e_cam;     // E
  GPtr<const uint8_t> e_dup;     // E: 1 = same (landmark,pose) as the previous sorted edge
  GPtr<const double> e_uv;       // [2][E]
  GPtr<const int8_t> blk_pa;     // nBlk upper blocks (pa<=pb) of the reduced system
  GPtr<const int8_t> blk_pb;
  // packed records: ONE 16-byte load per chunk / edge / landmark instead of a chain of dependent index loads
  GPtr<const int4> ch_desc;      // nCh: first sorted edge, #edges, first compact landmark, #landmarks
  GPtr<const int4> e_rec;        // E:   pose, free pose index (-1 fixed), landmark id (caller's), flags: bit0 cam, bit1 dup, bit2 landmark fixed, bit3 next edge is a dup, bit5 pose fixed, bits 8..15 chunk-local landmark, bits 16..23 position in the chunk's pose-major order (edges grouped by free pose, fixed-pose edges last)
  GPtr<const int4> l_rec;        // nLm: chunk-local first edge, #edges, landmark id (caller's), fixed
  GPtr<const uint16_t> pptr;     // nCh x (nP+1): segment of each pose inside the chunk's pose-major order
  // (the pair lists and the work items are built by the host marshalling OR, the default, by k_build_lists on the device:
  // the arrays are then scratch with a fixed capacity per chunk)
  GPtr<uint8_t> pair_a;          // nPairs: chunk-local leader edge a (pose pa)
  GPtr<uint8_t> pair_b;          // nPairs: chunk-local leader edge b (pose pb)
  GPtr<int> pair_ptr;            // nCh x (nBlk+1): absolute offsets into pair_a/pair_b
  GPtr<int4> bseg;               // work items of k_schur's block phase: (block or -1, first pair, end pair [chunk-relative], part | parts << 4)
  GPtr<int> bseg_ptr;            // nCh x 2: first item of the chunk in bseg, number of items
  int bseg_cap;             // device-built lists: items reserved per chunk (pairs: MAX_PAIRS per chunk)
  // device-side marshalling (HostPrep::dev_prep): the caller's arrays as they came, the host's counting results, and the
  // sorted order the device derives from them
  int dev_prep;
  int E_raw;                      // entries of the caller's edge arrays (== E except for an ssx_ba_window, whose storage keeps the
                                  // observations of removed keyframes as dead entries, edge_point < 0, until it is compacted)
  GPtr<const int> r_edge_pose;    // E_raw, caller's order
  GPtr<const int> r_edge_point;   // E
  GPtr<const double> r_edge_uv;   // E x 2 interleaved
  GPtr<const uint8_t> r_edge_cam; // E or null
  GPtr<const uint8_t> r_slot8;    // E: rank of the edge among its landmark's edges (caller's order)
  int no_err;                     // 1: nobody will ask for per-edge errors (err_lin / err_trial are not written: 32 bytes per edge and LM slot)
  int raw_fmt;                    // how the raw arrays crossed PCIe (lossless): bit 0 = r_edge_pose holds bytes, bit 1 = r_edge_point holds
                                  // 16-bit words, bit 2 = r_edge_uv holds floats (every coordinate was a float's value: keypoints are)
  GPtr<const int> lm_compact;     // L: caller's landmark -> compact landmark or -1
  GPtr<const int> pose_rank;      // P or null: a landmark's edges are ordered by this key instead of the pose index (an ssx_ba_window
                                  // orders its keyframes by the caller's ids, not by the slots they happen to live in)
  GPtr<int> perm;                 // E: sorted edge -> caller's edge
  GPtr<int> lm_chunk;             // nLm: compact landmark -> chunk (large windows, device-marshalled: the pair builder reads it)
  GPtr<double> c2_out;            // E: edge chi2 in the CALLER's order (results of a device-marshalled window)
  Cam K;
  double ext[14];
  double huber_delta, chi2_th;
  // state
  GPtr<double> pose[2];          // [P*7]
  GPtr<double> point[2];         // [L*3]
  GPtr<const double> pose_init;  // batched windows: the uploaded state, kept pristine so that a resident batch can be solved again
  GPtr<const double> point_init;
  // linearisation
  GPtr<double> W;                // [18][E]
  GPtr<double> err_lin;          // [2][E]
  GPtr<double> err_trial;        // [2][E]
  GPtr<double> Hll;              // [6][nLm]
  GPtr<double> bl;               // [3][nLm]
  GPtr<double> lin_slab;         // nCh x (nP*27 + 2)
  GPtr<double> Hpp;              // nP x 21   (this rank's part)
  GPtr<double> bp;               // nP x 6    (this rank's part)
  GPtr<double> iter_comm;        // [Hpp_g nP*21 | bp_g nP*6 | chi2 | maxdiag slots (world)]  all-reduced per iteration
  GPtr<double> schur_slab;       // nCh x (nBlk*36 + nP*6)
  GPtr<double> trial_comm;       // [S n*n | bs n]   all-reduced per trial (n = 6 nP), S without lambda
  GPtr<double> xp;               // n
  GPtr<double> trial_slab;       // nCh x 3
  GPtr<double> scal_comm;        // [tempChi, scale_l, nout]  all-reduced per trial
  GPtr<double> scal;             // SC_N scalars
  GPtr<double> lm_stat;          // device-driven LM: [3][SSX_BA_MAX_STATS] chi2 | lambda | trials per iteration
  GPtr<unsigned int> ticket;     // one word of its own: chunks of k_backsub_residual that have published their sums in this trial
};

// scal[] slots
enum { SC_CHI2_CUR = 0, SC_MAXDIAG = 1, SC_SOLVE_OK = 2, SC_SCALE_P = 3, SC_TEMP_CHI = 4, SC_SCALE_L = 5,
       SC_NOUT = 6, SC_LAMBDA = 7,
       // control block of the device-driven LM loop (small windows): the LM bookkeeping of
       // OptimizationAlgorithmLevenberg::solve runs on the device after every trial, so a whole optimize(iters) is
       // enqueued without a host round trip.  Kernels launched with cur < 0 take the state buffer from SC_CUR and
       // return at once when SC_STOP is set.
       SC_NI = 8, SC_CUR = 9, SC_IT = 10, SC_QMAX = 11, SC_STOP = 12, SC_NEEDLIN = 13, SC_ITERS = 14, SC_NSTAT = 15,
       SC_CURCHI = 16, SC_TRIALS_RUN = 17,
       SC_UNUSED18 = 18,              // (round 5 kept the chunk ticket of k_backsub_residual here, aliased onto a double: BaDev::ticket now)
       SC_N = 32 };

// Workgroup reductions (256 threads), fixed shape, hence deterministic: an xor tree inside each wave, then the four wave
// results in wave order.  `s` needs 16 doubles; two barriers per call (the tree of barriers it replaces took ten).
// Wave-wide reductions on the VALU: a butterfly through DPP inside each row of 16 lanes (quad_perm xor 1, xor 2, row_half_mirror,
// row_mirror: every lane of a row then holds the row's result), then the four rows through v_readlane, in row order.  `__shfl_xor`
// compiles to ds_bpermute_b32 -- two of them per double and step, 12 per wave_sum -- which are LDS-pipeline instructions with an LDS
// round trip each: the fused linearise + Schur kernel spent a fifth of its LDS cycles on them (140 static sites).
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)
{
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
constexpr int DPP_QUAD_XOR1 = 0xB1, DPP_QUAD_XOR2 = 0x4E, DPP_ROW_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;
__device__ __forceinline__ double lane_f64(double v, int lane)
{
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ double wave_sum(double v)
{
  v += dpp_f64<DPP_QUAD_XOR1>(v);
  v += dpp_f64<DPP_QUAD_XOR2>(v);
  v += dpp_f64<DPP_ROW_HALF_MIRROR>(v);
  v += dpp_f64<DPP_ROW_MIRROR>(v);
  return ((lane_f64(v, 0) + lane_f64(v, 16)) + lane_f64(v, 32)) + lane_f64(v, 48);
}
__device__ __forceinline__ double wave_max(double v)
{
  v = fmax(v, dpp_f64<DPP_QUAD_XOR1>(v));
  v = fmax(v, dpp_f64<DPP_QUAD_XOR2>(v));
  v = fmax(v, dpp_f64<DPP_ROW_HALF_MIRROR>(v));
  v = fmax(v, dpp_f64<DPP_ROW_MIRROR>(v));
  return fmax(fmax(lane_f64(v, 0), lane_f64(v, 16)), fmax(lane_f64(v, 32), lane_f64(v, 48)));
}
__device__ __forceinline__ double block_sum_256(double v, double* s)
{
  const int t = threadIdx.x;
  v = wave_sum(v);
  if ((t & 63) == 0) s[t >> 6] = v;
  __syncthreads();
  const double r = ((s[0] + s[1]) + s[2]) + s[3];
  __syncthreads();
  return r;
}
__device__ __forceinline__ double block_max_256(double v, double* s)
{
  const int t = threadIdx.x;
  v = wave_max(v);
  if ((t & 63) == 0) s[t >> 6] = v;
  __syncthreads();
  const double r = fmax(fmax(s[0], s[1]), fmax(s[2], s[3]));
  __syncthreads();
  return r;
}
// a, b, c summed and m maximised over the workgroup in one pass (one pair of barriers)
__device__ __forceinline__ void block_sum3_max_256(double& a, double& b, double& c, double& m, double* s)
{
  const int t = threadIdx.x;
  a = wave_sum(a); b = wave_sum(b); c = wave_sum(c); m = wave_max(m);
  if ((t & 63) == 0) { const int w = t >> 6; s[w] = a; s[4 + w] = b; s[8 + w] = c; s[12 + w] = m; }
  __syncthreads();
  a = ((s[0] + s[1]) + s[2]) + s[3];
  b = ((s[4] + s[5]) + s[6]) + s[7];
  c = ((s[8] + s[9]) + s[10]) + s[11];
  m = fmax(fmax(s[12], s[13]), fmax(s[14], s[15]));
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// k_linearize: residual + Jacobians + quadratic form of every edge of one chunk.
// restates BlockSolver::buildSystem (thirdparty/g2o/g2o/core/block_solver.hpp:463-521) +
// BaseBinaryEdge::constructQuadraticForm (base_binary_edge.hpp:61-134) for EdgeProjection.
// ------------------------------------------------------------------------------------------------
// LDS of the linearisation (carved from the workgroup's dynamic LDS so that the fused k_lin_schur can reuse the same
// bytes for the Schur phase)
constexpr int LIN_VA = SSX_LIN_VA;   // pose-block entries per round: 27 = 14 + 13
// One LDS layout for k_linearize, k_schur and the fused k_lin_schur: [0, BA_PHASE_BYTES) belongs to the running phase
// (linearise: sL 9 x CH + sV 14 x PW doubles; Schur: sY 18 x PW + sG, sGb 9 x PL doubles + sLm CH ints), the lists above
// it (pose segments, pair list) are loaded ONCE at the top of the kernel and survive the change of phase.
constexpr size_t BA_PHASE_LIN = sizeof(double) * (9 * (CH_E + 1) + LIN_VA * PW), BA_PHASE_SCHUR = sizeof(double) * (18 * PW + 9 * PL) + sizeof(int) * (CH_E + 1);
constexpr size_t BA_PHASE_BYTES = ((BA_PHASE_LIN > BA_PHASE_SCHUR ? BA_PHASE_LIN : BA_PHASE_SCHUR) + 63) & ~size_t(63);   // 47 360 at 255 edges
static_assert(SSX_CHUNK_E != 255 || BA_PHASE_BYTES == 47360, "the shipped layout");
constexpr size_t BA_OFF_PPTR = BA_PHASE_BYTES;                                   // uint16 [SSX_BA_SMALL_P + 2]
constexpr size_t BA_OFF_PAB = BA_OFF_PPTR + 64;                                  // uint16 [MAX_PAIRS]
constexpr size_t BA_LDS_BYTES = BA_OFF_PAB + ((2 * MAX_PAIRS + 63) & ~size_t(63));   // 51 776 B: three workgroups per CU
constexpr size_t LIN_LDS_BYTES = BA_LDS_BYTES;
static_assert(2 * (SSX_BA_SMALL_P + 2) <= 64 && SSX_LS_WGS * BA_LDS_BYTES <= 160 * 1024, "LDS budget");

// threadIdx.x behind an opaque move: everything a phase derives from it (LDS row addresses, quarter pointers ...) is then
// recomputed per chunk instead of being hoisted out of a persistent workgroup's chunk loop and kept in ~20 registers
// for its whole life (the fused kernel sits on the 168-register line of three workgroups per CU)
__device__ __forceinline__ int tid_opaque()
{
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// What a chunk's workgroup fetches before it looks at the LM state: nothing here depends on it, and the loads are in
// flight while the state words arrive (the kernel is a chain of dependent global loads: window -> state -> chunk ->
// edge records -> poses / points; every hop taken off the chain is ~1 us per workgroup).
struct ChunkLists {
  int4 cd;          // ch_desc
  int it0, n_items; // work items of the Schur block phase (BaDev::bseg)
  int4 item_rec;    // this lane's first work item
};
__device__ __forceinline__ void chunk_lists_load(const BaDev& d, int c, char* smem, bool want_pairs, ChunkLists& cl)
{
  const int t = tid_opaque();
  uint16_t* sPptr = reinterpret_cast<uint16_t*>(smem + BA_OFF_PPTR);
  uint16_t* sPab = reinterpret_cast<uint16_t*>(smem + BA_OFF_PAB);
  cl.cd = d.ch_desc[c];
  cl.it0 = 0; cl.n_items = 0; cl.item_rec = make_int4(-1, 0, 0, 1 << 4);
  if (d.big) return;
  if (t <= d.nP) sPptr[t] = d.pptr[(size_t)c * (d.nP + 1) + t];
  if (!want_pairs) return;
  cl.it0 = d.bseg_ptr[2 * c];
  cl.n_items = 4 * d.bseg_ptr[2 * c + 1];
  if (t < cl.n_items) cl.item_rec = d.bseg[cl.it0 + (t >> 2)];
  // the chunk's (edge a, edge b) pairs grouped by block: global -> LDS once, coalesced
  const int* gp = d.pair_ptr + (size_t)c * (d.nBlk + 1);
  const int q_base = gp[0], q_end = gp[d.nBlk];
  for (int q = t; q < q_end - q_base; q += CH) sPab[q] = (uint16_t)(d.pair_a[q_base + q] | (d.pair_b[q_base + q] << 8));
}

// the 27 owned entries of a pose (21 upper entries of Hpp, row-major, + 6 of bp): this edge's term of entries
// [K0, K0 + N).  (Ji w) Ji and Ji r in the same association as ever, so that the sums keep their bits.
template <int K0, int N>
__device__ __forceinline__ void pose_terms(const double* Ji, double w, double r0, double r1, double* V)
{
  int k = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int cc = r; cc < 6; ++cc) {
      if (k >= K0 && k < K0 + N) V[k - K0] = Ji[r] * w * Ji[cc] + Ji[6 + r] * w * Ji[6 + cc];
      ++k;
    }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    if (k >= K0 && k < K0 + N) V[k - K0] = Ji[a] * r0 + Ji[6 + a] * r1;
    ++k;
  }
}

// sum of row[s0 .. s1): the chunk's edges of one pose sit next to each other (pose-major positions), so the loads of
// several iterations are in flight together -- the former loop chased an index list with one dependent LDS round trip
// per edge and dominated the kernel (12 000 + 9 600 waiting of 44 000 cycles per workgroup)
__device__ __forceinline__ double run_sum(const double* row, int s0, int s1)
{
  double acc = 0.0;
  int s = s0;
  for (; s < s1; s += 8) {      // the last round reads past the run (inside the row or its neighbour) and adds zeros instead
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = row[s + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += (s + i < s1) ? v[i] : 0.0;
  }
  return acc;
}

// (Round 3 measured workgroups that walk a GROUP of chunks and keep one slab per group -- profiles/r03/persist_ab.md: 6.6x less
// slab traffic, but the kernel lost more than the reductions won; round 4 cuts the traffic the other way: a chunk writes only the
// parts of its slab it contributes to, see BaDev::touch.)
__device__ __forceinline__ bool chunk_touches(const BaDev& d, int c, int bit)
{
  return d.dense_slabs || ((d.touch[(size_t)c * TOUCH_WORDS + (bit >> 5)] >> (bit & 31)) & 1u);
}

// Wout (18, nullable): this thread's edge block W = Ji^T w Jj stays in registers for the caller; lmout (9, nullable):
// this thread's landmark sums (Hll 6 + bl 3).  cur must be >= 0 (the device-driven checks are the wrappers').
// erw_out (nullable): the flag word of this thread's edge record, for the Schur phase of the fused kernel.
template <int JAC>
__device__ __forceinline__ void k_linearize_body(const BaDev& d, const int bx, int cur, char* smem, const ChunkLists& cl, double* Wout, double* lmout,
                                                 int* erw_out, double* slab)
{
  double (*sL)[CH_E + 1] = reinterpret_cast<double (*)[CH_E + 1]>(smem);   // [9]: per-edge landmark contributions (6 Hll + 3 bl), edge order
  double* sV = reinterpret_cast<double*>(smem) + 9 * (CH_E + 1);                // [LIN_VA][PW]: per-edge pose-block terms, POSE-MAJOR order
  double* sRed = reinterpret_cast<double*>(smem);                       // 16 doubles over sL, which is dead by then
  const uint16_t* sPptr = reinterpret_cast<const uint16_t*>(smem + BA_OFF_PPTR);

  const int t = tid_opaque();
  (void)bx;
  const int4 cd = cl.cd;
  const int e0 = cd.x, ne = cd.y, lm0 = cd.z, nl = cd.w;
  const double* pose = d.pose[cur];
  const double* point = d.point[cur];
  const bool small = !d.big;

  double rho0 = 0.0;
  double Ji[12], wq = 0.0, r0 = 0.0, r1 = 0.0;
  int pos = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) Ji[k] = 0.0;
  if (t < ne) {
    const int e = e0 + t;
    const int4 er4 = d.e_rec[e];
    const int p = er4.x, pf = er4.y, lid = er4.z;
    const bool lfree = !(er4.w & 4);
    pos = (er4.w >> 16) & 0xFF;
    if (erw_out) *erw_out = er4.w;
    double T[7], X[3];
#pragma unroll
    for (int k = 0; k < 7; ++k) T[k] = pose[p * 7 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = point[lid * 3 + k];
    const double* ext = d.ext + 7 * (er4.w & 1);
    const double u = d.e_uv[e], v = d.e_uv[d.E + e];
    double er[2], p1[3], pc[3], Jj[6];
    ssx::edge_error(T, X, ext, d.K, u, v, er, p1, pc);
    if (JAC == SSX_JAC_NUMERIC_G2O) ssx::edge_jac_numeric(T, X, ext, d.K, u, v, Ji, Jj);
    else ssx::edge_jac_analytic(T, ext, d.K, p1, pc, Ji, Jj);
    double w;
    ssx::huber(er[0] * er[0] + er[1] * er[1], d.huber_delta, rho0, w);
    if (!d.no_err) {
      d.err_lin[e] = er[0];
      d.err_lin[d.E + e] = er[1];
    }
    // an edge whose vertices are both fixed is not active in g2o (sparse_optimizer.cpp:237): no chi2 term
    if (pf < 0 && !lfree) rho0 = 0.0;
    wq = w; r0 = -er[0] * w; r1 = -er[1] * w;
    // W = Ji^T w Jj  (6x3), only when both vertices are free (block_solver.hpp:196-222).  The conditions go into the WEIGHT (one
    // select each) instead of into every entry (27 selects of a double = 54 v_cndmask): a vanishing weight gives (signed) zeros.
    // (Non-finite Jacobians -- a point in the camera plane -- make the masked products NaN instead of 0.  They do not reach a sum that is
    // used: W of an edge with a fixed vertex is read by leaders only (k_schur_body: `leader` excludes it, its Y row is zeroed), and the
    // landmark sums sL of a FIXED landmark feed that landmark's own D / L^-1 bl, which only leader edges of the landmark would read.)
    const bool both = (pf >= 0) && lfree;
    const double wb = both ? w : 0.0, wl = lfree ? w : 0.0;
    const double r0l = -er[0] * wl, r1l = -er[1] * wl;
    if (d.store_w || Wout) {
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const double wv = Ji[a] * wb * Jj[b] + Ji[6 + a] * wb * Jj[3 + b];
          if (d.store_w) d.W[(size_t)(a * 3 + b) * d.E + e] = wv;
          if (Wout) Wout[a * 3 + b] = wv;
        }
    }
    // landmark contributions: Hll (6 unique) + bl
    int q = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = a; b < 3; ++b) sL[q++][t] = Jj[a] * wl * Jj[b] + Jj[3 + a] * wl * Jj[3 + b];
#pragma unroll
    for (int a = 0; a < 3; ++a) sL[6 + a][t] = Jj[a] * r0l + Jj[3 + a] * r1l;
    if (small) {
      double V[LIN_VA];
      pose_terms<0, LIN_VA>(Ji, wq, r0, r1, V);
#pragma unroll
      for (int k = 0; k < LIN_VA; ++k) sV[k * PW + pos] = V[k];
    }
  }
  __syncthreads();

  // per-landmark sums in edge order (one thread per landmark of the chunk)
  double maxd = 0.0;
  if (t < nl) {
    const int lc = lm0 + t;
    const int4 lr = d.l_rec[lc];
    const int a0 = lr.x, a1 = lr.x + lr.y;
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = a0; j < a1; ++j)
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[k] += sL[k][j];
#pragma unroll
    for (int k = 0; k < 6; ++k) d.Hll[(size_t)k * d.nLm + lc] = acc[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) d.bl[(size_t)k * d.nLm + lc] = acc[6 + k];
    if (lmout) {
#pragma unroll
      for (int k = 0; k < 9; ++k) lmout[k] = acc[k];
    }
    maxd = fmax(fabs(acc[0]), fmax(fabs(acc[3]), fabs(acc[5])));
  }

  // pose blocks: owned entries, each the sum of ITS pose's run of the pose-major term rows, in two rounds of 14 and 13
  // entries per pose (large windows build the pose blocks pose-major instead: k_pose_blocks)
  if (small) {
    const int nP = d.nP;
    // (a pose none of whose edges lies in this chunk is not written: the reduction skips it through BaDev::touch)
    const bool dense = d.dense_slabs != 0;
    // (entries dealt from the LAST thread down: the landmark sums above kept the first threads busy)
    for (int i = CH - 1 - t; i < nP * LIN_VA; i += CH) {
      const int p = i / LIN_VA, k = i - p * LIN_VA;
      const int s0 = sPptr[p], s1 = sPptr[p + 1];
      if (dense || s1 > s0) slab[p * 27 + k] = run_sum(sV + k * PW, s0, s1);
    }
    __syncthreads();
    if (t < ne) {
      double V[27 - LIN_VA];
      pose_terms<LIN_VA, 27 - LIN_VA>(Ji, wq, r0, r1, V);
#pragma unroll
      for (int k = 0; k < 27 - LIN_VA; ++k) sV[k * PW + pos] = V[k];
    }
    __syncthreads();
    for (int i = CH - 1 - t; i < nP * (27 - LIN_VA); i += CH) {
      const int p = i / (27 - LIN_VA), k = i - p * (27 - LIN_VA);
      const int s0 = sPptr[p], s1 = sPptr[p + 1];
      if (dense || s1 > s0) slab[p * 27 + LIN_VA + k] = run_sum(sV + k * PW, s0, s1);
    }
  }
  if (!small) __syncthreads();                   // sRed lies over sL: every landmark sum must have been read
  double chi = rho0, md = maxd, z0 = 0.0, z1 = 0.0;
  block_sum3_max_256(chi, z0, z1, md, sRed);
  if (t == 0) {
    slab[d.lin_stride - 2] = chi;
    slab[d.lin_stride - 1] = md;
  }
}

template <int JAC>
__device__ __forceinline__ void k_linearize_entry(const BaDev& d, int bx, int cur)
{
  extern __shared__ __attribute__((aligned(16))) char lin_smem[];
  ChunkLists cl;
  chunk_lists_load(d, bx, lin_smem, false, cl);
  if (cur < 0) {                                   // device-driven LM: skip when stopped or when the linearisation at the
    if (d.scal[SC_STOP] != 0.0 || d.scal[SC_NEEDLIN] == 0.0) return;   // kept state is still valid (rejected trial)
    cur = (int)d.scal[SC_CUR];
  }
  k_linearize_body<JAC>(d, bx, cur, lin_smem, cl, nullptr, nullptr, nullptr, d.lin_slab + (size_t)bx * d.lin_stride);
}
template <int JAC>
__global__ __launch_bounds__(CH) void k_linearize(BaDev d, int cur) { k_linearize_entry<JAC>(d, blockIdx.x, cur); }
// batched: blockIdx.y = window; every window brings its own BaDev (device array)
template <int JAC>
__global__ __launch_bounds__(CH) void k_linearize_b(const BaDev* __restrict__ dv, int cur)
{
  const BaDev& d = dv[blockIdx.y];       // by reference: a private copy of the 500-byte struct ends up in scratch memory
  if ((int)blockIdx.x >= d.nCh) return;
  k_linearize_entry<JAC>(d, blockIdx.x, cur);
}

// One entry of a window's slabs summed over the chunks that wrote it (bit `bit` of their touch mask), the part of lane group j
// (0 .. 3): the chunks c = j, j + 4, j + 8, ... in ascending order.  The caller adds the four parts in part order: a fixed
// association, the same whether the slabs are sparse or dense (a chunk that does not touch the entry would add an exact zero).
// sMask: the masks of the chunks [c_base, c_base + MASK_TILE) staged in LDS by the caller.
constexpr int MASK_TILE = 256;
__device__ __forceinline__ void stage_masks(const BaDev& d, int c_base, unsigned int* sMask)
{
  const int n = min(MASK_TILE, d.nCh - c_base) * TOUCH_WORDS;
  for (int i = threadIdx.x; i < n; i += CH) sMask[i] = d.dense_slabs ? 0xFFFFFFFFu : d.touch[(size_t)c_base * TOUCH_WORDS + i];
}
__device__ __forceinline__ double slab_sum_masked(const BaDev& d, const double* col, size_t stride, int j, int bit, int c_base, const unsigned int* sMask, double p)
{
  const int c_end = min(c_base + MASK_TILE, d.nCh);
  const int w = bit >> 5, sh = bit & 31;
  int c = c_base + j;                                // (MASK_TILE is a multiple of 4: the residues mod 4 continue across tiles)
  for (; c + 12 < c_end; c += 16) {                  // four loads in flight
    double v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool on = (sMask[(c + 4 * i - c_base) * TOUCH_WORDS + w] >> sh) & 1u;
      v[i] = on ? col[(size_t)(c + 4 * i) * stride] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) p += v[i];
  }
  for (; c < c_end; c += 4)
    if ((sMask[(c - c_base) * TOUCH_WORDS + w] >> sh) & 1u) p += col[(size_t)c * stride];
  return p;
}

// slabs -> Hpp (21 per pose), bp, chi2, max|diag(H)|: 64 entries x 4 lane groups per 256-thread workgroup, combined in a
// fixed order (deterministic); workgroup 0 also reduces chi2 / max-diagonal.
// (computeLambdaInit, optimization_algorithm_levenberg.cpp:152-166, wants the max over pose AND landmark
// diagonals; with several ranks the pose diagonals need the all-reduced Hpp, see k_lambda_init.)
__device__ __forceinline__ void k_reduce_lin_body(const BaDev& d, const int bx)
{
  __shared__ double sAcc[CH];
  __shared__ unsigned int sMask[MASK_TILE * TOUCH_WORDS];
  const int t = threadIdx.x;
  const int n = d.nP * 27;
  const int stride = n + 2;
  const int ent = bx * 64 + (t & 63), grp = t >> 6;
  double acc = 0.0;
  for (int cb = 0; cb < d.nCh; cb += MASK_TILE) {
    if (cb) __syncthreads();
    stage_masks(d, cb, sMask);
    __syncthreads();
    if (ent < n) acc = slab_sum_masked(d, d.lin_slab + ent, stride, grp, d.nBlk + ent / 27, cb, sMask, acc);
  }
  sAcc[t] = acc;
  __syncthreads();
  if (ent < n && grp == 0) {
    const double v = ((sAcc[t] + sAcc[t + 64]) + sAcc[t + 128]) + sAcc[t + 192];
    const int p = ent / 27, k = ent - p * 27;
    if (k < UPPER6) { d.Hpp[p * UPPER6 + k] = v; d.iter_comm[p * UPPER6 + k] = v; }
    else { d.bp[p * 6 + (k - UPPER6)] = v; d.iter_comm[d.nP * UPPER6 + p * 6 + (k - UPPER6)] = v; }
  }
  if (bx != 0) return;
  __syncthreads();
  // chi2 / max diagonal: every chunk writes them; the chunks over the threads, then the fixed tree of block_sum_256
  double chi = 0.0, md = 0.0;
  for (int c = t; c < d.nCh; c += CH) {
    chi += d.lin_slab[(size_t)c * stride + n];
    md = fmax(md, d.lin_slab[(size_t)c * stride + n + 1]);
  }
  chi = block_sum_256(chi, sAcc);
  md = block_max_256(md, sAcc);
  if (t == 0) {
    double* tail = d.iter_comm + d.nP * 27;
    tail[0] = chi;
    for (int r = 0; r < d.world; ++r) tail[1 + r] = (r == d.rank) ? md : 0.0;
    d.scal[SC_CHI2_CUR] = chi;     // final on a single GPU; k_lambda_init overwrites it after an all-reduce
  }
}

__global__ __launch_bounds__(CH) void k_reduce_lin(BaDev d) { k_reduce_lin_body(d, blockIdx.x); }
// batched: blockIdx.y = window; every window brings its own BaDev (device array)
__global__ __launch_bounds__(CH) void k_reduce_lin_b(const BaDev* __restrict__ dv)
{
  const BaDev& d = dv[blockIdx.y];       // by reference: a private copy of the 500-byte struct ends up in scratch memory
  if ((int)blockIdx.x >= ((d.nP * 27 + 63) / 64 > 0 ? (d.nP * 27 + 63) / 64 : 1)) return;
  k_reduce_lin_body(d, blockIdx.x);
}

// after the (optional) all-reduce of iter_comm: chi2, max diagonal, and lambda_0 = 1e-5 * max on iteration 0
__device__ __forceinline__ void k_lambda_init_body(const BaDev& d, const int bx, int first_iteration)
{
  if (bx != 0) return;
  const int t = threadIdx.x;                       // one wave
  const double* tail = d.iter_comm + d.nP * 27;
  const int diag[6] = {0, 6, 11, 15, 18, 20};
  double m = 0.0;
  for (int r = t; r < d.world; r += 64) m = fmax(m, tail[1 + r]);
  for (int i = t; i < d.nP * 6; i += 64) m = fmax(m, fabs(d.iter_comm[(i / 6) * UPPER6 + diag[i % 6]]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  if (t != 0) return;
  d.scal[SC_CHI2_CUR] = tail[0];
  d.scal[SC_MAXDIAG] = m;
  if (first_iteration) d.scal[SC_LAMBDA] = 1e-5 * m;
}

__global__ __launch_bounds__(64) void k_lambda_init(BaDev d, int first_iteration) { k_lambda_init_body(d, blockIdx.x, first_iteration); }
// batched: blockIdx.y = window; every window brings its own BaDev (device array)
__global__ __launch_bounds__(64) void k_lambda_init_b(const BaDev* __restrict__ dv, int first_iteration)
{
  const BaDev& d = dv[blockIdx.y];       // by reference: a private copy of the 500-byte struct ends up in scratch memory
  if ((int)blockIdx.x >= (1)) return;
  k_lambda_init_body(d, blockIdx.x, first_iteration);
}

// Device-driven LM: start of one optimize(iters) at state buffer `cur` (stop = 1: nothing to optimise on any rank)
__device__ __forceinline__ void k_lm_begin_body(const BaDev& d, const int bx, int cur, int iters, int nstat, int stop)
{
  if (threadIdx.x != 0 || bx != 0) return;
  d.scal[SC_NI] = 2.0; d.scal[SC_CUR] = (double)cur; d.scal[SC_IT] = 0.0; d.scal[SC_QMAX] = 0.0;
  d.scal[SC_STOP] = (stop || iters <= 0) ? 1.0 : 0.0; d.scal[SC_NEEDLIN] = 1.0; d.scal[SC_ITERS] = (double)iters;
  d.scal[SC_NSTAT] = (double)nstat; d.scal[SC_CURCHI] = 0.0; d.scal[SC_TRIALS_RUN] = 0.0;
  *d.ticket.get() = 0u;
}

__global__ __launch_bounds__(64) void k_lm_begin(BaDev d, int cur, int iters, int nstat, int stop) { k_lm_begin_body(d, blockIdx.x, cur, iters, nstat, stop); }
// batched: blockIdx.y = window; every window brings its own BaDev (device array)
__global__ __launch_bounds__(64) void k_lm_begin_b(const BaDev* __restrict__ dv, int cur, int iters, int nstat, int stop)
{
  const BaDev& d = dv[blockIdx.y];       // by reference: a private copy of the 500-byte struct ends up in scratch memory
  if ((int)blockIdx.x >= (1)) return;
  k_lm_begin_body(d, blockIdx.x, cur, iters, nstat, stop);
}

// The bookkeeping of one LM trial (OptimizationAlgorithmLevenberg::solve, optimization_algorithm_levenberg.cpp:99-140)
// on the trial's scalars; one thread, called by the kernel that completes them.
__device__ void lm_step(const BaDev& d)
{
  double* sc = d.scal;
  if (sc[SC_STOP] != 0.0) return;
  double lambda = sc[SC_LAMBDA], ni = sc[SC_NI];
  int it = (int)sc[SC_IT], q = (int)sc[SC_QMAX], cur = (int)sc[SC_CUR];
  double current_chi = sc[SC_CURCHI];
  if (q == 0) {
    current_chi = sc[SC_CHI2_CUR];
    if (it == 0) ni = 2.0;
  }
  const bool ok = sc[SC_SOLVE_OK] != 0.0;
  const double temp_chi = ok ? sc[SC_TEMP_CHI] : 1.7976931348623157e308;
  double rho = current_chi - temp_chi;
  rho /= sc[SC_SCALE_P] + sc[SC_SCALE_L] + 1e-3;
  bool lambda_bad = false, accepted = false;
  if (rho > 0 && isfinite(temp_chi)) {
    double alpha = 1. - pow((2 * rho - 1), 3.0);
    alpha = fmin(alpha, 2. / 3.);
    lambda *= fmax(1. / 3., alpha);
    ni = 2.0;
    current_chi = temp_chi;
    cur ^= 1;                                      // accept: the trial buffers become the state
    accepted = true;
  } else {
    lambda *= ni;
    ni *= 2.0;
    if (!isfinite(lambda)) lambda_bad = true;
  }
  if (!lambda_bad) ++q;
  sc[SC_LAMBDA] = lambda; sc[SC_NI] = ni; sc[SC_CUR] = (double)cur; sc[SC_CURCHI] = current_chi;
  sc[SC_TRIALS_RUN] += 1.0;
  if (!lambda_bad && rho < 0 && q < 10) {          // another trial of the same iteration, same linearisation
    sc[SC_QMAX] = (double)q; sc[SC_NEEDLIN] = 0.0;
    return;
  }
  const int ns = (int)sc[SC_NSTAT];
  if (ns < SSX_BA_MAX_STATS) {
    d.lm_stat[ns] = temp_chi;
    d.lm_stat[SSX_BA_MAX_STATS + ns] = lambda;
    d.lm_stat[2 * SSX_BA_MAX_STATS + ns] = (double)q;
  }
  sc[SC_NSTAT] = (double)(ns + 1);
  ++it;
  sc[SC_IT] = (double)it; sc[SC_QMAX] = 0.0; sc[SC_NEEDLIN] = 1.0;
  (void)accepted;
  if (q == 10 || rho == 0 || lambda_bad || it >= (int)sc[SC_ITERS]) sc[SC_STOP] = 1.0;
}

__global__ void k_set_lambda(BaDev d, double lambda)
{
  if (threadIdx.x == 0 && blockIdx.x == 0) d.scal[SC_LAMBDA] = lambda;
}

// ------------------------------------------------------------------------------------------------
// k_build_lists: the (edge a, edge b) pair lists of the reduced system's blocks and the balanced work items of k_schur's
// block phase, per chunk, ON THE DEVICE -- what the host marshalling spent 40 % of its time on (0.2 of 0.53 ms per C3
// window).  Same lists, byte for byte, as prepare() builds with SSX_BA_HOST_LISTS=1 (tests/test_ba_gpu.py compares the
// solves bit by bit): pairs grouped by block in block order, inside a block in landmark order (a landmark has at most one
// pair per block: its leaders see distinct poses), items sorted by part length with the parts of a block inside one wave.
// One workgroup per chunk; the landmarks are the lanes of waves 0 and 1, "which landmarks hold block b" is a ballot.
// ------------------------------------------------------------------------------------------------
constexpr int LIST_MAX_BLK = SSX_BA_SMALL_P * (SSX_BA_SMALL_P + 1) / 2;   // 136
__device__ __forceinline__ void k_build_lists_body(const BaDev& d, const int c)
{
  __shared__ uint8_t sEdgeOf[CH_L][SSX_BA_SMALL_P];
  __shared__ int8_t sLead[CH];                                            // free pose of a leader edge, -1 otherwise
  __shared__ int sCnt[2][LIST_MAX_BLK];
  __shared__ int sBp[LIST_MAX_BLK + 1];
  __shared__ int sLen[LIST_MAX_BLK], sK[LIST_MAX_BLK];
  __shared__ uint8_t sSorted[LIST_MAX_BLK];
  __shared__ int sMaxLen, sWaveTot[4], sWaveMax[4];
  __shared__ int sPosR[LIST_MAX_BLK + 1];                                 // first item of the r-th block in sorted order, padding included
  __shared__ int sKr[LIST_MAX_BLK];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int4 cd = d.ch_desc[c];
  const int e0 = cd.x, lm0 = cd.z, nl = cd.w;
  const int nP = d.nP, nBlk = d.nBlk;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  // 1. every unfixed landmark: which free poses see it (leader edges: free pose, not a duplicate), and through which edge.
  // (the edge records come in with ONE coalesced load per edge thread; a landmark thread walking its edges in global memory
  // paid a memory round trip per edge)
  if (t < cd.y) {
    const int4 er = d.e_rec[e0 + t];
    sLead[t] = (er.y >= 0 && !(er.w & 2)) ? (int8_t)er.y : (int8_t)-1;
  }
  int4 lr = make_int4(0, 0, 0, 1);
  if (t < nl) lr = d.l_rec[lm0 + t];
  __syncthreads();
  uint32_t mask = 0;
  if (t < nl && !lr.w)
    for (int j = lr.x; j < lr.x + lr.y; ++j) {
      const int pf = sLead[j];
      if (pf >= 0) { mask |= 1u << pf; sEdgeOf[t][pf] = (uint8_t)j; }
    }
  __syncthreads();
  // 2. pairs per block and wave
  if (wave < 2) {
    int pa = 0, pb = 0;
    for (int b = 0; b < nBlk; ++b) {
      const bool has = ((mask >> pa) & (mask >> pb) & 1u) != 0;
      const unsigned long long bal = __ballot(has);
      if (lane == 0) sCnt[wave][b] = __popcll(bal);
      if (++pb == nP) { ++pa; pb = pa; }
    }
  }
  __syncthreads();
  // 3. block offsets inside the chunk's list (block order: an exclusive scan over <= 136 counts), the longest list
  {
    const int n = t < nBlk ? sCnt[0][t] + sCnt[1][t] : 0;
    int inc = n, mx = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(inc, o); if (lane >= o) inc += up; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
    if (lane == 63) { sWaveTot[wave] = inc; sWaveMax[wave] = mx; }
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += sWaveTot[w];
    if (t < nBlk) sBp[t] = before + inc - n;
    if (t == nBlk) sBp[nBlk] = before + inc - n;                       // = the total (its own n is 0)
    if (t == 0) sMaxLen = max(max(sWaveMax[0], sWaveMax[1]), max(sWaveMax[2], sWaveMax[3]));
  }
  __syncthreads();
  const int base = c * MAX_PAIRS;
  for (int b = t; b <= nBlk; b += CH) d.pair_ptr[(size_t)c * (nBlk + 1) + b] = base + sBp[b];
  // 4. the pairs: landmark order inside a block = rank of the landmark among the holders of the block
  if (wave < 2) {
    int pa = 0, pb = 0;
    for (int b = 0; b < nBlk; ++b) {
      const bool has = ((mask >> pa) & (mask >> pb) & 1u) != 0;
      const unsigned long long bal = __ballot(has);
      if (has) {
        const int q = base + sBp[b] + (wave ? sCnt[0][b] : 0) + __popcll(bal & lt_mask);
        d.pair_a[q] = sEdgeOf[t][pa];
        d.pair_b[q] = sEdgeOf[t][pb];
      }
      if (++pb == nP) { ++pa; pb = pa; }
    }
  }
  // 4b. the chunk's touch mask: the blocks that have pairs, the free poses that have edges here (any edge: the pose blocks sum
  // over fixed landmarks' edges too)
  if (t < TOUCH_WORDS) {
    unsigned int m = 0;
    for (int b = 32 * t; b < min(32 * t + 32, nBlk + nP); ++b) {
      const bool on = b < nBlk ? (sBp[b + 1] > sBp[b]) : (d.pptr[(size_t)c * (nP + 1) + (b - nBlk) + 1] > d.pptr[(size_t)c * (nP + 1) + (b - nBlk)]);
      m |= (on || d.dense_slabs) ? 1u << (b & 31) : 0u;
    }
    d.touch[(size_t)c * TOUCH_WORDS + t] = m;
  }
  // 5. work items of the block phase (prepare()'s rule: parts of at least BSEG_MIN pairs, at most BSEG_PARTS per block, sorted by
  // part length -- ties in block order --, the parts of one block inside one group of FOUR items = one row of 16 lanes, so that the
  // parts meet through DPP row shifts).  A block without pairs gets no item (it is not written) unless the slabs are dense.
  const int seg = max(BSEG_MIN, (sMaxLen + BSEG_PARTS - 1) / BSEG_PARTS);
  if (t < nBlk) {
    const int n = sBp[t + 1] - sBp[t], k = (n == 0 && !d.dense_slabs) ? 0 : max(1, (n + seg - 1) / seg);
    sK[t] = k;
    sLen[t] = k ? (n + k - 1) / k : 0;
  }
  __syncthreads();
  if (t < nBlk) {
    const int len = sLen[t];
    int rank = 0;
    for (int b = 0; b < nBlk; ++b) { const int lb = sLen[b]; rank += (lb > len) || (lb == len && b < t); }
    sSorted[rank] = (uint8_t)t;
  }
  __syncthreads();
  if (t < nBlk) sKr[t] = sK[sSorted[t]];
  __syncthreads();
  if (t == 0) {
    // where every block's parts start: the only sequential piece (a block moves to the next group of 16 items when it would
    // straddle one), the loads do not depend on the running position
    int pos = 0;
    for (int r = 0; r < nBlk; ++r) {
      const int k = sKr[r];
      if ((pos & 3) + k > 4) pos = (pos + 3) & ~3;
      sPosR[r] = pos;
      pos += k;
    }
    sPosR[nBlk] = pos;
    d.bseg_ptr[2 * c] = c * d.bseg_cap;
    d.bseg_ptr[2 * c + 1] = pos;
  }
  __syncthreads();
  if (t < nBlk) {
    int4* out = d.bseg + (size_t)c * d.bseg_cap;
    const int b = sSorted[t], n = sBp[b + 1] - sBp[b], k = sK[b], len = sLen[b], p0 = sPosR[t];
    for (int i = 0; i < k; ++i) out[p0 + i] = make_int4(b, sBp[b] + min(n, i * len), sBp[b] + min(n, (i + 1) * len), i | (k << 4));
    for (int q = p0 + k; q < sPosR[t + 1]; ++q) out[q] = make_int4(-1, 0, 0, 1 << 4);   // the padding in front of the next block
  }
}
__global__ __launch_bounds__(CH) void k_build_lists(BaDev d) { k_build_lists_body(d, blockIdx.x); }
__global__ __launch_bounds__(CH) void k_build_lists_b(const BaDev* __restrict__ dv)
{
  const BaDev& d = dv[blockIdx.y];
  if ((int)blockIdx.x >= d.nCh || d.bseg_cap == 0) return;
  k_build_lists_body(d, blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// Device-side marshalling of a small window (what prepare() did on the host for every solve: 0.18 of the 0.92 ms of a C3
// window, 48 MB of marshalled blobs per 64-window batch): the caller's arrays are uploaded AS THEY ARE with two small host
// tables (edges per landmark -> lm_ptr / chunks, and slot8 = an edge's rank among its landmark's edges in caller order).
//   k_prep_scatter   stable counting sort by landmark: sorted position = lm_ptr[landmark] + slot8
//   k_prep_chunk     one workgroup per chunk: stable sort of every landmark's edges by pose (duplicates adjacent), packed
//                    edge / landmark records, duplicate flags, pose-major positions + per-pose segments, uv columns, the
//                    sorted -> caller permutation; then the chunk's pair lists and work items (k_build_lists_body)
// Byte for byte the arrays of the host marshalling (SSX_BA_HOST_PREP=1; test_device_marshalling_equals_host_marshalling).
// ------------------------------------------------------------------------------------------------
#define SSX_AS1(T) const __attribute__((address_space(1))) T*
__device__ __forceinline__ int raw_pose(const BaDev& d, int e)
{
  return (d.raw_fmt & 1) ? (int)((SSX_AS1(uint8_t))d.r_edge_pose.get())[e] : d.r_edge_pose[e];
}
__device__ __forceinline__ int raw_point(const BaDev& d, int e)
{
  return (d.raw_fmt & 2) ? (int)((SSX_AS1(uint16_t))d.r_edge_point.get())[e] : d.r_edge_point[e];
}
__device__ __forceinline__ double raw_uv(const BaDev& d, size_t i)
{
  return (d.raw_fmt & 4) ? (double)((SSX_AS1(float))d.r_edge_uv.get())[i] : d.r_edge_uv[i];
}
__device__ __forceinline__ void k_prep_scatter_body(const BaDev& d, const int bx)
{
  const int e = bx * CH + threadIdx.x;
  if (e >= d.E_raw) return;
  const int l = raw_point(d, e);
  if (l < 0) return;                                  // a dead entry of a window's storage
  d.perm[d.lm_ptr[d.lm_compact[l]] + d.r_slot8[e]] = e;
}
__global__ __launch_bounds__(CH) void k_prep_scatter(BaDev d) { k_prep_scatter_body(d, blockIdx.x); }
__global__ __launch_bounds__(CH) void k_prep_scatter_b(const BaDev* __restrict__ dv)
{
  const BaDev& d = dv[blockIdx.y];
  if (!d.dev_prep || (int)blockIdx.x * CH >= d.E_raw) return;
  k_prep_scatter_body(d, blockIdx.x);
}

__device__ __forceinline__ void k_prep_chunk_body(const BaDev& d, const int c)
{
  __shared__ int sOrig[CH], sPose[CH], sKey[CH];
  __shared__ uint8_t sLmOf[CH], sFix[CH_L];
  __shared__ int sLid[CH_L];
  __shared__ int sCnt[4][SSX_BA_SMALL_P + 1];
  __shared__ int sBase[SSX_BA_SMALL_P + 2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int4 cd = d.ch_desc[c];
  const int e0 = cd.x, ne = cd.y, lm0 = cd.z, nl = cd.w;
  const int nP = d.nP, E = d.E;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  if (t < ne) {
    const int og = d.perm[e0 + t];
    sOrig[t] = og;
    const int po = raw_pose(d, og);
    sPose[t] = po;
    sKey[t] = d.pose_rank.p ? d.pose_rank[po] : po;
  }
  int lm_a0 = 0, lm_k = 0;
  if (t < nl) {
    const int lc = lm0 + t;
    lm_a0 = d.lm_ptr[lc] - e0;
    lm_k = d.lm_ptr[lc + 1] - d.lm_ptr[lc];
    sLid[t] = d.lm_id[lc];
    sFix[t] = d.lm_fixed[lc];
  }
  __syncthreads();
  if (t < nl) {
    // stable insertion sort by pose (the edges of a landmark usually arrive in keyframe order: one pass, no move)
    for (int i = lm_a0 + 1; i < lm_a0 + lm_k; ++i) {
      const int po = sPose[i], og = sOrig[i], ky = sKey[i];
      int j = i - 1;
      while (j >= lm_a0 && sKey[j] > ky) { sPose[j + 1] = sPose[j]; sOrig[j + 1] = sOrig[j]; sKey[j + 1] = sKey[j]; --j; }
      sPose[j + 1] = po; sOrig[j + 1] = og; sKey[j + 1] = ky;
    }
    for (int i = lm_a0; i < lm_a0 + lm_k; ++i) sLmOf[i] = (uint8_t)t;
    const_cast<int4*>(static_cast<const int4*>(d.l_rec.p))[lm0 + t] = make_int4(lm_a0, lm_k, sLid[t], sFix[t]);
  }
  __syncthreads();
  int og = 0, pose = 0, l = 0, pf = -1, bucket = -1;
  if (t < ne) {
    og = sOrig[t]; pose = sPose[t]; l = sLmOf[t];
    pf = d.pose_free[pose];
    bucket = pf >= 0 ? pf : nP;                                  // fixed-pose edges go behind the free poses' segments
  }
  int rank = 0;
  const bool small = !d.big;                                     // (large windows have no pose-major order inside a chunk)
  if (small) {
  for (int p = 0; p <= nP; ++p) {
    const unsigned long long bal = __ballot(bucket == p);
    if (lane == 0) sCnt[wave][p] = __popcll(bal);
    if (bucket == p) rank = __popcll(bal & lt_mask);
  }
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int p = 0; p <= nP; ++p) { sBase[p] = run; run += sCnt[0][p] + sCnt[1][p] + sCnt[2][p] + sCnt[3][p]; }
    sBase[nP + 1] = run;
  }
  __syncthreads();
  if (t <= nP) const_cast<uint16_t*>(static_cast<const uint16_t*>(d.pptr.p))[(size_t)c * (nP + 1) + t] = (uint16_t)sBase[t];
  } else if (t < nl) {
    d.lm_chunk[lm0 + t] = c;
  }
  if (t < ne) {
    int pos = 0;
    if (small) {
      pos = sBase[bucket] + rank;
      for (int w = 0; w < wave; ++w) pos += sCnt[w][bucket];
    }
    const bool dup = t > 0 && sLmOf[t - 1] == l && sPose[t - 1] == pose;
    const bool next_dup = t + 1 < ne && sLmOf[t + 1] == l && sPose[t + 1] == pose;
    const uint8_t* rc = d.r_edge_cam;
    const int cam = (d.r_edge_cam.p && rc[og]) ? 1 : 0;
    const int flags = cam | ((int)dup << 1) | ((int)sFix[l] << 2) | ((int)next_dup << 3) | ((pf < 0 ? 1 : 0) << 5) | (l << 8) | (pos << 16);
    const int e = e0 + t;
    const_cast<int4*>(static_cast<const int4*>(d.e_rec.p))[e] = make_int4(pose, pf, sLid[l], flags);
    const_cast<uint8_t*>(static_cast<const uint8_t*>(d.e_dup.p))[e] = dup ? 1 : 0;
    double* uv = const_cast<double*>(static_cast<const double*>(d.e_uv.p));
    uv[e] = raw_uv(d, 2 * (size_t)og);
    uv[(size_t)E + e] = raw_uv(d, 2 * (size_t)og + 1);
    d.perm[e] = og;
    if (!small) {                                                  // the structure-of-arrays columns the large-window kernels read
      const_cast<int*>(static_cast<const int*>(d.e_pose.p))[e] = pose;
      const_cast<int*>(static_cast<const int*>(d.e_lmc.p))[e] = lm0 + l;
      const_cast<uint8_t*>(static_cast<const uint8_t*>(d.e_cam.p))[e] = (uint8_t)cam;
    }
  }
}

// large windows: keys / values of the stable sort that groups the sorted edges by free pose (BigDev::pe_edge)
__global__ __launch_bounds__(CH) void k_pe_keys(BaDev d, unsigned int* keys, unsigned int* vals)
{
  const int sidx = blockIdx.x * CH + threadIdx.x;
  if (sidx >= d.E) return;
  const int pf = d.e_rec[sidx].y;
  keys[sidx] = pf >= 0 ? (unsigned int)pf : (unsigned int)d.nP;      // fixed poses' edges sort behind every free pose's
  vals[sidx] = (unsigned int)sidx;
}

__global__ __launch_bounds__(CH) void k_prep_chunk(BaDev d)
{
  k_prep_chunk_body(d, blockIdx.x);
  __syncthreads();                                  // the records of this chunk are read back by the list builder below
  if (d.bseg_cap) k_build_lists_body(d, blockIdx.x);
}
// batched: every window's records (if it is device-marshalled) and lists (if they are device-built) in one launch
__global__ __launch_bounds__(CH) void k_prep_chunk_b(const BaDev* __restrict__ dv)
{
  const BaDev& d = dv[blockIdx.y];
  if ((int)blockIdx.x >= d.nCh) return;
  if (d.dev_prep) {
    k_prep_chunk_body(d, blockIdx.x);
    __syncthreads();
  }
  if (d.bseg_cap) k_build_lists_body(d, blockIdx.x);
}

// e0^2 + e1^2 exactly as the host forms it from the two downloaded components: two products, one sum, no contraction into a
// fused multiply-add (the results of a device-marshalled window must be the bits of a host-marshalled one)
__device__ __forceinline__ double chi2_of(double a, double b)
{
#pragma clang fp contract(off)
  const double aa = a * a, bb = b * b;
  return aa + bb;
}

// edge chi2 of a device-marshalled window in the CALLER's edge order (the host never sees the sorted order)
__device__ __forceinline__ void k_c2_out_body(const BaDev& d, const int bx, int trial_err)
{
  const int sidx = bx * CH + threadIdx.x;
  if (sidx >= d.E) return;
  if (trial_err == 2) trial_err = d.scal[SC_TRIALS_RUN] > 0.0;        // enqueued before the host has seen the control block
  const double* err = trial_err ? (const double*)d.err_trial : (const double*)d.err_lin;
  const double a = err[sidx], b = err[(size_t)d.E + sidx];
  d.c2_out[d.perm[sidx]] = chi2_of(a, b);
}
__global__ __launch_bounds__(CH) void k_c2_out(BaDev d, int trial_err) { k_c2_out_body(d, blockIdx.x, trial_err); }

// W_e = Ji^T w Jj (6x3) of sorted edge e at the linearisation state `cur`: what k_linearize computes, recomputed by the
// kernels that need it when d.store_w == 0 (analytic Jacobians: the same instruction sequence, the same bits)
__device__ __forceinline__ void edge_W(const BaDev& d, int cur, int e, double* W)
{
  const int4 er4 = d.e_rec[e];
  const int p = er4.x, lid = er4.z;
  const bool both = er4.y >= 0 && !(er4.w & 4);
  if (!both) {
#pragma unroll
    for (int k = 0; k < 18; ++k) W[k] = 0.0;
    return;
  }
  const double* pose = d.pose[cur];
  const double* point = d.point[cur];
  double T[7], X[3];
#pragma unroll
  for (int k = 0; k < 7; ++k) T[k] = pose[p * 7 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = point[lid * 3 + k];
  const double* ext = d.ext + 7 * (er4.w & 1);
  double er[2], p1[3], pc[3], Ji[12], Jj[6], rho0, w;
  ssx::edge_error(T, X, ext, d.K, d.e_uv[e], d.e_uv[d.E + e], er, p1, pc);
  ssx::edge_jac_analytic(T, ext, d.K, p1, pc, Ji, Jj);
  ssx::huber(er[0] * er[0] + er[1] * er[1], d.huber_delta, rho0, w);
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) W[a * 3 + b] = Ji[a] * w * Jj[b] + Ji[6 + a] * w * Jj[3 + b];
}

// ------------------------------------------------------------------------------------------------
// k_schur: landmark elimination for one chunk at damping lambda.
// restates the marginalisation loop of BlockSolver::solve (block_solver.hpp:342-393):
//   Dinv = (Hll + lambda I)^-1 ; c_i += W_i Dinv bl ; S_ij -= (W_i Dinv) W_j^T  (upper blocks)
// ------------------------------------------------------------------------------------------------
// Win (18, nullable): this thread's edge block W from a linearisation phase that just ran in the same kernel; lmin (9,
// nullable): this thread's landmark sums (Hll 6 + bl 3).  The stop / state checks are the wrappers'.
// erw_in (nullable): this thread's edge flag word from the linearisation phase (fused kernel).
__device__ __forceinline__ void k_schur_body(const BaDev& d, const int bx, int cur, double lambda, char* smem, const ChunkLists& cl, const double* Win,
                                             const double* lmin, const int* erw_in, double* slab)
{
  // With D = Hll + lambda I = L L^T (3x3 Cholesky) and Y_e = W_e L^-T, the Schur term of an edge pair is
  // W_a D^-1 W_b^T = Y_a Y_b^T and W D^-1 bl = Y (L^-1 bl): ONE 6x3 array per edge in LDS instead of W and W D^-1
  // (37 KB per chunk instead of 74; with <= 128 landmarks per chunk the whole workgroup needs 53 KB: three per CU).
  // pitch PW = CH + 1 doubles: the owned-entry loops read [component][edge] with the component varying across
  // lanes -- an even pitch would put all components on the same LDS bank
  double* sY = reinterpret_cast<double*>(smem);            // [18][PW]   Y = W L^-T of the leader edges
  double* sG = sY + 18 * PW;                               // [6][PL] per landmark: 1/l00, l10, l20, 1/l11, l21, 1/l22
  double* sGb = sG + 6 * PL;                               // [3][PL] per landmark: L^-1 bl
  int* sLm = reinterpret_cast<int*>(sGb + 3 * PL);         // [CH] local landmark of each edge
  const uint16_t* sPptr = reinterpret_cast<const uint16_t*>(smem + BA_OFF_PPTR);   // [SSX_BA_SMALL_P + 2]   (chunk_lists_load)
  const uint16_t* sPab = reinterpret_cast<const uint16_t*>(smem + BA_OFF_PAB);     // [MAX_PAIRS] edge a | edge b << 8, grouped by block

  const int t = tid_opaque();
  (void)bx;
  const int4 cd = cl.cd;
  const int e0 = cd.x, ne = cd.y, lm0 = cd.z, nl = cd.w;
  const int nP = d.nP;

  bool leader = false;
  double Wm[18];
  double z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // this edge's term of c = sum W D^-1 bl: Y (L^-1 bl)
  int zpos = 0;                                  // its position in the chunk's pose-major order
  const int it0 = cl.it0, n_items = cl.n_items;
  int4 item_rec = cl.item_rec;
  if (t < ne) {
    const int e = e0 + t;
    const int erw = erw_in ? *erw_in : d.e_rec[e].w;
    sLm[t] = (erw >> 8) & 0xFF;
    zpos = (erw >> 16) & 0xFF;
    leader = !(erw & (6 | 32));                              // free pose (bit 5 clear), free landmark, not a duplicate
    if (leader) {
      // merge duplicates (several edges of the same (landmark,pose) pair share one Hpl block in g2o)
      if (Win) {
#pragma unroll
        for (int k = 0; k < 18; ++k) Wm[k] = Win[k];
      } else if (d.store_w) {
#pragma unroll
        for (int k = 0; k < 18; ++k) Wm[k] = d.W[(size_t)k * d.E + e];
      } else {
        edge_W(d, cur, e, Wm);
      }
      for (int j = t + 1; (erw & 8) && j < ne && d.e_dup[e0 + j]; ++j) {   // bit 3: the next edge is a duplicate of this one (rare)
        double Wd[18];
        if (d.store_w) {                                   // (written by this workgroup's linearisation phase, a barrier ago, when fused)
#pragma unroll
          for (int k = 0; k < 18; ++k) Wd[k] = d.W[(size_t)k * d.E + e0 + j];
        } else {
          edge_W(d, cur, e0 + j, Wd);
        }
#pragma unroll
        for (int k = 0; k < 18; ++k) Wm[k] += Wd[k];
      }
    }
  }
  if (t < nl) {
    const int lc = lm0 + t;
    double D[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) D[k] = lmin ? lmin[k] : d.Hll[(size_t)k * d.nLm + lc];
    D[0] += lambda; D[3] += lambda; D[5] += lambda;
    // D = (d00 d01 d02 d11 d12 d22); a non-positive pivot yields NaN, the reduced solve then reports failure and the
    // LM step is rejected (g2o: Cholesky failure)
    const double i00 = 1.0 / sqrt(D[0]);
    const double l10 = D[1] * i00, l20 = D[2] * i00;
    const double i11 = 1.0 / sqrt(D[3] - l10 * l10);
    const double l21 = (D[4] - l20 * l10) * i11;
    const double i22 = 1.0 / sqrt(D[5] - l20 * l20 - l21 * l21);
    sG[t] = i00; sG[PL + t] = l10; sG[2 * PL + t] = l20; sG[3 * PL + t] = i11; sG[4 * PL + t] = l21; sG[5 * PL + t] = i22;
    const double b0 = lmin ? lmin[6] : d.bl[lc], b1 = lmin ? lmin[7] : d.bl[(size_t)d.nLm + lc], b2 = lmin ? lmin[8] : d.bl[(size_t)2 * d.nLm + lc];
    const double g0 = b0 * i00, g1 = (b1 - l10 * g0) * i11, g2 = (b2 - l20 * g0 - l21 * g1) * i22;
    sGb[t] = g0; sGb[PL + t] = g1; sGb[2 * PL + t] = g2;
  }
  __syncthreads();
  if (t < ne) {
    if (leader) {
      const int l = sLm[t];
      const double i00 = sG[l], l10 = sG[PL + l], l20 = sG[2 * PL + l], i11 = sG[3 * PL + l], l21 = sG[4 * PL + l], i22 = sG[5 * PL + l];
      const double g0 = sGb[l], g1 = sGb[PL + l], g2 = sGb[2 * PL + l];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double y0 = Wm[a * 3] * i00;
        const double y1 = (Wm[a * 3 + 1] - y0 * l10) * i11;
        const double y2 = (Wm[a * 3 + 2] - y0 * l20 - y1 * l21) * i22;
        sY[(a * 3) * PW + t] = y0; sY[(a * 3 + 1) * PW + t] = y1; sY[(a * 3 + 2) * PW + t] = y2;
        z[a] = y0 * g0 + y1 * g1 + y2 * g2;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 18; ++k) sY[k * PW + t] = 0.0;
    }
  }
  __syncthreads();

  // The reduced system's blocks: FOUR lanes per work item, each owning a 3x3 quarter of the 6x6 -- it walks (a part of)
  // the block's (edge a, edge b) pairs in landmark order with 9 independent accumulators: 18 LDS doubles per pair feed
  // 27 fused multiply-adds.  A wave takes as long as its longest list and nine tenths of the kernel's VALU
  // instructions are issued here, so the host cuts the lists (0 .. 40 pairs) into parts of equal length, sorts the
  // items by length and keeps the parts of one block in one row of 16 lanes (d.bseg): the first part collects the partial
  // sums through DPP row shifts, in part order.
  // (Tried and slower: reading only one 3x3 operand per lane and passing the other between the lanes of the quad
  // through DPP -- half the LDS traffic; an explicit software pipeline of index / operands / multiply.)
  const int nS = d.nBlk * 36;
  for (int base = 0; base < n_items; base += CH) {
    const int4 ir = item_rec;
    if (base + CH < n_items) item_rec = base + CH + t < n_items ? d.bseg[it0 + ((base + CH + t) >> 2)] : make_int4(-1, 0, 0, 1 << 4);
    const int blk = ir.x, qr = (t >> 1) & 1, qc = t & 1;                 // rows 3 qr .. 3 qr + 2, columns 3 qc .. 3 qc + 2
    const int q0 = ir.y, q1 = ir.z, part = ir.w & 15, parts = ir.w >> 4;
    double acc[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[i][j] = 0.0;
    const double* bdp = sY + (qr * 9) * PW;                              // component (row r, m) of Y = r * 3 + m
    const double* wp = sY + (qc * 9) * PW;
#pragma unroll 2
    for (int q = q0; q < q1; ++q) {
      const int ab = sPab[q];
      const int ea = ab & 0xFF, eb = ab >> 8;
      double bd[3][3], w[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int m = 0; m < 3; ++m) { bd[i][m] = bdp[(i * 3 + m) * PW + ea]; w[i][m] = wp[(i * 3 + m) * PW + eb]; }
      // three chained fused multiply-adds per entry (nine independent chains): 27 f64 instructions per pair instead of the
      // 36 of  acc += a b + c d + e f
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = fma(bd[i][2], w[j][2], fma(bd[i][1], w[j][1], fma(bd[i][0], w[j][0], acc[i][j])));
    }
    if (__any(parts > 1)) {                                              // wave-uniform
      // the parts of a block sit in consecutive items of ONE row of 16 lanes (k_build_lists): part q's sums are 4 q lanes up the
      // row -- DPP row shifts on the VALU (the __shfl_down they replace were 54 ds_bpermute_b32 per pass: LDS-pipeline instructions)
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double v1 = dpp_f64<0x104>(acc[i][j]), v2 = dpp_f64<0x108>(acc[i][j]), v3 = dpp_f64<0x10C>(acc[i][j]);   // row_shl:4 / 8 / 12
          if (part == 0) {
            if (parts > 1) acc[i][j] += v1;
            if (parts > 2) acc[i][j] += v2;
            if (parts > 3) acc[i][j] += v3;
          }
        }
    }
    if (blk >= 0 && part == 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) slab[blk * 36 + (3 * qr + i) * 6 + 3 * qc + j] = acc[i][j];
    }
  }
  // c: the per-edge terms z go to LDS in POSE-MAJOR positions (Y is dead), four threads per entry share the pose's run,
  // partial sums folded inside the quad (the former loop chased the pose's edge list: three dependent LDS round trips
  // per edge)
  __syncthreads();
  if (t < ne) {
#pragma unroll
    for (int a = 0; a < 6; ++a) sY[a * PW + zpos] = z[a];
  }
  __syncthreads();
  for (int base = 0; base < nP * 6 * 4; base += CH) {
    const int item = base + t;
    const bool on = item < nP * 6 * 4;
    const int idx = on ? item >> 2 : 0, part = item & 3;
    const int p = idx / 6, a = idx - p * 6;
    double acc = 0.0;
    const int s0 = on ? sPptr[p] : 0, s1 = on ? sPptr[p + 1] : 0;
    for (int s = s0 + part; s < s1; s += 4) acc += sY[a * PW + s];
    acc += dpp_f64<DPP_QUAD_XOR1>(acc);                              // (the sums of __shfl_xor(acc, 1), (acc, 2): same pairs, same bits)
    acc += dpp_f64<DPP_QUAD_XOR2>(acc);
    if (on && part == 0 && (d.dense_slabs || s1 > s0)) slab[nS + idx] = acc;     // (a pose without edges here: not written, not read)
  }
}

__device__ __forceinline__ void k_schur_entry(const BaDev& d, int bx)
{
  extern __shared__ __attribute__((aligned(16))) char schur_smem[];
  ChunkLists cl;
  chunk_lists_load(d, bx, schur_smem, true, cl);
  if (d.scal[SC_STOP] != 0.0) return;                             // device-driven LM, already terminated
  const int cur = (int)d.scal[SC_CUR];
  const double lambda = d.scal[SC_LAMBDA];
  k_schur_body(d, bx, cur, lambda, schur_smem, cl, nullptr, nullptr, nullptr, d.schur_slab + (size_t)bx * (d.nBlk * 36 + d.nP * 6));
}
__global__ __launch_bounds__(CH) void k_schur(BaDev d) { k_schur_entry(d, blockIdx.x); }
// batched: blockIdx.y = window; every window brings its own BaDev (device array)
__global__ __launch_bounds__(CH) void k_schur_b(const BaDev* __restrict__ dv)
{
  const BaDev& d = dv[blockIdx.y];       // by reference: a private copy of the 500-byte struct ends up in scratch memory
  if ((int)blockIdx.x >= d.nCh) return;
  k_schur_entry(d, blockIdx.x);
}

// k_lin_schur: one slot of the device-driven LM loop whose damping is already known (every slot but the first of an
// optimize()): (re)linearise the chunk if the last trial was accepted, then eliminate its landmarks at the current
// lambda -- ONE kernel, one pass over the chunk's edges: the edge blocks W and the landmark sums go from the
// linearisation to the Schur phase in registers, the LDS is reused.  With d.persist the workgroup walks the chunks of
// its GROUP one after the other and leaves one pair of slabs: 12 instead of 79 per C3 window (the slabs were 83 of the
// 181 MB a 64-window launch moved, and what the reductions re-read).
template <int JAC>
__device__ __forceinline__ void k_lin_schur_entry(const BaDev& d, int bx)
{
  extern __shared__ __attribute__((aligned(16))) char fused_smem[];
  const double stop = d.scal[SC_STOP], curd = d.scal[SC_CUR], lambda = d.scal[SC_LAMBDA], needlin = d.scal[SC_NEEDLIN];
  ChunkLists cl;
  chunk_lists_load(d, bx, fused_smem, true, cl);                   // issued beside the state words, not after them
  if (stop != 0.0) return;
  const int cur = (int)curd;
  double* lslab = d.lin_slab + (size_t)bx * d.lin_stride;
  double* sslab = d.schur_slab + (size_t)bx * (d.nBlk * 36 + d.nP * 6);
  if (needlin != 0.0) {
    double W[18], lm[9];
    int erw = 0;
#pragma unroll
    for (int k = 0; k < 18; ++k) W[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) lm[k] = 0.0;
    k_linearize_body<JAC>(d, bx, cur, fused_smem, cl, W, lm, &erw, lslab);
    __syncthreads();                                               // the linearisation's LDS is dead: the Schur phase takes it over
    k_schur_body(d, bx, cur, lambda, fused_smem, cl, W, lm, &erw, sslab);
  } else {
    k_schur_body(d, bx, cur, lambda, fused_smem, cl, nullptr, nullptr, nullptr, sslab);
  }
}
template <int JAC>
__global__ __launch_bounds__(CH, SSX_LS_WGS) void k_lin_schur(BaDev d) { k_lin_schur_entry<JAC>(d, blockIdx.x); }
template <int JAC>
__global__ __launch_bounds__(CH, SSX_LS_WGS) void k_lin_schur_b(const BaDev* __restrict__ dv)
{
  const BaDev& d = dv[blockIdx.y];
  if ((int)blockIdx.x >= d.nCh) return;
  k_lin_schur_entry<JAC>(d, blockIdx.x);
}

// slabs -> dense reduced system WITHOUT lambda:  S = Hpp - sum(schur),  bs = bp - sum(c).
// 64 entries x 4 lane groups per workgroup (slab_sum_masked), the four parts added in part order: deterministic.
// OWN_LIN: the entry's share of Hpp / bp is summed HERE from the linearisation's slabs, with the grouping and the order of
// k_reduce_lin (the same value to the last bit), instead of being read from k_reduce_lin's output -- the two reductions then do
// not depend on each other and run as ONE launch (k_reduce_both: one launch boundary less per LM slot).
template <bool OWN_LIN>
__device__ __forceinline__ void k_reduce_schur_body(const BaDev& d, const int bx)
{
  __shared__ double sAcc[3][64];
  __shared__ double sAccL[3][64];
  __shared__ unsigned int sMask[MASK_TILE * TOUCH_WORDS];
  const int nS = d.nBlk * 36;
  const int stride = nS + d.nP * 6;
  const int n = 6 * d.nP;
  const int t = threadIdx.x;
  const int ent = bx * 64 + (t & 63), grp = t >> 6;
  const int bit = ent < nS ? ent / 36 : d.nBlk + (ent - nS) / 6;
  // my entry of the linearisation's slabs (pose p, entry k of its 27): the diagonal blocks' entries and the right-hand side
  int lin_ent = -1, lin_pose = 0;
  if (OWN_LIN && ent < stride) {
    if (ent < nS) {
      const int blk = ent / 36, rc = ent - blk * 36;
      const int r = rc / 6, cc = rc - r * 6;
      const int pa = d.blk_pa[blk];
      if (pa == d.blk_pb[blk]) {
        const int rr = r < cc ? r : cc, c2 = r < cc ? cc : r;
        lin_pose = pa;
        lin_ent = pa * 27 + rr * 6 - (rr * (rr - 1)) / 2 + (c2 - rr);
      }
    } else {
      const int j = ent - nS;
      lin_pose = j / 6;
      lin_ent = lin_pose * 27 + UPPER6 + (j - 6 * lin_pose);
    }
  }
  double acc = 0.0, accl = 0.0;
  for (int cb = 0; cb < d.nCh; cb += MASK_TILE) {
    if (cb) __syncthreads();
    stage_masks(d, cb, sMask);
    __syncthreads();
    if (ent < stride) acc = slab_sum_masked(d, d.schur_slab + ent, stride, grp, bit, cb, sMask, acc);
    if (OWN_LIN && lin_ent >= 0) accl = slab_sum_masked(d, d.lin_slab + lin_ent, d.nP * 27 + 2, grp, d.nBlk + lin_pose, cb, sMask, accl);
  }
  if (grp > 0) { sAcc[grp - 1][t & 63] = acc; if (OWN_LIN) sAccL[grp - 1][t & 63] = accl; }
  __syncthreads();
  if (grp != 0 || ent >= stride) return;
  acc = ((acc + sAcc[0][t]) + sAcc[1][t]) + sAcc[2][t];
  if (OWN_LIN) accl = ((accl + sAccL[0][t]) + sAccL[1][t]) + sAccL[2][t];
  double* S = d.trial_comm;
  double* bs = d.trial_comm + (size_t)n * n;
  if (ent < nS) {
    const int blk = ent / 36, rc = ent - blk * 36;
    const int r = rc / 6, cc = rc - r * 6;
    const int pa = d.blk_pa[blk], pb = d.blk_pb[blk];
    double h = 0.0;
    if (pa == pb) {
      const int rr = r < cc ? r : cc, c2 = r < cc ? cc : r;
      const int k = rr * 6 - (rr * (rr - 1)) / 2 + (c2 - rr);   // index of (rr,c2) in the 21-entry upper layout
      h = OWN_LIN ? accl : d.Hpp[pa * UPPER6 + k];
    }
    const double v = h - acc;
    S[(size_t)(6 * pa + r) * n + 6 * pb + cc] = v;
    if (pa != pb) S[(size_t)(6 * pb + cc) * n + 6 * pa + r] = v;
  } else {
    const int j = ent - nS;
    bs[j] = (OWN_LIN ? accl : d.bp[j]) - acc;
  }
}

__global__ __launch_bounds__(CH) void k_reduce_schur(BaDev d) { k_reduce_schur_body<false>(d, blockIdx.x); }
// both reductions of an LM slot in one launch: blocks [0, n_rl) reduce the linearisation's slabs, the others the Schur slabs
__global__ __launch_bounds__(CH) void k_reduce_both(BaDev d, int n_rl)
{
  if ((int)blockIdx.x < n_rl) k_reduce_lin_body(d, blockIdx.x);
  else k_reduce_schur_body<true>(d, blockIdx.x - n_rl);
}
__global__ __launch_bounds__(CH) void k_reduce_both_b(const BaDev* __restrict__ dv, int max_rl)
{
  const BaDev& d = dv[blockIdx.y];
  if ((int)blockIdx.x < max_rl) {
    if ((int)blockIdx.x >= ((d.nP * 27 + 63) / 64 > 0 ? (d.nP * 27 + 63) / 64 : 1)) return;
    k_reduce_lin_body(d, blockIdx.x);
  } else {
    const int bx = (int)blockIdx.x - max_rl;
    if (bx >= ((d.nBlk * 36 + d.nP * 6 + 63) / 64)) return;
    k_reduce_schur_body<true>(d, bx);
  }
}
// batched: blockIdx.y = window; every window brings its own BaDev (device array)
__global__ __launch_bounds__(CH) void k_reduce_schur_b(const BaDev* __restrict__ dv)
{
  const BaDev& d = dv[blockIdx.y];       // by reference: a private copy of the 500-byte struct ends up in scratch memory
  if ((int)blockIdx.x >= ((d.nBlk * 36 + d.nP * 6 + 63) / 64)) return;
  k_reduce_schur_body<false>(d, blockIdx.x);
}

// (the reduced solve of a small window -- k_solve64 for <= 10 free keyframes, k_solve80 for 11 .. 13, k_solve for 14 .. 16
// -- is k_solve_tiles in ba_big.inc)

// ------------------------------------------------------------------------------------------------
// k_backsub_residual: landmark back-substitution (block_solver.hpp:422-442), landmark update, and the
// residuals / robust chi2 of the TRIAL state (computeActiveErrors + activeRobustChi2,
// sparse_optimizer.cpp:63-116).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void k_backsub_residual_body(const BaDev& d, const int bx, int finish)
{
  __shared__ double sPt[3][CH];
  __shared__ double sPart[3][CH];
  __shared__ double sRed[CH];
  const int c = bx, t = threadIdx.x;
  if (d.scal[SC_STOP] != 0.0) return;                             // device-driven LM, already terminated
  const int cur = (int)d.scal[SC_CUR];
  const double lambda = d.scal[SC_LAMBDA];
  const int4 cd = d.ch_desc[c];
  const int e0 = cd.x, ne = cd.y, lm0 = cd.z, nl = cd.w;
  const double* pt_src = d.point[cur];
  double* pt_dst = d.point[cur ^ 1];
  int4 er4 = make_int4(0, -1, 0, 0);
  if (t < ne) er4 = d.e_rec[e0 + t];
  // W_e^T x_p of every edge (one thread per edge: the 18 component loads are coalesced), summed per landmark below
  if (t < ne) {
    const int e = e0 + t;
    const int pf = er4.y;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
    if (pf >= 0) {
      double Wr[18];
      if (d.store_w) {
#pragma unroll
        for (int k = 0; k < 18; ++k) Wr[k] = d.W[(size_t)k * d.E + e];
      } else {
        edge_W(d, cur, e, Wr);
      }
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double xa = d.xp[pf * 6 + a];
        p0 = fma(Wr[a * 3], xa, p0);
        p1 = fma(Wr[a * 3 + 1], xa, p1);
        p2 = fma(Wr[a * 3 + 2], xa, p2);
      }
    }
    sPart[0][t] = p0; sPart[1][t] = p1; sPart[2][t] = p2;
  }
  __syncthreads();
  double scale_l = 0.0;
  if (t < nl) {
    const int lc = lm0 + t;
    const int4 lr = d.l_rec[lc];
    const int lid = lr.z;
    double X[3] = {pt_src[lid * 3], pt_src[lid * 3 + 1], pt_src[lid * 3 + 2]};
    if (!lr.w) {
      double D[6], Di[9];
#pragma unroll
      for (int k = 0; k < 6; ++k) D[k] = d.Hll[(size_t)k * d.nLm + lc];
      D[0] += lambda; D[3] += lambda; D[5] += lambda;
      ssx::inv3_sym(D, Di);
      const double b[3] = {d.bl[lc], d.bl[(size_t)d.nLm + lc], d.bl[(size_t)2 * d.nLm + lc]};
      double cl[3] = {b[0], b[1], b[2]};
      for (int j = lr.x; j < lr.x + lr.y; ++j) { cl[0] -= sPart[0][j]; cl[1] -= sPart[1][j]; cl[2] -= sPart[2][j]; }
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double xl = Di[r * 3] * cl[0] + Di[r * 3 + 1] * cl[1] + Di[r * 3 + 2] * cl[2];
        scale_l += xl * (lambda * xl + b[r]);
        X[r] += xl;
      }
    }
    pt_dst[lid * 3] = X[0]; pt_dst[lid * 3 + 1] = X[1]; pt_dst[lid * 3 + 2] = X[2];
    sPt[0][t] = X[0]; sPt[1][t] = X[1]; sPt[2][t] = X[2];
  }
  __syncthreads();
  double rho0 = 0.0, nout = 0.0;
  if (t < ne) {
    const int e = e0 + t;
    const int p = er4.x;
    const int l = (er4.w >> 8) & 0xFF;
    const double* pose = d.pose[cur ^ 1];
    double T[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) T[k] = pose[p * 7 + k];
    const double X[3] = {sPt[0][l], sPt[1][l], sPt[2][l]};
    double er[2], p1[3], pc[3], w;
    ssx::edge_error(T, X, d.ext + 7 * (er4.w & 1), d.K, d.e_uv[e], d.e_uv[d.E + e], er, p1, pc);
    if (!d.no_err) {
      d.err_trial[e] = er[0];
      d.err_trial[d.E + e] = er[1];
    }
    const double c2 = er[0] * er[0] + er[1] * er[1];
    ssx::huber(c2, d.huber_delta, rho0, w);
    if (er4.y < 0 && (er4.w & 4)) rho0 = 0.0;                        // inactive edge (all vertices fixed)
    nout = (c2 > d.chi2_th) ? 1.0 : 0.0;
  }
  double chi = rho0, sl = scale_l, no = nout, unused_max = 0.0;
  block_sum3_max_256(chi, sl, no, unused_max, sRed);
  if (!finish) {
    if (t == 0) {
      d.trial_slab[c * 3] = chi;
      d.trial_slab[c * 3 + 1] = sl;
      d.trial_slab[c * 3 + 2] = no;
    }
    return;
  }
  // finish (device-driven LM on one GPU): the LAST chunk to get here sums the chunks' contributions -- in the fixed order of
  // k_reduce_trial: same bits whichever chunk it is -- and takes the LM decision; the launch of k_reduce_trial and its boundary
  // (7 us of a 60 us slot of one window) are gone.
  // ORDERING.  Formally a release on the ticket + an acquire in the last chunk would do; at agent scope on gfx942 / gfx950 they
  // compile to buffer_wbl2 sc1 / buffer_inv sc1 -- the XCD's whole L2 written back per chunk (it holds the landmarks and errors this
  // kernel just wrote): measured 233 instead of 42 us per launch in round 2.  Only three doubles per chunk have to be visible, so
  // they leave as agent-scope atomic stores (global_store ... sc1: written through to memory, coherent across the XCDs' L2s), the
  // ticket is taken once the memory system has ACKNOWLEDGED them (s_waitcnt vmcnt(0): on gfx9 vmcnt counts stores as well -- gfx10+
  // moved them to vscnt, hence the static_assert), and the last chunk reads them with agent-scope atomic loads, which the
  // workgroup barrier behind the ticket orders after it.  tests/test_ba_gpu.py::test_trial_finish_litmus compares ~10 000
  // launches x 128 windows with the k_reduce_trial path bit for bit, also with the library built at -O1.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__GFX9__)
  static_assert(false, "k_backsub_residual's trial finish relies on gfx9's vmcnt covering stores");
#endif
  __shared__ int sLast;
  double* slab = d.trial_slab.p;
  if (t == 0) {
    __hip_atomic_store(&slab[c * 3], chi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&slab[c * 3 + 1], sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&slab[c * 3 + 2], no, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int prev = __hip_atomic_fetch_add(d.ticket.p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sLast = prev + 1u == (unsigned int)d.nCh;
  }
  __syncthreads();
  if (!sLast) return;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int cc = t; cc < d.nCh; cc += CH) {
    a0 += __hip_atomic_load(&slab[cc * 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a1 += __hip_atomic_load(&slab[cc * 3 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a2 += __hip_atomic_load(&slab[cc * 3 + 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();                                   // (sRed is reused)
  a0 = block_sum_256(a0, sRed);
  a1 = block_sum_256(a1, sRed);
  a2 = block_sum_256(a2, sRed);
  if (t == 0) {
    d.scal_comm[0] = a0; d.scal_comm[1] = a1; d.scal_comm[2] = a2;
    d.scal[SC_TEMP_CHI] = a0; d.scal[SC_SCALE_L] = a1; d.scal[SC_NOUT] = a2;
    *d.ticket.get() = 0u;                            // (for the next trial; ordered by the kernel boundary)
    lm_step(d);
  }
}

__global__ __launch_bounds__(CH) void k_backsub_residual(BaDev d, int finish) { k_backsub_residual_body(d, blockIdx.x, finish); }
// batched: blockIdx.y = window; every window brings its own BaDev (device array)
__global__ __launch_bounds__(CH) void k_backsub_residual_b(const BaDev* __restrict__ dv, int finish)
{
  const BaDev& d = dv[blockIdx.y];       // by reference: a private copy of the 500-byte struct ends up in scratch memory
  if ((int)blockIdx.x >= (d.nCh)) return;
  k_backsub_residual_body(d, blockIdx.x, finish);
}

__device__ __forceinline__ void k_reduce_trial_body(const BaDev& d, const int bx, int lm)
{
  __shared__ double sRed[CH];
  double chi = 0.0, sl = 0.0, no = 0.0;
  for (int c = threadIdx.x; c < d.nCh; c += CH) {
    chi += d.trial_slab[c * 3];
    sl += d.trial_slab[c * 3 + 1];
    no += d.trial_slab[c * 3 + 2];
  }
  chi = block_sum_256(chi, sRed);
  sl = block_sum_256(sl, sRed);
  no = block_sum_256(no, sRed);
  if (threadIdx.x == 0) {
    d.scal_comm[0] = chi;
    d.scal_comm[1] = sl;
    d.scal_comm[2] = no;
    // single GPU: these are final (with a collective hook k_publish_trial copies the all-reduced values)
    d.scal[SC_TEMP_CHI] = chi;
    d.scal[SC_SCALE_L] = sl;
    d.scal[SC_NOUT] = no;
    if (lm) lm_step(d);                            // device-driven LM on one GPU: the trial is complete here
  }
}

__global__ __launch_bounds__(CH) void k_reduce_trial(BaDev d, int lm) { k_reduce_trial_body(d, blockIdx.x, lm); }
// batched: blockIdx.y = window; every window brings its own BaDev (device array)
__global__ __launch_bounds__(CH) void k_reduce_trial_b(const BaDev* __restrict__ dv, int lm)
{
  const BaDev& d = dv[blockIdx.y];       // by reference: a private copy of the 500-byte struct ends up in scratch memory
  if ((int)blockIdx.x >= (1)) return;
  k_reduce_trial_body(d, blockIdx.x, lm);
}

// copy the (all-reduced) trial scalars next to the others so that ONE 64-byte download returns everything
__global__ void k_publish_trial(BaDev d)
{
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    d.scal[SC_TEMP_CHI] = d.scal_comm[0];
    d.scal[SC_SCALE_L] = d.scal_comm[1];
    d.scal[SC_NOUT] = d.scal_comm[2];
    lm_step(d);                                    // every rank takes the same decision from the all-reduced scalars
  }
}

// ---- batched small windows (ssx_ba_solve_batch): per-window control words live in one int array [3 n] = cur | nstat | stop
__global__ __launch_bounds__(64) void k_lm_begin_batch(const BaDev* __restrict__ dv, const int* ctrl, int n, int iters)
{
  const int w = blockIdx.x;
  if (w >= n) return;
  const BaDev& d = dv[w];
  k_lm_begin_body(d, 0, ctrl[w], iters, ctrl[n + w], ctrl[2 * n + w]);
}

// after the upload of a batch: the second state buffer (and a resident batch's pristine copy) from the uploaded one
__global__ __launch_bounds__(CH) void k_dup_state_b(const BaDev* __restrict__ dv)
{
  const BaDev& d = dv[blockIdx.y];
  const size_t nP7 = 7 * (size_t)d.P, nL3 = 3 * (size_t)d.L;
  double* pi = const_cast<double*>(static_cast<const double*>(d.pose_init.p));
  double* qi = const_cast<double*>(static_cast<const double*>(d.point_init.p));
  for (size_t i = (size_t)blockIdx.x * CH + threadIdx.x; i < nP7 + nL3; i += (size_t)gridDim.x * CH) {
    if (i < nP7) { const double v = d.pose[0][i]; d.pose[1][i] = v; if (pi) pi[i] = v; }
    else { const double v = d.point[0][i - nP7]; d.point[1][i - nP7] = v; if (qi) qi[i - nP7] = v; }
  }
}

// a resident batch is solved again: both state buffers of every window back to the uploaded state
__global__ __launch_bounds__(CH) void k_reset_state_b(const BaDev* __restrict__ dv)
{
  const BaDev& d = dv[blockIdx.y];       // by reference: a private copy of the 500-byte struct ends up in scratch memory
  const size_t nP7 = 7 * (size_t)d.P, nL3 = 3 * (size_t)d.L;
  for (size_t i = (size_t)blockIdx.x * CH + threadIdx.x; i < nP7 + nL3; i += (size_t)gridDim.x * CH) {
    if (i < nP7) { const double v = d.pose_init[i]; d.pose[0][i] = v; d.pose[1][i] = v; }
    else { const double v = d.point_init[i - nP7]; d.point[0][i - nP7] = v; d.point[1][i - nP7] = v; }
  }
}

// control blocks (what = 0: SC_N scalars) or LM statistics (what = 1: 3 x SSX_BA_MAX_STATS) of every window, contiguous
__global__ __launch_bounds__(CH) void k_gather_scal_b(const BaDev* __restrict__ dv, int n, double* out, int what)
{
  const int w = blockIdx.x;
  if (w >= n) return;
  const BaDev& d = dv[w];
  const int cnt = what ? 3 * SSX_BA_MAX_STATS : SC_N;
  const double* src = what ? d.lm_stat : d.scal;
  for (int i = threadIdx.x; i < cnt; i += CH) out[(size_t)w * cnt + i] = src[i];
}

// results of every window into one contiguous buffer (one download): [poses 7P | points 3L | errors 2E] at out_off[w]
__global__ __launch_bounds__(CH) void k_pack_out_b(const BaDev* __restrict__ dv, const int* ctrl, int n, const size_t* out_off, double* out, int want_err)
{
  const int w = blockIdx.y;
  const BaDev& d = dv[w];
  const int cur = ctrl[w], trial_err = ctrl[n + w];
  double* o = out + out_off[w];
  const size_t nP7 = 7 * (size_t)d.P, nL3 = 3 * (size_t)d.L, nE2 = want_err ? 2 * (size_t)d.E : 0;
  const double* err = trial_err ? (const double*)d.err_trial : (const double*)d.err_lin;
  for (size_t i = (size_t)blockIdx.x * CH + threadIdx.x; i < nP7 + nL3 + nE2; i += (size_t)gridDim.x * CH) {
    double v;
    if (i < nP7) v = d.pose[cur][i];
    else if (i < nP7 + nL3) v = d.point[cur][i - nP7];
    else if (!d.dev_prep) v = err[i - nP7 - nL3];
    else {
      // device-marshalled window: chi2 per edge at the CALLER's index (the first E of the 2 E slots are used)
      const size_t sidx = i - nP7 - nL3;
      if (sidx >= (size_t)d.E) continue;
      const double a = err[sidx], b = err[(size_t)d.E + sidx];
      o[nP7 + nL3 + d.perm[sidx]] = chi2_of(a, b);
      continue;
    }
    o[i] = v;
  }
}

// a packed block of results from HBM into pinned host memory, 16 bytes per lane and step (full-width PCIe writes)
__global__ __launch_bounds__(CH) void k_stream_out(const double* __restrict__ src, double* __restrict__ dst, size_t n)
{
  const size_t n2 = n / 2;
  const double2* s2 = reinterpret_cast<const double2*>(src);
  double2* d2 = reinterpret_cast<double2*>(dst);
  for (size_t i = (size_t)blockIdx.x * CH + threadIdx.x; i < n2; i += (size_t)gridDim.x * CH) d2[i] = s2[i];
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) dst[n - 1] = src[n - 1];
}

// ONE window's control block, LM statistics and current estimate into pinned host memory, straight from the kernel (the single-window
// path's three downloads -- state words, statistics, poses + landmarks -- each cost a copy and a stream synchronisation of their own:
// ~25 us of host round trip apiece in a 0.74 ms solve).  Enqueued behind the last slot of an optimize(): `cur` is read on the device.
__global__ __launch_bounds__(CH) void k_pack_one(BaDev d, double* __restrict__ hscal, double* __restrict__ hpose, double* __restrict__ hpoint)
{
  const int cur = (int)d.scal[SC_CUR];
  const size_t n0 = SC_N, n1 = n0 + 3 * SSX_BA_MAX_STATS, n2 = n1 + 7 * (size_t)d.P, n3 = n2 + 3 * (size_t)d.L;
  for (size_t i = (size_t)blockIdx.x * CH + threadIdx.x; i < n3; i += (size_t)gridDim.x * CH) {
    if (i < n0) hscal[i] = d.scal[i];
    else if (i < n1) hscal[i] = d.lm_stat[i - n0];                     // (the statistics sit behind the control block in the pinned buffer)
    else if (i < n2) hpose[i - n1] = d.pose[cur][i - n1];
    else hpoint[i - n2] = d.point[cur][i - n2];
  }
}

// the keyframe poses of every window only (what a backend that reads its landmarks lazily needs back per keyframe): [n][7 maxP]
__global__ __launch_bounds__(CH) void k_pack_poses_b(const BaDev* __restrict__ dv, const int* ctrl, int n, int maxP, double* out)
{
  const int w = blockIdx.x;
  if (w >= n) return;
  const BaDev& d = dv[w];
  const double* src = d.pose[ctrl ? ctrl[w] : (int)d.scal[SC_CUR]];   // (no host word: the state buffer the window's own LM loop ended on)
  for (int i = threadIdx.x; i < 7 * d.P; i += CH) out[(size_t)w * 7 * maxP + i] = src[i];
}

#include "ba_big.inc"
#include "ba_band.inc"
#include "ba_bcr.inc"

}  // namespace

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace {
// 1: round 3's dense slabs (every chunk writes and the reductions read every entry), the cross-check of the sparse form;
// SSX_BA_DENSE_SLABS=1 in the environment or ssx_debug_set_dense_slabs
std::atomic<int> g_dense_slabs{-1};
// 0: the trial's three sums are added by a launch of k_reduce_trial (rounds 1-4) instead of by the last chunk of k_backsub_residual:
// the cross-check of the ticket protocol (ssx_debug_set_trial_finish; same bits either way)
std::atomic<int> g_trial_finish{1};
inline int dense_slabs_mode()
{
  int m = g_dense_slabs.load(std::memory_order_relaxed);
  if (m < 0) {
    m = getenv("SSX_BA_DENSE_SLABS") ? 1 : 0;
    g_dense_slabs.store(m, std::memory_order_relaxed);
  }
  return m;
}
struct HostPrep {
  int P, L, E, nP, nLm, nCh, nBlk;
  int E_raw = 0;                     // entries of the caller's edge arrays (E of them alive; see BaDev::E_raw)
  int raw_fmt = 0;                   // BaDev::raw_fmt of the blob this window is uploaded in
  std::vector<int> pose_free, lm_id, lm_ptr, ch_lm, e_pose, e_lmc, perm, pair_ptr;
  std::vector<uint8_t> lm_fixed, e_cam, e_dup, pair_a, pair_b;
  std::vector<uint16_t> pptr;
  std::vector<double> e_uv;
  std::vector<int8_t> blk_pa, blk_pb;
  // large-window path
  bool big = false;
  std::vector<int> pe_ptr, pe_edge, sblk_pa, sblk_pb, spair_ptr;
  std::vector<int> bseg, bseg_ptr;   // see BaDev
  std::vector<int> thr_cnt, thr_pe;  // prepare() of a large window on several threads: per-thread landmark / pose counts
  std::vector<unsigned int> touch;   // host-built lists only: BaDev::touch
  bool dev_lists = false;            // small window: pair lists + work items are built by k_build_lists, not here
  bool dev_prep = false;             // small window: the edge sort by (landmark, pose), the packed records, the pose-major order and the
                                     // sorted uv columns are built ON THE DEVICE (k_prep_scatter / k_prep_chunk) from the caller's raw
                                     // arrays; the host only counts (slot8: rank of an edge among its landmark's edges in caller order)
  std::vector<uint8_t> slot8;
  std::vector<int> lm_compact;       // caller's landmark -> compact landmark or -1
  std::vector<int> pose_rank;        // empty, or BaDev::pose_rank (a window's keyframes in the order of their ids)
  std::vector<int> cnt_tmp, start_tmp, first_pf_tmp, visit_tmp, visit2_tmp;
  std::vector<uint32_t> tmp_pairs;   // scratch of prepare(), kept between calls
  std::vector<std::pair<int, int>> tmp_order;
  std::vector<int> ch_desc, e_rec, l_rec;   // packed records (4 ints each), see BaDev
  std::vector<int> lm_chunk;                // compact landmark -> chunk (large windows: the device-side pair builder)
  int band_w = -1;          // cyclic block bandwidth of this rank's part of the reduced system (max over its non-zero blocks)
};
}  // namespace

// upper bound of the host threads a batched call spreads its per-window work over (SSX_HOST_THREADS overrides it)
static int host_threads_cap()
{
  static const int cap = [] { const char* e = getenv("SSX_HOST_THREADS"); const int v = e ? atoi(e) : 0; return v > 0 ? std::min(v, 128) : 16; }();
  return cap;
}

// A few persistent host threads for the per-window host work of a batched call (staging copies, result unpacking): created
// on first use, parked on a condition variable between calls (the former code spawned up to 16 std::threads twice per call).
class ParPool {
 public:
  ~ParPool()
  {
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; ++gen_; }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  // fn(w) for w in [0, n) on at least T threads when the pool has them (the caller is one of them; threads created by an earlier,
  // wider call join in as well); returns when all are done.
  // The per-window pieces of a batched call are SHORT (a 10 KB copy, a counting pass over 2 000 observations) and a call runs five
  // such phases back to back: items are claimed in runs (one lock per run, not two per item -- 258 copies of 10 KB took 0.28 ms,
  // most of it on the mutex: 0.12 - 0.16 now).  Idle workers park on the condition variable (polling before they park measured no
  // gain in the headline region: profiles/r06/host_pool_ab.txt).
  template <class F>
  void run(int n, int T, F&& fn)
  {
    if (T <= 1 || n <= 1) { for (int w = 0; w < n; ++w) fn(w); return; }
    std::function<void(int)> f = fn;
    {
      std::unique_lock<std::mutex> lk(mu_);
      while ((int)th_.size() < T - 1) th_.emplace_back([this] { loop(); });
      job_ = &f; n_ = n; next_ = 0; pending_ = n;
      grain_ = std::max(1, n / (4 * (int)(th_.size() + 1)));
      ++gen_;
    }
    cv_.notify_all();
    work();
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [this] { return pending_ == 0; });
    job_ = nullptr;
  }

 private:
  void work()
  {
    for (;;) {
      int w0, w1;
      const std::function<void(int)>* f;
      {
        std::lock_guard<std::mutex> lk(mu_);
        if (!job_ || next_ >= n_) return;
        w0 = next_; w1 = std::min(n_, next_ + grain_); next_ = w1; f = job_;
      }
      for (int w = w0; w < w1; ++w) (*f)(w);
      std::lock_guard<std::mutex> lk(mu_);
      pending_ -= w1 - w0;
      if (pending_ == 0) done_cv_.notify_all();
    }
  }
  void loop()
  {
    unsigned long seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = gen_;
      }
      work();
    }
  }
  std::mutex mu_;                        // guards every member below
  std::condition_variable cv_, done_cv_;
  std::vector<std::thread> th_;
  const std::function<void(int)>* job_ = nullptr;
  int n_ = 0, next_ = 0, pending_ = 0, grain_ = 1;
  unsigned long gen_ = 0;                // one more per job: wakes the parked workers
  bool stop_ = false;
};

// ssx_ba_device_turns: the device phases of batched solves of DIFFERENT contexts run one after the other on the device (FIFO).
// A batched solve is a host phase (pending uploads, counting tables, marshalling) followed by a device phase (the LM slots of a
// round, enqueued at once, one synchronisation behind them).  Two host threads that drive two contexts side by side fall into lock
// step when their device phases interleave on the chip -- both end together, both threads then sit in their host phases with the
// device idle.  With turns a round's kernels WAIT (hipStreamWaitEvent, on the device) for the end of the round that was enqueued
// before it, whichever context that was: nothing is serialised on the host but the enqueueing itself, one context's kernels finish
// early, and its host phase lies beside the other's kernels.
class DeviceTurns {
 public:
  void enable(bool on) { on_.store(on, std::memory_order_relaxed); }
  bool enabled() const { return on_.load(std::memory_order_relaxed); }
  // ONE chain (mutex, last event) PER DEVICE: contexts on different GPUs never wait for each other, on the host or on the device.
  // (mutex held from begin to end: the rounds of the contexts of one device are enqueued one after the other, in the order of the chain)
  void begin(const void* owner, int device, hipStream_t s)
  {
    Chain& c = chain(device);
    c.mu.lock();
    if (c.last && c.owner != owner && hipStreamWaitEvent(s, c.last, 0) != hipSuccess) {
      (void)hipGetLastError();                       // the chain is broken: this round runs unordered, the next one starts a new chain
      c.last = nullptr; c.owner = nullptr;
    }
  }
  void end(const void* owner, int device, hipEvent_t ev, hipStream_t s)
  {
    Chain& c = chain(device);
    if (ev && hipEventRecord(ev, s) == hipSuccess) { c.last = ev; c.owner = owner; }
    else { (void)hipGetLastError(); c.last = nullptr; c.owner = nullptr; }
    c.mu.unlock();
  }
  void forget(const void* owner)                       // the owner's event is about to be destroyed
  {
    for (Chain& c : chains_) {
      std::lock_guard<std::mutex> lk(c.mu);
      if (c.owner == owner) { c.last = nullptr; c.owner = nullptr; }
    }
  }
 private:
  struct Chain { std::mutex mu; hipEvent_t last = nullptr; const void* owner = nullptr; };
  static constexpr int MAX_DEV = 16;
  Chain& chain(int device) { return chains_[(device >= 0 && device < MAX_DEV) ? device : 0]; }
  std::atomic<bool> on_{false};
  Chain chains_[MAX_DEV];
};
static DeviceTurns g_turns;

struct BaWorkspace {
  DevBuf arena;      // everything on the device
  HostBuf stage;     // pinned upload / download staging
  HostBuf scal;      // pinned scalars read back per trial
  DevBuf tiles;      // large windows: tile-sparsity lists of the factor
  HostBuf tiles_h;
  DevBuf pairs_a, pairs_b, pairs_c;   // large windows: device-built pair lists (inputs + scan | sort buffers | final lists)
  HostBuf pairs_h;
  // host marshalling scratch, kept between calls (a ctx is single-threaded by contract, so one set per ctx: the former
  // thread_local copies lived as long as the calling thread -- ~100 MB per thread after a 64-window batch)
  HostPrep prep1;                     // ssx_ba_solve / ssx_ba_linearize
  std::vector<HostPrep> preps;        // batched calls: one per window, trimmed back after a large batch
  ParPool pool;
  DevBuf recs;                        // large windows, device-marshalled: raw inputs + the records / columns built from them
  HostBuf recs_h;
  // the caller's observation columns of a large window, sent BEFORE prepare() counts them (raw_upload_early): 12 MB at
  // BASELINE configs[3] cross PCIe beside the host's counting pass instead of after it
  DevBuf raw_d;
  HostBuf raw_h;
  struct RawEarly { bool valid = false; const void* key = nullptr; int E = 0; size_t o_pose = 0, o_point = 0, o_uv = 0, o_cam = 0; } raw_early;
  DevBuf win_stage_d;                 // ssx_ba_window: pending uploads of the windows of a call, one block (ba_window.inc)
  HostBuf win_stage_h;
  hipEvent_t ev_turn = nullptr;       // ssx_ba_device_turns: the end of this context's last device phase
};

static void ssx_ba_workspace_free(BaWorkspace* w)
{
  if (!w) return;
  g_turns.forget(w);
  if (w->ev_turn) (void)hipEventDestroy(w->ev_turn);
  w->arena.release();
  w->stage.release();
  w->scal.release();
  w->tiles.release();
  w->tiles_h.release();
  w->pairs_a.release(); w->pairs_b.release(); w->pairs_c.release(); w->pairs_h.release();
  w->win_stage_d.release(); w->win_stage_h.release();
  w->recs.release(); w->recs_h.release();
  delete w;
}

namespace {


// chunks of whole landmarks, <= CH_E edges and <= CH_L landmarks each (h.lm_ptr, h.nLm given)
void make_chunks(HostPrep& h)
{
  h.ch_lm.clear();
  h.ch_lm.push_back(0);
  int acc_e = 0, acc_l = 0;
  for (int lc = 0; lc < h.nLm; ++lc) {
    const int k = h.lm_ptr[lc + 1] - h.lm_ptr[lc];
    if (acc_e + k > CH_E || acc_l + 1 > CH_L) {
      h.ch_lm.push_back(lc);
      acc_e = 0; acc_l = 0;
    }
    acc_e += k; acc_l += 1;
  }
  if (h.nLm > 0) h.ch_lm.push_back(h.nLm);
  h.nCh = (int)h.ch_lm.size() - 1;
  if (h.nCh < 0) h.nCh = 0;
}

// A window whose raw observation arrays and state live in device buffers of their own (ssx_ba_window): upload() then sends
// only the counting tables, and the solve starts from / leaves its result in the window's state buffers.
struct WinExt {
  const int* r_edge_pose = nullptr; const int* r_edge_point = nullptr; const double* r_edge_uv = nullptr; const uint8_t* r_edge_cam = nullptr;
  double* pose[2] = {nullptr, nullptr}; double* point[2] = {nullptr, nullptr};
  int cur = 0;                       // in: the buffer that holds the current estimate; out: the one that holds the result
  // the order the solve gives its vertices: the window's live keyframe / landmark SLOTS sorted by the caller's ids (what g2o does
  // with its vertex ids, sparse_optimizer.cpp:305-330) -- free-pose indices, the order of a landmark's edges, the landmark order of
  // the chunks all follow it, so the bits of a solve do not depend on which slots the window happened to reuse
  const int* pose_order = nullptr; int n_pose_order = 0;
  const int* lm_order = nullptr; int n_lm_order = 0;
};

static int g_prep_threads_override = 0;   // test hook (ssx_ba_debug_prepare_digest): threads of the large-window observation pass

// allow_dev_prep: small windows leave everything beyond counting to the device (see HostPrep::dev_prep); SSX_BA_HOST_PREP=1
// keeps the host marshalling below as the reference of the tests (same bits: test_device_marshalling_equals_host_marshalling)
ssx_status prepare(ssx_ctx* ctx, const ssx_ba_problem* pr, HostPrep& h, bool allow_dev_prep = true, const WinExt* ext = nullptr)
{
  const bool dead_ok = ext != nullptr;
  const int P = pr->P, L = pr->L, E = pr->E;
  if (P <= 0 || L < 0 || E < 0 || !pr->poses || (L && !pr->points) ||
      (E && (!pr->edge_pose || !pr->edge_point || !pr->edge_uv))) {
    ctx->set_error("ssx_ba: invalid problem (P=%d L=%d E=%d or null arrays)", P, L, E);
    return SSX_ERR_INVALID_ARG;
  }
  h.P = P; h.L = L; h.E = E; h.E_raw = E;
  h.pose_free.assign(P, -1);
  h.nP = 0;
  h.pose_rank.clear();
  if (ext && ext->pose_order) {
    h.pose_rank.assign(P, P);                             // (dead slots: behind every live keyframe; nothing refers to them)
    for (int i = 0; i < ext->n_pose_order; ++i) {
      const int sl = ext->pose_order[i];
      h.pose_rank[sl] = i;
      if (!(pr->pose_fixed && pr->pose_fixed[sl])) h.pose_free[sl] = h.nP++;
    }
  } else
  for (int i = 0; i < P; ++i)
    if (!(pr->pose_fixed && pr->pose_fixed[i])) h.pose_free[i] = h.nP++;
  static const bool host_prep_env = getenv("SSX_BA_HOST_PREP") != nullptr;
  static const bool host_lists_env = getenv("SSX_BA_HOST_LISTS") != nullptr;
  h.big = h.nP > SSX_BA_SMALL_P;
  h.dev_prep = allow_dev_prep && !host_prep_env && !host_lists_env;
  // counting sort of the edges by landmark
  std::vector<int>& cnt = h.cnt_tmp;
  cnt.assign(L + 1, 0);
  std::vector<int>& first_pf = h.first_pf_tmp;            // per landmark: the first free pose (in free-pose order) that observes it
  first_pf.assign((size_t)L + 1, h.nP + 1);
  if (h.dev_prep) h.slot8.resize((size_t)std::max(E, 1));
  int n_dead = 0;
  const bool big_dev = h.big && h.dev_prep;               // large window, device-marshalled: the host also counts edges per free pose
  if (big_dev) h.pe_ptr.assign((size_t)h.nP + 1, 0);
  // The one pass over the observations.  A large window (480 000 observations at BASELINE configs[3]: 1.05 ms on one core, a sixth of
  // a 10-iteration solve) takes it on the worker pool: every thread counts its range into tables of its own (slot8 = the rank
  // inside the range), the per-landmark offsets of the ranges are summed landmark-parallel, a second pass adds them -- the same
  // ranks as the serial loop, whatever the number of threads.
  static const int prep_threads = [] { const char* e = getenv("SSX_BA_PREP_THREADS"); const int v = e ? atoi(e) : 0;
                                       return v > 0 ? std::min(v, 32) : std::min(32, std::max(std::min(8, std::max(1, (int)std::thread::hardware_concurrency())), (int)std::thread::hardware_concurrency() / 2)); }();   // (measured at configs[3] on a 256-core host: 1.70 / 1.27 / 0.74 ms of prepare() on 8 / 16 / 32 threads, profiles/r06/c4_prepare_threads.txt)
  const int T = (big_dev && !dead_ok && E >= (1 << 16) && ctx->ba) ? (g_prep_threads_override > 0 ? g_prep_threads_override : prep_threads) : 1;
  if (T > 1) {
    h.thr_cnt.resize((size_t)T * L); h.thr_pe.resize((size_t)T * (h.nP + 1));
    std::vector<int> bad(T, -1);
    auto lo = [&](int t, int n) { return (int)((long long)n * t / T); };
    ctx->ba->pool.run(T, T, [&](int t) {
      int* c = h.thr_cnt.data() + (size_t)t * L; int* pe = h.thr_pe.data() + (size_t)t * (h.nP + 1);
      std::fill(c, c + L, 0); std::fill(pe, pe + h.nP + 1, 0);
      for (int e = lo(t, E), e1 = lo(t + 1, E); e < e1; ++e) {
        const int l = pr->edge_point[e], p = pr->edge_pose[e];
        if (l < 0 || l >= L || p < 0 || p >= P) { bad[t] = e; return; }
        h.slot8[e] = (uint8_t)c[l];
        c[l]++;
        const int pf = h.pose_free[p];
        if (pf >= 0) pe[pf + 1]++;
      }
    });
    for (int t = 0; t < T; ++t)
      if (bad[t] >= 0) {
        ctx->set_error("ssx_ba: edge %d references pose %d / point %d out of range", bad[t], pr->edge_pose[bad[t]], pr->edge_point[bad[t]]);
        return SSX_ERR_INVALID_ARG;
      }
    ctx->ba->pool.run(T, T, [&](int t) {
      for (int l = lo(t, L), l1 = lo(t + 1, L); l < l1; ++l) {
        int run = 0;
        for (int tt = 0; tt < T; ++tt) { int& c = h.thr_cnt[(size_t)tt * L + l]; const int k = c; c = run; run += k; }
        cnt[l + 1] = run;
      }
    });
    ctx->ba->pool.run(T - 1, T - 1, [&](int t1) {
      const int t = t1 + 1;
      const int* c = h.thr_cnt.data() + (size_t)t * L;
      for (int e = lo(t, E), e1 = lo(t + 1, E); e < e1; ++e) h.slot8[e] = (uint8_t)(h.slot8[e] + c[pr->edge_point[e]]);
    });
    for (int t = 0; t < T; ++t)
      for (int p = 0; p < h.nP; ++p) h.pe_ptr[p + 1] += h.thr_pe[(size_t)t * (h.nP + 1) + p + 1];
  } else
  for (int e = 0; e < E; ++e) {
    const int l = pr->edge_point[e], p = pr->edge_pose[e];
    if (dead_ok && l < 0) { ++n_dead; continue; }           // a window's storage: observation of a removed keyframe
    if (l < 0 || l >= L || p < 0 || p >= P) {
      ctx->set_error("ssx_ba: edge %d references pose %d / point %d out of range", e, p, l);
      return SSX_ERR_INVALID_ARG;
    }
    if (h.dev_prep) h.slot8[e] = (uint8_t)cnt[l + 1];      // (a count beyond CH_E is reported below: the wrapped value is never used)
    cnt[l + 1]++;
    { const int pfk = h.pose_free[p] >= 0 ? h.pose_free[p] : h.nP; if (pfk < first_pf[l]) first_pf[l] = pfk; }
    if (big_dev) { const int pf = h.pose_free[p]; if (pf >= 0) h.pe_ptr[pf + 1]++; }
  }
  if (n_dead && !h.dev_prep) { ctx->set_error("ssx_ba: dead observations need the device-side marshalling"); return SSX_ERR_UNSUPPORTED; }
  h.E = E - n_dead;
  // Lossless narrowing of the raw arrays on their way across PCIe (26 -> 13 bytes per observation): pose indices as bytes,
  // landmark indices as 16-bit words, and the pixel coordinates as floats when every one of them IS a float's value -- the
  // reference's measurements are cv::KeyPoint::pt (Point2f) widened to double (frontend.cpp:232-236, backend.cpp:126-160).
  h.raw_fmt = 0;
  if (h.dev_prep && !h.big && !dead_ok) {
    if (P <= 256) h.raw_fmt |= 1;
    if (L <= 65536) h.raw_fmt |= 2;
    bool exact = true;
    const double* uvp = pr->edge_uv;
    for (size_t i = 0; i < 2 * (size_t)E; ++i) exact &= (double)(float)uvp[i] == uvp[i];
    if (exact) h.raw_fmt |= 4;
  }
  h.lm_id.clear(); h.lm_ptr.clear(); h.lm_fixed.clear();
  std::vector<int>& lm_compact = h.lm_compact;
  std::vector<int>& start = h.start_tmp;
  lm_compact.assign(L, -1); start.assign(L + 1, 0);
  // The compact order of the landmarks: the caller's order (a window: ascending ids), then -- stable -- by the FIRST free pose that
  // observes a landmark.  Map points are created keyframe by keyframe, so real windows arrive almost sorted already; what the
  // sort buys is locality for every input: the landmarks of a chunk then share their poses, a chunk contributes to 15-25 of the
  // 55 blocks of a 10-keyframe reduced system instead of all of them, and writes / the reductions read only those (BaDev::touch).
  const bool lm_ordered = ext && ext->lm_order;
  const int n_visit = lm_ordered ? ext->n_lm_order : L;
  std::vector<int>& visit = h.visit_tmp;
  visit.clear();
  for (int i = 0; i < n_visit; ++i) {
    const int l = lm_ordered ? ext->lm_order[i] : i;
    if (cnt[l + 1] == 0) continue;
    if (cnt[l + 1] > CH_E) {
      ctx->set_error("ssx_ba: landmark %d has %d observations (> %d per landmark unsupported)", l, cnt[l + 1], CH_E);
      return SSX_ERR_UNSUPPORTED;
    }
    visit.push_back(l);
  }
  if (!h.big) {
    std::vector<int>& out = h.visit2_tmp;
    int bucket[SSX_BA_SMALL_P + 3] = {0};
    for (int l : visit) bucket[first_pf[l] + 1]++;
    for (int b = 0; b < SSX_BA_SMALL_P + 2; ++b) bucket[b + 1] += bucket[b];
    out.resize(visit.size());
    for (int l : visit) out[bucket[first_pf[l]]++] = l;
    visit.swap(out);
  }
  int run = 0;
  for (int l : visit) {
    lm_compact[l] = (int)h.lm_id.size();
    h.lm_id.push_back(l);
    h.lm_ptr.push_back(run);
    run += cnt[l + 1];
    h.lm_fixed.push_back(pr->point_fixed ? (pr->point_fixed[l] ? 1 : 0) : 0);
  }
  if (run != E - n_dead) { ctx->set_error("ssx_ba_window: an observation refers to a landmark that is not in the window's order list"); return SSX_ERR_INVALID_ARG; }
  h.lm_ptr.push_back(h.E);
  h.nLm = (int)h.lm_id.size();
  if (h.dev_prep) {
    // ---- the light path: chunks + chunk descriptors + the block table; the device does the rest ----
    make_chunks(h);
    h.ch_desc.resize(4 * (size_t)std::max(h.nCh, 1));
    for (int c = 0; c < h.nCh; ++c) {
      const int lm0 = h.ch_lm[c], lm1 = h.ch_lm[c + 1], e0 = h.lm_ptr[lm0], e1 = h.lm_ptr[lm1];
      int* cd = &h.ch_desc[4 * (size_t)c];
      cd[0] = e0; cd[1] = e1 - e0; cd[2] = lm0; cd[3] = lm1 - lm0;
    }
    h.blk_pa.clear(); h.blk_pb.clear();
    h.band_w = -1;
    h.perm.clear(); h.pptr.clear(); h.pair_ptr.clear(); h.pair_a.clear(); h.pair_b.clear(); h.bseg.clear(); h.bseg_ptr.clear();
    h.pe_edge.clear(); h.sblk_pa.clear(); h.sblk_pb.clear(); h.spair_ptr.assign(1, 0);
    if (h.big) {
      if (h.nP > 2048) { ctx->set_error("ssx_ba: %d free poses exceed the supported 2048", h.nP); return SSX_ERR_UNSUPPORTED; }
      for (int p = 0; p < h.nP; ++p) h.pe_ptr[p + 1] += h.pe_ptr[p];   // counts -> offsets; the edge list itself is the device's (big_records)
      h.nBlk = 0;
      h.dev_lists = false;
      return SSX_OK;
    }
    h.pe_ptr.clear();
    for (int a = 0; a < h.nP; ++a)
      for (int b = a; b < h.nP; ++b) { h.blk_pa.push_back((int8_t)a); h.blk_pb.push_back((int8_t)b); }
    h.nBlk = (int)h.blk_pa.size();
    h.dev_lists = true;
    return SSX_OK;
  }
  h.perm.assign(E, 0);
  {
    std::vector<int> fill((size_t)L, 0);
    for (int l = 0; l < L; ++l) if (lm_compact[l] >= 0) fill[l] = h.lm_ptr[lm_compact[l]];
    for (int e = 0; e < E; ++e) h.perm[fill[pr->edge_point[e]]++] = e;
  }
  // inside a landmark: stable sort by pose so that duplicates of a (landmark,pose) pair are adjacent
  for (int lc = 0; lc < h.nLm; ++lc) {
    const int a = h.lm_ptr[lc], b = h.lm_ptr[lc + 1];
    bool sorted = true;
    for (int s = a + 1; s < b && sorted; ++s) sorted = pr->edge_pose[h.perm[s - 1]] <= pr->edge_pose[h.perm[s]];
    if (!sorted)
      std::stable_sort(h.perm.begin() + a, h.perm.begin() + b, [&](int x, int y) { return pr->edge_pose[x] < pr->edge_pose[y]; });
  }
  h.e_pose.resize(E); h.e_lmc.resize(E); h.e_cam.resize(E); h.e_dup.assign(E, 0); h.e_uv.resize(2 * (size_t)E);
  for (int s = 0; s < E; ++s) {
    const int e = h.perm[s];
    h.e_pose[s] = pr->edge_pose[e];
    h.e_lmc[s] = lm_compact[pr->edge_point[e]];
    h.e_cam[s] = pr->edge_cam ? (pr->edge_cam[e] ? 1 : 0) : 0;
    h.e_uv[s] = pr->edge_uv[2 * (size_t)e];
    h.e_uv[(size_t)E + s] = pr->edge_uv[2 * (size_t)e + 1];
    if (s > 0 && h.e_lmc[s] == h.e_lmc[s - 1] && h.e_pose[s] == h.e_pose[s - 1]) h.e_dup[s] = 1;
  }
  make_chunks(h);
  h.ch_desc.resize(4 * (size_t)std::max(h.nCh, 1)); h.e_rec.resize(4 * (size_t)std::max(E, 1)); h.l_rec.resize(4 * (size_t)std::max(h.nLm, 1));
  h.lm_chunk.resize((size_t)std::max(h.nLm, 1));
  for (int c = 0; c < h.nCh; ++c) {
    const int lm0 = h.ch_lm[c], lm1 = h.ch_lm[c + 1], e0 = h.lm_ptr[lm0], e1 = h.lm_ptr[lm1];
    int* cd = &h.ch_desc[4 * (size_t)c];
    cd[0] = e0; cd[1] = e1 - e0; cd[2] = lm0; cd[3] = lm1 - lm0;
    for (int lc = lm0; lc < lm1; ++lc) {
      h.lm_chunk[lc] = c;
      int* lr = &h.l_rec[4 * (size_t)lc];
      lr[0] = h.lm_ptr[lc] - e0; lr[1] = h.lm_ptr[lc + 1] - h.lm_ptr[lc]; lr[2] = h.lm_id[lc]; lr[3] = h.lm_fixed[lc];
      for (int s2 = h.lm_ptr[lc]; s2 < h.lm_ptr[lc + 1]; ++s2) {
        int* er = &h.e_rec[4 * (size_t)s2];
        er[0] = h.e_pose[s2]; er[1] = h.pose_free[h.e_pose[s2]]; er[2] = h.lm_id[lc];
        const int next_dup = (s2 + 1 < h.lm_ptr[lc + 1] && h.e_dup[s2 + 1]) ? 1 : 0;   // duplicates are of the same landmark
        er[3] = (int)h.e_cam[s2] | ((int)h.e_dup[s2] << 1) | ((int)h.lm_fixed[lc] << 2) | (next_dup << 3) |
                ((h.pose_free[h.e_pose[s2]] < 0 ? 1 : 0) << 5) | ((lc - lm0) << 8);
      }
    }
  }
  h.blk_pa.clear(); h.blk_pb.clear();
  if (h.nP <= SSX_BA_SMALL_P)
    for (int a = 0; a < h.nP; ++a)
      for (int b = a; b < h.nP; ++b) { h.blk_pa.push_back((int8_t)a); h.blk_pb.push_back((int8_t)b); }
  h.nBlk = (int)h.blk_pa.size();
  if (h.big) {
    const int nP = h.nP;
    if (nP > 2048) { ctx->set_error("ssx_ba: %d free poses exceed the supported 2048", nP); return SSX_ERR_UNSUPPORTED; }
    // pose-major edge list (free poses)
    h.pe_ptr.assign(nP + 1, 0);
    for (int s = 0; s < E; ++s) { const int pf = h.pose_free[h.e_pose[s]]; if (pf >= 0) h.pe_ptr[pf + 1]++; }
    for (int p = 0; p < nP; ++p) h.pe_ptr[p + 1] += h.pe_ptr[p];
    h.pe_edge.assign(std::max(h.pe_ptr[nP], 1), 0);
    {
      std::vector<int> fill(h.pe_ptr.begin(), h.pe_ptr.end() - 1);
      for (int s = 0; s < E; ++s) { const int pf = h.pose_free[h.e_pose[s]]; if (pf >= 0) h.pe_edge[fill[pf]++] = s; }
    }
    // the non-zero blocks of the reduced system and their (edge, edge) pair lists are built on the device (build_pairs)
    h.sblk_pa.clear(); h.sblk_pb.clear(); h.spair_ptr.assign(1, 0);
    h.nBlk = 0;
    h.band_w = -1;
    h.bseg.clear(); h.bseg_ptr.clear();
    h.dev_lists = false;
    return SSX_OK;
  }
  // per-chunk index lists: edges grouped by free pose; leader pairs grouped by reduced-system block
  h.dev_lists = !host_lists_env;                // (SSX_BA_HOST_LISTS: the host builder stays as the reference of the tests)
  const int nP = h.nP, nBlk = h.nBlk;
  h.pptr.assign((size_t)h.nCh * (nP + 1) + 1, 0);
  h.pair_ptr.assign((size_t)h.nCh * (nBlk + 1) + 1, 0);
  h.pair_a.clear(); h.pair_b.clear();
  h.bseg.clear(); h.bseg_ptr.assign(2 * (size_t)h.nCh + 2, 0);
  h.touch.assign(TOUCH_WORDS * (size_t)(h.nCh + 1), 0u);
  std::vector<int> blk_of((size_t)std::max(nP, 1) * std::max(nP, 1), -1);
  for (int b = 0; b < nBlk; ++b) blk_of[(size_t)h.blk_pa[b] * nP + h.blk_pb[b]] = b;
  std::vector<int> pc(nP + 1), bc(nBlk + 1);
  std::vector<uint32_t>& tmp_pairs = h.tmp_pairs;
  std::vector<std::pair<int, int>>& order = h.tmp_order;   // (-part length, block)
  h.bseg.reserve(4 * ((size_t)h.nCh * (nBlk + 8)));
  for (int c = 0; c < h.nCh; ++c) {
    const int lm0 = h.ch_lm[c], lm1 = h.ch_lm[c + 1];
    const int e0 = h.lm_ptr[lm0], e1 = h.lm_ptr[lm1];
    // --- by pose ---
    std::fill(pc.begin(), pc.end(), 0);
    for (int s = e0; s < e1; ++s) { const int pf = h.pose_free[h.e_pose[s]]; if (pf >= 0) pc[pf + 1]++; }
    for (int p = 0; p < nP; ++p) pc[p + 1] += pc[p];
    uint16_t* pp = &h.pptr[(size_t)c * (nP + 1)];
    for (int p = 0; p <= nP; ++p) pp[p] = (uint16_t)pc[p];
    int tail = pc[nP];
    for (int s = e0; s < e1; ++s) {
      const int pf = h.pose_free[h.e_pose[s]];
      const int pos = pf >= 0 ? pc[pf]++ : tail++;
      h.e_rec[4 * (size_t)s + 3] = (h.e_rec[4 * (size_t)s + 3] & 0xFFFF) | (pos << 16);   // the inverse map, for the kernels that store pose-major
    }
    if (h.dev_lists) continue;                    // k_build_lists (same lists, on the device)
    // --- pairs by block: one pass over the landmarks of the chunk lists (block, edge a, edge b), a counting sort by
    // block keeps the landmark order inside a block ---
    std::fill(bc.begin(), bc.end(), 0);
    tmp_pairs.clear();
    for (int lc = lm0; lc < lm1; ++lc) {
      if (h.lm_fixed[lc]) continue;
      int nl = 0;
      uint8_t led[CH_E]; int16_t lpf[CH_E];
      for (int s = h.lm_ptr[lc]; s < h.lm_ptr[lc + 1]; ++s) {
        const int pf = h.pose_free[h.e_pose[s]];
        if (pf >= 0 && !h.e_dup[s]) { led[nl] = (uint8_t)(s - e0); lpf[nl] = (int16_t)pf; ++nl; }
      }
      for (int i = 0; i < nl; ++i) {
        const int* row = &blk_of[(size_t)lpf[i] * nP];
        for (int j = i; j < nl; ++j) {
          const int b = row[lpf[j]];                        // pa <= pb: edges of a landmark are sorted by pose
          bc[b + 1]++;
          tmp_pairs.push_back((uint32_t)b << 16 | (uint32_t)led[i] << 8 | led[j]);
        }
      }
    }
    {
      const int base = (int)h.pair_a.size();
      bc[0] = base;
      for (int b = 0; b < nBlk; ++b) bc[b + 1] += bc[b];
      int* bp = &h.pair_ptr[(size_t)c * (nBlk + 1)];
      for (int b = 0; b <= nBlk; ++b) bp[b] = bc[b];
      h.pair_a.resize(bc[nBlk]); h.pair_b.resize(bc[nBlk]);
      for (const uint32_t k : tmp_pairs) {
        const int q = bc[k >> 16]++;
        h.pair_a[q] = (uint8_t)(k >> 8); h.pair_b[q] = (uint8_t)k;
      }
    }
    // --- work items of the block phase.  A lane walks ONE pair list and a wave takes as long as its longest list, so
    // the lists (0 .. 40 pairs in a local window) are cut into parts of about the same length, the parts sorted by
    // length, and the parts of one block kept inside one wave (their partial sums meet through wave shuffles).
    {
      const int* bp = &h.pair_ptr[(size_t)c * (nBlk + 1)];
      const int base = bp[0];
      int maxlen = 0;
      for (int b = 0; b < nBlk; ++b) maxlen = std::max(maxlen, bp[b + 1] - bp[b]);
      const int seg = std::max(BSEG_MIN, (maxlen + BSEG_PARTS - 1) / BSEG_PARTS);
      const bool dense = dense_slabs_mode() != 0;
      // (BaDev::touch, as k_build_lists writes it: blocks with pairs, poses with edges)
      unsigned int* tm = &h.touch[(size_t)c * TOUCH_WORDS];
      for (int b = 0; b < nBlk + nP; ++b) {
        const bool on = b < nBlk ? (bp[b + 1] > bp[b]) : (pp[b - nBlk + 1] > pp[b - nBlk]);
        if (on || dense) tm[b >> 5] |= 1u << (b & 31);
      }
      order.clear();
      for (int b = 0; b < nBlk; ++b) {
        const int n = bp[b + 1] - bp[b], k = (n == 0 && !dense) ? 0 : std::max(1, (n + seg - 1) / seg);
        order.push_back({k ? -((n + k - 1) / k) : 0, b});
      }
      std::stable_sort(order.begin(), order.end());
      h.bseg_ptr[2 * c] = (int)(h.bseg.size() / 4);
      int pos = 0;                                // in items (16 per wave, four lanes each; a block's parts inside one row of 16 lanes)
      for (const auto& ob : order) {
        const int b = ob.second, n = bp[b + 1] - bp[b], k = (n == 0 && !dense) ? 0 : std::max(1, (n + seg - 1) / seg), len = k ? (n + k - 1) / k : 0;
        while ((pos & 3) + k > 4) { h.bseg.push_back(-1); h.bseg.push_back(0); h.bseg.push_back(0); h.bseg.push_back(1 << 4); ++pos; }
        for (int i = 0; i < k; ++i) {
          const int q0 = bp[b] - base + std::min(n, i * len), q1 = bp[b] - base + std::min(n, (i + 1) * len);
          h.bseg.push_back(b); h.bseg.push_back(q0); h.bseg.push_back(q1); h.bseg.push_back(i | (k << 4));
          ++pos;
        }
      }
      h.bseg_ptr[2 * c + 1] = (int)(h.bseg.size() / 4) - h.bseg_ptr[2 * c];
    }
  }
  return SSX_OK;
}

// carve the arena and upload the problem
// Segment plan of the band solver (ba_band.inc): w > 0 switches it on.  K interiors of >= w poses separated by w poses.
struct BandPlan {
  int w = 0, K = 1;
  std::vector<int> seg_p0, seg_m;
  BcrPlan bcr;                       // bcr.on: block cyclic reduction (ba_bcr.inc) solves the band instead of the segments
};

void plan_band(int nP, int w, BandPlan& bp)
{
  bp.w = w; bp.K = 1; bp.seg_p0.assign(1, 0); bp.seg_m.assign(1, nP - w);
  if (w <= 0) return;
  if (nP >= 48) {
    // dependent chain ~ nP / K interior pivots + 1.5 K w separator pivots (the top window is wider)
    int K = (int)std::lround(std::sqrt((double)nP / (1.5 * w)));
    K = std::max(2, std::min(K, 64));
    while (K > 1 && (nP - K * w) / K < w) --K;                      // every interior must hold >= w poses
    while ((nP - K * w + K - 1) / K > 480) ++K;                     // LDS of the back-substitution
    bp.K = K;
  }
  if (bp.K == 1) return;
  const int K = bp.K, inner = nP - K * w, base = inner / K, rem = inner % K;
  bp.seg_p0.resize(K); bp.seg_m.resize(K);
  int p = 0;
  for (int k = 0; k < K; ++k) {
    bp.seg_p0[k] = p;
    bp.seg_m[k] = base + (k < rem ? 1 : 0);
    p += bp.seg_m[k] + w;
  }
}

struct UploadPlace {          // where a window of a batch lives (nullptr = a single window in the ctx arena)
  bool dry = false;            // sizing pass: only in_bytes / rest_bytes are computed
  size_t in_bytes = 0, rest_bytes = 0;
  char* in_dev = nullptr;      // uploaded blob on the device
  char* rest_dev = nullptr;    // scratch on the device
  char* in_host = nullptr;     // pinned mirror of the blob
  bool keep_init = false;      // a RESIDENT batch keeps a pristine copy of the uploaded state (it is solved again from it)
};

ssx_status upload(ssx_ctx* ctx, const ssx_ba_problem* pr, const HostPrep& h, double huber_delta, double chi2_th,
                  int world, int rank, BaDev& d, BigDev& bd, const BandPlan& bp, BandDev& bnd, UploadPlace* place = nullptr,
                  const WinExt* ext = nullptr, const BaDev* recs = nullptr, const int* pe_ptr_dev = nullptr, const int* pe_edge_dev = nullptr)
{
  const bool rz = recs != nullptr;               // large window whose records / columns / raw arrays already live on the device (big_records)
  if (!ctx->ba) { ctx->ba = new BaWorkspace(); ctx->ba_free = ssx_ba_workspace_free; }
  BaWorkspace* ws = ctx->ba;
  const bool dup_state = place != nullptr;       // batched windows: the second state buffer is part of the uploaded blob
  const int P = h.P, L = h.L, E = h.E, nP = h.nP, nLm = h.nLm, nCh = h.nCh, nBlk = h.nBlk;
  const int n = 6 * nP;
  const bool big = h.big;
  const bool dev_lists = h.dev_lists && !big;
  const int bseg_cap = dev_lists ? 2 * nBlk * BSEG_PARTS + 16 : 0;
  const size_t nPairs = dev_lists ? 0 : h.pair_a.size();
  const int lin_stride = big ? 2 : nP * 27 + 2;
  const int n_pad = big ? ((n + NB - 1) / NB) * NB : 0;
  const size_t nBlkS = h.sblk_pa.size();
  Layout in;   // input blob (mirrored in pinned staging)
  const size_t o_pose_free = in.take(rz ? 0 : sizeof(int) * P);
  // (the landmark / chunk tables and the structure-of-arrays edge columns are read by the large-window kernels only: the
  // small-window kernels take everything from the packed records -- a quarter of a C3 window's blob not staged, not sent)
  const bool dev_prep = h.dev_prep && !big;
  const bool lm_tables = big || dev_prep;
  const size_t o_lm_fixed = in.take(lm_tables && !rz ? nLm : 0);
  const size_t o_lm_id = in.take(lm_tables && !rz ? sizeof(int) * nLm : 0);
  const size_t o_lm_ptr = in.take(lm_tables && !rz ? sizeof(int) * (nLm + 1) : 0);
  const size_t o_ch_lm = in.take(big && !rz ? sizeof(int) * (nCh + 1) : 0);
  const size_t o_e_pose = in.take(big && !rz ? sizeof(int) * E : 0);
  const size_t o_e_lmc = in.take(big && !rz ? sizeof(int) * E : 0);
  const size_t o_e_cam = in.take(big && !rz ? E : 0);
  // (device-marshalled windows upload the caller's arrays; the sorted columns / records are scratch, written by k_prep_chunk)
  size_t o_e_dup = (dev_prep || rz) ? 0 : in.take(E);
  size_t o_e_uv = (dev_prep || rz) ? 0 : in.take(sizeof(double) * 2 * E);
  const size_t o_ch_desc = in.take(rz ? 0 : sizeof(int) * 4 * (size_t)(nCh + 1));
  size_t o_e_rec = (dev_prep || rz) ? 0 : in.take(sizeof(int) * 4 * (size_t)(E + 1));
  size_t o_l_rec = (dev_prep || rz) ? 0 : in.take(sizeof(int) * 4 * (size_t)(nLm + 1));
  const size_t o_blk_pa = in.take(nBlk + 1);
  const size_t o_blk_pb = in.take(nBlk + 1);
  size_t o_pptr = (dev_prep || rz) ? 0 : in.take(sizeof(uint16_t) * (h.pptr.size() + 1));
  // (an ssx_ba_window keeps the raw observation arrays and the state in device buffers of its own: `ext`)
  const int E_raw = h.E_raw;
  const bool raw_in = dev_prep && !ext;
  const bool have_cam = dev_prep && (ext ? ext->r_edge_cam != nullptr : pr->edge_cam != nullptr);
  const size_t o_lm_compact = in.take(dev_prep ? sizeof(int) * (size_t)(L + 1) : 0);
  const bool have_rank = dev_prep && !h.pose_rank.empty();
  const size_t o_pose_rank = in.take(have_rank ? sizeof(int) * (size_t)P : 0);
  const int raw_fmt = raw_in && !rz ? h.raw_fmt : 0;
  const size_t o_r_pose = in.take(raw_in ? ((raw_fmt & 1) ? 1 : sizeof(int)) * (size_t)(E + 1) : 0);
  const size_t o_r_point = in.take(raw_in ? ((raw_fmt & 2) ? sizeof(uint16_t) : sizeof(int)) * (size_t)(E + 1) : 0);
  const size_t o_r_uv = in.take(raw_in ? ((raw_fmt & 4) ? sizeof(float) : sizeof(double)) * 2 * (size_t)(E + 1) : 0);
  const size_t o_r_cam = in.take(have_cam && raw_in ? (size_t)E + 1 : 0);
  const size_t o_slot8 = in.take(dev_prep ? (size_t)E_raw + 1 : 0);
  // (host-built lists travel with the blob; device-built ones are scratch behind it, a fixed capacity per chunk)
  size_t o_pair_a = dev_lists ? 0 : in.take(nPairs + 1);
  size_t o_pair_b = dev_lists ? 0 : in.take(nPairs + 1);
  size_t o_pair_ptr = dev_lists ? 0 : in.take(sizeof(int) * (h.pair_ptr.size() + 1));
  size_t o_bseg = dev_lists ? 0 : in.take(sizeof(int) * (h.bseg.size() + 4));
  size_t o_bseg_ptr = dev_lists ? 0 : in.take(sizeof(int) * (h.bseg_ptr.size() + 1));
  const size_t touch_bytes = big ? 0 : sizeof(unsigned int) * TOUCH_WORDS * (size_t)(nCh + 1);
  size_t o_touch = (dev_lists || big) ? 0 : in.take(touch_bytes);
  const size_t o_pe_ptr = in.take(rz ? 0 : sizeof(int) * (h.pe_ptr.size() + 1));
  const size_t o_pe_edge = in.take(rz ? 0 : sizeof(int) * (h.pe_edge.size() + 1));
  const size_t o_sblk_pa = in.take(sizeof(int) * (nBlkS + 1));
  const size_t o_sblk_pb = in.take(sizeof(int) * (nBlkS + 1));
  const size_t o_spair_ptr = in.take(sizeof(int) * (h.spair_ptr.size() + 1));
  const bool band = big && bp.w > 0;
  const size_t o_seg_p0 = in.take(sizeof(int) * (bp.seg_p0.size() + 1));
  const size_t o_seg_m = in.take(sizeof(int) * (bp.seg_m.size() + 1));
  const bool bcr = band && bp.bcr.on;                                 // block cyclic reduction of the band (ba_bcr.inc)
  const size_t o_bcr_p0 = in.take(bcr ? sizeof(int) * (bp.bcr.p0.size() + 1) : 0);
  const size_t o_bcr_elim = in.take(bcr ? sizeof(int) * (bp.bcr.elim.size() + 4) : 0);
  if (ext && !dev_prep) { ctx->set_error("ssx_ba: a window needs the device-side marshalling (<= %d free keyframes, no SSX_BA_HOST_PREP)", SSX_BA_SMALL_P); return SSX_ERR_UNSUPPORTED; }
  const size_t o_pose0 = in.take(ext ? 0 : sizeof(double) * 7 * P);
  const size_t o_point0 = in.take(ext ? 0 : sizeof(double) * 3 * (L + 1));
  // (the state crosses PCIe ONCE: the second buffer and, for a resident batch, the pristine copy are made on the device,
  // k_dup_state_b -- the blob of a C3 window carried three copies of its 96 KB of landmarks)
  const size_t in_bytes = in.off;
  Layout all = in;
  const size_t o_pose1 = ext ? 0 : all.take(sizeof(double) * 7 * P);
  const size_t o_point1 = ext ? 0 : all.take(sizeof(double) * 3 * (L + 1));
  const bool keep_init = dup_state && !ext && place->keep_init;
  const size_t o_pose_init = keep_init ? all.take(sizeof(double) * 7 * P) : 0;
  const size_t o_point_init = keep_init ? all.take(sizeof(double) * 3 * (L + 1)) : 0;
  size_t o_perm = 0, o_c2 = 0;
  if (dev_prep) {
    o_e_dup = all.take((size_t)E + 1);
    o_e_uv = all.take(sizeof(double) * 2 * (size_t)(E + 1));
    o_e_rec = all.take(sizeof(int) * 4 * (size_t)(E + 1));
    o_l_rec = all.take(sizeof(int) * 4 * (size_t)(nLm + 1));
    o_pptr = all.take(sizeof(uint16_t) * ((size_t)(nCh + 1) * (nP + 1) + 1));
    o_perm = all.take(sizeof(int) * (size_t)(E + 1));
    o_c2 = all.take(sizeof(double) * (size_t)(E_raw + 1));
  }
  if (dev_lists) {
    o_pair_a = all.take((size_t)(nCh + 1) * MAX_PAIRS);
    o_pair_b = all.take((size_t)(nCh + 1) * MAX_PAIRS);
    o_pair_ptr = all.take(sizeof(int) * ((size_t)(nCh + 1) * (nBlk + 1) + 1));
    o_bseg = all.take(sizeof(int) * 4 * ((size_t)(nCh + 1) * bseg_cap + 1));
    o_bseg_ptr = all.take(sizeof(int) * (2 * (size_t)nCh + 2));
    o_touch = all.take(touch_bytes);
  }
  const size_t o_W = all.take(sizeof(double) * 18 * (size_t)E);
  const size_t o_err_lin = all.take(sizeof(double) * 2 * (size_t)E);
  const size_t o_err_trial = all.take(sizeof(double) * 2 * (size_t)E);
  const size_t o_Hll = all.take(sizeof(double) * 6 * (size_t)nLm);
  const size_t o_bl = all.take(sizeof(double) * 3 * (size_t)nLm);
  const size_t o_lin_slab = all.take(sizeof(double) * (size_t)(nCh + 1) * lin_stride);
  const size_t o_Hpp = all.take(sizeof(double) * (nP + 1) * UPPER6);
  const size_t o_bp = all.take(sizeof(double) * (nP + 1) * 6);
  const size_t iter_count = (size_t)nP * 27 + 1 + world;
  // (band solver: iter_comm sits right behind [band | rhs] so that ONE all-reduce per trial carries the reduced system AND the
  // linearisation's pose blocks / chi2 -- see big_trial)
  const bool band_pre = big && bp.w > 0;
  size_t o_iter = band_pre ? 0 : all.take(sizeof(double) * (iter_count + 1));
  const size_t o_schur = all.take(big ? 256 : sizeof(double) * (size_t)(nCh + 1) * (nBlk * 36 + nP * 6));
  const size_t o_trial_comm = all.take(big ? 256 : sizeof(double) * ((size_t)n * n + n + 1));
  const size_t o_BDa = all.take(big ? sizeof(double) * 18 * (size_t)(E + 1) : 256);
  const size_t o_Wma = all.take(big ? sizeof(double) * 18 * (size_t)(E + 1) : 256);
  const size_t o_Cv = all.take(big ? sizeof(double) * 6 * (size_t)(E + 1) : 256);
  const size_t o_S = all.take((big && !band) ? sizeof(double) * (size_t)(n_pad + NB) * n_pad : 256);
  // band solver: band + rhs, segment updates, factors of both levels, the separator system
  const int bw = bp.w, bK = bp.K, bnPr = bK * bw, bwr = 2 * bw - 1;
  const int NW0 = 6 * (2 * bw + 1) + 1, LS0 = 36 + NW0 * 6;
  const int w1 = bK == 1 ? bw : bwr, NW1 = 6 * (w1 + 1 + bw) + 1, LS1 = 36 + NW1 * 6;
  const int NU = 12 * bw + 1;
  const size_t sb_count = band ? (size_t)nP * (bw + 1) * 36 + (size_t)n : 0;
  const size_t sr_count = (band && bK > 1) ? (size_t)bnPr * (bwr + 1) * 36 + 6 * (size_t)bnPr : 0;
  const size_t o_Sb = all.take(sizeof(double) * (sb_count + 1 + (band ? iter_count + 1 : 0)));
  if (band) o_iter = o_Sb + sizeof(double) * sb_count;
  const size_t o_U = all.take(band ? sizeof(double) * (size_t)bK * NU * NU : 256);
  const size_t o_Ls0 = all.take((band && bK > 1) ? sizeof(double) * (size_t)nP * LS0 : 256);
  const size_t o_Sr = all.take(sizeof(double) * (sr_count + 1));
  const size_t o_Ls1 = all.take(band ? sizeof(double) * (size_t)(bK > 1 ? bnPr : nP) * LS1 : 256);
  const size_t o_bcr_mem = all.take(bcr ? sizeof(double) * (bcr_mem_doubles(bp.bcr.N, bp.bcr.m) + 8) : 256);
  const size_t o_xr = all.take(sizeof(double) * (6 * (size_t)bnPr + 8));
  const size_t o_x = all.take(sizeof(double) * (n_pad + 8));
  const size_t o_Ld = all.take(sizeof(double) * NB * NB);
  const size_t o_invd = all.take(sizeof(double) * (n_pad + 8));
  const size_t o_Ninv = all.take(sizeof(double) * 4 * 256);
  const size_t o_scale_part = all.take(sizeof(double) * 64);
  const size_t o_xp = all.take(sizeof(double) * (n + 1));
  const size_t o_trial = all.take(sizeof(double) * 3 * (nCh + 1));
  const size_t o_scal_comm = all.take(sizeof(double) * 4);
  const size_t o_scal = all.take(sizeof(double) * SC_N);
  const size_t o_lmstat = all.take(sizeof(double) * 3 * SSX_BA_MAX_STATS);
  const size_t o_ticket = all.take(sizeof(unsigned int) * 4);

  if (place && place->dry) {                     // sizing pass of a batch
    place->in_bytes = in_bytes;
    place->rest_bytes = all.off - in_bytes;
    return SSX_OK;
  }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!place) {
    SSX_HIP_TRY(ctx, ws->arena.reserve(all.off));
    SSX_HIP_TRY(ctx, ws->stage.reserve(std::max(in_bytes, sizeof(double) * (7 * (size_t)P + 3 * (size_t)L + 2 * (size_t)E + (size_t)h.E_raw))));
    SSX_HIP_TRY(ctx, ws->scal.reserve(sizeof(double) * (SC_N + 3 * SSX_BA_MAX_STATS)));
  }
  char* hs = place ? place->in_host : ws->stage.as<char>();
  if (!rz) memcpy(hs + o_pose_free, h.pose_free.data(), sizeof(int) * P);
  if (lm_tables && nLm && !rz) {
    memcpy(hs + o_lm_fixed, h.lm_fixed.data(), nLm);
    memcpy(hs + o_lm_id, h.lm_id.data(), sizeof(int) * nLm);
  }
  if (lm_tables && !rz) memcpy(hs + o_lm_ptr, h.lm_ptr.data(), sizeof(int) * (nLm + 1));
  if (nCh && !rz) memcpy(hs + o_ch_desc, h.ch_desc.data(), sizeof(int) * 4 * (size_t)nCh);
  if (dev_prep) {
    if (L) memcpy(hs + o_lm_compact, h.lm_compact.data(), sizeof(int) * (size_t)L);
    if (have_rank) memcpy(hs + o_pose_rank, h.pose_rank.data(), sizeof(int) * (size_t)P);
    if (E && raw_in) {
      if (raw_fmt & 1) { uint8_t* o = (uint8_t*)(hs + o_r_pose); for (int e = 0; e < E; ++e) o[e] = (uint8_t)pr->edge_pose[e]; }
      else memcpy(hs + o_r_pose, pr->edge_pose, sizeof(int) * (size_t)E);
      if (raw_fmt & 2) { uint16_t* o = (uint16_t*)(hs + o_r_point); for (int e = 0; e < E; ++e) o[e] = (uint16_t)pr->edge_point[e]; }
      else memcpy(hs + o_r_point, pr->edge_point, sizeof(int) * (size_t)E);
      if (raw_fmt & 4) { float* o = (float*)(hs + o_r_uv); for (size_t i = 0; i < 2 * (size_t)E; ++i) o[i] = (float)pr->edge_uv[i]; }
      else memcpy(hs + o_r_uv, pr->edge_uv, sizeof(double) * 2 * (size_t)E);
      if (have_cam) memcpy(hs + o_r_cam, pr->edge_cam, (size_t)E);
    }
    if (E_raw) memcpy(hs + o_slot8, h.slot8.data(), (size_t)E_raw);
  } else if (!rz) {
  if (E) memcpy(hs + o_e_rec, h.e_rec.data(), sizeof(int) * 4 * (size_t)E);
  if (nLm) memcpy(hs + o_l_rec, h.l_rec.data(), sizeof(int) * 4 * (size_t)nLm);
  }
  if (big && !rz) memcpy(hs + o_ch_lm, h.ch_lm.data(), sizeof(int) * h.ch_lm.size());
  if (E && !rz) {
    if (big) {
      memcpy(hs + o_e_pose, h.e_pose.data(), sizeof(int) * E);
      memcpy(hs + o_e_lmc, h.e_lmc.data(), sizeof(int) * E);
      memcpy(hs + o_e_cam, h.e_cam.data(), E);
    }
    if (!dev_prep) {
      memcpy(hs + o_e_dup, h.e_dup.data(), E);
      memcpy(hs + o_e_uv, h.e_uv.data(), sizeof(double) * 2 * E);
    }
  }
  if (nBlk) {
    memcpy(hs + o_blk_pa, h.blk_pa.data(), nBlk);
    memcpy(hs + o_blk_pb, h.blk_pb.data(), nBlk);
  }
  if (!dev_prep && !h.pptr.empty()) memcpy(hs + o_pptr, h.pptr.data(), sizeof(uint16_t) * h.pptr.size());
  if (nPairs) {
    memcpy(hs + o_pair_a, h.pair_a.data(), nPairs);
    memcpy(hs + o_pair_b, h.pair_b.data(), nPairs);
  }
  if (!dev_lists) {
    if (!h.pair_ptr.empty()) memcpy(hs + o_pair_ptr, h.pair_ptr.data(), sizeof(int) * h.pair_ptr.size());
    if (!h.bseg.empty()) memcpy(hs + o_bseg, h.bseg.data(), sizeof(int) * h.bseg.size());
    if (!h.bseg_ptr.empty()) memcpy(hs + o_bseg_ptr, h.bseg_ptr.data(), sizeof(int) * h.bseg_ptr.size());
    if (!big && !h.touch.empty()) memcpy(hs + o_touch, h.touch.data(), sizeof(unsigned int) * h.touch.size());
  }
  if (big && !rz) {
    memcpy(hs + o_pe_ptr, h.pe_ptr.data(), sizeof(int) * h.pe_ptr.size());
    memcpy(hs + o_pe_edge, h.pe_edge.data(), sizeof(int) * h.pe_edge.size());
  }
  if (big) {
    memcpy(hs + o_sblk_pa, h.sblk_pa.data(), sizeof(int) * nBlkS);
    memcpy(hs + o_sblk_pb, h.sblk_pb.data(), sizeof(int) * nBlkS);
    memcpy(hs + o_spair_ptr, h.spair_ptr.data(), sizeof(int) * h.spair_ptr.size());
  }
  if (band) {
    memcpy(hs + o_seg_p0, bp.seg_p0.data(), sizeof(int) * bp.seg_p0.size());
    memcpy(hs + o_seg_m, bp.seg_m.data(), sizeof(int) * bp.seg_m.size());
    if (bcr) {
      memcpy(hs + o_bcr_p0, bp.bcr.p0.data(), sizeof(int) * bp.bcr.p0.size());
      memcpy(hs + o_bcr_elim, bp.bcr.elim.data(), sizeof(int) * bp.bcr.elim.size());
    }
  }
  if (!ext) {
    memcpy(hs + o_pose0, pr->poses, sizeof(double) * 7 * P);
    if (L) memcpy(hs + o_point0, pr->points, sizeof(double) * 3 * L);
  }
  // device addresses: the uploaded blob and the scratch behind it (one arena; a batch keeps all blobs together so that
  // ONE copy uploads every window)
  char* base_in = place ? place->in_dev : ws->arena.as<char>();
  char* base_rest = place ? place->rest_dev : base_in + in_bytes;
  auto at = [&](size_t o) -> char* { return o < in_bytes ? base_in + o : base_rest + (o - in_bytes); };
  if (!place) {
    SSX_HIP_TRY(ctx, hipMemcpyAsync(base_in, hs, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    // the second state buffer starts as a copy (landmarks without edges are never rewritten)
    if (!ext) {
    SSX_HIP_TRY(ctx, hipMemcpyAsync(at(o_pose1), at(o_pose0), sizeof(double) * 7 * P, hipMemcpyDeviceToDevice, ctx->stream));
    if (L)
      SSX_HIP_TRY(ctx, hipMemcpyAsync(at(o_point1), at(o_point0), sizeof(double) * 3 * L, hipMemcpyDeviceToDevice, ctx->stream));
    }
  }

  d.P = P; d.L = L; d.E = E; d.nP = nP; d.nLm = nLm; d.nCh = nCh; d.nBlk = nBlk; d.world = world; d.rank = rank;
  d.big = big ? 1 : 0; d.lin_stride = lin_stride;
  d.dense_slabs = dense_slabs_mode();
  d.touch = (unsigned int*)(at(o_touch));
  d.store_w = 1;                                 // the caller clears it for small windows with analytic Jacobians
  d.pose_free = (const int*)(at(o_pose_free));
  d.lm_fixed = (const uint8_t*)(at(o_lm_fixed));
  d.lm_id = (const int*)(at(o_lm_id));
  d.lm_ptr = (const int*)(at(o_lm_ptr));
  d.ch_lm = (const int*)(at(o_ch_lm));
  d.e_pose = (const int*)(at(o_e_pose));
  d.e_lmc = (const int*)(at(o_e_lmc));
  d.e_cam = (const uint8_t*)(at(o_e_cam));
  d.e_dup = (const uint8_t*)(at(o_e_dup));
  d.e_uv = (const double*)(at(o_e_uv));
  d.ch_desc = (const int4*)(at(o_ch_desc)); d.e_rec = (const int4*)(at(o_e_rec)); d.l_rec = (const int4*)(at(o_l_rec));
  d.blk_pa = (const int8_t*)(at(o_blk_pa));
  d.blk_pb = (const int8_t*)(at(o_blk_pb));
  d.pptr = (const uint16_t*)(at(o_pptr));
  d.pair_a = (uint8_t*)(at(o_pair_a));
  d.pair_b = (uint8_t*)(at(o_pair_b));
  d.pair_ptr = (int*)(at(o_pair_ptr));
  d.bseg = (int4*)(at(o_bseg)); d.bseg_ptr = (int*)(at(o_bseg_ptr));
  d.bseg_cap = bseg_cap;
  d.dev_prep = dev_prep ? 1 : 0;
  d.E_raw = E_raw;
  d.raw_fmt = raw_fmt;
  d.no_err = 0;                                  // (the solve entry points set it when no per-edge errors were asked for)
  if (ext) {
    d.r_edge_pose = ext->r_edge_pose; d.r_edge_point = ext->r_edge_point; d.r_edge_uv = ext->r_edge_uv; d.r_edge_cam = ext->r_edge_cam;
  } else {
  d.r_edge_pose = (const int*)(dev_prep ? at(o_r_pose) : nullptr); d.r_edge_point = (const int*)(dev_prep ? at(o_r_point) : nullptr);
  d.r_edge_uv = (const double*)(dev_prep ? at(o_r_uv) : nullptr); d.r_edge_cam = (const uint8_t*)(have_cam ? at(o_r_cam) : nullptr);
  }
  d.r_slot8 = (const uint8_t*)(dev_prep ? at(o_slot8) : nullptr); d.lm_compact = (const int*)(dev_prep ? at(o_lm_compact) : nullptr);
  d.perm = (int*)(dev_prep ? at(o_perm) : nullptr); d.c2_out = (double*)(dev_prep ? at(o_c2) : nullptr);
  d.pose_rank = (const int*)(have_rank ? at(o_pose_rank) : nullptr);
  d.K = Cam{pr->K[0], pr->K[1], pr->K[2], pr->K[3]};
  for (int i = 0; i < 14; ++i) d.ext[i] = pr->cam_ext[i];
  d.huber_delta = huber_delta; d.chi2_th = chi2_th;
  d.pose_init = keep_init ? (const double*)(at(o_pose_init)) : nullptr;
  d.point_init = keep_init ? (const double*)(at(o_point_init)) : nullptr;
  if (ext) {
    d.pose[0] = ext->pose[0]; d.pose[1] = ext->pose[1]; d.point[0] = ext->point[0]; d.point[1] = ext->point[1];
  } else {
  d.pose[0] = (double*)(at(o_pose0)); d.pose[1] = (double*)(at(o_pose1));
  d.point[0] = (double*)(at(o_point0)); d.point[1] = (double*)(at(o_point1));
  }
  d.W = (double*)(at(o_W));
  d.err_lin = (double*)(at(o_err_lin));
  d.err_trial = (double*)(at(o_err_trial));
  d.Hll = (double*)(at(o_Hll)); d.bl = (double*)(at(o_bl));
  d.lin_slab = (double*)(at(o_lin_slab));
  d.Hpp = (double*)(at(o_Hpp)); d.bp = (double*)(at(o_bp));
  d.iter_comm = (double*)(at(o_iter));
  d.schur_slab = (double*)(at(o_schur));
  d.trial_comm = (double*)(at(o_trial_comm));
  d.xp = (double*)(at(o_xp));
  d.trial_slab = (double*)(at(o_trial));
  d.scal_comm = (double*)(at(o_scal_comm));
  d.scal = (double*)(at(o_scal));
  d.lm_stat = (double*)(at(o_lmstat));
  d.ticket = (unsigned int*)(at(o_ticket));
  if (rz) {                                      // the records, columns and raw arrays of big_records
    d.dev_prep = 1; d.E_raw = recs->E_raw;
    d.pose_free = recs->pose_free; d.lm_fixed = recs->lm_fixed; d.lm_id = recs->lm_id; d.lm_ptr = recs->lm_ptr; d.ch_lm = recs->ch_lm;
    d.e_pose = recs->e_pose; d.e_lmc = recs->e_lmc; d.e_cam = recs->e_cam; d.e_dup = recs->e_dup; d.e_uv = recs->e_uv;
    d.ch_desc = recs->ch_desc; d.e_rec = recs->e_rec; d.l_rec = recs->l_rec; d.perm = recs->perm; d.c2_out = recs->c2_out; d.lm_chunk = recs->lm_chunk;
    d.r_edge_pose = recs->r_edge_pose; d.r_edge_point = recs->r_edge_point; d.r_edge_uv = recs->r_edge_uv; d.r_edge_cam = recs->r_edge_cam;
    d.r_slot8 = recs->r_slot8; d.lm_compact = recs->lm_compact; d.pose_rank = nullptr;
  }
  bd = BigDev{};
  bnd = BandDev{};
  if (big) {
    bd.n = n; bd.n_pad = n_pad; bd.ld = n_pad; bd.T = n_pad / NB; bd.nBlkS = (int)nBlkS;
    bd.pe_ptr = rz ? pe_ptr_dev : (const int*)(at(o_pe_ptr)); bd.pe_edge = rz ? pe_edge_dev : (const int*)(at(o_pe_edge));
    bd.sblk_pa = (const int*)(at(o_sblk_pa)); bd.sblk_pb = (const int*)(at(o_sblk_pb));
    bd.spair_ptr = (const int*)(at(o_spair_ptr)); bd.spair_ab = nullptr;   // the pair lists live in the workspace of build_pairs
    bd.BDa = (double*)(at(o_BDa)); bd.Wma = (double*)(at(o_Wma)); bd.Cv = (double*)(at(o_Cv));
    bnd = BandDev{};
    if (band) {
      bnd.on = 1; bnd.w = bw; bnd.K = bK; bnd.nP = nP; bnd.nPr = bnPr; bnd.wr = bwr;
      bnd.Sb = (double*)(at(o_Sb)); bnd.bsv = bnd.Sb + (size_t)nP * (bw + 1) * 36;
      bnd.seg_p0 = (const int*)(at(o_seg_p0)); bnd.seg_m = (const int*)(at(o_seg_m));
      bnd.U = (double*)(at(o_U)); bnd.Ls0 = (double*)(at(o_Ls0)); bnd.Sr = (double*)(at(o_Sr));
      bnd.Ls1 = (double*)(at(o_Ls1)); bnd.xr = (double*)(at(o_xr)); bnd.LS0 = LS0; bnd.LS1 = LS1;
      bnd.bcr = BcrDev{};
      if (bcr) {
        BcrDev& q = bnd.bcr;
        q.on = 1; q.N = bp.bcr.N; q.m = bp.bcr.m;
        q.p0 = (const int*)(at(o_bcr_p0)); q.elim = (const int4*)(at(o_bcr_elim));
        const size_t mmN = (size_t)q.N * q.m * q.m, mN = (size_t)q.N * q.m;
        double* base = (double*)(at(o_bcr_mem));
        q.D = base; q.E = q.D + mmN; q.DL = q.E + 2 * mmN;   /* E: two buffers, bcr_e_buf */ q.DR = q.DL + mmN; q.Lf = q.DR + mmN; q.Ul = q.Lf + mmN; q.Ur = q.Ul + mmN;
        q.R = q.Ur + mmN; q.RL = q.R + mN; q.RR = q.RL + mN; q.Y = q.RR + mN; q.X = q.Y + mN;
      }
    }
    bd.S = (double*)(at(o_S)); bd.x = (double*)(at(o_x)); bd.Ld = (double*)(at(o_Ld)); bd.invd = (double*)(at(o_invd)); bd.Ninv = (double*)(at(o_Ninv)); bd.scale_part = (double*)(at(o_scale_part));
  }
  if (!place && nCh > 0 && (dev_lists || dev_prep)) {   // (a batch marshals all its windows with one launch pair: batch_build)
    if (dev_prep) {
      hipLaunchKernelGGL(k_prep_scatter, dim3((E_raw + CH - 1) / CH), dim3(CH), 0, ctx->stream, d);
      hipLaunchKernelGGL(k_prep_chunk, dim3(nCh), dim3(CH), 0, ctx->stream, d);
    } else {
      hipLaunchKernelGGL(k_build_lists, dim3(nCh), dim3(CH), 0, ctx->stream, d);
    }
    SSX_HIP_TRY(ctx, hipGetLastError());
  }
  return SSX_OK;
}

// Large windows: the non-zero blocks of the reduced system and their pair lists, on the device (kernels in ba_big.inc).
// Fills h.sblk_pa / h.sblk_pb / h.spair_ptr (sorted by (pa, pb); every diagonal block present, possibly with an empty
// list) and h.band_w; the lists themselves stay in the workspace: *ab_dev.
// Large windows, device-side marshalling (HostPrep::dev_prep): the caller's arrays and the host's counting tables go up once
// (25 bytes per observation instead of ~62 of marshalled records and columns, and none of the ~3 ms of host work a
// 480 000-observation window cost), k_prep_scatter / k_prep_chunk build the (landmark, pose) order, the packed records and the
// structure-of-arrays columns, and a stable radix sort by free pose gives the pose-major edge list.  Everything lives in
// ws->recs for the duration of the solve; `r` receives the pointers (the pair builder and upload() take them from there).
// The observation columns as the caller holds them (pose index, landmark index, uv, camera) into pinned staging on the worker
// pool and on their way to the device; nothing here depends on prepare()'s counting, which then runs beside the copy.
ssx_status raw_upload_early(ssx_ctx* ctx, const ssx_ba_problem* pr)
{
  if (!ctx->ba) { ctx->ba = new BaWorkspace(); ctx->ba_free = ssx_ba_workspace_free; }
  BaWorkspace* ws = ctx->ba;
  ws->raw_early.valid = false;
  const int E = pr->E;
  if (E <= 0 || !pr->edge_pose || !pr->edge_point || !pr->edge_uv) return SSX_OK;      // (prepare() reports it)
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool have_cam = pr->edge_cam != nullptr;
  Layout in;
  BaWorkspace::RawEarly re;
  re.o_pose = in.take(sizeof(int) * (size_t)(E + 1)); re.o_point = in.take(sizeof(int) * (size_t)(E + 1));
  re.o_uv = in.take(sizeof(double) * 2 * (size_t)(E + 1)); re.o_cam = in.take(have_cam ? (size_t)E + 1 : 0);
  SSX_HIP_TRY(ctx, ws->raw_d.reserve(in.off));
  SSX_HIP_TRY(ctx, ws->raw_h.reserve(in.off));
  char* hs = ws->raw_h.as<char>();
  struct Cp { size_t off; const void* src; size_t n; };
  std::vector<Cp> cps;
  auto add = [&](size_t off, const void* src, size_t n) {
    for (size_t a = 0; a < n; a += (size_t)1 << 20) cps.push_back({off + a, (const char*)src + a, std::min(n - a, (size_t)1 << 20)});
  };
  add(re.o_pose, pr->edge_pose, sizeof(int) * (size_t)E); add(re.o_point, pr->edge_point, sizeof(int) * (size_t)E);
  add(re.o_uv, pr->edge_uv, sizeof(double) * 2 * (size_t)E);
  if (have_cam) add(re.o_cam, pr->edge_cam, (size_t)E);
  ws->pool.run((int)cps.size(), std::min<int>(16, (int)cps.size()), [&](int q) { memcpy(hs + cps[q].off, cps[q].src, cps[q].n); });
  SSX_HIP_TRY(ctx, hipMemcpyAsync(ws->raw_d.p, hs, in.off, hipMemcpyHostToDevice, ctx->stream));
  re.valid = true; re.key = pr->edge_pose; re.E = E;
  ws->raw_early = re;
  return SSX_OK;
}

ssx_status big_records(ssx_ctx* ctx, const ssx_ba_problem* pr, const HostPrep& h, BaDev& r, const int** pe_ptr_dev, const int** pe_edge_dev)
{
  if (!ctx->ba) { ctx->ba = new BaWorkspace(); ctx->ba_free = ssx_ba_workspace_free; }
  BaWorkspace* ws = ctx->ba;
  hipStream_t s = ctx->stream;
  const int P = h.P, L = h.L, E = h.E, nP = h.nP, nLm = h.nLm, nCh = h.nCh;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  int key_bits = 1;
  while ((1u << key_bits) < (unsigned)(nP + 1)) ++key_bits;
  size_t sort_tmp = 0;
  (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, (unsigned int*)nullptr, (unsigned int*)nullptr, (unsigned int*)nullptr, (unsigned int*)nullptr, (size_t)std::max(E, 1), 0, key_bits, s);
  const bool have_cam = pr->edge_cam != nullptr;
  // (the observation columns may be on the device already: raw_upload_early)
  const BaWorkspace::RawEarly early = ws->raw_early;
  const bool sent = early.valid && early.key == pr->edge_pose && early.E == E && E == h.E_raw;
  ws->raw_early.valid = false;
  Layout in;
  const size_t o_pose_free = in.take(sizeof(int) * P), o_lm_compact = in.take(sizeof(int) * (size_t)(L + 1));
  const size_t o_lm_ptr = in.take(sizeof(int) * (size_t)(nLm + 1)), o_lm_id = in.take(sizeof(int) * (size_t)(nLm + 1)), o_lm_fixed = in.take((size_t)nLm + 1);
  const size_t o_ch_lm = in.take(sizeof(int) * (size_t)(nCh + 1)), o_ch_desc = in.take(sizeof(int) * 4 * (size_t)(nCh + 1)), o_pe_ptr = in.take(sizeof(int) * (size_t)(nP + 1));
  const size_t o_r_pose = in.take(sent ? 0 : sizeof(int) * (size_t)(E + 1)), o_r_point = in.take(sent ? 0 : sizeof(int) * (size_t)(E + 1));
  const size_t o_r_uv = in.take(sent ? 0 : sizeof(double) * 2 * (size_t)(E + 1));
  const size_t o_r_cam = in.take(have_cam && !sent ? (size_t)E + 1 : 0), o_slot8 = in.take((size_t)E + 1);
  const size_t in_bytes = in.off;
  Layout all = in;
  const size_t o_perm = all.take(sizeof(int) * (size_t)(E + 1)), o_e_rec = all.take(sizeof(int) * 4 * (size_t)(E + 1)), o_l_rec = all.take(sizeof(int) * 4 * (size_t)(nLm + 1));
  const size_t o_e_dup = all.take((size_t)E + 1), o_e_uv = all.take(sizeof(double) * 2 * (size_t)(E + 1));
  const size_t o_e_pose = all.take(sizeof(int) * (size_t)(E + 1)), o_e_lmc = all.take(sizeof(int) * (size_t)(E + 1)), o_e_cam = all.take((size_t)E + 1);
  const size_t o_lm_chunk = all.take(sizeof(int) * (size_t)(nLm + 1)), o_pe_edge = all.take(sizeof(int) * (size_t)(E + 1)), o_c2 = all.take(sizeof(double) * (size_t)(E + 1));
  const size_t o_k0 = all.take(sizeof(int) * (size_t)(E + 1)), o_k1 = all.take(sizeof(int) * (size_t)(E + 1)), o_v0 = all.take(sizeof(int) * (size_t)(E + 1));
  const size_t o_tmp = all.take(sort_tmp + 256);
  SSX_HIP_TRY(ctx, ws->recs.reserve(all.off));
  SSX_HIP_TRY(ctx, ws->recs_h.reserve(in_bytes));
  char* hs = ws->recs_h.as<char>();
  char* dv = ws->recs.as<char>();
  memcpy(hs + o_pose_free, h.pose_free.data(), sizeof(int) * P);
  if (L) memcpy(hs + o_lm_compact, h.lm_compact.data(), sizeof(int) * (size_t)L);
  memcpy(hs + o_lm_ptr, h.lm_ptr.data(), sizeof(int) * (size_t)(nLm + 1));
  if (nLm) { memcpy(hs + o_lm_id, h.lm_id.data(), sizeof(int) * (size_t)nLm); memcpy(hs + o_lm_fixed, h.lm_fixed.data(), (size_t)nLm); }
  memcpy(hs + o_ch_lm, h.ch_lm.data(), sizeof(int) * h.ch_lm.size());
  if (nCh) memcpy(hs + o_ch_desc, h.ch_desc.data(), sizeof(int) * 4 * (size_t)nCh);
  memcpy(hs + o_pe_ptr, h.pe_ptr.data(), sizeof(int) * (size_t)(nP + 1));
  // the big columns on the worker pool (12 MB at 480 000 observations)
  struct Cp { size_t off; const void* src; size_t n; };
  std::vector<Cp> cps;
  auto add = [&](size_t off, const void* src, size_t n) {
    for (size_t a = 0; a < n; a += (size_t)1 << 20) cps.push_back({off + a, (const char*)src + a, std::min(n - a, (size_t)1 << 20)});
  };
  if (E) {
    if (!sent) {
      add(o_r_pose, pr->edge_pose, sizeof(int) * (size_t)E); add(o_r_point, pr->edge_point, sizeof(int) * (size_t)E);
      add(o_r_uv, pr->edge_uv, sizeof(double) * 2 * (size_t)E);
      if (have_cam) add(o_r_cam, pr->edge_cam, (size_t)E);
    }
    add(o_slot8, h.slot8.data(), (size_t)E);
  }
  ws->pool.run((int)cps.size(), std::min<int>(16, (int)cps.size()), [&](int q) { memcpy(hs + cps[q].off, cps[q].src, cps[q].n); });
  SSX_HIP_TRY(ctx, hipMemcpyAsync(dv, hs, in_bytes, hipMemcpyHostToDevice, s));
  r = BaDev{};
  r.P = P; r.L = L; r.E = E; r.E_raw = h.E_raw; r.nP = nP; r.nLm = nLm; r.nCh = nCh; r.nBlk = 0; r.big = 1; r.dev_prep = 1; r.bseg_cap = 0;
  r.pose_rank = nullptr;
  r.pose_free = (const int*)(dv + o_pose_free); r.lm_compact = (const int*)(dv + o_lm_compact); r.lm_ptr = (const int*)(dv + o_lm_ptr);
  r.lm_id = (const int*)(dv + o_lm_id); r.lm_fixed = (const uint8_t*)(dv + o_lm_fixed); r.ch_lm = (const int*)(dv + o_ch_lm);
  r.ch_desc = (const int4*)(dv + o_ch_desc);
  if (sent) {
    char* rd = ws->raw_d.as<char>();
    r.r_edge_pose = (const int*)(rd + early.o_pose); r.r_edge_point = (const int*)(rd + early.o_point); r.r_edge_uv = (const double*)(rd + early.o_uv);
    r.r_edge_cam = (const uint8_t*)(have_cam ? rd + early.o_cam : nullptr);
  } else {
    r.r_edge_pose = (const int*)(dv + o_r_pose); r.r_edge_point = (const int*)(dv + o_r_point); r.r_edge_uv = (const double*)(dv + o_r_uv);
    r.r_edge_cam = (const uint8_t*)(have_cam ? dv + o_r_cam : nullptr);
  }
  r.r_slot8 = (const uint8_t*)(dv + o_slot8);
  r.perm = (int*)(dv + o_perm); r.e_rec = (const int4*)(dv + o_e_rec); r.l_rec = (const int4*)(dv + o_l_rec); r.e_dup = (const uint8_t*)(dv + o_e_dup);
  r.e_uv = (const double*)(dv + o_e_uv); r.e_pose = (const int*)(dv + o_e_pose); r.e_lmc = (const int*)(dv + o_e_lmc); r.e_cam = (const uint8_t*)(dv + o_e_cam);
  r.lm_chunk = (int*)(dv + o_lm_chunk); r.c2_out = (double*)(dv + o_c2);
  r.pptr = (const uint16_t*)nullptr;
  *pe_ptr_dev = (const int*)(dv + o_pe_ptr);
  *pe_edge_dev = (const int*)(dv + o_pe_edge);
  if (E > 0 && nCh > 0) {
    hipLaunchKernelGGL(k_prep_scatter, dim3((h.E_raw + CH - 1) / CH), dim3(CH), 0, s, r);
    hipLaunchKernelGGL(k_prep_chunk, dim3(nCh), dim3(CH), 0, s, r);
    hipLaunchKernelGGL(k_pe_keys, dim3((E + CH - 1) / CH), dim3(CH), 0, s, r, (unsigned int*)(dv + o_k0), (unsigned int*)(dv + o_v0));
    if (rocprim::radix_sort_pairs(dv + o_tmp, sort_tmp, (unsigned int*)(dv + o_k0), (unsigned int*)(dv + o_k1), (unsigned int*)(dv + o_v0),
                                  (unsigned int*)(dv + o_pe_edge), (size_t)E, 0, key_bits, s) != hipSuccess) {
      ctx->set_error("ssx_ba: rocprim::radix_sort_pairs failed (pose-major edge list)"); return SSX_ERR_HIP;
    }
    SSX_HIP_TRY(ctx, hipGetLastError());
  }
  return SSX_OK;
}

// recs (nullable): the records already on the device (big_records)
ssx_status build_pairs(ssx_ctx* ctx, HostPrep& h, const unsigned long long** ab_dev, const BaDev* recs = nullptr)
{
  if (!ctx->ba) { ctx->ba = new BaWorkspace(); ctx->ba_free = ssx_ba_workspace_free; }
  BaWorkspace* ws = ctx->ba;
  hipStream_t s = ctx->stream;
  const int nLm = h.nLm, nP = h.nP, E = h.E, nCh = h.nCh;
  *ab_dev = nullptr;
  h.sblk_pa.clear(); h.sblk_pb.clear();
  auto add_diagonals_only = [&] {
    for (int p = 0; p < nP; ++p) { h.sblk_pa.push_back(p); h.sblk_pb.push_back(p); }
    h.spair_ptr.assign((size_t)nP + 1, 0);
    h.band_w = 0;
  };
  if (nLm == 0 || E == 0) { add_diagonals_only(); return SSX_OK; }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  // ---- stage A: records in, count + scan
  size_t scan_tmp = 0;
  (void)rocprim::exclusive_scan(nullptr, scan_tmp, (int*)nullptr, (int*)nullptr, 0, (size_t)nLm + 1, rocprim::plus<int>(), s);
  Layout la;
  const size_t a_erec = la.take(sizeof(int) * 4 * (size_t)E), a_lrec = la.take(sizeof(int) * 4 * (size_t)nLm), a_cd = la.take(sizeof(int) * 4 * (size_t)nCh);
  const size_t a_lmc = la.take(sizeof(int) * (size_t)nLm);
  const size_t a_in_bytes = la.off;
  const size_t a_cnt = la.take(sizeof(int) * ((size_t)nLm + 1)), a_off = la.take(sizeof(int) * ((size_t)nLm + 1)), a_scal = la.take(64), a_tmp = la.take(scan_tmp + 256);
  SSX_HIP_TRY(ctx, ws->pairs_a.reserve(la.off));
  SSX_HIP_TRY(ctx, ws->pairs_h.reserve(std::max(a_in_bytes, sizeof(int) * 2 * ((size_t)nP * (nP + 1) / 2 + 8))));
  char* da = ws->pairs_a.as<char>();
  char* hh = ws->pairs_h.as<char>();
  if (!recs) {
    memcpy(hh + a_erec, h.e_rec.data(), sizeof(int) * 4 * (size_t)E);
    memcpy(hh + a_lrec, h.l_rec.data(), sizeof(int) * 4 * (size_t)nLm);
    memcpy(hh + a_cd, h.ch_desc.data(), sizeof(int) * 4 * (size_t)nCh);
    memcpy(hh + a_lmc, h.lm_chunk.data(), sizeof(int) * (size_t)nLm);
    SSX_HIP_TRY(ctx, hipMemcpyAsync(da, hh, a_in_bytes, hipMemcpyHostToDevice, s));
  }
  SSX_HIP_TRY(ctx, hipMemsetAsync(da + a_cnt, 0, sizeof(int) * ((size_t)nLm + 1), s));
  SSX_HIP_TRY(ctx, hipMemsetAsync(da + a_scal, 0, 64, s));
  const int4* d_erec = recs ? (const int4*)recs->e_rec.p : (const int4*)(da + a_erec);
  const int4* d_lrec = recs ? (const int4*)recs->l_rec.p : (const int4*)(da + a_lrec);
  const int4* d_cd = recs ? (const int4*)recs->ch_desc.p : (const int4*)(da + a_cd);
  const int* d_lmc = recs ? (const int*)recs->lm_chunk.p : (const int*)(da + a_lmc);
  int* d_cnt = (int*)(da + a_cnt); int* d_off = (int*)(da + a_off); int* d_scal = (int*)(da + a_scal);
  hipLaunchKernelGGL(k_pairs_count, dim3((nLm + CH - 1) / CH), dim3(CH), 0, s, d_erec, d_lrec, d_cd, d_lmc, nLm, nP, d_cnt, d_scal);
  if (rocprim::exclusive_scan(da + a_tmp, scan_tmp, d_cnt, d_off, 0, (size_t)nLm + 1, rocprim::plus<int>(), s) != hipSuccess) {
    ctx->set_error("ssx_ba: rocprim::exclusive_scan failed"); return SSX_ERR_HIP;
  }
  int h_np_w[2] = {0, 0};
  SSX_HIP_TRY(ctx, hipMemcpyAsync(&h_np_w[0], d_off + nLm, sizeof(int), hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(&h_np_w[1], d_scal, sizeof(int), hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  const size_t NP = (size_t)h_np_w[0];
  if (NP == 0) { add_diagonals_only(); return SSX_OK; }
  // ---- stage B: emit, sort by block key, run-length encode
  int key_bits = 1;
  while ((1ull << key_bits) < (unsigned long long)nP * nP) ++key_bits;
  size_t sort_tmp = 0, rle_tmp = 0;
  (void)rocprim::radix_sort_pairs(nullptr, sort_tmp, (unsigned int*)nullptr, (unsigned int*)nullptr, (unsigned long long*)nullptr, (unsigned long long*)nullptr, NP, 0,
                                  key_bits, s);
  (void)rocprim::run_length_encode(nullptr, rle_tmp, (unsigned int*)nullptr, (unsigned int)NP, (unsigned int*)nullptr, (unsigned int*)nullptr, (unsigned int*)nullptr, s);
  const size_t max_blk = std::min((size_t)nP * (nP + 1) / 2, NP);
  Layout lb;
  const size_t b_k0 = lb.take(sizeof(unsigned int) * NP), b_k1 = lb.take(sizeof(unsigned int) * NP), b_v0 = lb.take(sizeof(unsigned long long) * NP);
  const size_t b_uq = lb.take(sizeof(unsigned int) * (max_blk + 1)), b_ct = lb.take(sizeof(unsigned int) * (max_blk + 1)), b_nr = lb.take(64);
  const size_t b_tmp = lb.take(std::max(sort_tmp, rle_tmp) + 256);
  SSX_HIP_TRY(ctx, ws->pairs_b.reserve(lb.off));
  SSX_HIP_TRY(ctx, ws->pairs_c.reserve(sizeof(unsigned long long) * NP + 64));
  char* db = ws->pairs_b.as<char>();
  unsigned int* d_k0 = (unsigned int*)(db + b_k0); unsigned int* d_k1 = (unsigned int*)(db + b_k1);
  unsigned long long* d_v0 = (unsigned long long*)(db + b_v0);
  unsigned long long* d_v1 = ws->pairs_c.as<unsigned long long>();   // the sorted values = the final lists
  unsigned int* d_uq = (unsigned int*)(db + b_uq); unsigned int* d_ct = (unsigned int*)(db + b_ct); unsigned int* d_nr = (unsigned int*)(db + b_nr);
  hipLaunchKernelGGL(k_pairs_emit, dim3((nLm + CH - 1) / CH), dim3(CH), 0, s, d_erec, d_lrec, d_cd, d_lmc, nLm, nP, (const int*)d_off, d_k0, d_v0);
  if (rocprim::radix_sort_pairs(db + b_tmp, sort_tmp, d_k0, d_k1, d_v0, d_v1, NP, 0, key_bits, s) != hipSuccess ||
      rocprim::run_length_encode(db + b_tmp, rle_tmp, d_k1, (unsigned int)NP, d_uq, d_ct, d_nr, s) != hipSuccess) {
    ctx->set_error("ssx_ba: rocprim radix_sort_pairs / run_length_encode failed"); return SSX_ERR_HIP;
  }
  unsigned int n_runs = 0;
  SSX_HIP_TRY(ctx, hipMemcpyAsync(&n_runs, d_nr, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  unsigned int* h_uq = reinterpret_cast<unsigned int*>(hh);
  unsigned int* h_ct = h_uq + n_runs;
  SSX_HIP_TRY(ctx, hipMemcpyAsync(h_uq, d_uq, sizeof(unsigned int) * n_runs, hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(h_ct, d_ct, sizeof(unsigned int) * n_runs, hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  // ---- the block list: the runs (sorted by key) merged with the diagonal blocks that have no pair (a pose whose
  // landmarks are all fixed still owns its Hpp block)
  h.spair_ptr.clear(); h.spair_ptr.push_back(0);
  unsigned int r = 0;
  int run_sum = 0;
  for (int p = 0; p < nP; ++p) {
    const unsigned int diag = (unsigned int)p * nP + p;
    bool have_diag = false;
    while (r < n_runs && h_uq[r] / (unsigned int)nP == (unsigned int)p) {      // the blocks of block-row p, ascending pb
      if (h_uq[r] > diag && !have_diag) { h.sblk_pa.push_back(p); h.sblk_pb.push_back(p); h.spair_ptr.push_back(run_sum); have_diag = true; }
      if (h_uq[r] == diag) have_diag = true;
      h.sblk_pa.push_back(p); h.sblk_pb.push_back((int)(h_uq[r] % (unsigned int)nP));
      run_sum += (int)h_ct[r];
      h.spair_ptr.push_back(run_sum);
      ++r;
    }
    if (!have_diag) { h.sblk_pa.push_back(p); h.sblk_pb.push_back(p); h.spair_ptr.push_back(run_sum); }
  }
  h.band_w = h_np_w[1];
  *ab_dev = d_v1;
  return SSX_OK;
}

size_t schur_lds_bytes()
{
  return BA_LDS_BYTES;
}

struct Comm {
  ssx_allreduce_fn fn = nullptr;
  void* user = nullptr;
  int world = 1;
};

ssx_status allreduce(ssx_ctx* ctx, const Comm& cm, double* buf, size_t count)
{
  if (!cm.fn) return SSX_OK;
  int rc = 0;
  SSX_PROF(ctx, KID_BA_COMM, rc = cm.fn(cm.user, buf, count, ctx->stream));
  if (rc != 0) {
    ctx->set_error("ssx_ba: the all-reduce hook reported a failure");
    return SSX_ERR_COMM;
  }
  return SSX_OK;
}

ssx_status launch_linearize(ssx_ctx* ctx, const BaDev& d, const BigDev& bd, const Comm& cm, int jac, int cur, int first_iteration)
{
  if (d.nCh > 0) {
    if (jac == SSX_JAC_NUMERIC_G2O) SSX_PROF(ctx, KID_BA_LINEARIZE, hipLaunchKernelGGL(k_linearize<SSX_JAC_NUMERIC_G2O>, dim3(d.nCh), dim3(CH), LIN_LDS_BYTES, ctx->stream, d, cur));
    else SSX_PROF(ctx, KID_BA_LINEARIZE, hipLaunchKernelGGL(k_linearize<SSX_JAC_ANALYTIC>, dim3(d.nCh), dim3(CH), LIN_LDS_BYTES, ctx->stream, d, cur));
  }
  if (d.big) {
    if (jac == SSX_JAC_NUMERIC_G2O) SSX_PROF(ctx, KID_BA_LINEARIZE, hipLaunchKernelGGL(k_pose_blocks<SSX_JAC_NUMERIC_G2O>, dim3(d.nP), dim3(CH), 0, ctx->stream, d, bd, cur));
    else SSX_PROF(ctx, KID_BA_LINEARIZE, hipLaunchKernelGGL(k_pose_blocks<SSX_JAC_ANALYTIC>, dim3(d.nP), dim3(CH), 0, ctx->stream, d, bd, cur));
    SSX_PROF(ctx, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_reduce_lin_big, dim3(1), dim3(CH), 0, ctx->stream, d));
  } else
  SSX_PROF(ctx, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_reduce_lin, dim3(std::max(1, (d.nP * 27 + 63) / 64)), dim3(CH), 0, ctx->stream, d));
  ssx_status st = allreduce(ctx, cm, d.iter_comm, (size_t)d.nP * 27 + 1 + d.world);
  if (st != SSX_OK) return st;
  // lambda_0 (first iteration of a round) and, after a collective, the global chi2
  if (first_iteration || cm.fn)
    SSX_PROF(ctx, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_lambda_init, dim3(1), dim3(64), 0, ctx->stream, d, first_iteration));
  SSX_HIP_TRY(ctx, hipGetLastError());
  return SSX_OK;
}

// Large systems: which 64x64 tiles of the Cholesky factor can be non-zero (shared by the large-window BA and the
// pose-graph optimisation).  blk_pa / blk_pb = the non-zero 6x6 blocks (free pose indices) of this rank's share of
// the system matrix.
ssx_status build_tile_lists(ssx_ctx* ctx, BaWorkspace* ws, const std::vector<int>& blk_pa, const std::vector<int>& blk_pb,
                            const Comm& cm, BigDev& bd, std::vector<int>& tl_row_cnt, std::vector<int>& tl_pair_cnt,
                            std::vector<uint8_t>& tl_next_diag)
{
  ssx_status st = SSX_OK;
  {
  // large windows: which 64x64 tiles of the factor can be non-zero.  The local co-visibility gives the tiles of this
  // rank's share of S; the union over the ranks (one small all-reduce of the T x T indicator) is the pattern of
  // the reduced system, and a symbolic elimination at tile level adds the fill.  A sliding window / odometry chain
  // gives a block-banded S: the panels then touch a handful of tiles instead of (T-k)^2 / 2.
    const int T = bd.T;
    SSX_HIP_TRY(ctx, ws->tiles_h.reserve(sizeof(double) * (size_t)T * T + 64));
    double* hp = ws->tiles_h.as<double>();
    std::fill(hp, hp + (size_t)T * T, 0.0);
    for (size_t q = 0; q < blk_pa.size(); ++q) {
      const int pa = blk_pa[q], pb = blk_pb[q];
      for (int ta = (6 * pa) / NB; ta <= (6 * pa + 5) / NB; ++ta)
        for (int tb = (6 * pb) / NB; tb <= (6 * pb + 5) / NB; ++tb)
          hp[(size_t)std::max(ta, tb) * T + std::min(ta, tb)] = 1.0;
    }
    if (cm.fn) {
      SSX_HIP_TRY(ctx, ws->tiles.reserve(sizeof(double) * (size_t)T * T + 64));
      SSX_HIP_TRY(ctx, hipMemcpyAsync(ws->tiles.p, hp, sizeof(double) * (size_t)T * T, hipMemcpyHostToDevice, ctx->stream));
      st = allreduce(ctx, cm, ws->tiles.as<double>(), (size_t)T * T);
      if (st != SSX_OK) return st;
      SSX_HIP_TRY(ctx, hipMemcpyAsync(hp, ws->tiles.p, sizeof(double) * (size_t)T * T, hipMemcpyDeviceToHost, ctx->stream));
      SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    std::vector<uint8_t> pat((size_t)T * T, 0);
    for (size_t i = 0; i < (size_t)T * T; ++i) pat[i] = hp[i] != 0.0;
    std::vector<int> init_bi, init_bj;
    for (int i = 0; i < T; ++i)
      for (int j = 0; j <= i; ++j)
        if (pat[(size_t)i * T + j] || i == j) { init_bi.push_back(i); init_bj.push_back(j); }
    std::vector<int> row_ptr(T + 1, 0), rows, pair_ptr(T + 1, 0), pair_bi, pair_bj, col_ptr(T + 1, 0), cols;
    std::vector<int> R;
    for (int k = 0; k < T; ++k) {
      R.clear();
      for (int i = k + 1; i < T; ++i) if (pat[(size_t)i * T + k]) R.push_back(i);
      for (size_t a = 0; a < R.size(); ++a)
        for (size_t c = 0; c <= a; ++c) pat[(size_t)R[a] * T + R[c]] = 1;       // fill
      R.push_back(T);                                                             // the rhs row tile
      for (int i : R) rows.push_back(i);
      row_ptr[k + 1] = (int)rows.size();
      for (size_t a = 0; a < R.size(); ++a)
        for (size_t c = 0; c <= a; ++c)
          if (R[c] != T) { pair_bi.push_back(R[a]); pair_bj.push_back(R[c]); }
      pair_ptr[k + 1] = (int)pair_bi.size();
    }
    for (int k = 0; k < T; ++k) {
      for (int j = 0; j < k; ++j) if (pat[(size_t)k * T + j]) cols.push_back(j);
      col_ptr[k + 1] = (int)cols.size();
    }
    tl_row_cnt.resize(T); tl_pair_cnt.resize(T); tl_next_diag.assign(T, 0);
    for (int k = 0; k < T; ++k) {
      tl_row_cnt[k] = row_ptr[k + 1] - row_ptr[k]; tl_pair_cnt[k] = pair_ptr[k + 1] - pair_ptr[k];
      // panel k's pair list holds (k+1, k+1) iff tile (k+1, k) is non-zero: k_syrk64 then also factors panel k+1's diagonal tile
      for (int q = pair_ptr[k]; q < pair_ptr[k + 1]; ++q)
        if (pair_bi[q] == k + 1 && pair_bj[q] == k + 1) tl_next_diag[k] = 1;
    }
    Layout tl;
    const size_t o_rp = tl.take(sizeof(int) * (T + 1)), o_r = tl.take(sizeof(int) * (rows.size() + 1));
    const size_t o_pp = tl.take(sizeof(int) * (T + 1)), o_pbi = tl.take(sizeof(int) * (pair_bi.size() + 1));
    const size_t o_pbj = tl.take(sizeof(int) * (pair_bj.size() + 1));
    const size_t o_cp = tl.take(sizeof(int) * (T + 1)), o_c = tl.take(sizeof(int) * (cols.size() + 1));
    const size_t o_ibi = tl.take(sizeof(int) * (init_bi.size() + 1)), o_ibj = tl.take(sizeof(int) * (init_bj.size() + 1));
    const size_t tl_lists = tl.off;
    const size_t o_spack = tl.take(cm.fn ? sizeof(double) * (init_bi.size() * (size_t)NB_TILE + bd.n_pad + 8) : 256);
    SSX_HIP_TRY(ctx, ws->tiles_h.reserve(tl_lists));
    SSX_HIP_TRY(ctx, ws->tiles.reserve(tl.off));
    char* th = ws->tiles_h.as<char>();
    memcpy(th + o_rp, row_ptr.data(), sizeof(int) * (T + 1)); memcpy(th + o_r, rows.data(), sizeof(int) * rows.size());
    memcpy(th + o_pp, pair_ptr.data(), sizeof(int) * (T + 1)); memcpy(th + o_pbi, pair_bi.data(), sizeof(int) * pair_bi.size());
    memcpy(th + o_pbj, pair_bj.data(), sizeof(int) * pair_bj.size());
    memcpy(th + o_cp, col_ptr.data(), sizeof(int) * (T + 1)); memcpy(th + o_c, cols.data(), sizeof(int) * cols.size());
    memcpy(th + o_ibi, init_bi.data(), sizeof(int) * init_bi.size()); memcpy(th + o_ibj, init_bj.data(), sizeof(int) * init_bj.size());
    SSX_HIP_TRY(ctx, hipMemcpyAsync(ws->tiles.p, th, tl_lists, hipMemcpyHostToDevice, ctx->stream));
    char* tb = ws->tiles.as<char>();
    bd.n_init = (int)init_bi.size();
    bd.tl_init_bi = (const int*)(tb + o_ibi); bd.tl_init_bj = (const int*)(tb + o_ibj);
    bd.Spack = (double*)(tb + o_spack);
    bd.tl_row_ptr = (const int*)(tb + o_rp); bd.tl_rows = (const int*)(tb + o_r);
    bd.tl_pair_ptr = (const int*)(tb + o_pp); bd.tl_pair_bi = (const int*)(tb + o_pbi); bd.tl_pair_bj = (const int*)(tb + o_pbj);
    bd.tl_col_ptr = (const int*)(tb + o_cp); bd.tl_cols = (const int*)(tb + o_c);
  }
  return SSX_OK;
}

}  // namespace

extern "C" {

void ssx_ba_default_options(ssx_ba_options* o)
{
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->outer_rounds = 5;
  o->iters = 10;
  o->chi2_th = 5.891;
  o->huber_delta = 5.891;
  o->inlier_ratio = 0.7;
  o->jac_mode = SSX_JAC_ANALYTIC;
  o->rank = 0;
  o->world_size = 1;
}

#ifndef SSX_NO_TEST_HOOKS   // kernel tap of the parity tests (include/ssx_test_hooks.h)
ssx_status ssx_ba_linearize(ssx_ctx* ctx, const ssx_ba_problem* prob, double huber_delta, int32_t jac_mode,
                            double* Hpp, double* bp, double* Hll, double* bl, double* Hpl, double* err,
                            double* chi2)
{
  if (!ctx || !prob) return SSX_ERR_INVALID_ARG;
  // the index lists are rebuilt per call (the window changes with every keyframe) but their storage is kept with the ctx:
  // ~20 vectors of up to E entries are not re-allocated and re-faulted every solve
  if (!ctx->ba) { ctx->ba = new BaWorkspace(); ctx->ba_free = ssx_ba_workspace_free; }
  HostPrep& h = ctx->ba->prep1;
  ssx_status st = prepare(ctx, prob, h, false);        // this hook returns per-edge blocks in the caller's order: it keeps the host's sort
  if (st != SSX_OK) return st;
  BaDev d;
  BigDev bd;
  BandPlan no_band;
  BandDev bnd;
  st = upload(ctx, prob, h, huber_delta, 5.891, 1, 0, d, bd, no_band, bnd);
  if (st != SSX_OK) return st;
  Comm cm;
  st = launch_linearize(ctx, d, bd, cm, jac_mode, 0, 1);
  if (st != SSX_OK) return st;
  const int P = h.P, L = h.L, E = h.E, nP = h.nP, nLm = h.nLm;
  std::vector<double> hHpp((size_t)nP * UPPER6 + 1), hbp((size_t)nP * 6 + 1), hHll((size_t)6 * nLm + 1), hbl((size_t)3 * nLm + 1),
      hW((size_t)18 * E + 1), herr((size_t)2 * E + 1), hscal(SC_N);
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hHpp.data(), d.Hpp, sizeof(double) * nP * UPPER6, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hbp.data(), d.bp, sizeof(double) * nP * 6, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hHll.data(), d.Hll, sizeof(double) * 6 * nLm, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hbl.data(), d.bl, sizeof(double) * 3 * nLm, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hW.data(), d.W, sizeof(double) * 18 * (size_t)E, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(herr.data(), d.err_lin, sizeof(double) * 2 * (size_t)E, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hscal.data(), d.scal, sizeof(double) * SC_N, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  static const int U_R[UPPER6] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5};
  static const int U_C[UPPER6] = {0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 2, 3, 4, 5, 3, 4, 5, 4, 5, 5};
  if (Hpp) memset(Hpp, 0, sizeof(double) * 36 * P);
  if (bp) memset(bp, 0, sizeof(double) * 6 * P);
  for (int p = 0; p < P; ++p) {
    const int pf = h.pose_free[p];
    if (pf < 0) continue;
    if (Hpp)
      for (int k = 0; k < UPPER6; ++k) {
        Hpp[36 * (size_t)p + U_R[k] * 6 + U_C[k]] = hHpp[(size_t)pf * UPPER6 + k];
        Hpp[36 * (size_t)p + U_C[k] * 6 + U_R[k]] = hHpp[(size_t)pf * UPPER6 + k];
      }
    if (bp) for (int k = 0; k < 6; ++k) bp[6 * (size_t)p + k] = hbp[(size_t)pf * 6 + k];
  }
  if (Hll) memset(Hll, 0, sizeof(double) * 9 * L);
  if (bl) memset(bl, 0, sizeof(double) * 3 * L);
  for (int lc = 0; lc < nLm; ++lc) {
    const int l = h.lm_id[lc];
    if (Hll) {
      const double a00 = hHll[lc], a01 = hHll[(size_t)nLm + lc], a02 = hHll[(size_t)2 * nLm + lc];
      const double a11 = hHll[(size_t)3 * nLm + lc], a12 = hHll[(size_t)4 * nLm + lc], a22 = hHll[(size_t)5 * nLm + lc];
      double* o = Hll + 9 * (size_t)l;
      o[0] = a00; o[1] = a01; o[2] = a02; o[3] = a01; o[4] = a11; o[5] = a12; o[6] = a02; o[7] = a12; o[8] = a22;
    }
    if (bl) for (int k = 0; k < 3; ++k) bl[3 * (size_t)l + k] = hbl[(size_t)k * nLm + lc];
  }
  for (int s = 0; s < E; ++s) {
    const int e = h.perm[s];
    if (Hpl) for (int k = 0; k < 18; ++k) Hpl[18 * (size_t)e + k] = hW[(size_t)k * E + s];
    if (err) {
      // an edge whose vertices are both fixed is not active in g2o (sparse_optimizer.cpp:237): its error is never computed
      const bool inactive = h.pose_free[h.e_pose[s]] < 0 && h.lm_fixed[h.e_lmc[s]];
      err[2 * (size_t)e] = inactive ? 0.0 : herr[s];
      err[2 * (size_t)e + 1] = inactive ? 0.0 : herr[(size_t)E + s];
    }
  }
  if (chi2) *chi2 = hscal[SC_CHI2_CUR];
  return SSX_OK;
}
#endif  // SSX_NO_TEST_HOOKS

}  // extern "C"

// ssx_ba_solve, and the solve of one ssx_ba_window (`ext`: raw arrays and state resident in the window's buffers)
static ssx_status ba_solve_impl(ssx_ctx* ctx, const ssx_ba_problem* prob, const ssx_ba_options* opt_in, ssx_ba_result* res, WinExt* ext)
{
  if (!ctx || !prob || !res) return SSX_ERR_INVALID_ARG;
  ssx_ba_options opt;
  if (opt_in) opt = *opt_in; else ssx_ba_default_options(&opt);
  // the index lists are rebuilt per call (the window changes with every keyframe) but their storage is kept with the ctx:
  // ~20 vectors of up to E entries are not re-allocated and re-faulted every solve
  if (!ctx->ba) { ctx->ba = new BaWorkspace(); ctx->ba_free = ssx_ba_workspace_free; }
  HostPrep& h = ctx->ba->prep1;
  static const bool timing = getenv("SSX_BA_TIMING") != nullptr;       // host phases of the call on stderr (tools/ba_c4_slope.py)
  const auto tc0 = std::chrono::steady_clock::now();
  auto tc_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc0).count(); };
  double tph[6] = {0, 0, 0, 0, 0, 0};
  {
    // a LARGE window (more than 16 free keyframes) with many observations: its columns start crossing PCIe before they are counted
    static const bool host_prep_env = getenv("SSX_BA_HOST_PREP") != nullptr || getenv("SSX_BA_HOST_LISTS") != nullptr;
    if (!ext && !host_prep_env && prob->E >= (1 << 16) && prob->P > SSX_BA_SMALL_P && prob->poses) {
      int n_free = 0;
      for (int i = 0; i < prob->P; ++i) n_free += !(prob->pose_fixed && prob->pose_fixed[i]);
      if (n_free > SSX_BA_SMALL_P) {
        const ssx_status st0 = raw_upload_early(ctx, prob);
        if (st0 != SSX_OK) return st0;
      }
    }
  }
  ssx_status st = prepare(ctx, prob, h, true, ext);
  if (st != SSX_OK || !(h.big && h.dev_prep)) ctx->ba->raw_early.valid = false;   // (never reaches big_records: the early copy is dropped)
  if (st != SSX_OK) return st;
  tph[0] = tc_ms();
  if (ext && (!h.dev_prep || h.big)) {
    ctx->set_error("ssx_ba_window: %d free keyframes (a window holds at most %d) or the device-side marshalling is switched off", h.nP, SSX_BA_SMALL_P);
    return SSX_ERR_UNSUPPORTED;
  }
  Comm cm;
  // world_size 1 with a hook is allowed (the hook is then an identity): it exercises the collective plumbing
  if (opt.comm) {                                   // RCCL inside the library (comm.hip): ncclAllReduce on the ctx stream
    cm.fn = ssx_comm_allreduce_f64; cm.user = opt.comm;
    (void)ssx_comm_info(opt.comm, &opt.rank, &opt.world_size);
    cm.world = opt.world_size;
  } else
  if (opt.allreduce && opt.world_size >= 1) { cm.fn = opt.allreduce; cm.user = opt.allreduce_user; cm.world = opt.world_size; }
  if (cm.fn && (opt.rank < 0 || opt.rank >= cm.world || cm.world > 64)) {
    ctx->set_error("ssx_ba_solve: invalid rank %d / world_size %d", opt.rank, cm.world);
    return SSX_ERR_INVALID_ARG;
  }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  SSX_HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  // collect_stats: every launch of this call is bracketed by HIP events (the SSX_PROF machinery of ssx_profile_begin),
  // summed per phase at the end; the guard switches it off again on every exit path
  struct StatsGuard {
    ssx_ctx* c; bool mine;
    ~StatsGuard() { if (mine) { c->prof.on = false; c->prof.recs.clear(); c->prof.used = 0; } }
  } stats_guard{ctx, opt.collect_stats != 0 && !ctx->prof.on};
  if (stats_guard.mine) { ctx->prof.on = true; ctx->prof.used = 0; ctx->prof.recs.clear(); }
  res->ms_linearize = res->ms_schur = res->ms_linear_solution = res->ms_update = res->ms_reduce = res->ms_comm = 0.f;
  BaDev d;
  BigDev bd;
  // large windows: trajectory-shaped co-visibility (cyclic block band) -> the sliding-window / nested-dissection solver
  // of ba_band.inc; anything else -> the 64x64-tile sparse Cholesky of ba_big.inc.  With several ranks the decision
  // must be common: the ranks exchange which bandwidth class their shard falls in (one tiny all-reduce).
  const unsigned long long* pairs_dev = nullptr;
  BaDev recs;
  const int* pe_ptr_dev = nullptr; const int* pe_edge_dev = nullptr;
  const bool big_dev = h.big && h.dev_prep;
  if (big_dev) {
    st = big_records(ctx, prob, h, recs, &pe_ptr_dev, &pe_edge_dev);
    if (st != SSX_OK) return st;
  }
  if (h.big) {
    st = build_pairs(ctx, h, &pairs_dev, big_dev ? &recs : nullptr);
    if (st != SSX_OK) return st;
  }
  tph[1] = tc_ms();
  BandPlan bp;
  if (h.big && opt.large_solver != SSX_LARGE_SOLVER_TILES) {
    int w = std::max(h.band_w, 1);
    if (w > BAND_WMAX) w = BAND_WMAX + 1;
    if (cm.fn) {
      if (!ctx->ba) { ctx->ba = new BaWorkspace(); ctx->ba_free = ssx_ba_workspace_free; }
      BaWorkspace* w0 = ctx->ba;
      double hist[BAND_WMAX + 2] = {0};
      hist[w] = 1.0;
      SSX_HIP_TRY(ctx, w0->tiles.reserve(sizeof(hist)));
      SSX_HIP_TRY(ctx, hipMemcpyAsync(w0->tiles.p, hist, sizeof(hist), hipMemcpyHostToDevice, ctx->stream));
      SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      st = allreduce(ctx, cm, w0->tiles.as<double>(), BAND_WMAX + 2);
      if (st != SSX_OK) return st;
      SSX_HIP_TRY(ctx, hipMemcpyAsync(hist, w0->tiles.p, sizeof(hist), hipMemcpyDeviceToHost, ctx->stream));
      SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      for (int i = 1; i <= BAND_WMAX + 1; ++i) if (hist[i] != 0.0) w = i;
    }
    if (w <= BAND_WMAX && h.nP >= 2 * w + 2) { plan_band(h.nP, w, bp); plan_bcr(h.nP, w, bp.bcr); }
  }
  if (h.big && opt.large_solver == SSX_LARGE_SOLVER_BAND && bp.w == 0) {
    ctx->set_error("ssx_ba_solve: the band solver was requested but the co-visibility bandwidth is %d poses (> %d)", h.band_w, BAND_WMAX);
    return SSX_ERR_UNSUPPORTED;
  }
  BandDev bnd;
  st = upload(ctx, prob, h, opt.huber_delta, opt.chi2_th, cm.world, cm.fn ? opt.rank : 0, d, bd, bp, bnd, nullptr, ext, big_dev ? &recs : nullptr, pe_ptr_dev, pe_edge_dev);
  if (st != SSX_OK) return st;
  tph[2] = tc_ms();
  d.store_w = (d.big || opt.jac_mode == SSX_JAC_NUMERIC_G2O) ? 1 : 0;
  d.no_err = (!d.big && !(res->edge_chi2 || res->edge_outlier)) ? 1 : 0;
  bd.spair_ab = pairs_dev;
  BaWorkspace* ws = ctx->ba;
  double* hscal = ws->scal.as<double>();
  const int n = 6 * d.nP;
  const int nCh = d.nCh;
  const size_t lds_schur = schur_lds_bytes();
  const size_t lds_fused = std::max(lds_schur, LIN_LDS_BYTES);
  const size_t lds_prep = sizeof(double) * (18 + 9 + 3) * PW + 64;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_lin_schur<SSX_JAC_ANALYTIC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fused);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_lin_schur<SSX_JAC_NUMERIC_G2O>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fused);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_linearize<SSX_JAC_ANALYTIC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LIN_LDS_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_linearize<SSX_JAC_NUMERIC_G2O>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LIN_LDS_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_schur), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_schur);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_schur_prep), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_prep);
    attr_set = true;
  }
  std::vector<int> tl_row_cnt, tl_pair_cnt;
  std::vector<uint8_t> tl_next_diag;
  if (d.big && !bnd.on) {
    st = build_tile_lists(ctx, ws, h.sblk_pa, h.sblk_pb, cm, bd, tl_row_cnt, tl_pair_cnt, tl_next_diag);
    if (st != SSX_OK) return st;
  }
  size_t lds_seg = 0, lds_top = 0, lds_back = 0;
  if (bnd.on) {
    const int w1 = bnd.K == 1 ? bnd.w : bnd.wr, n1 = bnd.K == 1 ? bnd.nP : bnd.nPr;
    int m_max = 0;
    for (int m : bp.seg_m) m_max = std::max(m_max, m);
    lds_seg = band_lds_elim(bnd.w, bnd.w);
    lds_top = std::max(band_lds_elim(w1, bnd.w), band_lds_back(w1, bnd.w, n1));
    lds_back = band_lds_back(bnd.w, bnd.w, m_max + 2 * bnd.w);
    static size_t set_seg = 0, set_top = 0, set_back = 0;            // raise the dynamic-LDS limits once per size class
    if (lds_seg > set_seg) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_band_seg), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_seg); set_seg = lds_seg; }
    if (lds_top > set_top) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_band_top), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_top); set_top = lds_top; }
    if (lds_back > set_back) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_band_back), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_back); set_back = lds_back; }
  }
  // large windows: Schur blocks -> dense S (+ rhs row) -> all-reduce -> blocked Cholesky (MFMA) -> back-substitution
  // fuse_iter: the trial's all-reduce also carries iter_comm (pose blocks, chi2, max-diagonal slots of the linearisation), which
  // then needs no collective of its own: two all-reduces per LM trial instead of three
  // (damping, state buffer and stop flag come from the device's LM control block: the kernels shared with the pose graph are told
  // so by cur = -1, lambda_arg = 0, use_dev_lambda = 2)
  auto big_trial = [&](bool fuse_iter) -> ssx_status {
    hipStream_t s = ctx->stream;
    if (bnd.on) {
      // Schur blocks straight into the band layout -> (all-reduce) -> segments || -> separator system -> segments ||
      const size_t band_doubles = (size_t)bnd.nP * (bnd.w + 1) * 36;
      SSX_HIP_TRY(ctx, hipMemsetAsync(bnd.Sb, 0, sizeof(double) * band_doubles, s));
      if (nCh > 0) SSX_PROF(ctx, KID_BA_SCHUR, hipLaunchKernelGGL(k_schur_prep, dim3(nCh), dim3(CH), lds_prep, s, d, bd));
      SSX_PROF(ctx, KID_BA_SCHUR, hipLaunchKernelGGL(k_schur_blocks_band, dim3((bd.nBlkS + 3) / 4), dim3(CH), 0, s, d, bd, bnd));
      SSX_PROF(ctx, KID_BA_REDUCE_SCHUR, hipLaunchKernelGGL(k_bs_band, dim3(d.nP), dim3(CH), 0, s, d, bd, bnd));
      ssx_status st2 = allreduce(ctx, cm, bnd.Sb, band_doubles + (size_t)bd.n + (fuse_iter ? (size_t)d.nP * 27 + 1 + d.world : 0));
      if (st2 != SSX_OK) return st2;
      if (fuse_iter) SSX_PROF(ctx, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_lambda_init, dim3(1), dim3(64), 0, s, d, 0));   // the global chi2 of the linearisation
      if (bnd.bcr.on) {
        // block cyclic reduction: log2(N) levels of concurrent super-block eliminations, then as many of back-substitution
        const std::vector<int>& lv = bp.bcr.lvl;
        SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_bcr_build, dim3(bnd.bcr.N), dim3(256), 0, s, d, bnd, bnd.bcr, 0.0, 2));
        const bool m24 = bnd.bcr.m == 24;
        const std::vector<int>& lm = bp.bcr.lvM;
        for (size_t q = 0; q < lm.size(); ++q) {
          const int cnt = lv[q + 1] - lv[q], sh = (int)q;
          if (m24) SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_bcr_fwd<24>, dim3(cnt, BCR_S), dim3(BCR_T), 0, s, d, bnd.bcr, sh, lm[q], 1));
          else SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_bcr_fwd<36>, dim3(cnt, BCR_S), dim3(BCR_T), 0, s, d, bnd.bcr, sh, lm[q], 1));
        }
        for (size_t q = lm.size(); q-- > 0;) {
          const int cnt = lv[q + 1] - lv[q], sh = (int)q;
          if (m24) SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_bcr_bwd<24>, dim3(cnt), dim3(256), 0, s, d, bnd.bcr, bd, sh, lm[q], 1));
          else SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_bcr_bwd<36>, dim3(cnt), dim3(256), 0, s, d, bnd.bcr, bd, sh, lm[q], 1));
        }
      } else {
      if (bnd.K > 1) {
        SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_band_seg, dim3(bnd.K), dim3(BAND_T), lds_seg, s, d, bnd));
        const int total = bnd.nPr * (bnd.wr + 1) * 36 + 6 * bnd.nPr;
        SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_band_assemble, dim3(std::min(64, (total + BAND_T - 1) / BAND_T)), dim3(BAND_T), 0, s, d, bnd));
      }
      SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_band_top, dim3(1), dim3(BAND_TOP_T), lds_top, s, d, bnd, bd));
      if (bnd.K > 1) SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_band_back, dim3(bnd.K), dim3(BAND_T), lds_back, s, d, bnd, bd));
      }
      const int nparts = std::min(32, (d.P + CH - 1) / CH);
      SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_pose_update_big, dim3(nparts), dim3(CH), 0, s, d, bd, -1, 0.0, 2));
      SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_scale_finish, dim3(1), dim3(64), 0, s, d, bd, nparts));
      return SSX_OK;
    }
    SSX_HIP_TRY(ctx, hipMemsetAsync(bd.S, 0, sizeof(double) * (size_t)(bd.n_pad + 1) * bd.ld, s));
    if (nCh > 0) SSX_PROF(ctx, KID_BA_SCHUR, hipLaunchKernelGGL(k_schur_prep, dim3(nCh), dim3(CH), lds_prep, s, d, bd));
    SSX_PROF(ctx, KID_BA_SCHUR, hipLaunchKernelGGL(k_schur_blocks, dim3((bd.nBlkS + 3) / 4), dim3(CH), 0, s, d, bd));
    SSX_PROF(ctx, KID_BA_REDUCE_SCHUR, hipLaunchKernelGGL(k_bs, dim3(d.nP), dim3(CH), 0, s, d, bd));
    if (cm.fn) {
      // exchange the non-zero tiles and the rhs row only
      hipLaunchKernelGGL(k_pack_tiles, dim3(bd.n_init + 1), dim3(CH), 0, s, bd, 0);
      ssx_status st2 = allreduce(ctx, cm, bd.Spack, (size_t)bd.n_init * NB_TILE + bd.n_pad);
      if (st2 != SSX_OK) return st2;
      hipLaunchKernelGGL(k_pack_tiles, dim3(bd.n_init + 1), dim3(CH), 0, s, bd, 1);
    }
    SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_add_lambda, dim3((bd.n + 255) / 256), dim3(256), 0, s, d, bd, 0.0, 2));
    for (int kb = 0; kb < bd.T; ++kb) {
      if (kb == 0 || !tl_next_diag[kb - 1])   // else the previous panel's k_syrk64 has factored this diagonal tile
        SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_potrf64, dim3(1), dim3(CH), 0, s, d, bd, kb));
      // the structurally non-zero row tiles below the panel (always the rhs row tile), then their pairs
      SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_trsm64, dim3(tl_row_cnt[kb]), dim3(CH), 0, s, bd, kb));
      if (tl_pair_cnt[kb] > 0) SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_syrk64, dim3(tl_pair_cnt[kb]), dim3(CH), 0, s, d, bd, kb));
    }
    SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_backsolve, dim3(1), dim3(1024), 0, s, bd));
    const int nparts = std::min(32, (d.P + CH - 1) / CH);
    SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_pose_update_big, dim3(nparts), dim3(CH), 0, s, d, bd, -1, 0.0, 2));
    SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_scale_finish, dim3(1), dim3(64), 0, s, d, bd, nparts));
    return SSX_OK;
  };
  const int nSchurEntries = d.nBlk * 36 + d.nP * 6;

  res->rounds = 0; res->n_iters = 0; res->n_inliers = 0; res->n_outliers = 0;
  int cur = ext ? ext->cur : 0; // index of the accepted state buffer
  // the download block in pinned memory (poses | points | errors), written by k_pack_one behind the last slot of an optimize() on one rank
  double* const pk_pose = reinterpret_cast<double*>(ws->stage.as<char>());
  double* const pk_point = pk_pose + 7 * (size_t)d.P;
  double* const pk_err = pk_point + 3 * (size_t)d.L;
  static const bool no_pack_env = getenv("SSX_BA_NO_PACK") != nullptr;       // (tools: the three copies of before, for A/B timing)
  const bool pack_ok = !cm.fn && !no_pack_env;
  const bool pack_err = pack_ok && (res->edge_chi2 || res->edge_outlier) && d.E > 0 && d.dev_prep;
  bool packed = false;                                                       // the pinned block holds the state the stream will end with
  bool have_trial_err = false; // err_trial holds the errors of the last trial evaluated
  int round = 0;
  // with several ranks every rank must take part in every collective, even with an empty shard
  const bool active = (nCh > 0) || cm.fn != nullptr;
  double n_out_total = 0.0;
  while (round < opt.outer_rounds) {
    // ---- one g2o optimize(iters): OptimizationAlgorithmLevenberg::solve per iteration.  The whole optimize(iters) is enqueued;
    // lm_step() on the device decides after every trial (no stream synchronisation per trial) ----
    // One slot = (re)linearise if needed + one trial.  A rejected trial consumes a slot without finishing its
    // iteration, so after the first `iters` slots the host looks at the control block once and tops up.
    hipLaunchKernelGGL(k_lm_begin, dim3(1), dim3(1), 0, ctx->stream, d, cur, opt.iters, res->n_iters, active ? 0 : 1);
    int slots_total = 0;
    bool first_slot = true;
    while (active && opt.iters > 0) {
      int slots = slots_total == 0 ? opt.iters : std::max(1, opt.iters - (int)hscal[SC_IT]);
      for (int sidx = 0; sidx < slots; ++sidx) {
        // the first slot of an optimize() needs lambda_0 between the linearisation and the Schur complement; every
        // later slot (and every slot with a collective between the two) knows its damping: one fused kernel
        const bool fused = !d.big && !first_slot && !cm.fn && nCh > 0 && n > 0;
        if (d.big) {
          // (k_linearize skips itself while the kept linearisation is valid; the pose blocks too unless a collective follows:
          // their all-reduced copy must be rebuilt from this rank's part before it is summed again)
          const int pb_cur = cm.fn ? -1 : -2;
          if (nCh > 0) {
            if (opt.jac_mode == SSX_JAC_NUMERIC_G2O) SSX_PROF(ctx, KID_BA_LINEARIZE, hipLaunchKernelGGL(k_linearize<SSX_JAC_NUMERIC_G2O>, dim3(nCh), dim3(CH), LIN_LDS_BYTES, ctx->stream, d, -1));
            else SSX_PROF(ctx, KID_BA_LINEARIZE, hipLaunchKernelGGL(k_linearize<SSX_JAC_ANALYTIC>, dim3(nCh), dim3(CH), LIN_LDS_BYTES, ctx->stream, d, -1));
          }
          if (opt.jac_mode == SSX_JAC_NUMERIC_G2O) SSX_PROF(ctx, KID_BA_LINEARIZE, hipLaunchKernelGGL(k_pose_blocks<SSX_JAC_NUMERIC_G2O>, dim3(d.nP), dim3(CH), 0, ctx->stream, d, bd, pb_cur));
          else SSX_PROF(ctx, KID_BA_LINEARIZE, hipLaunchKernelGGL(k_pose_blocks<SSX_JAC_ANALYTIC>, dim3(d.nP), dim3(CH), 0, ctx->stream, d, bd, pb_cur));
          SSX_PROF(ctx, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_reduce_lin_big, dim3(1), dim3(CH), 0, ctx->stream, d));
        } else
        if (fused) {
          if (opt.jac_mode == SSX_JAC_NUMERIC_G2O) SSX_PROF(ctx, KID_BA_LIN_SCHUR, hipLaunchKernelGGL(k_lin_schur<SSX_JAC_NUMERIC_G2O>, dim3(nCh), dim3(CH), lds_fused, ctx->stream, d));
          else SSX_PROF(ctx, KID_BA_LIN_SCHUR, hipLaunchKernelGGL(k_lin_schur<SSX_JAC_ANALYTIC>, dim3(nCh), dim3(CH), lds_fused, ctx->stream, d));
        } else if (nCh > 0) {
          if (opt.jac_mode == SSX_JAC_NUMERIC_G2O) SSX_PROF(ctx, KID_BA_LINEARIZE, hipLaunchKernelGGL(k_linearize<SSX_JAC_NUMERIC_G2O>, dim3(nCh), dim3(CH), LIN_LDS_BYTES, ctx->stream, d, -1));
          else SSX_PROF(ctx, KID_BA_LINEARIZE, hipLaunchKernelGGL(k_linearize<SSX_JAC_ANALYTIC>, dim3(nCh), dim3(CH), LIN_LDS_BYTES, ctx->stream, d, -1));
        }
        // later slots of a single-rank solve: the two reductions as one launch (the first slot needs lambda between them, ranks an all-reduce)
        static const bool no_both_env = getenv("SSX_BA_SPLIT_REDUCE") != nullptr;   // (tools: the two launches, for A/B timing)
        const bool both = !d.big && fused && !first_slot && !cm.fn && n > 0 && !no_both_env;
        const int n_rl = std::max(1, (d.nP * 27 + 63) / 64);
        if (both) SSX_PROF(ctx, KID_BA_REDUCE_SCHUR, hipLaunchKernelGGL(k_reduce_both, dim3(n_rl + (nSchurEntries + 63) / 64), dim3(CH), 0, ctx->stream, d, n_rl));
        else if (!d.big) SSX_PROF(ctx, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_reduce_lin, dim3(n_rl), dim3(CH), 0, ctx->stream, d));
        // (band solver, later slots: lambda is known, so the linearisation's sums travel with the trial's reduced system)
        const bool fuse_iter = d.big && bnd.on && cm.fn && !first_slot;
        if (!fuse_iter) {
          st = allreduce(ctx, cm, d.iter_comm, (size_t)d.nP * 27 + 1 + d.world);
          if (st != SSX_OK) return st;
          if (first_slot || cm.fn) SSX_PROF(ctx, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_lambda_init, dim3(1), dim3(64), 0, ctx->stream, d, first_slot ? 1 : 0));
        }
        first_slot = false;
        if (d.big) {
          st = big_trial(fuse_iter);
          if (st != SSX_OK) return st;
        } else {
        if (n > 0) {
          if (nCh > 0 && !fused) SSX_PROF(ctx, KID_BA_SCHUR, hipLaunchKernelGGL(k_schur, dim3(nCh), dim3(CH), lds_schur, ctx->stream, d));
          if (!both) SSX_PROF(ctx, KID_BA_REDUCE_SCHUR, hipLaunchKernelGGL(k_reduce_schur, dim3((nSchurEntries + 63) / 64), dim3(CH), 0, ctx->stream, d));
          st = allreduce(ctx, cm, d.trial_comm, (size_t)n * n + n);
          if (st != SSX_OK) return st;
        }
        if (n <= NB) SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_solve64, dim3(1), dim3(CH), 0, ctx->stream, d));
        else if (n <= 80) SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_solve80, dim3(1), dim3(CH), 0, ctx->stream, d));
        else SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_solve, dim3(1), dim3(CH), 0, ctx->stream, d));
        }
        // one GPU: the last chunk of k_backsub_residual sums the trial and takes the LM decision itself (finish)
        const bool finish = nCh > 0 && !cm.fn && g_trial_finish.load() != 0;
        if (nCh > 0) SSX_PROF(ctx, KID_BA_BACKSUB, hipLaunchKernelGGL(k_backsub_residual, dim3(nCh), dim3(CH), 0, ctx->stream, d, finish ? 1 : 0));
        if (!finish) SSX_PROF(ctx, KID_BA_REDUCE_TRIAL, hipLaunchKernelGGL(k_reduce_trial, dim3(1), dim3(CH), 0, ctx->stream, d, cm.fn ? 0 : 1));
        if (cm.fn) {
          st = allreduce(ctx, cm, d.scal_comm, 3);
          if (st != SSX_OK) return st;
          SSX_PROF(ctx, KID_BA_REDUCE_TRIAL, hipLaunchKernelGGL(k_publish_trial, dim3(1), dim3(1), 0, ctx->stream, d));
        }
      }
      slots_total += slots;
      SSX_HIP_TRY(ctx, hipGetLastError());
      if (pack_ok) {
        // one rank: the control block, the statistics and the estimate (and the per-edge chi2 of a device-marshalled window) leave in
        // ONE kernel-written block behind the last slot -- if this optimize() was the last one the download below finds everything there
        if (pack_err) {
          hipLaunchKernelGGL(k_c2_out, dim3((d.E + CH - 1) / CH), dim3(CH), 0, ctx->stream, d, have_trial_err ? 1 : 2);
          hipLaunchKernelGGL(k_stream_out, dim3((unsigned)std::min<size_t>(256, ((size_t)d.E_raw + 2 * CH - 1) / (2 * CH))), dim3(CH), 0, ctx->stream, (const double*)d.c2_out, pk_err, (size_t)d.E_raw);
        }
        const size_t n_pack = SC_N + 3 * SSX_BA_MAX_STATS + 7 * (size_t)d.P + 3 * (size_t)d.L;
        hipLaunchKernelGGL(k_pack_one, dim3((unsigned)std::min<size_t>(256, (n_pack + CH - 1) / CH)), dim3(CH), 0, ctx->stream, d, hscal, pk_pose, pk_point);
        SSX_HIP_TRY(ctx, hipGetLastError());
        packed = true;
      } else {
        SSX_HIP_TRY(ctx, hipMemcpyAsync(hscal, d.scal, sizeof(double) * SC_N, hipMemcpyDeviceToHost, ctx->stream));
      }
      SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // the one host round trip of an optimize(iters)
      if (hscal[SC_STOP] != 0.0) break;
    }
    if (active && opt.iters > 0) {
      cur = (int)hscal[SC_CUR];
      n_out_total = hscal[SC_NOUT];
      if (hscal[SC_TRIALS_RUN] > 0.0) have_trial_err = true;
      const int n_done = (int)hscal[SC_NSTAT];
      if (n_done > res->n_iters) {
        double* hstat = hscal + SC_N;                                // pinned, behind the scalar block
        if (!packed) {                                               // (k_pack_one brought them along)
          SSX_HIP_TRY(ctx, hipMemcpyAsync(hstat, d.lm_stat, sizeof(double) * 3 * SSX_BA_MAX_STATS, hipMemcpyDeviceToHost, ctx->stream));
          SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        for (int k = res->n_iters; k < n_done && k < SSX_BA_MAX_STATS; ++k) {
          res->iter_chi2[k] = hstat[k];
          res->iter_lambda[k] = hstat[SSX_BA_MAX_STATS + k];
          res->iter_trials[k] = (int)hstat[2 * SSX_BA_MAX_STATS + k];
        }
        res->n_iters = n_done;
      }
    }
    res->rounds++;
    // outlier statistics of this round from the errors of the last evaluated trial (backend.cpp:181-194);
    // with several ranks n_out_total is already the global count: compare with the global edge count
    double n_edges_total = (double)d.E;
    if (cm.fn) {
      double e_local = (double)d.E;
      SSX_HIP_TRY(ctx, hipMemcpyAsync(d.scal_comm, &e_local, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // e_local is a stack variable
      st = allreduce(ctx, cm, d.scal_comm, 1);
      if (st != SSX_OK) return st;
      SSX_HIP_TRY(ctx, hipMemcpyAsync(&n_edges_total, d.scal_comm, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    const double cnt_out = n_out_total, cnt_in = n_edges_total - cnt_out;
    res->n_outliers = (int)cnt_out;
    res->n_inliers = (int)cnt_in;
    const double ratio = (n_edges_total > 0) ? cnt_in / (cnt_in + cnt_out) : 1.0;
    if (ratio > opt.inlier_ratio) break;
    ++round;
  }

  // ---- download ----
  char* hs = ws->stage.as<char>();
  double* h_pose = reinterpret_cast<double*>(hs);
  double* h_point = h_pose + 7 * (size_t)d.P;
  double* h_err = h_point + 3 * (size_t)d.L;
  if (!packed) {
    SSX_HIP_TRY(ctx, hipMemcpyAsync(h_pose, d.pose[cur], sizeof(double) * 7 * d.P, hipMemcpyDeviceToHost, ctx->stream));
    if (d.L) SSX_HIP_TRY(ctx, hipMemcpyAsync(h_point, d.point[cur], sizeof(double) * 3 * d.L, hipMemcpyDeviceToHost, ctx->stream));
  }
  const bool want_err = (res->edge_chi2 || res->edge_outlier) && d.E > 0;
  if (want_err && !(packed && pack_err)) {
    if (!have_trial_err) {   // iters == 0: errors of the input state
      Comm none;
      st = launch_linearize(ctx, d, bd, none, SSX_JAC_ANALYTIC, cur, 0);
      if (st != SSX_OK) return st;
    }
    if (d.dev_prep) {                                  // chi2 per edge, already in the caller's order
      hipLaunchKernelGGL(k_c2_out, dim3((d.E + CH - 1) / CH), dim3(CH), 0, ctx->stream, d, have_trial_err ? 1 : 0);
      SSX_HIP_TRY(ctx, hipMemcpyAsync(h_err, d.c2_out, sizeof(double) * (size_t)d.E_raw, hipMemcpyDeviceToHost, ctx->stream));
    } else
    SSX_HIP_TRY(ctx, hipMemcpyAsync(h_err, have_trial_err ? d.err_trial : d.err_lin, sizeof(double) * 2 * (size_t)d.E,
                                    hipMemcpyDeviceToHost, ctx->stream));
  }
  SSX_HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  tph[3] = tc_ms();
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  tph[4] = tc_ms();
  if (res->poses_out) memcpy(res->poses_out, h_pose, sizeof(double) * 7 * d.P);
  if (res->points_out && d.L) memcpy(res->points_out, h_point, sizeof(double) * 3 * d.L);
  if (ext) ext->cur = cur;
  if (want_err && d.dev_prep) {
    for (int e = 0; e < d.E_raw; ++e) {
      if (ext && prob->edge_point[e] < 0) continue;                  // a dead entry of the window's storage: never evaluated
      if (res->edge_chi2) res->edge_chi2[e] = h_err[e];
      if (res->edge_outlier) res->edge_outlier[e] = h_err[e] > opt.chi2_th;
    }
  } else if (want_err) {
    for (int s = 0; s < d.E; ++s) {
      const int e = h.perm[s];
      const double c2 = h_err[s] * h_err[s] + h_err[(size_t)d.E + s] * h_err[(size_t)d.E + s];
      if (res->edge_chi2) res->edge_chi2[e] = c2;
      if (res->edge_outlier) res->edge_outlier[e] = c2 > opt.chi2_th;
    }
  }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  res->ms_total = ms;
  res->ms_setup = 0.f;
  if (timing)
    fprintf(stderr, "ssx_ba_solve P %d L %d E %d: (columns staged + sent early, large windows) + prepare %.3f | records + pairs %.3f | plan + upload %.3f | LM enqueued (and its host round trips) %.3f | "
                    "last sync %.3f | results %.3f ms (host clock); GPU first to last event %.3f ms\n", d.P, d.L, d.E, tph[0], tph[1] - tph[0],
            tph[2] - tph[1], tph[3] - tph[2], tph[4] - tph[3], tc_ms() - tph[4], ms);
  if (stats_guard.mine)
    for (const auto& r : ctx->prof.recs) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) continue;
      switch (r.id) {
        case KID_BA_LINEARIZE: res->ms_linearize += t; break;
        case KID_BA_SCHUR: res->ms_schur += t; break;
        case KID_BA_LIN_SCHUR: res->ms_schur += t; break;        // (the fused slot: linearisation + elimination in one kernel)
        case KID_BA_SOLVE: res->ms_linear_solution += t; break;
        case KID_BA_BACKSUB: res->ms_update += t; break;
        case KID_BA_COMM: res->ms_comm += t; break;
        default: res->ms_reduce += t; break;
      }
    }
  return SSX_OK;
}

extern "C" ssx_status ssx_ba_solve(ssx_ctx* ctx, const ssx_ba_problem* prob, const ssx_ba_options* opt_in, ssx_ba_result* res)
{
  return ba_solve_impl(ctx, prob, opt_in, res, nullptr);
}

// ---- batches of small windows ----------------------------------------------------------------------------------------------
// Many small windows together (one window per stereo pair of a batch, per stream of BASELINE configs[4], ...): every
// kernel of the small-window path runs ONCE for all windows (blockIdx.y = window), the device-driven LM loop of each
// window advances independently, one upload and one download carry all windows.  Same arithmetic as n calls of
// ssx_ba_solve -- identical bits per window.

struct ssx_ba_batch {
  ssx_ctx* ctx = nullptr;
  int device = 0;                                    // the ctx's device (ssx_ba_batch_destroy must not read it through ctx)
  int n = 0;
  ssx_ba_options opt;
  DevBuf arena_own; HostBuf stage_own, scal_own;     // a resident batch owns its memory; the one-call path borrows the ctx workspace
  DevBuf* arena = nullptr; HostBuf* stage = nullptr; HostBuf* scal = nullptr;
  std::vector<BaDev> devs;
  std::vector<std::vector<int>> perm;                // sorted edge -> caller's edge, per window
  std::vector<int> P, L, E, E_raw;
  std::vector<WinExt*> exts;                         // windows of ssx_ba_window objects (one-shot batches only), else empty
  const ssx_ba_problem* probs = nullptr;             // (valid during a one-shot call: the dead entries of a window's storage)
  std::vector<size_t> out_off;
  size_t out_total = 0, a_out = 0, a_gather = 0, a_head = 0, in_total = 0, o_dv = 0, o_ctrl = 0, o_ooff = 0;
  int max_ch = 1, max_rl = 1, max_rs = 1, total_ch = 0, min_ch = 0;
  bool any_solve64 = false, any_solve80 = false, any_solve = false, with_err = false, fresh = false;
  int threads = 1;
  int groups = 0;                                    // ssx_ba_batch_set_groups; 0: batch_groups(n)
};

namespace {

// Groups of windows a batch is run in, each on its own stream (batch_run).  Two: measured 2.61 / 2.45 / 2.39 / 3.01 ms for
// 64 windows in 1 / 2 / 3 / 4 groups in a process with nothing else on the GPU, but 2.61 / 2.45 / 3.24 ms next to a
// front-end on its own two streams (more streams than hardware queues: the groups then wait for each other).
int batch_groups(int n)
{
  static const int groups_env = getenv("SSX_BA_GROUPS") ? atoi(getenv("SSX_BA_GROUPS")) : 2;
  return n >= 8 ? std::min(std::max(groups_env, 1), 4) : 1;
}

// marshal + upload n small windows; SSX_ERR_UNSUPPORTED when one of them is a large window (> 16 free keyframes)
ssx_status batch_build(ssx_ctx* ctx, int n, const ssx_ba_problem* probs, const ssx_ba_options& opt, bool with_err, bool own, ssx_ba_batch* B,
                       WinExt* const* exts = nullptr)
{
  if (!ctx->ba) { ctx->ba = new BaWorkspace(); ctx->ba_free = ssx_ba_workspace_free; }
  BaWorkspace* ws = ctx->ba;
  // (the marshalling scratch of the windows is kept with the ctx between calls; after a batch larger than PREPS_KEEP
  // windows it is trimmed back, see the end of this function)
  if ((int)ws->preps.size() < n) ws->preps.resize(n);
  std::vector<HostPrep>& preps = ws->preps;
  const int hw = (int)std::thread::hardware_concurrency();
  const int T = std::max(1, std::min({n, host_threads_cap(), hw > 1 ? hw / 2 : 1}));
  B->ctx = ctx; B->device = ctx->device; B->n = n; B->opt = opt; B->threads = T; B->with_err = with_err;
  if (!own) B->groups = ctx->ba_batch_groups;                       // (a resident batch has its own setting: ssx_ba_batch_set_groups)
  static const int timing_mode = getenv("SSX_BATCH_TIMING") ? std::max(atoi(getenv("SSX_BATCH_TIMING")), 1) : 0;   // phase times on stderr
  const bool timing = timing_mode == 1;                              // 1: with synchronisations (tools/batch_time.py), 2: host clocks only
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms_since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(now() - t).count(); };
  const auto t_begin = now();
  // ---- 1. host marshalling of every window (edge sort, chunks, index lists), T threads
  std::vector<ssx_status> sts(n, SSX_OK);
  ws->pool.run(n, T, [&](int w) { sts[w] = prepare(ctx, &probs[w], preps[w], true, exts ? exts[w] : nullptr); });
  for (int w = 0; w < n; ++w) if (sts[w] != SSX_OK) return sts[w];
  for (int w = 0; w < n; ++w) if (preps[w].big || (exts && !preps[w].dev_prep)) return SSX_ERR_UNSUPPORTED;
  const double t_prepare = ms_since(t_begin);
  B->probs = probs;
  if (exts) B->exts.assign(exts, exts + n); else B->exts.clear();
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  B->arena = own ? &B->arena_own : &ws->arena;
  B->stage = own ? &B->stage_own : &ws->stage;
  B->scal = own ? &B->scal_own : &ws->scal;
  // ---- 2. sizes, one arena: [blobs of all windows | BaDev[n] | ctrl int[3n] | out offsets | scratch of all windows | packed outputs | gather]
  std::vector<UploadPlace> place(n);
  B->devs.assign(n, BaDev{});
  BandPlan no_band;
  size_t in_total = 0, rest_total = 0, out_total = 0;
  std::vector<size_t> in_off(n), rest_off(n);
  B->out_off.assign(n, 0); B->P.resize(n); B->L.resize(n); B->E.resize(n); B->E_raw.resize(n); B->perm.resize(n);
  for (int w = 0; w < n; ++w) {
    BigDev bd; BandDev bnd;
    place[w].dry = true;
    place[w].keep_init = own;
    ssx_status st = upload(ctx, &probs[w], preps[w], opt.huber_delta, opt.chi2_th, 1, 0, B->devs[w], bd, no_band, bnd, &place[w], exts ? exts[w] : nullptr);
    if (st != SSX_OK) return st;
    in_off[w] = in_total; in_total += place[w].in_bytes;
    rest_off[w] = rest_total; rest_total += place[w].rest_bytes;
    B->out_off[w] = out_total;
    B->P[w] = preps[w].P; B->L[w] = preps[w].L; B->E[w] = preps[w].E; B->E_raw[w] = preps[w].E_raw;
    out_total += 7 * (size_t)preps[w].P + 3 * (size_t)preps[w].L + (with_err ? std::max(2 * (size_t)preps[w].E, (size_t)preps[w].E_raw) : 0);
  }
  Layout tail;
  B->o_dv = tail.take(sizeof(BaDev) * n); B->o_ctrl = tail.take(sizeof(int) * 3 * n); B->o_ooff = tail.take(sizeof(size_t) * n);
  const size_t head_bytes = in_total + tail.off;                     // everything that is uploaded
  Layout arena;
  B->a_head = arena.take(head_bytes);
  const size_t a_rest = arena.take(rest_total);
  B->a_out = arena.take(sizeof(double) * (out_total + 1));
  B->a_gather = arena.take(sizeof(double) * (size_t)n * (3 * SSX_BA_MAX_STATS));
  B->in_total = in_total; B->out_total = out_total;
  // (resident windows: their storage grows with every keyframe until it is rewritten at twice the live size, and a grown arena
  // is a hipFree -- a device-wide synchronisation, 5-20 ms in the middle of a step -- so a reallocation asks for 2.5x the need)
  const double grow = exts ? 2.5 : 1.25;
  SSX_HIP_TRY(ctx, B->arena->reserve(arena.off, grow));
  SSX_HIP_TRY(ctx, B->stage->reserve(std::max(head_bytes, sizeof(double) * (out_total + 1)), grow));
  SSX_HIP_TRY(ctx, B->scal->reserve(sizeof(double) * (size_t)n * (SC_N + 3 * SSX_BA_MAX_STATS) + sizeof(int) * 3 * n + 64));
  char* dev_base = B->arena->as<char>();
  char* hst = B->stage->as<char>();
  // ---- 3. fill the pinned mirror (T threads) and upload it, in Q pieces: the copy engine moves one piece while the threads fill
  // the next (128 C3 windows: 0.7 ms of filling, 1.65 ms on PCIe for 86 MB)
  static const int pieces_env = getenv("SSX_BA_UPLOAD_PIECES") ? std::min(std::max(atoi(getenv("SSX_BA_UPLOAD_PIECES")), 1), 16) : 4;
  const int Q = n >= 32 && !exts ? pieces_env : 1;                   // (resident windows send a few KB each: one piece)
  for (int q = 0; q < Q; ++q) {
  const int q0 = (int)((long long)n * q / Q), q1 = (int)((long long)n * (q + 1) / Q);
  ws->pool.run(q1 - q0, T, [&](int wi) {
    const int w = q0 + wi;
    BigDev bd; BandDev bnd;
    place[w].dry = false;
    place[w].in_dev = dev_base + B->a_head + in_off[w];
    place[w].rest_dev = dev_base + a_rest + rest_off[w];
    place[w].in_host = hst + in_off[w];
    sts[w] = upload(ctx, &probs[w], preps[w], opt.huber_delta, opt.chi2_th, 1, 0, B->devs[w], bd, no_band, bnd, &place[w], exts ? exts[w] : nullptr);
    B->devs[w].store_w = opt.jac_mode == SSX_JAC_NUMERIC_G2O ? 1 : 0;
    B->devs[w].no_err = with_err ? 0 : 1;
    if (with_err) B->perm[w] = preps[w].perm;
  });
  for (int w = q0; w < q1; ++w) if (sts[w] != SSX_OK) { (void)hipStreamSynchronize(ctx->stream); return sts[w]; }
  if (q + 1 < Q) {
    const size_t b0 = in_off[q0], b1 = in_off[q1];
    if (b1 > b0) SSX_HIP_TRY(ctx, hipMemcpyAsync(dev_base + B->a_head + b0, hst + b0, b1 - b0, hipMemcpyHostToDevice, ctx->stream));
  }
  }
  const size_t up0 = Q > 1 ? in_off[(int)((long long)n * (Q - 1) / Q)] : 0;   // the last piece goes with the tail
  memcpy(hst + in_total + B->o_dv, B->devs.data(), sizeof(BaDev) * n);
  memset(hst + in_total + B->o_ctrl, 0, sizeof(int) * 3 * n);
  memcpy(hst + in_total + B->o_ooff, B->out_off.data(), sizeof(size_t) * n);
  for (int w = 0; w < n; ++w) {
    const BaDev& d = B->devs[w];
    B->max_ch = std::max(B->max_ch, d.nCh);
    B->min_ch = w == 0 ? d.nCh : std::min(B->min_ch, d.nCh);
    B->total_ch += d.nCh;
    B->max_rl = std::max(B->max_rl, (d.nP * 27 + 63) / 64);
    B->max_rs = std::max(B->max_rs, (d.nBlk * 36 + d.nP * 6 + 63) / 64);
    if (6 * d.nP <= NB) B->any_solve64 = true; else if (6 * d.nP <= 80) B->any_solve80 = true; else B->any_solve = true;
  }
  const double t_fill = ms_since(t_begin);
  SSX_HIP_TRY(ctx, hipMemcpyAsync(dev_base + B->a_head + up0, hst + up0, head_bytes - up0, hipMemcpyHostToDevice, ctx->stream));
  double t_up = 0.0;
  if (timing) { (void)hipStreamSynchronize(ctx->stream); t_up = ms_since(t_begin); }
  {
    // pair lists + work items of every window, on the device (windows marshalled with SSX_BA_HOST_LISTS brought theirs along)
    const BaDev* dvb = reinterpret_cast<const BaDev*>(dev_base + B->a_head + in_total + B->o_dv);
    if (!exts) hipLaunchKernelGGL(k_dup_state_b, dim3(16, n), dim3(CH), 0, ctx->stream, dvb);   // (windows keep both buffers themselves)
    int max_e = 1;
    bool any_prep = false;
    for (int w = 0; w < n; ++w) { max_e = std::max(max_e, B->devs[w].E_raw); any_prep = any_prep || B->devs[w].dev_prep; }
    if (any_prep) hipLaunchKernelGGL(k_prep_scatter_b, dim3((max_e + CH - 1) / CH, n), dim3(CH), 0, ctx->stream, dvb);
    hipLaunchKernelGGL(k_prep_chunk_b, dim3(B->max_ch, n), dim3(CH), 0, ctx->stream, dvb);
    SSX_HIP_TRY(ctx, hipGetLastError());
  }
  if (timing_mode == 2)
    fprintf(stderr, "[batch_build n=%d, no syncs] prepare %.3f | sizes + fill %.3f | enqueue of upload + marshalling kernels %.3f ms\n", n, t_prepare,
            t_fill - t_prepare, ms_since(t_begin) - t_fill);
  if (timing) {
    (void)hipStreamSynchronize(ctx->stream);
    fprintf(stderr, "[batch_build n=%d] prepare %.3f | sizes + fill (+ upload of 3 pieces of 4) %.3f | %.1f MB on the device %.3f later | device marshalling %.3f ms\n", n, t_prepare,
            t_fill - t_prepare, head_bytes / 1e6, t_up - t_fill, ms_since(t_begin) - t_up);
  }
  B->fresh = true;                                                   // the state buffers hold the uploaded state
  const size_t lds_schur = schur_lds_bytes();
  static bool attr_set_b = false;
  if (!attr_set_b) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_schur_b), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_schur);
    const int lf = (int)std::max(lds_schur, LIN_LDS_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_lin_schur_b<SSX_JAC_ANALYTIC>), hipFuncAttributeMaxDynamicSharedMemorySize, lf);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_lin_schur_b<SSX_JAC_NUMERIC_G2O>), hipFuncAttributeMaxDynamicSharedMemorySize, lf);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_linearize_b<SSX_JAC_ANALYTIC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LIN_LDS_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_linearize_b<SSX_JAC_NUMERIC_G2O>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LIN_LDS_BYTES);
    attr_set_b = true;
  }
  // the marshalling scratch stays allocated between calls up to 64 MB (device-marshalled windows keep ~6 bytes per observation:
  // 64 C3 windows = 8 MB; host-marshalled ones ~100 bytes: the cache is trimmed back to 16 windows after such a batch)
  size_t prep_bytes = 0;
  for (const HostPrep& hp : ws->preps)
    prep_bytes += hp.slot8.capacity() + sizeof(int) * (hp.cnt_tmp.capacity() + hp.start_tmp.capacity() + hp.lm_compact.capacity() + hp.e_rec.capacity() +
                                                       hp.perm.capacity() + hp.e_pose.capacity() + hp.e_lmc.capacity() + hp.bseg.capacity()) +
                  sizeof(double) * hp.e_uv.capacity() + hp.pair_a.capacity() + hp.pair_b.capacity();
  constexpr size_t PREPS_KEEP = 16;
  if (ws->preps.size() > PREPS_KEEP && prep_bytes > (size_t(64) << 20)) { ws->preps.resize(PREPS_KEEP); ws->preps.shrink_to_fit(); }
  return SSX_OK;
}

// optimise every window of a built batch; results may be null (nothing is downloaded then, counters only in `summary`)
ssx_status batch_run(ssx_ba_batch* B, ssx_ba_result* results, int32_t* lm_iterations_total)
{
  ssx_ctx* ctx = B->ctx;
  const int n = B->n;
  const ssx_ba_options& opt = B->opt;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  SSX_HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  char* dev_base = B->arena->as<char>();
  const BaDev* dv = reinterpret_cast<const BaDev*>(dev_base + B->a_head + B->in_total + B->o_dv);
  const size_t* d_ooff = reinterpret_cast<const size_t*>(dev_base + B->a_head + B->in_total + B->o_ooff);
  hipStream_t s = ctx->stream;
  const int wg_x = B->max_ch;                                        // workgroups per window of the linearise / Schur kernels
  if (!B->fresh) hipLaunchKernelGGL(k_reset_state_b, dim3(16, n), dim3(CH), 0, s, dv);
  B->fresh = false;
  // per-window host state of Backend::OptimizeActiveMap's outer loop (backend.cpp:175-203)
  struct WinState { int cur = 0, round = 0, rounds = 0, n_iters = 0, n_in = 0, n_outl = 0; bool done = false, trial_err = false; double n_out = 0; };
  std::vector<WinState> wsn(n);
  // nobody asked for landmarks or per-edge errors: only the poses cross PCIe (560 B instead of 97 KB per C3 window), and they are
  // requested speculatively at the end of every outer round (below)
  bool spec_poses = results != nullptr && !B->with_err;
  int spec_maxP = 0;
  if (results) for (int w = 0; w < n; ++w) { spec_poses = spec_poses && !results[w].points_out; spec_maxP = std::max(spec_maxP, B->P[w]); }
  spec_poses = spec_poses && (size_t)n * 7 * spec_maxP <= B->out_total;
  bool spec_done = false;                                            // a speculative poses download was really enqueued (no LM round may run at all)
  double* hscal = B->scal->as<double>();                             // n x SC_N, then n x 3 x MAX_STATS, then the ctrl words
  int* h_ctrl = reinterpret_cast<int*>(hscal + (size_t)n * (SC_N + 3 * SSX_BA_MAX_STATS));
  for (int w = 0; w < n; ++w) wsn[w].done = !(B->devs[w].nCh > 0) || opt.outer_rounds <= 0;
  if (!B->exts.empty()) for (int w = 0; w < n; ++w) wsn[w].cur = B->exts[w]->cur;   // windows: the buffer that holds their estimate
  const size_t lds_schur = schur_lds_bytes();
  const size_t lds_fused = std::max(lds_schur, LIN_LDS_BYTES);
  int G = std::min(B->groups > 0 ? std::min(B->groups, 4) : batch_groups(n), std::max(n, 1));   // never an empty group (gridDim.y == 0)
  for (int g = 0; g + 1 < G; ++g) {
    if (!ctx->grp[g] && ctx->make_stream(&ctx->grp[g], false) != hipSuccess) { (void)hipGetLastError(); G = g + 1; break; }
    if (!ctx->grp_ev[g] && hipEventCreateWithFlags(&ctx->grp_ev[g], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); G = g + 1; break; }
  }
  const bool split = G > 1;
  const bool turns_on = g_turns.enabled() && ctx->ba != nullptr;
  if (turns_on && !ctx->ba->ev_turn && hipEventCreateWithFlags(&ctx->ba->ev_turn, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); ctx->ba->ev_turn = nullptr; }
  auto all_done = [&] { for (int w = 0; w < n; ++w) if (!wsn[w].done) return false; return true; };
  while (!all_done() && opt.iters > 0) {
    for (int w = 0; w < n; ++w) { h_ctrl[w] = wsn[w].cur; h_ctrl[n + w] = wsn[w].n_iters; h_ctrl[2 * n + w] = wsn[w].done ? 1 : 0; }
    // (no copies: the control words are READ by the kernel from the pinned block, the state words and results are WRITTEN by the
    // gather / pack kernels into pinned host memory -- a hipMemcpyAsync of this runtime runs as a blit KERNEL on the compute units
    // whenever the SDMA engines are taken, tools/microbench/copy_engine.hip, and costs the host ~10 us each)
    hipLaunchKernelGGL(k_lm_begin_batch, dim3(n), dim3(64), 0, s, dv, (const int*)h_ctrl, n, opt.iters);
    int slots_total = 0;
    bool first_slot = true;
    for (;;) {
      // ssx_ba_device_turns: this round's kernels run after the round enqueued before it, whichever context enqueued that
      struct TurnScope {
        bool on; BaWorkspace* w; int dev; hipStream_t st;
        TurnScope(bool o, BaWorkspace* w_, int d, hipStream_t s_) : on(o), w(w_), dev(d), st(s_) { if (on) g_turns.begin(w, dev, st); }
        void close() { if (on) { g_turns.end(w, dev, w->ev_turn, st); on = false; } }
        ~TurnScope() { close(); }
      } turn(turns_on, ctx->ba, ctx->device, s);
      int slots = opt.iters;
      if (slots_total > 0) {
        slots = 1;
        for (int w = 0; w < n; ++w)
          if (!wsn[w].done && hscal[(size_t)w * SC_N + SC_STOP] == 0.0) slots = std::max(slots, opt.iters - (int)hscal[(size_t)w * SC_N + SC_IT]);
      }
      // The batch in G groups of windows on G streams: the narrow kernels of one half (one workgroup per window: the reduced
      // solve, the reductions -- a third of an iteration's time on a quarter of the chip) run beside the wide kernels
      // of the other.  The windows are independent; the halves meet again before the state words are gathered.
      if (split) {
        SSX_HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, s));
        for (int g = 0; g + 1 < G; ++g) SSX_HIP_TRY(ctx, hipStreamWaitEvent(ctx->grp[g], ctx->ev_fork, 0));
      }
      for (int sidx = 0; sidx < slots; ++sidx) {
        const bool fused = !first_slot;                                // see ssx_ba_solve: lambda is known after the first slot
        for (int g = 0; g < G; ++g) {
          hipStream_t hs = g ? ctx->grp[g - 1] : s;
          const int w0 = (int)((long long)n * g / G), hn = (int)((long long)n * (g + 1) / G) - w0;
          const BaDev* hv = dv + w0;
          const dim3 gCh(B->max_ch, hn), gWg(wg_x, hn), gRl(B->max_rl, hn), gRs(B->max_rs, hn), gOne(1, hn);
          const bool fin_b = B->min_ch > 0 && g_trial_finish.load() != 0;   // the last chunk of k_backsub_residual finishes the trial
          if (fused) {
            if (opt.jac_mode == SSX_JAC_NUMERIC_G2O) SSX_PROF_ON(ctx, hs, KID_BA_LIN_SCHUR, hipLaunchKernelGGL(k_lin_schur_b<SSX_JAC_NUMERIC_G2O>, gWg, dim3(CH), lds_fused, hs, hv));
            else SSX_PROF_ON(ctx, hs, KID_BA_LIN_SCHUR, hipLaunchKernelGGL(k_lin_schur_b<SSX_JAC_ANALYTIC>, gWg, dim3(CH), lds_fused, hs, hv));
          } else {
            if (opt.jac_mode == SSX_JAC_NUMERIC_G2O) SSX_PROF_ON(ctx, hs, KID_BA_LINEARIZE, hipLaunchKernelGGL(k_linearize_b<SSX_JAC_NUMERIC_G2O>, gWg, dim3(CH), LIN_LDS_BYTES, hs, hv, -1));
            else SSX_PROF_ON(ctx, hs, KID_BA_LINEARIZE, hipLaunchKernelGGL(k_linearize_b<SSX_JAC_ANALYTIC>, gWg, dim3(CH), LIN_LDS_BYTES, hs, hv, -1));
          }
          static const bool no_both_env = getenv("SSX_BA_SPLIT_REDUCE") != nullptr;   // (tools: the two launches, for A/B timing)
          const bool both = fused && !first_slot && !no_both_env;    // (the first slot needs lambda between the two reductions)
          if (both) SSX_PROF_ON(ctx, hs, KID_BA_REDUCE_SCHUR, hipLaunchKernelGGL(k_reduce_both_b, dim3(B->max_rl + B->max_rs, hn), dim3(CH), 0, hs, hv, B->max_rl));
          else SSX_PROF_ON(ctx, hs, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_reduce_lin_b, gRl, dim3(CH), 0, hs, hv));
          if (first_slot) SSX_PROF_ON(ctx, hs, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_lambda_init_b, gOne, dim3(64), 0, hs, hv, 1));
          if (!fused) SSX_PROF_ON(ctx, hs, KID_BA_SCHUR, hipLaunchKernelGGL(k_schur_b, gWg, dim3(CH), lds_schur, hs, hv));
          if (!both) SSX_PROF_ON(ctx, hs, KID_BA_REDUCE_SCHUR, hipLaunchKernelGGL(k_reduce_schur_b, gRs, dim3(CH), 0, hs, hv));
          if (B->any_solve64) SSX_PROF_ON(ctx, hs, KID_BA_SOLVE, hipLaunchKernelGGL(k_solve64_b, gOne, dim3(CH), 0, hs, hv));
          if (B->any_solve80) SSX_PROF_ON(ctx, hs, KID_BA_SOLVE, hipLaunchKernelGGL(k_solve80_b, gOne, dim3(CH), 0, hs, hv));
          if (B->any_solve) SSX_PROF_ON(ctx, hs, KID_BA_SOLVE, hipLaunchKernelGGL(k_solve_b, gOne, dim3(CH), 0, hs, hv));
          SSX_PROF_ON(ctx, hs, KID_BA_BACKSUB, hipLaunchKernelGGL(k_backsub_residual_b, gCh, dim3(CH), 0, hs, hv, fin_b ? 1 : 0));
          if (!fin_b) SSX_PROF_ON(ctx, hs, KID_BA_REDUCE_TRIAL, hipLaunchKernelGGL(k_reduce_trial_b, gOne, dim3(CH), 0, hs, hv, 1));   // (a window without chunks: nobody would finish its trial)
        }
        first_slot = false;
      }
      for (int g = 0; g + 1 < G; ++g) {
        SSX_HIP_TRY(ctx, hipEventRecord(ctx->grp_ev[g], ctx->grp[g]));
        SSX_HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->grp_ev[g], 0));
      }
      slots_total += slots;
      SSX_HIP_TRY(ctx, hipGetLastError());
      hipLaunchKernelGGL(k_gather_scal_b, dim3(n), dim3(CH), 0, s, dv, n, hscal, 0);
      if (spec_poses) {
        // poses-only results ride behind the control words of this round, before the host has looked at them: if the round turns
        // out to be the last one (the usual case) the solve ends on ONE synchronisation instead of two; otherwise the next round
        // overwrites them.  The packing kernel takes the state buffer index from the window's own control block.
        hipLaunchKernelGGL(k_gather_scal_b, dim3(n), dim3(CH), 0, s, dv, n, hscal + (size_t)n * SC_N, 1);
        hipLaunchKernelGGL(k_pack_poses_b, dim3(n), dim3(CH), 0, s, dv, (const int*)nullptr, n, spec_maxP, B->stage->as<double>());
        SSX_HIP_TRY(ctx, hipEventRecord(ctx->ev1, s));
        spec_done = true;
      }
      turn.close();
      SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
      bool stopped = true;
      for (int w = 0; w < n; ++w) if (!wsn[w].done && hscal[(size_t)w * SC_N + SC_STOP] == 0.0) stopped = false;
      if (stopped) break;
    }
    for (int w = 0; w < n; ++w) {
      WinState& st = wsn[w];
      if (st.done) continue;
      const double* sc = hscal + (size_t)w * SC_N;
      st.cur = (int)sc[SC_CUR];
      st.n_out = sc[SC_NOUT];
      if (sc[SC_TRIALS_RUN] > 0.0) st.trial_err = true;
      st.n_iters = std::max(st.n_iters, (int)sc[SC_NSTAT]);
      st.rounds++;
      const double n_edges = (double)B->devs[w].E, cnt_in = n_edges - st.n_out;
      st.n_outl = (int)st.n_out; st.n_in = (int)cnt_in;
      const double ratio = n_edges > 0 ? cnt_in / (cnt_in + st.n_out) : 1.0;
      if (ratio > opt.inlier_ratio) st.done = true;
      if (++st.round >= opt.outer_rounds) st.done = true;
    }
  }
  if (lm_iterations_total) { int t = 0; for (int w = 0; w < n; ++w) t += wsn[w].n_iters; *lm_iterations_total = t; }
  if (!B->exts.empty()) for (int w = 0; w < n; ++w) B->exts[w]->cur = wsn[w].cur;   // ... and the one that holds the result
  if (!results) {                                                    // nothing to download: the caller only wants the work done
    SSX_HIP_TRY(ctx, hipEventRecord(ctx->ev1, s));
    SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
    return SSX_OK;
  }
  // ---- statistics + results: one packing kernel, one download
  const bool want_err = B->with_err;
  // (iters <= 0, outer_rounds <= 0 or windows without a single chunk: no round ran, nothing was staged -- the ordinary
  // gather / pack / download returns the input state)
  const bool poses_only = spec_poses && spec_done;
  const int maxP = spec_maxP;
  double* h_out = B->stage->as<double>();
  if (!poses_only) {
  for (int w = 0; w < n; ++w) { h_ctrl[w] = wsn[w].cur; h_ctrl[n + w] = wsn[w].trial_err ? 1 : 0; h_ctrl[2 * n + w] = 1; }
  hipLaunchKernelGGL(k_gather_scal_b, dim3(n), dim3(CH), 0, s, dv, n, hscal + (size_t)n * SC_N, 1);
  if (want_err)                                                       // windows that never ran a trial: errors of the input state
    for (int w = 0; w < n; ++w)
      if (!wsn[w].trial_err && B->devs[w].nCh > 0)
        hipLaunchKernelGGL(k_linearize<SSX_JAC_ANALYTIC>, dim3(B->devs[w].nCh), dim3(CH), LIN_LDS_BYTES, s, B->devs[w], wsn[w].cur);
  if (want_err) {
    // (per-edge chi2 goes back in the CALLER's order: a scatter of 8-byte words, which belongs in HBM -- over PCIe every one of them
    // would be a transaction of its own; a streaming kernel then moves the packed block)
    double* d_out = reinterpret_cast<double*>(dev_base + B->a_out);
    hipLaunchKernelGGL(k_pack_out_b, dim3(64, n), dim3(CH), 0, s, dv, (const int*)h_ctrl, n, d_ooff, d_out, 1);
    hipLaunchKernelGGL(k_stream_out, dim3((unsigned)std::min<size_t>(1024, (B->out_total + 2 * CH - 1) / (2 * CH))), dim3(CH), 0, s, (const double*)d_out, h_out, B->out_total);
  } else {
    hipLaunchKernelGGL(k_pack_out_b, dim3(64, n), dim3(CH), 0, s, dv, (const int*)h_ctrl, n, d_ooff, h_out, 0);
  }
  SSX_HIP_TRY(ctx, hipEventRecord(ctx->ev1, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  }   // (!poses_only)
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  static const bool timing = getenv("SSX_BATCH_TIMING") != nullptr;
  const auto t_unpack = std::chrono::steady_clock::now();
  // (poses only: 560 bytes per window -- waking the worker threads costs more than copying them here)
  ctx->ba->pool.run(n, poses_only ? 1 : B->threads, [&](int w) {
    ssx_ba_result& r = results[w];
    const WinState& st = wsn[w];
    const int P = B->P[w], L = B->L[w], E = B->E[w];
    r.rounds = st.rounds; r.n_iters = st.n_iters; r.n_inliers = st.n_in; r.n_outliers = st.n_outl;
    r.ms_linearize = r.ms_schur = r.ms_linear_solution = r.ms_update = r.ms_reduce = r.ms_comm = 0.f;
    const double* o = poses_only ? h_out + (size_t)w * 7 * maxP : h_out + B->out_off[w];
    if (r.poses_out) memcpy(r.poses_out, o, sizeof(double) * 7 * P);
    if (r.points_out && L) memcpy(r.points_out, o + 7 * (size_t)P, sizeof(double) * 3 * L);
    if (want_err && (r.edge_chi2 || r.edge_outlier) && B->devs[w].dev_prep) {
      const double* c2 = o + 7 * (size_t)P + 3 * (size_t)L;          // already in the caller's order
      const int* ept = (!B->exts.empty() && B->probs) ? B->probs[w].edge_point : nullptr;
      for (int eo = 0; eo < B->E_raw[w]; ++eo) {
        if (ept && ept[eo] < 0) continue;                            // a dead entry of a window's storage
        if (r.edge_chi2) r.edge_chi2[eo] = c2[eo];
        if (r.edge_outlier) r.edge_outlier[eo] = c2[eo] > opt.chi2_th;
      }
    } else if (want_err && (r.edge_chi2 || r.edge_outlier)) {
      const double* e = o + 7 * (size_t)P + 3 * (size_t)L;
      const std::vector<int>& perm = B->perm[w];
      for (int sidx = 0; sidx < E; ++sidx) {
        const int eo = perm[sidx];
        const double c2 = e[sidx] * e[sidx] + e[(size_t)E + sidx] * e[(size_t)E + sidx];
        if (r.edge_chi2) r.edge_chi2[eo] = c2;
        if (r.edge_outlier) r.edge_outlier[eo] = c2 > opt.chi2_th;
      }
    }
    const double* hstat = hscal + (size_t)n * SC_N + (size_t)w * 3 * SSX_BA_MAX_STATS;
    for (int k = 0; k < r.n_iters && k < SSX_BA_MAX_STATS; ++k) {
      r.iter_chi2[k] = hstat[k];
      r.iter_lambda[k] = hstat[SSX_BA_MAX_STATS + k];
      r.iter_trials[k] = (int)hstat[2 * SSX_BA_MAX_STATS + k];
    }
    r.ms_total = ms;
    r.ms_setup = 0.f;
  });
  if (timing)
    fprintf(stderr, "[batch_run n=%d] solve + download of %.1f MB %.3f (GPU clock) | unpack %.3f ms\n", n, sizeof(double) * B->out_total / 1e6, ms,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_unpack).count());
  return SSX_OK;
}

}  // namespace

extern "C" {

#ifndef SSX_NO_TEST_HOOKS   // include/ssx_test_hooks.h: hooks of this repository's tests / tools, not part of the product ABI
// tools hook (no GPU needed): dynamic LDS bytes a kernel of this file is launched with (the compiler's resource report only
// knows static __shared__ arrays, and rocprofv3's dispatch rows show 0 for these); -1 = depends on the problem / unknown
// tests hook: 1 = the per-chunk slabs of the linearise / Schur kernels are written and read in full (round 3), 0 = only the blocks and
// poses a chunk touches (default), < 0 = the environment's choice (SSX_BA_DENSE_SLABS).  Same bits either way.  Applies to problems
// uploaded after the call.
void ssx_debug_set_dense_slabs(int32_t mode) { g_dense_slabs.store(mode < 0 ? -1 : (mode ? 1 : 0)); }
// tests hook: 0 = a trial's sums are added and its LM step is taken by a launch of k_reduce_trial, 1 (default) = by the last chunk of
// k_backsub_residual (the ticket protocol).  Same bits either way (test_trial_finish_litmus).
void ssx_debug_set_trial_finish(int32_t mode) { g_trial_finish.store(mode ? 1 : 0); }

int64_t ssx_debug_kernel_dynamic_lds(const char* kernel)
{
  if (!kernel) return -1;
  const std::string k(kernel);
  auto starts = [&](const char* p) { return k.rfind(p, 0) == 0; };
  if (starts("k_lin_schur") || starts("k_linearize") || k == "k_schur" || k == "k_schur_b") return (int64_t)BA_LDS_BYTES;
  if (k == "k_schur_prep") return (int64_t)(sizeof(double) * (18 + 9 + 3) * PW + 64);
  if (starts("k_band_")) return -1;
  return 0;
}

// tools hook (no GPU needed): seconds of host marshalling (edge sort, chunks, index lists) of one problem
double ssx_ba_debug_prepare_seconds(const ssx_ba_problem* prob, int32_t reps)
{
  if (!prob || reps < 1) return -1.0;
  ssx_ctx dummy;
  static BaWorkspace* wsl = new BaWorkspace();            // (its worker pool: large windows count their observations on several threads)
  dummy.ba = wsl;
  static thread_local HostPrep h;
  double best = -1.0;
  for (int i = 0; i < reps; ++i) {
    const auto t0 = std::chrono::steady_clock::now();
    if (prepare(&dummy, prob, h) != SSX_OK) { best = -1.0; break; }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (best < 0 || dt < best) best = dt;
  }
  dummy.ba = nullptr;
  return best;
}

// test hook (no GPU needed): FNV-1a digest of what prepare() hands on for a large window (per-landmark offsets, the rank of
// every observation inside its landmark, per-pose counts, chunk cuts), counted on `threads` host threads
uint64_t ssx_ba_debug_prepare_digest(const ssx_ba_problem* prob, int32_t threads)
{
  if (!prob) return 0;
  ssx_ctx dummy;
  static BaWorkspace* wsl = new BaWorkspace();
  dummy.ba = wsl;
  static thread_local HostPrep h;
  g_prep_threads_override = threads;
  const ssx_status st = prepare(&dummy, prob, h);
  g_prep_threads_override = 0;
  dummy.ba = nullptr;
  if (st != SSX_OK) return 0;
  uint64_t d = 1469598103934665603ull;
  auto eat = [&](const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; for (size_t i = 0; i < n; ++i) { d ^= b[i]; d *= 1099511628211ull; } };
  eat(h.lm_ptr.data(), sizeof(int) * h.lm_ptr.size()); eat(h.lm_id.data(), sizeof(int) * h.lm_id.size());
  eat(h.slot8.data(), (size_t)h.E_raw); eat(h.pe_ptr.data(), sizeof(int) * h.pe_ptr.size()); eat(h.ch_lm.data(), sizeof(int) * h.ch_lm.size());
  return d;
}

int32_t ssx_ba_debug_upload_format(const ssx_ba_problem* prob)
{
  if (!prob) return -1;
  ssx_ctx dummy;
  static thread_local HostPrep h;
  if (prepare(&dummy, prob, h) != SSX_OK) return -1;
  return h.raw_fmt;
}
#endif  // SSX_NO_TEST_HOOKS

ssx_status ssx_ba_solve_batch(ssx_ctx* ctx, int32_t n, const ssx_ba_problem* probs, const ssx_ba_options* opt_in, ssx_ba_result* results)
{
  if (!ctx || n < 0 || (n > 0 && (!probs || !results))) return SSX_ERR_INVALID_ARG;
  if (n == 0) return SSX_OK;
  ssx_ba_options opt;
  if (opt_in) opt = *opt_in; else ssx_ba_default_options(&opt);
  auto sequential = [&]() -> ssx_status {
    for (int w = 0; w < n; ++w) {
      const ssx_status st = ssx_ba_solve(ctx, &probs[w], &opt, &results[w]);
      if (st != SSX_OK) return st;
    }
    return SSX_OK;
  };
  if (opt.comm || opt.allreduce || n == 1) return sequential();
  bool with_err = false;
  for (int w = 0; w < n; ++w) if (results[w].edge_chi2 || results[w].edge_outlier) with_err = true;
  ssx_ba_batch B;
  ssx_status st = batch_build(ctx, n, probs, opt, with_err, false, &B);
  if (st == SSX_ERR_UNSUPPORTED) return sequential();                 // a large window in the batch
  if (st != SSX_OK) return st;
  return batch_run(&B, results, nullptr);
}

// A RESIDENT batch: the windows are marshalled and uploaded once and stay in HBM; every ssx_ba_batch_solve optimises
// them again from the uploaded state (bench.py times this with nothing crossing PCIe but the LM control words).
ssx_status ssx_ba_batch_create(ssx_ctx* ctx, int32_t n, const ssx_ba_problem* probs, const ssx_ba_options* opt_in, int32_t with_edge_errors,
                               ssx_ba_batch** out)
{
  if (!ctx || n <= 0 || !probs || !out) return SSX_ERR_INVALID_ARG;
  *out = nullptr;
  ssx_ba_options opt;
  if (opt_in) opt = *opt_in; else ssx_ba_default_options(&opt);
  if (opt.comm || opt.allreduce) { ctx->set_error("ssx_ba_batch_create: batches do not take a collective"); return SSX_ERR_UNSUPPORTED; }
  ssx_ba_batch* B = new ssx_ba_batch();
  const ssx_status st = batch_build(ctx, n, probs, opt, with_edge_errors != 0, true, B);
  if (st != SSX_OK) {
    if (st == SSX_ERR_UNSUPPORTED) ctx->set_error("ssx_ba_batch_create: a window has more than %d free keyframes (use ssx_ba_solve)", SSX_BA_SMALL_P);
    ssx_ba_batch_destroy(B);
    return st;
  }
  *out = B;
  return SSX_OK;
}

ssx_status ssx_ba_batch_solve(ssx_ba_batch* batch, ssx_ba_result* results, int32_t* lm_iterations_total)
{
  if (!batch) return SSX_ERR_INVALID_ARG;
  return batch_run(batch, results, lm_iterations_total);
}

void ssx_ba_device_turns(int32_t enable) { g_turns.enable(enable != 0); }

ssx_status ssx_ba_set_batch_groups(ssx_ctx* ctx, int32_t groups)
{
  if (!ctx || groups < 0 || groups > 4) return SSX_ERR_INVALID_ARG;
  ctx->ba_batch_groups = groups;
  return SSX_OK;
}

int32_t ssx_ba_batch_size(const ssx_ba_batch* batch) { return batch ? batch->n : 0; }

int32_t ssx_ba_batch_groups(const ssx_ba_batch* batch) { return !batch ? 0 : (batch->groups > 0 ? std::min(batch->groups, 4) : batch_groups(batch->n)); }

void ssx_ba_batch_set_groups(ssx_ba_batch* batch, int32_t groups) { if (batch) batch->groups = groups > 0 ? groups : 0; }

void ssx_ba_batch_destroy(ssx_ba_batch* batch)
{
  if (!batch) return;
  (void)hipSetDevice(batch->device);
  batch->arena_own.release(); batch->stage_own.release(); batch->scal_own.release();
  delete batch;
}

}  // extern "C"

#include "ba_window.inc"
#include "pg.inc"
