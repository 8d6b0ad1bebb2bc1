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
struct HostPrep {                    // what prepare() of ba_marshal.inc fills in (here: BaWorkspace below keeps them by value)
  // counting results: written on every path of prepare() (band_w: by build_pairs), read by the plan of the arena
  int P, L, E, nP, nLm, nCh, nBlk;
  int E_raw = 0;                     // entries of the caller's edge arrays (E of them alive; see BaDev::E_raw)
  int raw_fmt = 0;                   // BaDev::raw_fmt of the blob this window is uploaded in
  bool big = false;                  // more than SSX_BA_SMALL_P free poses: the large-window path
  bool dev_lists = false;            // small window: pair lists + work items are built by k_build_lists, not here
  bool dev_prep = false;             // the edge sort by (landmark, pose), the packed records, the pose-major order and the sorted uv columns
                                     // are built ON THE DEVICE (k_prep_scatter / k_prep_chunk) from the caller's raw arrays; the host only counts
  int band_w = -1;                   // cyclic block bandwidth of this rank's part of the reduced system (max over its non-zero blocks)
  // the light tables: built on every path, all that a device-marshalled window uploads beside the caller's arrays
  std::vector<int> pose_free, lm_id, lm_ptr, ch_lm;
  std::vector<uint8_t> lm_fixed, slot8;   // slot8: rank of an edge among its landmark's edges in caller order (device-marshalled windows)
  std::vector<int> lm_compact;       // caller's landmark -> compact landmark or -1
  std::vector<int> pose_rank;        // empty, or BaDev::pose_rank (a window's keyframes in the order of their ids)
  std::vector<int> ch_desc;          // packed chunk records (4 ints each), see BaDev
  std::vector<int8_t> blk_pa, blk_pb;
  // the host reference's arrays (ref_* of ba_marshal.inc; the device builds them otherwise): sorted columns, packed records, per-chunk lists
  std::vector<int> e_pose, e_lmc, perm, pair_ptr;
  std::vector<uint8_t> e_cam, e_dup, pair_a, pair_b;
  std::vector<uint16_t> pptr;
  std::vector<double> e_uv;
  std::vector<int> e_rec, l_rec;     // packed records (4 ints each), see BaDev
  std::vector<int> lm_chunk;         // compact landmark -> chunk (large windows: the device-side pair builder)
  std::vector<int> bseg, bseg_ptr;   // see BaDev
  std::vector<unsigned int> touch;   // BaDev::touch
  // the large-window lists: pe_ptr by prepare() (pe_edge by the reference only), the block list by build_pairs
  std::vector<int> pe_ptr, pe_edge, sblk_pa, sblk_pb, spair_ptr;
  // scratch of prepare(), kept between calls (thr_*: per-thread landmark / pose counts of a large window counted on several threads)
  std::vector<int> thr_cnt, thr_pe, cnt_tmp, start_tmp, first_pf_tmp, visit_tmp, visit2_tmp;
  std::vector<uint32_t> tmp_pairs;
  std::vector<std::pair<int, int>> tmp_order;
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

// the context's BA workspace, created on first use
static BaWorkspace* ba_workspace(ssx_ctx* ctx) { if (!ctx->ba) { ctx->ba = new BaWorkspace(); ctx->ba_free = ssx_ba_workspace_free; } return ctx->ba; }

#define SSX_TRY(expr) do { const ssx_status _st = (expr); if (_st != SSX_OK) return _st; } while (0)   // a failed step ends the call
namespace {
#include "ba_marshal.inc"

// dynamic LDS of k_schur, of the fused k_lin_schur, of k_schur_prep
constexpr size_t SCHUR_LDS_BYTES = BA_LDS_BYTES, FUSED_LDS_BYTES = std::max(BA_LDS_BYTES, LIN_LDS_BYTES), SCHUR_PREP_LDS_BYTES = sizeof(double) * (18 + 9 + 3) * PW + 64;
// the analytic or the numeric (g2o's central differences) instantiation of a kernel template: LAUNCH_JAC(jac, k_x, grid, block, lds, stream, args...)
#define LAUNCH_JAC(jac, kernel, ...) \
  do { if ((jac) == SSX_JAC_NUMERIC_G2O) hipLaunchKernelGGL(kernel<SSX_JAC_NUMERIC_G2O>, __VA_ARGS__); else hipLaunchKernelGGL(kernel<SSX_JAC_ANALYTIC>, __VA_ARGS__); } while (0)
// The instantiations of the kernel templates lie in the code object in the order in which host code first names them: named here
// once, so that the device code does not depend on how the host code below and in the included files is arranged.
[[maybe_unused]] const void* const KERNEL_TEMPLATE_ORDER[] = {(const void*)k_linearize<1>, (const void*)k_linearize<0>, (const void*)k_pose_blocks<1>,
    (const void*)k_pose_blocks<0>, (const void*)k_lin_schur<0>, (const void*)k_lin_schur<1>, (const void*)k_bcr_fwd<24>, (const void*)k_bcr_fwd<36>, (const void*)k_bcr_bwd<24>,
    (const void*)k_bcr_bwd<36>, (const void*)k_lin_schur_b<0>, (const void*)k_lin_schur_b<1>, (const void*)k_linearize_b<0>, (const void*)k_linearize_b<1>};

// Raise the dynamic-LDS limits of the kernels that are launched with more than the default: once per process for the small-window
// kernels (single and batched), once per size class for the band kernels (their LDS depends on the window: SolveDev::lds_*).
void raise_lds_limits(size_t lds_seg = 0, size_t lds_top = 0, size_t lds_back = 0)
{
  auto raise_lds = [](auto* kernel, size_t bytes) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); };
  static bool attr_set = false;
  if (!attr_set) {
    raise_lds(k_lin_schur<SSX_JAC_ANALYTIC>, FUSED_LDS_BYTES); raise_lds(k_lin_schur<SSX_JAC_NUMERIC_G2O>, FUSED_LDS_BYTES);
    raise_lds(k_linearize<SSX_JAC_ANALYTIC>, LIN_LDS_BYTES); raise_lds(k_linearize<SSX_JAC_NUMERIC_G2O>, LIN_LDS_BYTES);
    raise_lds(k_schur, SCHUR_LDS_BYTES); raise_lds(k_schur_prep, SCHUR_PREP_LDS_BYTES); raise_lds(k_schur_b, SCHUR_LDS_BYTES);
    raise_lds(k_lin_schur_b<SSX_JAC_ANALYTIC>, FUSED_LDS_BYTES); raise_lds(k_lin_schur_b<SSX_JAC_NUMERIC_G2O>, FUSED_LDS_BYTES);
    raise_lds(k_linearize_b<SSX_JAC_ANALYTIC>, LIN_LDS_BYTES); raise_lds(k_linearize_b<SSX_JAC_NUMERIC_G2O>, LIN_LDS_BYTES);
    attr_set = true;
  }
  static size_t set_seg = 0, set_top = 0, set_back = 0;
  if (lds_seg > set_seg) { raise_lds(k_band_seg, lds_seg); set_seg = lds_seg; }
  if (lds_top > set_top) { raise_lds(k_band_top, lds_top); set_top = lds_top; }
  if (lds_back > set_back) { raise_lds(k_band_back, lds_back); set_back = lds_back; }
}

struct Comm { ssx_allreduce_fn fn = nullptr; void* user = nullptr; int world = 1; };

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

// the collective of a solve from its options; an RCCL communicator fills in opt.rank / opt.world_size
// (world_size 1 with a hook is allowed -- the hook is then an identity: it exercises the collective plumbing)
ssx_status make_comm(ssx_ctx* ctx, ssx_ba_options& opt, Comm& cm)
{
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
  return SSX_OK;
}

// the linearisation of one window into its per-chunk slabs and their sum over the chunks (cur / pb_cur: the state buffer the
// observations / the pose blocks of a large window are taken at; < 0: see k_linearize, k_pose_blocks)
void launch_lin_kernels(ssx_ctx* ctx, const BaDev& d, const BigDev& bd, int jac, int cur, int pb_cur)
{
  if (d.nCh > 0) SSX_PROF(ctx, KID_BA_LINEARIZE, LAUNCH_JAC(jac, k_linearize, dim3(d.nCh), dim3(CH), LIN_LDS_BYTES, ctx->stream, d, cur));
  if (d.big) {
    SSX_PROF(ctx, KID_BA_LINEARIZE, LAUNCH_JAC(jac, k_pose_blocks, dim3(d.nP), dim3(CH), 0, ctx->stream, d, bd, pb_cur));
    SSX_PROF(ctx, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_reduce_lin_big, dim3(1), dim3(CH), 0, ctx->stream, d));
  } else
  SSX_PROF(ctx, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_reduce_lin, dim3(std::max(1, (d.nP * 27 + 63) / 64)), dim3(CH), 0, ctx->stream, d));
}

// the ranks' sum of a linearisation, then lambda_0 (first iteration of a round) and, after a collective, the global chi2
ssx_status share_linearization(ssx_ctx* ctx, const BaDev& d, const Comm& cm, int first_iteration)
{
  SSX_TRY(allreduce(ctx, cm, d.iter_comm, (size_t)d.nP * 27 + 1 + d.world));
  if (first_iteration || cm.fn)
    SSX_PROF(ctx, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_lambda_init, dim3(1), dim3(64), 0, ctx->stream, d, first_iteration));
  return SSX_OK;
}

ssx_status launch_linearize(ssx_ctx* ctx, const BaDev& d, const BigDev& bd, const Comm& cm, int jac, int cur, int first_iteration)
{
  launch_lin_kernels(ctx, d, bd, jac, cur, cur);
  SSX_TRY(share_linearization(ctx, d, cm, first_iteration));
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
      SSX_TRY(allreduce(ctx, cm, ws->tiles.as<double>(), (size_t)T * T));
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

// ---- the outer loop of Backend::OptimizeActiveMap (backend.cpp:175-203: optimize(iters), count the outliers, compare the inlier
// ratio, go again), stated once for ssx_ba_solve and the batched solves ----------------------------------------------------------
// What an entry point does with a window in which no optimize() can run (no chunk on any rank, or iters <= 0).  The two entry points
// have always differed here and callers see it in ssx_ba_result: ssx_ba_solve still walks the rounds of such a window (rounds = 1 and
// n_inliers = E when the inlier ratio lets it stop, else outer_rounds), a batch never starts them (rounds = 0, n_inliers = 0).
enum IdleRounds { IDLE_ROUNDS_COUNTED, IDLE_ROUNDS_SKIPPED };

struct OuterState {                                                        // host state of one window in that loop
  int cur = 0, round = 0, rounds = 0, n_iters = 0, n_in = 0, n_outl = 0;   // cur: index of the accepted state buffer
  bool done = false, trial_err = false; double n_out = 0;                  // trial_err: err_trial holds the errors of the last trial evaluated
  void begin(int cur0, bool idle, int outer_rounds, IdleRounds ir) { cur = cur0; done = outer_rounds <= 0 || (idle && ir == IDLE_ROUNDS_SKIPPED); }
  // After one optimize(iters): sc = the window's control scalars (nullptr: idle, nothing ran), n_edges = its edges on all ranks.
  // Outlier statistics of the last evaluated trial (backend.cpp:181-194); done when the inlier ratio is reached or the rounds are used up.
  void after_optimize(const double* sc, double n_edges, const ssx_ba_options& opt)
  {
    if (sc) {
      cur = (int)sc[SC_CUR];
      n_out = sc[SC_NOUT];
      if (sc[SC_TRIALS_RUN] > 0.0) trial_err = true;
      n_iters = std::max(n_iters, (int)sc[SC_NSTAT]);
    }
    rounds++;
    const double cnt_in = n_edges - n_out;
    n_outl = (int)n_out; n_in = (int)cnt_in;
    const double ratio = n_edges > 0 ? cnt_in / (cnt_in + n_out) : 1.0;
    done = ratio > opt.inlier_ratio || ++round >= opt.outer_rounds;
  }
  void report(ssx_ba_result& r) const { r.rounds = rounds; r.n_iters = n_iters; r.n_inliers = n_in; r.n_outliers = n_outl; }
};

// LM slots (one = (re)linearise if needed + one trial) to enqueue now for n windows, hscal = their control scalars; 0: all have finished.
// The whole optimize(iters) first; a rejected trial consumes a slot without finishing its iteration, so then the host tops up: at least 1.
int slots_to_enqueue(int iters, bool first_pass, const double* hscal, const OuterState* st, int n)
{
  if (first_pass) return iters;
  int slots = 0;
  for (int w = 0; w < n; ++w)
    if (!st[w].done && hscal[(size_t)w * SC_N + SC_STOP] == 0.0) slots = std::max({slots, 1, iters - (int)hscal[(size_t)w * SC_N + SC_IT]});
  return slots;
}

// LM history of the iterations [k0, k1) from a window's pinned statistics block (chi2 | lambda | trials, SSX_BA_MAX_STATS each)
void copy_lm_history(ssx_ba_result& r, const double* hstat, int k0, int k1)
{
  for (int k = k0; k < k1 && k < SSX_BA_MAX_STATS; ++k) {
    r.iter_chi2[k] = hstat[k];
    r.iter_lambda[k] = hstat[SSX_BA_MAX_STATS + k];
    r.iter_trials[k] = (int)hstat[2 * SSX_BA_MAX_STATS + k];
  }
}

// Per-edge chi2 and outlier flags of one window from either storage form.  perm == nullptr: err = chi2 per entry of the caller's
// arrays (E_raw of them, a device-marshalled window); dead_point[e] < 0 marks a dead entry of an ssx_ba_window's storage, never
// evaluated.  Else err = the two error columns of the E sorted edges, and perm[s] is the caller's edge of sorted edge s.
void unpack_edge_errors(ssx_ba_result& r, const double* err, int E, int E_raw, const int* perm, const int* dead_point, double chi2_th)
{
  if (!r.edge_chi2 && !r.edge_outlier) return;
  for (int s = 0, n = perm ? E : E_raw; s < n; ++s) {
    if (!perm && dead_point && dead_point[s] < 0) continue;
    const int e = perm ? perm[s] : s;
    const double c2 = perm ? err[s] * err[s] + err[(size_t)E + s] * err[(size_t)E + s] : err[s];
    if (r.edge_chi2) r.edge_chi2[e] = c2;
    if (r.edge_outlier) r.edge_outlier[e] = c2 > chi2_th;
  }
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
  HostPrep& h = ba_workspace(ctx)->prep1;
  ssx_status st = prepare(ctx, prob, h, false);        // this hook returns per-edge blocks in the caller's order: it keeps the host's sort
  if (st != SSX_OK) return st;
  BaDev d;
  BigDev bd;
  BandPlan no_band;
  BandDev bnd;
  SSX_TRY(upload(ctx, prob, h, huber_delta, 5.891, 1, 0, d, bd, no_band, bnd));
  Comm cm;
  SSX_TRY(launch_linearize(ctx, d, bd, cm, jac_mode, 0, 1));
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

namespace {   // ---- ssx_ba_solve in steps

// what the steps of one solve share: the device views, the solver plan of a large window, the launch sizes that depend on it
struct SolveDev {
  BaDev d; BigDev bd; BandDev bnd; BandPlan bp; Comm cm;
  int jac = SSX_JAC_ANALYTIC;
  size_t lds_seg = 0, lds_top = 0, lds_back = 0;                                 // band solver (bnd.on): dynamic LDS of its kernels
  std::vector<int> tl_row_cnt, tl_pair_cnt; std::vector<uint8_t> tl_next_diag;   // tile Cholesky (d.big && !bnd.on): build_tile_lists
  // one rank: control block, statistics, estimate (pack_err: and per-edge chi2) leave in ONE kernel-written pinned block (fetch_control)
  bool pack_ok = false, pack_err = false, packed = false;
};

// a LARGE window (more than 16 free keyframes) with many observations: its columns start crossing PCIe before they are counted
ssx_status start_early_upload(ssx_ctx* ctx, const ssx_ba_problem* prob, const WinExt* ext)
{
  static const bool host_prep_env = getenv("SSX_BA_HOST_PREP") != nullptr || getenv("SSX_BA_HOST_LISTS") != nullptr;
  if (ext || host_prep_env || prob->E < (1 << 16) || prob->P <= SSX_BA_SMALL_P || !prob->poses) return SSX_OK;
  int n_free = 0;
  for (int i = 0; i < prob->P; ++i) n_free += !(prob->pose_fixed && prob->pose_fixed[i]);
  return n_free > SSX_BA_SMALL_P ? raw_upload_early(ctx, prob) : SSX_OK;
}

// Large windows: trajectory-shaped co-visibility (cyclic block band) -> the sliding-window / nested-dissection solver
// of ba_band.inc; anything else -> the 64x64-tile sparse Cholesky of ba_big.inc.  With several ranks the decision
// must be common: the ranks exchange which bandwidth class their shard falls in (one tiny all-reduce).
ssx_status plan_large_solver(ssx_ctx* ctx, const HostPrep& h, const ssx_ba_options& opt, const Comm& cm, BandPlan& bp)
{
  if (!h.big) return SSX_OK;
  if (opt.large_solver != SSX_LARGE_SOLVER_TILES) {
    int w = std::max(h.band_w, 1);
    if (w > BAND_WMAX) w = BAND_WMAX + 1;
    if (cm.fn) {
      BaWorkspace* w0 = ba_workspace(ctx);
      double hist[BAND_WMAX + 2] = {0};
      hist[w] = 1.0;
      SSX_HIP_TRY(ctx, w0->tiles.reserve(sizeof(hist)));
      SSX_HIP_TRY(ctx, hipMemcpyAsync(w0->tiles.p, hist, sizeof(hist), hipMemcpyHostToDevice, ctx->stream));
      SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      SSX_TRY(allreduce(ctx, cm, w0->tiles.as<double>(), BAND_WMAX + 2));
      SSX_HIP_TRY(ctx, hipMemcpyAsync(hist, w0->tiles.p, sizeof(hist), hipMemcpyDeviceToHost, ctx->stream));
      SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      for (int i = 1; i <= BAND_WMAX + 1; ++i) if (hist[i] != 0.0) w = i;
    }
    if (w <= BAND_WMAX && h.nP >= 2 * w + 2) { plan_band(h.nP, w, bp); plan_bcr(h.nP, w, bp.bcr); }
  }
  if (opt.large_solver == SSX_LARGE_SOLVER_BAND && bp.w == 0) {
    ctx->set_error("ssx_ba_solve: the band solver was requested but the co-visibility bandwidth is %d poses (> %d)", h.band_w, BAND_WMAX);
    return SSX_ERR_UNSUPPORTED;
  }
  return SSX_OK;
}

// the end of every trial of a large window: the step applied to the poses, the sums of its scale
void big_trial_update(ssx_ctx* ctx, const SolveDev& S)
{
  const int nparts = std::min(32, (S.d.P + CH - 1) / CH);
  SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_pose_update_big, dim3(nparts), dim3(CH), 0, ctx->stream, S.d, S.bd, -1, 0.0, 2));
  SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_scale_finish, dim3(1), dim3(64), 0, ctx->stream, S.d, S.bd, nparts));
}

// One trial of a large window.  Damping, state buffer and stop flag come from the device's LM control block: the kernels shared with the
// pose graph are told so by cur = -1, lambda_arg = 0, use_dev_lambda = 2.
// BAND solver: Schur blocks straight into the band layout -> (all-reduce) -> block cyclic reduction, or segments || -> separator system
// -> segments ||.  fuse_iter: the trial's all-reduce also carries iter_comm (pose blocks, chi2, max-diagonal slots of the linearisation),
// which then needs no collective of its own: two all-reduces per LM trial instead of three
ssx_status big_trial_band(ssx_ctx* ctx, const SolveDev& S, bool fuse_iter)
{
  const BaDev& d = S.d; const BigDev& bd = S.bd; const BandDev& bnd = S.bnd; const Comm& cm = S.cm;
  const size_t lds_seg = S.lds_seg, lds_top = S.lds_top, lds_back = S.lds_back;
  hipStream_t s = ctx->stream;
  const size_t band_doubles = (size_t)bnd.nP * (bnd.w + 1) * 36;
  SSX_HIP_TRY(ctx, hipMemsetAsync(bnd.Sb, 0, sizeof(double) * band_doubles, s));
  if (d.nCh > 0) SSX_PROF(ctx, KID_BA_SCHUR, hipLaunchKernelGGL(k_schur_prep, dim3(d.nCh), dim3(CH), SCHUR_PREP_LDS_BYTES, s, d, bd));
  SSX_PROF(ctx, KID_BA_SCHUR, hipLaunchKernelGGL(k_schur_blocks_band, dim3((bd.nBlkS + 3) / 4), dim3(CH), 0, s, d, bd, bnd));
  SSX_PROF(ctx, KID_BA_REDUCE_SCHUR, hipLaunchKernelGGL(k_bs_band, dim3(d.nP), dim3(CH), 0, s, d, bd, bnd));
  SSX_TRY(allreduce(ctx, cm, bnd.Sb, band_doubles + (size_t)bd.n + (fuse_iter ? (size_t)d.nP * 27 + 1 + d.world : 0)));
  if (fuse_iter) SSX_PROF(ctx, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_lambda_init, dim3(1), dim3(64), 0, s, d, 0));   // the global chi2 of the linearisation
  if (bnd.bcr.on) {
    // block cyclic reduction: log2(N) levels of concurrent super-block eliminations, then as many of back-substitution
    const std::vector<int>& lv = S.bp.bcr.lvl;
    SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_bcr_build, dim3(bnd.bcr.N), dim3(256), 0, s, d, bnd, bnd.bcr, 0.0, 2));
    const bool m24 = bnd.bcr.m == 24;
    const std::vector<int>& lm = S.bp.bcr.lvM;
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
  big_trial_update(ctx, S);
  return SSX_OK;
}

// TILE solver: Schur blocks -> dense S -> (all-reduce of the non-zero tiles) -> blocked Cholesky (MFMA) -> back-substitution
ssx_status big_trial_tiles(ssx_ctx* ctx, const SolveDev& S)
{
  const BaDev& d = S.d; const BigDev& bd = S.bd; const Comm& cm = S.cm;
  const std::vector<int>& tl_row_cnt = S.tl_row_cnt; const std::vector<int>& tl_pair_cnt = S.tl_pair_cnt; const std::vector<uint8_t>& tl_next_diag = S.tl_next_diag;
  hipStream_t s = ctx->stream;
  SSX_HIP_TRY(ctx, hipMemsetAsync(bd.S, 0, sizeof(double) * (size_t)(bd.n_pad + 1) * bd.ld, s));
  if (d.nCh > 0) SSX_PROF(ctx, KID_BA_SCHUR, hipLaunchKernelGGL(k_schur_prep, dim3(d.nCh), dim3(CH), SCHUR_PREP_LDS_BYTES, s, d, bd));
  SSX_PROF(ctx, KID_BA_SCHUR, hipLaunchKernelGGL(k_schur_blocks, dim3((bd.nBlkS + 3) / 4), dim3(CH), 0, s, d, bd));
  SSX_PROF(ctx, KID_BA_REDUCE_SCHUR, hipLaunchKernelGGL(k_bs, dim3(d.nP), dim3(CH), 0, s, d, bd));
  if (cm.fn) {
    // exchange the non-zero tiles and the rhs row only
    hipLaunchKernelGGL(k_pack_tiles, dim3(bd.n_init + 1), dim3(CH), 0, s, bd, 0);
    SSX_TRY(allreduce(ctx, cm, bd.Spack, (size_t)bd.n_init * NB_TILE + bd.n_pad));
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
  big_trial_update(ctx, S);
  return SSX_OK;
}

// the end of every trial: back-substitution, the trial's residuals, its sums and the LM decision (lm_step on the device);
// one GPU: the last chunk of k_backsub_residual sums the trial and takes the LM decision itself (finish)
ssx_status finish_trial(ssx_ctx* ctx, const SolveDev& S)
{
  const BaDev& d = S.d; const Comm& cm = S.cm;
  const bool finish = d.nCh > 0 && !cm.fn && g_trial_finish.load() != 0;
  if (d.nCh > 0) SSX_PROF(ctx, KID_BA_BACKSUB, hipLaunchKernelGGL(k_backsub_residual, dim3(d.nCh), dim3(CH), 0, ctx->stream, d, finish ? 1 : 0));
  if (!finish) SSX_PROF(ctx, KID_BA_REDUCE_TRIAL, hipLaunchKernelGGL(k_reduce_trial, dim3(1), dim3(CH), 0, ctx->stream, d, cm.fn ? 0 : 1));
  if (cm.fn) {
    SSX_TRY(allreduce(ctx, cm, d.scal_comm, 3));
    SSX_PROF(ctx, KID_BA_REDUCE_TRIAL, hipLaunchKernelGGL(k_publish_trial, dim3(1), dim3(1), 0, ctx->stream, d));
  }
  return SSX_OK;
}

// One LM slot of a SMALL window.  The first slot of an optimize() needs lambda_0 between the linearisation and the Schur
// complement; every later slot of a single-rank solve knows its damping: one fused kernel, and the two reductions as one launch.
ssx_status enqueue_slot_small(ssx_ctx* ctx, const SolveDev& S, bool first_slot)
{
  const BaDev& d = S.d; const Comm& cm = S.cm;
  const int n = 6 * d.nP, nCh = d.nCh, nSchurEntries = d.nBlk * 36 + d.nP * 6;
  const bool fused = !first_slot && !cm.fn && nCh > 0 && n > 0;
  static const bool no_both_env = getenv("SSX_BA_SPLIT_REDUCE") != nullptr;   // (tools: the two launches, for A/B timing)
  const bool both = fused && !no_both_env;
  if (fused) {
    const int n_rl = std::max(1, (d.nP * 27 + 63) / 64);
    SSX_PROF(ctx, KID_BA_LIN_SCHUR, LAUNCH_JAC(S.jac, k_lin_schur, dim3(nCh), dim3(CH), FUSED_LDS_BYTES, ctx->stream, d));
    if (both) SSX_PROF(ctx, KID_BA_REDUCE_SCHUR, hipLaunchKernelGGL(k_reduce_both, dim3(n_rl + (nSchurEntries + 63) / 64), dim3(CH), 0, ctx->stream, d, n_rl));
    else SSX_PROF(ctx, KID_BA_REDUCE_LIN, hipLaunchKernelGGL(k_reduce_lin, dim3(n_rl), dim3(CH), 0, ctx->stream, d));
  } else
    launch_lin_kernels(ctx, d, S.bd, S.jac, -1, -1);
  SSX_TRY(share_linearization(ctx, d, cm, first_slot ? 1 : 0));
  if (n > 0) {
    if (nCh > 0 && !fused) SSX_PROF(ctx, KID_BA_SCHUR, hipLaunchKernelGGL(k_schur, dim3(nCh), dim3(CH), SCHUR_LDS_BYTES, ctx->stream, d));
    if (!both) SSX_PROF(ctx, KID_BA_REDUCE_SCHUR, hipLaunchKernelGGL(k_reduce_schur, dim3((nSchurEntries + 63) / 64), dim3(CH), 0, ctx->stream, d));
    SSX_TRY(allreduce(ctx, cm, d.trial_comm, (size_t)n * n + n));
  }
  if (n <= NB) SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_solve64, dim3(1), dim3(CH), 0, ctx->stream, d));
  else if (n <= 80) SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_solve80, dim3(1), dim3(CH), 0, ctx->stream, d));
  else SSX_PROF(ctx, KID_BA_SOLVE, hipLaunchKernelGGL(k_solve, dim3(1), dim3(CH), 0, ctx->stream, d));
  return finish_trial(ctx, S);
}

// One LM slot of a LARGE window.  k_linearize skips itself while the kept linearisation is valid; the pose blocks too unless a
// collective follows: their all-reduced copy must be rebuilt from this rank's part before it is summed again.
ssx_status enqueue_slot_big(ssx_ctx* ctx, const SolveDev& S, bool first_slot)
{
  launch_lin_kernels(ctx, S.d, S.bd, S.jac, -1, S.cm.fn ? -1 : -2);
  // (band solver, later slots: lambda is known, so the linearisation's sums travel with the trial's reduced system)
  const bool fuse_iter = S.bnd.on && S.cm.fn && !first_slot;
  ssx_status st = fuse_iter ? SSX_OK : share_linearization(ctx, S.d, S.cm, first_slot ? 1 : 0);
  if (st == SSX_OK) st = S.bnd.on ? big_trial_band(ctx, S, fuse_iter) : big_trial_tiles(ctx, S);
  return st != SSX_OK ? st : finish_trial(ctx, S);
}

// Behind the last slot of an optimize(): the control block to the host, on one rank with everything else a last round leaves
// (SolveDev::pack_ok).  stage = the download block in pinned memory (poses | points | errors).
ssx_status fetch_control(ssx_ctx* ctx, SolveDev& S, double* hscal, double* stage, bool have_trial_err)
{
  const BaDev& d = S.d;
  if (!S.pack_ok) {
    SSX_HIP_TRY(ctx, hipMemcpyAsync(hscal, d.scal, sizeof(double) * SC_N, hipMemcpyDeviceToHost, ctx->stream));
    return SSX_OK;
  }
  double* const pk_point = stage + 7 * (size_t)d.P;
  if (S.pack_err) {
    hipLaunchKernelGGL(k_c2_out, dim3((d.E + CH - 1) / CH), dim3(CH), 0, ctx->stream, d, have_trial_err ? 1 : 2);
    hipLaunchKernelGGL(k_stream_out, dim3((unsigned)std::min<size_t>(256, ((size_t)d.E_raw + 2 * CH - 1) / (2 * CH))), dim3(CH), 0, ctx->stream, (const double*)d.c2_out, pk_point + 3 * (size_t)d.L, (size_t)d.E_raw);
  }
  const size_t n_pack = SC_N + 3 * SSX_BA_MAX_STATS + 7 * (size_t)d.P + 3 * (size_t)d.L;
  hipLaunchKernelGGL(k_pack_one, dim3((unsigned)std::min<size_t>(256, (n_pack + CH - 1) / CH)), dim3(CH), 0, ctx->stream, d, hscal, stage, pk_point);
  SSX_HIP_TRY(ctx, hipGetLastError());
  S.packed = true;
  return SSX_OK;
}

// enqueue what the caller asked for and the pinned block does not hold yet: the estimate, the per-edge errors
ssx_status enqueue_download(ssx_ctx* ctx, const SolveDev& S, double* stage, const OuterState& os, bool want_err)
{
  const BaDev& d = S.d;
  double* h_point = stage + 7 * (size_t)d.P;
  double* h_err = h_point + 3 * (size_t)d.L;
  if (!S.packed) {
    SSX_HIP_TRY(ctx, hipMemcpyAsync(stage, d.pose[os.cur], sizeof(double) * 7 * d.P, hipMemcpyDeviceToHost, ctx->stream));
    if (d.L) SSX_HIP_TRY(ctx, hipMemcpyAsync(h_point, d.point[os.cur], sizeof(double) * 3 * d.L, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (!want_err || (S.packed && S.pack_err)) return SSX_OK;
  if (!os.trial_err) {   // iters == 0: errors of the input state
    Comm none;
    SSX_TRY(launch_linearize(ctx, d, S.bd, none, SSX_JAC_ANALYTIC, os.cur, 0));
  }
  if (d.dev_prep) {                                  // chi2 per edge, already in the caller's order
    hipLaunchKernelGGL(k_c2_out, dim3((d.E + CH - 1) / CH), dim3(CH), 0, ctx->stream, d, os.trial_err ? 1 : 0);
    SSX_HIP_TRY(ctx, hipMemcpyAsync(h_err, d.c2_out, sizeof(double) * (size_t)d.E_raw, hipMemcpyDeviceToHost, ctx->stream));
  } else
  SSX_HIP_TRY(ctx, hipMemcpyAsync(h_err, os.trial_err ? d.err_trial : d.err_lin, sizeof(double) * 2 * (size_t)d.E, hipMemcpyDeviceToHost, ctx->stream));
  return SSX_OK;
}

// collect_stats: the HIP-event records of this call, summed per phase
void sum_phase_times(ssx_ctx* ctx, ssx_ba_result* res)
{
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
}

}  // namespace

// ssx_ba_solve, and the solve of one ssx_ba_window (`ext`: raw arrays and state resident in the window's buffers)
static ssx_status ba_solve_impl(ssx_ctx* ctx, const ssx_ba_problem* prob, const ssx_ba_options* opt_in, ssx_ba_result* res, WinExt* ext)
{
  if (!ctx || !prob || !res) return SSX_ERR_INVALID_ARG;
  ssx_ba_options opt;
  if (opt_in) opt = *opt_in; else ssx_ba_default_options(&opt);
  // the index lists are rebuilt per call (the window changes with every keyframe) but their storage is kept with the ctx:
  // ~20 vectors of up to E entries are not re-allocated and re-faulted every solve
  BaWorkspace* ws = ba_workspace(ctx);
  HostPrep& h = ws->prep1;
  static const bool timing = getenv("SSX_BA_TIMING") != nullptr;       // host phases of the call on stderr (tools/ba_c4_slope.py)
  const auto tc0 = std::chrono::steady_clock::now();
  auto tc_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc0).count(); };
  double tph[6] = {0, 0, 0, 0, 0, 0};
  SSX_TRY(start_early_upload(ctx, prob, ext));
  const ssx_status st = prepare(ctx, prob, h, true, ext);
  if (st != SSX_OK || !(h.big && h.dev_prep)) ws->raw_early.valid = false;   // (never reaches big_records: the early copy is dropped)
  if (st != SSX_OK) return st;
  tph[0] = tc_ms();
  if (ext && (!h.dev_prep || h.big)) {
    ctx->set_error("ssx_ba_window: %d free keyframes (a window holds at most %d) or the device-side marshalling is switched off", h.nP, SSX_BA_SMALL_P);
    return SSX_ERR_UNSUPPORTED;
  }
  SolveDev S; BaDev& d = S.d;
  SSX_TRY(make_comm(ctx, opt, S.cm));
  const Comm& cm = S.cm;
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
  const unsigned long long* pairs_dev = nullptr;
  BaDev recs;
  const int* pe_ptr_dev = nullptr; const int* pe_edge_dev = nullptr;
  const bool big_dev = h.big && h.dev_prep;
  if (big_dev) SSX_TRY(big_records(ctx, prob, h, recs, &pe_ptr_dev, &pe_edge_dev));
  if (h.big) SSX_TRY(build_pairs(ctx, h, &pairs_dev, big_dev ? &recs : nullptr));
  tph[1] = tc_ms();
  SSX_TRY(plan_large_solver(ctx, h, opt, cm, S.bp));
  SSX_TRY(upload(ctx, prob, h, opt.huber_delta, opt.chi2_th, cm.world, cm.fn ? opt.rank : 0, d, S.bd, S.bp, S.bnd, ext, big_dev ? &recs : nullptr, pe_ptr_dev, pe_edge_dev));
  tph[2] = tc_ms();
  d.store_w = (d.big || opt.jac_mode == SSX_JAC_NUMERIC_G2O) ? 1 : 0;
  d.no_err = (!d.big && !(res->edge_chi2 || res->edge_outlier)) ? 1 : 0;
  S.bd.spair_ab = pairs_dev;
  S.jac = opt.jac_mode;
  double* hscal = ws->scal.as<double>();
  double* const stage = reinterpret_cast<double*>(ws->stage.as<char>());   // the download block in pinned memory (poses | points | errors)
  if (S.bnd.on) {
    const BandDev& bnd = S.bnd;
    const int w1 = bnd.K == 1 ? bnd.w : bnd.wr, n1 = bnd.K == 1 ? bnd.nP : bnd.nPr;
    const int m_max = *std::max_element(S.bp.seg_m.begin(), S.bp.seg_m.end());
    S.lds_seg = band_lds_elim(bnd.w, bnd.w);
    S.lds_top = std::max(band_lds_elim(w1, bnd.w), band_lds_back(w1, bnd.w, n1));
    S.lds_back = band_lds_back(bnd.w, bnd.w, m_max + 2 * bnd.w);
  }
  raise_lds_limits(S.lds_seg, S.lds_top, S.lds_back);
  if (d.big && !S.bnd.on) SSX_TRY(build_tile_lists(ctx, ws, h.sblk_pa, h.sblk_pb, cm, S.bd, S.tl_row_cnt, S.tl_pair_cnt, S.tl_next_diag));
  res->rounds = 0; res->n_iters = 0; res->n_inliers = 0; res->n_outliers = 0;
  const bool want_err = (res->edge_chi2 || res->edge_outlier) && d.E > 0;
  static const bool no_pack_env = getenv("SSX_BA_NO_PACK") != nullptr;       // (tools: the three copies of before, for A/B timing)
  S.pack_ok = !cm.fn && !no_pack_env;
  S.pack_err = S.pack_ok && want_err && d.dev_prep;
  // with several ranks every rank must take part in every collective, even with an empty shard
  const bool active = (d.nCh > 0) || cm.fn != nullptr;
  const bool idle = !active || opt.iters <= 0;
  OuterState os;
  os.begin(ext ? ext->cur : 0, idle, opt.outer_rounds, IDLE_ROUNDS_COUNTED);
  while (!os.done) {
    // ---- one g2o optimize(iters): OptimizationAlgorithmLevenberg::solve per iteration.  The whole optimize(iters) is enqueued;
    // lm_step() on the device decides after every trial (no stream synchronisation per trial) ----
    hipLaunchKernelGGL(k_lm_begin, dim3(1), dim3(1), 0, ctx->stream, d, os.cur, opt.iters, os.n_iters, active ? 0 : 1);
    bool first_slot = true;
    for (int pass = 0; !idle; ++pass) {
      const int slots = slots_to_enqueue(opt.iters, pass == 0, hscal, &os, 1);
      if (slots == 0) break;
      for (int sidx = 0; sidx < slots; ++sidx, first_slot = false) SSX_TRY(d.big ? enqueue_slot_big(ctx, S, first_slot) : enqueue_slot_small(ctx, S, first_slot));
      SSX_HIP_TRY(ctx, hipGetLastError());
      SSX_TRY(fetch_control(ctx, S, hscal, stage, os.trial_err));
      SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));          // the one host round trip of an optimize(iters)
    }
    if (!idle && (int)hscal[SC_NSTAT] > os.n_iters) {
      double* hstat = hscal + SC_N;                                  // pinned, behind the scalar block
      if (!S.packed) {                                               // (k_pack_one brought them along)
        SSX_HIP_TRY(ctx, hipMemcpyAsync(hstat, d.lm_stat, sizeof(double) * 3 * SSX_BA_MAX_STATS, hipMemcpyDeviceToHost, ctx->stream));
        SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      }
      copy_lm_history(*res, hstat, os.n_iters, (int)hscal[SC_NSTAT]);
    }
    double n_edges_total = (double)d.E;                              // with several ranks n_out is the global count: so must this be
    if (cm.fn) {
      double e_local = (double)d.E;
      SSX_HIP_TRY(ctx, hipMemcpyAsync(d.scal_comm, &e_local, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // e_local is a stack variable
      SSX_TRY(allreduce(ctx, cm, d.scal_comm, 1));
      SSX_HIP_TRY(ctx, hipMemcpyAsync(&n_edges_total, d.scal_comm, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    os.after_optimize(idle ? nullptr : hscal, n_edges_total, opt);
    os.report(*res);
  }
  SSX_TRY(enqueue_download(ctx, S, stage, os, want_err));
  SSX_HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  tph[3] = tc_ms();
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  tph[4] = tc_ms();
  if (res->poses_out) memcpy(res->poses_out, stage, sizeof(double) * 7 * d.P);
  if (res->points_out && d.L) memcpy(res->points_out, stage + 7 * (size_t)d.P, sizeof(double) * 3 * d.L);
  if (ext) ext->cur = os.cur;
  if (want_err) unpack_edge_errors(*res, stage + 7 * (size_t)d.P + 3 * (size_t)d.L, d.E, d.E_raw, d.dev_prep ? nullptr : h.perm.data(), ext ? prob->edge_point : nullptr, opt.chi2_th);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
  res->ms_total = ms;
  res->ms_setup = 0.f;
  if (timing)
    fprintf(stderr, "ssx_ba_solve P %d L %d E %d: (columns staged + sent early, large windows) + prepare %.3f | records + pairs %.3f | plan + upload %.3f | LM enqueued (and its host round trips) %.3f | "
                    "last sync %.3f | results %.3f ms (host clock); GPU first to last event %.3f ms\n", d.P, d.L, d.E, tph[0], tph[1] - tph[0],
            tph[2] - tph[1], tph[3] - tph[2], tph[4] - tph[3], tc_ms() - tph[4], ms);
  if (stats_guard.mine) sum_phase_times(ctx, res);
  return SSX_OK;
}

extern "C" ssx_status ssx_ba_solve(ssx_ctx* ctx, const ssx_ba_problem* prob, const ssx_ba_options* opt_in, ssx_ba_result* res) { return ba_solve_impl(ctx, prob, opt_in, res, nullptr); }

#include "ba_batch.inc"

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
  if (k == "k_schur_prep") return (int64_t)SCHUR_PREP_LDS_BYTES;
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

// test hook (no GPU needed): FNV-1a digest of everything prepare() hands on to the upload -- every scalar and array of HostPrep the
// upload reads -- with the large window's observations counted on `threads` host threads, and of the plan of the arena made from it:
// every offset in declaration order, the blob's bytes and the total, without and with the pristine copy of a resident batch (a single
// window is laid out like a window of a one-shot batch), for one and two ranks and as a resident window, a large window also on the band solver
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
  auto eat_v = [&](const auto& v, size_t n) { n = std::min(n, v.size()); eat(&n, sizeof(n)); eat(v.data(), sizeof(v[0]) * n); };
  const size_t all = ~size_t(0), ref = h.dev_prep ? 0 : all;         // (a device-marshalled window leaves the reference's arrays as they were)
  const int sc[13] = {h.P, h.L, h.E, h.E_raw, h.nP, h.nLm, h.nCh, h.nBlk, h.raw_fmt, h.big, h.dev_lists, h.dev_prep, h.band_w};
  eat(sc, sizeof(sc));
  eat_v(h.lm_ptr, all); eat_v(h.lm_id, all); eat_v(h.slot8, h.dev_prep ? h.E_raw : 0); eat_v(h.pe_ptr, all); eat_v(h.ch_lm, all);
  eat_v(h.pose_free, all); eat_v(h.lm_fixed, all); eat_v(h.lm_compact, all); eat_v(h.pose_rank, all); eat_v(h.ch_desc, 4 * (size_t)h.nCh);
  eat_v(h.blk_pa, all); eat_v(h.blk_pb, all);
  eat_v(h.e_pose, ref); eat_v(h.e_lmc, ref); eat_v(h.e_cam, ref); eat_v(h.e_dup, ref); eat_v(h.e_uv, ref); eat_v(h.perm, all);
  eat_v(h.e_rec, std::min(ref, 4 * (size_t)h.E)); eat_v(h.l_rec, std::min(ref, 4 * (size_t)h.nLm)); eat_v(h.lm_chunk, std::min(ref, (size_t)h.nLm));
  eat_v(h.pptr, all); eat_v(h.pair_a, all); eat_v(h.pair_b, all); eat_v(h.pair_ptr, all); eat_v(h.bseg, all); eat_v(h.bseg_ptr, all);
  eat_v(h.touch, (ref && !h.big) ? all : 0);
  eat_v(h.pe_edge, all); eat_v(h.sblk_pa, all); eat_v(h.sblk_pb, all); eat_v(h.spair_ptr, all);
  BandPlan bands[2];
  if (h.big) { plan_band(h.nP, 3, bands[1]); plan_bcr(h.nP, 3, bands[1].bcr); }
  const WinExt win;                                                  // (a resident window: state and raw arrays in buffers of its own)
  for (int v = 0; v < (h.dev_prep && !h.big ? 3 : 2); ++v)           // one rank, one of two ranks, a resident window
   for (int keep_init = 0; keep_init < 2; ++keep_init)
    for (int b = 0; b < (h.big ? 2 : 1); ++b) {
      const ArenaPlan p = plan_arena(prob, h, bands[b], v == 1 ? 2 : 1, keep_init != 0, v == 2 ? &win : nullptr, h.big && h.dev_prep);
      for (const Span* s = p.spans_begin(); s != p.spans_end(); ++s) eat(&s->off, sizeof(size_t));
      eat(&p.in_bytes, sizeof(size_t)); eat(&p.total, sizeof(size_t));
    }
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

}  // extern "C"

#include "ba_window.inc"
#include "pg.inc"
#include "loop_correct.inc"
#include "ba_window_loop.inc"
