// ssvio_amd/csrc/pose_only.hip -- per-frame pose-only robust optimisation on gfx950 (ssx_pose_only_opt).
//
// Replaces the optimisation core of FrontEnd::EstimateCurrentPose (/root/reference/src/ssvio/frontend.cpp:184-270):
// one VertexPose, one EdgeProjectionPoseOnly per tracked map point (analytic 2x6 Jacobian,
// include/ssvio/g2otypes.hpp:67-110), Huber kernel (delta 1.0 = g2o's default ctor), LinearSolverDense, LM;
// 4 rounds x optimize(10) with chi2 > 5.991 => outlier (level 1) after every round and the kernels removed before
// the last round (frontend.cpp:236-269).
//
// The problem is tiny (50-400 edges, 6 unknowns) and strictly sequential across LM trials, so the WHOLE procedure --
// all rounds, iterations and LM trials -- runs inside ONE launch of ONE 256-thread workgroup: no host round trip,
// no second kernel.  k_pose_only<EPT> (M <= 256 * EPT) keeps every edge (map point, pixel, last error, level) in the
// registers of its thread for the whole launch; the 6x6 normal equations (21 + 6 values) and every chi2 are summed by
// a wave butterfly + one LDS exchange between the 4 waves (ONE barrier per sum, double-buffered), and every thread
// then runs the 6x6 Cholesky, the pose update and the LM bookkeeping of OptimizationAlgorithmLevenberg::solve
// (thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:58-175) redundantly on identical values -- no
// broadcast, no second barrier.  k_pose_only_generic (any M) is the same procedure with the edges in global memory
// and an LDS tree reduction.
//
// LoopClosing::OptimizeCurrentPose (src/ssvio/loopclosing.cpp:245-351) is the same procedure behind one extra optimize(10) over all
// edges (:305-306), and g2o restarts lambda and ni at iteration 0 of every optimize(): PoDev::warmup counts such passes (no
// classification behind them, the robust kernel on).  Its initial pose is the result of a kernel (pnp.hip), so PoDev::pose may be
// device memory and PoDev::gate a device word that calls the whole launch off (po_launch_device, pose_only.hpp).
#include <cmath>

#include "ctx.hpp"
#include "pose_only.hpp"
#include "se3.hpp"
#include "../../include/ssx_test_hooks.h"

namespace {

constexpr int PT = 256;
static_assert(PT == kPoThreads, "po_class (pose_only.hpp) counts edges per thread of this workgroup");
constexpr int NRED = 28;   // 21 (upper 6x6) + 6 (b) + 1 (chi2)

// The record of the traced instantiations (include/ssx_test_hooks.h: ssx_pose_only_debug_trace; never part of a product build and
// never an argument of the shipped kernels).  What g2o exposes in postIteration, slot (warmup + round) * iters + it: the robust chi2
// of the edges' current errors (the trial state after a rejected last trial), lambda, the trials of the iteration; per optimize()
// 4 ints: active edges, iterations run, 1 = its last iteration terminated, outliers after the classification (-1: a warm-up pass).
struct PoTrace {
  double* chi2;
  double* lambda;
  int* trials;
  int* round_rec;
};

__device__ __forceinline__ void po_error(const double* T, const PoDev& d, int i, double* e, double* pc)
{
  const double X[3] = {d.xyz[3 * i], d.xyz[3 * i + 1], d.xyz[3 * i + 2]};
  ssx::se3_act(T, X, pc);
  const double hx = d.K.fx * pc[0] + d.K.cx * pc[2];
  const double hy = d.K.fy * pc[1] + d.K.cy * pc[2];
  e[0] = d.uv[2 * i] - hx / pc[2];
  e[1] = d.uv[2 * i + 1] - hy / pc[2];
}

// all threads: reduce `n` values per thread (column-major sRed[k][t]) with one tree; result in sRed[k][0]
__device__ __forceinline__ void tree_reduce(double (*sRed)[PT], int n)
{
  const int t = threadIdx.x;
  __syncthreads();
  for (int o = PT / 2; o > 0; o >>= 1) {
    if (t < o)
      for (int k = 0; k < n; ++k) sRed[k][t] += sRed[k][t + o];
    __syncthreads();
  }
}

// the record of a traced instantiation (the one element of the kernel's parameter pack), nothing for a shipped one
__device__ __forceinline__ const PoTrace* po_trace_of() { return nullptr; }
__device__ __forceinline__ const PoTrace* po_trace_of(const PoTrace& tr) { return &tr; }
__device__ __forceinline__ const PoTrace* po_trace_at(const PoTrace* tv, unsigned problem) { return tv + problem; }

// one workgroup, one problem with its edges in device memory: the body of k_pose_only_generic and k_pose_only_generic_jobs.
// TRACE: the traced instantiation of the test hook writes its record through tr
template <bool TRACE>
__device__ __forceinline__ void pose_only_generic_block(const PoDev& d, [[maybe_unused]] const PoTrace* tr)
{
  __shared__ double sRed[NRED][PT];
  __shared__ double sT[7], sTbak[7], sX[6];
  __shared__ double sCtl[8];      // 0 lambda, 1 ni, 2 currentChi, 3 rho, 4 qmax, 5 stop flag, 6 accepted
  __shared__ int sUseKernel;
  const int t = threadIdx.x;
  if (d.gate && *d.gate == 0) return;
  if (t < 7) sT[t] = d.pose[t];
  if (t == 0) sUseKernel = 1;
  for (int i = t; i < d.M; i += PT) { d.level[i] = 0; d.outlier[i] = 0; d.err[2 * i] = 0.0; d.err[2 * i + 1] = 0.0; }
  __syncthreads();

  // errors of the active (level 0) edges at the current pose + robust chi2 -> sRed[27][0]
  auto errors_and_chi2 = [&]() {
    double T[7];
    for (int k = 0; k < 7; ++k) T[k] = sT[k];
    double chi = 0.0;
    for (int i = t; i < d.M; i += PT) {
      if (d.level[i]) continue;
      double e[2], pc[3];
      po_error(T, d, i, e, pc);
      d.err[2 * i] = e[0]; d.err[2 * i + 1] = e[1];
      const double c2 = e[0] * e[0] + e[1] * e[1];
      double r0 = c2, w = 1.0;
      if (sUseKernel) ssx::huber(c2, d.huber_delta, r0, w);
      chi += r0;
    }
    sRed[27][t] = chi;
    tree_reduce(sRed + 27, 1);
    return sRed[27][0];
  };

  int cnt_outliers = 0;
  for (int round = -d.warmup; round < d.rounds; ++round) {   // round < 0: a warm-up pass
    // initializeOptimization(0): only level-0 edges are active
    int mine = 0;
    for (int i = t; i < d.M; i += PT) mine += !d.level[i];
    sRed[0][t] = (double)mine;
    tree_reduce(sRed, 1);
    const int n_active = (int)sRed[0][0];
    __syncthreads();
    int its_run = 0;
    bool terminated = false;
    for (int it = 0; it < d.iters && n_active > 0; ++it) {
      const double chi_now = errors_and_chi2();
      __syncthreads();
      // ---- linearise: H (upper 21), b (6) ----
      {
        double T[7];
        for (int k = 0; k < 7; ++k) T[k] = sT[k];
        double acc[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) acc[k] = 0.0;
        for (int i = t; i < d.M; i += PT) {
          if (d.level[i]) continue;
          const double Xw[3] = {d.xyz[3 * i], d.xyz[3 * i + 1], d.xyz[3 * i + 2]};
          double pc[3];
          ssx::se3_act(T, Xw, pc);
          const double X = pc[0], Y = pc[1], Z = pc[2];
          const double Zinv = 1.0 / (Z + 1e-18), Zinv2 = Zinv * Zinv;
          // EdgeProjectionPoseOnly::linearizeOplus, g2otypes.hpp:86-101
          const double J[12] = {-d.K.fx * Zinv, 0, d.K.fx * X * Zinv2, d.K.fx * X * Y * Zinv2, -d.K.fx - d.K.fx * X * X * Zinv2,
                                d.K.fx * Y * Zinv, 0, -d.K.fy * Zinv, d.K.fy * Y * Zinv2, d.K.fy + d.K.fy * Y * Y * Zinv2,
                                -d.K.fy * X * Y * Zinv2, -d.K.fy * X * Zinv};
          const double e0 = d.err[2 * i], e1 = d.err[2 * i + 1];
          double r0, w = 1.0;
          if (sUseKernel) ssx::huber(e0 * e0 + e1 * e1, d.huber_delta, r0, w);
          int q = 0;
#pragma unroll
          for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int c = a; c < 6; ++c) acc[q++] += J[a] * w * J[c] + J[6 + a] * w * J[6 + c];
          }
#pragma unroll
          for (int a = 0; a < 6; ++a) acc[21 + a] -= w * (J[a] * e0 + J[6 + a] * e1);
        }
#pragma unroll
        for (int k = 0; k < 27; ++k) sRed[k][t] = acc[k];
        tree_reduce(sRed, 27);
      }
      if (t == 0) {
        if (it == 0) {
          // computeLambdaInit: 1e-5 * max |diag(H)|; diagonal entries of the upper layout: 0,6,11,15,18,20
          const int dg[6] = {0, 6, 11, 15, 18, 20};
          double m = 0.0;
          for (int k = 0; k < 6; ++k) m = fmax(m, fabs(sRed[dg[k]][0]));
          sCtl[0] = 1e-5 * m; sCtl[1] = 2.0;
        }
        sCtl[2] = chi_now; sCtl[4] = 0.0; sCtl[5] = 0.0;
      }
      __syncthreads();
      // ---- LM trials ----
      [[maybe_unused]] double last_chi = 0.0;
      while (true) {
        if (t == 0) {
          for (int k = 0; k < 7; ++k) sTbak[k] = sT[k];
          // (H + lambda I) x = b by Cholesky (LinearSolverDense: Eigen LDLT, false when not positive)
          double A[36];
          int q = 0;
          for (int a = 0; a < 6; ++a)
            for (int c = a; c < 6; ++c) { const double v = sRed[q++][0]; A[a * 6 + c] = v; A[c * 6 + a] = v; }
          for (int a = 0; a < 6; ++a) A[a * 6 + a] += sCtl[0];
          bool ok = true;
          for (int j = 0; j < 6 && ok; ++j) {
            double dj = A[j * 6 + j];
            for (int k = 0; k < j; ++k) dj -= A[j * 6 + k] * A[j * 6 + k];
            if (!(dj > 0.0) || !isfinite(dj)) { ok = false; break; }
            dj = sqrt(dj);
            A[j * 6 + j] = dj;
            for (int i = j + 1; i < 6; ++i) {
              double s = A[i * 6 + j];
              for (int k = 0; k < j; ++k) s -= A[i * 6 + k] * A[j * 6 + k];
              A[i * 6 + j] = s / dj;
            }
          }
          double y[6], x[6] = {0, 0, 0, 0, 0, 0};
          if (ok) {
            for (int i = 0; i < 6; ++i) {
              double s = sRed[21 + i][0];
              for (int k = 0; k < i; ++k) s -= A[i * 6 + k] * y[k];
              y[i] = s / A[i * 6 + i];
            }
            for (int i = 5; i >= 0; --i) {
              double s = y[i];
              for (int k = i + 1; k < 6; ++k) s -= A[k * 6 + i] * x[k];
              x[i] = s / A[i * 6 + i];
            }
          }
          for (int k = 0; k < 6; ++k) sX[k] = x[k];
          double T[7], out[7];
          for (int k = 0; k < 7; ++k) T[k] = sT[k];
          ssx::pose_oplus(T, x, out);
          for (int k = 0; k < 7; ++k) sT[k] = out[k];
          sCtl[6] = ok ? 1.0 : 0.0;
        }
        __syncthreads();
        // the H/b in sRed[0..26][0] must survive the chi2 reduction: it only touches row 27
        double tempChi = errors_and_chi2();
        if constexpr (TRACE) last_chi = tempChi;
        if (t == 0) {
          if (sCtl[6] == 0.0) tempChi = 1.7976931348623157e308;
          double rho = sCtl[2] - tempChi;
          double scale = 0.0;
          for (int j = 0; j < 6; ++j) scale += sX[j] * (sCtl[0] * sX[j] + sRed[21 + j][0]);
          scale += 1e-3;
          rho /= scale;
          bool lambda_bad = false;
          if (rho > 0 && isfinite(tempChi)) {
            double alpha = 1. - pow((2 * rho - 1), 3.0);
            alpha = fmin(alpha, 2. / 3.);
            sCtl[0] *= fmax(1. / 3., alpha);
            sCtl[1] = 2.0;
            sCtl[2] = tempChi;
          } else {
            sCtl[0] *= sCtl[1];
            sCtl[1] *= 2.0;
            for (int k = 0; k < 7; ++k) sT[k] = sTbak[k];     // pop(): vertices only, errors stay at the trial state
            if (!isfinite(sCtl[0])) lambda_bad = true;
          }
          sCtl[4] += lambda_bad ? 0.0 : 1.0;
          const double qmax = sCtl[4];
          // do { } while (rho < 0 && qmax < 10);  then Terminate if qmax == 10 || rho == 0 || lambda non-finite
          const bool again = !lambda_bad && (rho < 0) && (qmax < 10.0);
          sCtl[3] = again ? 1.0 : 0.0;
          sCtl[5] = (qmax == 10.0 || rho == 0 || lambda_bad) ? 1.0 : 0.0;
        }
        __syncthreads();
        if (sCtl[3] == 0.0) break;
      }
      if constexpr (TRACE) {
        ++its_run;
        terminated = sCtl[5] != 0.0;
        if (t == 0) {
          const int slot = (round + d.warmup) * d.iters + it;
          tr->chi2[slot] = last_chi; tr->lambda[slot] = sCtl[0]; tr->trials[slot] = (int)sCtl[4];
        }
      }
      if (sCtl[5] != 0.0) break;   // Terminate: optimize() stops iterating
      __syncthreads();
    }
    __syncthreads();
    if constexpr (TRACE) {
      if (t == 0) {
        int* rr = tr->round_rec + 4 * (round + d.warmup);
        rr[0] = n_active; rr[1] = its_run; rr[2] = terminated ? 1 : 0; rr[3] = -1;
      }
    }
    if (round < 0) continue;
    // frontend.cpp:243-268: recompute the error only for features flagged outlier, classify, set levels
    {
      double T[7];
      for (int k = 0; k < 7; ++k) T[k] = sT[k];
      int co = 0;
      for (int i = t; i < d.M; i += PT) {
        if (d.outlier[i]) {
          double e[2], pc[3];
          po_error(T, d, i, e, pc);
          d.err[2 * i] = e[0]; d.err[2 * i + 1] = e[1];
        }
        const double c2 = d.err[2 * i] * d.err[2 * i] + d.err[2 * i + 1] * d.err[2 * i + 1];
        if (c2 > d.chi2_th) { d.outlier[i] = 1; d.level[i] = 1; ++co; }
        else { d.outlier[i] = 0; d.level[i] = 0; }
      }
      sRed[0][t] = (double)co;
      tree_reduce(sRed, 1);
      cnt_outliers = (int)sRed[0][0];
      __syncthreads();
      if constexpr (TRACE) {
        if (t == 0) tr->round_rec[4 * (round + d.warmup) + 3] = cnt_outliers;
      }
      if (t == 0 && round == d.rounds - 2) sUseKernel = 0;   // e->setRobustKernel(nullptr)
      __syncthreads();
    }
  }
  if (t < 7) d.pose_out[t] = sT[t];
  if (t == 0) *d.n_inliers = d.M - cnt_outliers;
}

// TR: empty for the shipped kernel -- its parameters and its code are what they were before the record existed --, PoTrace for the
// traced instantiation of the test hook
template <class... TR>
__global__ __launch_bounds__(PT) void k_pose_only_generic(PoDev d, TR... trace)
{
  pose_only_generic_block<(sizeof...(TR) > 0)>(d, po_trace_of(trace...));
}

// the same for every problem of a table the device can read (blockIdx.x = problem): the generic jobs of ssx_pnp_pose_batch in one launch
__global__ __launch_bounds__(PT) void k_pose_only_generic_jobs(const PoDev* dv)
{
  const PoDev d = dv[blockIdx.x];
  pose_only_generic_block<false>(d, nullptr);
}

// ---- register-resident variant ------------------------------------------------------------------------------------
constexpr int NW = PT / 64;

// lane exchange inside a row of 16 lanes on the VALU (DPP) -- a shuffle through the LDS crossbar costs ~100 cycles of
// latency per step, and the 27-value reduction below is on the critical path of every LM iteration
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)
{
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double read_lane_f64(double v, int lane)
{
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
// sum over the 64 lanes, the same value in every lane
__device__ __forceinline__ double wave_sum_f64(double v)
{
  v += dpp_f64<0xB1>(v);     // quad_perm [1,0,3,2]: lane ^ 1
  v += dpp_f64<0x4E>(v);     // quad_perm [2,3,0,1]: lane ^ 2
  v += dpp_f64<0x141>(v);    // row_half_mirror: the other quad of the 8-lane half
  v += dpp_f64<0x140>(v);    // row_mirror: the other half of the 16-lane row
  return (read_lane_f64(v, 0) + read_lane_f64(v, 16)) + (read_lane_f64(v, 32) + read_lane_f64(v, 48));
}

// sum of N values per thread over the workgroup, returned to every thread.  buf alternates between calls, so a single
// barrier per call is enough: a thread can only reach the next call on the same buffer after every thread has passed
// the barrier of the call in between, i.e. has finished reading.
template <int N>
__device__ __forceinline__ void block_sum(double* v, double (*sPart)[NRED][NW], int& buf)
{
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_sum_f64(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) sPart[buf][k][wave] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double s = sPart[buf][k][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += sPart[buf][k][w];
    v[k] = s;
  }
  buf ^= 1;
}

// The 27 sums of a linearisation (upper H + b).  A butterfly over all lanes costs ~30 instructions per value on the
// critical path; here every thread drops its 27 values into LDS ([value][thread], conflict-free), thread (value k,
// part p) of the first 216 adds 32 of them (reads rotated by the lane so a wave touches every bank pair at most
// twice), 3 DPP steps fold the 8 parts, and every thread reads the 27 totals back: ~130 instructions, two barriers.
// sT is private to this function (the alternating buffers of block_sum are not touched).
__device__ __forceinline__ void block_sum27(double* v, double (*sT)[PT], double* sTot)
{
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 27; ++k) sT[k][t] = v[k];
  __syncthreads();
  if (t < 27 * 8) {
    const int k = t >> 3, part = t & 7;
    const double* row = &sT[k][part * 32];
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int j = 0; j < 32; j += 2) {
      s0 += row[(j + t) & 31];
      s1 += row[(j + 1 + t) & 31];
    }
    double s = s0 + s1;
    s += dpp_f64<0xB1>(s);
    s += dpp_f64<0x4E>(s);
    s += dpp_f64<0x141>(s);
    if (part == 0) sTot[k] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 27; ++k) v[k] = sTot[k];
}

// 1 / sqrt(d): v_rsq_f64 + two Newton steps instead of an IEEE sqrt followed by an IEEE divide (~45 dependent
// instructions -> 9) on the serial pivot chain
__device__ __forceinline__ double rsqrt_nr(double d)
{
  double y = __builtin_amdgcn_rsq(d);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double e = fma(-(d * y), y, 1.0);
    y = fma(0.5 * y, e, y);
  }
  return y;
}

// (H + lambda I) x = b for the upper-triangular H[21] by Cholesky, fully unrolled; false when a pivot is not positive
// (LinearSolverDense: Eigen's LDLT reports failure the same way)
__device__ __forceinline__ bool solve6(const double* Hb, double lambda, double* x)
{
  double A[6][6];
  int q = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int c = a; c < 6; ++c) { A[c][a] = Hb[q]; ++q; }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) A[a][a] += lambda;
  bool ok = true;
  double rd[6];                                              // 1 / L[j][j]
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double dj = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) dj -= A[j][k] * A[j][k];
    if (!(dj > 0.0) || !isfinite(dj)) { ok = false; dj = 1.0; }
    const double inv = rsqrt_nr(dj);
    rd[j] = inv;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double sum = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) sum -= A[i][k] * A[j][k];
      A[i][j] = sum * inv;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double sum = Hb[21 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) sum -= A[i][k] * y[k];
    y[i] = sum * rd[i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double sum = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) sum -= A[k][i] * x[k];
    x[i] = sum * rd[i];
  }
  if (!ok) {
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = 0.0;
  }
  return ok;
}

// dv: one descriptor per problem of the batch (blockIdx.x = problem); ssx_pose_only_opt is a batch of one.  The descriptors
// and a problem's inputs live in a pinned host block the kernel reads DIRECTLY (each value once, at the top), its results go
// straight back into that block: one launch and one synchronisation per batch, no copy in either direction.
// TR: as for k_pose_only_generic; a traced launch passes one `const PoTrace*`, the records of its problems
template <int EPT, class... TR>
__global__ __launch_bounds__(PT) void k_pose_only(const PoDev* __restrict__ dv, TR... trace_v)
{
  constexpr bool TRACE = sizeof...(TR) > 0;
  const PoDev d = dv[blockIdx.x];
  if (d.gate && *d.gate == 0) return;
  [[maybe_unused]] const PoTrace* tr = nullptr;
  if constexpr (TRACE) tr = po_trace_at(trace_v..., blockIdx.x);
  __shared__ double sPart[2][NRED][NW];
  __shared__ double sT[27][PT];
  __shared__ double sTot[27];
  const int t = threadIdx.x;
  int buf = 0;
  // this thread's edges: i = t + k * PT
  double X[EPT][3], z[EPT][2], e[EPT][2];
  bool valid[EPT], level[EPT], outl[EPT];
#pragma unroll
  for (int k = 0; k < EPT; ++k) {
    const int i = t + k * PT;
    valid[k] = i < d.M;
    level[k] = false; outl[k] = false;
    e[k][0] = 0.0; e[k][1] = 0.0;
    const int ii = valid[k] ? i : 0;
    X[k][0] = d.xyz[3 * ii]; X[k][1] = d.xyz[3 * ii + 1]; X[k][2] = d.xyz[3 * ii + 2];
    z[k][0] = d.uv[2 * ii]; z[k][1] = d.uv[2 * ii + 1];
  }
  double T[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) T[k] = d.pose[k];
  bool use_kernel = true;
  const ssx::Cam K = d.K;
  const double delta = d.huber_delta;

  // errors of the active (level 0) edges at pose T + their robust chi2, summed over the workgroup
  auto errors_and_chi2 = [&]() {
    double chi = 0.0;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      double pc[3];
      ssx::se3_act(T, X[k], pc);
      const double hx = K.fx * pc[0] + K.cx * pc[2], hy = K.fy * pc[1] + K.cy * pc[2];
      const double e0 = z[k][0] - hx / pc[2], e1 = z[k][1] - hy / pc[2];
      const bool act = valid[k] && !level[k];
      e[k][0] = act ? e0 : e[k][0];
      e[k][1] = act ? e1 : e[k][1];
      const double c2 = e0 * e0 + e1 * e1;
      double r0 = c2, w = 1.0;
      if (use_kernel) ssx::huber(c2, delta, r0, w);
      chi += act ? r0 : 0.0;
    }
    block_sum<1>(&chi, sPart, buf);
    return chi;
  };

  int cnt_outliers = 0;
  for (int round = -d.warmup; round < d.rounds; ++round) {   // round < 0: a warm-up pass
    double na = 0.0;
#pragma unroll
    for (int k = 0; k < EPT; ++k) na += (valid[k] && !level[k]) ? 1.0 : 0.0;
    block_sum<1>(&na, sPart, buf);
    const bool any_active = na > 0.0;                       // initializeOptimization(0): only level-0 edges are active
    double lambda = 0.0, ni = 2.0, current_chi = 0.0;
    [[maybe_unused]] int its_run = 0;
    [[maybe_unused]] bool terminated = false;
    for (int it = 0; it < d.iters && any_active; ++it) {
      // solve() starts with computeActiveErrors() + activeRobustChi2(); after an accepted trial (the only way to get
      // here with it > 0) the errors and the chi2 of that trial ARE those values -- no second pass over the edges
      if (it == 0) current_chi = errors_and_chi2();
      // ---- linearise: H (upper 21) and b (6) ----
      double Hb[27];
#pragma unroll
      for (int k = 0; k < 27; ++k) Hb[k] = 0.0;
#pragma unroll
      for (int k = 0; k < EPT; ++k) {
        double pc[3];
        ssx::se3_act(T, X[k], pc);
        const double Xc = pc[0], Yc = pc[1], Zc = pc[2];
        const double Zinv = 1.0 / (Zc + 1e-18), Zinv2 = Zinv * Zinv;
        // EdgeProjectionPoseOnly::linearizeOplus, g2otypes.hpp:86-101
        const double J[12] = {-K.fx * Zinv, 0, K.fx * Xc * Zinv2, K.fx * Xc * Yc * Zinv2, -K.fx - K.fx * Xc * Xc * Zinv2, K.fx * Yc * Zinv,
                              0, -K.fy * Zinv, K.fy * Yc * Zinv2, K.fy + K.fy * Yc * Yc * Zinv2, -K.fy * Xc * Yc * Zinv2, -K.fy * Xc * Zinv};
        const double e0 = e[k][0], e1 = e[k][1];
        double r0, w = 1.0;
        if (use_kernel) ssx::huber(e0 * e0 + e1 * e1, delta, r0, w);
        w = (valid[k] && !level[k]) ? w : 0.0;
        int q = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
          for (int c = a; c < 6; ++c) { Hb[q] += J[a] * w * J[c] + J[6 + a] * w * J[6 + c]; ++q; }
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) Hb[21 + a] -= w * (J[a] * e0 + J[6 + a] * e1);
      }
      block_sum27(Hb, sT, sTot);
      if (it == 0) {
        // computeLambdaInit: 1e-5 * max |diag(H)|; diagonal entries of the upper layout: 0,6,11,15,18,20
        const double m = fmax(fmax(fmax(fabs(Hb[0]), fabs(Hb[6])), fmax(fabs(Hb[11]), fabs(Hb[15]))), fmax(fabs(Hb[18]), fabs(Hb[20])));
        lambda = 1e-5 * m; ni = 2.0;
      }
      // ---- LM trials ----
      int qmax = 0;
      bool stop = false;
      [[maybe_unused]] double last_chi = 0.0;
      while (true) {
        double Tbak[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) Tbak[k] = T[k];
        double x[6];
        const bool ok = solve6(Hb, lambda, x);
        double Tn[7];
        ssx::pose_oplus(T, x, Tn);
#pragma unroll
        for (int k = 0; k < 7; ++k) T[k] = Tn[k];
        double temp_chi = errors_and_chi2();
        if constexpr (TRACE) last_chi = temp_chi;
        if (!ok) temp_chi = 1.7976931348623157e308;
        double scale = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) scale += x[j] * (lambda * x[j] + Hb[21 + j]);
        scale += 1e-3;
        const double rho = (current_chi - temp_chi) / scale;
        bool lambda_bad = false;
        if (rho > 0 && isfinite(temp_chi)) {
          const double c = 2 * rho - 1;
          double alpha = 1. - c * c * c;
          alpha = fmin(alpha, 2. / 3.);
          lambda *= fmax(1. / 3., alpha);
          ni = 2.0;
          current_chi = temp_chi;
        } else {
          lambda *= ni;
          ni *= 2.0;
#pragma unroll
          for (int k = 0; k < 7; ++k) T[k] = Tbak[k];          // pop(): vertices only, errors stay at the trial state
          if (!isfinite(lambda)) lambda_bad = true;
        }
        qmax += lambda_bad ? 0 : 1;
        // do { } while (rho < 0 && qmax < 10);  then Terminate if qmax == 10 || rho == 0 || lambda non-finite
        stop = (qmax == 10 || rho == 0 || lambda_bad);
        if (!(!lambda_bad && rho < 0 && qmax < 10)) break;
      }
      if constexpr (TRACE) {
        ++its_run;
        terminated = stop;
        if (t == 0) {
          const int slot = (round + d.warmup) * d.iters + it;
          tr->chi2[slot] = last_chi; tr->lambda[slot] = lambda; tr->trials[slot] = qmax;
        }
      }
      if (stop) break;                                         // Terminate: optimize() stops iterating
    }
    if constexpr (TRACE) {
      if (t == 0) {
        int* rr = tr->round_rec + 4 * (round + d.warmup);
        rr[0] = (int)na; rr[1] = its_run; rr[2] = terminated ? 1 : 0; rr[3] = -1;
      }
    }
    if (round < 0) continue;
    // frontend.cpp:243-268: recompute the error only for features flagged outlier, classify, set levels
    double co = 0.0;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      if (outl[k]) {
        double pc[3];
        ssx::se3_act(T, X[k], pc);
        const double hx = K.fx * pc[0] + K.cx * pc[2], hy = K.fy * pc[1] + K.cy * pc[2];
        e[k][0] = z[k][0] - hx / pc[2]; e[k][1] = z[k][1] - hy / pc[2];
      }
      const double c2 = e[k][0] * e[k][0] + e[k][1] * e[k][1];
      const bool out = valid[k] && c2 > d.chi2_th;
      outl[k] = out; level[k] = out;
      co += out ? 1.0 : 0.0;
    }
    block_sum<1>(&co, sPart, buf);
    cnt_outliers = (int)co;
    if constexpr (TRACE) {
      if (t == 0) tr->round_rec[4 * (round + d.warmup) + 3] = cnt_outliers;
    }
    if (round == d.rounds - 2) use_kernel = false;             // e->setRobustKernel(nullptr)
  }
#pragma unroll
  for (int k = 0; k < EPT; ++k)
    if (valid[k]) d.outlier[t + k * PT] = outl[k] ? 1 : 0;
  if (t < 7) d.pose_out[t] = T[t];
  if (t == 0) *d.n_inliers = d.M - cnt_outliers;
}

}  // namespace

namespace {

// The only launches of the three kernels: n problems of class cls (po_class) whose descriptors start at dv -- memory the device reads
// for the register classes, one descriptor handed over by value for the generic kernel.  tv: the records of a traced launch (test
// hook), null for the shipped kernels, which alone are profiled.
void po_launch(ssx_ctx* ctx, int cls, unsigned n, const PoDev* dv, const PoTrace* tv)
{
  const dim3 grid(n), block(PT);
  if (cls == 2) {
#ifndef SSX_NO_TEST_HOOKS
    if (tv) hipLaunchKernelGGL((k_pose_only_generic<PoTrace>), grid, block, 0, ctx->stream, *dv, *tv);
    else
#endif
    SSX_PROF(ctx, KID_POSE_ONLY, hipLaunchKernelGGL(k_pose_only_generic<>, grid, block, 0, ctx->stream, *dv));
    return;
  }
  if (!tv) {
    if (cls == 0) SSX_PROF(ctx, KID_POSE_ONLY, hipLaunchKernelGGL(k_pose_only<2>, grid, block, 0, ctx->stream, dv));
    else SSX_PROF(ctx, KID_POSE_ONLY, hipLaunchKernelGGL(k_pose_only<6>, grid, block, 0, ctx->stream, dv));
    return;
  }
#ifndef SSX_NO_TEST_HOOKS
  if (cls == 0) hipLaunchKernelGGL((k_pose_only<2, const PoTrace*>), grid, block, 0, ctx->stream, dv, tv);
  else hipLaunchKernelGGL((k_pose_only<6, const PoTrace*>), grid, block, 0, ctx->stream, dv, tv);
#endif
}

// A batch as a plain value.  The jobs of the register classes share ONE pinned block, which the kernels read and write in place (no
// copy in either direction):  [descriptors: class 0 first, then class 1, job order inside a class | the problem of each, in that
// order | the record table of a traced batch (nothing for the entry points: their block is not enlarged for the hook)].
// The generic jobs follow one by one, in job order (pose_only_generic); an empty job is in neither list.
struct PoBatchPlan {
  struct Job { int job; PoProblem p; };
  struct Launch { int cls; unsigned grid; size_t first; };
  std::vector<Job> reg;
  size_t n2 = 0;                // the first n2 of reg are of class 0
  std::vector<int> generic;
  bool traced = false;
  PoDev* dv = nullptr;
  PoTrace* tv = nullptr;
  template <class F> void each(F&& f)
  {
    f(dv, sizeof(PoDev) * reg.size());
    for (Job& j : reg) j.p.each(f);
    f(tv, traced ? sizeof(PoTrace) * reg.size() : 0);
  }
  // at most two launches over the block's descriptors
  int launches(Launch* out) const
  {
    int k = 0;
    if (n2) out[k++] = Launch{0, (unsigned)n2, 0};
    if (reg.size() > n2) out[k++] = Launch{1, (unsigned)(reg.size() - n2), n2};
    return k;
  }
};

template <class MOf> PoBatchPlan po_plan_batch(int n, MOf&& M_of, bool traced)
{
  PoBatchPlan pl;
  pl.traced = traced;
  pl.reg.reserve((size_t)n);
  for (int c = 0; c < 3; ++c) {
    for (int j = 0; j < n; ++j) {
      const int M = M_of(j);
      if (M == 0 || po_class(M) != c) continue;
      if (c < 2) pl.reg.push_back({j, PoProblem{M}}); else pl.generic.push_back(j);
    }
    if (c == 0) pl.n2 = pl.reg.size();
  }
  return pl;
}

bool po_job_ok(const ssx_pose_only_job& q)
{
  return q.pose_io && q.K4 && q.M >= 0 && (q.M == 0 || (q.xyz && q.uv)) && q.rounds >= 0 && q.iters >= 0;
}

// the generic kernel (M > 6 x 256 edges: never a front-end's frame) keeps its edges in device memory, one problem per call: the
// block in the arena and its mirror in the pinned block, the inputs sent up in one copy, the result brought back in one
// (warmup, tr: the test hook's -- 0 and nullptr from the entry points; tr's pointers are memory the device can write)
ssx_status pose_only_generic(ssx_ctx* ctx, const ssx_pose_only_job& q, int32_t warmup, const PoTrace* tr)
{
  PoProblem dev{q.M}, host{q.M};
  const size_t bytes = carve(nullptr, [&](auto&& f) { dev.each(f); });
  SSX_HIP_TRY(ctx, ctx->po_arena.reserve(bytes));
  SSX_HIP_TRY(ctx, ctx->po_stage.reserve(bytes));
  char* hs = ctx->po_stage.as<char>();
  carve(ctx->po_arena.as<char>(), [&](auto&& f) { dev.each(f); });
  carve(hs, [&](auto&& f) { host.each(f); });
  host.stage(q.xyz, q.uv, q.pose_io);
  SSX_HIP_TRY(ctx, hipMemcpyAsync(ctx->po_arena.p, hs, (size_t)(host.sent() - hs), hipMemcpyHostToDevice, ctx->stream));
  PoDev d;
  po_set_scalars(d, q.M, warmup, q.rounds, q.iters, q.chi2_th, q.huber_delta, q.K4, nullptr);
  dev.wire(d);
  po_launch(ctx, 2, 1, &d, tr);
  SSX_HIP_TRY(ctx, hipGetLastError());
  SSX_HIP_TRY(ctx, hipMemcpyAsync(host.res, dev.res, host.result_bytes(), hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  po_read_result(host.res, q.M, q.pose_io, q.inlier_out, q.n_inliers);
  return SSX_OK;
}

// the batch behind ssx_pose_only_opt_batch (warmup = 0, trace = nullptr) and behind the test hook (trace[j]: the record of job j).
// Register classes: no copy, at most two launches, one synchronisation; then each generic job with its own upload, launch, download
// and synchronisation.
ssx_status po_batch(ssx_ctx* ctx, int32_t n, const ssx_pose_only_job* jobs, int32_t warmup, const PoTrace* trace)
{
  if (!ctx || n < 0 || (n > 0 && !jobs)) return SSX_ERR_INVALID_ARG;
  for (int j = 0; j < n; ++j)
    if (!po_job_ok(jobs[j])) return SSX_ERR_INVALID_ARG;
  if (n == 0) return SSX_OK;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (int j = 0; j < n; ++j)
    if (jobs[j].M == 0 && jobs[j].n_inliers) *jobs[j].n_inliers = 0;      // (an empty job: no inliers, the pose as it came)
  PoBatchPlan pl = po_plan_batch(n, [&](int j) { return jobs[j].M; }, trace != nullptr);
  if (!pl.reg.empty()) {
    SSX_HIP_TRY(ctx, ctx->po_stage.reserve(carve(nullptr, [&](auto&& f) { pl.each(f); }), 2.0));
    carve(ctx->po_stage.as<char>(), [&](auto&& f) { pl.each(f); });
    for (size_t k = 0; k < pl.reg.size(); ++k) {
      const ssx_pose_only_job& q = jobs[pl.reg[k].job];
      const PoProblem& p = pl.reg[k].p;
      p.stage(q.xyz, q.uv, q.pose_io);
      po_set_scalars(pl.dv[k], q.M, warmup, q.rounds, q.iters, q.chi2_th, q.huber_delta, q.K4, nullptr);
      p.wire(pl.dv[k]);
      if (trace) pl.tv[k] = trace[pl.reg[k].job];
    }
    PoBatchPlan::Launch ls[2];
    for (int i = 0, nl = pl.launches(ls); i < nl; ++i) po_launch(ctx, ls[i].cls, ls[i].grid, pl.dv + ls[i].first, trace ? pl.tv + ls[i].first : nullptr);
    SSX_HIP_TRY(ctx, hipGetLastError());
    SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (const PoBatchPlan::Job& j : pl.reg) po_read_result(j.p.res, j.p.M, jobs[j.job].pose_io, jobs[j.job].inlier_out, jobs[j.job].n_inliers);
  }
  for (int j : pl.generic) {
    const ssx_status st = pose_only_generic(ctx, jobs[j], warmup, trace ? trace + j : nullptr);
    if (st != SSX_OK) return st;
  }
  return SSX_OK;
}

}  // namespace

hipError_t po_launch_device(ssx_ctx* ctx, const PoDev* d)
{
  po_launch(ctx, po_class(d->M), 1, d, nullptr);
  return hipGetLastError();
}

hipError_t po_launch_device_table(ssx_ctx* ctx, int cls, unsigned n, const PoDev* dv)
{
  if (cls == 2) SSX_PROF(ctx, KID_POSE_ONLY, hipLaunchKernelGGL(k_pose_only_generic_jobs, dim3(n), dim3(PT), 0, ctx->stream, dv));
  else po_launch(ctx, cls, n, dv, nullptr);
  return hipGetLastError();
}

// n problems in one call (one frame of each of n streams: FrontEnd::EstimateCurrentPose, frontend.cpp:184-300): one workgroup per
// problem, ONE launch per register class of the kernel.  Per problem the bits of ssx_pose_only_opt (which is a batch of one).
extern "C" ssx_status ssx_pose_only_opt_batch(ssx_ctx* ctx, int32_t n, const ssx_pose_only_job* jobs)
{
  return po_batch(ctx, n, jobs, 0, nullptr);
}

extern "C" ssx_status ssx_pose_only_opt(ssx_ctx* ctx, double* pose_io, const double* K4, int32_t M, const double* xyz,
                                        const double* uv, int32_t rounds, int32_t iters, double chi2_th, double huber_delta,
                                        uint8_t* inlier_out, int32_t* n_inliers)
{
  ssx_pose_only_job q;
  q.pose_io = pose_io; q.K4 = K4; q.M = M; q.xyz = xyz; q.uv = uv; q.rounds = rounds; q.iters = iters; q.chi2_th = chi2_th; q.huber_delta = huber_delta;
  q.inlier_out = inlier_out; q.n_inliers = n_inliers;
  return po_batch(ctx, 1, &q, 0, nullptr);
}

#ifndef SSX_NO_TEST_HOOKS   // include/ssx_test_hooks.h
// The record lives in one pinned block of this call's own (the kernels write it in place, as they write their results), laid out job
// after job: (warmup + rounds) * iters slots of chi2, lambda and trials, (warmup + rounds) * 4 ints per job.
extern "C" ssx_status ssx_pose_only_debug_trace(ssx_ctx* ctx, int32_t n, const ssx_pose_only_job* jobs, int32_t warmup, double* it_chi2,
                                                double* it_lambda, int32_t* it_trials, int32_t* round_rec)
{
  if (!ctx || n < 0 || (n > 0 && !jobs) || warmup < 0 || !it_chi2 || !it_lambda || !it_trials || !round_rec) return SSX_ERR_INVALID_ARG;
  size_t n_it = 0, n_rd = 0;
  for (int j = 0; j < n; ++j) {
    if (jobs[j].rounds < 0 || jobs[j].iters < 0) return SSX_ERR_INVALID_ARG;
    n_it += (size_t)(warmup + jobs[j].rounds) * (size_t)jobs[j].iters;
    n_rd += (size_t)(warmup + jobs[j].rounds);
  }
  if (n == 0) return SSX_OK;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  PoTrace all;                                                              // the four arrays, all jobs
  auto arrays = [&](auto&& f) { f(all.chi2, sizeof(double) * n_it); f(all.lambda, sizeof(double) * n_it); f(all.trials, sizeof(int) * n_it); f(all.round_rec, sizeof(int) * 4 * n_rd); };
  const size_t bytes = carve(nullptr, arrays);
  HostBuf rec;
  hipError_t e = rec.reserve(bytes + 256);
  if (e != hipSuccess) { SSX_HIP_TRY(ctx, e); }
  memset(rec.p, 0, bytes);
  carve(rec.as<char>(), arrays);
  std::vector<PoTrace> tv((size_t)n);
  size_t k_it = 0, k_rd = 0;
  for (int j = 0; j < n; ++j) {
    tv[j] = PoTrace{all.chi2 + k_it, all.lambda + k_it, all.trials + k_it, all.round_rec + 4 * k_rd};
    k_it += (size_t)(warmup + jobs[j].rounds) * (size_t)jobs[j].iters;
    k_rd += (size_t)(warmup + jobs[j].rounds);
  }
  const ssx_status st = po_batch(ctx, n, jobs, warmup, tv.data());        // (synchronises the stream before it returns)
  if (st == SSX_OK) {
    memcpy(it_chi2, all.chi2, sizeof(double) * n_it); memcpy(it_lambda, all.lambda, sizeof(double) * n_it);
    memcpy(it_trials, all.trials, sizeof(int) * n_it); memcpy(round_rec, all.round_rec, sizeof(int) * 4 * n_rd);
  }
  rec.release();
  return st;
}

// what po_batch would do with jobs of M[0 .. n) edges, and what plan_pnp (pnp.hip) makes of (pnp_M, pnp_H, pnp_tap); no device
extern "C" ssx_status ssx_po_debug_plan(int32_t n, const int32_t* M, int32_t traced, ssx_po_plan_info* out, int32_t pnp_M, int32_t pnp_H,
                                        int32_t pnp_tap, ssx_pnp_plan_info* pnp_out)
{
  if (out) {
    if (n < 0 || n > SSX_PO_MAX_INFO_JOBS || (n > 0 && !M)) return SSX_ERR_INVALID_ARG;
    for (int j = 0; j < n; ++j)
      if (M[j] < 0) return SSX_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    out->n_jobs = n;
    for (int j = 0; j < n; ++j) { out->job[j].cls = M[j] ? po_class(M[j]) : 3; out->job[j].block = -1; }
    PoBatchPlan pl = po_plan_batch(n, [&](int j) { return M[j]; }, traced != 0);
    // (carved from a null base, a plan's pointers are its offsets)
    auto spans = [&](PoProblem& p, int job) {
      int k = 0;
      p.each([&](auto*& ptr, size_t bytes) { out->job[job].span_off[k] = reinterpret_cast<uintptr_t>(ptr); out->job[job].span_bytes[k] = bytes; ++k; });
      out->job[job].block = out->n_blocks;
    };
    if (!pl.reg.empty()) {
      auto& b = out->block[out->n_blocks];
      b.bytes = carve(nullptr, [&](auto&& f) { pl.each(f); });
      b.desc_off = reinterpret_cast<uintptr_t>(pl.dv); b.desc_bytes = sizeof(PoDev) * pl.reg.size();
      b.trace_off = reinterpret_cast<uintptr_t>(pl.tv); b.trace_bytes = pl.traced ? sizeof(PoTrace) * pl.reg.size() : 0;
      for (PoBatchPlan::Job& j : pl.reg) spans(j.p, j.job);
      PoBatchPlan::Launch ls[2];
      for (int i = 0, nl = pl.launches(ls); i < nl; ++i) {
        auto& l = out->launch[out->n_launches++];
        l.cls = ls[i].cls; l.grid = (int32_t)ls[i].grid; l.block = out->n_blocks; l.first_desc = (int32_t)ls[i].first;
      }
      ++out->n_blocks;
    }
    for (int j : pl.generic) {
      PoProblem p{M[j]};
      auto& b = out->block[out->n_blocks];
      b.bytes = carve(nullptr, [&](auto&& f) { p.each(f); });
      b.sent = reinterpret_cast<uintptr_t>(p.sent()); b.ret_off = reinterpret_cast<uintptr_t>(p.res); b.ret_bytes = p.result_bytes();
      spans(p, j);
      auto& l = out->launch[out->n_launches++];
      l.cls = 2; l.grid = 1; l.block = out->n_blocks; l.first_desc = -1;
      ++out->n_blocks;
    }
  }
  if (pnp_out) {
    if (pnp_M < 0 || pnp_H < 0) return SSX_ERR_INVALID_ARG;
    pnp_describe_plan(pnp_M, pnp_H, pnp_tap != 0, pnp_out);
  }
  return SSX_OK;
}
#endif  // SSX_NO_TEST_HOOKS
