// ssvio_amd/csrc/pnp.hip -- the pose correction of loop closing: P3P-RANSAC and its refinement, on the device.
//
// LoopClosing::ComputeCorrectPose (src/ssvio/loopclosing.cpp:147-243) hands the matched (map point of the loop keyframe, pixel of the
// current keyframe) pairs to cv::solvePnPRansac(..., 100 iterations, 5.991 px, 0.99), takes ONLY the pose from it (never the inliers)
// and refines that pose over all pairs in OptimizeCurrentPose (:245-351).  OpenCV's sampler and sequential early exit cannot be
// restated to the bit, so the RANSAC here is a contract of its own, stated once more in tools/pnp_model.py; the refinement is g2o's,
// which pose_only.hip already restates (one warm-up pass, then the four classified rounds).
//
// k_pnp_ransac   one wavefront per hypothesis, four per workgroup.  Hypothesis h samples three distinct points as a pure function of
//                (seed, h, M) -- a counter-based mixer, multiply-high draws from [0, M), [0, M-1), [0, M-2), each lifted past the earlier
//                picks -- so the result does not depend on the launch.  Every lane solves the P3P of the triple (up to four poses; the
//                solver is described in tools/pnp_model.py and uses + - * / sqrt only, with fixed numbers of Newton steps), then the
//                lanes stride over the M points per solution: inlier = positive depth and ex^2 + ey^2 <= thr^2 (thr in PIXELS: the
//                reference passes its chi-square constant as OpenCV's pixel threshold), counted by ballot + popcount.  A degenerate
//                triple yields no solution and scores 0: validity is decided by finiteness tests, no NaN reaches a comparison, and a
//                solution is handed on only if it satisfies the three quadrics (kResidCut) and spans a triangle of the area of the
//                points' (kAreaCut: the sides of a needle hold to rounding while R is stretched along its normal) -- both cut-offs are
//                stated against the 60-digit reference tests/golden/p3p_hp.npz in tools/pnp_model.py.  Two plane pairs for D1 and D2
//                (both determinants 0: an equilateral triangle on the axis) need no cubic: g = 0.
//                ALL max_iters hypotheses are scored: the confidence-driven early exit of OpenCV's loop is a sequential notion, a
//                launch has no use for it.
//                Selection: max over (count << 32) | ~(4 h + s) -- the most inliers, then the lowest hypothesis, then the lowest
//                solution, what a sequential loop with `>` keeps -- folded through LDS, one 64-bit atomicMax per workgroup behind a
//                read.  The LAST workgroup to finish (a ticket) solves the winner's triple again and writes its pose
//                (qx qy qz qw tx ty tz, normalised, qw >= 0), its inlier mask and the header: they stay in device memory, where
//                the refinement (k_pose_only*, gated by the header's `found`) picks the pose up.
//
// ssx_pnp_pose_batch (relocalisation: one pose per candidate keyframe) is n of these in one call: k_pnp_ransac_jobs is the same workgroup
// body with the job as blockIdx.y -- a table of PnpDev, each with its own best / ticket words and header -- and the refinement one launch
// per kernel class over a table of descriptors, each gated on its job's header.
//
// This file is compiled with -ffp-contract=off: every operation rounds as the model's does (tests/test_p3p_gpu.py: R, t and the pose of
// every slot of ssx_pnp_debug_p3p are the model's bytes).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "pose_only.hpp"
#include "se3.hpp"
#include "../../include/ssx_test_hooks.h"

namespace {

constexpr int kNewtonSteps = 16;    // on the cubic
constexpr int kGnSteps = 3;         // on the three quadrics
constexpr double kResidCut = 5.9e-9;    // on the three quadrics, relative to l1^2 + l2^2 + l3^2 (tools/pnp_model.py: RESID_CUT)
constexpr double kAreaCut = 1e-6;       // on |q1 x q2|^2 / |p1 x p2|^2 - 1 (AREA_CUT)
constexpr int kMinInliers = 4;      // a hypothesis explains its own three points: a pose needs one more

struct PnpHdr {                     // results of k_pnp_ransac, in device memory
  double pose[7];
  int32_t found, n_inliers, best, pad;
};

struct PnpDev {
  int M, H;
  uint32_t seed;
  double fx, fy, cx, cy, thr2;
  const double* xyz;
  const double* uv;
  unsigned long long* best;         // zero before the launch
  unsigned int* ticket;             // zero before the launch
  PnpHdr* hdr;
  uint8_t* inlier;                  // M
  int32_t* hyp_counts;              // nullable (tap): the best count of each hypothesis
};

__device__ __forceinline__ uint32_t mix32(uint32_t x)
{
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// three distinct indices of [0, M), M >= 3
__device__ __forceinline__ void sample_triple(uint32_t seed, int h, int M, int* tri)
{
  const uint32_t r0 = mix32(seed ^ mix32(3u * (uint32_t)h + 1u)), r1 = mix32(seed ^ mix32(3u * (uint32_t)h + 2u)),
                 r2 = mix32(seed ^ mix32(3u * (uint32_t)h + 3u));
  const int a = (int)(((uint64_t)r0 * (uint32_t)M) >> 32);
  int b = (int)(((uint64_t)r1 * (uint32_t)(M - 1)) >> 32);
  int c = (int)(((uint64_t)r2 * (uint32_t)(M - 2)) >> 32);
  b += b >= a ? 1 : 0;
  const int lo = min(a, b), hi = max(a, b);
  c += c >= lo ? 1 : 0;
  c += c >= hi ? 1 : 0;
  tri[0] = a; tri[1] = b; tri[2] = c;
}

// symmetric 3x3 as (m00 m01 m02 m11 m12 m22)
__device__ __forceinline__ void adj_sym(const double* m, double* o)
{
  o[0] = m[3] * m[5] - m[4] * m[4];
  o[1] = m[2] * m[4] - m[1] * m[5];
  o[2] = m[1] * m[4] - m[2] * m[3];
  o[3] = m[0] * m[5] - m[2] * m[2];
  o[4] = m[1] * m[2] - m[0] * m[4];
  o[5] = m[0] * m[3] - m[1] * m[1];
}
__device__ __forceinline__ double dot_sym(const double* a, const double* b)
{
  return a[0] * b[0] + a[3] * b[3] + a[5] * b[5] + 2.0 * (a[1] * b[1] + a[2] * b[2] + a[4] * b[4]);
}
__device__ __forceinline__ double quad_sym(const double* q, const double* u, const double* v)
{
  return u[0] * (q[0] * v[0] + q[1] * v[1] + q[2] * v[2]) + u[1] * (q[1] * v[0] + q[3] * v[1] + q[4] * v[2]) +
         u[2] * (q[2] * v[0] + q[4] * v[1] + q[5] * v[2]);
}
__device__ __forceinline__ void cross3(const double* a, const double* b, double* o)
{
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// a real root of r^3 + b r^2 + c r + d (finite b, c, d): a start beyond the turning points, from where Newton's iteration is monotone.
// Where an intermediate overflows, that non-finite value is returned before it is compared; the caller tests the result.
__device__ __forceinline__ double cubic_root(double b, double c, double d)
{
  const double disc = b * b - 3.0 * c;
  if (!isfinite(disc)) return disc;
  double r;
  if (disc > 0.0) {
    const double v = sqrt(disc);
    const double t1 = (-b - v) / 3.0;
    double k = ((t1 + b) * t1 + c) * t1 + d;
    if (!isfinite(k)) return k;
    if (k > 0.0) {                                            // the local maximum is above the axis: the root left of it
      r = t1 - sqrt(k / v);
    } else {                                                  // else the root right of the local minimum
      const double t2 = (-b + v) / 3.0;
      k = ((t2 + b) * t2 + c) * t2 + d;
      r = t2 + sqrt(-k / v);
    }
  } else {                                                    // monotone: from the inflection
    r = -b / 3.0;
    if (fabs((3.0 * r + 2.0 * b) * r + c) < 1e-4) r = r + 1.0;
  }
  for (int it = 0; it < kNewtonSteps; ++it) {
    const double fx = ((r + b) * r + c) * r + d;
    const double fp = (3.0 * r + 2.0 * b) * r + c;
    r = r - fx / fp;
  }
  return r;
}

__device__ __forceinline__ bool fin3(const double* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

struct P3P {
  bool valid[4];
  double R[4][9], t[4][3];          // solution 2 p + r is root r of plane p
};

// the P3P of points X[3][3] seen at pixels z[3][2]; tools/pnp_model.py::_p3p, line by line
__device__ __forceinline__ void p3p_solve(const PnpDev& d, const double (*X)[3], const double (*z)[2], P3P& out)
{
#pragma unroll
  for (int k = 0; k < 4; ++k) out.valid[k] = false;
  double y[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double bx = (z[i][0] - d.cx) / d.fx, by = (z[i][1] - d.cy) / d.fy;
    const double n = sqrt(bx * bx + by * by + 1.0);
    y[i][0] = bx / n; y[i][1] = by / n; y[i][2] = 1.0 / n;
  }
  auto d2 = [](const double* p, const double* q) {
    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return dx * dx + dy * dy + dz * dz;
  };
  auto dot = [](const double* p, const double* q) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]; };
  const double A12 = d2(X[0], X[1]), A13 = d2(X[0], X[2]), A23 = d2(X[1], X[2]);
  const double S = A12 + A13 + A23;
  if (!(isfinite(S) && S > 0.0)) return;
  const double a12 = A12 / S, a13 = A13 / S, a23 = A23 / S;
  const double b12 = -2.0 * dot(y[0], y[1]), b13 = -2.0 * dot(y[0], y[2]), b23 = -2.0 * dot(y[1], y[2]);
  const double h12 = 0.5 * b12, h13 = 0.5 * b13, h23 = 0.5 * b23;
  const double D1[6] = {a23, a23 * h12, 0.0, a23 - a12, -(a12 * h23), -a12};
  const double D2[6] = {a23, 0.0, a23 * h13, -a13, -(a13 * h23), a23 - a13};
  double J1[6], J2[6];
  adj_sym(D1, J1);
  adj_sym(D2, J2);
  const double det1 = D1[0] * J1[0] + D1[1] * J1[1] + D1[2] * J1[2];
  const double det2 = D2[0] * J2[0] + D2[1] * J2[1] + D2[2] * J2[2];
  if (!(isfinite(det1) && isfinite(det2))) return;
  const bool keep = fabs(det2) >= fabs(det1);                 // the cubic is made monic by the larger determinant
  double Da[6], Db[6], Ja[6], Jb[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    Da[k] = keep ? D1[k] : D2[k]; Db[k] = keep ? D2[k] : D1[k];
    Ja[k] = keep ? J1[k] : J2[k]; Jb[k] = keep ? J2[k] : J1[k];
  }
  const double deta = keep ? det1 : det2, detb = keep ? det2 : det1;
  double g = 0.0;                                             // detb = 0, hence deta = 0: Da is a plane pair itself (a12 = a23 and b12 = b23, say)
  if (fabs(detb) > 0.0) {
    const double cb = dot_sym(Da, Jb) / detb, cc = dot_sym(Ja, Db) / detb, cd = deta / detb;   // (a tiny detb can make them infinite)
    if (!(isfinite(cb) && isfinite(cc) && isfinite(cd))) return;
    g = cubic_root(cb, cc, cd);
    if (!isfinite(g)) return;
  }
  double C[6], Q[6];
  const bool q_b = fabs(g) <= 1.0;                            // on the planes Da = -g Db: the one that is not small there
#pragma unroll
  for (int k = 0; k < 6; ++k) { C[k] = Da[k] + g * Db[k]; Q[k] = q_b ? Db[k] : Da[k]; }
  // C = l m' + m l' with p = l x m: -adj(C) = p p', and C + [p]x = 2 m l'
  double Jc[6], B[6];
  adj_sym(C, Jc);
#pragma unroll
  for (int k = 0; k < 6; ++k) B[k] = -Jc[k];
  if (!(fin3(B) && fin3(B + 3))) return;
  double bii, p[3];
  if (B[0] >= B[3] && B[0] >= B[5]) { bii = B[0]; p[0] = B[0]; p[1] = B[1]; p[2] = B[2]; }
  else if (B[3] >= B[5]) { bii = B[3]; p[0] = B[1]; p[1] = B[3]; p[2] = B[4]; }
  else { bii = B[5]; p[0] = B[2]; p[1] = B[4]; p[2] = B[5]; }
  if (!(bii > 0.0)) return;
  const double beta = sqrt(bii);
  p[0] = p[0] / beta; p[1] = p[1] / beta; p[2] = p[2] / beta;
  const double N[3][3] = {{C[0], C[1] - p[2], C[2] + p[1]}, {C[1] + p[2], C[3], C[4] - p[0]}, {C[2] - p[1], C[4] + p[0], C[5]}};
  if (!(fin3(N[0]) && fin3(N[1]) && fin3(N[2]))) return;
  double best = -1.0;
  double row[3] = {0.0, 0.0, 0.0}, col[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (fabs(N[j][k]) > best) {
        best = fabs(N[j][k]);
        row[0] = N[j][0]; row[1] = N[j][1]; row[2] = N[j][2];
        col[0] = N[0][k]; col[1] = N[1][k]; col[2] = N[2][k];
      }
    }
  }
  const double sqS = sqrt(S);
#pragma unroll
  for (int pl = 0; pl < 2; ++pl) {
    const double n[3] = {pl == 0 ? row[0] : col[0], pl == 0 ? row[1] : col[1], pl == 0 ? row[2] : col[2]};
    const double u[3] = {n[1] - n[2], n[2] - n[0], n[0] - n[1]};   // n x (1, 1, 1): never zero for a plane that meets the positive octant
    double v[3];
    cross3(n, u, v);
    const double qa = quad_sym(Q, u, u), qb = quad_sym(Q, u, v), qc = quad_sym(Q, v, v);
    const double disc = qb * qb - qa * qc;
    if (!(isfinite(disc) && disc >= 0.0)) continue;
    const double sq = sqrt(disc);
    const double q = qb >= 0.0 ? -(qb + sq) : -(qb - sq);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const double s = r == 0 ? q : qc, t = r == 0 ? qa : q;     // the two roots (s : t) of qa s^2 + 2 qb s t + qc t^2
      double l1 = s * u[0] + t * v[0], l2 = s * u[1] + t * v[1], l3 = s * u[2] + t * v[2];
      const double w = 2.0 * (l1 * l1 + l2 * l2 + l3 * l3) + b12 * (l1 * l2) + b13 * (l1 * l3) + b23 * (l2 * l3);   // = a12 + a13 + a23 = 1
      if (!(isfinite(w) && w > 0.0)) continue;
      double sc = 1.0 / sqrt(w);
      if (l1 < 0.0) sc = -sc;
      l1 = l1 * sc; l2 = l2 * sc; l3 = l3 * sc;
      for (int it = 0; it < kGnSteps; ++it) {
        const double r0 = l1 * l1 + l2 * l2 + b12 * (l1 * l2) - a12;
        const double r1 = l1 * l1 + l3 * l3 + b13 * (l1 * l3) - a13;
        const double r2 = l2 * l2 + l3 * l3 + b23 * (l2 * l3) - a23;
        const double j00 = 2.0 * l1 + b12 * l2, j01 = 2.0 * l2 + b12 * l1;
        const double j10 = 2.0 * l1 + b13 * l3, j12 = 2.0 * l3 + b13 * l1;
        const double j21 = 2.0 * l2 + b23 * l3, j22 = 2.0 * l3 + b23 * l2;
        const double det = -(j00 * (j12 * j21)) - j01 * (j10 * j22);
        // Cramer for [[j00 j01 0] [j10 0 j12] [0 j21 j22]]
        const double e1 = (r0 * (-(j12 * j21)) - j01 * (r1 * j22 - j12 * r2)) / det;
        const double e2 = (j00 * (r1 * j22 - j12 * r2) - r0 * (j10 * j22)) / det;
        const double e3 = (j00 * (-(r1 * j21)) - j01 * (j10 * r2) + r0 * (j10 * j21)) / det;
        l1 = l1 - e1; l2 = l2 - e2; l3 = l3 - e3;
      }
      if (!(isfinite(l1) && isfinite(l2) && isfinite(l3) && l1 > 0.0 && l2 > 0.0 && l3 > 0.0)) continue;
      {
        // a solution satisfies the three quadrics: where the iteration has not arrived (a plane pair that is none, a multiple root)
        // there is no pose to hand on
        const double r0 = l1 * l1 + l2 * l2 + b12 * (l1 * l2) - a12;
        const double r1 = l1 * l1 + l3 * l3 + b13 * (l1 * l3) - a13;
        const double r2 = l2 * l2 + l3 * l3 + b23 * (l2 * l3) - a23;
        const double cut = kResidCut * (l1 * l1 + l2 * l2 + l3 * l3);
        if (!(isfinite(r0) && isfinite(r1) && isfinite(r2) && isfinite(cut) && fabs(r0) <= cut && fabs(r1) <= cut && fabs(r2) <= cut)) continue;
      }
      l1 = l1 * sqS; l2 = l2 * sqS; l3 = l3 * sqS;
      const double Y[3][3] = {{l1 * y[0][0], l1 * y[0][1], l1 * y[0][2]}, {l2 * y[1][0], l2 * y[1][1], l2 * y[1][2]}, {l3 * y[2][0], l3 * y[2][1], l3 * y[2][2]}};
      const double p1[3] = {X[1][0] - X[0][0], X[1][1] - X[0][1], X[1][2] - X[0][2]};
      const double p2[3] = {X[2][0] - X[0][0], X[2][1] - X[0][1], X[2][2] - X[0][2]};
      const double q1[3] = {Y[1][0] - Y[0][0], Y[1][1] - Y[0][1], Y[1][2] - Y[0][2]};
      const double q2[3] = {Y[2][0] - Y[0][0], Y[2][1] - Y[0][1], Y[2][2] - Y[0][2]};
      double p3[3], q3[3], w1[3], w2[3];
      cross3(p1, p2, p3);
      cross3(q1, q2, q3);
      const double det = p3[0] * p3[0] + p3[1] * p3[1] + p3[2] * p3[2];
      if (!(isfinite(det) && det > 0.0)) continue;
      // ... and spans a triangle congruent to the points': a needle's height is lost in the rounding of its sides, and the frames below
      // would stretch R along the normal by the ratio of the two areas
      const double area = q3[0] * q3[0] + q3[1] * q3[1] + q3[2] * q3[2];
      const double acut = kAreaCut * det;
      if (!(isfinite(area) && isfinite(acut) && fabs(area - det) <= acut)) continue;
      cross3(p2, p3, w1);                                     // rows of the inverse of [p1 p2 p3], times det
      cross3(p3, p1, w2);
      const int k = 2 * pl + r;
      bool ok = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out.R[k][a * 3 + c] = (q1[a] * w1[c] + q2[a] * w2[c] + q3[a] * p3[c]) / det;
        out.t[k][a] = Y[0][a] - (out.R[k][a * 3] * X[0][0] + out.R[k][a * 3 + 1] * X[0][1] + out.R[k][a * 3 + 2] * X[0][2]);
        ok = ok && fin3(&out.R[k][a * 3]) && isfinite(out.t[k][a]);
      }
      out.valid[k] = ok;
    }
  }
}

__device__ __forceinline__ void load_triple(const PnpDev& d, int h, double (*X)[3], double (*z)[2])
{
  int tri[3];
  sample_triple(d.seed, h, d.M, tri);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    X[i][0] = d.xyz[3 * tri[i]]; X[i][1] = d.xyz[3 * tri[i] + 1]; X[i][2] = d.xyz[3 * tri[i] + 2];
    z[i][0] = d.uv[2 * tri[i]]; z[i][1] = d.uv[2 * tri[i] + 1];
  }
}

__device__ __forceinline__ bool is_inlier(const PnpDev& d, const double* R, const double* t, int i)
{
  const double x = d.xyz[3 * i], y = d.xyz[3 * i + 1], z = d.xyz[3 * i + 2];
  const double px = R[0] * x + R[1] * y + R[2] * z + t[0];
  const double py = R[3] * x + R[4] * y + R[5] * z + t[1];
  const double pz = R[6] * x + R[7] * y + R[8] * z + t[2];
  const double ex = d.fx * (px / pz) + d.cx - d.uv[2 * i];
  const double ey = d.fy * (py / pz) + d.cy - d.uv[2 * i + 1];
  const double e2 = ex * ex + ey * ey;
  return isfinite(pz) && pz > 0.0 && isfinite(e2) && e2 <= d.thr2;
}

__device__ __forceinline__ void rot_to_quat(const double* R, double* q)
{
  const double tr = R[0] + R[4] + R[8];
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    q[0] = (R[7] - R[5]) / s; q[1] = (R[2] - R[6]) / s; q[2] = (R[3] - R[1]) / s; q[3] = 0.25 * s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0;
    q[0] = 0.25 * s; q[1] = (R[1] + R[3]) / s; q[2] = (R[2] + R[6]) / s; q[3] = (R[7] - R[5]) / s;
  } else if (R[4] > R[8]) {
    const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0;
    q[0] = (R[1] + R[3]) / s; q[1] = 0.25 * s; q[2] = (R[5] + R[7]) / s; q[3] = (R[2] - R[6]) / s;
  } else {
    const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0;
    q[0] = (R[2] + R[6]) / s; q[1] = (R[5] + R[7]) / s; q[2] = 0.25 * s; q[3] = (R[3] - R[1]) / s;
  }
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double sg = q[3] < 0.0 ? -n : n;
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = q[k] / sg;
}

// the workgroup blockIdx.x of the gridDim.x that score one problem's hypotheses: the body of k_pnp_ransac and k_pnp_ransac_jobs
__device__ __forceinline__ void ransac_block(const PnpDev& d)
{
  __shared__ unsigned long long s_best[4];
  __shared__ int s_last;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int h = blockIdx.x * 4 + wave;
  unsigned long long best_key = 0;
  if (h < d.H) {
    double X[3][3], z[3][2];
    load_triple(d, h, X, z);
    P3P sol;
    p3p_solve(d, X, z, sol);
    int hyp_best = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      int count = 0;
      if (sol.valid[s]) {                                     // (uniform: every lane solved the same triple)
        for (int base = 0; base < d.M; base += 64) {
          const int i = base + lane;
          const bool in = i < d.M && is_inlier(d, sol.R[s], sol.t[s], i);
          count += __popcll(__ballot(in));
        }
      }
      hyp_best = max(hyp_best, count);
      best_key = max(best_key, ((unsigned long long)(unsigned)count << 32) | (unsigned)~(4 * h + s));
    }
    if (d.hyp_counts && lane == 0) d.hyp_counts[h] = hyp_best;
  }
  if (lane == 0) s_best[wave] = best_key;
  __syncthreads();
  if (threadIdx.x == 0) {
    // one atomic per workgroup, and none when the word already holds a larger key (it only ever grows)
    const unsigned long long k = max(max(s_best[0], s_best[1]), max(s_best[2], s_best[3]));
    if (k > __hip_atomic_load(d.best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(d.best, k);
    // the ticket releases this workgroup's key and, in the last workgroup, acquires everybody's
    const unsigned int prev = __hip_atomic_fetch_add(d.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = prev + 1u == gridDim.x;
  }
  __syncthreads();
  if (!s_last) return;
  // ---- finish: the winner's pose, mask and header ----
  const unsigned long long key = __hip_atomic_load(d.best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int n_best = (int)(key >> 32);
  const int id = (int)~(unsigned)key;                         // 4 h + s
  const bool found = n_best >= kMinInliers;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  if (found) {
    double X[3][3], z[3][2];
    load_triple(d, id >> 2, X, z);
    P3P sol;
    p3p_solve(d, X, z, sol);
    const int s = id & 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k == s) {
#pragma unroll
        for (int a = 0; a < 9; ++a) R[a] = sol.R[k][a];
        t[0] = sol.t[k][0]; t[1] = sol.t[k][1]; t[2] = sol.t[k][2];
      }
    }
  }
  for (int i = threadIdx.x; i < d.M; i += blockDim.x) d.inlier[i] = found && is_inlier(d, R, t, i) ? 1 : 0;
  if (threadIdx.x == 0) {
    double q[4];
    rot_to_quat(R, q);
    d.hdr->pose[0] = q[0]; d.hdr->pose[1] = q[1]; d.hdr->pose[2] = q[2]; d.hdr->pose[3] = q[3];
    d.hdr->pose[4] = t[0]; d.hdr->pose[5] = t[1]; d.hdr->pose[6] = t[2];
    d.hdr->found = found ? 1 : 0;
    d.hdr->n_inliers = found ? n_best : 0;
    d.hdr->best = found ? id : -1;
    d.hdr->pad = 0;
  }
}

__global__ __launch_bounds__(256) void k_pnp_ransac(PnpDev d)
{
  ransac_block(d);
}

// grid (ceil(H / 4), job): every job of ssx_pnp_pose_batch has its own problem, `best` / `ticket` words and header in the table; H is
// shared, so the last workgroup of a grid row finishes that row's job
__global__ __launch_bounds__(256) void k_pnp_ransac_jobs(const PnpDev* jobs)
{
  const PnpDev d = jobs[blockIdx.y];
  ransac_block(d);
}

// tap: one thread per triple, the solver and the quaternion as k_pnp_ransac calls them; slots that are not valid are zeros
__global__ void k_pnp_p3p_tap(PnpDev d, int n, int32_t* valid, double* R, double* t, double* pose)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double X[3][3], z[3][2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    X[k][0] = d.xyz[9 * (size_t)i + 3 * k]; X[k][1] = d.xyz[9 * (size_t)i + 3 * k + 1]; X[k][2] = d.xyz[9 * (size_t)i + 3 * k + 2];
    z[k][0] = d.uv[6 * (size_t)i + 2 * k]; z[k][1] = d.uv[6 * (size_t)i + 2 * k + 1];
  }
  P3P sol;
  p3p_solve(d, X, z, sol);
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const size_t o = 4 * (size_t)i + s;
    const bool ok = sol.valid[s];
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    if (ok) rot_to_quat(sol.R[s], q);
    valid[o] = ok ? 1 : 0;
#pragma unroll
    for (int a = 0; a < 9; ++a) R[9 * o + a] = ok ? sol.R[s][a] : 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) t[3 * o + a] = ok ? sol.t[s][a] : 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) pose[7 * o + a] = q[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) pose[7 * o + 4 + a] = ok ? sol.t[s][a] : 0.0;
  }
}

__global__ void k_pnp_samples(uint32_t seed, int M, int H, int32_t* out)
{
  const int h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= H) return;
  int tri[3];
  sample_triple(seed, h, M, tri);
  out[3 * h] = tri[0]; out[3 * h + 1] = tri[1]; out[3 * h + 2] = tri[2];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

bool finite4(const double* K4) { return std::isfinite(K4[0]) && std::isfinite(K4[1]) && std::isfinite(K4[2]) && std::isfinite(K4[3]); }

// One block for the whole of ComputeCorrectPose, each buffer stated once and in memory order: the RANSAC's best key and ticket (16
// bytes, zero before the launch), the refinement's problem (pose_only.hpp), the RANSAC's header and mask, the tap's counts, and the
// refinement's descriptor, which only the pinned mirror uses.  [best .. pose in] go up in one copy, [result .. mask] come back in one.
struct PnpBlock {
  unsigned long long* best = nullptr;
  PoProblem po;
  PnpHdr* hdr = nullptr;
  uint8_t* mask = nullptr;
  int32_t* counts = nullptr;
  PoDev* refine = nullptr;
};

struct PnpPlan {
  int M = 0, H = 0;
  bool tap = false;
  size_t bytes = 0;
  PnpBlock dev, host;               // the block in the arena and its mirror in the pinned block (wired by pnp_upload)
  template <class F> void each(PnpBlock& b, F&& f)
  {
    f(b.best, 16);
    b.po.each(f);
    f(b.hdr, sizeof(PnpHdr)); f(b.mask, (size_t)M);
    f(b.counts, tap ? sizeof(int32_t) * (size_t)H : 0);
    f(b.refine, sizeof(PoDev));
  }
  size_t wire(PnpBlock& b, char* base) { return carve(base, [&](auto&& f) { each(b, f); }); }
  size_t returned() const { return (size_t)(reinterpret_cast<const char*>(host.mask) + M - reinterpret_cast<const char*>(host.po.res)); }
};

PnpPlan plan_pnp(int M, int H, bool tap)
{
  PnpPlan p;
  p.M = M; p.H = H; p.tap = tap;
  p.dev.po.M = p.host.po.M = M;
  p.bytes = p.wire(p.host, nullptr);
  return p;
}

// stage the inputs (pose7 nullable) and send them up
ssx_status pnp_upload(ssx_ctx* ctx, PnpPlan& p, const double* xyz, const double* uv, const double* pose7)
{
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  SSX_HIP_TRY(ctx, ctx->pnp_arena.reserve(p.bytes));
  SSX_HIP_TRY(ctx, ctx->pnp_stage.reserve(p.bytes));
  char* hs = ctx->pnp_stage.as<char>();
  p.wire(p.dev, ctx->pnp_arena.as<char>());
  p.wire(p.host, hs);
  memset(p.host.best, 0, 16);
  p.host.po.stage(xyz, uv, pose7);
  SSX_HIP_TRY(ctx, hipMemcpyAsync(ctx->pnp_arena.p, hs, (size_t)(p.host.po.sent() - hs), hipMemcpyHostToDevice, ctx->stream));
  return SSX_OK;
}

ssx_status pnp_launch_ransac(ssx_ctx* ctx, const PnpPlan& p, const double* K4, double reproj_px, uint32_t seed)
{
  PnpDev d;
  d.M = p.M; d.H = p.H; d.seed = seed;
  d.fx = K4[0]; d.fy = K4[1]; d.cx = K4[2]; d.cy = K4[3]; d.thr2 = reproj_px * reproj_px;
  d.xyz = p.dev.po.xyz; d.uv = p.dev.po.uv;
  d.best = p.dev.best; d.ticket = reinterpret_cast<unsigned int*>(p.dev.best + 1);
  d.hdr = p.dev.hdr; d.inlier = p.dev.mask;
  d.hyp_counts = p.tap ? p.dev.counts : nullptr;
  SSX_PROF(ctx, KID_PNP_RANSAC, hipLaunchKernelGGL(k_pnp_ransac, dim3((unsigned)((p.H + 3) / 4)), dim3(256), 0, ctx->stream, d));
  SSX_HIP_TRY(ctx, hipGetLastError());
  return SSX_OK;
}

// OptimizeCurrentPose: one warm-up optimize(10), then 4 rounds x optimize(10), from the uploaded pose or, with hdr, from the pose the
// RANSAC left in its header (device memory), called off where it found none
ssx_status pnp_launch_refine(ssx_ctx* ctx, const PnpPlan& p, const double* K4, const PnpHdr* hdr, double chi2_th, double huber_delta)
{
  PoDev& d = *p.host.refine;
  po_set_scalars(d, p.M, 1, 4, 10, chi2_th, huber_delta, K4, hdr ? &hdr->found : nullptr);
  p.dev.po.wire(d, hdr ? hdr->pose : nullptr);
  SSX_HIP_TRY(ctx, po_launch_device(ctx, &d));
  return SSX_OK;
}

// the results, the tap's counts behind them, and the synchronisation of the call
ssx_status pnp_download(ssx_ctx* ctx, const PnpPlan& p)
{
  SSX_HIP_TRY(ctx, hipMemcpyAsync(p.host.po.res, p.dev.po.res, p.returned(), hipMemcpyDeviceToHost, ctx->stream));
  if (p.tap) SSX_HIP_TRY(ctx, hipMemcpyAsync(p.host.counts, p.dev.counts, sizeof(int32_t) * (size_t)p.H, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return SSX_OK;
}

bool pnp_args_ok(ssx_ctx* ctx, const double* K4, int32_t M, const double* xyz, const double* uv, int32_t max_iters)
{
  return ctx && K4 && M >= 0 && (M == 0 || (xyz && uv)) && max_iters >= 1 && max_iters <= SSX_PNP_MAX_ITERS && finite4(K4);
}

const double kIdentity[7] = {0, 0, 0, 1, 0, 0, 0};

}  // namespace

extern "C" {

ssx_status ssx_pnp_ransac(ssx_ctx* ctx, const double* K4, int32_t M, const double* xyz, const double* uv, int32_t max_iters, double reproj_px,
                          uint32_t seed, double* pose_out, uint8_t* inlier_out, int32_t* n_inliers, int32_t* best_hypothesis, int32_t* found)
{
  if (!pnp_args_ok(ctx, K4, M, xyz, uv, max_iters) || !pose_out || !n_inliers || !found || !(reproj_px >= 0.0)) return SSX_ERR_INVALID_ARG;
  *found = 0; *n_inliers = 0;
  if (best_hypothesis) *best_hypothesis = -1;
  memcpy(pose_out, kIdentity, sizeof(kIdentity));
  if (inlier_out && M > 0) memset(inlier_out, 0, (size_t)M);
  if (M < 3) return SSX_OK;                                   // no triple to sample
  PnpPlan p = plan_pnp(M, max_iters, false);
  ssx_status st = pnp_upload(ctx, p, xyz, uv, nullptr);
  if (st == SSX_OK) st = pnp_launch_ransac(ctx, p, K4, reproj_px, seed);
  if (st == SSX_OK) st = pnp_download(ctx, p);
  if (st != SSX_OK) return st;
  const PnpHdr& hdr = *p.host.hdr;
  *found = hdr.found; *n_inliers = hdr.n_inliers;
  if (best_hypothesis) *best_hypothesis = hdr.best;
  memcpy(pose_out, hdr.pose, sizeof(double) * 7);
  if (inlier_out) memcpy(inlier_out, p.host.mask, (size_t)M);
  return SSX_OK;
}

ssx_status ssx_loop_pose_opt(ssx_ctx* ctx, double* pose_io, const double* K4, int32_t M, const double* xyz, const double* uv, double chi2_th,
                             double huber_delta, uint8_t* inlier_out, int32_t* n_inliers)
{
  if (!ctx || !pose_io || !K4 || M < 0 || (M > 0 && (!xyz || !uv)) || !finite4(K4)) return SSX_ERR_INVALID_ARG;
  if (n_inliers) *n_inliers = 0;
  if (M == 0) return SSX_OK;
  PnpPlan p = plan_pnp(M, 0, false);
  ssx_status st = pnp_upload(ctx, p, xyz, uv, pose_io);
  if (st == SSX_OK) st = pnp_launch_refine(ctx, p, K4, nullptr, chi2_th, huber_delta);
  if (st == SSX_OK) st = pnp_download(ctx, p);
  if (st != SSX_OK) return st;
  po_read_result(p.host.po.res, M, pose_io, inlier_out, n_inliers);
  return SSX_OK;
}

ssx_status ssx_loop_compute_pose(ssx_ctx* ctx, int32_t n_pairs, const double* loop_xyz, const uint8_t* has_point, const double* cur_uv,
                                 const double* T_cur, const double* T_loop, const double* K4, int32_t max_iters, uint32_t seed, uint8_t* kept,
                                 ssx_loop_pose_result* out)
{
  if (!ctx || n_pairs < 0 || (n_pairs > 0 && (!loop_xyz || !has_point || !cur_uv || !kept)) || !T_cur || !T_loop || !K4 || !out || max_iters < 1 ||
      max_iters > SSX_PNP_MAX_ITERS || !finite4(K4))
    return SSX_ERR_INVALID_ARG;
  memset(out, 0, sizeof(*out));
  out->best_hypothesis = -1;
  memcpy(out->corrected_pose, kIdentity, sizeof(kIdentity));
  memcpy(out->relative_to_loop, kIdentity, sizeof(kIdentity));
  // the pairs whose map point is alive (loopclosing.cpp:153-174; the others are erased from the set)
  std::vector<double> xyz, uv;
  std::vector<int32_t> src;
  for (int32_t i = 0; i < n_pairs; ++i) {
    kept[i] = has_point[i] ? 1 : 0;
    if (!has_point[i]) continue;
    src.push_back(i);
    xyz.insert(xyz.end(), loop_xyz + 3 * (size_t)i, loop_xyz + 3 * (size_t)i + 3);
    uv.insert(uv.end(), cur_uv + 2 * (size_t)i, cur_uv + 2 * (size_t)i + 2);
  }
  const int32_t M = (int32_t)src.size();
  out->n_with_point = M;
  if (M < 10) { out->verdict = SSX_LOOP_FEW_MAP_POINTS; return SSX_OK; }           // :193
  const double thr = 5.991, chi2_th = 5.991, huber_delta = 1.0;                   // :206, :301, g2o's RobustKernelHuber
  PnpPlan p = plan_pnp(M, max_iters, false);
  ssx_status st = pnp_upload(ctx, p, xyz.data(), uv.data(), nullptr);
  if (st == SSX_OK) st = pnp_launch_ransac(ctx, p, K4, thr, seed);
  if (st == SSX_OK) st = pnp_launch_refine(ctx, p, K4, p.dev.hdr, chi2_th, huber_delta);
  if (st == SSX_OK) st = pnp_download(ctx, p);
  if (st != SSX_OK) return st;
  const PnpHdr& hdr = *p.host.hdr;
  out->n_ransac_inliers = hdr.n_inliers;
  out->best_hypothesis = hdr.best;
  if (!hdr.found) { out->verdict = SSX_LOOP_NO_POSE; return SSX_OK; }              // the exception of :203-210
  po_read_result(p.host.po.res, M, out->corrected_pose, kept, &out->n_inliers, src.data());   // (kept: the erase of :338-344)
  if (out->n_inliers < 10) { out->verdict = SSX_LOOP_FEW_INLIERS; return SSX_OK; } // :219
  double inv[7], rel[7], lg[6];
  ssx::se3_inverse(out->corrected_pose, inv);
  ssx::se3_mul(T_cur, inv, rel);
  ssx::se3_log(rel, lg);
  double n2 = 0.0;
  for (int k = 0; k < 6; ++k) n2 += lg[k] * lg[k];
  out->error = std::sqrt(n2);                                                     // :224-225
  out->need_correct = (out->error > 1 && out->error < 15) ? 1 : 0;                 // :226
  ssx::se3_inverse(T_loop, inv);
  ssx::se3_mul(out->corrected_pose, inv, out->relative_to_loop);                   // :237-238
  out->verdict = SSX_LOOP_OK;
  return SSX_OK;
}

// n times (ssx_pnp_ransac, then ssx_loop_pose_opt from the pose it found) in one block, one upload, one launch of k_pnp_ransac_jobs, one
// launch of the refinement per kernel class, one download and one synchronisation.  The jobs with a triple to sample (M >= 3) are
// ordered by class (po_class), in job order inside a class, so that each class's descriptors are one run of the table.
ssx_status ssx_pnp_pose_batch(ssx_ctx* ctx, const double* K4, int32_t n, ssx_pnp_pose_job* jobs, int32_t max_iters, double reproj_px, double chi2_th,
                              double huber_delta)
{
  if (!ctx || !K4 || n < 0 || n > SSX_PNP_BATCH_MAX || (n > 0 && !jobs) || max_iters < 1 || max_iters > SSX_PNP_MAX_ITERS || !finite4(K4) || !(reproj_px >= 0.0))
    return SSX_ERR_INVALID_ARG;
  for (int j = 0; j < n; ++j)
    if (jobs[j].M < 0 || (jobs[j].M > 0 && (!jobs[j].xyz || !jobs[j].uv))) return SSX_ERR_INVALID_ARG;
  std::vector<int> act;                                       // the jobs that run, in table order
  int first[4] = {0, 0, 0, 0};                                // class c is act[first[c] .. first[c + 1])
  for (int c = 0; c < 3; ++c) {
    for (int j = 0; j < n; ++j)
      if (jobs[j].M >= 3 && po_class(jobs[j].M) == c) act.push_back(j);
    first[c + 1] = (int)act.size();
  }
  for (int j = 0; j < n; ++j) {
    ssx_pnp_pose_job& q = jobs[j];
    q.found = 0; q.n_ransac_inliers = 0; q.best_hypothesis = -1; q.n_inliers = 0;
    memcpy(q.pose_out, kIdentity, sizeof(kIdentity));
    if (q.inlier_out && q.M > 0) memset(q.inlier_out, 0, (size_t)q.M);
  }
  const size_t na = act.size();
  if (na == 0) return SSX_OK;
  struct Block {
    unsigned long long* zero = nullptr;                       // (best, ticket) of every job: zero before the launch
    PnpDev* rt = nullptr;                                     // the RANSAC's job table
    PoDev* pt = nullptr;                                      // the refinement's descriptors
    std::vector<PoProblem> po;
    std::vector<PnpHdr*> hdr;
    std::vector<uint8_t*> mask;
    char *sent = nullptr, *ret = nullptr;                     // [start, sent) goes up, [ret, end) comes back
  } dev, host;
  auto wire_block = [&](Block& b, char* base) {
    b.po.assign(na, PoProblem{}); b.hdr.assign(na, nullptr); b.mask.assign(na, nullptr);
    return carve(base, [&](auto&& f) {
      f(b.zero, 16 * na); f(b.rt, sizeof(PnpDev) * na); f(b.pt, sizeof(PoDev) * na);
      for (size_t k = 0; k < na; ++k) {
        PoProblem& p = b.po[k];
        p.M = jobs[act[k]].M;
        f(p.xyz, sizeof(double) * 3 * (size_t)p.M); f(p.uv, sizeof(double) * 2 * (size_t)p.M); f(p.pose_in, sizeof(double) * 8);
      }
      f(b.sent, 0);
      for (size_t k = 0; k < na; ++k) {                       // what only the device uses: the generic kernel's scratch, the RANSAC's mask
        PoProblem& p = b.po[k];
        const size_t scratch = po_class(p.M) == 2 ? (size_t)p.M : 0;
        f(p.err, sizeof(double) * 2 * scratch); f(p.level, scratch); f(b.mask[k], (size_t)p.M);
      }
      f(b.ret, 0);
      for (size_t k = 0; k < na; ++k) { f(b.po[k].res, b.po[k].result_bytes()); f(b.hdr[k], sizeof(PnpHdr)); }
    });
  };
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t bytes = wire_block(host, nullptr);
  SSX_HIP_TRY(ctx, ctx->pnp_arena.reserve(bytes));
  SSX_HIP_TRY(ctx, ctx->pnp_stage.reserve(bytes));
  char* hs = ctx->pnp_stage.as<char>();
  char* ds = ctx->pnp_arena.as<char>();
  wire_block(dev, ds);
  wire_block(host, hs);
  memset(host.zero, 0, 16 * na);
  for (size_t k = 0; k < na; ++k) {
    const ssx_pnp_pose_job& q = jobs[act[k]];
    host.po[k].stage(q.xyz, q.uv, nullptr);
    PnpDev& r = host.rt[k];
    r.M = q.M; r.H = max_iters; r.seed = q.seed;
    r.fx = K4[0]; r.fy = K4[1]; r.cx = K4[2]; r.cy = K4[3]; r.thr2 = reproj_px * reproj_px;
    r.xyz = dev.po[k].xyz; r.uv = dev.po[k].uv;
    r.best = dev.zero + 2 * k; r.ticket = reinterpret_cast<unsigned int*>(dev.zero + 2 * k + 1);
    r.hdr = dev.hdr[k]; r.inlier = dev.mask[k]; r.hyp_counts = nullptr;
    // OptimizeCurrentPose from the pose in the job's header, called off where the RANSAC found none (as pnp_launch_refine)
    PoDev& d = host.pt[k];
    po_set_scalars(d, q.M, 1, 4, 10, chi2_th, huber_delta, K4, &dev.hdr[k]->found);
    dev.po[k].wire(d, dev.hdr[k]->pose);
  }
  hipStream_t s = ctx->stream;
  SSX_HIP_TRY(ctx, hipMemcpyAsync(ds, hs, (size_t)(host.sent - hs), hipMemcpyHostToDevice, s));
  SSX_PROF(ctx, KID_PNP_RANSAC, hipLaunchKernelGGL(k_pnp_ransac_jobs, dim3((unsigned)((max_iters + 3) / 4), (unsigned)na), dim3(256), 0, s, dev.rt));
  SSX_HIP_TRY(ctx, hipGetLastError());
  for (int c = 0; c < 3; ++c)
    if (first[c + 1] > first[c]) SSX_HIP_TRY(ctx, po_launch_device_table(ctx, c, (unsigned)(first[c + 1] - first[c]), dev.pt + first[c]));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(host.ret, dev.ret, bytes - (size_t)(host.ret - hs), hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  for (size_t k = 0; k < na; ++k) {
    ssx_pnp_pose_job& q = jobs[act[k]];
    const PnpHdr& hdr = *host.hdr[k];
    q.n_ransac_inliers = hdr.n_inliers; q.best_hypothesis = hdr.best;
    if (!hdr.found) continue;                                 // (the refinement was called off: its record holds nothing)
    q.found = 1;
    po_read_result(host.po[k].res, q.M, q.pose_out, q.inlier_out, &q.n_inliers);
  }
  return SSX_OK;
}

#ifndef SSX_NO_TEST_HOOKS
ssx_status ssx_pnp_debug_samples(ssx_ctx* ctx, uint32_t seed, int32_t M, int32_t H, int32_t* triples_out)
{
  if (!ctx || M < 3 || H < 1 || H > SSX_PNP_MAX_ITERS || !triples_out) return SSX_ERR_INVALID_ARG;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t *dev = nullptr, *host = nullptr;
  const size_t tri_bytes = sizeof(int32_t) * 3 * (size_t)H, bytes = carve(nullptr, [&](auto&& f) { f(dev, tri_bytes); });
  SSX_HIP_TRY(ctx, ctx->pnp_arena.reserve(bytes));
  SSX_HIP_TRY(ctx, ctx->pnp_stage.reserve(bytes));
  carve(ctx->pnp_arena.as<char>(), [&](auto&& f) { f(dev, tri_bytes); });
  carve(ctx->pnp_stage.as<char>(), [&](auto&& f) { f(host, tri_bytes); });
  hipLaunchKernelGGL(k_pnp_samples, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, ctx->stream, seed, M, H, dev);
  SSX_HIP_TRY(ctx, hipGetLastError());
  SSX_HIP_TRY(ctx, hipMemcpyAsync(host, dev, tri_bytes, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(triples_out, host, tri_bytes);
  return SSX_OK;
}

ssx_status ssx_pnp_debug_counts(ssx_ctx* ctx, const double* K4, int32_t M, const double* xyz, const double* uv, int32_t max_iters, double reproj_px,
                                uint32_t seed, int32_t* counts_out)
{
  if (!pnp_args_ok(ctx, K4, M, xyz, uv, max_iters) || M < 3 || !counts_out) return SSX_ERR_INVALID_ARG;
  PnpPlan p = plan_pnp(M, max_iters, true);
  ssx_status st = pnp_upload(ctx, p, xyz, uv, nullptr);
  if (st == SSX_OK) st = pnp_launch_ransac(ctx, p, K4, reproj_px, seed);
  if (st == SSX_OK) st = pnp_download(ctx, p);
  if (st != SSX_OK) return st;
  memcpy(counts_out, p.host.counts, sizeof(int32_t) * (size_t)max_iters);
  return SSX_OK;
}

ssx_status ssx_pnp_debug_p3p(ssx_ctx* ctx, const double* K4, int32_t n, const double* xyz, const double* uv, int32_t* valid_out, double* R_out,
                             double* t_out, double* pose_out)
{
  if (!ctx || !K4 || n < 0 || !finite4(K4) || (n > 0 && (!xyz || !uv || !valid_out || !R_out || !t_out || !pose_out))) return SSX_ERR_INVALID_ARG;
  if (n == 0) return SSX_OK;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t N = (size_t)n;
  // the triples go up, [R .. valid] come back
  struct Block { double *xyz, *uv, *R, *t, *pose; int32_t* valid; } dev{}, host{};
  auto wire_block = [&](Block& b, char* base) {
    return carve(base, [&](auto&& f) {
      f(b.xyz, sizeof(double) * 9 * N); f(b.uv, sizeof(double) * 6 * N);
      f(b.R, sizeof(double) * 36 * N); f(b.t, sizeof(double) * 12 * N); f(b.pose, sizeof(double) * 28 * N); f(b.valid, sizeof(int32_t) * 4 * N);
    });
  };
  const size_t bytes = wire_block(dev, nullptr);
  SSX_HIP_TRY(ctx, ctx->pnp_arena.reserve(bytes));
  SSX_HIP_TRY(ctx, ctx->pnp_stage.reserve(bytes));
  char* hs = ctx->pnp_stage.as<char>();
  wire_block(dev, ctx->pnp_arena.as<char>());
  wire_block(host, hs);
  memcpy(host.xyz, xyz, sizeof(double) * 9 * N);
  memcpy(host.uv, uv, sizeof(double) * 6 * N);
  SSX_HIP_TRY(ctx, hipMemcpyAsync(dev.xyz, hs, (size_t)(reinterpret_cast<char*>(host.R) - hs), hipMemcpyHostToDevice, ctx->stream));
  PnpDev d = {};
  d.fx = K4[0]; d.fy = K4[1]; d.cx = K4[2]; d.cy = K4[3];
  d.xyz = dev.xyz; d.uv = dev.uv;
  hipLaunchKernelGGL(k_pnp_p3p_tap, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, ctx->stream, d, n, dev.valid, dev.R, dev.t, dev.pose);
  SSX_HIP_TRY(ctx, hipGetLastError());
  SSX_HIP_TRY(ctx, hipMemcpyAsync(host.R, dev.R, (size_t)(hs + bytes - reinterpret_cast<char*>(host.R)), hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(R_out, host.R, sizeof(double) * 36 * N);
  memcpy(t_out, host.t, sizeof(double) * 12 * N);
  memcpy(pose_out, host.pose, sizeof(double) * 28 * N);
  memcpy(valid_out, host.valid, sizeof(int32_t) * 4 * N);
  return SSX_OK;
}
#endif

}  // extern "C"

#ifndef SSX_NO_TEST_HOOKS
void pnp_describe_plan(int M, int H, bool tap, ssx_pnp_plan_info* out)
{
  memset(out, 0, sizeof(*out));
  PnpPlan p = plan_pnp(M, H, tap);                            // (carved from a null base, the mirror's pointers are its offsets)
  auto span = [&](int k, auto* ptr, size_t bytes) { out->span_off[k] = reinterpret_cast<uintptr_t>(ptr); out->span_bytes[k] = bytes; };
  int k = 0;
  p.each(p.host, [&](auto*& ptr, size_t bytes) { span(k++, ptr, bytes); });
  out->bytes = p.bytes;
  out->sent = reinterpret_cast<uintptr_t>(p.host.po.sent());
  out->ret_off = reinterpret_cast<uintptr_t>(p.host.po.res);
  out->ret_bytes = p.returned();
  out->refine_cls = M ? po_class(M) : 3;
}
#endif
