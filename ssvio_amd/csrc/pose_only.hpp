// ssvio_amd/csrc/pose_only.hpp -- what the pose-only kernels (pose_only.hip) read and write, for their callers inside the library: the
// front end's batch (pose_only.hip) and the refine step of loop closing (pnp.hip), which starts from the pose a kernel has just written.
#pragma once
#include "ctx.hpp"
#include "se3.hpp"

// the descriptor of one problem as the kernels take it
struct PoDev {
  int M, rounds, iters;
  double chi2_th, huber_delta;
  ssx::Cam K;
  const double* xyz;   // M x 3
  const double* uv;    // M x 2
  double* err;         // M x 2 (last computed error of each edge, like g2o's _error)
  uint8_t* level;      // M: 1 = outlier level (not optimised)
  uint8_t* outlier;    // M: features[i]->is_outlier_
  const double* pose;  // 7 in (never written: it may be another kernel's result)
  double* pose_out;    // 7 out
  int* n_inliers;
  int warmup;          // optimize(iters) passes over all edges before the classified rounds (0: EstimateCurrentPose)
  const int* gate;     // nullable: *gate == 0 ends the launch before it writes anything
};

// The kernel of a problem of M > 0 edges: 0 = k_pose_only<2> (up to 2 edges in the registers of each of the 256 threads), 1 =
// k_pose_only<6> (up to 6), 2 = k_pose_only_generic (edges in device memory, any M).
constexpr int kPoThreads = 256;
constexpr int po_class(int M) { return M <= kPoThreads * 2 ? 0 : M <= kPoThreads * 6 ? 1 : 2; }
constexpr int po_register_edges() { return kPoThreads * 6; }      // up to this many edges a problem stays in registers
static_assert(po_class(po_register_edges()) == 1 && po_class(po_register_edges() + 1) == 2, "po_register_edges() is the last M of class 1");

// what a launch leaves behind: the record and, right behind it, M outlier flags (1 = the edge ends as outlier)
struct PoResult {
  double pose[8];      // 7 used
  int32_t n_inliers, pad;
};

// The buffers of one problem, each stated ONCE and in memory order (carve, ctx.hpp): the inputs, the generic kernel's scratch (empty up
// to po_register_edges() edges), the result.  A copy that sends the block up ends at sent(); result_bytes() from `res` come back.
struct PoProblem {
  int M = 0;
  double *xyz = nullptr, *uv = nullptr, *pose_in = nullptr, *err = nullptr;
  uint8_t* level = nullptr;
  PoResult* res = nullptr;
  template <class F> void each(F&& f)
  {
    const size_t m = (size_t)M, scratch = po_class(M) == 2 ? m : 0;
    f(xyz, sizeof(double) * 3 * m); f(uv, sizeof(double) * 2 * m); f(pose_in, sizeof(double) * 8);
    f(err, sizeof(double) * 2 * scratch); f(level, scratch);
    f(res, result_bytes());
  }
  size_t result_bytes() const { return sizeof(PoResult) + (size_t)M; }
  uint8_t* flags() const { return reinterpret_cast<uint8_t*>(res + 1); }
  const char* sent() const { return reinterpret_cast<const char*>(err); }     // (the end of pose_in's span, whether or not there is scratch)
  // the inputs into a block the host can write (pose7 nullable: the start is another kernel's result)
  void stage(const double* xyz_in, const double* uv_in, const double* pose7) const
  {
    memcpy(xyz, xyz_in, sizeof(double) * 3 * (size_t)M);
    memcpy(uv, uv_in, sizeof(double) * 2 * (size_t)M);
    if (pose7) memcpy(pose_in, pose7, sizeof(double) * 7);
  }
  // the pointer half of a descriptor (start: where the pose to start from lies, when not in pose_in)
  void wire(PoDev& d, const double* start = nullptr) const
  {
    const bool scratch = po_class(M) == 2;
    d.xyz = xyz; d.uv = uv; d.pose = start ? start : pose_in;
    d.err = scratch ? err : nullptr; d.level = scratch ? level : nullptr;
    d.pose_out = res->pose; d.n_inliers = &res->n_inliers; d.outlier = flags();
  }
};

// the scalar half of a descriptor
inline void po_set_scalars(PoDev& d, int M, int warmup, int rounds, int iters, double chi2_th, double huber_delta, const double* K4, const int* gate)
{
  d.M = M; d.warmup = warmup; d.rounds = rounds; d.iters = iters; d.chi2_th = chi2_th; d.huber_delta = huber_delta;
  d.K = ssx::Cam{K4[0], K4[1], K4[2], K4[3]}; d.gate = gate;
}

// A result as the entry points hand it out, from a record the host can read: the pose, the count, and per edge 1 = inlier at
// inlier_out[src ? src[k] : k].  Each output may be null.
inline void po_read_result(const PoResult* r, int M, double* pose7, uint8_t* inlier_out, int32_t* n_inliers, const int32_t* src = nullptr)
{
  if (pose7) memcpy(pose7, r->pose, sizeof(double) * 7);
  if (n_inliers) *n_inliers = r->n_inliers;
  const uint8_t* outlier = reinterpret_cast<const uint8_t*>(r + 1);
  if (inlier_out) for (int k = 0; k < M; ++k) inlier_out[src ? src[k] : k] = !outlier[k];
}

// One launch of the kernel of d->M > 0 edges on ctx->stream, no synchronisation.  d is a filled descriptor in pinned memory of the
// caller's own, which stays as it is until the stream is idle (the register-resident kernels read it from there).
hipError_t po_launch_device(ssx_ctx* ctx, const PoDev* d);
// One launch for n > 0 problems that are all of class cls (po_class), one workgroup each: dv[0 .. n) are their descriptors in memory the
// device can read, which stays as it is until the stream is idle.  No synchronisation.
hipError_t po_launch_device_table(ssx_ctx* ctx, int cls, unsigned n, const PoDev* dv);

#ifndef SSX_NO_TEST_HOOKS
struct ssx_pnp_plan_info;
void pnp_describe_plan(int M, int H, bool tap, ssx_pnp_plan_info* out);   // pnp.hip, for ssx_po_debug_plan
#endif
