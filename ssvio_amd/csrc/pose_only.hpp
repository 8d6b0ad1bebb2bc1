// ssvio_amd/csrc/pose_only.hpp -- the pose-only kernels (pose_only.hip) for callers inside the library whose problem already
// lies in device memory: the refine step of loop closing (pnp.hip), which starts from the pose a kernel has just written.
#pragma once
#include "ctx.hpp"

struct PoDeviceJob {
  int32_t M;                  // > 0
  int32_t warmup;             // optimize(iters) passes with every edge at level 0 and the robust kernel on, before the classified rounds
  int32_t rounds, iters;
  double chi2_th, huber_delta;
  double K4[4];
  const double* xyz;          // M x 3   (every pointer: device memory)
  const double* uv;           // M x 2
  const double* pose_in;      // 7
  const int32_t* gate;        // nullable: the kernel returns at once, writing nothing, when *gate == 0
  double* err;                // M x 2 and M bytes of scratch, used above po_register_edges() edges only
  uint8_t* level;
  uint8_t* outlier;           // M: 1 = the edge ends as outlier
  double* pose_out;           // 7
  int32_t* n_inliers;
};

int po_register_edges();      // up to this many edges a problem stays in registers

// one launch on ctx->stream, no synchronisation (ctx->po_stage carries the descriptor: it is the caller's until the stream is idle)
hipError_t po_launch_device(ssx_ctx* ctx, const PoDeviceJob& job);
