// ssvio_amd/csrc/undistort.hip -- image undistortion on the device: Camera::UndistortImage (src/ssvio/camera.cpp:43-55, a cv::undistort
// with K and k1 k2 p1 p2), which FrontEnd::GrabSteroImage applies to both images of a frame when Camera.NeedUndistortion is set
// (src/ssvio/frontend.cpp:39-45).  OpenCV cannot be pinned, so the contract is a model: tools/undistort_model.py.
//
// k_undistort    grid (ceil(cols / 256), ceil(rows / 4), jobs), block 64 x 4.  One thread produces four consecutive destination pixels of a
//                row and stores them as one dword (byte stores on the row tail and where the pitch leaves the address unaligned); a
//                wavefront covers 256 pixels of one row, so its taps fall on a few neighbouring source lines; a workgroup covers four
//                rows.  No LDS, no scratch.  Per pixel the map is computed inline in f64, one operation per statement in the order of the
//                model (about 40 operations), quantised to 1/32 pixel by ud_q -- its NaN case and its clamp are written out, not left to
//                a conversion instruction -- and the four taps are weighted with the 10-bit products of the 5-bit fractions.  Every tap
//                is tested on its integer coordinates before its address is formed; a tap outside the image reads 0.
//                The map is not kept between calls: 6 bytes per pixel of map traffic would cost more HBM time than the image itself,
//                and there is no state to invalidate when the parameters change (profiles/undistort/time.txt has the measured time).
//
// ssx_undistort  n jobs of one image size in ONE launch.  Host images: the job table and the sources go up in one copy (pinned staging),
//                the results come down in one copy, one synchronisation.  images_on_device: only the job table goes up, the kernel reads
//                and writes the images where they lie (device or pinned memory), nothing comes down.
//
// This file is compiled with -ffp-contract=off: every f64 operation rounds on its own, as the model's does
// (tests/test_undistort_gpu.py: the output is the model's bytes).
#include <cmath>
#include <cstdint>
#include <cstring>

#include "ctx.hpp"
#include "../../include/ssx_test_hooks.h"

namespace {

constexpr int UD_PX = 4;                    // destination pixels per thread: one dword
constexpr int UD_BX = 64, UD_BY = 4;        // a wavefront per row segment of 256 pixels, four rows per workgroup
constexpr int UD_MAX_SIDE = 32768;

// one job as the kernel reads it (wave-uniform: scalar loads)
struct UdJob {
  const uint8_t* src;
  uint8_t* dst;
  int64_t src_stride, dst_stride;
  double K[4], dist[5], iR[9];
};

// q(t) of the model: 0 for NaN, else round to nearest (ties to even) clamped to [-2^31, 2^31 - 1]
__device__ __forceinline__ int32_t ud_q(double t)
{
  if (t != t) return 0;
  const double r = rint(t);
  if (r <= -2147483648.0) return INT32_MIN;
  if (r >= 2147483647.0) return INT32_MAX;
  return (int32_t)r;
}

// p(Y, X) of the model: the source byte, or 0 outside [0, rows) x [0, cols); the address is formed behind the test
__device__ __forceinline__ uint32_t ud_tap(const uint8_t* __restrict__ src, int64_t stride, int32_t rows, int32_t cols, int32_t Y, int32_t X)
{
  if (Y < 0 || Y >= rows || X < 0 || X >= cols) return 0u;
  return src[(int64_t)Y * stride + (int64_t)X];
}

__device__ __forceinline__ uint32_t ud_pixel(const UdJob& jb, int32_t rows, int32_t cols, int32_t i, int32_t j)
{
  const double dj = (double)j, di = (double)i;
  const double X = (dj * jb.iR[0] + di * jb.iR[1]) + jb.iR[2];
  const double Y = (dj * jb.iR[3] + di * jb.iR[4]) + jb.iR[5];
  const double W = (dj * jb.iR[6] + di * jb.iR[7]) + jb.iR[8];
  const double w = 1.0 / W;
  const double x = X * w;
  const double y = Y * w;
  const double x2 = x * x;
  const double y2 = y * y;
  const double r2 = x2 + y2;
  const double _2xy = (2.0 * x) * y;
  const double k1 = jb.dist[0], k2 = jb.dist[1], p1 = jb.dist[2], p2 = jb.dist[3], k3 = jb.dist[4];
  const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
  const double xd = (x * kr + p1 * _2xy) + p2 * (r2 + 2.0 * x2);
  const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * _2xy;
  const double u = jb.K[0] * xd + jb.K[2];
  const double v = jb.K[1] * yd + jb.K[3];
  const int32_t iu = ud_q(u * 32.0);
  const int32_t iv = ud_q(v * 32.0);
  const int32_t X0 = iu >> 5, Y0 = iv >> 5;                       // arithmetic shifts: |X0|, |Y0| <= 2^26, so X0 + 1 cannot overflow
  const uint32_t a = (uint32_t)(iu & 31), b = (uint32_t)(iv & 31);
  const uint32_t p00 = ud_tap(jb.src, jb.src_stride, rows, cols, Y0, X0);
  const uint32_t p01 = ud_tap(jb.src, jb.src_stride, rows, cols, Y0, X0 + 1);
  const uint32_t p10 = ud_tap(jb.src, jb.src_stride, rows, cols, Y0 + 1, X0);
  const uint32_t p11 = ud_tap(jb.src, jb.src_stride, rows, cols, Y0 + 1, X0 + 1);
  const uint32_t acc = (32u - a) * (32u - b) * p00 + a * (32u - b) * p01 + (32u - a) * b * p10 + a * b * p11;   // <= 1024 * 255
  return (acc + 512u) >> 10;
}

__global__ void __launch_bounds__(UD_BX * UD_BY) k_undistort(const UdJob* __restrict__ jobs, int32_t rows, int32_t cols)
{
  const int32_t i = (int32_t)(blockIdx.y * UD_BY + threadIdx.y);
  const int32_t j0 = (int32_t)((blockIdx.x * UD_BX + threadIdx.x) * UD_PX);
  if (i >= rows || j0 >= cols) return;
  const UdJob& jb = jobs[blockIdx.z];
  uint8_t* out = jb.dst + (int64_t)i * jb.dst_stride + (int64_t)j0;
  if (j0 + UD_PX <= cols && (reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < UD_PX; ++k) word |= ud_pixel(jb, rows, cols, i, j0 + k) << (8 * k);
    *reinterpret_cast<uint32_t*>(out) = word;
  } else {
    for (int k = 0; k < UD_PX && j0 + k < cols; ++k) out[k] = (uint8_t)ud_pixel(jb, rows, cols, i, j0 + k);
  }
}

// [first, last) of an image in memory: from its pointer to the end of its last row
inline void ud_span(const uint8_t* p, int64_t stride, int32_t rows, int32_t cols, uintptr_t* first, uintptr_t* last)
{
  *first = reinterpret_cast<uintptr_t>(p);
  *last = *first + (uintptr_t)((int64_t)(rows - 1) * stride + cols);
}

}  // namespace

extern "C" {

void ssx_undistort_default(const double K4[4], const double dist5[5], ssx_undistort_params* out)
{
  if (!K4 || !dist5 || !out) return;
  std::memcpy(out->K, K4, sizeof(out->K));
  std::memcpy(out->dist, dist5, sizeof(out->dist));
  const double fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
  const double iR[9] = {1.0 / fx, 0.0, -cx / fx, 0.0, 1.0 / fy, -cy / fy, 0.0, 0.0, 1.0};
  std::memcpy(out->iR, iR, sizeof(out->iR));
}

ssx_status ssx_undistort(ssx_ctx* ctx, int32_t n, const ssx_undistort_job* jobs, int32_t rows, int32_t cols, int32_t images_on_device)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  ctx->undistort = KfChainStats{};
  // every refusal comes before anything is touched
  if (n < 0 || n > SSX_UNDISTORT_MAX_JOBS) { ctx->set_error("ssx_undistort: n = %d outside [0, %d]", n, SSX_UNDISTORT_MAX_JOBS); return SSX_ERR_INVALID_ARG; }
  if (rows < 1 || cols < 1) { ctx->set_error("ssx_undistort: rows = %d, cols = %d (both must be >= 1)", rows, cols); return SSX_ERR_INVALID_ARG; }
  if (n > 0 && !jobs) { ctx->set_error("ssx_undistort: jobs is null"); return SSX_ERR_INVALID_ARG; }
  for (int32_t k = 0; k < n; ++k) {
    if (!jobs[k].src || !jobs[k].dst) { ctx->set_error("ssx_undistort: job %d has a null %s", k, jobs[k].src ? "dst" : "src"); return SSX_ERR_INVALID_ARG; }
    if (jobs[k].src_stride < cols || jobs[k].dst_stride < cols) {
      ctx->set_error("ssx_undistort: job %d has a stride (src %d, dst %d) smaller than cols = %d", k, jobs[k].src_stride, jobs[k].dst_stride, cols);
      return SSX_ERR_INVALID_ARG;
    }
  }
  for (int32_t d = 0; d < n; ++d) {
    uintptr_t d0, d1;
    ud_span(jobs[d].dst, jobs[d].dst_stride, rows, cols, &d0, &d1);
    for (int32_t s = 0; s < n; ++s) {
      uintptr_t s0, s1;
      ud_span(jobs[s].src, jobs[s].src_stride, rows, cols, &s0, &s1);
      if (d0 < s1 && s0 < d1) {
        ctx->set_error("ssx_undistort: the dst of job %d overlaps the src of job %d (there is no in-place form)", d, s);
        return SSX_ERR_INVALID_ARG;
      }
    }
  }
  if (rows > UD_MAX_SIDE || cols > UD_MAX_SIDE) { ctx->set_error("ssx_undistort: %d x %d is above %d a side", rows, cols, UD_MAX_SIDE); return SSX_ERR_UNSUPPORTED; }
  if (n == 0) return SSX_OK;

  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool staged = images_on_device == 0;
  // staged images are packed: sources at a pitch of cols, results at a pitch of cols rounded up to a dword (every store but the tail's is one)
  const size_t src_bytes = (size_t)rows * (size_t)cols, dpitch = ((size_t)cols + 3) & ~size_t(3), dst_bytes = (size_t)rows * dpitch;
  Layout lay;
  const size_t o_tab = lay.take(sizeof(UdJob) * (size_t)n);
  const size_t o_src = staged ? lay.take(src_bytes * (size_t)n) : 0;
  const size_t up_bytes = lay.off;
  const size_t o_dst = staged ? lay.take(dst_bytes * (size_t)n) : 0;
  SSX_HIP_TRY(ctx, ctx->ud_arena.reserve(lay.off));
  SSX_HIP_TRY(ctx, ctx->ud_stage.reserve(lay.off));
  char* dev = ctx->ud_arena.as<char>();
  char* stage = ctx->ud_stage.as<char>();
  KfChainStats st{};

  UdJob* tab = reinterpret_cast<UdJob*>(stage + o_tab);
  for (int32_t k = 0; k < n; ++k) {
    UdJob& t = tab[k];
    if (staged) {
      uint8_t* s = reinterpret_cast<uint8_t*>(stage + o_src + src_bytes * (size_t)k);
      for (int32_t r = 0; r < rows; ++r) std::memcpy(s + (size_t)r * cols, jobs[k].src + (size_t)r * jobs[k].src_stride, (size_t)cols);
      t.src = reinterpret_cast<const uint8_t*>(dev + o_src + src_bytes * (size_t)k);
      t.dst = reinterpret_cast<uint8_t*>(dev + o_dst + dst_bytes * (size_t)k);
      t.src_stride = cols; t.dst_stride = (int64_t)dpitch;
    } else {
      t.src = jobs[k].src; t.dst = jobs[k].dst;
      t.src_stride = jobs[k].src_stride; t.dst_stride = jobs[k].dst_stride;
    }
    std::memcpy(t.K, jobs[k].prm.K, sizeof(t.K));
    std::memcpy(t.dist, jobs[k].prm.dist, sizeof(t.dist));
    std::memcpy(t.iR, jobs[k].prm.iR, sizeof(t.iR));
  }
  SSX_HIP_TRY(ctx, hipMemcpyAsync(dev, stage, up_bytes, hipMemcpyHostToDevice, ctx->stream));
  st.bytes_up += (int64_t)up_bytes;
  const dim3 grid((unsigned)((cols + UD_BX * UD_PX - 1) / (UD_BX * UD_PX)), (unsigned)((rows + UD_BY - 1) / UD_BY), (unsigned)n);
  SSX_PROF(ctx, KID_UNDISTORT, hipLaunchKernelGGL(k_undistort, grid, dim3(UD_BX, UD_BY), 0, ctx->stream, reinterpret_cast<const UdJob*>(dev + o_tab), rows, cols));
  SSX_HIP_TRY(ctx, hipGetLastError());
  ++st.launches;
  if (staged) {
    SSX_HIP_TRY(ctx, hipMemcpyAsync(stage + o_dst, dev + o_dst, dst_bytes * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    st.bytes_down += (int64_t)(dst_bytes * (size_t)n);
  }
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ++st.syncs;
  if (staged)
    for (int32_t k = 0; k < n; ++k) {
      const uint8_t* d = reinterpret_cast<const uint8_t*>(stage + o_dst + dst_bytes * (size_t)k);
      for (int32_t r = 0; r < rows; ++r) std::memcpy(jobs[k].dst + (size_t)r * jobs[k].dst_stride, d + (size_t)r * dpitch, (size_t)cols);
    }
  ctx->undistort = st;
  return SSX_OK;
}

#ifndef SSX_NO_TEST_HOOKS   // include/ssx_test_hooks.h
ssx_status ssx_undistort_debug_last_call(ssx_ctx* ctx, int32_t* launches, int32_t* synchronisations, int64_t* bytes_up, int64_t* bytes_down)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  const KfChainStats& s = ctx->undistort;
  if (launches) *launches = s.launches;
  if (synchronisations) *synchronisations = s.syncs;
  if (bytes_up) *bytes_up = s.bytes_up;
  if (bytes_down) *bytes_down = s.bytes_down;
  return SSX_OK;
}
#endif

}  // extern "C"
