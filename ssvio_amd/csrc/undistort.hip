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
//                This is the single-pair path of the unbatched system.
//
// The batched form over many streams keeps the map (ssx_undistort_plan_*; profiles/undistort_plan/time.txt):
// k_undistort_map    once per camera: ud_map -- the f64 chain k_undistort calls too -- and the packing of the model's pack_map, three
//                    u16 per pixel.
// k_undistort_remap  the launch shape of k_undistort, no f64: a thread reads 8 bytes of each map plane and makes four pixels.  n jobs,
//                    whatever maps they name, are one launch.
// ssx_undistort_plan_apply  host images staged like ssx_undistort's; with images_on_device, host (pinned) images are copied by the DMA
//                    engines -- an arena's slices in ONE copy each way -- and the kernel runs device to device; device images are
//                    used where they lie.
//
// ssx_undistort  n jobs of one image size in ONE launch.  Host images: the job table and the sources go up in one copy (pinned staging),
//                the results come down in one copy, one synchronisation.  images_on_device: only the job table goes up, the kernel reads
//                and writes the images where they lie (device or pinned memory), nothing comes down.
//
// Lens models (contract tools/rectify_model.py): every job and every stored map names its lens, SSX_LENS_RADTAN -- the map
// above, and what ssx_undistort / ssx_undistort_plan_add pass -- or SSX_LENS_KB4 (Kannala-Brandt, its atan the contract's own f64
// operations: ud_atan).  The model is wave-uniform, so jobs of mixed models stay one launch.  ssx_stereo_rectify, the common rectified
// camera of a raw rig, is host arithmetic in this file because of the next sentence.
//
// This file is compiled with -ffp-contract=off: every f64 operation rounds on its own, as the model's does
// (tests/test_undistort_gpu.py, tests/test_rectify_gpu.py: the output is the model's bytes; tests/test_rectify_abi.py: ssx_stereo_rectify's
// are the model's bits).
#include <algorithm>
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
  int32_t model, reserved;                  // SSX_LENS_*: one lens a job, so the choice is wave-uniform too
  double K[4], coeffs[5], iR[9];
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

// atan_c of tools/rectify_model.py for r >= 0, in its operations and its order: the reduction at 7/16, 11/16, 19/16, 39/16 with the
// high / low constants, the 11-term odd polynomial in its two Horner halves.  The four reductions are selects of one quotient's
// operands, not branches: a wavefront's pixels lie on both sides of a breakpoint, and the one division rounds as the model's does
// because its operands are the model's.  No library atan.
__device__ __forceinline__ double ud_atan(double r)
{
  const bool c0 = r < 0.4375, c1 = r < 0.6875, c2 = r < 1.1875, c3 = r < 2.4375;
  const double n1 = 2.0 * r - 1.0, d1 = 2.0 + r;
  const double n2 = r - 1.0, d2 = r + 1.0;
  const double n3 = r - 1.5, d3 = 1.0 + 1.5 * r;
  const double num = c1 ? n1 : c2 ? n2 : c3 ? n3 : -1.0;
  const double den = c1 ? d1 : c2 ? d2 : c3 ? d3 : r;
  const double quo = num / den;
  const double t = c0 ? r : quo;
  const double hi = c1 ? 4.63647609000806093515e-01 : c2 ? 7.85398163397448278999e-01 : c3 ? 9.82793723247329054082e-01 : 1.57079632679489655800e+00;
  const double lo = c1 ? 2.26987774529616870924e-17 : c2 ? 3.06161699786838301793e-17 : c3 ? 1.39033110312309984516e-17 : 6.12323399573676603587e-17;
  const double z = t * t;
  const double w = z * z;
  const double s1 = z * (3.33333333333329318027e-01 + w * (1.42857142725034663711e-01 + w * (9.09088713343650656196e-02 + w * (6.66107313738753120669e-02 +
                         w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
  const double s2 = w * (-1.99999999998764832476e-01 + w * (-1.11111104054623557880e-01 + w * (-7.69187620504482999495e-02 + w * (-5.83357013379057348645e-02 +
                         w * -3.65315727442169155270e-02))));
  const double p = t * (s1 + s2);
  const double small = t - p;
  const double big = hi - ((p - lo) - t);
  double out = c0 ? small : big;
  if (r >= 73786976294838206464.0) out = 1.57079632679489655800e+00;   // 2^66
  if (r != r) out = r;
  return out;
}

// The map of the model up to its quantisation: the source position (iu, iv) of destination pixel (row i, column j) in 1/32 pixel, f64,
// one operation per statement in the model's order (tools/undistort_model.py for SSX_LENS_RADTAN, tools/rectify_model.py's lens_map for
// SSX_LENS_KB4).  `model` is wave-uniform -- a job's, or a launch's -- so the choice is a scalar branch and neither lens runs the
// other's chain.  k_undistort and k_undistort_map both call it: the inline map and the stored one cannot drift.
__device__ __forceinline__ void ud_map(int32_t model, const double* __restrict__ K, const double* __restrict__ dist, const double* __restrict__ iR, int32_t i,
                                       int32_t j, int32_t* iu_out, int32_t* iv_out)
{
  const double dj = (double)j, di = (double)i;
  const double X = (dj * iR[0] + di * iR[1]) + iR[2];
  const double Y = (dj * iR[3] + di * iR[4]) + iR[5];
  const double W = (dj * iR[6] + di * iR[7]) + iR[8];
  const double w = 1.0 / W;
  const double x = X * w;
  const double y = Y * w;
  if (model == SSX_LENS_KB4) {
    const double xx = x * x;
    const double yy = y * y;
    const double r2 = xx + yy;
    const double r = sqrt(r2);                                   // (f64 sqrt: correctly rounded)
    const double th = ud_atan(r);
    const double t2 = th * th;
    const double k1 = dist[0], k2 = dist[1], k3 = dist[2], k4 = dist[3];
    const double poly = 1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)));
    const double thd = th * poly;
    const double quo = thd / r;
    const double s = r == 0.0 ? 1.0 : quo;
    const double xs = x * s;
    const double ys = y * s;
    double u = K[0] * xs + K[2];
    double v = K[1] * ys + K[3];
    if (!(W > 0.0)) { u = -HUGE_VAL; v = -HUGE_VAL; }            // behind the camera, or NaN: every tap is outside
    *iu_out = ud_q(u * 32.0);
    *iv_out = ud_q(v * 32.0);
    return;
  }
  const double x2 = x * x;
  const double y2 = y * y;
  const double r2 = x2 + y2;
  const double _2xy = (2.0 * x) * y;
  const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
  const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
  const double xd = (x * kr + p1 * _2xy) + p2 * (r2 + 2.0 * x2);
  const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * _2xy;
  const double u = K[0] * xd + K[2];
  const double v = K[1] * yd + K[3];
  *iu_out = ud_q(u * 32.0);
  *iv_out = ud_q(v * 32.0);
}

// the four taps weighted with the 10-bit products of the 5-bit fractions a, b, as the model weighs them
__device__ __forceinline__ uint32_t ud_weigh(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, uint32_t a, uint32_t b)
{
  const uint32_t acc = (32u - a) * (32u - b) * p00 + a * (32u - b) * p01 + (32u - a) * b * p10 + a * b * p11;   // <= 1024 * 255
  return (acc + 512u) >> 10;
}

// the integer bilinear sample of the model at integer position (Y0, X0) with the 5-bit fractions a, b, each tap tested on its integer
// coordinates before its address is formed
__device__ __forceinline__ uint32_t ud_sample(const uint8_t* __restrict__ src, int64_t stride, int32_t rows, int32_t cols, int32_t Y0, int32_t X0, uint32_t a,
                                              uint32_t b)
{
  const uint32_t p00 = ud_tap(src, stride, rows, cols, Y0, X0);
  const uint32_t p01 = ud_tap(src, stride, rows, cols, Y0, X0 + 1);
  const uint32_t p10 = ud_tap(src, stride, rows, cols, Y0 + 1, X0);
  const uint32_t p11 = ud_tap(src, stride, rows, cols, Y0 + 1, X0 + 1);
  return ud_weigh(p00, p01, p10, p11, a, b);
}

// The four taps of k_undistort_remap at the stored position (xe, ye) = (X0 + 2, Y0 + 2).  The same tests on the integer coordinates
// as ud_tap's, two per axis and shared by the taps: as unsigned numbers X0 = -2, -1 lie far above cols, so `X0 < cols` is the whole test.
// Behind its test every tap gets its address: its own, or -- for a tap outside, whose byte is then dropped -- the image's first byte.
// No address outside the image is formed, and none of a thread's sixteen loads waits behind a branch.  The pointer is stated to be
// global memory, which a pointer read from the job table is not known to be.  (Measured, profiles/undistort_plan/time.txt: neither the
// branches nor the instruction count bound the kernel -- 447 instructions with ud_tap, 327 so, 292 with 32-bit offsets, one time.)
typedef const __attribute__((address_space(1))) uint8_t* UdGlobalBytes;
__device__ __forceinline__ uint32_t ud_tap_select(UdGlobalBytes src, int64_t at, bool inside)
{
  const uint32_t v = src[inside ? at : (int64_t)0];
  return inside ? v : 0u;
}
__device__ __forceinline__ uint32_t ud_sample_stored(UdGlobalBytes src, int64_t stride, uint32_t rows, uint32_t cols, uint32_t xe, uint32_t ye, uint32_t a, uint32_t b)
{
  const uint32_t X0 = xe - 2u, Y0 = ye - 2u;
  const bool x0 = X0 < cols, x1 = X0 + 1u < cols, y0 = Y0 < rows, y1 = Y0 + 1u < rows;
  const int64_t at = (int64_t)(int32_t)Y0 * stride + (int64_t)(int32_t)X0;
  const uint32_t p00 = ud_tap_select(src, at, y0 && x0);
  const uint32_t p01 = ud_tap_select(src, at + 1, y0 && x1);
  const uint32_t p10 = ud_tap_select(src, at + stride, y1 && x0);
  const uint32_t p11 = ud_tap_select(src, at + stride + 1, y1 && x1);
  return ud_weigh(p00, p01, p10, p11, a, b);
}

__device__ __forceinline__ uint32_t ud_pixel(const UdJob& jb, int32_t rows, int32_t cols, int32_t i, int32_t j)
{
  int32_t iu, iv;
  ud_map(jb.model, jb.K, jb.coeffs, jb.iR, i, j, &iu, &iv);
  const int32_t X0 = iu >> 5, Y0 = iv >> 5;                       // arithmetic shifts: |X0|, |Y0| <= 2^26, so X0 + 1 cannot overflow
  return ud_sample(jb.src, jb.src_stride, rows, cols, Y0, X0, (uint32_t)(iu & 31), (uint32_t)(iv & 31));
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

// ---- the stored map (ssx_undistort_plan) ----
// Three u16 planes (xs, ys, ab of tools/undistort_model.py's pack_map) of `rows` rows at a pitch of cols rounded up to UD_PX, one
// behind the other: a thread's four pixels are 8 aligned bytes of each plane, and a wavefront's loads are 512 consecutive bytes.
constexpr int UD_MAP_MAX_SIDE = 65533;      // position + 2 is a u16
struct UdPrm { int32_t model, reserved; double K[4], coeffs[5], iR[9]; };
static_assert(sizeof(UdPrm) == sizeof(ssx_lens_params), "the kernel's parameter block is the ABI's");

// grid (ceil(cols / 64), ceil(rows / 4)), block 64 x 4: one pixel a thread.  ud_map, then the packing of the model's pack_map.
__global__ void __launch_bounds__(UD_BX * UD_BY) k_undistort_map(UdPrm prm, int32_t rows, int32_t cols, int64_t pitch, uint16_t* __restrict__ map)
{
  const int32_t i = (int32_t)(blockIdx.y * UD_BY + threadIdx.y);
  const int32_t j = (int32_t)(blockIdx.x * UD_BX + threadIdx.x);
  if (i >= rows || j >= cols) return;
  int32_t iu, iv;
  ud_map(prm.model, prm.K, prm.coeffs, prm.iR, i, j, &iu, &iv);
  int32_t X0 = iu >> 5, Y0 = iv >> 5;
  X0 = X0 < -2 ? -2 : X0 > cols ? cols : X0;
  Y0 = Y0 < -2 ? -2 : Y0 > rows ? rows : Y0;
  const int64_t plane = (int64_t)rows * pitch, at = (int64_t)i * pitch + j;
  map[at] = (uint16_t)(X0 + 2);
  map[plane + at] = (uint16_t)(Y0 + 2);
  map[2 * plane + at] = (uint16_t)((iu & 31) | ((iv & 31) << 5));
}

#ifndef SSX_NO_TEST_HOOKS   // include/ssx_test_hooks.h: ssx_lens_debug_atan
__global__ void __launch_bounds__(256) k_lens_debug_atan(const double* __restrict__ r, int32_t n, double* __restrict__ atan_out, double* __restrict__ sqrt_out)
{
  const int32_t k = (int32_t)(blockIdx.x * 256u + threadIdx.x);
  if (k >= n) return;
  const double v = r[k];
  atan_out[k] = ud_atan(v);
  sqrt_out[k] = sqrt(v);
}
#endif

// one job of k_undistort_remap (wave-uniform: scalar loads)
struct UdRemapJob {
  const uint8_t* src;
  uint8_t* dst;
  int64_t src_stride, dst_stride;
  const uint16_t* map;
};

// grid (ceil(cols / 256), ceil(rows / 4), jobs), block 64 x 4, the shape of k_undistort: a thread makes four consecutive destination
// pixels from 8 bytes of each map plane and stores one dword (byte stores on the row tail and where the pitch leaves the address
// unaligned).  No f64, no LDS, no scratch.  Jobs that name the same map read the same 2.8 MB (1241 x 376): the cache serves them, a
// thread does not loop over jobs (profiles/undistort_plan/time.txt).  A stored position is a u16 and every tap is tested on its
// integer coordinates before its address is formed, so no map content can take a load outside the source image.  The kernel is bound
// by its sixteen byte gathers a thread, neither by memory traffic nor by instruction issue (profiles/undistort_plan/time.txt).
__global__ void __launch_bounds__(UD_BX * UD_BY) k_undistort_remap(const UdRemapJob* __restrict__ jobs, int32_t rows, int32_t cols, int64_t pitch)
{
  const int32_t i = (int32_t)(blockIdx.y * UD_BY + threadIdx.y);
  const int32_t j0 = (int32_t)((blockIdx.x * UD_BX + threadIdx.x) * UD_PX);
  if (i >= rows || j0 >= cols) return;
  const UdRemapJob& jb = jobs[blockIdx.z];
  const int64_t plane = (int64_t)rows * pitch, at = (int64_t)i * pitch + j0;       // (pitch is a multiple of UD_PX: `at` is, and the loads are aligned)
  typedef uint32_t __attribute__((ext_vector_type(2))) UdTwoWords;                  // four u16 entries
  typedef const __attribute__((address_space(1))) UdTwoWords* UdGlobalMap;
  const UdTwoWords xs = *(UdGlobalMap)(jb.map + at);
  const UdTwoWords ys = *(UdGlobalMap)(jb.map + plane + at);
  const UdTwoWords ab = *(UdGlobalMap)(jb.map + 2 * plane + at);
  const UdGlobalBytes src = (UdGlobalBytes)jb.src;
  const uint32_t xw[2] = {xs.x, xs.y}, yw[2] = {ys.x, ys.y}, fw[2] = {ab.x, ab.y};
  uint32_t px[UD_PX];
#pragma unroll
  for (int k = 0; k < UD_PX; ++k) {
    const int sh = 16 * (k & 1);
    const uint32_t f = (fw[k >> 1] >> sh) & 0xffffu;
    px[k] = ud_sample_stored(src, jb.src_stride, (uint32_t)rows, (uint32_t)cols, (xw[k >> 1] >> sh) & 0xffffu, (yw[k >> 1] >> sh) & 0xffffu, f & 31u, (f >> 5) & 31u);
  }
  uint8_t* out = jb.dst + (int64_t)i * jb.dst_stride + (int64_t)j0;
  if (j0 + UD_PX <= cols && (reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
    *reinterpret_cast<uint32_t*>(out) = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
  } else {
#pragma unroll
    for (int k = 0; k < UD_PX; ++k)
      if (j0 + k < cols) out[k] = (uint8_t)px[k];
  }
}

// [first, last) of an image in memory: from its pointer to the end of its last row
inline void ud_span(const uint8_t* p, int64_t stride, int32_t rows, int32_t cols, uintptr_t* first, uintptr_t* last)
{
  *first = reinterpret_cast<uintptr_t>(p);
  *last = *first + (uintptr_t)((int64_t)(rows - 1) * stride + cols);
}

inline size_t ud_bytes(int32_t stride, int32_t rows, int32_t cols) { return (size_t)((int64_t)(rows - 1) * stride + cols); }

// does a dst of the call overlap a src of the call?  Sorted sources and the furthest end among those that begin no later: n log n for
// the call that is accepted; the pair of a refused call is then found in job order, as ssx_undistort names it
bool ud_find_overlap(int32_t n, const ssx_undistort_plan_job* jobs, int32_t rows, int32_t cols, int32_t* d_out, int32_t* s_out)
{
  struct Iv { uintptr_t a, b; };
  std::vector<Iv> src((size_t)std::max(n, 0));
  for (int32_t k = 0; k < n; ++k) ud_span(jobs[k].src, jobs[k].src_stride, rows, cols, &src[k].a, &src[k].b);
  std::sort(src.begin(), src.end(), [](const Iv& x, const Iv& y) { return x.a < y.a; });
  for (size_t k = 1; k < src.size(); ++k) src[k].b = std::max(src[k].b, src[k - 1].b);
  bool any = false;
  for (int32_t d = 0; d < n && !any; ++d) {
    uintptr_t d0, d1;
    ud_span(jobs[d].dst, jobs[d].dst_stride, rows, cols, &d0, &d1);
    const size_t cnt = (size_t)(std::lower_bound(src.begin(), src.end(), d1, [](const Iv& x, uintptr_t v) { return x.a < v; }) - src.begin());
    any = cnt > 0 && src[cnt - 1].b > d0;
  }
  if (!any) return false;
  for (int32_t d = 0; d < n; ++d) {
    uintptr_t d0, d1;
    ud_span(jobs[d].dst, jobs[d].dst_stride, rows, cols, &d0, &d1);
    for (int32_t s = 0; s < n; ++s) {
      uintptr_t s0, s1;
      ud_span(jobs[s].src, jobs[s].src_stride, rows, cols, &s0, &s1);
      if (d0 < s1 && s0 < d1) { *d_out = d; *s_out = s; return true; }
    }
  }
  return false;
}

// Where the images of one side of an images_on_device call lie (the sources, or the results), asked of the runtime: look-ups in its
// table of allocations, no copy, no launch, no synchronisation.
//   range    host images that go in ONE copy: in job order ascending, each at least one image behind the last, the whole no longer
//            than twice the images, and -- the runtime's word, arithmetic is not enough: images allocated one by one can stand just
//            like that, and one copy over them would cross whatever lies between two allocations -- in ONE allocation (choose_intake
//            and lk_facts of lk.hip).  Results also stand at one constant distance and at a stride of cols: the 2-D copy that brings
//            them down then writes the images and nothing between them.
//   host[k]  otherwise: image k is pinned host memory (a copy of its own) or device memory (used where it lies)
struct UdImage { const uint8_t* p; int32_t stride; };
struct UdSide {
  bool range = false;
  size_t range_bytes = 0, distance = 0;
  std::vector<char> host;
};

// 1: host memory the runtime knows (pinned), 0: device memory, -1: neither
int ud_kind(const void* p)
{
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
  if (at.type == hipMemoryTypeHost) return 1;
  if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged) return 0;
  return -1;
}

bool ud_classify(const std::vector<UdImage>& im, int32_t rows, int32_t cols, bool results, UdSide& side, int32_t* bad)
{
  const size_t n = im.size();
  side = UdSide{};
  side.host.assign(n, 0);
  size_t longest = 0;
  for (const UdImage& i : im) longest = std::max(longest, ud_bytes(i.stride, rows, cols));
  bool ok = n >= 2;
  for (size_t k = 1; ok && k < n; ++k) ok = im[k].p > im[k - 1].p && (size_t)(im[k].p - im[k - 1].p) >= ud_bytes(im[k - 1].stride, rows, cols);
  const size_t range = ok ? (size_t)(im[n - 1].p - im[0].p) + ud_bytes(im[n - 1].stride, rows, cols) : 0;
  ok = ok && range <= 2 * n * longest;
  if (ok && results) {
    side.distance = (size_t)(im[1].p - im[0].p);
    for (size_t k = 0; ok && k < n; ++k) ok = im[k].stride == cols && (k == 0 || (size_t)(im[k].p - im[k - 1].p) == side.distance);
  }
  if (ok) {
    const uint8_t* const last_end = im[n - 1].p + ud_bytes(im[n - 1].stride, rows, cols);
    hipDeviceptr_t base0 = nullptr, base1 = nullptr;
    size_t size0 = 0, size1 = 0;
    const bool one = hipMemGetAddressRange(&base0, &size0, (hipDeviceptr_t)im[0].p) == hipSuccess &&
                     hipMemGetAddressRange(&base1, &size1, (hipDeviceptr_t)im[n - 1].p) == hipSuccess && base0 == base1 &&
                     (const uint8_t*)base0 <= im[0].p && last_end <= (const uint8_t*)base0 + size0;
    if (!one) (void)hipGetLastError();
    if (one) {
      const int kind = ud_kind(im[0].p);
      if (kind < 0) { *bad = 0; return false; }
      if (kind == 1) { side.range = true; side.range_bytes = range; }
      return true;                                                             // (one device allocation: every image where it lies)
    }
  }
  for (size_t k = 0; k < n; ++k) {
    const int kind = ud_kind(im[k].p);
    if (kind < 0) { *bad = (int32_t)k; return false; }
    side.host[k] = kind == 1;
  }
  return true;
}

// what a plan's last call issued (ssx_undistort_plan_debug_last_call)
struct UdPlanStats { int32_t launches = 0, syncs = 0, copies_up = 0, copies_down = 0; int64_t bytes_up = 0, bytes_down = 0; };

}  // namespace

// the stored maps of one image size, and the device block and the pinned staging of the calls that apply them
struct ssx_undistort_plan {
  ssx_ctx* ctx = nullptr;
  int32_t rows = 0, cols = 0;
  int64_t pitch = 0;                          // entries of a map row: cols rounded up to UD_PX
  size_t map_bytes = 0;                       // three planes
  std::vector<ssx_lens_params> prm;           // prm[m]: the parameter bytes of maps[m] (a set of ssx_undistort_plan_add: as its RADTAN lens)
  std::vector<uint16_t*> maps;
  DevBuf arena;
  HostBuf stage;
  UdPlanStats last;
};

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

}  // extern "C"

namespace {

inline bool ud_known_model(int32_t model) { return model == SSX_LENS_RADTAN || model == SSX_LENS_KB4; }

// the RADTAN lens that a parameter set of ssx_undistort is: the same bytes whichever entry point it came through
inline ssx_lens_params ud_as_lens(const ssx_undistort_params& p)
{
  ssx_lens_params l;
  std::memset(&l, 0, sizeof l);
  l.model = SSX_LENS_RADTAN;
  std::memcpy(l.K, p.K, sizeof l.K);
  std::memcpy(l.coeffs, p.dist, sizeof l.coeffs);
  std::memcpy(l.iR, p.iR, sizeof l.iR);
  return l;
}

// ssx_undistort_lens, and ssx_undistort as its RADTAN case; `who` names the entry point in the messages
ssx_status ud_run(ssx_ctx* ctx, const char* who, int32_t n, const ssx_lens_job* jobs, int32_t rows, int32_t cols, int32_t images_on_device)
{
  ctx->undistort = KfChainStats{};
  // every refusal comes before anything is touched
  if (n < 0 || n > SSX_UNDISTORT_MAX_JOBS) { ctx->set_error("%s: n = %d outside [0, %d]", who, n, SSX_UNDISTORT_MAX_JOBS); return SSX_ERR_INVALID_ARG; }
  if (rows < 1 || cols < 1) { ctx->set_error("%s: rows = %d, cols = %d (both must be >= 1)", who, rows, cols); return SSX_ERR_INVALID_ARG; }
  if (n > 0 && !jobs) { ctx->set_error("%s: jobs is null", who); return SSX_ERR_INVALID_ARG; }
  for (int32_t k = 0; k < n; ++k) {
    if (!jobs[k].src || !jobs[k].dst) { ctx->set_error("%s: job %d has a null %s", who, k, jobs[k].src ? "dst" : "src"); return SSX_ERR_INVALID_ARG; }
    if (jobs[k].src_stride < cols || jobs[k].dst_stride < cols) {
      ctx->set_error("%s: job %d has a stride (src %d, dst %d) smaller than cols = %d", who, k, jobs[k].src_stride, jobs[k].dst_stride, cols);
      return SSX_ERR_INVALID_ARG;
    }
    if (!ud_known_model(jobs[k].prm.model)) {
      ctx->set_error("%s: job %d names lens model %d (SSX_LENS_RADTAN = 0, SSX_LENS_KB4 = 1)", who, k, jobs[k].prm.model);
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
        ctx->set_error("%s: the dst of job %d overlaps the src of job %d (there is no in-place form)", who, d, s);
        return SSX_ERR_INVALID_ARG;
      }
    }
  }
  if (rows > UD_MAX_SIDE || cols > UD_MAX_SIDE) { ctx->set_error("%s: %d x %d is above %d a side", who, rows, cols, UD_MAX_SIDE); return SSX_ERR_UNSUPPORTED; }
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
    t.model = jobs[k].prm.model; t.reserved = 0;
    std::memcpy(t.K, jobs[k].prm.K, sizeof(t.K));
    std::memcpy(t.coeffs, jobs[k].prm.coeffs, sizeof(t.coeffs));
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

// ssx_undistort_plan_add_lens, and ssx_undistort_plan_add as its RADTAN case (definition below the plan's entry points)
ssx_status ud_plan_add(ssx_undistort_plan* plan, const char* who, const ssx_lens_params* prm, int32_t* map_index);

// ---- ssx_stereo_rectify: rectify() of tools/rectify_model.py, statement for statement (host f64, this file has no contraction) ----
const char* const UD_WHY_MODEL = "unknown lens model";
const char* const UD_WHY_FINITE = "a non-finite input";
const char* const UD_WHY_BASELINE = "the baseline is zero";
const char* const UD_WHY_ROTATION = "R is not a rotation: max|R R^T - I| > 1e-6";
const char* const UD_WHY_SIDE = "the right camera is not to the right of the left one (e1[0] <= 0)";
const char* const UD_WHY_AXES = "the optical axes lie along the baseline (|e3'|^2 < 1e-12)";

inline bool ud_all_finite(const double* v, int n)
{
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

// iR = S^T newK^-1 in closed form; in the third column the left-most product is taken first
inline void ud_rect_iR(const double S[9], double f, double cx, double cy, double iR[9])
{
  const double g = 1.0 / f;
  const double mx = -cx / f;
  const double my = -cy / f;
  for (int i = 0; i < 3; ++i) {
    iR[3 * i + 0] = S[0 + i] * g;
    iR[3 * i + 1] = S[3 + i] * g;
    const double a = S[0 + i] * mx;
    const double b = S[3 + i] * my;
    const double ab = a + b;
    iR[3 * i + 2] = ab + S[6 + i];
  }
}

// -> nullptr and *o filled, or the model's reason and *o untouched
const char* ud_rectify(const ssx_stereo_raw_rig& rig, ssx_stereo_rectified* o)
{
  for (int s = 0; s < 2; ++s)
    if (!ud_known_model(rig.cam[s].model)) return UD_WHY_MODEL;
  const double over[3] = {rig.f, rig.cx, rig.cy};
  bool fin = ud_all_finite(rig.R, 9) && ud_all_finite(rig.t, 3) && ud_all_finite(over, 3);
  for (int s = 0; s < 2; ++s) fin = fin && ud_all_finite(rig.cam[s].K, 4) && ud_all_finite(rig.cam[s].coeffs, 5);
  if (!fin) return UD_WHY_FINITE;
  const double* R = rig.R;
  const double* t = rig.t;
  double c[3];
  for (int i = 0; i < 3; ++i) {
    const double a0 = (-R[0 + i]) * t[0];
    const double a1 = (-R[3 + i]) * t[1];
    const double a2 = (-R[6 + i]) * t[2];
    const double a01 = a0 + a1;
    c[i] = a01 + a2;
  }
  const double c00 = c[0] * c[0], c11 = c[1] * c[1], c22 = c[2] * c[2];
  const double cc = c00 + c11;
  const double b = std::sqrt(cc + c22);
  if (b == 0.0) return UD_WHY_BASELINE;
  double worst = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double p0 = R[3 * i + 0] * R[3 * j + 0], p1 = R[3 * i + 1] * R[3 * j + 1], p2 = R[3 * i + 2] * R[3 * j + 2];
      const double p01 = p0 + p1;
      const double dot = p01 + p2;
      const double dev = std::fabs(dot - (i == j ? 1.0 : 0.0));
      if (dev > worst) worst = dev;
    }
  if (worst > 1e-6) return UD_WHY_ROTATION;
  double e1[3], e2[3], e3[3], e3p[3];
  for (int i = 0; i < 3; ++i) e1[i] = c[i] / b;
  if (e1[0] <= 0.0) return UD_WHY_SIDE;
  const double zm[3] = {0.0 + R[6], 0.0 + R[7], 1.0 + R[8]};
  const double d0 = zm[0] * e1[0], d1 = zm[1] * e1[1], d2 = zm[2] * e1[2];
  const double d01 = d0 + d1;
  const double d = d01 + d2;
  for (int i = 0; i < 3; ++i) {
    const double de = d * e1[i];
    e3p[i] = zm[i] - de;
  }
  const double q0 = e3p[0] * e3p[0], q1 = e3p[1] * e3p[1], q2 = e3p[2] * e3p[2];
  const double q01 = q0 + q1;
  const double n2 = q01 + q2;
  if (n2 < 1e-12) return UD_WHY_AXES;
  const double nn = std::sqrt(n2);
  for (int i = 0; i < 3; ++i) e3[i] = e3p[i] / nn;
  {
    const double a0 = e3[1] * e1[2], b0 = e3[2] * e1[1];
    const double a1 = e3[2] * e1[0], b1 = e3[0] * e1[2];
    const double a2 = e3[0] * e1[1], b2 = e3[1] * e1[0];
    e2[0] = a0 - b0; e2[1] = a1 - b1; e2[2] = a2 - b2;
  }
  ssx_stereo_rectified r;
  std::memset(&r, 0, sizeof r);
  for (int i = 0; i < 3; ++i) { r.R_l[i] = e1[i]; r.R_l[3 + i] = e2[i]; r.R_l[6 + i] = e3[i]; }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double p0 = r.R_l[3 * i + 0] * R[3 * j + 0], p1 = r.R_l[3 * i + 1] * R[3 * j + 1], p2 = r.R_l[3 * i + 2] * R[3 * j + 2];
      const double p01 = p0 + p1;
      r.R_r[3 * i + j] = p01 + p2;
    }
  const double* Kl = rig.cam[0].K;
  const double* Kr = rig.cam[1].K;
  double f = rig.f, cx = rig.cx, cy = rig.cy;
  if (f == 0.0) {
    const double sl = Kl[0] + Kl[1], sr = Kr[0] + Kr[1];
    const double s4 = sl + sr;
    f = s4 / 4.0;
  }
  if (cx == 0.0) { const double s2 = Kl[2] + Kr[2]; cx = s2 / 2.0; }
  if (cy == 0.0) { const double s2 = Kl[3] + Kr[3]; cy = s2 / 2.0; }
  r.newK[0] = f; r.newK[1] = f; r.newK[2] = cx; r.newK[3] = cy;
  r.baseline = b;
  for (int s = 0; s < 2; ++s) {
    r.cam[s].model = rig.cam[s].model;                               // (reserved stays 0: equal lenses are equal bytes)
    std::memcpy(r.cam[s].K, rig.cam[s].K, sizeof r.cam[s].K);
    std::memcpy(r.cam[s].coeffs, rig.cam[s].coeffs, sizeof r.cam[s].coeffs);
    ud_rect_iR(s == 0 ? r.R_l : r.R_r, f, cx, cy, r.cam[s].iR);
  }
  *o = r;
  return nullptr;
}

}  // namespace

extern "C" {

ssx_status ssx_undistort_lens(ssx_ctx* ctx, int32_t n, const ssx_lens_job* jobs, int32_t rows, int32_t cols, int32_t images_on_device)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  return ud_run(ctx, "ssx_undistort_lens", n, jobs, rows, cols, images_on_device);
}

ssx_status ssx_undistort(ssx_ctx* ctx, int32_t n, const ssx_undistort_job* jobs, int32_t rows, int32_t cols, int32_t images_on_device)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  std::vector<ssx_lens_job> lens;                                    // (a count or a table that will be refused goes through as it is)
  if (jobs && n > 0 && n <= SSX_UNDISTORT_MAX_JOBS) {
    lens.resize((size_t)n);
    for (int32_t k = 0; k < n; ++k) lens[k] = ssx_lens_job{jobs[k].src, jobs[k].src_stride, jobs[k].dst, jobs[k].dst_stride, ud_as_lens(jobs[k].prm)};
  }
  return ud_run(ctx, "ssx_undistort", n, lens.empty() ? nullptr : lens.data(), rows, cols, images_on_device);
}

ssx_status ssx_stereo_rectify(const ssx_stereo_raw_rig* rig, ssx_stereo_rectified* out, char* why, int32_t why_cap)
{
  const char* reason = !rig ? "rig is null" : !out ? "out is null" : ud_rectify(*rig, out);
  if (why && why_cap > 0) {
    std::strncpy(why, reason ? reason : "", (size_t)why_cap);
    why[why_cap - 1] = '\0';
  }
  return reason ? SSX_ERR_INVALID_ARG : SSX_OK;
}

// ---- the plan: stored maps of one image size, applied to n images in one launch ----

ssx_status ssx_undistort_plan_create(ssx_ctx* ctx, int32_t rows, int32_t cols, ssx_undistort_plan** plan)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  if (!plan) { ctx->set_error("ssx_undistort_plan_create: plan is null"); return SSX_ERR_INVALID_ARG; }
  *plan = nullptr;
  if (rows < 1 || cols < 1) { ctx->set_error("ssx_undistort_plan_create: rows = %d, cols = %d (both must be >= 1)", rows, cols); return SSX_ERR_INVALID_ARG; }
  if (rows > UD_MAP_MAX_SIDE || cols > UD_MAP_MAX_SIDE) {
    ctx->set_error("ssx_undistort_plan_create: %d x %d is above %d a side (a stored position + 2 is a u16)", rows, cols, UD_MAP_MAX_SIDE);
    return SSX_ERR_UNSUPPORTED;
  }
  ssx_undistort_plan* p = new ssx_undistort_plan();
  p->ctx = ctx; p->rows = rows; p->cols = cols;
  p->pitch = ((int64_t)cols + UD_PX - 1) / UD_PX * UD_PX;
  p->map_bytes = (size_t)3 * (size_t)rows * (size_t)p->pitch * sizeof(uint16_t);
  *plan = p;
  return SSX_OK;
}

void ssx_undistort_plan_destroy(ssx_undistort_plan* plan)
{
  if (!plan) return;
  (void)hipSetDevice(plan->ctx->device);
  for (uint16_t* m : plan->maps) (void)hipFree(m);
  plan->arena.release();
  plan->stage.release();
  delete plan;
}

ssx_status ssx_undistort_plan_size(const ssx_undistort_plan* plan, int32_t* rows, int32_t* cols, int32_t* n_maps)
{
  if (!plan) return SSX_ERR_INVALID_ARG;
  if (rows) *rows = plan->rows;
  if (cols) *cols = plan->cols;
  if (n_maps) *n_maps = (int32_t)plan->maps.size();
  return SSX_OK;
}

ssx_status ssx_undistort_plan_add(ssx_undistort_plan* plan, const ssx_undistort_params* prm, int32_t* map_index)
{
  if (!plan) return SSX_ERR_INVALID_ARG;
  ssx_lens_params lens;
  if (prm) lens = ud_as_lens(*prm);
  return ud_plan_add(plan, "ssx_undistort_plan_add", prm ? &lens : nullptr, map_index);
}

ssx_status ssx_undistort_plan_add_lens(ssx_undistort_plan* plan, const ssx_lens_params* prm, int32_t* map_index)
{
  if (!plan) return SSX_ERR_INVALID_ARG;
  return ud_plan_add(plan, "ssx_undistort_plan_add_lens", prm, map_index);
}

}  // extern "C"

namespace {

ssx_status ud_plan_add(ssx_undistort_plan* plan, const char* who, const ssx_lens_params* prm, int32_t* map_index)
{
  ssx_ctx* ctx = plan->ctx;
  plan->last = UdPlanStats{};
  if (!prm || !map_index) { ctx->set_error("%s: %s is null", who, prm ? "map_index" : "prm"); return SSX_ERR_INVALID_ARG; }
  if (!ud_known_model(prm->model)) {
    ctx->set_error("%s: lens model %d (SSX_LENS_RADTAN = 0, SSX_LENS_KB4 = 1)", who, prm->model);
    return SSX_ERR_INVALID_ARG;
  }
  // (parameter sets are equal when their bytes are: -0.0 and 0.0, or two NaNs, are different sets with equal maps, which costs a map and
  // no more)
  for (size_t m = 0; m < plan->prm.size(); ++m)
    if (std::memcmp(&plan->prm[m], prm, sizeof *prm) == 0) { *map_index = (int32_t)m; return SSX_OK; }
  if (plan->maps.size() >= SSX_UNDISTORT_PLAN_MAX_MAPS) {
    ctx->set_error("%s: the plan holds SSX_UNDISTORT_PLAN_MAX_MAPS = %d maps already", who, SSX_UNDISTORT_PLAN_MAX_MAPS);
    return SSX_ERR_CAPACITY;
  }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint16_t* map = nullptr;
  SSX_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&map), plan->map_bytes));
  UdPrm k;
  std::memcpy(&k, prm, sizeof k);
  const dim3 grid((unsigned)((plan->cols + UD_BX - 1) / UD_BX), (unsigned)((plan->rows + UD_BY - 1) / UD_BY), 1u);
  hipError_t e = hipMemsetAsync(map, 0, plan->map_bytes, ctx->stream);         // (the pitch columns: read by a row's last thread, never used)
  if (e == hipSuccess) {
    SSX_PROF(ctx, KID_UNDISTORT_MAP, hipLaunchKernelGGL(k_undistort_map, grid, dim3(UD_BX, UD_BY), 0, ctx->stream, k, plan->rows, plan->cols, plan->pitch, map));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    (void)hipFree(map);
    ctx->set_error("%s: %s", who, hipGetErrorString(e));
    return SSX_ERR_HIP;
  }
  plan->last.launches = 1; plan->last.syncs = 1;
  plan->maps.push_back(map);
  plan->prm.push_back(*prm);
  *map_index = (int32_t)plan->maps.size() - 1;
  return SSX_OK;
}

}  // namespace

extern "C" {

ssx_status ssx_undistort_plan_apply(ssx_undistort_plan* plan, int32_t n, const ssx_undistort_plan_job* jobs, int32_t images_on_device)
{
  if (!plan) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = plan->ctx;
  const int32_t rows = plan->rows, cols = plan->cols;
  plan->last = UdPlanStats{};
  // every refusal comes before anything is touched
  if (n < 0 || n > SSX_UNDISTORT_MAX_JOBS) { ctx->set_error("ssx_undistort_plan_apply: n = %d outside [0, %d]", n, SSX_UNDISTORT_MAX_JOBS); return SSX_ERR_INVALID_ARG; }
  if (n > 0 && !jobs) { ctx->set_error("ssx_undistort_plan_apply: jobs is null"); return SSX_ERR_INVALID_ARG; }
  for (int32_t k = 0; k < n; ++k) {
    if (!jobs[k].src || !jobs[k].dst) { ctx->set_error("ssx_undistort_plan_apply: job %d has a null %s", k, jobs[k].src ? "dst" : "src"); return SSX_ERR_INVALID_ARG; }
    if (jobs[k].src_stride < cols || jobs[k].dst_stride < cols) {
      ctx->set_error("ssx_undistort_plan_apply: job %d has a stride (src %d, dst %d) smaller than cols = %d", k, jobs[k].src_stride, jobs[k].dst_stride, cols);
      return SSX_ERR_INVALID_ARG;
    }
    if (jobs[k].map < 0 || (size_t)jobs[k].map >= plan->maps.size()) {
      ctx->set_error("ssx_undistort_plan_apply: job %d names map %d, the plan holds %d", k, jobs[k].map, (int)plan->maps.size());
      return SSX_ERR_INVALID_ARG;
    }
  }
  {
    int32_t d = 0, s = 0;
    if (ud_find_overlap(n, jobs, rows, cols, &d, &s)) {
      ctx->set_error("ssx_undistort_plan_apply: the dst of job %d overlaps the src of job %d (there is no in-place form)", d, s);
      return SSX_ERR_INVALID_ARG;
    }
  }
  if (n == 0) return SSX_OK;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool staged = images_on_device == 0;
  UdSide src_side, dst_side;
  if (!staged) {
    std::vector<UdImage> si((size_t)n), di((size_t)n);
    for (int32_t k = 0; k < n; ++k) { si[k] = {jobs[k].src, jobs[k].src_stride}; di[k] = {jobs[k].dst, jobs[k].dst_stride}; }
    int32_t bad = -1;
    if (!ud_classify(si, rows, cols, false, src_side, &bad)) {
      ctx->set_error("ssx_undistort_plan_apply: the src of job %d is neither device memory nor pinned host memory (images_on_device = %d)", bad, images_on_device);
      return SSX_ERR_INVALID_ARG;
    }
    if (!ud_classify(di, rows, cols, true, dst_side, &bad)) {
      ctx->set_error("ssx_undistort_plan_apply: the dst of job %d is neither device memory nor pinned host memory (images_on_device = %d)", bad, images_on_device);
      return SSX_ERR_INVALID_ARG;
    }
  }

  // the device block: [job table | sources] | results.  Staged images are packed: sources at a pitch of cols, results at a pitch of
  // cols rounded up to a dword.  Host images of images_on_device: the sources of a range keep the range's layout (one copy), other
  // host sources stand one by one at their own stride; the results of a range are images of rows * cols bytes at a stride of cols (one
  // 2-D copy: a row of it is an image), other host results stand one by one at the dword pitch.
  const size_t img_bytes = (size_t)rows * (size_t)cols, dpitch = ((size_t)cols + 3) & ~size_t(3), dst_bytes = (size_t)rows * dpitch;
  const size_t range_img = (img_bytes + 255) & ~size_t(255);
  Layout lay;
  const size_t o_tab = lay.take(sizeof(UdRemapJob) * (size_t)n);
  std::vector<size_t> o_src((size_t)n, 0), o_dst((size_t)n, 0);
  if (staged) {
    for (int32_t k = 0; k < n; ++k) o_src[k] = lay.take(img_bytes);
  } else if (src_side.range) {
    const size_t base = lay.take(src_side.range_bytes + 16);
    for (int32_t k = 0; k < n; ++k) o_src[k] = base + (size_t)(jobs[k].src - jobs[0].src);
  } else {
    for (int32_t k = 0; k < n; ++k) if (src_side.host[k]) o_src[k] = lay.take(ud_bytes(jobs[k].src_stride, rows, cols));
  }
  const size_t up_bytes = lay.off;                                              // (staged: what the one copy up carries)
  const size_t o_dst0 = lay.off;
  if (staged) {
    for (int32_t k = 0; k < n; ++k) o_dst[k] = lay.take(dst_bytes);
  } else if (dst_side.range) {
    for (int32_t k = 0; k < n; ++k) o_dst[k] = lay.take(range_img);
  } else {
    for (int32_t k = 0; k < n; ++k) if (dst_side.host[k]) o_dst[k] = lay.take(dst_bytes);
  }
  SSX_HIP_TRY(ctx, plan->arena.reserve(lay.off));
  SSX_HIP_TRY(ctx, plan->stage.reserve(staged ? lay.off : o_tab + sizeof(UdRemapJob) * (size_t)n));
  char* dev = plan->arena.as<char>();
  char* stage = plan->stage.as<char>();
  hipStream_t s = ctx->stream;
  UdPlanStats st{};

  UdRemapJob* tab = reinterpret_cast<UdRemapJob*>(stage + o_tab);
  for (int32_t k = 0; k < n; ++k) {
    UdRemapJob& t = tab[k];
    t.map = plan->maps[(size_t)jobs[k].map];
    if (staged) {
      uint8_t* h = reinterpret_cast<uint8_t*>(stage + o_src[k]);
      for (int32_t r = 0; r < rows; ++r) std::memcpy(h + (size_t)r * cols, jobs[k].src + (size_t)r * jobs[k].src_stride, (size_t)cols);
      t.src = reinterpret_cast<const uint8_t*>(dev + o_src[k]); t.src_stride = cols;
      t.dst = reinterpret_cast<uint8_t*>(dev + o_dst[k]); t.dst_stride = (int64_t)dpitch;
      continue;
    }
    const bool sh = src_side.range || src_side.host[k], dh = dst_side.range || dst_side.host[k];
    t.src = sh ? reinterpret_cast<const uint8_t*>(dev + o_src[k]) : jobs[k].src;
    t.src_stride = jobs[k].src_stride;
    t.dst = dh ? reinterpret_cast<uint8_t*>(dev + o_dst[k]) : jobs[k].dst;
    t.dst_stride = !dh ? (int64_t)jobs[k].dst_stride : dst_side.range ? (int64_t)cols : (int64_t)dpitch;
  }
  if (staged) {
    SSX_HIP_TRY(ctx, hipMemcpyAsync(dev, stage, up_bytes, hipMemcpyHostToDevice, s));
    st.bytes_up += (int64_t)up_bytes; ++st.copies_up;
  } else {
    const size_t tab_bytes = sizeof(UdRemapJob) * (size_t)n;
    SSX_HIP_TRY(ctx, hipMemcpyAsync(dev + o_tab, stage + o_tab, tab_bytes, hipMemcpyHostToDevice, s));
    st.bytes_up += (int64_t)tab_bytes;
    if (src_side.range) {
      SSX_HIP_TRY(ctx, hipMemcpyAsync(dev + o_src[0], jobs[0].src, src_side.range_bytes, hipMemcpyHostToDevice, s));
      st.bytes_up += (int64_t)src_side.range_bytes; ++st.copies_up;
    } else {
      for (int32_t k = 0; k < n; ++k) {
        if (!src_side.host[k]) continue;
        const size_t b = ud_bytes(jobs[k].src_stride, rows, cols);
        SSX_HIP_TRY(ctx, hipMemcpyAsync(dev + o_src[k], jobs[k].src, b, hipMemcpyHostToDevice, s));
        st.bytes_up += (int64_t)b; ++st.copies_up;
      }
    }
  }
  const dim3 grid((unsigned)((cols + UD_BX * UD_PX - 1) / (UD_BX * UD_PX)), (unsigned)((rows + UD_BY - 1) / UD_BY), (unsigned)n);
  SSX_PROF(ctx, KID_UNDISTORT_REMAP, hipLaunchKernelGGL(k_undistort_remap, grid, dim3(UD_BX, UD_BY), 0, s, reinterpret_cast<const UdRemapJob*>(dev + o_tab), rows, cols, plan->pitch));
  SSX_HIP_TRY(ctx, hipGetLastError());
  ++st.launches;
  if (staged) {
    const size_t down = lay.off - o_dst0;
    SSX_HIP_TRY(ctx, hipMemcpyAsync(stage + o_dst0, dev + o_dst0, down, hipMemcpyDeviceToHost, s));
    st.bytes_down += (int64_t)down; ++st.copies_down;
  } else if (dst_side.range) {
    // a row of the copy is an image: rows * cols bytes, `distance` apart on the host -- nothing between the images is written
    SSX_HIP_TRY(ctx, hipMemcpy2DAsync(jobs[0].dst, dst_side.distance, dev + o_dst[0], range_img, img_bytes, (size_t)n, hipMemcpyDeviceToHost, s));
    st.bytes_down += (int64_t)(img_bytes * (size_t)n); ++st.copies_down;
  } else {
    for (int32_t k = 0; k < n; ++k) {
      if (!dst_side.host[k]) continue;                                          // (rows of cols bytes: the pitch bytes of the destination stay)
      SSX_HIP_TRY(ctx, hipMemcpy2DAsync(jobs[k].dst, (size_t)jobs[k].dst_stride, dev + o_dst[k], dpitch, (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost, s));
      st.bytes_down += (int64_t)img_bytes; ++st.copies_down;
    }
  }
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  ++st.syncs;
  if (staged)
    for (int32_t k = 0; k < n; ++k) {
      const uint8_t* d = reinterpret_cast<const uint8_t*>(stage + o_dst[k]);
      for (int32_t r = 0; r < rows; ++r) std::memcpy(jobs[k].dst + (size_t)r * jobs[k].dst_stride, d + (size_t)r * dpitch, (size_t)cols);
    }
  plan->last = st;
  return SSX_OK;
}

#ifndef SSX_NO_TEST_HOOKS   // include/ssx_test_hooks.h
ssx_status ssx_undistort_plan_debug_last_call(const ssx_undistort_plan* plan, int32_t* launches, int32_t* synchronisations, int64_t* bytes_up, int64_t* bytes_down,
                                              int32_t* copies_up, int32_t* copies_down)
{
  if (!plan) return SSX_ERR_INVALID_ARG;
  const UdPlanStats& s = plan->last;
  if (launches) *launches = s.launches;
  if (synchronisations) *synchronisations = s.syncs;
  if (bytes_up) *bytes_up = s.bytes_up;
  if (bytes_down) *bytes_down = s.bytes_down;
  if (copies_up) *copies_up = s.copies_up;
  if (copies_down) *copies_down = s.copies_down;
  return SSX_OK;
}

ssx_status ssx_undistort_plan_debug_map(ssx_undistort_plan* plan, int32_t map_index, uint16_t* out)
{
  if (!plan) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = plan->ctx;
  if (!out || map_index < 0 || (size_t)map_index >= plan->maps.size()) {
    ctx->set_error("ssx_undistort_plan_debug_map: map %d of %d, out %s", map_index, (int)plan->maps.size(), out ? "given" : "null");
    return SSX_ERR_INVALID_ARG;
  }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  // the three planes one behind the other are 3 * rows rows of `pitch` entries: the copy drops the pitch columns
  SSX_HIP_TRY(ctx, hipMemcpy2D(out, (size_t)plan->cols * sizeof(uint16_t), plan->maps[(size_t)map_index], (size_t)plan->pitch * sizeof(uint16_t),
                               (size_t)plan->cols * sizeof(uint16_t), (size_t)3 * (size_t)plan->rows, hipMemcpyDeviceToHost));
  return SSX_OK;
}

ssx_status ssx_lens_debug_atan(ssx_ctx* ctx, int32_t n, const double* r, double* atan_out, double* sqrt_out)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  if (n < 0 || n > (1 << 24) || (n > 0 && !r)) { ctx->set_error("ssx_lens_debug_atan: n = %d outside [0, 2^24], or r is null", n); return SSX_ERR_INVALID_ARG; }
  if (n == 0) return SSX_OK;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t bytes = sizeof(double) * (size_t)n;
  SSX_HIP_TRY(ctx, ctx->ud_arena.reserve(3 * bytes));
  double* dev = ctx->ud_arena.as<double>();
  SSX_HIP_TRY(ctx, hipMemcpyAsync(dev, r, bytes, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_lens_debug_atan, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, dev, n, dev + n, dev + 2 * (size_t)n);
  SSX_HIP_TRY(ctx, hipGetLastError());
  if (atan_out) SSX_HIP_TRY(ctx, hipMemcpyAsync(atan_out, dev + n, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (sqrt_out) SSX_HIP_TRY(ctx, hipMemcpyAsync(sqrt_out, dev + 2 * (size_t)n, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return SSX_OK;
}

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
