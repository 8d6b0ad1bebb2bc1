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
// camera of a raw rig, is host arithmetic in rectify.inc, included at the end of this file because of the last paragraph.
//
// The host side: ssx_undistort, ssx_undistort_lens and ssx_undistort_plan_apply are each check, facts, build, issue.
//   ud_check   every refusal of a job table, one list for the three job structs (a UdView each), with the one overlap search
//   ud_facts   what only the runtime knows about the image pointers: one allocation or several, pinned host / device / neither
//   ud_build   the call as a plain value, UdCall: launch, block layout, table entries, intakes, the copies up and down in order
//   ud_issue   reserve, pack rows, copy up, launch, copy down, synchronise once, unpack rows, count what was issued
// ud_check and ud_build make no HIP call: ssx_undistort_debug_plan shows their value without a device (tests/test_undistort_call_plan.py).
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

// ---- the host side of a call (the header has its four steps).  ud_check and ud_build make no HIP call and touch no workspace:
// ssx_undistort_debug_plan runs them without a device, and tests/test_undistort_call_plan.py holds the value to the rules stated here ----
constexpr int UD_ERR = 256;                 // bytes of the text that says why a call is refused
enum UdWhich { UD_INLINE = 0, UD_STORED = 1 };   // ssx_undistort / ssx_undistort_lens (k_undistort), ssx_undistort_plan_apply (k_undistort_remap)
#define UD_REFUSE(status, ...) do { std::snprintf(err, UD_ERR, __VA_ARGS__); return (status); } while (0)

inline bool ud_known_model(int32_t model) { return model == SSX_LENS_RADTAN || model == SSX_LENS_KB4; }

// one job of any entry point as the checks and the plan see it: two images, and `tag` -- its lens model (UD_INLINE) or its map index
struct UdView { const uint8_t* src; int32_t src_stride; uint8_t* dst; int32_t dst_stride; int32_t tag; };
struct UdImage { const uint8_t* p; int32_t stride; };
inline UdImage ud_image(const UdView& v, bool results) { return results ? UdImage{v.dst, v.dst_stride} : UdImage{v.src, v.src_stride}; }

// the bytes of an image from its pointer to the end of its last row, and that as [first, last) in memory
inline size_t ud_bytes(int32_t stride, int32_t rows, int32_t cols) { return (size_t)((int64_t)(rows - 1) * stride + cols); }
inline void ud_span(const UdImage& im, int32_t rows, int32_t cols, uintptr_t* first, uintptr_t* last)
{
  *first = reinterpret_cast<uintptr_t>(im.p);
  *last = *first + (uintptr_t)ud_bytes(im.stride, rows, cols);
}

// does a dst of the call overlap a src of the call?  Sorted sources and the furthest end among those that begin no later: n log n for
// the call that is accepted; the pair of a refused call is the first in job order (its dst, then its src)
bool ud_find_overlap(const std::vector<UdView>& v, int32_t rows, int32_t cols, int32_t* d_out, int32_t* s_out)
{
  struct Iv { uintptr_t a, b; };
  const int32_t n = (int32_t)v.size();
  std::vector<Iv> src(v.size());
  for (int32_t k = 0; k < n; ++k) ud_span(ud_image(v[k], false), rows, cols, &src[k].a, &src[k].b);
  std::sort(src.begin(), src.end(), [](const Iv& x, const Iv& y) { return x.a < y.a; });
  for (size_t k = 1; k < src.size(); ++k) src[k].b = std::max(src[k].b, src[k - 1].b);
  for (int32_t d = 0; d < n; ++d) {
    uintptr_t d0, d1;
    ud_span(ud_image(v[d], true), rows, cols, &d0, &d1);
    const size_t cnt = (size_t)(std::lower_bound(src.begin(), src.end(), d1, [](const Iv& x, uintptr_t e) { return x.a < e; }) - src.begin());
    if (cnt == 0 || src[cnt - 1].b <= d0) continue;                             // (exact: the source that ends furthest begins in front of d1)
    for (int32_t s = 0; s < n; ++s) {
      uintptr_t s0, s1;
      ud_span(ud_image(v[s], false), rows, cols, &s0, &s1);
      if (d0 < s1 && s0 < d1) { *d_out = d; *s_out = s; return true; }
    }
  }
  return false;
}

// Every refusal of a job table, before anything is touched, in the order the entry points have always stated them: the count, the
// image size (UD_INLINE: a plan's was checked when it was created), the table, per job its pointers, its strides and its tag, the
// overlap, and (UD_INLINE) the largest side.  view(k) is job k of the caller's table, read only once the count and the table are
// accepted.  -> the status, the text in err, the views in v.
template <class View>
ssx_status ud_check(char* err, const char* who, UdWhich which, int32_t n, bool table, int32_t rows, int32_t cols, int32_t n_maps, View&& view, std::vector<UdView>& v)
{
  if (n < 0 || n > SSX_UNDISTORT_MAX_JOBS) UD_REFUSE(SSX_ERR_INVALID_ARG, "%s: n = %d outside [0, %d]", who, n, SSX_UNDISTORT_MAX_JOBS);
  if (which == UD_INLINE && (rows < 1 || cols < 1)) UD_REFUSE(SSX_ERR_INVALID_ARG, "%s: rows = %d, cols = %d (both must be >= 1)", who, rows, cols);
  if (n > 0 && !table) UD_REFUSE(SSX_ERR_INVALID_ARG, "%s: jobs is null", who);
  v.resize((size_t)n);
  for (int32_t k = 0; k < n; ++k) {
    const UdView& j = v[k] = view(k);
    if (!j.src || !j.dst) UD_REFUSE(SSX_ERR_INVALID_ARG, "%s: job %d has a null %s", who, k, j.src ? "dst" : "src");
    if (j.src_stride < cols || j.dst_stride < cols)
      UD_REFUSE(SSX_ERR_INVALID_ARG, "%s: job %d has a stride (src %d, dst %d) smaller than cols = %d", who, k, j.src_stride, j.dst_stride, cols);
    if (which == UD_INLINE && !ud_known_model(j.tag))
      UD_REFUSE(SSX_ERR_INVALID_ARG, "%s: job %d names lens model %d (SSX_LENS_RADTAN = 0, SSX_LENS_KB4 = 1)", who, k, j.tag);
    if (which == UD_STORED && (j.tag < 0 || j.tag >= n_maps)) UD_REFUSE(SSX_ERR_INVALID_ARG, "%s: job %d names map %d, the plan holds %d", who, k, j.tag, n_maps);
  }
  int32_t d = 0, s = 0;
  if (ud_find_overlap(v, rows, cols, &d, &s)) UD_REFUSE(SSX_ERR_INVALID_ARG, "%s: the dst of job %d overlaps the src of job %d (there is no in-place form)", who, d, s);
  if (which == UD_INLINE && (rows > UD_MAX_SIDE || cols > UD_MAX_SIDE)) UD_REFUSE(SSX_ERR_UNSUPPORTED, "%s: %d x %d is above %d a side", who, rows, cols, UD_MAX_SIDE);
  return SSX_OK;
}

// How the images of one side of a call (the sources, or the results) reach the device and leave it:
//   UD_STAGED    host images, images_on_device = 0: rows packed into pinned staging, one copy each way
//   UD_IN_PLACE  the kernel reads / writes every image where it lies; nothing is copied
//   UD_RANGE     pinned host images that go in ONE copy: in job order ascending, each at least one image behind the last, the whole no
//                longer than twice the images (ud_range_arith), and -- the runtime's word, arithmetic is not enough: images allocated one by
//                one can stand just like that, and one copy over them would cross whatever lies between two allocations -- in ONE
//                allocation (choose_intake and lk_facts of lk.hip).  Results also stand at one constant distance and at a stride of cols:
//                the 2-D copy that brings them down then writes the images and nothing between them.
//   UD_EACH      otherwise: a pinned host image gets a copy of its own, a device image is used where it lies
// ssx_undistort* take UD_STAGED or UD_IN_PLACE and ask nothing; ssx_undistort_plan_apply takes any of the four, per side.
enum UdIntake { UD_STAGED = 0, UD_IN_PLACE, UD_RANGE, UD_EACH };

// What the runtime knows about one side's images and arithmetic does not (ud_facts asks, and only where the answer decides;
// ssx_undistort_debug_plan is told): do they lie in one allocation, and kind[k] of image k -- when they do, only kind[0] is looked at.
enum : int8_t { UD_NEITHER = -1, UD_DEVICE = 0, UD_PINNED = 1 };
struct UdSideFacts { bool one_allocation = false; std::vector<int8_t> kind; };
struct UdFacts { UdSideFacts src, dst; };

// the arithmetic of UD_RANGE: does it hold; the bytes from the first image to the end of the last; for results their distance
struct UdRange { bool ok = false; size_t bytes = 0, distance = 0; };
UdRange ud_range_arith(const std::vector<UdView>& v, bool results, int32_t rows, int32_t cols)
{
  const size_t n = v.size();
  const auto im = [&](size_t k) { return ud_image(v[k], results); };
  UdRange r;
  size_t longest = 0;
  for (size_t k = 0; k < n; ++k) longest = std::max(longest, ud_bytes(im(k).stride, rows, cols));
  r.ok = n >= 2;
  for (size_t k = 1; r.ok && k < n; ++k) r.ok = im(k).p > im(k - 1).p && (size_t)(im(k).p - im(k - 1).p) >= ud_bytes(im(k - 1).stride, rows, cols);
  if (r.ok) r.bytes = (size_t)(im(n - 1).p - im(0).p) + ud_bytes(im(n - 1).stride, rows, cols);
  r.ok = r.ok && r.bytes <= 2 * n * longest;
  if (r.ok && results) {
    r.distance = (size_t)(im(1).p - im(0).p);
    for (size_t k = 0; r.ok && k < n; ++k) r.ok = im(k).stride == cols && (k == 0 || (size_t)(im(k).p - im(k - 1).p) == r.distance);
  }
  return r;
}

// the intake of one side of ssx_undistort_plan_apply with images_on_device; false: image *bad is neither device nor pinned host memory
// (job 0 when a one-allocation range is of unknown kind, otherwise the first unknown image)
bool ud_choose(const std::vector<UdView>& v, bool results, int32_t rows, int32_t cols, const UdSideFacts& f, UdIntake* intake, UdRange* r, int32_t* bad)
{
  *r = ud_range_arith(v, results, rows, cols);
  const bool one = r->ok && f.one_allocation;
  *intake = one && f.kind[0] == UD_PINNED ? UD_RANGE : UD_IN_PLACE;              // (one device allocation: every image where it lies)
  for (size_t k = 0; k < (one ? 1 : v.size()); ++k) {
    if (f.kind[k] == UD_NEITHER) { *bad = (int32_t)k; return false; }
    if (!one && f.kind[k] == UD_PINNED) *intake = UD_EACH;
  }
  return true;
}

// A call as a plain value.  The device block is [job table | sources] | results, the table at its start and each part at a multiple of
// 256: everything that is sent lies in front of up_bytes, everything that comes back behind it.
//   UD_STAGED   sources packed at a pitch of cols, results at a pitch of cols rounded up to a dword (every store but the tail's is one).
//               ssx_undistort* pack the images of a side as one run; ssx_undistort_plan_apply rounds each image's slot to 256.
//   UD_RANGE    the sources keep the range's layout (one copy): image k at base + (src_k - src_0), at its own stride; the results are
//               images of rows * cols bytes at a stride of cols in slots rounded to 256 (one 2-D copy: a row of it is an image)
//   UD_EACH     pinned host sources stand one by one at their own stride, pinned host results one by one at the dword pitch
// (UdCallJob, UdUp and UdDown are ssx_undistort_call_info's job, up and down, member for member.)
constexpr size_t UD_WHERE_IT_LIES = ~size_t(0);                                 // UdCallJob::*_off: the table entry carries the caller's pointer
struct UdCallJob { size_t src_off, dst_off; int64_t src_stride, dst_stride; };  // what table entry k will carry
struct UdUp { size_t off; const void* host; size_t bytes, images; };            // to arena + off, from `host` (null: staging + off); images: it carries some
struct UdDown { void* host; size_t hpitch, off, dpitch, width, height; };       // 2-D to `host` from arena + off; host null: `width` bytes to staging + off
typedef ssx_ctx::UdStats UdStats;                                               // what a call issued: KfChainStats and the copies that carried images
struct UdCall {
  int32_t n = 0, rows = 0, cols = 0;
  unsigned grid[3] = {0, 0, 0}, block[3] = {UD_BX, UD_BY, 1};
  UdIntake src_intake, dst_intake;        // UD_STAGED sources are packed into staging before the copies, UD_STAGED results unpacked behind the synchronisation
  size_t tab_bytes = 0, up_bytes = 0, arena_bytes = 0, stage_bytes = 0;
  std::vector<UdCallJob> jobs;
  std::vector<UdUp> up;                   // in the order they are issued: the table first
  std::vector<UdDown> down;
};

ssx_status ud_build(char* err, const char* who, UdWhich which, const std::vector<UdView>& v, int32_t rows, int32_t cols, int32_t images_on_device, const UdFacts& facts,
                    UdCall& c)
{
  const size_t n = v.size();
  const bool staged = images_on_device == 0;
  c.n = (int32_t)n; c.rows = rows; c.cols = cols;
  c.grid[0] = (unsigned)((cols + UD_BX * UD_PX - 1) / (UD_BX * UD_PX)); c.grid[1] = (unsigned)((rows + UD_BY - 1) / UD_BY); c.grid[2] = (unsigned)n;
  c.src_intake = c.dst_intake = staged ? UD_STAGED : UD_IN_PLACE;
  UdRange sr, dr;
  int32_t bad = -1;
  if (!staged && which == UD_STORED && !ud_choose(v, false, rows, cols, facts.src, &c.src_intake, &sr, &bad))
    UD_REFUSE(SSX_ERR_INVALID_ARG, "%s: the src of job %d is neither device memory nor pinned host memory (images_on_device = %d)", who, bad, images_on_device);
  if (!staged && which == UD_STORED && !ud_choose(v, true, rows, cols, facts.dst, &c.dst_intake, &dr, &bad))
    UD_REFUSE(SSX_ERR_INVALID_ARG, "%s: the dst of job %d is neither device memory nor pinned host memory (images_on_device = %d)", who, bad, images_on_device);
  const size_t img_bytes = (size_t)rows * (size_t)cols, dpitch = ((size_t)cols + 3) & ~size_t(3), dst_bytes = (size_t)rows * dpitch;
  const auto slot = [&](size_t bytes) { return which == UD_STORED ? (bytes + 255) & ~size_t(255) : bytes; };
  c.jobs.resize(n);
  for (size_t k = 0; k < n; ++k) c.jobs[k] = UdCallJob{UD_WHERE_IT_LIES, UD_WHERE_IT_LIES, v[k].src_stride, v[k].dst_stride};
  Layout lay;
  c.tab_bytes = (which == UD_INLINE ? sizeof(UdJob) : sizeof(UdRemapJob)) * n;
  lay.take(c.tab_bytes);
  if (c.src_intake == UD_STAGED) {
    const size_t base = lay.take(slot(img_bytes) * n);
    for (size_t k = 0; k < n; ++k) { c.jobs[k].src_off = base + slot(img_bytes) * k; c.jobs[k].src_stride = cols; }
  } else if (c.src_intake == UD_RANGE) {
    const size_t base = lay.take(sr.bytes + 16);
    for (size_t k = 0; k < n; ++k) c.jobs[k].src_off = base + (size_t)(v[k].src - v[0].src);
    c.up.push_back(UdUp{base, v[0].src, sr.bytes, 1});
  }
  for (size_t k = 0; c.src_intake == UD_EACH && k < n; ++k) {
    if (facts.src.kind[k] != UD_PINNED) continue;
    c.jobs[k].src_off = lay.take(ud_bytes(v[k].src_stride, rows, cols));
    c.up.push_back(UdUp{c.jobs[k].src_off, v[k].src, ud_bytes(v[k].src_stride, rows, cols), 1});
  }
  c.up_bytes = lay.off;
  // the table goes up first: in the one copy of staged sources, else beside the images (ssx_undistort*: its span, plan_apply: its bytes)
  c.up.insert(c.up.begin(), UdUp{0, nullptr, staged || which == UD_INLINE ? c.up_bytes : c.tab_bytes, staged});
  if (c.dst_intake == UD_STAGED || c.dst_intake == UD_RANGE) {
    // UD_RANGE: a row of the copy is an image, rows * cols bytes, `distance` apart on the host -- nothing between the images is written
    const bool range = c.dst_intake == UD_RANGE;
    const size_t each = slot(range ? img_bytes : dst_bytes), base = lay.take(each * n);
    for (size_t k = 0; k < n; ++k) { c.jobs[k].dst_off = base + each * k; c.jobs[k].dst_stride = range ? (int64_t)cols : (int64_t)dpitch; }
    c.down.push_back(range ? UdDown{v[0].dst, dr.distance, base, each, img_bytes, n} : UdDown{nullptr, 0, base, 0, each * n, 1});
  }
  for (size_t k = 0; c.dst_intake == UD_EACH && k < n; ++k) {
    if (facts.dst.kind[k] != UD_PINNED) continue;                                  // (rows of cols bytes: the pitch bytes of the destination stay)
    c.jobs[k].dst_off = lay.take(dst_bytes);
    c.jobs[k].dst_stride = (int64_t)dpitch;
    c.down.push_back(UdDown{v[k].dst, (size_t)v[k].dst_stride, c.jobs[k].dst_off, dpitch, (size_t)cols, (size_t)rows});
  }
  c.arena_bytes = lay.off;
  c.stage_bytes = staged ? c.arena_bytes : c.up[0].bytes;
  return SSX_OK;
}

// what issuing `c` counts: one launch, one synchronisation, the bytes of its copies, and the copies that carry images
UdStats ud_predict(const UdCall& c)
{
  UdStats st{};
  st.launches = 1; st.syncs = 1;
  for (const UdUp& u : c.up) { st.bytes_up += (int64_t)u.bytes; st.copies_up += (int32_t)u.images; }
  for (const UdDown& d : c.down) { st.bytes_down += (int64_t)(d.width * d.height); ++st.copies_down; }
  return st;
}

// ---- the asking: look-ups in the runtime's table of allocations, no copy, no launch, no synchronisation ----
int8_t ud_kind(const void* p)
{
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return UD_NEITHER; }
  if (at.type == hipMemoryTypeHost) return UD_PINNED;
  return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged ? UD_DEVICE : UD_NEITHER;
}

// one side's facts, asked only where ud_choose will look; false: an image of unknown kind was met (no image behind it is asked)
bool ud_ask(const std::vector<UdView>& v, bool results, int32_t rows, int32_t cols, UdSideFacts& f)
{
  const size_t n = v.size();
  f.kind.assign(n, UD_DEVICE);
  const UdRange r = ud_range_arith(v, results, rows, cols);
  const uint8_t* const first = ud_image(v[0], results).p;
  hipDeviceptr_t base0 = nullptr, base1 = nullptr;
  size_t size0 = 0, size1 = 0;
  f.one_allocation = r.ok && hipMemGetAddressRange(&base0, &size0, (hipDeviceptr_t)first) == hipSuccess &&
                     hipMemGetAddressRange(&base1, &size1, (hipDeviceptr_t)ud_image(v[n - 1], results).p) == hipSuccess && base0 == base1 &&
                     (const uint8_t*)base0 <= first && first + r.bytes <= (const uint8_t*)base0 + size0;
  if (r.ok && !f.one_allocation) (void)hipGetLastError();
  for (size_t k = 0; k < (f.one_allocation ? 1 : n); ++k)
    if ((f.kind[k] = ud_kind(ud_image(v[k], results).p)) == UD_NEITHER) return false;
  return true;
}

// (ssx_undistort* ask nothing; a side behind a refused one is not asked)
UdFacts ud_facts(UdWhich which, const std::vector<UdView>& v, int32_t rows, int32_t cols, int32_t images_on_device)
{
  UdFacts f;
  if (which == UD_STORED && images_on_device != 0 && ud_ask(v, false, rows, cols, f.src)) (void)ud_ask(v, true, rows, cols, f.dst);
  return f;
}

// ---- the issuing: reserve, fill the table and pack rows into staging, copy up, launch, copy down, synchronise once, unpack rows, count.
// Entry is UdJob or UdRemapJob (both begin with the pointers and the strides); fill(k, entry) writes the rest of entry k ----
template <class Entry, class Fill, class Launch>
ssx_status ud_issue(ssx_ctx* ctx, const UdCall& c, const std::vector<UdView>& v, DevBuf& arena, HostBuf& staging, Fill&& fill, Launch&& launch, UdStats* out)
{
  SSX_HIP_TRY(ctx, arena.reserve(c.arena_bytes));
  SSX_HIP_TRY(ctx, staging.reserve(c.stage_bytes));
  char* dev = arena.as<char>();
  char* stage = staging.as<char>();
  const size_t cols = (size_t)c.cols;
  Entry* tab = reinterpret_cast<Entry*>(stage);
  for (int32_t k = 0; k < c.n; ++k) {
    const UdCallJob& j = c.jobs[k];
    Entry& t = tab[k];
    t.src = j.src_off == UD_WHERE_IT_LIES ? v[k].src : reinterpret_cast<const uint8_t*>(dev + j.src_off);
    t.dst = j.dst_off == UD_WHERE_IT_LIES ? v[k].dst : reinterpret_cast<uint8_t*>(dev + j.dst_off);
    t.src_stride = j.src_stride; t.dst_stride = j.dst_stride;
    fill(k, t);
    if (c.src_intake != UD_STAGED) continue;
    uint8_t* s = reinterpret_cast<uint8_t*>(stage + j.src_off);
    for (int32_t r = 0; r < c.rows; ++r) std::memcpy(s + (size_t)r * cols, v[k].src + (size_t)r * v[k].src_stride, cols);
  }
  for (const UdUp& u : c.up) SSX_HIP_TRY(ctx, hipMemcpyAsync(dev + u.off, u.host ? u.host : stage + u.off, u.bytes, hipMemcpyHostToDevice, ctx->stream));
  launch(reinterpret_cast<const Entry*>(dev), dim3(c.grid[0], c.grid[1], c.grid[2]), dim3(c.block[0], c.block[1], c.block[2]));
  SSX_HIP_TRY(ctx, hipGetLastError());
  for (const UdDown& d : c.down) {
    if (d.host) SSX_HIP_TRY(ctx, hipMemcpy2DAsync(d.host, d.hpitch, dev + d.off, d.dpitch, d.width, d.height, hipMemcpyDeviceToHost, ctx->stream));
    else SSX_HIP_TRY(ctx, hipMemcpyAsync(stage + d.off, dev + d.off, d.width, hipMemcpyDeviceToHost, ctx->stream));
  }
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (c.dst_intake == UD_STAGED)
    for (int32_t k = 0; k < c.n; ++k) {
      const uint8_t* d = reinterpret_cast<const uint8_t*>(stage + c.jobs[k].dst_off);
      for (int32_t r = 0; r < c.rows; ++r) std::memcpy(v[k].dst + (size_t)r * v[k].dst_stride, d + (size_t)r * (size_t)c.jobs[k].dst_stride, cols);
    }
  *out = ud_predict(c);                                                          // (every copy of the lists was issued, and nothing else)
  return SSX_OK;
}

}  // namespace

// ---- the entry points ----

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
  UdStats last;                               // what the last add or apply issued (ssx_undistort_plan_debug_last_call)
};

namespace {

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
inline const ssx_lens_params& ud_as_lens(const ssx_lens_params& p) { return p; }

// ssx_undistort_lens (Job = ssx_lens_job), and ssx_undistort (ssx_undistort_job) as its RADTAN case: check, facts, build, issue
template <class Job>
ssx_status ud_run(ssx_ctx* ctx, const char* who, int32_t n, const Job* jobs, int32_t rows, int32_t cols, int32_t images_on_device)
{
  ctx->undistort = UdStats{};
  char err[UD_ERR] = {0};
  std::vector<UdView> v;
  const auto view = [&](int32_t k) { return UdView{jobs[k].src, jobs[k].src_stride, jobs[k].dst, jobs[k].dst_stride, ud_as_lens(jobs[k].prm).model}; };
  UdCall call;
  ssx_status st = ud_check(err, who, UD_INLINE, n, jobs != nullptr, rows, cols, 0, view, v);
  if (st == SSX_OK && n > 0) st = ud_build(err, who, UD_INLINE, v, rows, cols, images_on_device, UdFacts{}, call);
  if (st != SSX_OK) { ctx->set_error("%s", err); return st; }
  if (n == 0) return SSX_OK;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const auto fill = [&](int32_t k, UdJob& t) {
    const ssx_lens_params& p = ud_as_lens(jobs[k].prm);
    t.model = p.model; t.reserved = 0;
    std::memcpy(t.K, p.K, sizeof(t.K));
    std::memcpy(t.coeffs, p.coeffs, sizeof(t.coeffs));
    std::memcpy(t.iR, p.iR, sizeof(t.iR));
  };
  const auto launch = [&](const UdJob* tab, dim3 grid, dim3 block) {
    SSX_PROF(ctx, KID_UNDISTORT, hipLaunchKernelGGL(k_undistort, grid, block, 0, ctx->stream, tab, rows, cols));
  };
  return ud_issue<UdJob>(ctx, call, v, ctx->ud_arena, ctx->ud_stage, fill, launch, &ctx->undistort);
}

// ssx_undistort_plan_add_lens, and ssx_undistort_plan_add as its RADTAN case
ssx_status ud_plan_add(ssx_undistort_plan* plan, const char* who, const ssx_lens_params* prm, int32_t* map_index)
{
  ssx_ctx* ctx = plan->ctx;
  plan->last = UdStats{};
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

void ssx_undistort_default(const double K4[4], const double dist5[5], ssx_undistort_params* out)
{
  if (!K4 || !dist5 || !out) return;
  std::memcpy(out->K, K4, sizeof(out->K));
  std::memcpy(out->dist, dist5, sizeof(out->dist));
  const double fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
  const double iR[9] = {1.0 / fx, 0.0, -cx / fx, 0.0, 1.0 / fy, -cy / fy, 0.0, 0.0, 1.0};
  std::memcpy(out->iR, iR, sizeof(out->iR));
}

ssx_status ssx_undistort_lens(ssx_ctx* ctx, int32_t n, const ssx_lens_job* jobs, int32_t rows, int32_t cols, int32_t images_on_device)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  return ud_run(ctx, "ssx_undistort_lens", n, jobs, rows, cols, images_on_device);
}

ssx_status ssx_undistort(ssx_ctx* ctx, int32_t n, const ssx_undistort_job* jobs, int32_t rows, int32_t cols, int32_t images_on_device)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  return ud_run(ctx, "ssx_undistort", n, jobs, rows, cols, images_on_device);
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

// check, facts, build, issue
ssx_status ssx_undistort_plan_apply(ssx_undistort_plan* plan, int32_t n, const ssx_undistort_plan_job* jobs, int32_t images_on_device)
{
  if (!plan) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = plan->ctx;
  const char* const who = "ssx_undistort_plan_apply";
  const int32_t rows = plan->rows, cols = plan->cols;
  plan->last = UdStats{};
  char err[UD_ERR] = {0};
  std::vector<UdView> v;
  const auto view = [&](int32_t k) { return UdView{jobs[k].src, jobs[k].src_stride, jobs[k].dst, jobs[k].dst_stride, jobs[k].map}; };
  ssx_status st = ud_check(err, who, UD_STORED, n, jobs != nullptr, rows, cols, (int32_t)plan->maps.size(), view, v);
  if (st != SSX_OK) { ctx->set_error("%s", err); return st; }
  if (n == 0) return SSX_OK;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  UdCall call;
  st = ud_build(err, who, UD_STORED, v, rows, cols, images_on_device, ud_facts(UD_STORED, v, rows, cols, images_on_device), call);
  if (st != SSX_OK) { ctx->set_error("%s", err); return st; }
  const auto fill = [&](int32_t k, UdRemapJob& t) { t.map = plan->maps[(size_t)v[k].tag]; };
  const auto launch = [&](const UdRemapJob* tab, dim3 grid, dim3 block) {
    SSX_PROF(ctx, KID_UNDISTORT_REMAP, hipLaunchKernelGGL(k_undistort_remap, grid, block, 0, ctx->stream, tab, rows, cols, plan->pitch));
  };
  return ud_issue<UdRemapJob>(ctx, call, v, plan->arena, plan->stage, fill, launch, &plan->last);
}

#ifndef SSX_NO_TEST_HOOKS   // include/ssx_test_hooks.h
ssx_status ssx_undistort_debug_plan(int32_t entry, int32_t rows, int32_t cols, int32_t images_on_device, int32_t n, const ssx_undistort_job_facts* jobs,
                                    int32_t n_maps, const ssx_undistort_side_facts* src_facts, const ssx_undistort_side_facts* dst_facts,
                                    ssx_undistort_call_info* out)
{
  static const char* const names[3] = {"ssx_undistort", "ssx_undistort_lens", "ssx_undistort_plan_apply"};
  if (!out || entry < 0 || entry > 2) return SSX_ERR_INVALID_ARG;
  std::memset(out, 0, sizeof *out);
  static_assert(sizeof(out->error) == UD_ERR, "ssx_undistort_call_info::error holds the refusal's text");
  const UdWhich which = entry == SSX_UD_ENTRY_PLAN_APPLY ? UD_STORED : UD_INLINE;
  // views whose pointers say what the facts say and are never followed: ud_check and ud_build only compare and subtract them
  uint8_t* const base = reinterpret_cast<uint8_t*>(uintptr_t(SSX_UD_BASE));
  const auto view = [&](int32_t k) {
    const ssx_undistort_job_facts& q = jobs[k];
    return UdView{q.flags & SSX_UD_SRC_IS_NULL ? nullptr : base + q.src_off, q.src_stride, q.flags & SSX_UD_DST_IS_NULL ? nullptr : base + q.dst_off, q.dst_stride, q.tag};
  };
  std::vector<UdView> v;
  UdCall c;
  out->status = ud_check(out->error, names[entry], which, n, jobs != nullptr, rows, cols, n_maps, view, v);
  if (out->status != SSX_OK || n == 0) return (ssx_status)out->status;
  UdFacts f;
  const auto told = [&](const ssx_undistort_side_facts* t, UdSideFacts& side) {
    side.one_allocation = t && t->one_allocation != 0;
    if (t && t->kind) side.kind.assign(t->kind, t->kind + n); else side.kind.assign((size_t)n, UD_DEVICE);
  };
  told(src_facts, f.src); told(dst_facts, f.dst);
  out->status = ud_build(out->error, names[entry], which, v, rows, cols, images_on_device, f, c);
  if (out->status != SSX_OK) return (ssx_status)out->status;
  for (int i = 0; i < 3; ++i) { out->grid[i] = (int32_t)c.grid[i]; out->block[i] = (int32_t)c.block[i]; }
  out->src_intake = c.src_intake; out->dst_intake = c.dst_intake;
  const uint64_t parts[4] = {0, (c.tab_bytes + 255) & ~size_t(255), c.up_bytes, c.arena_bytes};     // table, sources, results
  for (int i = 0; i < 3; ++i) { out->span_off[i] = parts[i]; out->span_bytes[i] = i == 0 ? c.tab_bytes : parts[i + 1] - parts[i]; }
  out->up_bytes = c.up_bytes; out->arena_bytes = c.arena_bytes; out->stage_bytes = c.stage_bytes;
  out->n_jobs = c.n; out->n_up = (int32_t)c.up.size(); out->n_down = (int32_t)c.down.size();
  static_assert(sizeof(UdCallJob) == sizeof(out->job[0]) && sizeof(UdUp) == sizeof(out->up[0]) && sizeof(UdDown) == sizeof(out->down[0]), "member for member");
  std::memcpy(out->job, c.jobs.data(), sizeof(UdCallJob) * c.jobs.size());
  std::memcpy(out->up, c.up.data(), sizeof(UdUp) * c.up.size());
  if (!c.down.empty()) std::memcpy(out->down, c.down.data(), sizeof(UdDown) * c.down.size());
  const UdStats st = ud_predict(c);
  out->launches = st.launches; out->syncs = st.syncs; out->copies_up = st.copies_up; out->copies_down = st.copies_down;
  out->bytes_up = st.bytes_up; out->bytes_down = st.bytes_down;
  return SSX_OK;
}

ssx_status ssx_undistort_plan_debug_last_call(const ssx_undistort_plan* plan, int32_t* launches, int32_t* synchronisations, int64_t* bytes_up, int64_t* bytes_down,
                                              int32_t* copies_up, int32_t* copies_down)
{
  if (!plan) return SSX_ERR_INVALID_ARG;
  const UdStats& s = plan->last;
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

#include "rectify.inc"
