// ssvio_amd/csrc/dense.hip -- dense stereo: census + semi-global matching, a disparity for every pixel of a rectified pair.
//
// The contract is tools/dense_model.py: every value is a small integer and the device is held to the model bit for
// bit.  There is no floating point in this file.
//
//   k_dense_census   a pixel per thread, both images of every job of a group: the 62 clamped taps of the 9 x 7 window -> one u64
//   k_dense_paths    ONE wavefront per path, lane = disparity (D = 128: lane l holds d = 2l and 2l + 1).  The wave walks its path
//                    pixel by pixel; the matching cost is computed on the fly from the census words (lane d loads censusR(y, x - d):
//                    64 consecutive words), no cost volume is stored.  The d +- 1 neighbours are DPP wave shifts and the minimum over
//                    the wave a DPP reduction: registers only, no LDS, no barrier.  The direction is wave-uniform, so all 4 or 8
//                    directions of all jobs of a group are ONE launch.  L(p, .) is added into the u16 volume S with one 32-bit
//                    atomic per lane that carries two disparities (S <= 2040: no carry between the halves); integer sums make any
//                    order give the same bits.
//   k_dense_right    a wave per left pixel: lane d offers (S(y, x, d) << 8) | d to the right pixel x - d with an atomic minimum;
//                    the packed key makes the first minimum win, in any order
//   k_dense_select   a wave per left pixel: first minimum by the same key, uniqueness as a wave-wide "any", the left-right check
//                    against k_dense_right's result, the integer sub-pixel step with a floor division
//
// Workspace per job: 16 bytes of census, 2 D bytes of S and 4 bytes of right key per pixel.  A call works through its jobs in groups
// whose workspace stays under SSX_DENSE_WORKSPACE_CAP (one pair always runs, whatever it takes); the images go up in one copy, the
// maps come down in one copy, and the call synchronises once.
//
// What follows a map -- the speckle filter and the keyframe's samples, ssx_dense_postprocess and the chained ssx_stereo_dense_post -- is
// dense_post.inc, included at the end of this file (contract: tools/dense_post_model.py).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "../../include/ssx_test_hooks.h"

namespace {

constexpr int DN_MIN_SIDE = 40, DN_MAX_SIDE = 4000;
constexpr int DN_CENSUS_BX = 64, DN_CENSUS_BY = 4;
constexpr int DN_WAVES = 4;                 // waves of a 256-thread block: they share nothing
constexpr int DN_AHEAD_1 = 8, DN_AHEAD_2 = 6;   // k_dense_paths<1>, <2>: pixels whose census words are in flight ahead of the recurrence
constexpr uint32_t DN_FAR = 0x7fffu;        // a neighbour that does not exist (d = -1, d = D): above every L + P1

// one pair of a call, as the kernels see it (device pointers, strides in elements)
struct DnJob {
  const uint8_t* left;
  const uint8_t* right;
  int16_t* disp;
  int32_t left_stride, right_stride, disp_stride, reserved;
};

// ---- cross-lane moves on registers (DPP) ----
// lanes that have no source (and rows the mask leaves out) keep `old`
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dn_dpp(uint32_t old, uint32_t v)
{
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, 0xf, false);
}
// lane l <- lane l - 1 (wave_shr:1), lane l <- lane l + 1 (wave_shl:1)
__device__ __forceinline__ uint32_t dn_from_below(uint32_t v, uint32_t edge) { return dn_dpp<0x138>(edge, v); }
__device__ __forceinline__ uint32_t dn_from_above(uint32_t v, uint32_t edge) { return dn_dpp<0x130>(edge, v); }
// the minimum over the 64 lanes, in every lane: row_shr 1 2 4 8 leave a row's minimum in its lane 15, row_bcast:15 and :31 carry it
// on to lane 63
__device__ __forceinline__ uint32_t dn_wave_min(uint32_t v)
{
  v = min(v, dn_dpp<0x111>(v, v));
  v = min(v, dn_dpp<0x112>(v, v));
  v = min(v, dn_dpp<0x114>(v, v));
  v = min(v, dn_dpp<0x118>(v, v));
  v = min(v, dn_dpp<0x142, 0xa>(v, v));
  v = min(v, dn_dpp<0x143, 0xc>(v, v));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

__global__ void __launch_bounds__(DN_CENSUS_BX * DN_CENSUS_BY) k_dense_census(const DnJob* __restrict__ jobs, int32_t rows, int32_t cols,
                                                                               uint64_t* __restrict__ census)
{
  const int x = (int)(blockIdx.x * DN_CENSUS_BX + threadIdx.x), y = (int)(blockIdx.y * DN_CENSUS_BY + threadIdx.y);
  if (x >= cols || y >= rows) return;
  const DnJob& j = jobs[blockIdx.z >> 1];
  const bool is_right = (blockIdx.z & 1) != 0;
  const uint8_t* img = is_right ? j.right : j.left;
  const int64_t stride = is_right ? j.right_stride : j.left_stride;
  const uint32_t c = img[(int64_t)y * stride + x];
  uint64_t w = 0;
#pragma unroll
  for (int dy = -3; dy <= 3; ++dy) {
    const uint8_t* row = img + (int64_t)min(max(y + dy, 0), rows - 1) * stride;
#pragma unroll
    for (int dx = -4; dx <= 4; ++dx) {
      if (dx == 0 && dy == 0) continue;
      const uint32_t nb = row[min(max(x + dx, 0), cols - 1)];
      w = (w << 1) | (uint64_t)(nb < c);
    }
  }
  census[(int64_t)blockIdx.z * rows * cols + (int64_t)y * cols + x] = w;
}

// V = disparities per lane (D = 64 V).  Directions dir_first .. dir_first + dir_count - 1 of the contract's order; a job has
// `per_job` paths: rows for the two horizontal directions, cols for the two vertical ones, rows + cols - 1 for each diagonal.
// census: per job the left words, then the right words.  S: per job rows x cols x D u16, d fastest, zero before the launch.
template <int V>
__global__ void __launch_bounds__(64 * DN_WAVES) k_dense_paths(const uint64_t* __restrict__ census, uint32_t* __restrict__ S, int32_t rows, int32_t cols,
                                                              int32_t n_jobs, int32_t dir_first, int32_t per_job, uint32_t p1, uint32_t p2)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * DN_WAVES + (threadIdx.x >> 6)));
  if (wave >= (int64_t)n_jobs * per_job) return;
  const int job = (int)(wave / per_job);
  int i = (int)(wave % per_job), k = dir_first;
  for (;;) {
    const int nk = k < 2 ? rows : (k < 4 ? cols : rows + cols - 1);
    if (i < nk) break;
    i -= nk;
    ++k;
  }
  const int dx = (int)((0x8252u >> (2 * k)) & 3u) - 1, dy = (int)((0x2225u >> (2 * k)) & 3u) - 1;   // 1 -1 0 0 1 -1 -1 1 / 0 0 1 -1 1 -1 1 -1
  int x, y;
  if (dy == 0) { x = dx > 0 ? 0 : cols - 1; y = i; }
  else if (i < cols) { x = i; y = dy > 0 ? 0 : rows - 1; }            // (the vertical directions have only these)
  else { x = dx > 0 ? 0 : cols - 1; y = dy > 0 ? i - cols + 1 : rows - 2 - (i - cols); }

  const int64_t pix = (int64_t)rows * cols;
  const uint64_t* cl = census + (int64_t)job * 2 * pix;
  const uint64_t* cr = cl + pix;
  uint32_t* Sj = S + (int64_t)job * pix * (32 * V);
  const int d = V * lane;                                              // this lane's first disparity
  const int left_x = dx > 0 ? cols - x : (dx < 0 ? x + 1 : 0x7fffffff), left_y = dy > 0 ? rows - y : (dy < 0 ? y + 1 : 0x7fffffff);
  const int len = min(left_x, left_y);                                 // pixels on this path
  const int x0 = x;
  const int64_t p0 = (int64_t)y * cols + x, pstep = (int64_t)dy * cols + dx;

  constexpr int A = V == 2 ? DN_AHEAD_2 : DN_AHEAD_1;
  // The census words do not depend on the recurrence, so they are asked for A pixels ahead of it: a block of A pixels is in
  // flight while the block before it walks its dependent chain (one load per step would leave the long horizontal paths waiting a
  // memory latency per pixel once the short paths are done).  cost[u] = C(d) | C(d + 1) << 8 of pixel base + u.
  uint64_t wl[A], wa[A], wb[A];
  uint32_t cost[A];
#define DN_LOAD(base)                                                                                   \
  _Pragma("unroll") for (int u = 0; u < A; ++u) {                                                \
    const int t = (base) + u;                                                                           \
    wl[u] = 0; wa[u] = 0; wb[u] = 0;                                                                    \
    if (t < len) {                                                                                      \
      const int xt = x0 + t * dx;                                                                       \
      const int64_t pt = p0 + t * pstep;                                                                \
      wl[u] = cl[pt];                                                                                   \
      if (xt - d >= 0) wa[u] = cr[pt - d];                                                              \
      if (V == 2 && xt - d - 1 >= 0) wb[u] = cr[pt - d - 1];                                            \
    }                                                                                                   \
  }
#define DN_COST(base)                                                                                   \
  _Pragma("unroll") for (int u = 0; u < A; ++u) {                                                \
    const int xt = x0 + ((base) + u) * dx;                                                              \
    const uint32_t a = xt - d >= 0 ? (uint32_t)__popcll(wl[u] ^ wa[u]) : 63u;                           \
    const uint32_t b = (V == 2 && xt - d - 1 >= 0) ? (uint32_t)__popcll(wl[u] ^ wb[u]) : 63u;           \
    cost[u] = a | (b << 8);                                                                             \
  }
  DN_LOAD(0)
  DN_COST(0)
  uint32_t La = 0, Lb = 0, m = 0;
  for (int base = 0; base < len; base += A) {
    DN_LOAD(base + A)
#pragma unroll
    for (int u = 0; u < A; ++u) {
      const int t = base + u;
      if (t >= len) break;
      const uint32_t ca = cost[u] & 0xffu, cb = cost[u] >> 8;
      if (t == 0) {
        La = ca;
        Lb = cb;
      } else if (V == 1) {
        const uint32_t lo = dn_from_below(La, DN_FAR), hi = dn_from_above(La, DN_FAR);
        La = ca + min(min(La, min(lo, hi) + p1), m + p2) - m;
      } else {
        const uint32_t a_lo = dn_from_below(Lb, DN_FAR), b_hi = dn_from_above(La, DN_FAR);
        const uint32_t na = ca + min(min(La, min(a_lo, Lb) + p1), m + p2) - m;
        const uint32_t nb = cb + min(min(Lb, min(La, b_hi) + p1), m + p2) - m;
        La = na;
        Lb = nb;
      }
      m = dn_wave_min(V == 2 ? min(La, Lb) : La);
      const int64_t pt = p0 + t * pstep;
      if (V == 2) {
        atomicAdd(Sj + pt * 64 + lane, La | (Lb << 16));
      } else {
        const uint32_t up = dn_dpp<0xF5>(0u, La);                      // quad_perm [1,1,3,3]: an even lane reads its odd neighbour
        if ((lane & 1) == 0) atomicAdd(Sj + pt * 32 + (lane >> 1), La | (up << 16));
      }
    }
    DN_COST(base + A)
  }
#undef DN_LOAD
#undef DN_COST
}

// right_key: per job rows x cols u32, all ones before the launch
__global__ void __launch_bounds__(64 * DN_WAVES) k_dense_right(const uint16_t* __restrict__ S, uint32_t* __restrict__ right_key, int32_t cols, int64_t n_pix, int32_t D)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t p = (int64_t)blockIdx.x * DN_WAVES + (threadIdx.x >> 6);   // pixel index over all jobs of the group
  if (p >= n_pix) return;
  const int x = (int)(p % cols);
  const uint16_t* s = S + p * D;
  for (int d = lane; d < D; d += 64)
    if (x - d >= 0) atomicMin(right_key + (p - d), ((uint32_t)s[d] << 8) | (uint32_t)d);
}

__global__ void __launch_bounds__(64 * DN_WAVES) k_dense_select(const uint16_t* __restrict__ S, const uint32_t* __restrict__ right_key, const DnJob* __restrict__ jobs,
                                                               int32_t rows, int32_t cols, int64_t n_pix, int32_t D, int32_t uniqueness, int32_t lr_tolerance)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t p = (int64_t)blockIdx.x * DN_WAVES + (threadIdx.x >> 6);
  if (p >= n_pix) return;
  const int64_t pix = (int64_t)rows * cols;
  const int job = (int)(p / pix);
  const int64_t q = p % pix;
  const int x = (int)(q % cols), y = (int)(q / cols);
  const uint16_t* s = S + p * D;
  const uint32_t sa = s[lane], sb = D == 128 ? (uint32_t)s[lane + 64] : 0xffffu;
  uint32_t key = (sa << 8) | (uint32_t)lane;
  if (D == 128) key = min(key, (sb << 8) | (uint32_t)(lane + 64));
  key = dn_wave_min(key);
  const int d0 = (int)(key & 0xffu);
  const int s0 = (int)(key >> 8);
  bool valid = d0 >= 1 && d0 <= D - 2 && d0 <= x;
  const int w = 100 - uniqueness, bar = s0 * 100;
  bool rival = abs(lane - d0) > 1 && (int)sa * w < bar;
  if (D == 128) rival = rival || (abs(lane + 64 - d0) > 1 && (int)sb * w < bar);
  if (__ballot(rival) != 0ull) valid = false;
  if (valid && lr_tolerance >= 0) {
    const int dr = (int)(right_key[p - d0] & 0xffu);
    valid = abs(dr - d0) <= lr_tolerance;
  }
  if (lane != 0) return;
  int out = -16;
  if (valid) {
    const int sm = s[d0 - 1], sp = s[d0 + 1];
    const int den = max(sm + sp - 2 * s0, 1);
    const int num = (sm - sp) * 16 + den, den2 = 2 * den;
    int sub = num / den2;
    if (num % den2 < 0) --sub;                                          // floor, not C's truncation
    out = 16 * d0 + sub;
  }
  const DnJob& j = jobs[job];
  j.disp[(int64_t)y * j.disp_stride + x] = (int16_t)out;
}

// ---- host side ----
struct DnPlan {
  int32_t n = 0, rows = 0, cols = 0, D = 0;
  size_t pix = 0;
  size_t per_job = 0;                       // workspace bytes of one job
  int32_t group = 1;                        // jobs per group
};

inline size_t dn_job_bytes(size_t pix, int32_t D) { return pix * (16 + 2 * (size_t)D + 4) + 3 * 256; }

// the checks of ssx_stereo_dense on its parameters -> nullptr or what is wrong (msg, cap)
bool dn_bad_params(const ssx_dense_params* p, char* msg, size_t cap)
{
  if (p->disparities != 64 && p->disparities != 128) { snprintf(msg, cap, "disparities = %d (64 or 128)", p->disparities); return true; }
  if (p->p1 < 1 || p->p2 < p->p1 || p->p2 > 192) { snprintf(msg, cap, "p1 = %d, p2 = %d (1 <= p1 <= p2 <= 192: a path value is a byte)", p->p1, p->p2); return true; }
  if (p->uniqueness < 0 || p->uniqueness > 99) { snprintf(msg, cap, "uniqueness = %d outside [0, 99]", p->uniqueness); return true; }
  if (p->lr_tolerance < -1 || p->lr_tolerance > p->disparities) { snprintf(msg, cap, "lr_tolerance = %d outside [-1, %d]", p->lr_tolerance, p->disparities); return true; }
  if (p->paths != 4 && p->paths != 8) { snprintf(msg, cap, "paths = %d (4 or 8)", p->paths); return true; }
  if (p->reserved[0] != 0 || p->reserved[1] != 0) { snprintf(msg, cap, "reserved is not zero"); return true; }
  return false;
}

struct DnWork {
  uint64_t* census = nullptr;
  uint16_t* S = nullptr;
  uint32_t* right_key = nullptr;
};

size_t dn_carve(DnWork& w, char* base, size_t jobs, size_t pix, int32_t D)
{
  return carve(base, [&](auto&& f) {
    f(w.census, jobs * pix * 16);
    f(w.S, jobs * pix * 2 * (size_t)D);
    f(w.right_key, jobs * pix * 4);
  });
}

inline int32_t dn_paths_per_job(int32_t rows, int32_t cols, int32_t dir_first, int32_t dir_count)
{
  int32_t t = 0;
  for (int32_t k = dir_first; k < dir_first + dir_count; ++k) t += k < 2 ? rows : (k < 4 ? cols : rows + cols - 1);
  return t;
}

// the launches of one group of g jobs (table entries tab .. tab + g) up to the volume S of directions dir_first ..
ssx_status dn_volume(ssx_ctx* ctx, const DnWork& w, const DnJob* tab, int32_t g, int32_t rows, int32_t cols, const ssx_dense_params& prm,
                     int32_t dir_first, int32_t dir_count, bool with_census, KfChainStats& st)
{
  const size_t pix = (size_t)rows * cols;
  const int32_t D = prm.disparities;
  if (with_census) {
    const dim3 grid((unsigned)((cols + DN_CENSUS_BX - 1) / DN_CENSUS_BX), (unsigned)((rows + DN_CENSUS_BY - 1) / DN_CENSUS_BY), (unsigned)(2 * g));
    SSX_PROF(ctx, KID_DENSE_CENSUS, hipLaunchKernelGGL(k_dense_census, grid, dim3(DN_CENSUS_BX, DN_CENSUS_BY), 0, ctx->stream, tab, rows, cols, w.census));
    SSX_HIP_TRY(ctx, hipGetLastError());
    ++st.launches;
  }
  SSX_HIP_TRY(ctx, hipMemsetAsync(w.S, 0, (size_t)g * pix * 2 * (size_t)D, ctx->stream));
  ++st.launches;
  const int32_t per_job = dn_paths_per_job(rows, cols, dir_first, dir_count);
  const unsigned blocks = (unsigned)(((int64_t)g * per_job + DN_WAVES - 1) / DN_WAVES);
  if (D == 128)
    SSX_PROF(ctx, KID_DENSE_PATHS, hipLaunchKernelGGL(k_dense_paths<2>, dim3(blocks), dim3(64 * DN_WAVES), 0, ctx->stream, w.census, reinterpret_cast<uint32_t*>(w.S),
                                                     rows, cols, g, dir_first, per_job, (uint32_t)prm.p1, (uint32_t)prm.p2));
  else
    SSX_PROF(ctx, KID_DENSE_PATHS, hipLaunchKernelGGL(k_dense_paths<1>, dim3(blocks), dim3(64 * DN_WAVES), 0, ctx->stream, w.census, reinterpret_cast<uint32_t*>(w.S),
                                                     rows, cols, g, dir_first, per_job, (uint32_t)prm.p1, (uint32_t)prm.p2));
  SSX_HIP_TRY(ctx, hipGetLastError());
  ++st.launches;
  return SSX_OK;
}

ssx_status dn_right(ssx_ctx* ctx, const DnWork& w, int32_t g, int32_t rows, int32_t cols, int32_t D, KfChainStats& st)
{
  const int64_t n_pix = (int64_t)g * rows * cols;
  SSX_HIP_TRY(ctx, hipMemsetAsync(w.right_key, 0xff, (size_t)n_pix * 4, ctx->stream));
  ++st.launches;
  const unsigned blocks = (unsigned)((n_pix + DN_WAVES - 1) / DN_WAVES);
  SSX_PROF(ctx, KID_DENSE_RIGHT, hipLaunchKernelGGL(k_dense_right, dim3(blocks), dim3(64 * DN_WAVES), 0, ctx->stream, w.S, w.right_key, cols, n_pix, D));
  SSX_HIP_TRY(ctx, hipGetLastError());
  ++st.launches;
  return SSX_OK;
}

ssx_status dn_select(ssx_ctx* ctx, const DnWork& w, const DnJob* tab, int32_t g, int32_t rows, int32_t cols, const ssx_dense_params& prm, KfChainStats& st)
{
  const int64_t n_pix = (int64_t)g * rows * cols;
  const unsigned blocks = (unsigned)((n_pix + DN_WAVES - 1) / DN_WAVES);
  SSX_PROF(ctx, KID_DENSE_SELECT, hipLaunchKernelGGL(k_dense_select, dim3(blocks), dim3(64 * DN_WAVES), 0, ctx->stream, w.S, w.right_key, tab, rows, cols, n_pix,
                                                    prm.disparities, prm.uniqueness, prm.lr_tolerance));
  SSX_HIP_TRY(ctx, hipGetLastError());
  ++st.launches;
  return SSX_OK;
}

// the cap a call of ctx groups its jobs by: SSX_DENSE_WORKSPACE_CAP, unless a test has set another (ssx_dense_debug_set_workspace_cap)
inline size_t dn_cap(const ssx_ctx* ctx)
{
#ifndef SSX_NO_TEST_HOOKS
  if (ctx->dense_cap != 0) return (size_t)ctx->dense_cap;
#endif
  (void)ctx;
  return (size_t)SSX_DENSE_WORKSPACE_CAP;
}

// jobs per group: as many as stay under the cap, at least one
inline int32_t dn_group_size(const ssx_ctx* ctx, size_t pix, int32_t D, int32_t n)
{
  const size_t one = dn_job_bytes(pix, D);
  const size_t fit = std::max<size_t>(1, dn_cap(ctx) / one);
  return (int32_t)std::min<size_t>(fit, (size_t)n);
}

}  // namespace

extern "C" {

void ssx_dense_default_params(ssx_dense_params* p)
{
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->disparities = 128;
  p->p1 = 7;
  p->p2 = 86;
  p->uniqueness = 10;
  p->lr_tolerance = 1;
  p->paths = 8;
}

ssx_status ssx_stereo_dense(ssx_ctx* ctx, int32_t n, const ssx_dense_job* jobs, int32_t rows, int32_t cols, const ssx_dense_params* prm,
                            int32_t images_on_device)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  const char* who = "ssx_stereo_dense";
  ctx->dense = KfChainStats{};
  ctx->dense_groups = 0;
  // every refusal comes before anything is touched
  if (!prm) { ctx->set_error("%s: prm is null", who); return SSX_ERR_INVALID_ARG; }
  char why[160];
  if (dn_bad_params(prm, why, sizeof why)) { ctx->set_error("%s: %s", who, why); return SSX_ERR_INVALID_ARG; }
  if (n < 0 || n > SSX_DENSE_MAX_JOBS) { ctx->set_error("%s: n = %d outside [0, %d]", who, n, SSX_DENSE_MAX_JOBS); return SSX_ERR_INVALID_ARG; }
  if (rows < DN_MIN_SIDE || cols < DN_MIN_SIDE || rows > DN_MAX_SIDE || cols > DN_MAX_SIDE) {
    ctx->set_error("%s: %d x %d (rows x cols) outside [%d, %d] a side", who, rows, cols, DN_MIN_SIDE, DN_MAX_SIDE);
    return SSX_ERR_INVALID_ARG;
  }
  if (n > 0 && !jobs) { ctx->set_error("%s: jobs is null", who); return SSX_ERR_INVALID_ARG; }
  for (int32_t k = 0; k < n; ++k) {
    if (!jobs[k].left || !jobs[k].right || !jobs[k].disp) {
      ctx->set_error("%s: job %d has a null %s", who, k, !jobs[k].left ? "left" : (!jobs[k].right ? "right" : "disp"));
      return SSX_ERR_INVALID_ARG;
    }
    if (jobs[k].left_stride < cols || jobs[k].right_stride < cols || jobs[k].disp_stride < cols) {
      ctx->set_error("%s: job %d has a stride (left %d, right %d, disp %d) smaller than cols = %d", who, k, jobs[k].left_stride, jobs[k].right_stride,
                     jobs[k].disp_stride, cols);
      return SSX_ERR_INVALID_ARG;
    }
  }
  if (n == 0) return SSX_OK;

  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool staged = images_on_device == 0;
  const size_t pix = (size_t)rows * (size_t)cols;
  const int32_t D = prm->disparities;
  // one block that goes up (the job table and, staged, the images) and one that comes down (staged: the maps)
  Layout lay;
  const size_t o_tab = lay.take(sizeof(DnJob) * (size_t)n);
  const size_t o_img = staged ? lay.take(2 * pix * (size_t)n) : 0;
  const size_t up_bytes = lay.off;
  const size_t o_disp = staged ? lay.take(2 * pix * (size_t)n) : 0;
  SSX_HIP_TRY(ctx, ctx->dn_arena.reserve(lay.off));
  SSX_HIP_TRY(ctx, ctx->dn_stage.reserve(lay.off));
  const int32_t group = dn_group_size(ctx, pix, D, n);
  DnWork w;
  SSX_HIP_TRY(ctx, ctx->dn_work.reserve(dn_carve(w, nullptr, (size_t)group, pix, D), 1.0));
  dn_carve(w, ctx->dn_work.as<char>(), (size_t)group, pix, D);
  char* dev = ctx->dn_arena.as<char>();
  char* stage = ctx->dn_stage.as<char>();
  KfChainStats st{};

  DnJob* tab = reinterpret_cast<DnJob*>(stage + o_tab);
  for (int32_t k = 0; k < n; ++k) {
    DnJob& t = tab[k];
    t.reserved = 0;
    if (staged) {
      uint8_t* l = reinterpret_cast<uint8_t*>(stage + o_img + 2 * pix * (size_t)k);
      uint8_t* r = l + pix;
      for (int32_t y = 0; y < rows; ++y) {
        std::memcpy(l + (size_t)y * cols, jobs[k].left + (size_t)y * jobs[k].left_stride, (size_t)cols);
        std::memcpy(r + (size_t)y * cols, jobs[k].right + (size_t)y * jobs[k].right_stride, (size_t)cols);
      }
      t.left = reinterpret_cast<const uint8_t*>(dev + o_img + 2 * pix * (size_t)k);
      t.right = t.left + pix;
      t.disp = reinterpret_cast<int16_t*>(dev + o_disp + 2 * pix * (size_t)k);
      t.left_stride = t.right_stride = t.disp_stride = cols;
    } else {
      t.left = jobs[k].left; t.right = jobs[k].right; t.disp = jobs[k].disp;
      t.left_stride = jobs[k].left_stride; t.right_stride = jobs[k].right_stride; t.disp_stride = jobs[k].disp_stride;
    }
  }
  SSX_HIP_TRY(ctx, hipMemcpyAsync(dev, stage, up_bytes, hipMemcpyHostToDevice, ctx->stream));
  st.bytes_up += (int64_t)up_bytes;
  const DnJob* dtab = reinterpret_cast<const DnJob*>(dev + o_tab);
  int32_t groups = 0;
  for (int32_t first = 0; first < n; first += group, ++groups) {
    const int32_t g = std::min(group, n - first);
    ssx_status s = dn_volume(ctx, w, dtab + first, g, rows, cols, *prm, 0, prm->paths, true, st);
    if (s == SSX_OK && prm->lr_tolerance >= 0) s = dn_right(ctx, w, g, rows, cols, D, st);
    if (s == SSX_OK) s = dn_select(ctx, w, dtab + first, g, rows, cols, *prm, st);
    if (s != SSX_OK) return s;
  }
  if (staged) {
    SSX_HIP_TRY(ctx, hipMemcpyAsync(stage + o_disp, dev + o_disp, 2 * pix * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    st.bytes_down += (int64_t)(2 * pix * (size_t)n);
  }
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ++st.syncs;
  if (staged)
    for (int32_t k = 0; k < n; ++k) {
      const int16_t* d = reinterpret_cast<const int16_t*>(stage + o_disp + 2 * pix * (size_t)k);
      for (int32_t y = 0; y < rows; ++y) std::memcpy(jobs[k].disp + (size_t)y * jobs[k].disp_stride, d + (size_t)y * cols, 2 * (size_t)cols);
    }
  ctx->dense = st;
  ctx->dense_groups = groups;
  return SSX_OK;
}

#ifndef SSX_NO_TEST_HOOKS   // include/ssx_test_hooks.h

ssx_status ssx_dense_debug_last_call(ssx_ctx* ctx, int32_t* launches, int32_t* synchronisations, int64_t* bytes_up, int64_t* bytes_down, int32_t* groups)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  if (launches) *launches = ctx->dense.launches;
  if (synchronisations) *synchronisations = ctx->dense.syncs;
  if (bytes_up) *bytes_up = ctx->dense.bytes_up;
  if (bytes_down) *bytes_down = ctx->dense.bytes_down;
  if (groups) *groups = ctx->dense_groups;
  return SSX_OK;
}

ssx_status ssx_dense_debug_set_workspace_cap(ssx_ctx* ctx, uint64_t bytes)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  ctx->dense_cap = bytes;
  return SSX_OK;
}

// the stages of one pair of host images, through the kernels of ssx_stereo_dense; not a fast path (a synchronisation per stage)
ssx_status ssx_dense_debug_stages(ssx_ctx* ctx, const uint8_t* left, int32_t left_stride, const uint8_t* right, int32_t right_stride, int32_t rows, int32_t cols,
                                  const ssx_dense_params* prm, int32_t direction, uint64_t* census_left, uint64_t* census_right, uint8_t* path_volume,
                                  uint16_t* sum_volume, uint8_t* right_disparity)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  const char* who = "ssx_dense_debug_stages";
  char why[160];
  if (!prm || !left || !right) { ctx->set_error("%s: a null argument", who); return SSX_ERR_INVALID_ARG; }
  if (dn_bad_params(prm, why, sizeof why)) { ctx->set_error("%s: %s", who, why); return SSX_ERR_INVALID_ARG; }
  if (rows < DN_MIN_SIDE || cols < DN_MIN_SIDE || rows > DN_MAX_SIDE || cols > DN_MAX_SIDE || left_stride < cols || right_stride < cols) {
    ctx->set_error("%s: %d x %d or a stride out of range", who, rows, cols);
    return SSX_ERR_INVALID_ARG;
  }
  if (path_volume && (direction < 0 || direction >= prm->paths)) { ctx->set_error("%s: direction = %d outside [0, %d)", who, direction, prm->paths); return SSX_ERR_INVALID_ARG; }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t pix = (size_t)rows * cols;
  const int32_t D = prm->disparities;
  Layout lay;
  const size_t o_tab = lay.take(sizeof(DnJob));
  const size_t o_img = lay.take(2 * pix);
  const size_t o_disp = lay.take(2 * pix);
  SSX_HIP_TRY(ctx, ctx->dn_arena.reserve(lay.off));
  DnWork w;
  SSX_HIP_TRY(ctx, ctx->dn_work.reserve(dn_carve(w, nullptr, 1, pix, D), 1.0));
  dn_carve(w, ctx->dn_work.as<char>(), 1, pix, D);
  char* dev = ctx->dn_arena.as<char>();
  std::vector<uint8_t> img(2 * pix);
  for (int32_t y = 0; y < rows; ++y) {
    std::memcpy(img.data() + (size_t)y * cols, left + (size_t)y * left_stride, (size_t)cols);
    std::memcpy(img.data() + pix + (size_t)y * cols, right + (size_t)y * right_stride, (size_t)cols);
  }
  DnJob t{};
  t.left = reinterpret_cast<const uint8_t*>(dev + o_img);
  t.right = t.left + pix;
  t.disp = reinterpret_cast<int16_t*>(dev + o_disp);
  t.left_stride = t.right_stride = t.disp_stride = cols;
  SSX_HIP_TRY(ctx, hipMemcpyAsync(dev + o_tab, &t, sizeof t, hipMemcpyHostToDevice, ctx->stream));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(dev + o_img, img.data(), 2 * pix, hipMemcpyHostToDevice, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const DnJob* dtab = reinterpret_cast<const DnJob*>(dev + o_tab);
  KfChainStats st{};
  std::vector<uint16_t> vol(pix * (size_t)D);
  bool census_done = false;
  if (path_volume) {
    const ssx_status s = dn_volume(ctx, w, dtab, 1, rows, cols, *prm, direction, 1, true, st);
    if (s != SSX_OK) return s;
    census_done = true;
    SSX_HIP_TRY(ctx, hipMemcpyAsync(vol.data(), w.S, vol.size() * 2, hipMemcpyDeviceToHost, ctx->stream));
    SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < vol.size(); ++k) path_volume[k] = (uint8_t)std::min<uint16_t>(vol[k], 255);
  }
  {
    const ssx_status s = dn_volume(ctx, w, dtab, 1, rows, cols, *prm, 0, prm->paths, !census_done, st);
    if (s != SSX_OK) return s;
  }
  if (census_left) SSX_HIP_TRY(ctx, hipMemcpyAsync(census_left, w.census, pix * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (census_right) SSX_HIP_TRY(ctx, hipMemcpyAsync(census_right, w.census + pix, pix * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (sum_volume) SSX_HIP_TRY(ctx, hipMemcpyAsync(sum_volume, w.S, pix * (size_t)D * 2, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (right_disparity) {
    const ssx_status s = dn_right(ctx, w, 1, rows, cols, D, st);
    if (s != SSX_OK) return s;
    std::vector<uint32_t> key(pix);
    SSX_HIP_TRY(ctx, hipMemcpyAsync(key.data(), w.right_key, pix * 4, hipMemcpyDeviceToHost, ctx->stream));
    SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < pix; ++k) right_disparity[k] = (uint8_t)(key[k] & 0xffu);
  }
  return SSX_OK;
}

#endif

}  // extern "C"

#include "dense_post.inc"   // the speckle filter and the keyframe's samples: ssx_dense_postprocess, ssx_stereo_dense_post
