// ssvio_amd/csrc/dense_post.inc -- what follows a disparity map: the speckle filter and the samples a keyframe keeps.  Part of dense.hip
// (included at its end: it uses DnJob, DnWork and the launches of ssx_stereo_dense).
//
// The contract is tools/dense_post_model.py (DESIGN.md 6p), integers only; the device is held to it bit for bit.  A pixel is valid iff
// its value is > 0; two 4-neighbours are joined iff both are valid and differ by at most speckle_range; a component's root is its
// smallest raster index.  The partition does not depend on the order of the unions, so atomics are free to run in any order.
//
//   k_dense_label_tile    a workgroup per DP_TW x DP_TH tile, labels in LDS: a row's runs come from ONE ballot per row (lane = column),
//                         the rows of a tile are then joined by union-find on LDS.  Workgroups do not talk to each other here.  Writes
//                         label = the tile-local root as a raster index of the job, and size = 0.
//   k_dense_label_merge   a thread per pixel on the first row / column of a tile: joins it to the pixel across the tile border by
//                         union-find on the global labels -- an agent-scope atomic minimum on the root, confirmed by the value it
//                         returns and retried from there otherwise (Playne / Komura).  Row ends and job seams are not neighbours: only
//                         x > 0 and y > 0 inside the job are looked at.  A union that three others imply is left out.
//   k_dense_label_count   after the kernel boundary: every pixel follows its chain to the root, stores it, and adds into size[root] --
//                         one atomic per DISTINCT root among the 256 consecutive pixels of a wave, carrying their number
//   k_dense_speckle       size[root] <= speckle_size writes -16 into the job's map
//   k_dense_sample_rows   a wave per sample row: how many of its samples pass disp >= min_disp16
//   k_dense_sample_write  a wave per sample row: the rows before it summed (an exclusive scan, at most 4000 terms), the place inside the
//                         row from a ballot -- an ORDERED compaction, raster order, no atomic append
//
// Six launches per group at most (four for the filter, two for the samples), whatever the image size or content.  Every loop whose exit
// depends on a word another thread writes has a bound derived from the pixel count; past it the kernel raises the flag of the call's
// result block and leaves, and the call fails with a message.

namespace {

constexpr int DP_TW = 64, DP_TH = 16;      // the labelling tile: a wave's lanes are its columns; 6 KB of LDS a workgroup
constexpr int DP_TILE = DP_TW * DP_TH;
constexpr int DP_MAX_STRIDE = 4000;

// one map of a call, as the post-processing kernels see it (device pointers, strides in elements)
struct DpJob {
  int16_t* disp;
  const uint8_t* left;
  uint64_t* samples;                        // 8-byte records: u16 u, u16 v, i16 disp16, u8 intensity, u8 0
  int32_t disp_stride, left_stride;
};

struct DpWork {
  int32_t* label = nullptr;                 // per job rows x cols: the parent of a valid pixel as a raster index of the job, -1 else
  int32_t* size = nullptr;                  // per job rows x cols: at a root, the pixels of its component
  int32_t* row_count = nullptr;             // per job ceil(rows / stride): the samples of a sample row
};

inline size_t dp_job_bytes(size_t pix, int32_t rows) { return pix * 8 + (size_t)rows * 4 + 3 * 256; }

size_t dp_carve(DpWork& w, char* base, size_t jobs, size_t pix, int32_t rows)
{
  return carve(base, [&](auto&& f) {
    f(w.label, jobs * pix * 4);
    f(w.size, jobs * pix * 4);
    f(w.row_count, jobs * (size_t)rows * 4);
  });
}

// The chain from r to its root.  A label is never above its own index and only ever decreases, so every step moves to a strictly
// smaller index that is at least 0: a chain has fewer than n steps among n pixels.  `over` is raised past that, or on a label that
// is no index of a chain (which nothing here writes).
template <int SCOPE>
__device__ __forceinline__ int dp_find(const int32_t* lab, int r, int n, bool& over)
{
  for (int it = 0;; ++it) {
    const int p = __hip_atomic_load(lab + r, __ATOMIC_RELAXED, SCOPE);
    if (p == r) return r;
    if (it >= n || (unsigned)p > (unsigned)r) { over = true; return r; }
    r = p;
  }
}

// Joins the components of a and b among n pixels; false past the bound.  The larger root is pointed at the smaller with an atomic
// minimum.  If the value it returns is the root itself the union is done; otherwise another thread lowered that label first, the
// returned value is below a, and the union goes on from there.  Every pass that does not end the loop therefore lowers a or b (a
// find only lowers them too), both stay at least 0 and below n: a + b falls by at least one a pass, so 2 n passes are never reached.
template <int SCOPE>
__device__ __forceinline__ bool dp_union(int32_t* lab, int a, int b, int n)
{
  bool over = false;
  for (int it = 0; it <= 2 * n; ++it) {
    a = dp_find<SCOPE>(lab, a, n, over);
    b = dp_find<SCOPE>(lab, b, n, over);
    if (over) return false;
    if (a == b) return true;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return true;
    a = old;
  }
  return false;
}

__device__ __forceinline__ bool dp_joined(int a, int b, int range) { return a > 0 && b > 0 && abs(a - b) <= range; }

__global__ void __launch_bounds__(256) k_dense_label_tile(const DpJob* __restrict__ jobs, int32_t rows, int32_t cols, int32_t range, int32_t* __restrict__ label,
                                                          int32_t* __restrict__ size, int32_t* __restrict__ result)
{
  __shared__ int32_t lab[DP_TILE];
  __shared__ int16_t val[DP_TILE];
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const DpJob& j = jobs[blockIdx.z];
  const int x0 = (int)blockIdx.x * DP_TW, y0 = (int)blockIdx.y * DP_TH;
  const int x = x0 + lane;
  // the runs of a row: lane l starts one unless it is joined to lane l - 1; a pixel's label is the start of its run
  for (int ly = wave; ly < DP_TH; ly += 4) {
    const int y = y0 + ly;
    int v = 0;
    if (x < cols && y < rows) v = j.disp[(int64_t)y * j.disp_stride + x];
    const int left = __shfl_up(v, 1);
    const bool joined = lane > 0 && dp_joined(v, left, range);
    const uint64_t starts = __ballot(!joined) & (~0ull >> (63 - lane));      // bit 0 is always set
    const int start = 63 - __clzll((long long)starts);
    val[ly * DP_TW + lane] = (int16_t)v;
    lab[ly * DP_TW + lane] = v > 0 ? ly * DP_TW + start : -1;
  }
  __syncthreads();
  bool ok = true;
  for (int ly = wave; ly < DP_TH; ly += 4) {
    if (ly == 0) continue;
    const int l = ly * DP_TW + lane;
    if (dp_joined(val[l], val[l - DP_TW], range)) ok = dp_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, l, l - DP_TW, DP_TILE) && ok;
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.z * rows * cols;
  for (int ly = wave; ly < DP_TH; ly += 4) {
    const int y = y0 + ly;
    if (x >= cols || y >= rows) continue;
    const int l = ly * DP_TW + lane;
    int g = -1;
    if (val[l] > 0) {
      bool over = false;
      const int r = dp_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, l, DP_TILE, over);
      ok = ok && !over;
      g = (y0 + r / DP_TW) * cols + x0 + r % DP_TW;
    }
    label[base + (int64_t)y * cols + x] = g;
    size[base + (int64_t)y * cols + x] = 0;
  }
  if (!ok) atomicOr(result, 1);
}

// per job n_h = (tile rows - 1) * cols pixels below a horizontal border, then n_v = (tile columns - 1) * rows right of a vertical one.
// A union is left out where three others imply it: with q the pixel before this one along the border, "this ~ q", "across ~ q's across"
// (both inside a tile, so k_dense_label_tile has made them) and "q ~ q's across" (the thread before this one, or what implies it in
// turn).  Not where q lies in another tile: at a corner the two borders' threads would each rely on the other.
__global__ void __launch_bounds__(256) k_dense_label_merge(const DpJob* __restrict__ jobs, int32_t rows, int32_t cols, int32_t range, int32_t* __restrict__ label,
                                                           int32_t n_h, int32_t n_v, int64_t total, int32_t* __restrict__ result)
{
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int per = n_h + n_v;
  const int job = (int)(t / per);
  int i = (int)(t % per), x, y, ax, ay;                                     // the pixel; (ax, ay) = the step along its border
  if (i < n_h) {
    y = (i / cols + 1) * DP_TH; x = i % cols;                               // y <= (tile rows - 1) * DP_TH < rows
    ax = 1; ay = 0;
  } else {
    i -= n_h;
    x = (i / rows + 1) * DP_TW; y = i % rows;                               // x <= (tile columns - 1) * DP_TW < cols
    ax = 0; ay = 1;
  }
  const int ox = x - ay, oy = y - ax;                                       // the pixel across the border
  const DpJob& j = jobs[job];
  const int v = j.disp[(int64_t)y * j.disp_stride + x], u = j.disp[(int64_t)oy * j.disp_stride + ox];
  if (!dp_joined(v, u, range)) return;
  if (ax ? x % DP_TW != 0 : y % DP_TH != 0) {                               // q = (x - ax, y - ay) is in this pixel's tile
    const int qv = j.disp[(int64_t)(y - ay) * j.disp_stride + x - ax], qu = j.disp[(int64_t)(oy - ay) * j.disp_stride + ox - ax];
    if (dp_joined(qv, v, range) && dp_joined(qu, u, range) && dp_joined(qv, qu, range)) return;
  }
  const int pix = rows * cols;
  if (!dp_union<__HIP_MEMORY_SCOPE_AGENT>(label + (int64_t)job * pix, y * cols + x, oy * cols + ox, pix)) atomicOr(result, 2);
}

// total = pixels of the group (below 2^31: a group's labels and sizes stay under SSX_DENSE_WORKSPACE_CAP, and one job has at most
// 4000 x 4000).  The forest does not change in this launch except that a pixel is pointed at its root, which is on its chain anyway.
// A wave takes DP_COUNT_PER x 64 consecutive pixels and sends ONE add per distinct root among them: a plane that fills the image would
// otherwise draw an atomic per wave onto one word.
constexpr int DP_COUNT_PER = 4;
__global__ void __launch_bounds__(256) k_dense_label_count(int32_t* __restrict__ label, int32_t* __restrict__ size, int32_t pix, int32_t total,
                                                           int32_t* __restrict__ result)
{
  const int lane = (int)(threadIdx.x & 63);
  const int64_t first = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 * DP_COUNT_PER) + lane;
  int key[DP_COUNT_PER];                                                    // the root's index in the group's arrays, -1: no valid pixel
  uint64_t pending[DP_COUNT_PER];
#pragma unroll
  for (int u = 0; u < DP_COUNT_PER; ++u) {
    const int64_t t = first + 64 * u;
    key[u] = -1;
    if (t < total) {
      const int base = (int)(t / pix) * pix;
      const int l = label[t];
      if (l >= 0) {
        bool over = false;
        const int r = dp_find<__HIP_MEMORY_SCOPE_WAVEFRONT>(label + base, l, pix, over);
        if (over) atomicOr(result, 4);
        __hip_atomic_store(label + t, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        key[u] = base + r;
      }
    }
    pending[u] = __ballot(key[u] >= 0);
  }
  // each pass retires every pixel of the wave that shares the first pending pixel's root (64 DP_COUNT_PER passes at most)
#pragma unroll
  for (int u = 0; u < DP_COUNT_PER; ++u)
    while (pending[u] != 0ull) {
      const int lead = __ffsll((long long)pending[u]) - 1;
      const int k = __shfl(key[u], lead);
      int n = 0;
#pragma unroll
      for (int w = u; w < DP_COUNT_PER; ++w) {
        const uint64_t same = __ballot(key[w] == k);
        n += (int)__popcll(same);
        pending[w] &= ~same;
      }
      if (lane == lead) atomicAdd(size + k, n);
    }
}

__global__ void __launch_bounds__(256) k_dense_speckle(const DpJob* __restrict__ jobs, const int32_t* __restrict__ label, const int32_t* __restrict__ size,
                                                       int32_t cols, int32_t pix, int32_t total, int32_t speckle_size)
{
  const int t = (int)(blockIdx.x * 256 + threadIdx.x);
  if (t >= total) return;
  const int l = label[t];
  if (l < 0) return;
  const int job = t / pix, q = t % pix;
  if (size[job * pix + l] > speckle_size) return;
  const DpJob& j = jobs[job];
  j.disp[(int64_t)(q / cols) * j.disp_stride + q % cols] = (int16_t)-16;
}

__device__ __forceinline__ int dp_wave_sum(int v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// a wave per sample row: n_srows = ceil(rows / stride) of n_scols = ceil(cols / stride) samples a job
__global__ void __launch_bounds__(256) k_dense_sample_rows(const DpJob* __restrict__ jobs, int32_t n_jobs, int32_t n_srows, int32_t n_scols, int32_t stride,
                                                           int32_t min_d, int32_t* __restrict__ row_count)
{
  const int lane = (int)(threadIdx.x & 63);
  const int w = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (w >= n_jobs * n_srows) return;
  const DpJob& j = jobs[w / n_srows];
  const int16_t* row = j.disp + (int64_t)(w % n_srows) * stride * j.disp_stride;
  int cnt = 0;
  for (int base = 0; base < n_scols; base += 64) {
    const int i = base + lane;
    const bool pass = i < n_scols && row[(int64_t)i * stride] >= min_d;
    cnt += (int)__popcll(__ballot(pass));
  }
  if (lane == 0) row_count[w] = cnt;
}

// count[job] is written by the wave of the job's last sample row.  A sample's place is below n_srows * n_scols, which the call has
// checked against the capacity.
__global__ void __launch_bounds__(256) k_dense_sample_write(const DpJob* __restrict__ jobs, int32_t n_jobs, int32_t n_srows, int32_t n_scols, int32_t stride,
                                                            int32_t min_d, const int32_t* __restrict__ row_count, int32_t* __restrict__ count)
{
  const int lane = (int)(threadIdx.x & 63);
  const int w = (int)(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (w >= n_jobs * n_srows) return;
  const int job = w / n_srows, r = w % n_srows;
  const DpJob& j = jobs[job];
  int pre = 0;
  for (int i = lane; i < r; i += 64) pre += row_count[job * n_srows + i];
  int at = dp_wave_sum(pre);
  const int v = r * stride;
  const int16_t* row = j.disp + (int64_t)v * j.disp_stride;
  const uint8_t* img = j.left + (int64_t)v * j.left_stride;
  for (int base = 0; base < n_scols; base += 64) {
    const int i = base + lane;
    const int u = i * stride;
    const int d = i < n_scols ? (int)row[u] : 0;
    const bool pass = i < n_scols && d >= min_d;
    const uint64_t m = __ballot(pass);
    if (pass) {
      const int place = at + (int)__popcll(m & ((1ull << lane) - 1ull));
      j.samples[place] = (uint64_t)(uint32_t)u | ((uint64_t)(uint32_t)v << 16) | ((uint64_t)(uint16_t)d << 32) | ((uint64_t)img[u] << 48);
    }
    at += (int)__popcll(m);
  }
  if (r == n_srows - 1 && lane == 0) count[job] = at;
}

inline int32_t dp_ceil_div(int32_t a, int32_t b) { return (a + b - 1) / b; }

// the launches of one group of g maps (table entries tab .. tab + g): the filter, then the samples of the filtered maps
ssx_status dp_launch(ssx_ctx* ctx, const DpWork& w, const DpJob* tab, int32_t g, int32_t rows, int32_t cols, const ssx_dense_post& post, int32_t* result,
                     int32_t* count, KfChainStats& st)
{
  const int32_t pix = rows * cols;
  const int32_t total = g * pix;
  const unsigned per_pixel = (unsigned)((total + 255) / 256);
  if (post.speckle_size > 0) {
    const int32_t tx = dp_ceil_div(cols, DP_TW), ty = dp_ceil_div(rows, DP_TH);
    SSX_PROF(ctx, KID_DENSE_LABEL_TILE, hipLaunchKernelGGL(k_dense_label_tile, dim3((unsigned)tx, (unsigned)ty, (unsigned)g), dim3(256), 0, ctx->stream, tab, rows, cols,
                                                          post.speckle_range, w.label, w.size, result));
    SSX_HIP_TRY(ctx, hipGetLastError());
    const int32_t n_h = (ty - 1) * cols, n_v = (tx - 1) * rows;
    const int64_t borders = (int64_t)g * (n_h + n_v);
    SSX_PROF(ctx, KID_DENSE_LABEL_MERGE, hipLaunchKernelGGL(k_dense_label_merge, dim3((unsigned)std::max<int64_t>(1, (borders + 255) / 256)), dim3(256), 0, ctx->stream, tab,
                                                           rows, cols, post.speckle_range, w.label, n_h, n_v, borders, result));
    SSX_HIP_TRY(ctx, hipGetLastError());
    SSX_PROF(ctx, KID_DENSE_LABEL_COUNT, hipLaunchKernelGGL(k_dense_label_count, dim3((unsigned)((total + 256 * DP_COUNT_PER - 1) / (256 * DP_COUNT_PER))), dim3(256), 0, ctx->stream, w.label, w.size, pix, total, result));
    SSX_HIP_TRY(ctx, hipGetLastError());
    SSX_PROF(ctx, KID_DENSE_SPECKLE, hipLaunchKernelGGL(k_dense_speckle, dim3(per_pixel), dim3(256), 0, ctx->stream, tab, w.label, w.size, cols, pix, total,
                                                       post.speckle_size));
    SSX_HIP_TRY(ctx, hipGetLastError());
    st.launches += 4;
  }
  if (post.cloud_stride > 0) {
    const int32_t n_srows = dp_ceil_div(rows, post.cloud_stride), n_scols = dp_ceil_div(cols, post.cloud_stride);
    const int32_t min_d = std::max(post.cloud_min_disp16, 1);
    const unsigned blocks = (unsigned)((g * n_srows + 3) / 4);
    SSX_PROF(ctx, KID_DENSE_SAMPLE_ROWS, hipLaunchKernelGGL(k_dense_sample_rows, dim3(blocks), dim3(256), 0, ctx->stream, tab, g, n_srows, n_scols, post.cloud_stride, min_d,
                                                           w.row_count));
    SSX_HIP_TRY(ctx, hipGetLastError());
    SSX_PROF(ctx, KID_DENSE_SAMPLE_WRITE, hipLaunchKernelGGL(k_dense_sample_write, dim3(blocks), dim3(256), 0, ctx->stream, tab, g, n_srows, n_scols, post.cloud_stride,
                                                            min_d, w.row_count, count));
    SSX_HIP_TRY(ctx, hipGetLastError());
    st.launches += 2;
  }
  return SSX_OK;
}

bool dp_bad_post(const ssx_dense_post* p, int32_t rows, int32_t cols, char* msg, size_t cap)
{
  if (p->speckle_size < 0 || (int64_t)p->speckle_size > (int64_t)rows * cols) { snprintf(msg, cap, "speckle_size = %d outside [0, rows * cols = %d]", p->speckle_size, rows * cols); return true; }
  if (p->speckle_range < 0 || p->speckle_range > 32767) { snprintf(msg, cap, "speckle_range = %d outside [0, 32767]", p->speckle_range); return true; }
  if (p->cloud_stride < 0 || p->cloud_stride > DP_MAX_STRIDE) { snprintf(msg, cap, "cloud_stride = %d outside [0, %d]", p->cloud_stride, DP_MAX_STRIDE); return true; }
  if (p->cloud_min_disp16 < 1 || p->cloud_min_disp16 > 32768) { snprintf(msg, cap, "cloud_min_disp16 = %d outside [1, 32768]", p->cloud_min_disp16); return true; }
  for (int k = 0; k < 4; ++k)
    if (p->reserved[k] != 0) { snprintf(msg, cap, "reserved is not zero"); return true; }
  return false;
}

// Both calls.  chain: the launches of ssx_stereo_dense on every group, then the post-processing of its maps; else the maps are the
// caller's, read and written in place.
ssx_status dp_run(ssx_ctx* ctx, const char* who, int32_t n, const ssx_dense_job* jobs, ssx_dense_cloud* clouds, int32_t rows, int32_t cols,
                  const ssx_dense_params* prm, bool chain, const ssx_dense_post* post, int32_t on_device)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  ctx->dense = KfChainStats{};
  ctx->dense_groups = 0;
  // every refusal comes before anything is touched
  char why[160];
  if (chain) {
    if (!prm) { ctx->set_error("%s: prm is null", who); return SSX_ERR_INVALID_ARG; }
    if (dn_bad_params(prm, why, sizeof why)) { ctx->set_error("%s: %s", who, why); return SSX_ERR_INVALID_ARG; }
  }
  if (!post) { ctx->set_error("%s: post is null", who); return SSX_ERR_INVALID_ARG; }
  if (n < 0 || n > SSX_DENSE_MAX_JOBS) { ctx->set_error("%s: n = %d outside [0, %d]", who, n, SSX_DENSE_MAX_JOBS); return SSX_ERR_INVALID_ARG; }
  if (rows < DN_MIN_SIDE || cols < DN_MIN_SIDE || rows > DN_MAX_SIDE || cols > DN_MAX_SIDE) {
    ctx->set_error("%s: %d x %d (rows x cols) outside [%d, %d] a side", who, rows, cols, DN_MIN_SIDE, DN_MAX_SIDE);
    return SSX_ERR_INVALID_ARG;
  }
  if (dp_bad_post(post, rows, cols, why, sizeof why)) { ctx->set_error("%s: %s", who, why); return SSX_ERR_INVALID_ARG; }
  const bool sampling = post->cloud_stride > 0;
  if (sampling != (clouds != nullptr)) {
    ctx->set_error("%s: clouds is %s with cloud_stride = %d (null if and only if the stride is 0)", who, clouds ? "given" : "null", post->cloud_stride);
    return SSX_ERR_INVALID_ARG;
  }
  if (n > 0 && !jobs) { ctx->set_error("%s: jobs is null", who); return SSX_ERR_INVALID_ARG; }
  const int32_t need = sampling ? dp_ceil_div(rows, post->cloud_stride) * dp_ceil_div(cols, post->cloud_stride) : 0;
  bool any_disp = false, any_scratch = false;
  for (int32_t k = 0; k < n; ++k) {
    const ssx_dense_job& j = jobs[k];
    const bool need_left = chain || sampling, need_disp = !(chain && sampling);
    const char* null_what = (need_left && !j.left) ? "left" : ((chain && !j.right) ? "right" : ((need_disp && !j.disp) ? "disp" : nullptr));
    if (null_what) { ctx->set_error("%s: job %d has a null %s", who, k, null_what); return SSX_ERR_INVALID_ARG; }
    if ((need_left && j.left_stride < cols) || (chain && j.right_stride < cols) || (j.disp && j.disp_stride < cols)) {
      ctx->set_error("%s: job %d has a stride (left %d, right %d, disp %d) smaller than cols = %d", who, k, j.left_stride, j.right_stride, j.disp_stride, cols);
      return SSX_ERR_INVALID_ARG;
    }
    if (sampling) {
      if (!clouds[k].samples) { ctx->set_error("%s: cloud %d has null samples", who, k); return SSX_ERR_INVALID_ARG; }
      if (clouds[k].capacity < need) {
        ctx->set_error("%s: cloud %d has capacity %d, below ceil(rows / stride) * ceil(cols / stride) = %d", who, k, clouds[k].capacity, need);
        return SSX_ERR_INVALID_ARG;
      }
      if (on_device != 0 && (reinterpret_cast<uintptr_t>(clouds[k].samples) & 7u) != 0) {
        ctx->set_error("%s: cloud %d has samples that are not 8-byte aligned", who, k);
        return SSX_ERR_INVALID_ARG;
      }
    }
    any_disp = any_disp || j.disp != nullptr;
    any_scratch = any_scratch || j.disp == nullptr;
  }
  if (n == 0) return SSX_OK;

  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const bool staged = on_device == 0;
  const bool filtering = post->speckle_size > 0;
  const size_t pix = (size_t)rows * (size_t)cols, N = (size_t)n;
  // One block goes up: the tables, the zeroed result block (the flag, a count per job) and, staged, the images or the maps.  One
  // comes down: the result block and, staged, the samples and the maps.  The result block belongs to both.
  Layout lay;
  const size_t o_tab = lay.take(chain ? sizeof(DnJob) * N : 0);
  const size_t o_ptab = lay.take(sizeof(DpJob) * N);
  const size_t img_per = chain ? 2 * pix : (sampling ? pix : 0);
  const size_t o_img = lay.take(staged ? img_per * N : 0);
  size_t o_map = 0;
  if (!chain && staged) o_map = lay.take(2 * pix * N);
  const size_t o_res = lay.take(4 * (1 + N));
  const size_t up_bytes = lay.off;
  const size_t o_smp = lay.take(staged ? 8 * (size_t)need * N : 0);
  const size_t smp_end = lay.off;
  if (chain && (staged || any_scratch)) o_map = lay.take(2 * pix * N);
  size_t down_from = o_res, down_to = o_res + 4 * (1 + N);
  if (staged) {
    if (chain) down_to = any_disp ? lay.off : smp_end;
    else { down_from = filtering ? o_map : o_res; down_to = smp_end; }
  }
  SSX_HIP_TRY(ctx, ctx->dn_arena.reserve(lay.off));
  SSX_HIP_TRY(ctx, ctx->dn_stage.reserve(lay.off));
  DnWork w;
  DpWork pw;
  int32_t group;
  if (chain) {
    group = dn_group_size(ctx, pix, prm->disparities, n);
    SSX_HIP_TRY(ctx, ctx->dn_work.reserve(dn_carve(w, nullptr, (size_t)group, pix, prm->disparities), 1.0));
    dn_carve(w, ctx->dn_work.as<char>(), (size_t)group, pix, prm->disparities);
    // the census words (16 bytes a pixel) are dead once the paths kernel is done: labels, sizes and row counts (8 bytes a pixel and 4 a
    // row, and a row has at least 40 pixels) take their place
    pw.label = reinterpret_cast<int32_t*>(w.census);
    pw.size = pw.label + (size_t)group * pix;
    pw.row_count = pw.size + (size_t)group * pix;
  } else {
    group = (int32_t)std::min<size_t>(std::max<size_t>(1, dn_cap(ctx) / dp_job_bytes(pix, rows)), N);
    SSX_HIP_TRY(ctx, ctx->dn_work.reserve(dp_carve(pw, nullptr, (size_t)group, pix, rows), 1.0));
    dp_carve(pw, ctx->dn_work.as<char>(), (size_t)group, pix, rows);
  }
  char* dev = ctx->dn_arena.as<char>();
  char* stage = ctx->dn_stage.as<char>();
  KfChainStats st{};

  DnJob* tab = reinterpret_cast<DnJob*>(stage + o_tab);
  DpJob* ptab = reinterpret_cast<DpJob*>(stage + o_ptab);
  std::memset(stage + o_res, 0, 4 * (1 + N));
  for (int32_t k = 0; k < n; ++k) {
    const ssx_dense_job& j = jobs[k];
    DpJob& p = ptab[k];
    int16_t* own_map = reinterpret_cast<int16_t*>(dev + o_map + 2 * pix * (size_t)k);
    if (staged) {
      uint8_t* l = reinterpret_cast<uint8_t*>(stage + o_img + img_per * (size_t)k);
      if (img_per > 0)
        for (int32_t y = 0; y < rows; ++y) std::memcpy(l + (size_t)y * cols, j.left + (size_t)y * j.left_stride, (size_t)cols);
      if (chain)
        for (int32_t y = 0; y < rows; ++y) std::memcpy(l + pix + (size_t)y * cols, j.right + (size_t)y * j.right_stride, (size_t)cols);
      else {
        int16_t* m = reinterpret_cast<int16_t*>(stage + o_map + 2 * pix * (size_t)k);
        for (int32_t y = 0; y < rows; ++y) std::memcpy(m + (size_t)y * cols, j.disp + (size_t)y * j.disp_stride, 2 * (size_t)cols);
      }
      p.disp = own_map;
      p.left = reinterpret_cast<const uint8_t*>(dev + o_img + img_per * (size_t)k);
      p.samples = reinterpret_cast<uint64_t*>(dev + o_smp + 8 * (size_t)need * (size_t)k);
      p.disp_stride = p.left_stride = cols;
    } else {
      p.disp = j.disp ? j.disp : own_map;
      p.left = j.left;
      p.samples = sampling ? reinterpret_cast<uint64_t*>(clouds[k].samples) : nullptr;
      p.disp_stride = j.disp ? j.disp_stride : cols;
      p.left_stride = j.left_stride;
    }
    if (chain) {
      DnJob& t = tab[k];
      t.reserved = 0;
      t.left = p.left; t.right = staged ? p.left + pix : j.right; t.disp = p.disp;
      t.left_stride = p.left_stride; t.right_stride = staged ? cols : j.right_stride; t.disp_stride = p.disp_stride;
    }
  }
  SSX_HIP_TRY(ctx, hipMemcpyAsync(dev, stage, up_bytes, hipMemcpyHostToDevice, ctx->stream));
  st.bytes_up += (int64_t)up_bytes;
  const DnJob* dtab = reinterpret_cast<const DnJob*>(dev + o_tab);
  const DpJob* dptab = reinterpret_cast<const DpJob*>(dev + o_ptab);
  int32_t* dres = reinterpret_cast<int32_t*>(dev + o_res);
  int32_t groups = 0;
  for (int32_t first = 0; first < n; first += group, ++groups) {
    const int32_t g = std::min(group, n - first);
    ssx_status s = SSX_OK;
    if (chain) {
      s = dn_volume(ctx, w, dtab + first, g, rows, cols, *prm, 0, prm->paths, true, st);
      if (s == SSX_OK && prm->lr_tolerance >= 0) s = dn_right(ctx, w, g, rows, cols, prm->disparities, st);
      if (s == SSX_OK) s = dn_select(ctx, w, dtab + first, g, rows, cols, *prm, st);
    }
    if (s == SSX_OK) s = dp_launch(ctx, pw, dptab + first, g, rows, cols, *post, dres, dres + 1 + first, st);
    if (s != SSX_OK) return s;
  }
  SSX_HIP_TRY(ctx, hipMemcpyAsync(stage + down_from, dev + down_from, down_to - down_from, hipMemcpyDeviceToHost, ctx->stream));
  st.bytes_down += (int64_t)(down_to - down_from);
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ++st.syncs;
  ctx->dense = st;
  ctx->dense_groups = groups;
  const int32_t* res = reinterpret_cast<const int32_t*>(stage + o_res);
  if (res[0] != 0) {
    ctx->set_error("%s: a labelling loop passed its bound (flags %d); the maps and the samples are not to be used", who, res[0]);
    return SSX_ERR_HIP;
  }
  const bool maps_down = staged && (chain ? any_disp : filtering);
  for (int32_t k = 0; k < n; ++k) {
    if (maps_down && jobs[k].disp) {
      const int16_t* d = reinterpret_cast<const int16_t*>(stage + o_map + 2 * pix * (size_t)k);
      for (int32_t y = 0; y < rows; ++y) std::memcpy(jobs[k].disp + (size_t)y * jobs[k].disp_stride, d + (size_t)y * cols, 2 * (size_t)cols);
    }
    if (sampling) {
      const int32_t c = res[1 + k];
      if (staged) std::memcpy(clouds[k].samples, stage + o_smp + 8 * (size_t)need * (size_t)k, 8 * (size_t)c);
      clouds[k].count = c;
    }
  }
  return SSX_OK;
}

}  // namespace

static_assert(sizeof(ssx_dense_post) == 32 && sizeof(ssx_dense_sample) == 8 && sizeof(ssx_dense_cloud) == 16, "include/ssx.h");
static_assert(sizeof(DpJob) == 32, "the table of the post-processing kernels");

extern "C" {

void ssx_dense_default_post(ssx_dense_post* p)
{
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->speckle_range = 16;
  p->cloud_min_disp16 = 1;
}

// the contract's min_disp16: the first d whose depth is within max_depth; the correctly rounded quotient is monotone in d
int32_t ssx_dense_min_disp16(double bf, double max_depth)
{
  int32_t lo = 1, hi = 32768;
  while (lo < hi) {
    const int32_t mid = (lo + hi) / 2;
    if (bf * 16.0 / (double)mid <= max_depth) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

ssx_status ssx_dense_postprocess(ssx_ctx* ctx, int32_t n, const ssx_dense_job* jobs, ssx_dense_cloud* clouds, int32_t rows, int32_t cols, const ssx_dense_post* post,
                                 int32_t on_device)
{
  return dp_run(ctx, "ssx_dense_postprocess", n, jobs, clouds, rows, cols, nullptr, false, post, on_device);
}

ssx_status ssx_stereo_dense_post(ssx_ctx* ctx, int32_t n, const ssx_dense_job* jobs, ssx_dense_cloud* clouds, int32_t rows, int32_t cols, const ssx_dense_params* prm,
                                 const ssx_dense_post* post, int32_t images_on_device)
{
  return dp_run(ctx, "ssx_stereo_dense_post", n, jobs, clouds, rows, cols, prm, true, post, images_on_device);
}

#ifndef SSX_NO_TEST_HOOKS   // include/ssx_test_hooks.h

// size and root per pixel of ONE host map, through the labelling kernels of the calls above; not a fast path
ssx_status ssx_dense_debug_components(ssx_ctx* ctx, const int16_t* disp, int32_t disp_stride, int32_t rows, int32_t cols, int32_t speckle_range, int32_t* size,
                                      int32_t* root)
{
  if (!ctx) return SSX_ERR_INVALID_ARG;
  const char* who = "ssx_dense_debug_components";
  if (!disp || rows < DN_MIN_SIDE || cols < DN_MIN_SIDE || rows > DN_MAX_SIDE || cols > DN_MAX_SIDE || disp_stride < cols || speckle_range < 0 || speckle_range > 32767) {
    ctx->set_error("%s: a null map, %d x %d, a stride or a range out of range", who, rows, cols);
    return SSX_ERR_INVALID_ARG;
  }
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t pix = (size_t)rows * cols;
  Layout lay;
  const size_t o_ptab = lay.take(sizeof(DpJob));
  const size_t o_res = lay.take(8);
  const size_t o_map = lay.take(2 * pix);
  SSX_HIP_TRY(ctx, ctx->dn_arena.reserve(lay.off));
  DpWork pw;
  SSX_HIP_TRY(ctx, ctx->dn_work.reserve(dp_carve(pw, nullptr, 1, pix, rows), 1.0));
  dp_carve(pw, ctx->dn_work.as<char>(), 1, pix, rows);
  char* dev = ctx->dn_arena.as<char>();
  std::vector<char> up(lay.off, 0);
  DpJob* p = reinterpret_cast<DpJob*>(up.data() + o_ptab);
  p->disp = reinterpret_cast<int16_t*>(dev + o_map);
  p->disp_stride = cols;
  for (int32_t y = 0; y < rows; ++y) std::memcpy(up.data() + o_map + 2 * (size_t)y * cols, disp + (size_t)y * disp_stride, 2 * (size_t)cols);
  SSX_HIP_TRY(ctx, hipMemcpyAsync(dev, up.data(), up.size(), hipMemcpyHostToDevice, ctx->stream));
  ssx_dense_post post;
  ssx_dense_default_post(&post);
  post.speckle_size = (int32_t)pix;                                        // every component is a speckle: the map on the device is scratch
  post.speckle_range = speckle_range;
  KfChainStats st{};
  int32_t* dres = reinterpret_cast<int32_t*>(dev + o_res);
  const ssx_status s = dp_launch(ctx, pw, reinterpret_cast<const DpJob*>(dev + o_ptab), 1, rows, cols, post, dres, dres + 1, st);
  if (s != SSX_OK) return s;
  std::vector<int32_t> lab(pix), siz(pix);
  int32_t flag = 0;
  SSX_HIP_TRY(ctx, hipMemcpyAsync(lab.data(), pw.label, pix * 4, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(siz.data(), pw.size, pix * 4, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipMemcpyAsync(&flag, dres, 4, hipMemcpyDeviceToHost, ctx->stream));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (flag != 0) { ctx->set_error("%s: a labelling loop passed its bound (flags %d)", who, flag); return SSX_ERR_HIP; }
  for (size_t k = 0; k < pix; ++k) {
    if (root) root[k] = lab[k];
    if (size) size[k] = lab[k] >= 0 ? siz[(size_t)lab[k]] : 0;
  }
  return SSX_OK;
}

#endif

}  // extern "C"
