// ssvio_amd/csrc/loop_guided.inc -- the guided search of relocalisation (included at the end of loop.hip; the rule: tools/guided_model.py).
//
// Behind an accepted candidate the host projects the candidate's local map into the frame with the pose just found; each point looks
// for its feature in a small window round its projection.  The stored keyframes' descriptors and class ids are in the arena, the
// frame's are what describe_enqueue leaves (or a caller's arrays), the points and the pose come up with the call.
//
// k_kfdb_project  one wavefront per point, four per workgroup.  Every lane projects the point (the same f64 operations in every lane,
//                 each rounded on its own: loop.hip is compiled with -ffp-contract=off).  The lanes scan the keyframe's class ids in
//                 64-entry chunks and collect the point's descriptors with ballot and prefix, in order, into the wave's LDS slice of
//                 kGuidedBatch descriptors; a class with more is taken batch by batch.  Per batch the lanes stride over the frame's
//                 DESCRIPTORS: taken[c], the window on feat_xy[c], and inside it the minimum over the batch of 4 x __popcll.  A lane
//                 keeps its best two keys (d << 32) | c with distinct c; a key of a class it already holds lowers that entry, so the
//                 two are the lane's best two CLASSES whatever the order of descriptors and batches.  The wave's best is a
//                 min-reduction, its second a min-reduction over each lane's best key of another class than the winner's.  Integer
//                 minima only: a pure function of the inputs.
// k_kfdb_claim    a thread per point, launched twice.  <0>: an accepted point lowers its feature's word (preset to all ones) with one
//                 64-bit atomicMin of (d1 << 32) | point.  <1>, behind the launch boundary: it reads the word and is MATCHED or
//                 CLAIMED; the matched are counted with an integer atomicAdd.
// Three launches, one result block, one synchronisation, whatever P, F, n_cur and the number of stored keyframes are.

namespace {

constexpr int kGuidedWaves = 4;     // wavefronts (points) per workgroup of k_kfdb_project
constexpr int kGuidedBatch = 64;    // descriptors of a point a wavefront holds in LDS at once
constexpr unsigned long long kNoKey = ~0ull;

struct GuidedCam { double K[4]; double T[12]; double radius; int32_t rows, cols, max_distance, ratio_pct; };
struct GuidedIn {
  const char* arena; const KfRow* rows;                                        // the database
  const double* xyz; const int32_t* prow; const int32_t* pcls; int32_t P;      // the points: position, row of the keyframe (-1: unknown), class id there
  const float* feat_xy; const uint8_t* taken; int32_t F;                       // the frame's features (taken null: none is)
  // the frame's descriptors: a caller's (cur_cls) or describe_enqueue's, read in place (cur_kps[j].class_id, where keep[j])
  const uint8_t* cur_desc; const int32_t* cur_cls; const ssx_keypoint* cur_kps; const uint8_t* keep; int32_t n_cur;
};
struct GuidedHdr { int32_t n_matched, pad[3]; };
struct GuidedOut { GuidedHdr* hdr; int32_t* feat; int32_t* d1; int32_t* d2; int32_t* status; double* uv; unsigned long long* words; };

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long m)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = min(m, (unsigned long long)__shfl_xor((long long)m, o));
  return m;
}

__global__ __launch_bounds__(64 * kGuidedWaves) void k_kfdb_project(GuidedIn in, GuidedCam cam, GuidedOut out)
{
  __shared__ unsigned long long s_desc[kGuidedWaves][kGuidedBatch][4];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && threadIdx.x == 0) out.hdr->n_matched = 0;             // k_kfdb_claim<1>, two launches on, counts into it
  const int p = blockIdx.x * kGuidedWaves + wave;
  if (p >= in.P) return;                                                       // (a whole wavefront: the kernel has no block-wide barrier)
  const double X = in.xyz[3 * (size_t)p], Y = in.xyz[3 * (size_t)p + 1], Z = in.xyz[3 * (size_t)p + 2];
  const double* T = cam.T;
  const double xc = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
  const double yc = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
  const double zc = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
  int status = SSX_GUIDED_MATCHED, feat = -1, d1 = -1, d2 = -1;
  double u = 0.0, v = 0.0;
  if (!(isfinite(xc) && isfinite(yc) && isfinite(zc)) || !(zc > 0.0)) {
    status = SSX_GUIDED_BEHIND;
  } else {
    u = cam.K[0] * (xc / zc) + cam.K[2];
    v = cam.K[1] * (yc / zc) + cam.K[3];
    if (!(u >= 0.0 && u < (double)cam.cols && v >= 0.0 && v < (double)cam.rows)) status = SSX_GUIDED_OUTSIDE;
  }
  if (status == SSX_GUIDED_MATCHED) {                                          // (every lane holds the same values: the branches are wave-uniform)
    const int row = in.prow[p], cls = in.pcls[p];
    const KfRow r = row >= 0 ? in.rows[row] : KfRow{0, 0, -1};
    unsigned long long k1 = kNoKey, k2 = kNoKey;                               // the lane's best two keys, of distinct classes
    // the frame's descriptors against the `fill` descriptors of the point in the wave's LDS slice
    auto scan = [&](int fill) __attribute__((always_inline)) {
      for (int j = lane; j < in.n_cur; j += 64) {
        if (in.keep && !in.keep[j]) continue;
        const int c = in.cur_kps ? in.cur_kps[j].class_id : in.cur_cls[j];
        if ((unsigned)c >= (unsigned)in.F) continue;                           // (refused by the host for a caller's arrays; describe writes the feature's index)
        if (in.taken && in.taken[c]) continue;
        const double x = (double)in.feat_xy[2 * (size_t)c], y = (double)in.feat_xy[2 * (size_t)c + 1];
        if (!(fabs(x - u) <= cam.radius && fabs(y - v) <= cam.radius)) continue;
        const unsigned long long* b = reinterpret_cast<const unsigned long long*>(in.cur_desc + (size_t)32 * j);
        const unsigned long long b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
        int d = 257;
        for (int q = 0; q < fill; ++q) {
          const unsigned long long* a = s_desc[wave][q];
          d = min(d, __popcll(a[0] ^ b0) + __popcll(a[1] ^ b1) + __popcll(a[2] ^ b2) + __popcll(a[3] ^ b3));
        }
        const unsigned long long key = ((unsigned long long)(unsigned)d << 32) | (unsigned)c;
        if ((unsigned)k1 == (unsigned)c) {
          k1 = min(k1, key);
        } else if ((unsigned)k2 == (unsigned)c) {
          k2 = min(k2, key);
          if (k2 < k1) { const unsigned long long t = k1; k1 = k2; k2 = t; }
        } else if (key < k1) {
          k2 = k1; k1 = key;
        } else if (key < k2) {
          k2 = key;
        }
      }
    };
    bool any = false;
    if (r.n_desc > 0) {
      const char* blob = in.arena + r.off;
      const int32_t* kcls = reinterpret_cast<const int32_t*>(blob + blob_class(r.n_bow));
      const unsigned long long* kdesc = reinterpret_cast<const unsigned long long*>(blob + blob_desc(r.n_bow, r.n_desc));
      int fill = 0;
      for (int base = 0; base < r.n_desc; base += 64) {
        const int k = base + lane;
        const bool hit = k < r.n_desc && kcls[k] == cls;
        const unsigned long long m = __ballot(hit);
        const int cnt = __popcll(m);
        if (cnt == 0) continue;
        any = true;
        if (fill + cnt > kGuidedBatch) {                                       // the slice is full: its batch first
          scan(fill);
          fill = 0;
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();                                     // every lane has read the batch before it is overwritten
        }
        if (hit) {
          const int pos = fill + __popcll(m & ((1ull << lane) - 1));           // in stored order
          const unsigned long long* a = kdesc + (size_t)4 * k;
          s_desc[wave][pos][0] = a[0]; s_desc[wave][pos][1] = a[1]; s_desc[wave][pos][2] = a[2]; s_desc[wave][pos][3] = a[3];
        }
        fill += cnt;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();                                       // the wave's own writes, before any lane reads them
      }
      if (fill > 0) scan(fill);
    }
    if (!any) {
      status = SSX_GUIDED_NO_DESCRIPTOR;
    } else {
      const unsigned long long best = wave_min_u64(k1);
      const unsigned long long second = wave_min_u64((unsigned)k1 == (unsigned)best ? k2 : k1);   // each lane's best of another class
      if (best == kNoKey) {
        status = SSX_GUIDED_NO_FEATURE;
      } else {
        d1 = (int)(best >> 32);
        d2 = second == kNoKey ? -1 : (int)(second >> 32);
        if (d1 > cam.max_distance) status = SSX_GUIDED_DISTANCE;
        else if (d2 >= 0 && !(100 * d1 < cam.ratio_pct * d2)) status = SSX_GUIDED_RATIO;
        else feat = (int)(unsigned)best;                                       // accepted: MATCHED until k_kfdb_claim says otherwise
      }
    }
  }
  if (lane == 0) {
    out.feat[p] = feat; out.d1[p] = d1; out.d2[p] = d2; out.status[p] = status;
    out.uv[2 * (size_t)p] = u; out.uv[2 * (size_t)p + 1] = v;
  }
}

template <int PHASE>
__global__ __launch_bounds__(256) void k_kfdb_claim(int P, GuidedOut out)
{
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P || out.status[p] != SSX_GUIDED_MATCHED) return;
  const int f = out.feat[p];
  if (PHASE == 0) {
    atomicMin(&out.words[f], ((unsigned long long)(unsigned)out.d1[p] << 32) | (unsigned)p);   // the lowest d1, then the lowest point
  } else if ((unsigned)out.words[f] == (unsigned)p) {
    atomicAdd(&out.hdr->n_matched, 1);
  } else {
    out.status[p] = SSX_GUIDED_CLAIMED; out.feat[p] = -1;                      // no fall-back to its second
  }
}

// what both entry points share: the arguments but for the frame's descriptors
struct GuidedArgs {
  const double* K4; const double* T; int32_t rows, cols, F; const uint8_t* taken; int32_t P; const int64_t* point_kf; const int32_t* point_cls; const double* xyz;
  double radius; int32_t max_distance, ratio_pct; int32_t* feat_out; int32_t* d1_out; int32_t* d2_out; int32_t* status_out; double* uv_out; int32_t* n_matched;
};
bool guided_args_ok(const GuidedArgs& a)
{
  if (!a.K4 || !a.T || a.P < 0 || a.F < 0 || a.rows <= 0 || a.cols <= 0 || !a.n_matched) return false;
  if (a.P > 0 && (!a.point_kf || !a.point_cls || !a.xyz || !a.feat_out || !a.d1_out || !a.d2_out || !a.status_out)) return false;
  if (!std::isfinite(a.radius) || a.radius < 0.0 || a.max_distance < 0 || a.max_distance > 256 || a.ratio_pct < 0 || a.ratio_pct > 100) return false;
  for (int k = 0; k < 4; ++k) if (!std::isfinite(a.K4[k])) return false;
  for (int k = 0; k < 12; ++k) if (!std::isfinite(a.T[k])) return false;
  return true;
}
ssx_status guided_points_bound(ssx_ctx* ctx, const char* who, int P)
{
  if (P <= 65535) return SSX_OK;
  ctx->set_error("%s: %d points: more than 65535", who, P);
  return SSX_ERR_UNSUPPORTED;
}

// The frame's side: a caller's arrays, which go up with the points (host_desc, host_cls), or what describe_enqueue left on the device.
struct GuidedFrame {
  const float* feat_xy = nullptr; const ssx_keypoint* features = nullptr;     // positions as [F, 2] floats or as keypoints, on the host
  int n_cur = 0; const uint8_t* host_desc = nullptr; const int32_t* host_cls = nullptr;
  const uint8_t* dev_desc = nullptr; const ssx_keypoint* dev_kps = nullptr; const uint8_t* dev_keep = nullptr;
};

// One upload [points | features | (descriptors)], k_kfdb_project, k_kfdb_claim twice, one copy of the result block, ONE synchronisation.
ssx_status guided_run(ssx_kf_database* db, const GuidedArgs& a, const GuidedFrame& fr, KfChainStats& st)
{
  ssx_ctx* ctx = db->ctx;
  const int P = a.P, F = a.F, n_cur = fr.n_cur;
  const bool up_desc = fr.host_desc != nullptr && n_cur > 0;
  double* d_xyz; int32_t* d_prow; int32_t* d_pcls; float* d_xy; uint8_t* d_taken; uint8_t* d_desc; int32_t* d_cls; char* d_end_in;
  GuidedOut o{};
  char* d_end;
  auto bufs = [&](auto&& f) {
    f(d_xyz, (size_t)24 * P); f(d_prow, (size_t)4 * P); f(d_pcls, (size_t)4 * P); f(d_xy, (size_t)8 * F); f(d_taken, a.taken ? (size_t)F : 0);
    f(d_desc, up_desc ? (size_t)32 * n_cur : 0); f(d_cls, up_desc ? (size_t)4 * n_cur : 0); f(d_end_in, 0);
    f(o.words, (size_t)8 * F);
    f(o.hdr, sizeof(GuidedHdr)); f(o.feat, (size_t)4 * P); f(o.d1, (size_t)4 * P); f(o.d2, (size_t)4 * P); f(o.status, (size_t)4 * P); f(o.uv, (size_t)16 * P);
    f(d_end, 0);
  };
  const size_t total = carve(nullptr, bufs);
  SSX_HIP_TRY(ctx, db->io.reserve(total));
  SSX_HIP_TRY(ctx, db->stage.reserve(total));
  char* base = db->io.as<char>();
  char* hs = db->stage.as<char>();
  carve(base, bufs);
  auto host = [&](const void* dev) { return hs + ((const char*)dev - base); };
  // the points: the keyframe's id resolved to its row through the host mirror, -1 for an id that is not stored
  if (P > 0) {
    memcpy(host(d_xyz), a.xyz, (size_t)24 * P);
    memcpy(host(d_pcls), a.point_cls, (size_t)4 * P);
    int32_t* prow = (int32_t*)host(d_prow);
    for (int p = 0; p < P; ++p) {
      const auto it = std::lower_bound(db->ids.begin(), db->ids.end(), a.point_kf[p]);
      prow[p] = (it != db->ids.end() && *it == a.point_kf[p]) ? (int32_t)(it - db->ids.begin()) : -1;
    }
  }
  if (F > 0) {
    float* xy = (float*)host(d_xy);
    if (fr.feat_xy) memcpy(xy, fr.feat_xy, (size_t)8 * F);
    else for (int i = 0; i < F; ++i) { xy[2 * i] = fr.features[i].x; xy[2 * i + 1] = fr.features[i].y; }
    if (a.taken) memcpy(host(d_taken), a.taken, (size_t)F);
  }
  if (up_desc) { memcpy(host(d_desc), fr.host_desc, (size_t)32 * n_cur); memcpy(host(d_cls), fr.host_cls, (size_t)4 * n_cur); }
  const size_t in_bytes = (size_t)(d_end_in - base), o_res = (size_t)((char*)o.hdr - base), res_bytes = (size_t)(d_end - (char*)o.hdr);
  hipStream_t s = ctx->stream;
  if (in_bytes) SSX_HIP_TRY(ctx, hipMemcpyAsync(base, hs, in_bytes, hipMemcpyHostToDevice, s));
  if (F > 0) SSX_HIP_TRY(ctx, hipMemsetAsync(o.words, 0xff, (size_t)8 * F, s));
  GuidedIn in{};
  in.arena = db->arena.as<char>(); in.rows = db->table.as<KfRow>();
  in.xyz = d_xyz; in.prow = d_prow; in.pcls = d_pcls; in.P = P;
  in.feat_xy = d_xy; in.taken = a.taken ? d_taken : nullptr; in.F = F;
  in.n_cur = n_cur;
  if (up_desc) { in.cur_desc = d_desc; in.cur_cls = d_cls; }
  else { in.cur_desc = fr.dev_desc; in.cur_kps = fr.dev_kps; in.keep = fr.dev_keep; if (!fr.dev_desc) in.n_cur = 0; }
  GuidedCam cam{};
  memcpy(cam.K, a.K4, sizeof cam.K); memcpy(cam.T, a.T, sizeof cam.T);
  cam.radius = a.radius; cam.rows = a.rows; cam.cols = a.cols; cam.max_distance = a.max_distance; cam.ratio_pct = a.ratio_pct;
  // (the grids never shrink to nothing: P == 0 issues the same three launches, whose wavefronts exit)
  const int g_project = std::max((P + kGuidedWaves - 1) / kGuidedWaves, 1), g_claim = std::max((P + 255) / 256, 1);
  SSX_PROF(ctx, KID_LOOP_GUIDED, hipLaunchKernelGGL(k_kfdb_project, dim3(g_project), dim3(64 * kGuidedWaves), 0, s, in, cam, o));
  SSX_PROF(ctx, KID_LOOP_GUIDED, hipLaunchKernelGGL(k_kfdb_claim<0>, dim3(g_claim), dim3(256), 0, s, P, o));
  SSX_PROF(ctx, KID_LOOP_GUIDED, hipLaunchKernelGGL(k_kfdb_claim<1>, dim3(g_claim), dim3(256), 0, s, P, o));
  SSX_HIP_TRY(ctx, hipGetLastError());
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + o_res, o.hdr, res_bytes, hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  st.launches += 3; ++st.syncs; st.bytes_up += (int64_t)in_bytes; st.bytes_down += (int64_t)res_bytes;
  *a.n_matched = ((const GuidedHdr*)host(o.hdr))->n_matched;
  if (P > 0) {
    memcpy(a.feat_out, host(o.feat), (size_t)4 * P); memcpy(a.d1_out, host(o.d1), (size_t)4 * P); memcpy(a.d2_out, host(o.d2), (size_t)4 * P);
    memcpy(a.status_out, host(o.status), (size_t)4 * P);
    if (a.uv_out) memcpy(a.uv_out, host(o.uv), (size_t)16 * P);
  }
  return SSX_OK;
}

}  // namespace

extern "C" {

ssx_status ssx_kfdb_project_match(ssx_kf_database* db, const double* K4, const double* T_cw12, int32_t rows, int32_t cols, int32_t F, const float* feat_xy,
                                  const uint8_t* taken, int32_t n_cur, const uint8_t* cur_desc, const int32_t* cur_cls, int32_t P, const int64_t* point_kf,
                                  const int32_t* point_cls, const double* xyz, double radius, int32_t max_distance, int32_t ratio_pct, int32_t* feat_out,
                                  int32_t* d1_out, int32_t* d2_out, int32_t* status_out, double* uv_out, int32_t* n_matched)
{
  static const char* const who = "ssx_kfdb_project_match";
  const GuidedArgs a{K4, T_cw12, rows, cols, F, taken, P, point_kf, point_cls, xyz, radius, max_distance, ratio_pct, feat_out, d1_out, d2_out, status_out, uv_out, n_matched};
  if (!db || !guided_args_ok(a) || n_cur < 0 || (F > 0 && !feat_xy) || (n_cur > 0 && (!cur_desc || !cur_cls))) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = db->ctx;
  for (int32_t j = 0; j < n_cur; ++j)
    if (cur_cls[j] < 0 || cur_cls[j] >= F) { ctx->set_error("%s: descriptor %d has class id %d outside [0, %d)", who, j, cur_cls[j], F); return SSX_ERR_INVALID_ARG; }
  if (ssx_status s = guided_points_bound(ctx, who, P)) return s;
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  GuidedFrame fr; fr.feat_xy = feat_xy; fr.n_cur = n_cur; fr.host_desc = cur_desc; fr.host_cls = cur_cls;
  KfChainStats st{};
  return guided_run(db, a, fr, st);
}

ssx_status ssx_kfdb_guided_search(ssx_kf_database* db, const uint8_t* img, int32_t stride, int32_t rows, int32_t cols, const ssx_orb_params* prm, int32_t n_features,
                                  const ssx_keypoint* features, int32_t pyramid_levels, const uint8_t* taken, const double* K4, const double* T_cw12, int32_t P,
                                  const int64_t* point_kf, const int32_t* point_cls, const double* xyz, double radius, int32_t max_distance, int32_t ratio_pct,
                                  int32_t* feat_out, int32_t* d1_out, int32_t* d2_out, int32_t* status_out, double* uv_out, int32_t* n_matched)
{
  static const char* const who = "ssx_kfdb_guided_search";
  const FrameArgs fa{img, stride, rows, cols, prm, n_features, features, pyramid_levels, 0, nullptr};
  const GuidedArgs a{K4, T_cw12, rows, cols, n_features, taken, P, point_kf, point_cls, xyz, radius, max_distance, ratio_pct, feat_out, d1_out, d2_out, status_out, uv_out,
                     n_matched};
  if (!db || !frame_args_ok(fa) || !guided_args_ok(a)) return SSX_ERR_INVALID_ARG;
  ssx_ctx* ctx = db->ctx;
  if (ssx_status s = check_pyramid_bound(ctx, who, -1, fa)) return s;
  if (ssx_status s = guided_points_bound(ctx, who, P)) return s;
  db->last = KfChainStats{};
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  KfChainStats st{};
  GuidedFrame fr; fr.features = features;
  const int N = n_features * pyramid_levels;
  if (N > 0) {                                                // the frame described exactly as the query describes it; its arrays are read where they lie
    ssxorb::Described d;
    if (ssx_status s = ssxorb::describe_enqueue(ctx, img, stride, rows, cols, *prm, features, n_features, pyramid_levels, &d)) return s;
    st.launches += d.launches; st.syncs += d.syncs; st.bytes_up += (int64_t)d.bytes_up;
    fr.n_cur = N; fr.dev_desc = d.desc; fr.dev_kps = d.kps; fr.dev_keep = d.keep;
  }
  const ssx_status rs = guided_run(db, a, fr, st);
  if (rs == SSX_OK) db->last = st;
  return rs;
}

}  // extern "C"
