// ssvio_amd/csrc/pg.inc -- pose-graph optimisation (SURVEY.md section 8-F, N3), included at the end of ba.hip.
//
// Replaces the optimisation of LoopClosing::PoseGraphOptimization (/root/reference/src/ssvio/loopclosing.cpp:458-539):
// VertexPose per keyframe (initial / active / loop keyframes fixed), EdgePoseGraph per temporal or loop constraint
// (include/ssvio/g2otypes.hpp:164-199: e = log(M^-1 T_i T_j^-1), information = I, no robust kernel, g2o's numeric
// Jacobians), BlockSolver<6,6> + LinearSolverEigen + OptimizationAlgorithmLevenberg, optimize(20).
// No vertex is marginalised, so there is no Schur complement: the system matrix is the block-sparse Hpp itself (a
// chain plus loop closures = block-banded), and the solve is the tile-sparse blocked Cholesky of the large-window
// bundle adjustment (ba_big.inc: k_potrf64 / k_trsm64 / k_syrk64 on v_mfma_f64_16x16x4_f64, k_backsolve).
//   k_pg_linearize   one thread per edge: error, numeric Jacobians (24 error evaluations), the edge's 6x6 blocks
//                    J_i^T J_i, J_i^T J_j, J_j^T J_j and -J^T e
//   k_pg_assemble    one 64-thread workgroup per non-zero block: sums its edges' contributions in list order
//                    (deterministic), writes both triangles of the dense matrix, the rhs row, max |diag|
//   k_pg_reduce      chi2 = sum e^T e (fixed tree)
// The LM control loop is the one of ssx_ba_solve (optimization_algorithm_levenberg.cpp:58-175), on the host.
namespace {

constexpr int PG_EBLK = 36 * 3 + 12;       // doubles per edge: Aii | Aij | Ajj | gi | gj

struct PgDev {
  int P, E, nP, nBlk;
  const int* ei; const int* ej;
  const double* meas;                       // [E][7]
  const uint8_t* active;                    // [E] at least one free vertex
  double* eblk;                             // [E][PG_EBLK]
  double* err;                              // [E][6]
  const int* blk_pa; const int* blk_pb;     // nBlk blocks, pa <= pb (free indices); the first nP are the diagonal
  const int* blk_ptr;                       // nBlk+1
  const int* blk_item;                      // edge * 4 + kind: 0 Aii, 1 Ajj, 2 Aij, 3 Aij^T
  const int* g_ptr;                         // nP+1
  const int* g_item;                        // edge * 2 + (0: gi, 1: gj)
  double* maxd;                             // nP: max |diag| of each diagonal block
};

__global__ __launch_bounds__(64) void k_pg_linearize(BaDev d, PgDev g, int cur, int with_jac)
{
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= g.E) return;
  double* er = g.err + 6 * (size_t)e;
  if (!g.active[e]) { for (int r = 0; r < 6; ++r) er[r] = 0.0; return; }
  const int vi = g.ei[e], vj = g.ej[e];
  double M[7], T0[7], T1[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) { M[k] = g.meas[7 * (size_t)e + k]; T0[k] = d.pose[cur][7 * (size_t)vi + k]; T1[k] = d.pose[cur][7 * (size_t)vj + k]; }
  double err[6];
  ssx::pg_error(M, T0, T1, err);
#pragma unroll
  for (int r = 0; r < 6; ++r) er[r] = err[r];
  if (!with_jac) return;
  const bool fi = d.pose_free[vi] >= 0, fj = d.pose_free[vj] >= 0;
  double Ji[36], Jj[36];
  for (int k = 0; k < 36; ++k) { Ji[k] = 0.0; Jj[k] = 0.0; }
  if (fi) ssx::pg_jac_numeric(M, T0, T1, 0, Ji);
  if (fj) ssx::pg_jac_numeric(M, T0, T1, 1, Jj);
  double* o = g.eblk + (size_t)PG_EBLK * e;
  for (int r = 0; r < 6; ++r) {
    double gi = 0.0, gj = 0.0;
    for (int m = 0; m < 6; ++m) { gi += Ji[m * 6 + r] * (-err[m]); gj += Jj[m * 6 + r] * (-err[m]); }
    o[108 + r] = gi; o[114 + r] = gj;
    for (int c = 0; c < 6; ++c) {
      double hii = 0.0, hij = 0.0, hjj = 0.0;
      for (int m = 0; m < 6; ++m) {
        hii += Ji[m * 6 + r] * Ji[m * 6 + c];
        hij += Ji[m * 6 + r] * Jj[m * 6 + c];
        hjj += Jj[m * 6 + r] * Jj[m * 6 + c];
      }
      o[r * 6 + c] = hii; o[36 + r * 6 + c] = hij; o[72 + r * 6 + c] = hjj;
    }
  }
}

__global__ __launch_bounds__(64) void k_pg_assemble(BaDev d, PgDev g, BigDev b)
{
  const int q = blockIdx.x, t = threadIdx.x;
  const int pa = g.blk_pa[q], pb = g.blk_pb[q];
  if (t < 36) {
    const int r = t / 6, c = t - r * 6;
    double s = 0.0;
    for (int k = g.blk_ptr[q]; k < g.blk_ptr[q + 1]; ++k) {
      const int it = g.blk_item[k], e = it >> 2, kind = it & 3;
      const double* o = g.eblk + (size_t)PG_EBLK * e;
      s += kind == 0 ? o[r * 6 + c] : kind == 1 ? o[72 + r * 6 + c] : kind == 2 ? o[36 + r * 6 + c] : o[36 + c * 6 + r];
    }
    b.S[(size_t)(6 * pa + r) * b.ld + 6 * pb + c] = s;
    if (pa != pb) b.S[(size_t)(6 * pb + c) * b.ld + 6 * pa + r] = s;   // off-diagonal: mirror into the lower triangle
  } else if (q < g.nP && t < 42) {
    // right-hand side of this pose (q == pa for the diagonal blocks)
    const int r = t - 36;
    double s = 0.0;
    for (int k = g.g_ptr[pa]; k < g.g_ptr[pa + 1]; ++k) {
      const int it = g.g_item[k];
      s += g.eblk[(size_t)PG_EBLK * (it >> 1) + 108 + 6 * (it & 1) + r];
    }
    b.S[(size_t)b.n_pad * b.ld + 6 * pa + r] = s;
    d.iter_comm[(size_t)d.nP * UPPER6 + 6 * pa + r] = s;     // b, read by k_pose_update_big (computeScale)
  }
  if (q == 0)                                             // padded diagonal = 1 (the factorisation runs over n_pad)
    for (int i = b.n + t; i < b.n_pad; i += 64) b.S[(size_t)i * b.ld + i] = 1.0;
  if (q < g.nP) {
    __shared__ double sd[6];
    __syncthreads();
    if (t < 36 && (t / 6) == (t % 6)) sd[t / 6] = fabs(b.S[(size_t)(6 * pa + t / 6) * b.ld + 6 * pa + t / 6]);
    __syncthreads();
    if (t == 0) { double m = 0.0; for (int k = 0; k < 6; ++k) m = fmax(m, sd[k]); g.maxd[pa] = m; }
  }
}

// the same sums into the BAND layout of ba_band.inc (block (pa, pb), pb - pa <= w, at Sb[pa][pb - pa]; rhs behind it): a pose graph
// whose free keyframes couple only to neighbours a few positions away -- the reference's: one edge per consecutive pair, loop edges
// that end at FIXED keyframes (loopclosing.cpp:484-489) -- is block-tridiagonal, and the block cyclic reduction of ba_bcr.inc solves
// it in 2 log2(nP / 3) short launches instead of a chain of nP / 10 tile steps.  (Sb is zeroed before: blocks without an edge.)
__global__ __launch_bounds__(64) void k_pg_assemble_band(BaDev d, PgDev g, BandDev bd)
{
  const int q = blockIdx.x, t = threadIdx.x;
  const int pa = g.blk_pa[q], pb = g.blk_pb[q];
  __shared__ double sd[6];
  if (t < 36) {
    const int r = t / 6, c = t - r * 6;
    double s = 0.0;
    for (int k = g.blk_ptr[q]; k < g.blk_ptr[q + 1]; ++k) {
      const int it = g.blk_item[k], e = it >> 2, kind = it & 3;
      const double* o = g.eblk + (size_t)PG_EBLK * e;
      s += kind == 0 ? o[r * 6 + c] : kind == 1 ? o[72 + r * 6 + c] : kind == 2 ? o[36 + r * 6 + c] : o[36 + c * 6 + r];
    }
    bd.Sb[((size_t)pa * (bd.w + 1) + (pb - pa)) * 36 + r * 6 + c] = s;
    if (q < g.nP && r == c) sd[r] = fabs(s);
  } else if (q < g.nP && t < 42) {
    const int r = t - 36;
    double s = 0.0;
    for (int k = g.g_ptr[pa]; k < g.g_ptr[pa + 1]; ++k) {
      const int it = g.g_item[k];
      s += g.eblk[(size_t)PG_EBLK * (it >> 1) + 108 + 6 * (it & 1) + r];
    }
    bd.bsv[(size_t)pa * 6 + r] = s;
    d.iter_comm[(size_t)d.nP * UPPER6 + 6 * pa + r] = s;     // b, read by k_pose_update_big (computeScale)
  }
  if (q == 0 && t == 63) d.scal[SC_SOLVE_OK] = 1.0;
  if (q < g.nP) {
    __syncthreads();
    if (t == 0) { double m = 0.0; for (int k = 0; k < 6; ++k) m = fmax(m, sd[k]); g.maxd[pa] = m; }
  }
}

// chi2 = sum over the edges of e^T e into d.scal[slot]; slot == SC_CHI2_CUR with init_lambda also sets lambda_0
__global__ __launch_bounds__(CH) void k_pg_reduce(BaDev d, PgDev g, int slot, int init_lambda)
{
  __shared__ double sRed[CH];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int e = t; e < g.E; e += CH) {
    const double* er = g.err + 6 * (size_t)e;
    double c = 0.0;
    for (int r = 0; r < 6; ++r) c += er[r] * er[r];
    s += c;
  }
  s = block_sum_256(s, sRed);
  if (t == 0) d.scal[slot] = s;
  if (init_lambda) {
    double m = 0.0;
    for (int p = t; p < g.nP; p += CH) m = fmax(m, g.maxd[p]);
    __syncthreads();
    sRed[t] = m;
    __syncthreads();
    for (int o = CH / 2; o > 0; o >>= 1) { if (t < o) sRed[t] = fmax(sRed[t], sRed[t + o]); __syncthreads(); }
    if (t == 0) { d.scal[SC_MAXDIAG] = sRed[0]; d.scal[SC_LAMBDA] = 1e-5 * sRed[0]; }   // computeLambdaInit, tau = 1e-5
  }
}

// ---- the host side of a pose graph, shared by ssx_pose_graph_opt and ssx_loop_correct (loop_correct.inc) ----
// pg_plan      the block lists of the graph and the offsets of its inputs in the staging blob; a caller with inputs of its own takes
//              them from `in` afterwards, so that everything goes up in ONE copy
// pg_layout    the working buffers behind the inputs (`all`; a caller takes its own behind them)
// pg_stage     the inputs into the pinned staging blob
// pg_wire      device pointers (no stream operation)
// pg_lm_loop   the solver's lists, then OptimizationAlgorithmLevenberg::solve per iteration; returns the buffer the state lies in
struct PgPlan {
  int P = 0, E = 0, nP = 0, nBlk = 0, band_w = 1, n = 0, n_pad = 0;
  bool use_bcr = false;
  std::vector<int> pose_free, blk_pa, blk_pb, blk_ptr, blk_item, g_ptr, g_item;
  std::vector<uint8_t> active;
  BcrPlan bcrp;
  size_t sb_count = 0;
  Layout in, all;
  size_t in_bytes = 0;
  size_t o_pose0, o_meas, o_pf, o_ei, o_ej, o_act, o_bpa, o_bpb, o_bptr, o_bit, o_gptr, o_git, o_bcr_p0, o_bcr_elim;
  size_t o_pose1, o_eblk, o_err, o_maxd, o_iter, o_S, o_x, o_Sb, o_bcr_mem, o_Ld, o_invd, o_Ninv, o_sp, o_xp, o_scal;
};
struct PgRun {
  BaDev d{};
  PgDev g{};
  BigDev bd{};
  BandDev bnd{};
};
struct PgStats {                      // where the per-iteration statistics go (each nullable)
  int cap = 0;
  double* chi2 = nullptr; double* lambda = nullptr; int32_t* trials = nullptr;
};

// host lists: non-zero blocks (diagonal first) with their contributing (edge, kind) in edge order.  pose_fixed [P]; nP >= 1, E >= 1
static void pg_plan(PgPlan& pl, int P, int E, const uint8_t* pose_fixed, const int32_t* edge_i, const int32_t* edge_j)
{
  pl.P = P; pl.E = E;
  pl.pose_free.assign(P, -1);
  int nP = 0;
  for (int i = 0; i < P; ++i) if (!pose_fixed[i]) pl.pose_free[i] = nP++;
  pl.nP = nP;
  const std::vector<int>& pose_free = pl.pose_free;
  std::vector<uint8_t>& active = pl.active;
  std::vector<int>& blk_pa = pl.blk_pa; std::vector<int>& blk_pb = pl.blk_pb;
  active.assign(E, 0);
  for (int p = 0; p < nP; ++p) { blk_pa.push_back(p); blk_pb.push_back(p); }
  std::vector<std::vector<int>> items(nP), gitems(nP);
  // (a keyframe has at most a handful of edges, but a linear search over all off-diagonal blocks would be
  //  quadratic: index them per smaller pose instead)
  std::vector<std::vector<std::pair<int, int>>> off_of(nP);   // pa -> (pb, block id)
  for (int k = 0; k < E; ++k) {
    const int a = pose_free[edge_i[k]], c = pose_free[edge_j[k]];
    active[k] = (a >= 0 || c >= 0);
    if (a >= 0) { items[a].push_back(k * 4 + 0); gitems[a].push_back(k * 2 + 0); }
    if (c >= 0) { items[c].push_back(k * 4 + 1); gitems[c].push_back(k * 2 + 1); }
    if (a >= 0 && c >= 0 && a != c) {
      const int pa = std::min(a, c), pb = std::max(a, c);
      int id = -1;
      for (auto& pr : off_of[pa]) if (pr.first == pb) { id = pr.second; break; }
      if (id < 0) {
        id = (int)blk_pa.size();
        blk_pa.push_back(pa); blk_pb.push_back(pb);
        off_of[pa].push_back({pb, id});
        items.emplace_back();
      }
      items[id].push_back(k * 4 + (a < c ? 2 : 3));           // block (pa,pb) = Aij when i is the smaller index, else Aij^T
    } else if (a >= 0 && c >= 0 && a == c) {
      // an edge from a keyframe to itself: both Jacobians act on the same block
      items[a].push_back(k * 4 + 2); items[a].push_back(k * 4 + 3);
    }
  }
  const int nBlk = pl.nBlk = (int)blk_pa.size();
  pl.blk_ptr.assign(nBlk + 1, 0); pl.g_ptr.assign(nP + 1, 0);
  for (int q = 0; q < nBlk; ++q) { for (int it : items[q]) pl.blk_item.push_back(it); pl.blk_ptr[q + 1] = (int)pl.blk_item.size(); }
  for (int p = 0; p < nP; ++p) { for (int it : gitems[p]) pl.g_item.push_back(it); pl.g_ptr[p + 1] = (int)pl.g_item.size(); }
  // the band of the free keyframes' couplings: <= BAND_WMAX positions -> block cyclic reduction (SSX_PG_TILES: the tile solver, for A/B)
  int band_w = 1;
  for (int q = nP; q < nBlk; ++q) band_w = std::max(band_w, blk_pb[q] - blk_pa[q]);
  pl.band_w = band_w;
  static const bool pg_tiles_env = getenv("SSX_PG_TILES") != nullptr;
  if (band_w <= BAND_WMAX && !pg_tiles_env) plan_bcr(nP, band_w, pl.bcrp);
  pl.use_bcr = pl.bcrp.on != 0;
  pl.n = 6 * nP; pl.n_pad = ((pl.n + NB - 1) / NB) * NB;
  Layout& in = pl.in;
  pl.o_pose0 = in.take(sizeof(double) * 7 * P); pl.o_meas = in.take(sizeof(double) * 7 * (size_t)E);
  pl.o_pf = in.take(sizeof(int) * P); pl.o_ei = in.take(sizeof(int) * E); pl.o_ej = in.take(sizeof(int) * E);
  pl.o_act = in.take((size_t)E);
  pl.o_bpa = in.take(sizeof(int) * nBlk); pl.o_bpb = in.take(sizeof(int) * nBlk); pl.o_bptr = in.take(sizeof(int) * (nBlk + 1));
  pl.o_bit = in.take(sizeof(int) * (pl.blk_item.size() + 1)); pl.o_gptr = in.take(sizeof(int) * (nP + 1)); pl.o_git = in.take(sizeof(int) * (pl.g_item.size() + 1));
  pl.o_bcr_p0 = in.take(pl.use_bcr ? sizeof(int) * (pl.bcrp.p0.size() + 1) : 0); pl.o_bcr_elim = in.take(pl.use_bcr ? sizeof(int) * (pl.bcrp.elim.size() + 4) : 0);
}

static void pg_layout(PgPlan& pl)
{
  const int P = pl.P, E = pl.E, nP = pl.nP, n = pl.n, n_pad = pl.n_pad;
  const bool use_bcr = pl.use_bcr;
  pl.in_bytes = pl.in.off;
  pl.all = pl.in;
  Layout& all = pl.all;
  pl.o_pose1 = all.take(sizeof(double) * 7 * P);
  pl.o_eblk = all.take(sizeof(double) * PG_EBLK * (size_t)E); pl.o_err = all.take(sizeof(double) * 6 * (size_t)E);
  pl.o_maxd = all.take(sizeof(double) * nP); pl.o_iter = all.take(sizeof(double) * ((size_t)nP * 27 + 8));
  pl.o_S = all.take(use_bcr ? 256 : sizeof(double) * (size_t)(n_pad + NB) * n_pad); pl.o_x = all.take(sizeof(double) * (n_pad + 8));
  pl.sb_count = use_bcr ? band_rhs_doubles(nP, pl.band_w) : 0;
  pl.o_Sb = all.take(sizeof(double) * (pl.sb_count + 1)); pl.o_bcr_mem = all.take(use_bcr ? sizeof(double) * (bcr_mem_doubles(pl.bcrp.N, pl.bcrp.m) + 8) : 256);
  pl.o_Ld = all.take(sizeof(double) * NB * NB); pl.o_invd = all.take(sizeof(double) * (n_pad + 8)); pl.o_Ninv = all.take(sizeof(double) * 4 * 256);
  pl.o_sp = all.take(sizeof(double) * 64); pl.o_xp = all.take(sizeof(double) * (n + 1)); pl.o_scal = all.take(sizeof(double) * SC_N);
}

static void pg_stage(const PgPlan& pl, char* hs, const double* poses, const int32_t* edge_i, const int32_t* edge_j, const double* edge_meas)
{
  const int P = pl.P, E = pl.E, nP = pl.nP, nBlk = pl.nBlk;
  memcpy(hs + pl.o_pose0, poses, sizeof(double) * 7 * P);
  memcpy(hs + pl.o_meas, edge_meas, sizeof(double) * 7 * (size_t)E);
  memcpy(hs + pl.o_pf, pl.pose_free.data(), sizeof(int) * P);
  memcpy(hs + pl.o_ei, edge_i, sizeof(int) * E); memcpy(hs + pl.o_ej, edge_j, sizeof(int) * E);
  memcpy(hs + pl.o_act, pl.active.data(), (size_t)E);
  memcpy(hs + pl.o_bpa, pl.blk_pa.data(), sizeof(int) * nBlk); memcpy(hs + pl.o_bpb, pl.blk_pb.data(), sizeof(int) * nBlk);
  memcpy(hs + pl.o_bptr, pl.blk_ptr.data(), sizeof(int) * (nBlk + 1)); memcpy(hs + pl.o_bit, pl.blk_item.data(), sizeof(int) * pl.blk_item.size());
  memcpy(hs + pl.o_gptr, pl.g_ptr.data(), sizeof(int) * (nP + 1)); memcpy(hs + pl.o_git, pl.g_item.data(), sizeof(int) * pl.g_item.size());
  if (pl.use_bcr) { memcpy(hs + pl.o_bcr_p0, pl.bcrp.p0.data(), sizeof(int) * pl.bcrp.p0.size()); memcpy(hs + pl.o_bcr_elim, pl.bcrp.elim.data(), sizeof(int) * pl.bcrp.elim.size()); }
}

static void pg_wire(const PgPlan& pl, char* base, PgRun& r)
{
  const int P = pl.P, E = pl.E, nP = pl.nP;
  BaDev& d = r.d;
  d.P = P; d.nP = nP;
  d.pose_free = (const int*)(base + pl.o_pf);
  d.pose[0] = (double*)(base + pl.o_pose0); d.pose[1] = (double*)(base + pl.o_pose1);
  d.iter_comm = (double*)(base + pl.o_iter); d.xp = (double*)(base + pl.o_xp); d.scal = (double*)(base + pl.o_scal);
  PgDev& g = r.g;
  g.P = P; g.E = E; g.nP = nP; g.nBlk = pl.nBlk;
  g.ei = (const int*)(base + pl.o_ei); g.ej = (const int*)(base + pl.o_ej); g.meas = (const double*)(base + pl.o_meas);
  g.active = (const uint8_t*)(base + pl.o_act);
  g.eblk = (double*)(base + pl.o_eblk); g.err = (double*)(base + pl.o_err); g.maxd = (double*)(base + pl.o_maxd);
  g.blk_pa = (const int*)(base + pl.o_bpa); g.blk_pb = (const int*)(base + pl.o_bpb); g.blk_ptr = (const int*)(base + pl.o_bptr);
  g.blk_item = (const int*)(base + pl.o_bit); g.g_ptr = (const int*)(base + pl.o_gptr); g.g_item = (const int*)(base + pl.o_git);
  BigDev& bd = r.bd;
  bd.n = pl.n; bd.n_pad = pl.n_pad; bd.ld = pl.n_pad; bd.T = pl.n_pad / NB;
  bd.S = (double*)(base + pl.o_S); bd.x = (double*)(base + pl.o_x); bd.Ld = (double*)(base + pl.o_Ld);
  bd.invd = (double*)(base + pl.o_invd); bd.Ninv = (double*)(base + pl.o_Ninv); bd.scale_part = (double*)(base + pl.o_sp);
  BandDev& bnd = r.bnd;
  if (pl.use_bcr) {
    bnd.on = 1; bnd.w = pl.band_w; bnd.K = 1; bnd.nP = nP;
    bnd.Sb = (double*)(base + pl.o_Sb); bnd.bsv = bnd.Sb + band_doubles(nP, pl.band_w);
    bnd.bcr.p0 = (const int*)(base + pl.o_bcr_p0); bnd.bcr.elim = (const int4*)(base + pl.o_bcr_elim);
    bcr_carve(bnd.bcr, (double*)(base + pl.o_bcr_mem), pl.bcrp.N, pl.bcrp.m);
  }
}

// the state is r.d.pose[0] with its copy in r.d.pose[1] (the fixed keyframes); *cur_out = the buffer the accepted state lies in
static ssx_status pg_lm_loop(ssx_ctx* ctx, BaWorkspace* ws, const PgPlan& pl, PgRun& run, int iterations, const PgStats& so,
                             ssx_pose_graph_result* res, int* cur_out)
{
  const int P = pl.P, E = pl.E, nBlk = pl.nBlk;
  const bool use_bcr = pl.use_bcr;
  const BcrPlan& bcrp = pl.bcrp;
  const size_t sb_count = pl.sb_count;
  BaDev& d = run.d; PgDev& g = run.g; BigDev& bd = run.bd; BandDev& bnd = run.bnd;
  hipStream_t s = ctx->stream;
  Comm cm;                                                    // single GPU: the graph is tiny next to a BA
  std::vector<int> tl_row_cnt, tl_pair_cnt;
  std::vector<uint8_t> tl_next_diag;
  ssx_status st = SSX_OK;
  if (!use_bcr) {
    st = build_tile_lists(ctx, ws, pl.blk_pa, pl.blk_pb, cm, bd, tl_row_cnt, tl_pair_cnt, tl_next_diag);
    if (st != SSX_OK) return st;
  }
  double* hscal = ws->scal.as<double>();
  const int egrid = (E + 63) / 64;
  auto trial = [&](double lambda, int dev_lambda, int cur) -> ssx_status {
    if (use_bcr) {
      SSX_HIP_TRY(ctx, hipMemsetAsync(bnd.Sb, 0, sizeof(double) * sb_count, s));
      hipLaunchKernelGGL(k_pg_assemble_band, dim3(nBlk), dim3(64), 0, s, d, g, bnd);
      hipLaunchKernelGGL(k_bcr_build, dim3(bnd.bcr.N), dim3(256), 0, s, d, bnd, bnd.bcr, lambda, dev_lambda);
      const bool m24 = bnd.bcr.m == 24;
      const std::vector<int>& lv = bcrp.lvl;
      const std::vector<int>& lm = bcrp.lvM;
      for (size_t q = 0; q < lm.size(); ++q) {
        const int cnt = lv[q + 1] - lv[q], sh = (int)q;
        if (m24) hipLaunchKernelGGL(k_bcr_fwd<24>, dim3(cnt, BCR_S), dim3(BCR_T), 0, s, d, bnd.bcr, sh, lm[q], 0);
        else hipLaunchKernelGGL(k_bcr_fwd<36>, dim3(cnt, BCR_S), dim3(BCR_T), 0, s, d, bnd.bcr, sh, lm[q], 0);
      }
      for (size_t q = lm.size(); q-- > 0;) {
        const int cnt = lv[q + 1] - lv[q], sh = (int)q;
        if (m24) hipLaunchKernelGGL(k_bcr_bwd<24>, dim3(cnt), dim3(256), 0, s, d, bnd.bcr, bd, sh, lm[q], 0);
        else hipLaunchKernelGGL(k_bcr_bwd<36>, dim3(cnt), dim3(256), 0, s, d, bnd.bcr, bd, sh, lm[q], 0);
      }
    } else {
    SSX_HIP_TRY(ctx, hipMemsetAsync(bd.S, 0, sizeof(double) * (size_t)(bd.n_pad + 1) * bd.ld, s));
    hipLaunchKernelGGL(k_pg_assemble, dim3(nBlk), dim3(64), 0, s, d, g, bd);
    hipLaunchKernelGGL(k_add_lambda, dim3((bd.n + 255) / 256), dim3(256), 0, s, d, bd, lambda, dev_lambda);
    for (int kb = 0; kb < bd.T; ++kb) {
      if (kb == 0 || !tl_next_diag[kb - 1]) hipLaunchKernelGGL(k_potrf64, dim3(1), dim3(CH), 0, s, d, bd, kb);
      hipLaunchKernelGGL(k_trsm64, dim3(tl_row_cnt[kb]), dim3(CH), 0, s, bd, kb);
      if (tl_pair_cnt[kb] > 0) hipLaunchKernelGGL(k_syrk64, dim3(tl_pair_cnt[kb]), dim3(CH), 0, s, d, bd, kb);
    }
    hipLaunchKernelGGL(k_backsolve, dim3(1), dim3(1024), 0, s, bd);
    }
    const int nparts = std::min(32, (P + CH - 1) / CH);
    hipLaunchKernelGGL(k_pose_update_big, dim3(nparts), dim3(CH), 0, s, d, bd, cur, lambda, dev_lambda);
    hipLaunchKernelGGL(k_scale_finish, dim3(1), dim3(64), 0, s, d, bd, nparts);
    hipLaunchKernelGGL(k_pg_linearize, dim3(egrid), dim3(64), 0, s, d, g, cur ^ 1, 0);
    hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(CH), 0, s, d, g, (int)SC_TEMP_CHI, 0);
    SSX_HIP_TRY(ctx, hipGetLastError());
    SSX_HIP_TRY(ctx, hipMemcpyAsync(hscal, d.scal, sizeof(double) * SC_N, hipMemcpyDeviceToHost, s));
    SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
    return SSX_OK;
  };
  // ---- OptimizationAlgorithmLevenberg::solve per iteration (optimization_algorithm_levenberg.cpp:58-150) ----
  int cur = 0;
  double lambda = -1.0, ni = 2.0;
  for (int it = 0; it < iterations; ++it) {
    hipLaunchKernelGGL(k_pg_linearize, dim3(egrid), dim3(64), 0, s, d, g, cur, 1);
    hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(CH), 0, s, d, g, (int)SC_CHI2_CUR, 0);
    double currentChi = 0.0, tempChi = 0.0, rho = 0.0;
    int qmax = 0;
    bool lambda_bad = false;
    do {
      const int dev_lambda = (it == 0 && qmax == 0) ? 1 : 0;
      if (dev_lambda) {
        // lambda_0 needs max |diag H|: assemble once into S and reduce (the trial assembles again after its memset)
        if (use_bcr) {
          hipLaunchKernelGGL(k_pg_assemble_band, dim3(nBlk), dim3(64), 0, s, d, g, bnd);
        } else {
        SSX_HIP_TRY(ctx, hipMemsetAsync(bd.S, 0, sizeof(double) * (size_t)(bd.n_pad + 1) * bd.ld, s));
        hipLaunchKernelGGL(k_pg_assemble, dim3(nBlk), dim3(64), 0, s, d, g, bd);
        }
        hipLaunchKernelGGL(k_pg_reduce, dim3(1), dim3(CH), 0, s, d, g, (int)SC_CHI2_CUR, 1);
      }
      st = trial(lambda, dev_lambda, cur);
      if (st != SSX_OK) return st;
      if (dev_lambda) lambda = hscal[SC_LAMBDA];
      if (qmax == 0) { currentChi = hscal[SC_CHI2_CUR]; if (it == 0) res->chi2_initial = currentChi; }
      tempChi = hscal[SC_TEMP_CHI];
      if (hscal[SC_SOLVE_OK] == 0.0) tempChi = std::numeric_limits<double>::max();
      rho = currentChi - tempChi;
      double scale = hscal[SC_SCALE_P];
      scale += 1e-3;
      rho /= scale;
      if (rho > 0 && std::isfinite(tempChi)) {
        double alpha = 1. - std::pow((2 * rho - 1), 3);
        alpha = std::min(alpha, 2. / 3.);
        lambda *= std::max(1. / 3., alpha);
        ni = 2;
        currentChi = tempChi;
        cur ^= 1;                                            // accept: the trial buffer becomes the state
      } else {
        lambda *= ni;
        ni *= 2;
        if (!std::isfinite(lambda)) { lambda_bad = true; break; }
      }
      qmax++;
    } while (rho < 0 && qmax < 10);
    res->n_iters = it + 1;
    if (res->stats_n < so.cap) {
      const int k = res->stats_n;
      if (so.chi2) so.chi2[k] = hscal[SC_TEMP_CHI];   // chi2 of the last evaluation, as g2o reports it
      if (so.lambda) so.lambda[k] = lambda;
      if (so.trials) so.trials[k] = qmax;
      res->stats_n = k + 1;
    }
    res->chi2_final = currentChi;
    if (qmax == 10 || rho == 0 || lambda_bad) break;
  }
  *cur_out = cur;
  return SSX_OK;
}

}  // namespace

extern "C" {

ssx_status ssx_pose_graph_opt(ssx_ctx* ctx, const ssx_pose_graph_problem* prob, int32_t iterations, ssx_pose_graph_result* res)
{
  if (!ctx || !prob || !res || prob->n_poses < 1 || prob->n_edges < 0 || !prob->poses || !prob->pose_fixed ||
      (prob->n_edges > 0 && (!prob->edge_i || !prob->edge_j || !prob->edge_meas)))
    return SSX_ERR_INVALID_ARG;
  const int P = prob->n_poses, E = prob->n_edges;
  int nP = 0;
  for (int i = 0; i < P; ++i) if (!prob->pose_fixed[i]) nP++;
  res->n_iters = 0; res->chi2_initial = 0.0; res->chi2_final = 0.0; res->stats_n = 0;
  for (int k = 0; k < E; ++k)
    if (prob->edge_i[k] < 0 || prob->edge_i[k] >= P || prob->edge_j[k] < 0 || prob->edge_j[k] >= P) {
      ctx->set_error("ssx_pose_graph_opt: edge %d references a keyframe outside [0, %d)", k, P);
      return SSX_ERR_INVALID_ARG;
    }
  if (nP == 0 || E == 0) return SSX_OK;                        // nothing to optimise (g2o: optimize() returns -1)
  if (nP > 2048) { ctx->set_error("ssx_pose_graph_opt: %d free keyframes exceed the supported 2048", nP); return SSX_ERR_UNSUPPORTED; }
  BaWorkspace* ws = ba_workspace(ctx);
  SSX_HIP_TRY(ctx, hipSetDevice(ctx->device));
  PgPlan pl;
  pg_plan(pl, P, E, prob->pose_fixed, prob->edge_i, prob->edge_j);
  pg_layout(pl);
  SSX_HIP_TRY(ctx, ws->arena.reserve(pl.all.off));
  SSX_HIP_TRY(ctx, ws->stage.reserve(std::max(pl.in_bytes, sizeof(double) * (7 * (size_t)P + 6 * (size_t)E))));
  SSX_HIP_TRY(ctx, ws->scal.reserve(sizeof(double) * SC_N));
  char* hs = ws->stage.as<char>();
  pg_stage(pl, hs, prob->poses, prob->edge_i, prob->edge_j, prob->edge_meas);
  char* base = ws->arena.as<char>();
  hipStream_t s = ctx->stream;
  SSX_HIP_TRY(ctx, hipMemcpyAsync(base, hs, pl.in_bytes, hipMemcpyHostToDevice, s));
  PgRun run;
  pg_wire(pl, base, run);
  SSX_HIP_TRY(ctx, hipMemcpyAsync(run.d.pose[1], run.d.pose[0], sizeof(double) * 7 * P, hipMemcpyDeviceToDevice, s));   // fixed keyframes
  PgStats so;
  so.cap = prob->stats_cap; so.chi2 = prob->stats_chi2; so.lambda = prob->stats_lambda; so.trials = prob->stats_trials;
  int cur = 0;
  const ssx_status st = pg_lm_loop(ctx, ws, pl, run, iterations, so, res, &cur);
  if (st != SSX_OK) return st;
  // results: the accepted state, and the edges' errors of the last evaluation (what g2o leaves in _error)
  SSX_HIP_TRY(ctx, hipMemcpyAsync(hs, run.d.pose[cur], sizeof(double) * 7 * P, hipMemcpyDeviceToHost, s));
  if (prob->edge_err_out) SSX_HIP_TRY(ctx, hipMemcpyAsync(hs + sizeof(double) * 7 * P, run.g.err, sizeof(double) * 6 * (size_t)E, hipMemcpyDeviceToHost, s));
  SSX_HIP_TRY(ctx, hipStreamSynchronize(s));
  memcpy(prob->poses, hs, sizeof(double) * 7 * P);
  if (prob->edge_err_out) memcpy(prob->edge_err_out, hs + sizeof(double) * 7 * P, sizeof(double) * 6 * (size_t)E);
  return SSX_OK;
}

}  // extern "C"
