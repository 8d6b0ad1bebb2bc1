// ssvio_amd/csrc/ba_big.inc -- large-window bundle adjustment (free poses > SSX_BA_SMALL_P), included by ba.hip.
//
// Same mathematics as the small-window path (g2o BlockSolver<6,3> Schur complement + Cholesky,
// thirdparty/g2o/g2o/core/block_solver.hpp:315-447), laid out for hundreds of poses (BASELINE config 4: 500 keyframes,
// 80 000 landmarks, 480 000 edges -- the reference itself has no global BA, SURVEY.md section 5):
//   k_pose_blocks     one workgroup per free pose over a POSE-MAJOR edge list: recomputes residual + pose Jacobian of its
//                     edges and tree-reduces the 6x6 + 6 block (no atomics, deterministic)
//   k_schur_prep      per chunk (landmark-major): (Hll + lambda I)^-1, W D^-1 and W D^-1 bl of every observation (AoS)
//   k_schur_blocks    one wave per NON-ZERO block (pa,pb) of the reduced system walking a host-prepared list of the
//                     (edge, edge) pairs that contribute to it: S_ab = Hpp - sum (W_a D^-1) W_b^T, written to the dense
//                     matrix (both triangles); k_bs builds the right-hand side as an extra row of that matrix
//   k_potrf64 / k_trsm64 / k_syrk64   right-looking blocked Cholesky, 64-column panels; the trailing update is a
//                     64x64x64 tile product on the MATRIX CORES: v_mfma_f64_16x16x4_f64, operands staged in LDS.
//                     The right-hand side row rides along (forward substitution for free).
//   k_backsolve                       blocked backward substitution  L^T x = y, one persistent workgroup
//   k_pose_update_big                 exp(x) T per pose + the pose part of computeScale
// The landmark kernels (k_linearize, k_backsub_residual, reductions) are shared with the small path.

constexpr int NB_TILE = 64 * 64;

struct BigDev {
  int n, n_pad, ld, T;          // unknowns, padded to 64, leading dimension, panels
  int nBlkS;
  const int* pe_ptr;            // nP+1: edges of each free pose (pose-major)
  const int* pe_edge;           // sorted-edge index of each pose-major slot
  const int* sblk_pa;           // nBlkS
  const int* sblk_pb;
  const int* spair_ptr;         // nBlkS+1
  const unsigned long long* spair_ab;   // per pair: leader sorted-edge indices a (high 32 bits) | b (low), grouped by block, landmark order inside
  double* BDa;                  // [E][18]
  double* Wma;                  // [E][18]  W merged over duplicates (leaders)
  double* Cv;                   // [E][6]   W D^-1 bl (leaders, 0 otherwise)
  double* S;                    // (n_pad + 64) x ld ; row n_pad = right-hand side
  double* x;                    // n_pad
  double* Ld;                   // 64 x 64: copy of the current panel's diagonal factor (k_potrf64 -> k_trsm64)
  double* invd;                 // n_pad: 1 / L_ii
  double* Ninv;                 // 4 x 16 x 16: inverses of the current panel's 16x16 diagonal sub-blocks
  // 64x64-tile sparsity of the factor (symbolic elimination on the host, identical on every rank): panel kb only
  // touches the row tiles of tl_rows (the rhs row tile T is always among them) and the tile pairs of tl_pair_*
  const int* tl_row_ptr;        // T+1
  const int* tl_rows;
  const int* tl_pair_ptr;       // T+1
  const int* tl_pair_bi;        // row tile (may be T = rhs)
  const int* tl_pair_bj;        // column tile
  const int* tl_col_ptr;        // T+1: non-zero column tiles j < kb of row tile kb (back-substitution)
  const int* tl_cols;
  // the structurally non-zero lower tiles of S itself (before fill): what the ranks exchange
  int n_init;
  const int* tl_init_bi;
  const int* tl_init_bj;
  double* Spack;                // n_init x 64 x 64 tiles, then the right-hand side row (n_pad)
  double* scale_part;           // per-pose partial of computeScale
};

// ---- the (edge, edge) pair lists of the reduced system's blocks, built ON THE DEVICE --------------------------------
// A landmark with leader observations (free pose, first of its duplicates) in poses p_0 <= p_1 <= ... contributes the
// term W_i D^-1 W_j^T to block (p_i, p_j) for every i <= j.  Round 1 built the lists on the host (two passes over all
// landmarks with a P x P block-id table: ~5 of the ~10 ms of host marshalling of a BASELINE configs[3] solve, plus 13 MB
// of upload).  Now: count per landmark -> exclusive scan -> emit (key = pa * nP + pb, value = (a, b)) -> stable radix sort
// by key (rocPRIM) -> run-length encode = the non-zero blocks and their list lengths.  Same lists as the host version up
// to the (irrelevant) numbering of the blocks: inside a block the pairs stay in landmark order, so every sum keeps its order.
__device__ __forceinline__ bool pair_leader(const int4 er) { return er.y >= 0 && !(er.w & 6); }

__global__ __launch_bounds__(CH) void k_pairs_count(const int4* __restrict__ e_rec, const int4* __restrict__ l_rec, const int4* __restrict__ ch_desc,
                                                    const int* __restrict__ lm_chunk, int nLm, int nP, int* __restrict__ cnt, int* __restrict__ wmax)
{
  const int lc = blockIdx.x * CH + threadIdx.x;
  int c = 0, w = 0;
  if (lc < nLm) {
    const int4 lr = l_rec[lc];
    if (!lr.w) {
      const int e0 = ch_desc[lm_chunk[lc]].x + lr.x;
      int nl = 0, pmin = 0, plast = 0;
      for (int s = 0; s < lr.y; ++s) {
        const int4 er = e_rec[e0 + s];
        if (!pair_leader(er)) continue;
        if (nl == 0) pmin = er.y;
        plast = er.y;
        ++nl;
      }
      c = nl * (nl + 1) / 2;
      // largest cyclic distance between two of its poses (sorted ascending): exact when the span is at most half the
      // ring; otherwise every pair is checked
      const int span = plast - pmin;
      if (2 * span <= nP) w = span;
      else
        for (int i = 0; i < lr.y; ++i) {
          const int4 ei = e_rec[e0 + i];
          if (!pair_leader(ei)) continue;
          for (int j = i + 1; j < lr.y; ++j) {
            const int4 ej = e_rec[e0 + j];
            if (!pair_leader(ej)) continue;
            const int dd = ej.y - ei.y;
            w = max(w, min(dd, nP - dd));
          }
        }
    }
    cnt[lc] = c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) w = max(w, __shfl_xor(w, o));
  if ((threadIdx.x & 63) == 0 && w > 0) atomicMax(wmax, w);
}

__global__ __launch_bounds__(CH) void k_pairs_emit(const int4* __restrict__ e_rec, const int4* __restrict__ l_rec, const int4* __restrict__ ch_desc,
                                                   const int* __restrict__ lm_chunk, int nLm, int nP, const int* __restrict__ off,
                                                   unsigned int* __restrict__ keys, unsigned long long* __restrict__ vals)
{
  const int lc = blockIdx.x * CH + threadIdx.x;
  if (lc >= nLm) return;
  const int4 lr = l_rec[lc];
  if (lr.w) return;
  const int e0 = ch_desc[lm_chunk[lc]].x + lr.x;
  int q = off[lc];
  for (int i = 0; i < lr.y; ++i) {
    const int4 ei = e_rec[e0 + i];
    if (!pair_leader(ei)) continue;
    for (int j = i; j < lr.y; ++j) {
      const int4 ej = e_rec[e0 + j];
      if (!pair_leader(ej)) continue;
      keys[q] = (unsigned int)(ei.y * nP + ej.y);
      vals[q] = ((unsigned long long)(unsigned int)(e0 + i) << 32) | (unsigned int)(e0 + j);
      ++q;
    }
  }
}

// ---- pose blocks -------------------------------------------------------------------------------
template <int JAC>
__global__ __launch_bounds__(CH) void k_pose_blocks(BaDev d, BigDev b, int cur)
{
  __shared__ double sRed[27][CH];
  const int pf = blockIdx.x, t = threadIdx.x;
  if (cur < 0) {                                    // device-driven LM: the state buffer comes from the control block
    if (d.scal[SC_STOP] != 0.0) return;
    if (cur == -2 && d.scal[SC_NEEDLIN] == 0.0) return;   // rejected trial: the kept pose blocks are still valid
    cur = (int)d.scal[SC_CUR];
  }
  // find the pose index with this free index: pose_free is monotone, binary search is overkill for P <= 4096
  int p = -1;
  for (int i = pf; i < d.P; ++i) if (d.pose_free[i] == pf) { p = i; break; }
  double T[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) T[k] = d.pose[cur][p * 7 + k];
  double acc[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = 0.0;
  for (int s = b.pe_ptr[pf] + t; s < b.pe_ptr[pf + 1]; s += CH) {
    const int e = b.pe_edge[s];
    const int lid = d.lm_id[d.e_lmc[e]];
    const double X[3] = {d.point[cur][lid * 3], d.point[cur][lid * 3 + 1], d.point[cur][lid * 3 + 2]};
    const double* ext = d.ext + 7 * d.e_cam[e];
    const double u = d.e_uv[e], v = d.e_uv[d.E + e];
    double er[2], p1[3], pc[3], Ji[12], Jj[6], rho0, w;
    ssx::edge_error(T, X, ext, d.K, u, v, er, p1, pc);
    if (JAC == SSX_JAC_NUMERIC_G2O) ssx::edge_jac_numeric(T, X, ext, d.K, u, v, Ji, Jj);
    else ssx::edge_jac_analytic(T, ext, d.K, p1, pc, Ji, Jj);
    ssx::huber(er[0] * er[0] + er[1] * er[1], d.huber_delta, rho0, w);
    const double r0 = -er[0] * w, r1 = -er[1] * w;
    int q = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int c = a; c < 6; ++c) acc[q++] += Ji[a] * w * Ji[c] + Ji[6 + a] * w * Ji[6 + c];
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] += Ji[a] * r0 + Ji[6 + a] * r1;
  }
#pragma unroll
  for (int k = 0; k < 27; ++k) sRed[k][t] = acc[k];
  __syncthreads();
  for (int o = CH / 2; o > 0; o >>= 1) {
    if (t < o)
      for (int k = 0; k < 27; ++k) sRed[k][t] += sRed[k][t + o];
    __syncthreads();
  }
  if (t < 27) {
    const double v = sRed[t][0];
    if (t < UPPER6) { d.Hpp[pf * UPPER6 + t] = v; d.iter_comm[pf * UPPER6 + t] = v; }
    else { d.bp[pf * 6 + (t - UPPER6)] = v; d.iter_comm[d.nP * UPPER6 + pf * 6 + (t - UPPER6)] = v; }
  }
}

// chi2 / landmark max-diagonal over the chunks (the slab holds 2 values per chunk in the big path)
__global__ __launch_bounds__(CH) void k_reduce_lin_big(BaDev d)
{
  __shared__ double sAcc[CH];
  const int t = threadIdx.x;
  double chi = 0.0, md = 0.0;
  for (int c = t; c < d.nCh; c += CH) {
    chi += d.lin_slab[(size_t)c * 2];
    md = fmax(md, d.lin_slab[(size_t)c * 2 + 1]);
  }
  chi = block_sum_256(chi, sAcc);
  md = block_max_256(md, sAcc);
  if (t == 0) {
    double* tail = d.iter_comm + d.nP * 27;
    tail[0] = chi;
    for (int r = 0; r < d.world; ++r) tail[1 + r] = (r == d.rank) ? md : 0.0;
    d.scal[SC_CHI2_CUR] = chi;
  }
}

// ---- Schur complement --------------------------------------------------------------------------
__global__ __launch_bounds__(CH) void k_schur_prep(BaDev d, BigDev b)
{
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* sW = reinterpret_cast<double*>(smem);   // [18][PW]
  double* sDinv = sW + 18 * PW;                   // [9][PW]
  double* sDb = sDinv + 9 * PW;                   // [3][PW]
  const int c = blockIdx.x, t = threadIdx.x;
  if (d.scal[SC_STOP] != 0.0) return;                                  // device-driven LM, already terminated
  const double lambda = d.scal[SC_LAMBDA];
  const int lm0 = d.ch_lm[c], lm1 = d.ch_lm[c + 1];
  const int e0 = d.lm_ptr[lm0], e1 = d.lm_ptr[lm1];
  const int ne = e1 - e0, nl = lm1 - lm0;
  bool leader = false;
  int l = 0;
  if (t < ne) {
    const int e = e0 + t;
#pragma unroll
    for (int k = 0; k < 18; ++k) sW[k * PW + t] = d.W[(size_t)k * d.E + e];
    const int lc = d.e_lmc[e];
    l = lc - lm0;
    leader = (d.pose_free[d.e_pose[e]] >= 0) && !d.lm_fixed[lc] && !d.e_dup[e];
  }
  if (t < nl) {
    const int lc = lm0 + t;
    double D[6], Di[9];
#pragma unroll
    for (int k = 0; k < 6; ++k) D[k] = d.Hll[(size_t)k * d.nLm + lc];
    D[0] += lambda; D[3] += lambda; D[5] += lambda;
    ssx::inv3_sym(D, Di);
    const double b0 = d.bl[lc], b1 = d.bl[(size_t)d.nLm + lc], b2 = d.bl[(size_t)2 * d.nLm + lc];
#pragma unroll
    for (int k = 0; k < 9; ++k) sDinv[k * PW + t] = Di[k];
#pragma unroll
    for (int r = 0; r < 3; ++r) sDb[r * PW + t] = Di[r * 3] * b0 + Di[r * 3 + 1] * b1 + Di[r * 3 + 2] * b2;
  }
  __syncthreads();
  // every edge's records in registers (zeros for non-leaders: never referenced by a pair list) ...
  double BD[18], WM[18], CVv[6];
#pragma unroll
  for (int k = 0; k < 18; ++k) { BD[k] = 0.0; WM[k] = 0.0; }
#pragma unroll
  for (int a = 0; a < 6; ++a) CVv[a] = 0.0;
  if (t < ne && leader) {
#pragma unroll
    for (int k = 0; k < 18; ++k) WM[k] = sW[k * PW + t];
    for (int j = t + 1; j < ne && d.e_dup[e0 + j]; ++j)
#pragma unroll
      for (int k = 0; k < 18; ++k) WM[k] += sW[k * PW + j];
    double Di[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Di[k] = sDinv[k * PW + l];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int q = 0; q < 3; ++q) BD[a * 3 + q] = WM[a * 3] * Di[q] + WM[a * 3 + 1] * Di[3 + q] + WM[a * 3 + 2] * Di[6 + q];
      CVv[a] = WM[a * 3] * sDb[l] + WM[a * 3 + 1] * sDb[PW + l] + WM[a * 3 + 2] * sDb[2 * PW + l];
    }
  }
  // ... and out through LDS: the chunk's records are contiguous in memory (edge-major, 144 / 48 bytes each), so the
  // workgroup writes them as one linear, coalesced stream instead of 42 stores of 8 bytes at a 144-byte stride per lane
  double* buf = sW;                                                  // 18 x PW doubles >= 255 x 18
  double* const outs[3] = {b.BDa + (size_t)e0 * 18, b.Wma + (size_t)e0 * 18, b.Cv + (size_t)e0 * 6};
#pragma unroll
  for (int which = 0; which < 3; ++which) {
    const int rec = which == 2 ? 6 : 18;
    __syncthreads();                                                 // the buffer is free (sW read / previous stream written)
    if (t < ne) {
      if (which == 0) {
#pragma unroll
        for (int k = 0; k < 18; ++k) buf[t * 18 + k] = BD[k];
      } else if (which == 1) {
#pragma unroll
        for (int k = 0; k < 18; ++k) buf[t * 18 + k] = WM[k];
      } else {
#pragma unroll
        for (int a = 0; a < 6; ++a) buf[t * 6 + a] = CVv[a];
      }
    }
    __syncthreads();
    for (int i = t; i < ne * rec; i += CH) outs[which][i] = buf[i];
  }
}

// ONE WAVE per non-zero block of S: lane = (pair slot 0..15, quarter 0..3).  A lane owns the 3x3 quarter (rows 3 qr ..,
// columns 3 qc ..) of every 16th (edge, edge) pair of the block's list -- 9 + 9 doubles of the two 144-byte records per
// pair, 9 accumulators -- and the 16 partial quarters are summed by a fixed xor tree over the lanes (deterministic).
// [One entry per lane (36 of 64 lanes busy, one pair at a time) read 48 bytes per lane per pair -- 1.7 KB of L1 traffic
//  for 288 distinct bytes -- and was bound by the texture-address unit: 0.56 ms on BASELINE configs[3]; four lanes per
//  block without the pair slots had too few threads in flight: 0.74 ms.]
__device__ __forceinline__ void schur_block_quarter(const BaDev& d, const BigDev& b, int blk, int lane, double (&out)[3][3])
{
  const int quarter = lane & 3, slot = lane >> 2, qr = quarter >> 1, qc = quarter & 1;
  double acc[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = 0.0;
  const int q0 = b.spair_ptr[blk], q1 = b.spair_ptr[blk + 1];
  for (int q = q0 + slot; q < q1; q += 16) {
    const unsigned long long ab = b.spair_ab[q];
    const double* bd = b.BDa + (size_t)(ab >> 32) * 18 + qr * 9;
    const double* wm = b.Wma + (size_t)(ab & 0xffffffffull) * 18 + qc * 9;
    double x[9], y[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { x[k] = bd[k]; y[k] = wm[k]; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[i][j] += x[i * 3] * y[j * 3] + x[i * 3 + 1] * y[j * 3 + 1] + x[i * 3 + 2] * y[j * 3 + 2];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double v = acc[i][j];
#pragma unroll
      for (int o = 4; o < 64; o <<= 1) v += __shfl_xor(v, o);        // lanes with the same quarter: slots 0..15
      acc[i][j] = v;
    }
  const int pa = b.sblk_pa[blk], pb = b.sblk_pb[blk];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double h = 0.0;
      if (pa == pb) {
        const int r = 3 * qr + i, c = 3 * qc + j;
        const int rr = r < c ? r : c, c2 = r < c ? c : r;
        h = d.Hpp[pa * UPPER6 + rr * 6 - (rr * (rr - 1)) / 2 + (c2 - rr)];
      }
      out[i][j] = h - acc[i][j];
    }
}

__global__ __launch_bounds__(CH) void k_schur_blocks(BaDev d, BigDev b)
{
  const int lane = threadIdx.x & 63;
  const int blk = blockIdx.x * 4 + (threadIdx.x >> 6), qr = (lane >> 1) & 1, qc = lane & 1;
  if (blk >= b.nBlkS) return;
  double v[3][3];
  schur_block_quarter(d, b, blk, lane, v);
  if (lane >= 4) return;                                             // the slot-0 lanes hold the sums
  const int pa = b.sblk_pa[blk], pb = b.sblk_pb[blk];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int r = 3 * qr + i, c = 3 * qc + j;
      b.S[(size_t)(6 * pa + r) * b.ld + 6 * pb + c] = v[i][j];
      if (pa != pb) b.S[(size_t)(6 * pb + c) * b.ld + 6 * pa + r] = v[i][j];
    }
}

// right-hand side bs = bp - sum_e Cv[e] (pose-major, fixed tree), stored as row n_pad of S; padded diagonal = 1
__global__ __launch_bounds__(CH) void k_bs(BaDev d, BigDev b)
{
  __shared__ double sRed[6][CH];
  const int pf = blockIdx.x, t = threadIdx.x;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int s = b.pe_ptr[pf] + t; s < b.pe_ptr[pf + 1]; s += CH) {
    const double* cv = b.Cv + (size_t)b.pe_edge[s] * 6;
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[a] += cv[a];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) sRed[a][t] = acc[a];
  __syncthreads();
  for (int o = CH / 2; o > 0; o >>= 1) {
    if (t < o)
      for (int a = 0; a < 6; ++a) sRed[a][t] += sRed[a][t + o];
    __syncthreads();
  }
  if (t < 6) b.S[(size_t)b.n_pad * b.ld + 6 * pf + t] = d.bp[pf * 6 + t] - sRed[t][0];
  if (pf == 0)
    for (int i = b.n + t; i < b.n_pad; i += CH) b.S[(size_t)i * b.ld + i] = 1.0;
}

__global__ void k_add_lambda(BaDev d, BigDev b, double lambda_arg, int use_dev_lambda)
{
  const double lambda = use_dev_lambda ? d.scal[SC_LAMBDA] : lambda_arg;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < b.n) b.S[(size_t)i * b.ld + i] += lambda;
  if (i == 0) d.scal[SC_SOLVE_OK] = 1.0;
}

// ---- exchange buffer: only the non-zero lower tiles of S (+ the rhs row) travel through the all-reduce ----------
// (a block-banded 3000 x 3000 system is ~150 tiles = 5 MB instead of the dense 72 MB)
__global__ __launch_bounds__(CH) void k_pack_tiles(BigDev b, int unpack)
{
  const int q = blockIdx.x, t = threadIdx.x;
  if (q == b.n_init) {                              // the right-hand side row
    double* y = b.S + (size_t)b.n_pad * b.ld;
    double* p = b.Spack + (size_t)b.n_init * NB_TILE;
    for (int i = t; i < b.n_pad; i += CH) { if (unpack) y[i] = p[i]; else p[i] = y[i]; }
    return;
  }
  double* tile = b.S + (size_t)(b.tl_init_bi[q] * 64) * b.ld + b.tl_init_bj[q] * 64;
  double* p = b.Spack + (size_t)q * NB_TILE;
  for (int i = t; i < NB_TILE; i += CH) {
    double* g = tile + (size_t)(i >> 6) * b.ld + (i & 63);
    if (unpack) *g = p[i]; else p[i] = *g;
  }
}

// ---- blocked Cholesky (lower, in place), 64-column panels --------------------------------------
constexpr int NB = 64;

__device__ __forceinline__ double bcast_lane(double v, int lane)   // lane: compile-time or wave-uniform
{
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// 1 / sqrt(d): v_rsq_f64 + two Newton steps (the pivot chain of the factorisation is latency-bound; an IEEE
// sqrt followed by an IEEE divide is ~45 dependent instructions, this is 9)
__device__ __forceinline__ double rsqrt_nr(double d)
{
  double y = __builtin_amdgcn_rsq(d);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double e = fma(-(d * y), y, 1.0);
    y = fma(0.5 * y, e, y);
  }
  return y;
}

// diagonal block: 64x64 Cholesky in LDS, blocked by 16.  Per 16-column sub-panel: (i) 16x16 factorisation by ONE
// wave with the rows in registers (pivot and column broadcast with v_readlane: no barrier inside), (ii) the rows
// below solved against it, one thread per row, (iii) the trailing sub-blocks updated.  Three barriers per
// sub-panel instead of three per column.  Also leaves a copy of the factor (b.Ld) and the reciprocal diagonal
// (b.invd) for k_trsm64 / k_backsolve.
struct PotrfLds {
  double A[NB][NB + 1];
  double sInv[NB];
  double sN[4][16][17];                             // inverses of the four 16x16 diagonal sub-blocks
  int sBad;
};

// factor the 64x64 tile L.A in place (lower triangle), 256 threads; expects L.sBad = 0 and a barrier before the call
__device__ __forceinline__ void potrf64_tile(PotrfLds& L)
{
  double (*A)[NB + 1] = L.A;
  double* sInv = L.sInv;
  double (*sN)[16][17] = L.sN;
  int& sBad = L.sBad;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll 1
  for (int c0 = 0; c0 < NB; c0 += 16) {
    if (wave == 0) {
      const int i = lane & 15;
      double r[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) r[k] = A[c0 + i][c0 + k];
      bool bad = false;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double dj = bcast_lane(r[j], j);
        bad = bad || !(dj > 0.0) || !isfinite(dj);
        const double y = rsqrt_nr(dj);
        const double l = r[j] * y;                  // l_ij for i > j
        r[j] = (i == j) ? dj * y : l;
        if (lane == j) sInv[c0 + j] = y;
#pragma unroll
        for (int k = j + 1; k < 16; ++k) r[k] = fma(-l, bcast_lane(l, k), r[k]);
      }
      if (lane < 16) {
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (k <= i) A[c0 + i][c0 + k] = r[k];
      }
      if (bad && lane == 0) sBad = 1;
    }
    __syncthreads();
    if (sBad) break;                                // uniform
    const int m = NB - c0 - 16;                     // rows / columns behind the sub-panel
    if (wave == 3 && lane < 16) {
      // N = L_bb^-1 (lower triangular), lane = column: forward substitution against the identity.  Runs beside the
      // row solves below (those use threads 0 .. m-1 <= 47); k_trsm64 multiplies by N instead of substituting.
      double mcol[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        double s2 = (i == lane) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) s2 = fma(-A[c0 + i][c0 + k], mcol[k], s2);
        mcol[i] = s2 * sInv[c0 + i];
        sN[c0 >> 4][i][lane] = mcol[i];
      }
    }
    if (t < m) {
      const int row = c0 + 16 + t;
      double x[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) x[k] = A[row][c0 + k];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        double s = x[j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = fma(-x[k], A[c0 + j][c0 + k], s);
        x[j] = s * sInv[c0 + j];
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) A[row][c0 + k] = x[k];
    }
    __syncthreads();
    for (int q = t; q < m * m; q += CH) {
      const int ii = q / m, kk = q - ii * m;
      if (kk <= ii) {
        const int ri = c0 + 16 + ii, rk = c0 + 16 + kk;
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) s = fma(A[ri][c0 + j], A[rk][c0 + j], s);
        A[ri][rk] -= s;
      }
    }
    __syncthreads();
  }
}

// write the factored tile of panel kb back: lower triangle into S, the copy for k_trsm64 (b.Ld), 1 / L_ii and the
// sub-block inverses
__device__ __forceinline__ void potrf64_publish(const PotrfLds& L, BaDev d, BigDev b, int kb)
{
  const int t = threadIdx.x;
  if (L.sBad) { if (t == 0) d.scal[SC_SOLVE_OK] = 0.0; return; }
  double* base = b.S + (size_t)(kb * NB) * b.ld + kb * NB;
  for (int i = t; i < NB * NB; i += CH) {
    const double v = ((i & 63) <= (i >> 6)) ? L.A[i >> 6][i & 63] : 0.0;
    base[(size_t)(i >> 6) * b.ld + (i & 63)] = v;
    b.Ld[i] = v;
  }
  if (t < NB) b.invd[kb * NB + t] = L.sInv[t];
  for (int i = t; i < 4 * 256; i += CH) b.Ninv[i] = L.sN[i >> 8][(i >> 4) & 15][i & 15];
}

__global__ __launch_bounds__(CH) void k_potrf64(BaDev d, BigDev b, int kb)
{
  __shared__ PotrfLds L;
  const int t = threadIdx.x;
  const double* base = b.S + (size_t)(kb * NB) * b.ld + kb * NB;
  for (int i = t; i < NB * NB; i += CH) L.A[i >> 6][i & 63] = base[(size_t)(i >> 6) * b.ld + (i & 63)];
  if (t == 0) L.sBad = 0;
  __syncthreads();
  potrf64_tile(L);
  potrf64_publish(L, d, b, kb);
}

typedef double double4_t __attribute__((ext_vector_type(4)));

// panel below the diagonal block: X <- X * L11^-T for one 64-row tile per workgroup (the last tile holds the
// right-hand side row), blocked by 16 columns on the matrix cores:
//     X_b = (A_b - sum_{c<b} X_c L_bc^T) N_b^T,      N_b = L_bb^-1 from k_potrf64
// Wave w owns rows 16w .. 16w+15 of the tile and never reads another wave's rows, so after the initial load there
// is no workgroup barrier; a finished X_b goes back to the LDS tile (accumulator layout -> operand layout).
// v_mfma_f64_16x16x4_f64 fragment maps: A lane l -> A[i = l&15][k = l>>4], B lane l -> B[k = l>>4][j = l&15],
// D reg r of lane l -> row (l>>4) + 4r, col l&15.  (A per-row substitution with the factor in LDS or in SGPRs is
// bound by the latency of ~2000 dependent operand fetches: 29 us and 40 us per panel; this is 40 MFMAs per wave.)
__global__ __launch_bounds__(CH) void k_trsm64(BigDev b, int kb)
{
  __shared__ double sA[NB][NB + 1];
  __shared__ double sL[NB][NB + 1];
  __shared__ double sN[4][16][17];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int bi = b.tl_rows[b.tl_row_ptr[kb] + blockIdx.x];   // row tile; bi == T is the rhs row tile (one valid row)
  const int row0 = bi * NB;
  const int rows_valid = (bi == b.T) ? 1 : NB;
  for (int i = t; i < NB * NB; i += CH) {
    const int r = i >> 6, k = i & 63;
    sA[r][k] = (r < rows_valid) ? b.S[(size_t)(row0 + r) * b.ld + kb * NB + k] : 0.0;
    sL[r][k] = b.Ld[i];
  }
  for (int i = t; i < 4 * 256; i += CH) sN[i >> 8][(i >> 4) & 15][i & 15] = b.Ninv[i];
  __syncthreads();
  const int li = lane & 15, lq = lane >> 4;
  const int r0 = 16 * wave;
#pragma unroll
  for (int bb = 0; bb < 4; ++bb) {
    double4_t acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = sA[r0 + lq + 4 * r][16 * bb + li];
#pragma unroll
    for (int c = 0; c < bb; ++c)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-sA[r0 + li][16 * c + 4 * kk + lq], sL[16 * bb + li][16 * c + 4 * kk + lq], acc, 0, 0, 0);
    // acc (accumulator layout) -> LDS -> operand layout; only this wave touches these rows
#pragma unroll
    for (int r = 0; r < 4; ++r) sA[r0 + lq + 4 * r][16 * bb + li] = acc[r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    double4_t x = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
      x = __builtin_amdgcn_mfma_f64_16x16x4f64(sA[r0 + li][16 * bb + 4 * kk + lq], sN[bb][li][4 * kk + lq], x, 0, 0, 0);
    __builtin_amdgcn_wave_barrier();                  // every lane has read the block before it is overwritten
#pragma unroll
    for (int r = 0; r < 4; ++r) sA[r0 + lq + 4 * r][16 * bb + li] = x[r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  for (int i = t; i < NB * NB; i += CH) {
    const int r = i >> 6, k = i & 63;
    if (r < rows_valid) b.S[(size_t)(row0 + r) * b.ld + kb * NB + k] = sA[r][k];
  }
}



// trailing update C(bi,bj) -= A(bi,kb) * A(bj,kb)^T for the tile pairs bi >= bj > kb that are structurally non-zero
// in panel kb (and the rhs row tile), one 64x64 tile per workgroup: both 64x64 operand tiles in LDS, 4 waves x 4 column tiles x 16 k-steps of v_mfma_f64_16x16x4_f64.
// fragment maps (cdna_hip_programming.md section 3): A lane l -> A[i = l&15][k = l>>4], B lane l -> B[k = l>>4][j = l&15],
// D reg r of lane l -> row (l>>4) + 4r, col l&15.
// The workgroup that updates the NEXT diagonal tile (kb+1, kb+1) goes on to factor it (the tile has then received
// the updates of every earlier panel): k_potrf64 disappears from the per-panel chain (two dependent launches per
// panel instead of three).
struct SyrkLds { double sA[NB][NB + 1]; double sB[NB][NB + 1]; };
union SyrkPotrfLds { SyrkLds mm; PotrfLds po; };

__global__ __launch_bounds__(CH) void k_syrk64(BaDev d, BigDev b, int kb)
{
  __shared__ SyrkPotrfLds lds;
  double (*sA)[NB + 1] = lds.mm.sA;
  double (*sB)[NB + 1] = lds.mm.sB;
  const int pq = b.tl_pair_ptr[kb] + blockIdx.x;
  const int bj = b.tl_pair_bj[pq];                    // column tile
  const int bi = b.tl_pair_bi[pq];                    // row tile >= bj; == T is the rhs row tile
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int row0 = bi * NB, col0 = bj * NB;
  const int rows_valid = (bi == b.T) ? 1 : NB;        // the rhs tile has a single row
  for (int i = t; i < NB * NB; i += CH) {
    const int r = i / NB, k = i % NB;
    sA[r][k] = (r < rows_valid) ? b.S[(size_t)(row0 + r) * b.ld + kb * NB + k] : 0.0;
    sB[r][k] = b.S[(size_t)(col0 + r) * b.ld + kb * NB + k];
  }
  __syncthreads();
  double4_t acc[4];
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) acc[tj] = double4_t{0.0, 0.0, 0.0, 0.0};
  const int ai = 16 * wave + (lane & 15), kq = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < NB / 4; ++kk) {
    const double a = sA[ai][4 * kk + kq];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
      const double bv = sB[16 * tj + (lane & 15)][4 * kk + kq];
      acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[tj], 0, 0, 0);
    }
  }
  const bool next_diag = (bi == kb + 1 && bj == kb + 1);      // workgroup-uniform
  if (!next_diag) {
#pragma unroll
    for (int tj = 0; tj < 4; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = 16 * wave + (lane >> 4) + 4 * r, lc = 16 * tj + (lane & 15);
        if (lr < rows_valid) b.S[(size_t)(row0 + lr) * b.ld + col0 + lc] -= acc[tj][r];
      }
    return;
  }
  __syncthreads();                                    // every wave is done with sA / sB: the LDS becomes the tile to factor
#pragma unroll
  for (int tj = 0; tj < 4; ++tj)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = 16 * wave + (lane >> 4) + 4 * r, lc = 16 * tj + (lane & 15);
      lds.po.A[lr][lc] = b.S[(size_t)(row0 + lr) * b.ld + col0 + lc] - acc[tj][r];
    }
  if (t == 0) lds.po.sBad = 0;
  __syncthreads();
  potrf64_tile(lds.po);
  potrf64_publish(lds.po, d, b, kb + 1);
}

// ---- backward substitution L^T x = y (y = row n_pad of S after the factorisation) --------------
// ONE persistent 1024-thread workgroup walks the panels from the last to the first (the chain is sequential by
// nature; 2 x 47 dependent launches cost more than the arithmetic): the 64x64 triangle is solved by one wave with
// x in registers (v_readlane broadcast, reciprocal diagonal from k_potrf64), then y[c] -= L[panel rows][c] . x
// for the columns c before the panel, coalesced over c.
__global__ __launch_bounds__(1024) void k_backsolve(BigDev b)
{
  __shared__ double sL[NB][NB + 1];
  __shared__ double sx[NB];
  const int t = threadIdx.x;
  double* y = b.S + (size_t)b.n_pad * b.ld;
  for (int kb = b.T - 1; kb >= 0; --kb) {
    const double* lb = b.S + (size_t)(kb * NB) * b.ld + kb * NB;
    for (int i = t; i < NB * NB; i += 1024) sL[i >> 6][i & 63] = lb[(size_t)(i >> 6) * b.ld + (i & 63)];
    __syncthreads();
    if (t < 64) {
      double xv = y[kb * NB + t];
      const double ivd = b.invd[kb * NB + t];
#pragma unroll
      for (int i = NB - 1; i >= 0; --i) {
        const double xi = bcast_lane(xv * ivd, i);        // x_i = (y_i - sum) / L_ii, final once the rows above are done
        if (t == i) xv = xi;
        else if (t < i) xv = fma(-sL[i][t], xi, xv);
      }
      sx[t] = xv;
      b.x[kb * NB + t] = xv;
    }
    __syncthreads();
    // one CU streams the whole factor: keep many wide loads in flight (column PAIRS as 16-byte loads, 16 rows deep)
    const int ct0 = b.tl_col_ptr[kb], nct = b.tl_col_ptr[kb + 1] - ct0;     // non-zero column tiles of this row tile
    for (int it = t; it < nct * 32; it += 1024) {
      const int cp = b.tl_cols[ct0 + (it >> 5)] * 32 + (it & 31);          // column pair
      const double2* col = reinterpret_cast<const double2*>(b.S + (size_t)(kb * NB) * b.ld) + cp;
      const size_t ld2 = (size_t)b.ld / 2;
      double a0 = 0.0, a1 = 0.0;
#pragma unroll 1
      for (int r0 = 0; r0 < NB; r0 += 16) {
        double2 v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = col[(size_t)(r0 + r) * ld2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { a0 = fma(v[r].x, sx[r0 + r], a0); a1 = fma(v[r].y, sx[r0 + r], a1); }
      }
      double2* yp = reinterpret_cast<double2*>(y) + cp;
      double2 yy = *yp;
      yy.x -= a0; yy.y -= a1;
      *yp = yy;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(CH) void k_pose_update_big(BaDev d, BigDev b, int cur, double lambda_arg, int use_dev_lambda)
{
  __shared__ double sRed[CH];
  if (cur < 0) {                                    // device-driven LM
    if (d.scal[SC_STOP] != 0.0) return;
    cur = (int)d.scal[SC_CUR];
  }
  const double lambda = use_dev_lambda ? d.scal[SC_LAMBDA] : lambda_arg;
  const bool ok = d.scal[SC_SOLVE_OK] != 0.0;
  const double* bp_g = d.iter_comm + d.nP * UPPER6;
  double part = 0.0;
  for (int p = blockIdx.x * CH + threadIdx.x; p < d.P; p += gridDim.x * CH) {
    const int pf = d.pose_free[p];
    double T[7], out[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) T[k] = d.pose[cur][p * 7 + k];
    if (pf >= 0) {
      double dx[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        dx[k] = ok ? b.x[pf * 6 + k] : 0.0;
        d.xp[pf * 6 + k] = dx[k];
        part += dx[k] * (lambda * dx[k] + bp_g[pf * 6 + k]);
      }
      ssx::pose_oplus(T, dx, out);
    } else {
#pragma unroll
      for (int k = 0; k < 7; ++k) out[k] = T[k];
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) d.pose[cur ^ 1][p * 7 + k] = out[k];
  }
  part = block_sum_256(part, sRed);
  if (threadIdx.x == 0) b.scale_part[blockIdx.x] = part;
}

__global__ void k_scale_finish(BaDev d, BigDev b, int nparts)
{
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < nparts; ++i) s += b.scale_part[i];
    d.scal[SC_SCALE_P] = s;
  }
}

// ---- small windows with n = 6 nP <= 64 unknowns (<= 10 free keyframes, the reference's active window is 7): the
// reduced system is ONE 64x64 tile.  Same 16-blocked in-LDS Cholesky as k_potrf64 with the right-hand side riding
// along as row 64 (forward substitution for free), backward substitution by one wave with v_readlane, then the
// pose update and the pose part of computeScale -- the role of k_solve (which stays for 11..16 keyframes) at half
// its latency (the 6-column LDL^T steps of k_solve cost two barriers per keyframe on 256 threads).
// k_solve_tiles: (S + lambda I) x = bs for a small window, the role of LinearSolverCSparse::solve
// (thirdparty/g2o/g2o/solvers/csparse/linear_solver_csparse.h:106-142: false when not positive definite), then the pose
// update T <- exp(x) T into the trial buffer (SparseOptimizer::update, sparse_optimizer.cpp:433-446) and the pose part of
// computeScale (optimization_algorithm_levenberg.cpp:168-175).
//
// Cholesky on TS x TS REGISTER TILES, n <= 16 TS, padded with an identity block: TS = 4 (k_solve64, <= 10 free keyframes:
// 30 us per solve), TS = 5 (k_solve80, 11 .. 13 -- the reference's window is 12: 46 us), TS = 6 (k_solve, 14 .. 16: 70 us;
// 288 live doubles per thread, the tiles shuttle through AGPRs).  The blocked LDL^T with 6-column steps they replace took
// 57 .. 85 us for 12 .. 16 keyframes.  Thread (ty, tx) of the 16 x 16 grid owns tile (ty, tx) of the lower triangle, the threads of tile row 15
// also one row of the right-hand side (forward substitution for free).  Step k: the owner factors the diagonal tile (the
// only serial part: TS dependent rsqrt), the tiles below it solve against it and publish the panel in LDS, every
// trailing tile takes L_ik L_jk^T from two LDS tile reads.  Two barriers per step, 16 steps; L is then spilled to LDS
// (packed lower triangle) and one wave back-substitutes.
// (Before: n <= 64 kept the matrix in LDS, 16-column panels, one wave factoring the 16x16 diagonal block with v_readlane
// pivots, one thread per row below it -- 52 000 cycles of factorisation, now 43 000, of which the 64 dependent pivots are
// ~13 000.)
template <int TS>
__device__ __forceinline__ void k_solve_tiles_body(const BaDev& d, const int bx)
{
  constexpr int NT = 16 * TS, T2 = TS * TS;
  __shared__ __attribute__((aligned(16))) double sDg[2][T2];          // L_kk row-major; the diagonal entries hold 1 / l_cc
  __shared__ __attribute__((aligned(16))) double sPn[2][17][T2];      // panel tiles of the step (16 tile rows + the rhs row)
  __shared__ double sLt[NT * (NT + 1) / 2];                           // L, packed lower triangle: row i starts at i (i + 1) / 2
  __shared__ double sInv[NT];
  __shared__ double sX[NT];
  __shared__ int sBad;
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int n = 6 * d.nP;
  const double* S = d.trial_comm;
  const double* bs = d.trial_comm + (size_t)n * n;
  // the loads do not depend on the LM state: issued before it is looked at
  const bool lower = tx <= ty;
  double T[TS][TS], R[TS];
#pragma unroll
  for (int r = 0; r < TS; ++r)
#pragma unroll
    for (int c = 0; c < TS; ++c) {
      const int i = TS * ty + r, j = TS * tx + c;
      T[r][c] = (lower && i < n && j < n) ? S[(size_t)i * n + j] : 0.0;
    }
#pragma unroll
  for (int c = 0; c < TS; ++c) R[c] = (ty == 15 && TS * tx + c < n) ? bs[TS * tx + c] : 0.0;
  const double bp0 = (t < n) ? d.iter_comm[d.nP * UPPER6 + t] : 0.0;   // the (all-reduced) pose part of b, for the scale at the end
  const double bp1 = (NT > 64 && t < 64 && t + 64 < n) ? d.iter_comm[d.nP * UPPER6 + t + 64] : 0.0;
  if (d.scal[SC_STOP] != 0.0) return;              // device-driven LM, already terminated
  const int cur = (int)d.scal[SC_CUR];
  const double lambda = d.scal[SC_LAMBDA];
  // the poses this workgroup updates at the end: on their way during the factorisation
  const double* src = d.pose[cur];
  double* dst = d.pose[cur ^ 1];
  double Tp[7] = {0, 0, 0, 1, 0, 0, 0};
  int pf = -1;
  if (t < d.P) {
    pf = d.pose_free[t];
#pragma unroll
    for (int k = 0; k < 7; ++k) Tp[k] = src[t * 7 + k];
  }
  if (tx == ty) {
#pragma unroll
    for (int r = 0; r < TS; ++r) {
      const int i = TS * ty + r;
      if (i < n) T[r][r] += lambda; else T[r][r] = 1.0;      // padding: identity
    }
  }
  if (t == 0) sBad = 0;
  __syncthreads();
  double inv[TS];                                             // 1 / l_cc of the diagonal tile (its owner)
#pragma unroll
  for (int r = 0; r < TS; ++r) inv[r] = 1.0;
  const int nsteps = (n + TS - 1) / TS;                      // the tiles behind them are the identity padding: nothing to factor
#pragma unroll 1
  for (int k = 0; k < nsteps; ++k) {
    const int pb = k & 1;
    if (ty == k && tx == k) {
      bool bad = false;
#pragma unroll
      for (int c = 0; c < TS; ++c) {
        double dc = T[c][c];
#pragma unroll
        for (int m = 0; m < c; ++m) dc = fma(-T[c][m], T[c][m], dc);
        bad = bad || !(dc > 0.0) || !isfinite(dc);
        const double y = rsqrt_nr(dc);
        inv[c] = y;
        T[c][c] = dc * y;
#pragma unroll
        for (int r = c + 1; r < TS; ++r) {
          double v = T[r][c];
#pragma unroll
          for (int m = 0; m < c; ++m) v = fma(-T[r][m], T[c][m], v);
          T[r][c] = v * y;
        }
      }
#pragma unroll
      for (int r = 0; r < TS; ++r)
#pragma unroll
        for (int c = 0; c < TS; ++c) sDg[pb][r * TS + c] = (r == c) ? inv[r] : (c < r ? T[r][c] : 0.0);
      if (bad) sBad = 1;
    }
    __syncthreads();
    // (a non-positive pivot is only recorded: the NaNs it breeds are harmless and the solve is declared failed at the end;
    // testing the flag here would put one more LDS round trip into every step)
    if (tx == k && ty >= k) {
      double Lk[T2];
#pragma unroll
      for (int q = 0; q < T2; ++q) Lk[q] = sDg[pb][q];
      if (ty > k) {
        // X L_kk^T = A  ->  x_c = (a_c - sum_{m<c} x_m l_cm) / l_cc, row by row
#pragma unroll
        for (int r = 0; r < TS; ++r) {
#pragma unroll
          for (int c = 0; c < TS; ++c) {
            double v = T[r][c];
#pragma unroll
            for (int m = 0; m < c; ++m) v = fma(-T[r][m], Lk[c * TS + m], v);
            T[r][c] = v * Lk[c * TS + c];
          }
        }
#pragma unroll
        for (int r = 0; r < TS; ++r)
#pragma unroll
          for (int c = 0; c < TS; ++c) sPn[pb][ty][r * TS + c] = T[r][c];
      }
      if (ty == 15) {                                          // the rhs row (also when k == 15: its last entries)
#pragma unroll
        for (int c = 0; c < TS; ++c) {
          double v = R[c];
#pragma unroll
          for (int m = 0; m < c; ++m) v = fma(-R[m], Lk[c * TS + m], v);
          R[c] = v * Lk[c * TS + c];
        }
#pragma unroll
        for (int c = 0; c < TS; ++c) sPn[pb][16][c] = R[c];
      }
    }
    __syncthreads();
    if (tx > k && lower) {
      double A[T2], B[T2];
#pragma unroll
      for (int q = 0; q < T2; ++q) { A[q] = sPn[pb][ty][q]; B[q] = sPn[pb][tx][q]; }
#pragma unroll
      for (int r = 0; r < TS; ++r)
#pragma unroll
        for (int c = 0; c < TS; ++c) {
          double v = T[r][c];
#pragma unroll
          for (int m = 0; m < TS; ++m) v = fma(-A[r * TS + m], B[c * TS + m], v);
          T[r][c] = v;
        }
      if (ty == 15) {
#pragma unroll
        for (int c = 0; c < TS; ++c) {
          double v = R[c];
#pragma unroll
          for (int m = 0; m < TS; ++m) v = fma(-sPn[pb][16][m], B[c * TS + m], v);
          R[c] = v;
        }
      }
    }
  }
  const int ok = sBad ? 0 : 1;
  // L, 1 / l_ii and y = L^-1 b to LDS for the back substitution by one wave
  if (lower) {
#pragma unroll
    for (int r = 0; r < TS; ++r)
#pragma unroll
      for (int c = 0; c < TS; ++c) {
        const int i = TS * ty + r, j = TS * tx + c;
        if (j <= i) sLt[i * (i + 1) / 2 + j] = T[r][c];
      }
  }
  if (tx == ty) {
#pragma unroll
    for (int r = 0; r < TS; ++r) sInv[TS * ty + r] = inv[r];
  }
  if (ty == 15) {
#pragma unroll
    for (int c = 0; c < TS; ++c) sX[TS * tx + c] = R[c];
  }
  __syncthreads();
  if (t < 64) {
    // L^T x = y: lane t holds x_t (and x_{t+64}); rows of L are read EIGHT at a time, ahead of the dependent chain (they do
    // not depend on x)
    double x0 = ok ? sX[t] : 0.0, x1 = (ok && NT > 64 && t + 64 < NT) ? sX[t + 64] : 0.0;
    const double iv0 = sInv[t], iv1 = (NT > 64 && t + 64 < NT) ? sInv[t + 64] : 1.0;
    if (ok) {
#pragma unroll 1
      for (int i0 = NT - 1; i0 >= 0; i0 -= 8) {
        double l0[8], l1[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int i = i0 - q, row = i * (i + 1) / 2;
          l0[q] = (t <= i) ? sLt[row + t] : 0.0;
          l1[q] = (NT > 64 && t + 64 <= i) ? sLt[row + t + 64] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int i = i0 - q;                              // wave-uniform
          if (NT > 64 && i >= 64) {
            const double xi = bcast_lane(x1 * iv1, i - 64);
            if (t + 64 == i) x1 = xi;
            else if (t + 64 < i) x1 = fma(-l1[q], xi, x1);
            x0 = fma(-l0[q], xi, x0);
          } else {
            const double xi = bcast_lane(x0 * iv0, i);
            if (t == i) x0 = xi;
            else if (t < i) x0 = fma(-l0[q], xi, x0);
          }
        }
      }
    }
    sX[t] = x0;
    if (t < n) d.xp[t] = x0;
    if (NT > 64 && t + 64 < NT) { sX[t + 64] = x1; if (t + 64 < n) d.xp[t + 64] = x1; }
  }
  __syncthreads();
  for (int p = t; p < d.P; p += CH) {
    double T2p[7], out[7];
    int pf2 = pf;
    if (p == t) {
#pragma unroll
      for (int k = 0; k < 7; ++k) T2p[k] = Tp[k];
    } else {                                           // (more than 256 poses in a small window: never; kept for generality)
      pf2 = d.pose_free[p];
#pragma unroll
      for (int k = 0; k < 7; ++k) T2p[k] = src[p * 7 + k];
    }
    if (pf2 >= 0) {
      double dx[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) dx[k] = sX[pf2 * 6 + k];
      ssx::pose_oplus(T2p, dx, out);
    } else {
#pragma unroll
      for (int k = 0; k < 7; ++k) out[k] = T2p[k];
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) dst[p * 7 + k] = out[k];
  }
  if (t < 64) {
    double s = t < n ? sX[t] * (lambda * sX[t] + bp0) : 0.0;
    if (NT > 64 && t + 64 < n) s += sX[t + 64] * (lambda * sX[t + 64] + bp1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (t == 0) {
      d.scal[SC_SOLVE_OK] = ok ? 1.0 : 0.0;
      d.scal[SC_SCALE_P] = s;
    }
  }
}

// k_solve64 (<= 10 free keyframes, n <= 60), round 5: the matrix in REGISTERS by rows, the scheme of ba_bcr.inc's k_bcr_fwd.  Thread
// (rg, c) of 4 row groups (= waves) x 64 columns owns column c of the rows rg, rg + 4, ..; column 63 carries the right-hand side
// through the elimination (forward substitution for free).  Step k: the wave that owns row k has published it (one LDS row, double
// buffered, ONE barrier per step); everybody reads the pivot, its column's entry and -- broadcast -- the entries of its rows;
// the NEXT pivot row is updated first and goes out to LDS before the other 15 fmas.  60 steps of ~450 cycles against 15 tile steps
// of ~2 900 (diagonal tile by one thread, panel, trailing update: two barriers each); the back-substitution reads row t of L^T
// into lane t's registers once and runs unrolled on readlane.  25 -> 15 us per solve (profiles/r05/solve64.md).
__device__ __forceinline__ void k_solve_rows64_body(const BaDev& d)
{
  constexpr int M = 64, RG = 4, NR = M / RG, RHS = M - 1, OP = M + 1;     // OP: row pitch of O (lane t reads row t: no bank conflicts)
  __shared__ double O[M * OP];                                            // O[k][c] = L[c][k] (c > k), 1 / L[k][k] (c == k), y_k (c == RHS)
  __shared__ double rowbuf[2][M];
  __shared__ double sX[M];
  __shared__ int sBad;
  const int t = threadIdx.x, rg = t >> 6, c = t & 63;
  const int n = 6 * d.nP;                                                 // <= 60
  const double* S = d.trial_comm;
  const double* bs = d.trial_comm + (size_t)n * n;
  // the loads do not depend on the LM state: issued before it is looked at.  Branch-free: a clamped address and a factor.
  double a[NR];
  {
    const bool colS = c < n, colR = c == RHS;
    double v[NR];
#pragma unroll
    for (int nn = 0; nn < NR; ++nn) {
      const int i = rg + RG * nn, ic = i < n ? i : 0;
      const double* ptr = colR ? bs + ic : S + (size_t)ic * n + (colS ? c : 0);
      v[nn] = *ptr;
    }
#pragma unroll
    for (int nn = 0; nn < NR; ++nn) a[nn] = (rg + RG * nn < n && (colS || colR)) ? v[nn] : 0.0;
  }
  const double bp0 = (t < n) ? d.iter_comm[d.nP * UPPER6 + t] : 0.0;   // the (all-reduced) pose part of b, for the scale at the end
  if (d.scal[SC_STOP] != 0.0) return;              // device-driven LM, already terminated
  const int cur = (int)d.scal[SC_CUR];
  const double lambda = d.scal[SC_LAMBDA];
  // the poses this workgroup updates at the end: on their way during the factorisation
  const double* src = d.pose[cur];
  double* dst = d.pose[cur ^ 1];
  double Tp[7] = {0, 0, 0, 1, 0, 0, 0};
  int pf = -1;
  if (t < d.P) {
    pf = d.pose_free[t];
#pragma unroll
    for (int k = 0; k < 7; ++k) Tp[k] = src[t * 7 + k];
  }
#pragma unroll
  for (int nn = 0; nn < NR; ++nn) if (rg + RG * nn == c && c < n) a[nn] += lambda;
  if (t == 0) sBad = 0;
  if (rg == 0) rowbuf[0][c] = a[0];
  // O is written by rows k < n, right of the diagonal; the back-substitution loads whole rows: the rest reads as zeros, not as whatever
  // the LDS held (the values are never consumed, but they would flow through fma / readlane as undefined bits).  The first write to
  // O follows the first barrier of the loop below.
  for (int i = t; i < M * OP; i += RG * M) O[i] = 0.0;
  bool bad = false;
#pragma unroll
  for (int nk = 0; nk < NR; ++nk) {
#pragma unroll
    for (int rk = 0; rk < RG; ++rk) {
      const int k = RG * nk + rk, k1 = k + 1 < M ? k + 1 : k;
      if (k >= n) continue;                                             // (uniform: the rows behind are padding)
      const double* rb = rowbuf[k & 1];
      __syncthreads();
      double piv = rb[k], akc = rb[c], rnx = rb[k1];
      asm volatile("" : "+v"(piv), "+v"(akc), "+v"(rnx));               // one LDS round trip for the three the next pivot row waits for
      double ri[NR];
#pragma unroll
      for (int nn = nk; nn < NR; ++nn) ri[nn] = rb[rg + RG * nn];
      bad = bad || !(piv > 0.0) || !isfinite(piv);                      // (recorded; the NaNs it breeds are harmless, the solve is declared failed at the end)
      double x = __builtin_amdgcn_rcp(piv);                             // akc / piv for the updates: 6 dependent instructions to the next pivot row
      x = fma(fma(-piv, x, 1.0), x, x);
      x = fma(fma(-piv, x, 1.0), x, x);
      const double f = akc * x;
      const double pub = fma(-rnx, f, a[k1 / RG]);
      if (k + 1 < M && rg == k1 % RG) rowbuf[k1 & 1][c] = pub;
      const double s = rsqrt_nr(piv);                                   // (for the stored factor only: off the critical path)
      if (rg == rk && c >= k) O[k * OP + c] = c == k ? s : akc * s;
      // every register of the rows >= 4 nk takes the update, needed or not (finished rows and the lower triangle hold values nobody
      // reads); the empty asm keeps the compiler from deferring a row's updates to the step that publishes it
#pragma unroll
      for (int nn = nk; nn < NR; ++nn) { a[nn] = fma(-ri[nn], f, a[nn]); asm volatile("" : "+v"(a[nn])); }
    }
  }
  if (bad) sBad = 1;
  __syncthreads();
  const int ok = sBad ? 0 : 1;
  if (t < 64) {
    // L^T x = y, last unknown first: lane t holds row t of O (its entries right of the diagonal: L[.][t]) and its running right-hand side
    double lrow[M];
#pragma unroll
    for (int kk = 0; kk < M; ++kk) lrow[kk] = O[t * OP + kk];
    double v = lrow[RHS], xi = 0.0;
#pragma unroll
    for (int kk = M - 2; kk >= 0; --kk) {
      if (kk >= n) continue;                                            // (uniform)
      const double vk = bcast_lane(v, kk), dk = bcast_lane(lrow[kk], kk);
      const double xk = vk * dk;
      if (t == kk) xi = xk;
      v = fma(-lrow[kk], xk, v);                                        // (lanes >= kk: values nobody reads)
    }
    const double x0 = (ok && t < n) ? xi : 0.0;
    sX[t] = x0;
    if (t < n) d.xp[t] = x0;
  }
  __syncthreads();
  for (int p = t; p < d.P; p += CH) {
    double T2p[7], out[7];
    int pf2 = pf;
    if (p == t) {
#pragma unroll
      for (int k = 0; k < 7; ++k) T2p[k] = Tp[k];
    } else {                                           // (more than 256 poses in a small window: never; kept for generality)
      pf2 = d.pose_free[p];
#pragma unroll
      for (int k = 0; k < 7; ++k) T2p[k] = src[p * 7 + k];
    }
    if (pf2 >= 0) {
      double dx[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) dx[k] = sX[pf2 * 6 + k];
      ssx::pose_oplus(T2p, dx, out);
    } else {
#pragma unroll
      for (int k = 0; k < 7; ++k) out[k] = T2p[k];
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) dst[p * 7 + k] = out[k];
  }
  if (t < 64) {
    double s = t < n ? sX[t] * (lambda * sX[t] + bp0) : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (t == 0) {
      d.scal[SC_SOLVE_OK] = ok ? 1.0 : 0.0;
      d.scal[SC_SCALE_P] = s;
    }
  }
}

__global__ __launch_bounds__(CH) void k_solve64(BaDev d) { k_solve_rows64_body(d); }
__global__ __launch_bounds__(CH) void k_solve80(BaDev d) { k_solve_tiles_body<5>(d, blockIdx.x); }
__global__ __launch_bounds__(CH) void k_solve(BaDev d) { k_solve_tiles_body<6>(d, blockIdx.x); }
// batched: blockIdx.y = window; every window brings its own BaDev (device array)
__global__ __launch_bounds__(CH) void k_solve64_b(const BaDev* __restrict__ dv)
{
  const BaDev& d = dv[blockIdx.y];       // by reference: a private copy of the 500-byte struct ends up in scratch memory
  if ((int)blockIdx.x >= ((6 * d.nP <= 64) ? 1 : 0)) return;
  k_solve_rows64_body(d);
}
__global__ __launch_bounds__(CH) void k_solve_b(const BaDev* __restrict__ dv)
{
  const BaDev& d = dv[blockIdx.y];
  if ((int)blockIdx.x >= ((6 * d.nP > 80) ? 1 : 0)) return;
  k_solve_tiles_body<6>(d, blockIdx.x);
}
__global__ __launch_bounds__(CH) void k_solve80_b(const BaDev* __restrict__ dv)
{
  const BaDev& d = dv[blockIdx.y];
  if ((int)blockIdx.x >= ((6 * d.nP > 64 && 6 * d.nP <= 80) ? 1 : 0)) return;
  k_solve_tiles_body<5>(d, blockIdx.x);
}
