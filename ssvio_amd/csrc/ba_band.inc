// ssvio_amd/csrc/ba_band.inc -- reduced-system solve for trajectory-shaped windows (included by ba.hip after ba_big.inc).
//
// The reduced pose system S x = b of a large window (BlockSolver::solve, thirdparty/g2o/g2o/core/block_solver.hpp:342-447;
// the reference hands it to CSparse with a block-AMD ordering, solvers/csparse/linear_solver_csparse.h:106-142,246-308)
// is, for keyframes along a trajectory, CYCLICALLY BLOCK-BANDED: pose p shares landmarks only with poses within w
// positions (BASELINE configs[3]: 6 consecutive observations per landmark -> w = 5; a loop closure wraps the band
// around).  Dense 64x64 panels chained through ~140 launches (ba_big.inc) spend 2.4 ms per trial on a 4 Mflop job;
// here the band is stored as such and eliminated by a SLIDING WINDOW with 6x6 block pivots:
//
//   * band storage  Sb[p][d] = block (p, (p+d) mod nP), d = 0..w          (0.86 MB for 499 poses instead of 72 MB)
//   * one workgroup keeps the (2w+1)-block window of the partially eliminated matrix in LDS: the w band rows below the
//     pivot, the rows of a FIXED pose set that fill in along the way (the left neighbours of a segment / the wrap-around
//     rows), and the right-hand side as one more row (forward substitution for free).  Per pivot: every thread factors
//     the 6x6 block redundantly in registers (no broadcast), one thread per row solves its 6 panel entries, 3x6 register
//     tiles apply the rank-6 update, the next pose of the band enters the freed slot (its blocks were prefetched into
//     registers at the start of the step): 3 barriers and ~0.5 us per pose.
//   * NESTED DISSECTION ALONG THE TRAJECTORY: the poses are cut into K segments separated by w poses each; the K
//     interiors are eliminated CONCURRENTLY by K workgroups (k_band_seg), each leaving its Schur update on its two
//     separators; the separator system (K w poses, block bandwidth 2w-1, cyclic) is assembled and factored by one
//     workgroup with the same routine (k_band_top), then the interiors back-substitute concurrently (k_band_back).
//     The dependent pivot chain shrinks from nP to nP/K + K w poses; a trial's solve is 4 launches.
// The landmark-sharded multi-GPU solve all-reduces the band (+ rhs) once per trial and every rank runs this solver
// redundantly: it is no longer the Amdahl term (DESIGN.md section 7).
//
// Determinism: fixed elimination order, no atomics; identical bits from run to run and on every rank.

constexpr int BAND_WMAX = 5;       // block bandwidth handled here: one 3x6 register tile per thread needs 2 (2w+1)^2 + 2w+1 <= 256 (level 0)
                                   // and 2 (3w)^2 + 3w <= 512 (top level)
constexpr int BAND_T = 256;        // threads per workgroup
constexpr int BAND_TOP_T = 512;    // the top level: its window is wider (up to 18 blocks), twice the update tiles
constexpr int BAND_G = 8;          // poses per back-substitution prefetch group

struct BandSys {                   // one cyclic block-banded SPD system + right-hand side
  int nP, w;
  const double* Sb;                // [nP][w+1][36]
  const double* bs;                // [6 nP]
};

struct BandJob {                   // what one workgroup eliminates
  int p0, m;                       // interior poses p0 .. p0+m-1 (mod nP), in this order
  int nF;                          // fixed poses p0-nF .. p0-1 (mod nP): their rows stay in the window (eliminated last if elim_fixed)
  int nR;                          // poses p0+m .. p0+m+nR-1 enter the band behind the interior and stay (level 0: the right separator)
  int elim_fixed;                  // top level: complete factorisation
  int sep_zero;                    // level 0: entries between two non-interior poses start at zero (the window then ends as the pure Schur update)
};

// block cyclic reduction of the same band (ba_bcr.inc): device view and host plan
struct BcrDev {
  int on, N, m;
  const int* p0;                 // N + 1: first pose of every super-block
  const int4* elim;              // eliminations in order: (j, left neighbour or -1, right neighbour or -1, 0)
  double* D; double* E; double* DL; double* DR; double* Lf; double* Ul; double* Ur;    // N x m x m each (E: 2 N x m x m, bcr_e_buf)
  double* R; double* RL; double* RR; double* Y; double* X;                              // N x m each
};

// host plan: block boundaries and the elimination schedule (depends on nP and w only)
struct BcrPlan {
  int on = 0, N = 0, m = 0;
  std::vector<int> p0, elim, lvl, lvM;             // elim: 4 ints per elimination (the schedule spelled out; the kernels derive it:
                                                   // bcr_who); lvl: first elimination of every level (+ end); lvM: active blocks per level
};

struct BandDev {
  int on, w, K, nP;                // on = this window uses the band solver; K segments (1 = single level)
  int nPr, wr;                     // reduced (separator) system: K w poses, bandwidth 2w-1
  double* Sb;                      // band + rhs, contiguous: [nP (w+1) 36 | 6 nP]  (what the ranks all-reduce)
  double* bsv;
  const int* seg_p0;               // K: first interior pose of segment k
  const int* seg_m;                // K: interior length
  double* U;                       // K x NU x NU, NU = 12 w + 1: Schur update of segment k on [left separator | right separator | rhs]
  double* Ls0;                     // level-0 factor: per free pose LS0 doubles: [36: L with 1/diag] [NW0 x 6: panel]
  double* Sr;                      // reduced system, same layout as Sb: [nPr (wr+1) 36 | 6 nPr]
  double* Ls1;                     // top-level factor
  double* xr;                      // reduced solution (6 nPr)
  int LS0, LS1;
  BcrDev bcr;                      // bcr.on: the trials are solved by ba_bcr.inc instead of the kernels below
};

__device__ __forceinline__ int band_nw(int w, int nF) { return 6 * (w + 1 + nF) + 1; }

// S[6 qa + r][6 qb + c] of a cyclic band system (0 outside the band)
__device__ __forceinline__ double band_get(const BandSys& sy, int qa, int qb, int r, int c)
{
  int d = qb - qa;
  if (d < 0) d += sy.nP;
  if (d <= sy.w) return sy.Sb[((size_t)qa * (sy.w + 1) + d) * 36 + r * 6 + c];
  d = sy.nP - d;
  if (d <= sy.w) return sy.Sb[((size_t)qb * (sy.w + 1) + d) * 36 + c * 6 + r];
  return 0.0;
}

// window row-block -> pose of the system (or -1), at elimination step e.  Band slot s holds local pose
// j = e + ((s - e) mod (w+1)) for e < m (the pivot's slot holds e itself); fixed slot f holds pose p0 - nF + f.
__device__ __forceinline__ int band_pose_of(const BandSys& sy, const BandJob& jb, int e, int rb, bool* interior)
{
  const int nb = sy.w + 1;
  *interior = false;
  if (rb >= nb) {
    int q = jb.p0 - jb.nF + (rb - nb);
    if (q < 0) q += sy.nP;
    return q;
  }
  if (e >= jb.m) return -1;                                  // the band is empty while the fixed poses are eliminated
  const int pb = e % nb;
  int off = rb - pb;
  if (off < 0) off += nb;
  const int j = e + off;
  if (j >= jb.m + jb.nR) return -1;
  *interior = j < jb.m;
  int q = jb.p0 + j;
  if (q >= sy.nP) q -= sy.nP;
  return q;
}

// value of window entry (row-block ra, r) x (row-block rb2, c) when loaded from the system at step e
__device__ __forceinline__ double band_entry(const BandSys& sy, const BandJob& jb, double lambda, int e, int ra, int r, int rb2, int c)
{
  bool ia, ib;
  const int qa = band_pose_of(sy, jb, e, ra, &ia), qb = band_pose_of(sy, jb, e, rb2, &ib);
  if (qa < 0 || qb < 0) return 0.0;
  if (jb.sep_zero && !ia && !ib) return 0.0;
  double v = band_get(sy, qa, qb, r, c);
  if (ra == rb2 && r == c) v += lambda;
  return v;
}

__device__ __forceinline__ double band_rhs(const BandSys& sy, const BandJob& jb, int e, int ra, int r)
{
  bool ia;
  const int qa = band_pose_of(sy, jb, e, ra, &ia);
  if (qa < 0 || (jb.sep_zero && !ia)) return 0.0;
  return sy.bs[(size_t)qa * 6 + r];
}

// Workgroup barrier that only waits for this wave's LDS traffic: the global loads prefetched for the next pose (and
// the factor stores) stay in flight across it.  __syncthreads() would drain vmcnt as well, i.e. put a full global-memory
// round trip into every step of the pivot chain.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Eliminate the interior (and, top level, the fixed poses) of one job.  smem: Wm [NW][NWP] | Pn [NW][7].
// Ls + e * LS receives, per eliminated pose e: L (36, row-major lower, diagonal replaced by 1 / L_cc) and the panel
// X = rows-below x 6 in window-row order (rows of the pivot block are zero).  Returns 0 when a pivot is not positive.
// The window matrix lives in REGISTERS: thread t owns one 3x6 tile (half-block row rh, block column cb) for the whole
// elimination (threads ntile .. ntile+nblk-1: a 1x6 tile of the rhs row).  Only the 6 columns of the NEXT pivot pass
// through LDS (Cb, double buffered, written by their owners after the update) for the factorisation and the panel solve,
// plus the panel itself (Pn).  [The first version kept the window in LDS: its read-modify-write of 18 entries per thread
// per step ran into 3-way bank conflicts and cost 2400 of the 6100 cycles of a step.]
struct BandTile {
  double W[3][6];
  int rh, cb;            // regular tile: rh >= 0; rhs-row tile: rh == -2; idle thread: rh == -1
};

// Eliminate the interior (and, top level, the fixed poses) of one job.  smem: Cb [2][NW][7] | Pn [NW][7].
// Ls + e * LS receives, per eliminated pose e: L (36, row-major lower, diagonal replaced by 1 / L_cc) and the panel
// X = rows-below x 6 in window-row order (rows of the pivot block are zero).  Returns 0 when a pivot is not positive.
// On return `tl` holds this thread's tile of the remaining window (level 0: the Schur update on the separators).
template <int NT>
__device__ __forceinline__ int band_eliminate(const BandSys sy, const BandJob jb, double lambda, double* Ls, int LS, double* smem, BandTile& tl)
{
  const int t = threadIdx.x;
  const int nb = sy.w + 1, nblk = nb + jb.nF;
  const int RH = 6 * nblk, NW = RH + 1;
  double* Cb = smem;                                                 // [2][NW][7]
  double* Pn = smem + (size_t)2 * NW * 7;                            // [NW][7]
  double* Eb = Pn + (size_t)NW * 7;                                  // [nblk * 36 + 6]: the entering pose's entries, see below
  const int n_elim = jb.m + (jb.elim_fixed ? jb.nF : 0);
  const int ntile = 2 * nblk * nblk;
  tl.rh = -1; tl.cb = 0;
  if (t < ntile) { tl.rh = t / nblk; tl.cb = t - tl.rh * nblk; }
  else if (t < ntile + nblk) { tl.rh = -2; tl.cb = t - ntile; }
  const int rb = tl.rh >= 0 ? (tl.rh >> 1) : -1;                     // row block of a regular tile
  const int r0 = tl.rh >= 0 ? 3 * (tl.rh & 1) : 0;                   // first row of the tile inside its 6x6 block
  // poses the tile's row block / column block hold right now (-1: empty slot), interior flags
  const int eb_row = tl.cb * 36 + r0 * 6, eb_col = (rb >= 0 ? rb : 0) * 36 + r0;   // where (d) finds this tile's new entries in Eb
  const int pub0 = (tl.rh >= 0 ? 3 * tl.rh : RH) * 7;                // where this tile's rows go in the pivot-column buffer
  bool ir = false, ic = false;
  int q_r = rb >= 0 ? band_pose_of(sy, jb, 0, rb, &ir) : -1;
  int q_c = tl.rh != -1 ? band_pose_of(sy, jb, 0, tl.cb, &ic) : -1;
  // entry (i, k) of the tile for poses (qr, qc): the system's value, 0 outside the band / for an empty slot / between two
  // separator poses at level 0; lambda on the diagonal
  auto entry_addr = [&](int qr, bool intr, int qc, bool intc, int r, int c, bool* valid) -> int {
    *valid = qr >= 0 && qc >= 0 && !(jb.sep_zero && !intr && !intc);
    int dd = qc - qr;
    if (dd < 0) dd += sy.nP;
    const int db = sy.nP - dd;
    *valid = *valid && (dd <= sy.w || db <= sy.w);
    const int i_fwd = (qr * nb + dd) * 36 + r * 6 + c, i_bwd = (qc * nb + db) * 36 + c * 6 + r;
    return *valid ? (dd <= sy.w ? i_fwd : i_bwd) : 0;
  };
  // ---- initial window
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      double v = 0.0;
      if (tl.rh >= 0) {
        bool valid;
        const int idx = entry_addr(q_r, ir, q_c, ic, r0 + i, k, &valid);
        v = valid ? sy.Sb[idx] : 0.0;
        if (valid && rb == tl.cb && r0 + i == k) v += lambda;
      } else if (tl.rh == -2 && i == 0) {
        v = (q_c >= 0 && !(jb.sep_zero && !ic)) ? sy.bs[(size_t)q_c * 6 + k] : 0.0;
      }
      tl.W[i][k] = v;
    }
  // publish the columns of the first pivot (block 0)
  int cur = 0;
  if (tl.cb == 0) {
    if (tl.rh >= 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 6; ++k) Cb[(3 * tl.rh + i) * 7 + k] = tl.W[i][k];
    } else if (tl.rh == -2) {
#pragma unroll
      for (int k = 0; k < 6; ++k) Cb[RH * 7 + k] = tl.W[0][k];
    }
  }
  // the <= NF values of an entering pose this thread fetches: value v = t + NT k -> row-block f_rb, entry (f_r, f_c) of the
  // block (entering pose, pose of f_rb), or (f_rb == -2) entry f_r of its rhs; f_q = the pose f_rb holds right now
  constexpr int NF = 2;                                              // nvals <= 11 * 36 + 6 (NT = 256) / 15 * 36 + 6 (NT = 512)
  const int nvals = nblk * 36 + 6;
  int f_rb[NF], f_r[NF], f_c[NF], f_q[NF];
  bool f_int[NF], pv[NF];
  double pre[NF];
  int q_in = jb.p0 + nb;                                             // pose that enters after step e: p0 + e + nb (mod nP)
  while (q_in >= sy.nP) q_in -= sy.nP;
#pragma unroll
  for (int k = 0; k < NF; ++k) {
    const int v = t + k * NT;
    f_rb[k] = -1; f_r[k] = f_c[k] = 0; f_q[k] = -1; f_int[k] = false; pv[k] = false; pre[k] = 0.0;
    if (v < nblk * 36) {
      f_rb[k] = v / 36;
      const int rc = v - f_rb[k] * 36;
      f_r[k] = rc / 6; f_c[k] = rc - f_r[k] * 6;
      f_q[k] = band_pose_of(sy, jb, 0, f_rb[k], &f_int[k]);
    } else if (v < nvals) {
      f_rb[k] = -2; f_r[k] = v - nblk * 36;
    }
    // prologue: the pose that enters after step 0 (slot 0 is then the diagonal)
    const bool ent0 = (0 < jb.m) && (nb < jb.m + jb.nR);
    const bool int0 = nb < jb.m;
    if (f_rb[k] >= 0 && ent0) {
      const int qo = f_rb[k] == 0 ? q_in : f_q[k];
      const bool oint = f_rb[k] == 0 ? int0 : f_int[k];
      const bool valid = qo >= 0 && !(jb.sep_zero && !int0 && !oint);
      const double val = valid ? band_get(sy, q_in, qo, f_r[k], f_c[k]) : 0.0;
      pv[k] = valid; pre[k] = val;
    } else if (f_rb[k] == -2 && ent0) {
      const bool valid = !(jb.sep_zero && !int0);
      pv[k] = valid; pre[k] = valid ? sy.bs[(size_t)q_in * 6 + f_r[k]] : 0.0;
    }
  }
  __syncthreads();
  int ok = 1;
  int pb_band = 0;                                                   // e mod nb, kept incrementally
  for (int e = 0; e < n_elim; ++e) {
    const int pb = (e < jb.m) ? pb_band : nb + (e - jb.m);
    int pb_next = -1;
    if (e + 1 < n_elim) pb_next = (e + 1 < jb.m) ? (pb_band + 1 == nb ? 0 : pb_band + 1) : nb + (e + 1 - jb.m);
    const bool entering = (e < jb.m) && (e + nb < jb.m + jb.nR);
    const bool in_int = e + nb < jb.m;
    const double* cb_cur = Cb + (size_t)cur * NW * 7;
    double* cb_nxt = Cb + (size_t)(cur ^ 1) * NW * 7;
    // ---- the entering pose (it takes the pivot's slot after this step): its entries against every window pose, its
    // diagonal block and its rhs -- Eb[rbk * 36 + r * 6 + c] = S(entering pose row r, pose of row-block rbk column c),
    // Eb[nblk * 36 + r] = rhs -- were fetched from global memory DURING THE PREVIOUS STEP (<= NF values per thread, `pre`)
    // and go to LDS now; the owners of the tiles in the pivot's row / column block pick them up in (d).  Then the loads
    // for the next step are issued (unconditional, from an always-valid address; nothing waits on them in this step).
    const bool repl_r = rb == pb, repl_c = tl.cb == pb && tl.rh != -1;
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const int v = t + k * NT;
      if (v < nvals) Eb[v] = pv[k] ? pre[k] : 0.0;
    }
    {
      const bool ent_n = (e + 1 < jb.m) && (e + 1 + nb < jb.m + jb.nR);
      const bool int_n = e + 1 + nb < jb.m;
      int q_n = q_in + 1;
      if (q_n >= sy.nP) q_n -= sy.nP;
#pragma unroll
      for (int k = 0; k < NF; ++k) {
        int idx = 0;
        bool valid = false;
        const double* base = sy.Sb;
        if (f_rb[k] >= 0) {
          // the pose row-block f_rb[k] holds while the NEXT step runs
          int qo = f_q[k];
          bool oint = f_int[k];
          if (f_rb[k] == pb) { qo = entering ? q_in : -1; oint = entering && in_int; }
          if (f_rb[k] == pb_next) { qo = q_n; oint = int_n; }        // the diagonal block of the pose entering next
          valid = ent_n && qo >= 0 && !(jb.sep_zero && !int_n && !oint);
          int dd = qo - q_n;
          if (dd < 0) dd += sy.nP;
          const int db = sy.nP - dd;
          const int i_fwd = (q_n * nb + dd) * 36 + f_r[k] * 6 + f_c[k];
          const int i_bwd = (qo * nb + db) * 36 + f_c[k] * 6 + f_r[k];
          idx = dd <= sy.w ? i_fwd : i_bwd;
          valid = valid && (dd <= sy.w || db <= sy.w);
        } else if (f_rb[k] == -2) {
          valid = ent_n && !(jb.sep_zero && !int_n);
          base = sy.bs;
          idx = q_n * 6 + f_r[k];
        }
        pv[k] = valid;
        pre[k] = base[valid ? idx : 0];
      }
    }
    // ---- (a) factor the 6x6 pivot block: every thread, redundantly, identical arithmetic
    double L[6][6], inv[6];
    {
      const double* P = cb_cur + (size_t)(6 * pb) * 7;
      double A[6][6];
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) A[r][c] = P[r * 7 + c];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double dc = A[c][c];
#pragma unroll
        for (int k = 0; k < c; ++k) dc = fma(-L[c][k], L[c][k], dc);
        if (!(dc > 0.0) || !isfinite(dc)) ok = 0;
        const double y = rsqrt_nr(dc);
        inv[c] = y;
        L[c][c] = dc * y;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
          double v = A[r][c];
#pragma unroll
          for (int k = 0; k < c; ++k) v = fma(-L[r][k], L[c][k], v);
          L[r][c] = v * y;
        }
      }
    }
    if (!ok) break;                                                  // uniform
    double* out = Ls + (size_t)e * LS;
    if (t >= NT - 64 && t < NT - 64 + 36) {                          // (the last wave has no panel rows to solve)
      const int q = t - (NT - 64), r = q / 6, c = q - r * 6;
      double v = 0.0;
#pragma unroll
      for (int rr = 0; rr < 6; ++rr)
#pragma unroll
        for (int cc = 0; cc < 6; ++cc)
          if (rr == r && cc == c) v = (cc < rr) ? L[rr][cc] : (cc == rr ? inv[rr] : 0.0);
      out[q] = v;
    }
    // ---- (b) one thread per window row: its 6 panel entries  x L^T = c
    if (t < NW) {
      double x[6] = {0, 0, 0, 0, 0, 0};
      if (t < 6 * pb || t >= 6 * pb + 6) {
        const double* row = cb_cur + (size_t)t * 7;
        double cv[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) cv[j] = row[j];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          double sacc = cv[j];
#pragma unroll
          for (int k = 0; k < j; ++k) sacc = fma(-x[k], L[j][k], sacc);
          x[j] = sacc * inv[j];
        }
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) { Pn[t * 7 + j] = x[j]; out[36 + t * 6 + j] = x[j]; }
    }
    lds_barrier();
    // ---- (c) rank-6 update of the tile in registers (tiles of the pivot's row / column block are replaced in (d))
    if (tl.rh >= 0) {
      if (!repl_r && !repl_c) {
        double a[3][6], bq[6][6];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 6; ++j) a[i][j] = Pn[(3 * tl.rh + i) * 7 + j];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j < 6; ++j) bq[i][j] = Pn[(6 * tl.cb + i) * 7 + j];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int kk = 0; kk < 6; ++kk) {
            double sacc = 0.0;
#pragma unroll
            for (int j = 0; j < 6; ++j) sacc = fma(a[i][j], bq[kk][j], sacc);
            tl.W[i][kk] -= sacc;
          }
      }
    } else if (tl.rh == -2 && !repl_c) {
      double a[6], bq[6][6];
#pragma unroll
      for (int j = 0; j < 6; ++j) a[j] = Pn[RH * 7 + j];
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) bq[i][j] = Pn[(6 * tl.cb + i) * 7 + j];
#pragma unroll
      for (int kk = 0; kk < 6; ++kk) {
        double sacc = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) sacc = fma(a[j], bq[kk][j], sacc);
        tl.W[0][kk] -= sacc;
      }
    }
    // ---- (d) the freed slot: tiles of the pivot's row / column block take the entering pose's entries (zeros when no
    // pose enters) from Eb; lambda on the diagonal of an interior pose (level 0 separators start at zero).
    // A tile in the pivot's ROW block reads S(entering row r0 + i, pose of its column block, column k); a tile only in the
    // pivot's COLUMN block reads the transposed entry S(entering row k, pose of its row block, column r0 + i).
    if (tl.rh >= 0 && (repl_r || repl_c)) {
      const int eb0 = repl_r ? eb_row : eb_col, si = repl_r ? 6 : 1, sk = repl_r ? 1 : 6;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 6; ++k) tl.W[i][k] = Eb[eb0 + i * si + k * sk];
      if (repl_r && repl_c && entering && !(jb.sep_zero && !in_int)) {
        if (r0 == 0) { tl.W[0][0] += lambda; tl.W[1][1] += lambda; tl.W[2][2] += lambda; }
        else { tl.W[0][3] += lambda; tl.W[1][4] += lambda; tl.W[2][5] += lambda; }
      }
    } else if (tl.rh == -2 && repl_c) {
#pragma unroll
      for (int k = 0; k < 6; ++k) tl.W[0][k] = Eb[nblk * 36 + k];
    }
    if (repl_r) { q_r = entering ? q_in : -1; ir = entering && in_int; }
    if (repl_c) { q_c = entering ? q_in : -1; ic = entering && in_int; }
    // ---- publish the columns of the next pivot
    if (tl.cb == pb_next && tl.rh != -1) {
#pragma unroll
      for (int k = 0; k < 6; ++k) cb_nxt[pub0 + k] = tl.W[0][k];
      if (tl.rh >= 0) {
#pragma unroll
        for (int i = 1; i < 3; ++i)
#pragma unroll
          for (int k = 0; k < 6; ++k) cb_nxt[pub0 + i * 7 + k] = tl.W[i][k];
      }
    }
    // which pose the fetch slots' row-blocks hold from now on
#pragma unroll
    for (int k = 0; k < NF; ++k)
      if (f_rb[k] == pb) { f_q[k] = entering ? q_in : -1; f_int[k] = entering && in_int; }
    lds_barrier();
    cur ^= 1;
    if (e < jb.m) {
      if (++pb_band == nb) pb_band = 0;
      if (++q_in == sy.nP) q_in = 0;
    }
  }
  __syncthreads();
  return ok;
}

// Back-substitution of the poses a job eliminated, last to first:  x_e = L^-T (y_e - X_e^T x_rows).
// xs (LDS): solution per LOCAL pose slot -- [0, m) interior, [m, m+nR) the poses behind it, [m+nR, m+nR+nF) the fixed
// poses; the caller fills the entries of poses that were not eliminated here.  The factor is streamed from global
// memory in groups of BAND_G poses through a double-buffered LDS ring by the whole workgroup; wave 0 does the arithmetic.
template <int NT>
__device__ __forceinline__ void band_backsub(const BandSys sy, const BandJob jb, const double* Ls, int LS, double* xs, double* ring)
{
  constexpr int NREG = (BAND_G * 690 + NT - 1) / NT;                 // a group is BAND_G * rec <= 8 * 690 doubles
  const int t = threadIdx.x;
  const int nb = sy.w + 1, nblk = nb + jb.nF, RH = 6 * nblk, NW = RH + 1;
  const int n_elim = jb.m + (jb.elim_fixed ? jb.nF : 0);
  const int rec = 36 + NW * 6;                                       // doubles of one pose's record actually used
  const int ngroups = (n_elim + BAND_G - 1) / BAND_G;
  // group g covers e in [n_elim - (g+1) G, n_elim - g G) ∩ [0, n_elim)
  auto load_group = [&](int g, double* regs, int* cnt) {
    const int hi = n_elim - g * BAND_G, lo = max(hi - BAND_G, 0);
    const int total = (hi - lo) * rec;
    *cnt = total;
#pragma unroll
    for (int k = 0; k < NREG; ++k) {
      const int i = t + k * NT;
      if (i < total) {
        const int pe = i / rec, off = i - pe * rec;
        regs[k] = Ls[(size_t)(lo + pe) * LS + off];
      }
    }
  };
  double regs[NREG];
  int cnt = 0;
  if (ngroups > 0) load_group(0, regs, &cnt);
  for (int g = 0; g < ngroups; ++g) {
    double* buf = ring + (size_t)(g & 1) * BAND_G * rec;
#pragma unroll
    for (int k = 0; k < NREG; ++k) {
      const int i = t + k * NT;
      if (i < cnt) buf[i] = regs[k];
    }
    __syncthreads();
    if (g + 1 < ngroups) load_group(g + 1, regs, &cnt);              // in flight while wave 0 works through group g
    if (t < 64) {
      const int hi = n_elim - g * BAND_G, lo = max(hi - BAND_G, 0);
      for (int e = hi - 1; e >= lo; --e) {
        const double* R = buf + (size_t)(e - lo) * rec;
        const int pb = (e < jb.m) ? (e % nb) : nb + (e - jb.m);
        // lane l owns window rows l and l + 64 (NW <= 109)
        double acc[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int row = t + 64 * h;
          if (row >= RH) continue;
          const int rb = row / 6, rr = row - rb * 6;
          if (rb == pb) continue;
          // local solution slot of the pose in row-block rb at step e
          int slot = -1;
          if (rb >= nb) {
            const int f = rb - nb;
            if (e < jb.m || f > e - jb.m) slot = jb.m + jb.nR + f;
          } else if (e < jb.m) {
            int off = rb - pb;
            if (off < 0) off += nb;
            const int j = e + off;
            if (j < jb.m + jb.nR) slot = j;
          }
          if (slot < 0) continue;
          const double xv = xs[slot * 6 + rr];
#pragma unroll
          for (int c = 0; c < 6; ++c) acc[c] = fma(R[36 + row * 6 + c], xv, acc[c]);
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o);
        }
        // every lane: v = y - acc, solve L^T z = v (6 unknowns, redundantly)
        double z[6];
#pragma unroll
        for (int c = 5; c >= 0; --c) {
          double s = R[36 + RH * 6 + c] - acc[c];
#pragma unroll
          for (int r = c + 1; r < 6; ++r) s = fma(-R[r * 6 + c], z[r], s);
          z[c] = s * R[c * 6 + c];
        }
        const int slot_e = (e < jb.m) ? e : jb.m + jb.nR + (e - jb.m);
        if (t < 6) {
          double v = z[0];
#pragma unroll
          for (int c = 1; c < 6; ++c) if (t == c) v = z[c];
          xs[slot_e * 6 + t] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
      }
    }
    __syncthreads();
  }
}

// LDS bytes of the elimination window / of the back-substitution (xs + ring) for a job shape
static inline size_t band_lds_elim(int w, int nF)
{
  const int NW = 6 * (w + 1 + nF) + 1;
  return sizeof(double) * ((size_t)3 * NW * 7 + (size_t)(w + 1 + nF) * 36 + 8);
}
static inline size_t band_lds_back(int w, int nF, int nslots)
{
  const int NW = 6 * (w + 1 + nF) + 1;
  return sizeof(double) * ((size_t)nslots * 6 + 2 * (size_t)BAND_G * (36 + NW * 6));
}

// ---- level 0: one workgroup per segment ----------------------------------------------------------------------------
__global__ __launch_bounds__(BAND_T, 1) void k_band_seg(BaDev d, BandDev bd)
{
  extern __shared__ __attribute__((aligned(16))) double band_smem[];
  if (d.scal[SC_STOP] != 0.0) return;                                  // device-driven LM, already terminated
  const double lambda = d.scal[SC_LAMBDA];
  const int k = blockIdx.x, t = threadIdx.x, w = bd.w;
  BandSys sy{bd.nP, w, bd.Sb, bd.bsv};
  BandJob jb{bd.seg_p0[k], bd.seg_m[k], w, w, 0, 1};
  BandTile tl;
  const int ok = band_eliminate<BAND_T>(sy, jb, lambda, bd.Ls0 + (size_t)jb.p0 * bd.LS0, bd.LS0, band_smem, tl);
  if (!ok) { if (t == 0) d.scal[SC_SOLVE_OK] = 0.0; return; }
  // the tiles now hold the Schur update on [band slots of the right separator | left separator | rhs]: every thread
  // writes its entries at their canonical place [left separator | right separator | rhs] of U
  const int nb = w + 1, RH = 6 * (nb + w);
  const int NU = 12 * w + 1;
  double* U = bd.U + (size_t)k * NU * NU;
  auto canon = [&](int wrow) -> int {                                // window row -> canonical index, -1 = not part of the result
    if (wrow == RH) return NU - 1;
    const int blk = wrow / 6, r = wrow - 6 * blk;
    if (blk >= nb) return 6 * (blk - nb) + r;                        // left separator = the fixed rows
    // band slot blk holds the right-separator pose j in [m, m + w) with j mod nb == blk (one slot is empty)
    int j = jb.m + ((blk - jb.m % nb) + nb) % nb;
    if (j >= jb.m + w) return -1;
    return 6 * w + 6 * (j - jb.m) + r;
  };
  if (tl.rh >= 0 || tl.rh == -2) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (tl.rh == -2 && i > 0) break;
      const int ca = canon(tl.rh >= 0 ? 3 * tl.rh + i : RH);
#pragma unroll
      for (int kk = 0; kk < 6; ++kk) {
        const int cbn = canon(6 * tl.cb + kk);
        if (ca >= 0 && cbn >= 0) U[(size_t)ca * NU + cbn] = tl.W[i][kk];
      }
    }
  }
}

// ---- separator system: S_sep + lambda I + the segments' updates, in band layout (nPr = K w poses, bandwidth 2w-1) --------
// reduced pose i = k w + a  <->  pose seg_p0[k] + seg_m[k] + a  (separator k sits behind segment k's interior)
__global__ __launch_bounds__(BAND_T) void k_band_assemble(BaDev d, BandDev bd)
{
  const double lambda = d.scal[SC_LAMBDA];
  const int w = bd.w, K = bd.K, wr = bd.wr, nPr = bd.nPr;
  const int NU = 12 * w + 1;
  BandSys sy{bd.nP, w, bd.Sb, bd.bsv};
  const int total = nPr * (wr + 1) * 36 + 6 * nPr;
  for (int idx = blockIdx.x * BAND_T + threadIdx.x; idx < total; idx += gridDim.x * BAND_T) {
    double v = 0.0;
    if (idx < nPr * (wr + 1) * 36) {
      const int i = idx / ((wr + 1) * 36), rem = idx - i * (wr + 1) * 36, dd = rem / 36, rc = rem - dd * 36, r = rc / 6, c = rc - r * 6;
      const int i2 = (i + dd) % nPr;
      const int ka = i / w, aa = i - ka * w, kb = i2 / w, ab = i2 - kb * w;
      const int qa = (bd.seg_p0[ka] + bd.seg_m[ka] + aa) % bd.nP, qb = (bd.seg_p0[kb] + bd.seg_m[kb] + ab) % bd.nP;
      v = band_get(sy, qa, qb, r, c);
      if (i == i2 && r == c) v += lambda;
      if (ka == kb) {
        // separator ka is the RIGHT separator of segment ka and the LEFT separator of segment ka + 1
        const int kn = (ka + 1) % K;
        v += bd.U[(size_t)ka * NU * NU + (size_t)(6 * w + 6 * aa + r) * NU + (6 * w + 6 * ab + c)];
        v += bd.U[(size_t)kn * NU * NU + (size_t)(6 * aa + r) * NU + (6 * ab + c)];
      } else {
        // two different separators are coupled through the segment between them (for K == 2 through both segments):
        // segment kb has ka on its left, or segment ka has kb on its left
        if (kb == (ka + 1) % K) v += bd.U[(size_t)kb * NU * NU + (size_t)(6 * w + 6 * ab + c) * NU + (6 * aa + r)];
        if (ka == (kb + 1) % K) v += bd.U[(size_t)ka * NU * NU + (size_t)(6 * w + 6 * aa + r) * NU + (6 * ab + c)];
      }
    } else {
      const int j = idx - nPr * (wr + 1) * 36, i = j / 6, r = j - i * 6;
      const int ka = i / w, aa = i - ka * w, kn = (ka + 1) % K;
      const int qa = (bd.seg_p0[ka] + bd.seg_m[ka] + aa) % bd.nP;
      v = bd.bsv[(size_t)qa * 6 + r];
      v += bd.U[(size_t)ka * NU * NU + (size_t)(NU - 1) * NU + (6 * w + 6 * aa + r)];
      v += bd.U[(size_t)kn * NU * NU + (size_t)(NU - 1) * NU + (6 * aa + r)];
    }
    bd.Sr[idx] = v;
  }
}

// ---- top level: complete factorisation + back-substitution of a (small) cyclic band system by ONE workgroup ------------
// single level (K == 1): the whole reduced pose system, the last w poses as fixed rows (they carry the wrap-around);
// K > 1: the separator system from k_band_assemble (lambda already inside).
__global__ __launch_bounds__(BAND_TOP_T, 1) void k_band_top(BaDev d, BandDev bd, BigDev b)
{
  extern __shared__ __attribute__((aligned(16))) double band_smem[];
  const int t = threadIdx.x;
  if (d.scal[SC_STOP] != 0.0) return;                                  // device-driven LM, already terminated
  const bool single = bd.K == 1;
  const double lambda = single ? d.scal[SC_LAMBDA] : 0.0;
  const int nP = single ? bd.nP : bd.nPr, w = single ? bd.w : bd.wr, nF = bd.w;
  const double* Sb = single ? bd.Sb : bd.Sr;
  BandSys sy{nP, w, Sb, Sb + (size_t)nP * (w + 1) * 36};
  BandJob jb{0, nP - nF, nF, 0, 1, 0};
  if (d.scal[SC_SOLVE_OK] == 0.0) return;                            // a segment met a non-positive pivot
  BandTile tl;
  const int ok = band_eliminate<BAND_TOP_T>(sy, jb, lambda, bd.Ls1, bd.LS1, band_smem, tl);
  if (!ok) { if (t == 0) d.scal[SC_SOLVE_OK] = 0.0; return; }
  __syncthreads();
  double* xs = band_smem;
  double* ring = band_smem + (size_t)nP * 6;
  __threadfence_block();
  band_backsub<BAND_TOP_T>(sy, jb, bd.Ls1, bd.LS1, xs, ring);
  __syncthreads();
  // local slot order = pose order here (interior 0..m-1, then the fixed poses m..nP-1)
  if (single) {
    for (int i = t; i < 6 * nP; i += BAND_TOP_T) b.x[i] = xs[i];
  } else {
    for (int i = t; i < 6 * nP; i += BAND_TOP_T) {
      bd.xr[i] = xs[i];
      const int pr = i / 6, ka = pr / bd.w, aa = pr - ka * bd.w;
      const int q = (bd.seg_p0[ka] + bd.seg_m[ka] + aa) % bd.nP;
      b.x[(size_t)q * 6 + i % 6] = xs[i];
    }
  }
}

// ---- level 0 back-substitution: one workgroup per segment ---------------------------------------------------------------
__global__ __launch_bounds__(BAND_T, 1) void k_band_back(BaDev d, BandDev bd, BigDev b)
{
  extern __shared__ __attribute__((aligned(16))) double band_smem[];
  if (d.scal[SC_SOLVE_OK] == 0.0 || d.scal[SC_STOP] != 0.0) return;
  const int k = blockIdx.x, t = threadIdx.x, w = bd.w;
  BandSys sy{bd.nP, w, bd.Sb, bd.bsv};
  BandJob jb{bd.seg_p0[k], bd.seg_m[k], w, w, 0, 1};
  double* xs = band_smem;
  double* ring = band_smem + (size_t)(jb.m + 2 * w) * 6;
  // separators: right = separator k (poses p0+m ..), left = separator k-1 (poses p0-w ..)
  for (int i = t; i < 6 * w; i += BAND_T) {
    const int qr = (jb.p0 + jb.m + i / 6) % bd.nP;
    int ql = jb.p0 - w + i / 6;
    if (ql < 0) ql += bd.nP;
    xs[(jb.m + i / 6) * 6 + i % 6] = b.x[(size_t)qr * 6 + i % 6];
    xs[(jb.m + w + i / 6) * 6 + i % 6] = b.x[(size_t)ql * 6 + i % 6];
  }
  __syncthreads();
  band_backsub<BAND_T>(sy, jb, bd.Ls0 + (size_t)jb.p0 * bd.LS0, bd.LS0, xs, ring);
  __syncthreads();
  for (int i = t; i < 6 * jb.m; i += BAND_T) b.x[(size_t)((jb.p0 + i / 6) % bd.nP) * 6 + i % 6] = xs[i];
}

// one wave per non-zero block of S (as k_schur_blocks), written into the band layout; wrap-around blocks transposed
__global__ __launch_bounds__(CH) void k_schur_blocks_band(BaDev d, BigDev b, BandDev bd)
{
  if (d.scal[SC_STOP] != 0.0) return;                                  // device-driven LM, already terminated
  const int lane = threadIdx.x & 63;
  const int blk = blockIdx.x * 4 + (threadIdx.x >> 6), qr = (lane >> 1) & 1, qc = lane & 1;
  if (blk >= b.nBlkS) return;
  double v[3][3];
  schur_block_quarter(d, b, blk, lane, v);
  if (lane >= 4) return;                                             // the slot-0 lanes hold the sums
  const int pa = b.sblk_pa[blk], pb = b.sblk_pb[blk];
  const int dd = pb - pa;                                            // pa <= pb
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int r = 3 * qr + i, c = 3 * qc + j;
      if (dd <= bd.w) bd.Sb[((size_t)pa * (bd.w + 1) + dd) * 36 + r * 6 + c] = v[i][j];
      else bd.Sb[((size_t)pb * (bd.w + 1) + (bd.nP - dd)) * 36 + c * 6 + r] = v[i][j];
    }
}

// right-hand side bs = bp - sum_e Cv[e] (pose-major, fixed tree) into the band buffer; also resets the solve flag
__global__ __launch_bounds__(CH) void k_bs_band(BaDev d, BigDev b, BandDev bd)
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
  if (t < 6) bd.bsv[6 * pf + t] = d.bp[pf * 6 + t] - sRed[t][0];
  if (pf == 0 && t == 0) d.scal[SC_SOLVE_OK] = 1.0;
}
