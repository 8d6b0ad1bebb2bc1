// ssvio_amd/csrc/ba_bcr.inc -- BLOCK CYCLIC REDUCTION of the cyclic block band (included by ba.hip after ba_band.inc).
//
// The reduced pose system of a trajectory-shaped window (BlockSolver::solve, thirdparty/g2o/g2o/core/block_solver.hpp:342-447;
// the reference factors it with CSparse, solvers/csparse/linear_solver_csparse.h:106-142) is cyclically block-banded with
// bandwidth w <= 5 poses (ba_band.inc).  The sliding-window / nested-dissection solver of ba_band.inc walks a chain of
// nP / K + K w DEPENDENT 6x6 pivots (98 at BASELINE configs[3]) at 2.4 - 4.5 us each: 0.43 ms per LM trial, which every rank of
// a landmark-sharded solve repeats (DESIGN.md section 7).  Here the chain is log2(N) long:
//
//   * the poses are cut into N = floor(nP / w) SUPER-BLOCKS of w or w + 1 consecutive poses (padded to m = 24 or 36 unknowns
//     with identity rows).  Every super-block holds >= w poses, so two poses that share a block of the band lie in the same or
//     in ADJACENT super-blocks: the system is block-TRIDIAGONAL, cyclic (the wrap-around couples the last super-block to the
//     first), with dense m x m blocks  D_i  (diagonal),  E_i = block (i, right neighbour of i).
//   * CYCLIC REDUCTION: a level eliminates every other super-block of the still active (cyclic) list, all of them concurrently,
//     one workgroup each: D_j = L L^T;  U_l = L^-1 E_l^T,  U_r = L^-1 E_j,  y = L^-1 r_j  (one augmented in-place elimination:
//     the right-hand columns ride with the Cholesky steps);  the neighbours take  D_l -= U_l^T U_l,  D_r -= U_r^T U_r,
//     r_l -= U_l^T y,  r_r -= U_r^T y  and become neighbours of each other through  E_l <- - U_l^T U_r.   N = 100 at configs[3]:
//     50 + 25 + 12 + 6 + 3 + 2 + 1 + 1 eliminations in 8 levels, then 8 levels of back-substitution
//     x_j = L^-T (y - U_l x_l - U_r x_r) -- 17 short launches instead of a 98-pivot chain.
//     Measured at configs[3] (profiles/r05/bcr.md): 14 us per elimination level, 4.7 us per back-substitution level, 7.7 us
//     for the build: 0.16 ms per trial against 0.43 ms of the chain.
//   * no atomics, fixed order: a kept super-block receives the update of its RIGHT eliminated neighbour in DR / RR and of its
//     LEFT one in DL / RL (one writer per buffer and level, levels ordered by the stream), and reads D - DL - DR when its own turn
//     comes.  Identical bits from run to run and on every rank of a sharded solve.
//
// 10 x the floating-point work of the band elimination (dense 36 x 36 blocks: ~30 Mflop per trial) -- irrelevant on this chip: what
// the band solver spends is the LATENCY of its dependent chain.

constexpr int BCR_T = 256;                         // forward kernel: 2 row groups x 128 columns (one wave per SIMD: the cheapest barrier)
constexpr int BCR_S = 4;                           // workgroups per eliminated super-block (they share its products and stores)
constexpr int BCR_MMAX = 6 * (BAND_WMAX + 1);      // 36 unknowns per super-block at w = 5
constexpr int BCR_MIN_BLOCKS = 8;                  // below that the one-workgroup band solver is as fast

// (struct BcrDev / BcrPlan: ba_band.inc, beside BandDev)

static void plan_bcr(int nP, int w, BcrPlan& bp)
{
  bp = BcrPlan{};
  static const bool off = getenv("SSX_BA_BAND_CHAIN") != nullptr;     // (tools / tests: the sliding-window solver of ba_band.inc instead)
  if (off || w <= 0 || w > BAND_WMAX || nP / w < BCR_MIN_BLOCKS) return;
  // super-blocks of g or g + 1 consecutive poses, g >= w (two poses that share a block of the band then lie in the same or in adjacent
  // super-blocks); narrow bands (w <= 2: pose graphs, stereo-only tracks) take g = 3 -- a quarter of the 24-wide kernels' columns would
  // be identity padding at g = 1 and the reduction two levels deeper
  const int g = std::max(w, 3);
  if (nP / g < BCR_MIN_BLOCKS) return;
  const int N = nP / g, rem = nP - N * g;          // rem < g: the blocks 1, 3, .. 2 rem - 1 hold g + 1 poses -- all of them go in
                                                   // level 0 (N >= 8 > 2 rem - 1 for g <= 5), later levels mostly skip the padding
  bp.on = 1; bp.N = N;
  bp.m = 6 * (g + (rem > 0 ? 1 : 0)) <= 24 ? 24 : 36;               // the kernels come in two sizes; the rest of a block is identity padding
  bp.p0.resize(N + 1);
  int p = 0;
  for (int i = 0; i < N; ++i) { bp.p0[i] = p; p += g + ((i & 1) && i < 2 * rem ? 1 : 0); }
  bp.p0[N] = p;
  std::vector<int> act(N);
  for (int i = 0; i < N; ++i) act[i] = i;
  auto push = [&](int j, int l, int r) { bp.elim.push_back(j); bp.elim.push_back(l); bp.elim.push_back(r); bp.elim.push_back(0); };
  while (act.size() > 2) {
    bp.lvl.push_back((int)bp.elim.size() / 4);
    const int M = (int)act.size();
    bp.lvM.push_back(M);
    std::vector<int> keep;
    for (int pos = 0; pos < M; ++pos) {
      if (pos & 1) push(act[pos], act[pos - 1], act[(pos + 1) % M]);
      else keep.push_back(act[pos]);
    }
    act.swap(keep);
  }
  if (act.size() == 2) {                            // two blocks, coupled in both directions
    bp.lvl.push_back((int)bp.elim.size() / 4);
    bp.lvM.push_back(2);
    push(act[1], act[0], act[0]);
    act.resize(1);
  }
  bp.lvl.push_back((int)bp.elim.size() / 4);
  bp.lvM.push_back(1);
  push(act[0], -1, -1);
  bp.lvl.push_back((int)bp.elim.size() / 4);
}

// Who a workgroup of a level eliminates, from the level alone (the list `elim` of the plan says the same; reading it would put a
// memory round trip in front of every load of the kernel): the active list of level q is { pos << q }, Mq long, the odd positions go.
__device__ __forceinline__ void bcr_who(int sh, int Mq, int b, int& j, int& l, int& r)
{
  if (Mq == 1) { j = 0; l = r = -1; return; }                         // the last super-block, alone
  const int pos = 2 * b + 1, pr = pos + 1 == Mq ? 0 : pos + 1;        // (Mq == 2: l == r, coupled in both directions)
  j = pos << sh; l = (pos - 1) << sh; r = pr << sh;
}

static inline size_t bcr_mem_doubles(int N, int m) { return (size_t)N * (8 * (size_t)m * m + 5 * (size_t)m); }
// the memory of a reduction of N super-blocks of m columns, carved from the bcr_mem_doubles(N, m) doubles at base
static inline void bcr_carve(BcrDev& q, double* base, int N, int m)
{
  q.on = 1; q.N = N; q.m = m;
  const size_t mmN = (size_t)N * m * m, mN = (size_t)N * m;
  q.D = base; q.E = q.D + mmN; q.DL = q.E + 2 * mmN;   /* E: two buffers, bcr_e_buf */ q.DR = q.DL + mmN; q.Lf = q.DR + mmN; q.Ul = q.Lf + mmN; q.Ur = q.Ul + mmN;
  q.R = q.Ur + mmN; q.RL = q.R + mN; q.RR = q.RL + mN; q.Y = q.RR + mN; q.X = q.Y + mN;
}
// doubles of the band of nP poses at bandwidth w (BandDev::Sb), and of [band | rhs] (the rhs, BandDev::bsv, starts behind the band)
static inline size_t band_doubles(int nP, int w) { return (size_t)nP * (w + 1) * 36; }
static inline size_t band_rhs_doubles(int nP, int w) { return band_doubles(nP, w) + 6 * (size_t)nP; }

// The coupling blocks E live in TWO buffers (BcrDev::E, E + N m m).  The BCR_S workgroups that eliminate j all read E_l, and one of
// them stores the new coupling (l, r) = - U_l^T U_r under the same index l: written where it is read, a workgroup dispatched late
// (other streams keeping the chip busy) would load a partly updated E_l.  So the new block goes to the OTHER buffer, and which
// buffer holds the current E_i follows from the schedule alone: E_i changes buffers at every level at which i is kept at a position
// whose right neighbour is eliminated (every kept position but the last one of an odd-length list; not when two blocks are left).
__device__ __forceinline__ int bcr_e_buf(int N, int i, int sh)
{
  int buf = 0, Mk = N;
  for (int k = 0; k < sh; ++k) {
    if (Mk > 2 && (i >> k) + 1 < Mk) buf ^= 1;
    Mk = (Mk + 1) >> 1;
  }
  return buf;
}

// ---- the super-blocks out of the band storage (lambda on the diagonal of real poses, identity on the padding) ----------------
__global__ __launch_bounds__(256) void k_bcr_build(BaDev d, BandDev bd, BcrDev q, double lambda_arg, int use_dev_lambda)
{
  if (use_dev_lambda == 2 && d.scal[SC_STOP] != 0.0) return;          // device-driven LM, already terminated
  const double lambda = use_dev_lambda ? d.scal[SC_LAMBDA] : lambda_arg;
  const int i = blockIdx.x, t = threadIdx.x, m = q.m, mm = m * m;
  const int nx = i + 1 == q.N ? 0 : i + 1;
  const int pi = q.p0[i], ni = q.p0[i + 1] - pi, pn = q.p0[nx], nn = q.p0[nx + 1] - pn;
  BandSys sy{bd.nP, bd.w, bd.Sb, bd.bsv};
  for (int idx = t; idx < mm; idx += 256) {
    const int a = idx / m, b = idx - a * m;
    const int pa = a / 6, ra = a - 6 * pa, pb = b / 6, rb = b - 6 * pb;
    double dv = a == b ? 1.0 : 0.0, ev = 0.0;
    if (pa < ni && pb < ni) dv = band_get(sy, pi + pa, pi + pb, ra, rb) + (a == b ? lambda : 0.0);
    if (pa < ni && pb < nn && q.N > 1) ev = band_get(sy, pi + pa, pn + pb, ra, rb);
    const size_t o = (size_t)i * mm + idx;
    q.D[o] = dv; q.E[o] = ev; q.DL[o] = 0.0; q.DR[o] = 0.0;     // (E: buffer 0, see bcr_e_buf)
  }
  for (int a = t; a < m; a += 256) {
    const int pa = a / 6;
    const size_t o = (size_t)i * m + a;
    q.R[o] = pa < ni ? bd.bsv[(size_t)(pi + pa) * 6 + (a - 6 * pa)] : 0.0;
    q.RL[o] = 0.0; q.RR[o] = 0.0;
  }
}

// ---- one level of the reduction: one workgroup per eliminated super-block ---------------------------------------------------
// The augmented block  [ D_j | block (j, l) | block (j, r) | r_j ]  (M rows x W = 3 M + 1 columns) lives in REGISTERS: thread
// (rg, c) of RG row groups x 128 columns owns column c of the rows rg, rg + RG, rg + 2 RG, ...  A Cholesky step k: the row group that
// owns row k publishes it (one LDS row, double buffered: ONE barrier per step), every thread takes the pivot, its column's entry
// and -- broadcast reads -- the entries of its rows, and updates its <= M / 3 registers.  [The first version kept the block in LDS
// and read-modified-wrote it: 2 000 cycles per step, 47 us per level.]  The scaled pivot rows  O = [ L^T | U_l | U_r | y ]  go to
// LDS for the products  [U_l U_r]^T [U_l U_r y]  (4 x 4 register tiles) and from there to global memory.
template <int M>
__global__ __launch_bounds__(BCR_T) void k_bcr_fwd(BaDev d, BcrDev q, int sh, int Mq, int dev_lm)
{
  constexpr int W = 3 * M + 1, RG = BCR_T / 128, NR = M / RG;
  static_assert(M % 4 == 0 && M % (BCR_T / 128) == 0, "row groups, 4 x 4 product tiles");
  __shared__ double O[M * W];
  __shared__ double rowbuf[2][128];
  if (d.scal[SC_SOLVE_OK] == 0.0 || (dev_lm && d.scal[SC_STOP] != 0.0)) return;
  const int t = threadIdx.x, mm = M * M;
  int j, l, r;
  bcr_who(sh, Mq, blockIdx.x, j, l, r);
  const bool both = l >= 0 && l == r;                                  // two blocks left: j and l are coupled in both directions
  const int rg = t >> 7, c = t & 127;
  const int mreal = 6 * (q.p0[j + 1] - q.p0[j]);                       // the rows behind are identity padding: no elimination steps for them
  // the block's sources, branch-free: three strided streams and their signs per thread (a column class per thread; a condition
  // per element costs a branch and a memory round trip each -- 26 000 cycles of 68 000 in the first build).  Unused streams read
  // D_j[0][0] with sign 0.
  const double* dummy = q.D + (size_t)j * mm;
  const size_t e_buf = (size_t)q.N * mm;                               // the second buffer of the coupling blocks (bcr_e_buf)
  const double* Ej = q.E + (size_t)bcr_e_buf(q.N, j, sh) * e_buf + (size_t)j * mm;
  const int lbuf = l >= 0 ? bcr_e_buf(q.N, l, sh) : 0;
  const double* El = q.E + (size_t)lbuf * e_buf + (size_t)(l >= 0 ? l : 0) * mm;
  double* El_new = q.E + (size_t)(lbuf ^ 1) * e_buf + (size_t)(l >= 0 ? l : 0) * mm;   // never the buffer the sibling workgroups read
  const double *pA = dummy, *pB = dummy, *pC = dummy;
  int stA = 0, stB = 0, stC = 0;
  double sA = 0.0, sB = 0.0, sC = 0.0;
  if (c < M) {
    const size_t o = (size_t)j * mm + rg * M + c;
    pA = q.D + o; pB = q.DL + o; pC = q.DR + o; stA = stB = stC = RG * M; sA = 1.0; sB = sC = -1.0;
  } else if (c < 2 * M) {
    const int cc = c - M;
    if (l >= 0) { pA = El + cc * M + rg; stA = RG; sA = 1.0; }                              // block (j, l) = E_l^T
    if (both) { pB = Ej + rg * M + cc; stB = RG * M; sB = 1.0; }                            // + block (j, r = l) = E_j
  } else if (c < 3 * M) {
    const int cc = c - 2 * M;
    if (r >= 0 && !both) { pA = Ej + rg * M + cc; stA = RG * M; sA = 1.0; }                 // block (j, r) = E_j
  } else if (c == 3 * M) {
    const size_t o = (size_t)j * M + rg;
    pA = q.R + o; pB = q.RL + o; pC = q.RR + o; stA = stB = stC = RG; sA = 1.0; sB = sC = -1.0;
  }
  double a[NR];
  {
    double va[NR], vb[NR], vc[NR];
#pragma unroll
    for (int n = 0; n < NR; ++n) { va[n] = pA[n * stA]; vb[n] = pB[n * stB]; vc[n] = pC[n * stC]; }
#pragma unroll
    for (int n = 0; n < NR; ++n) a[n] = fma(sC, vc[n], fma(sB, vb[n], sA * va[n]));         // (D - DL) - DR, exactly
  }
  int ok = 1;
  if (rg == 0) rowbuf[0][c] = a[0];
#pragma unroll
  for (int nk = 0; nk < NR; ++nk) {
#pragma unroll
    for (int rk = 0; rk < RG; ++rk) {
      const int k = RG * nk + rk, k1 = k + 1 < M ? k + 1 : k;
      const double* rb = rowbuf[k & 1];
      if (k >= mreal) continue;                                        // (uniform over the workgroup)
      __syncthreads();
      double piv = rb[k], akc = rb[c], rnx = rb[k1];
      asm volatile("" : "+v"(piv), "+v"(akc), "+v"(rnx));              // the three the next pivot row waits for: one LDS round trip
      double ri[NR];
#pragma unroll
      for (int n = nk; n < NR; ++n) ri[n] = rb[rg + RG * n];             // (broadcast reads, behind the rsqrt chain: the pivot row's entries of my rows)
      if (!(piv > 0.0) || !isfinite(piv)) ok = 0;                      // (every thread reads the same value)
      // akc / piv for the updates: v_rcp_f64 + two Newton steps, 6 dependent instructions up to the next pivot row (through
      // rsqrt and s * s: 10); the rsqrt is for the stored factor only, off the critical path
      double x = __builtin_amdgcn_rcp(piv);
      x = fma(fma(-piv, x, 1.0), x, x);
      x = fma(fma(-piv, x, 1.0), x, x);
      const double f = akc * x;
      const double s = rsqrt_nr(piv);
      // the NEXT pivot row first, and out to LDS: the critical path of a step is  barrier - read - rsqrt - one fma - write
      const double pub = fma(-rnx, f, a[k1 / RG]);
      if (k + 1 < M && rg == k1 % RG) rowbuf[k1 & 1][c] = pub;
      if (rg == rk && c >= k && c < W) O[k * W + c] = c == k ? s : akc * s;   // (the diagonal holds 1 / L_kk: the back-substitution multiplies)
      // every register of the rows >= nk RG takes the update, needed or not: finished rows and the lower triangle hold values
      // nobody reads, and a condition here costs a branch around each LDS read (the first build: 1 800 cycles per step).  The
      // empty asm pins the results here: left alone the compiler defers each row's updates to the step that publishes it --
      // a chain of up to 35 dependent fmas on the critical path.
#pragma unroll
      for (int n = nk; n < NR; ++n) { a[n] = fma(-ri[n], f, a[n]); asm volatile("" : "+v"(a[n])); }
    }
  }
  for (int idx = mreal * W + t; idx < M * W; idx += BCR_T) {           // the padding rows of O: unit diagonal, nothing else
    const int k = idx / W, cc = idx - k * W;
    O[idx] = cc == k ? 1.0 : 0.0;
  }
  __syncthreads();
  if (!ok) { if (t == 0) d.scal[SC_SOLVE_OK] = 0.0; return; }
  // The rest is shared by the BCR_S workgroups of this super-block (blockIdx.y; each repeated the elimination above: the chip has
  // five times more CUs than a level has super-blocks, and the products were 14 000 of 68 000 cycles in one workgroup).
  const int part = blockIdx.y;
  // the factor and the solved columns, for the back-substitution (strictly lower part of Lf: zero): a matrix per workgroup
  if (part < 3) {
    double* dstm = (part == 0 ? q.Lf : part == 1 ? q.Ul : q.Ur) + (size_t)j * mm;
    const int off = part * M;
#pragma unroll 1
    for (int idx = t; idx < mm; idx += BCR_T) {
      const int k = idx / M, cc = idx - k * M;
      dstm[idx] = (part > 0 || cc >= k) ? O[k * W + off + cc] : 0.0;
    }
  } else {
    for (int k = t; k < M; k += BCR_T) q.Y[(size_t)j * M + k] = O[k * W + 3 * M];
  }
  // the neighbours' Schur updates and their new coupling:  Z^T [Z | y]  with  Z = [U_l U_r]  (M x 2 M), in 2 x 4 register tiles
  // (TA = M / 2 tile rows, TB = M / 4 tile columns):  tiles [0, TU) = the upper triangle of U_l^T U_l (nobody reads the lower one
  // of D - DL - DR; tile row ta holds the columns tb >= ta / 2), [TU, TU + T2) = U_l^T U_r, then the upper triangle of U_r^T U_r;
  // dealt to the BCR_S workgroups in turn.  The old values of the accumulation targets are requested BEFORE the products.
  constexpr int TA = M / 2, TB = M / 4, T2 = TA * TB, TU = 2 * (TB * (TB + 1) / 2), NT = 2 * TU + T2;
  static_assert((NT + BCR_S - 1) / BCR_S <= BCR_T - 2 * M, "one tile per thread, the last 2 M threads free");
  const int u = t * BCR_S + part;
  if (u < NT) {
    int blk, ta, tb;
    if (u >= TU && u < TU + T2) { blk = 1; ta = (u - TU) / TB; tb = (u - TU) - ta * TB; }
    else {
      blk = u < TU ? 0 : 2;
      int v = u < TU ? u : u - TU - T2;
      ta = 0;
      while (v >= TB - (ta >> 1)) { v -= TB - (ta >> 1); ++ta; }        // tile row ta of the triangle holds TB - ta / 2 tiles
      tb = (ta >> 1) + v;
    }
    const int ca = (blk == 2 ? 2 * M : M) + 2 * ta, cb = (blk == 0 ? M : 2 * M) + 4 * tb;
    const bool on = blk == 0 ? (l >= 0) : (r >= 0 && !both && (blk == 2 || l >= 0));
    double* dst = blk == 0 ? q.DR + (size_t)(l >= 0 ? l : 0) * mm       // this block is the RIGHT neighbour of l
                : blk == 2 ? q.DL + (size_t)(r >= 0 ? r : 0) * mm       // ... and the LEFT neighbour of r
                           : El_new;                                    // l and r are neighbours from now on: block (l, r)
    dst += (2 * ta) * M + 4 * tb;
    double old[2][4];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y) old[x][y] = (on && blk != 1) ? dst[x * M + y] : 0.0;
    double acc[2][4];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y) acc[x][y] = 0.0;
    const int kend = (mreal + 3) & ~3;                                 // (rows [mreal, kend): zero in the U columns)
#pragma unroll 4
    for (int k = 0; k < kend; ++k) {
      double za[2], zb[4];
#pragma unroll
      for (int x = 0; x < 2; ++x) za[x] = O[k * W + ca + x];
#pragma unroll
      for (int y = 0; y < 4; ++y) zb[y] = O[k * W + cb + y];
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = fma(za[x], zb[y], acc[x][y]);
    }
    if (on) {
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) dst[x * M + y] = blk == 1 ? -acc[x][y] : old[x][y] + acc[x][y];
    }
  }
  if (part == BCR_S - 1 && t >= BCR_T - 2 * M) {                       // Z^T y: the last 2 M threads of the last workgroup (no tile there)
    const int a2 = t - (BCR_T - 2 * M);                                // column of Z
    double v = 0.0;
#pragma unroll 4
    for (int k = 0; k < M; ++k) v = fma(O[k * W + M + a2], O[k * W + 3 * M], v);
    if (a2 < M) { if (l >= 0) q.RR[(size_t)l * M + a2] += v; }
    else if (r >= 0 && !both) q.RL[(size_t)r * M + (a2 - M)] += v;
  }
}

// ---- one level of the back-substitution: x_j = L^-T (y - U_l x_l - U_r x_r); one workgroup per super-block ------------------------
// Everything the block needs is requested in ONE memory round trip at the top (row t of Lf into the registers of lane t of the
// first wave, the quarter rows of U_l / U_r, the neighbours' x, y); the triangular solve runs unrolled out of registers, the
// running right-hand sides passed between lanes with readlane.  [First version: Lf staged through LDS behind the load of the
// elimination list, conditional loads in the products: 23 000 cycles; the chain of 36 steps itself is ~1 500.]
template <int M>
__global__ __launch_bounds__(256) void k_bcr_bwd(BaDev d, BcrDev q, BigDev b, int sh, int Mq, int dev_lm)
{
  __shared__ double sX[2 * M];
  __shared__ double sPart[4][M];
  if (d.scal[SC_SOLVE_OK] == 0.0 || (dev_lm && d.scal[SC_STOP] != 0.0)) return;
  const int t = threadIdx.x, mm = M * M;
  int j, l, r;
  bcr_who(sh, Mq, blockIdx.x, j, l, r);
  const bool both = l >= 0 && l == r;
  const bool use_r = r >= 0 && !both;
  constexpr int Q = M / 4;                                             // terms of U_l (and of U_r) per thread: four threads per row
  const int k = t >> 2, part = t & 3;
  double ul[Q] = {}, ur[Q] = {}, lrow[M] = {}, yv = 0.0, xn = 0.0;
  if (t < 2 * M) xn = t < M ? (l >= 0 ? q.X[(size_t)l * M + t] : 0.0) : (use_r ? q.X[(size_t)r * M + (t - M)] : 0.0);
  if (k < M) {
    const double* pl = q.Ul + (size_t)j * mm + (size_t)k * M + part;
    const double* pr = q.Ur + (size_t)j * mm + (size_t)k * M + part;
#pragma unroll
    for (int i = 0; i < Q; ++i) { ul[i] = pl[4 * i]; ur[i] = pr[4 * i]; }
  }
  if (t < M) {
    yv = q.Y[(size_t)j * M + t];
    const double2* pL = reinterpret_cast<const double2*>(q.Lf + (size_t)j * mm + (size_t)t * M);   // row t = L[.][t], 16-byte aligned (M even)
#pragma unroll
    for (int i = 0; i < M / 2; ++i) { const double2 v2 = pL[i]; lrow[2 * i] = v2.x; lrow[2 * i + 1] = v2.y; }
  }
  if (t < 2 * M) sX[t] = xn;
  __syncthreads();
  if (k < M) {
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < Q; ++i) acc = fma(ul[i], sX[part + 4 * i], acc);
#pragma unroll
    for (int i = 0; i < Q; ++i) acc = fma(ur[i], sX[M + part + 4 * i], acc);
    sPart[part][k] = acc;
  }
  __syncthreads();
  if (t >= 64) return;
  double v = 0.0;
  if (t < M) v = yv - (((sPart[0][t] + sPart[1][t]) + sPart[2][t]) + sPart[3][t]);
  // L^T x = v, last unknown first: lrow[k] = L[k][t]; lane t keeps its own running right-hand side
  double xi = 0.0;
#pragma unroll
  for (int kk = M - 1; kk >= 0; --kk) {
    const double vk = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), kk), __builtin_amdgcn_readlane(__double2loint(v), kk));
    const double dk = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(lrow[kk]), kk), __builtin_amdgcn_readlane(__double2loint(lrow[kk]), kk));
    const double xk = vk * dk;                                          // (the diagonal of Lf holds 1 / L_kk)
    if (t == kk) xi = xk;
    v = fma(-lrow[kk], xk, v);                                          // (lanes >= kk: values nobody reads)
  }
  if (t < M) {
    q.X[(size_t)j * M + t] = xi;
    const int pa = t / 6, p = q.p0[j] + pa;
    if (p < q.p0[j + 1]) b.x[(size_t)p * 6 + (t - 6 * pa)] = xi;
  }
}
