// ssvio_amd/csrc/orb_ws.hpp -- device-side view and per-ctx workspace of the ORB / stereo front-end.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "ctx.hpp"

namespace ssxorb {

constexpr int MAX_LEVELS = 8;
// candidates kept per grid cell.  No two survivors of the strict 3x3 NMS touch, so a cell whose FAST interior is iw x ih px keeps at
// most ceil(iw / 2) * ceil(ih / 2): 256 for a 31 x 32 interior.  The grid allows more -- a cell is 30 .. 59 px a side (wCell =
// ceil(width / floor(width / 30)): at most 45 once a level has two columns of cells, up to 59 with one), i.e. up to 30 * 30 -- but
// images stay below 256 (uniform noise at threshold 0: 194 in a 32 x 44 cell, where the bound is 352; isolated pixels every 4 px, the
// densest lattice of corners that do not suppress each other: one per 16 px, at most 225 in the largest cell).  A cell with more
// raises the candidate bit of the status word (value 1) and the call returns SSX_ERR_CAPACITY: nothing is dropped silently.
constexpr int CELL_CAP = 256;
constexpr int CAND_CAP = 16384;    // candidates per (image, level) the octree keeps in LDS (16 per thread)
constexpr int CAND_CAP_BIG = 65535;  // ... and in global scratch for larger images (64 per thread): the most a 16-bit node count holds
constexpr int SEL_CAP = 4096;      // selected keypoints per (image, level)
constexpr int EDGE_THRESHOLD = 19; // orbextractor.cpp:13
constexpr int OCT_THREADS = 1024;
constexpr int OCT_MAX_ROOTS = 64;  // root nodes (nIni, a level's width / height rounded) of k_octree: one wave places them; more is refused by the plan
// key slots behind a candidate capacity: whole slots-per-thread rows of the [slot][thread] layout (also keeps what follows the keys aligned)
constexpr int oct_key_slots(int cap) { return (cap + OCT_THREADS - 1) / OCT_THREADS * OCT_THREADS; }

struct Cell {
  int16_t x0, y0;   // ROI origin in the level image
  int16_t w, h;     // ROI size (cell + 6, clipped)
  int16_t ox, oy;   // j*wCell, i*hCell added to ROI-local coordinates (orbextractor.cpp:816-817)
  int16_t level, pad;
};

// octree (octree.hip): OCT_NODE_BYTES per node-table entry; the tables live in LDS, or in a per (image, level) global
// scratch block when the per-level budget is too large for LDS (OrbDev::oct_global_tab).
constexpr int OCT_NODE_BYTES = 50;
constexpr int OCT_LDS_BUDGET = 158 * 1024;   // dynamic LDS the octree workgroup may ask for (160 KB per CU, ~1 KB static)

struct ResizeQuad;

struct OrbDev {
  // geometry
  int I;                         // images in the batch
  int nlevels;
  int lvl_rows[MAX_LEVELS], lvl_cols[MAX_LEVELS], lvl_pitch[MAX_LEVELS];
  size_t lvl_off[MAX_LEVELS];    // byte offset of a level inside one image's pyramid
  size_t pyr_bytes;              // bytes of one image's pyramid
  float scale[MAX_LEVELS];       // mvScaleFactor
  int feat[MAX_LEVELS];          // mnFeaturesPerLevel (or nfeatures for the single-level Detect)
  int lvl_cell0[MAX_LEVELS + 1]; // first cell of each level
  int n_cells;
  int ini_th, min_th;
  int has_mask;
  int detect_only;               // ORBextractor::Detect: level 0 only, no orientation / descriptors
  int out_cap;                   // keypoints per image in the output arrays
  int fast_tile_bytes;           // LDS bytes of one ROI tile (max over cells, pitch rounded to 4)
  int fast_lds_per_wave;         // image tile + score tile + compaction list
  int gauss_tile0[MAX_LEVELS + 1]; // first blur tile RUN of each level (one launch covers all levels)
  int gauss_run;                 // tiles per workgroup of k_gauss7: 4 for a batch (the next tile's loads fly during a tile's passes), 1 for a
                                 // frame or two (the chip is empty: every tile its own workgroup is the shorter chain)
  int rs_xoff[MAX_LEVELS], rs_yoff[MAX_LEVELS];   // first row of level l in the cv::resize tables below
  int rs_wide8[MAX_LEVELS];      // every quad of the level reads <= 8 consecutive source bytes
  // buffers
  const Cell* cells;
  const ResizeQuad* rs_xtab;     // per quad of destination columns (levels concatenated), see k_resize
  const uint2* rs_ytab;          // per destination row:    sy0 | sy1<<16, b0 | b1<<16
  uint8_t* pyr;                  // [I][pyr_bytes]
  uint8_t* maskpyr;              // [I][pyr_bytes] (only when has_mask)
  uint8_t* blur;                 // [I][pyr_bytes]
  int* cell_count;               // [I][n_cells]
  uint32_t* cell_cand;           // [I][n_cells][CELL_CAP]   x | y<<12 | score<<24 (relative to the 16-px border)
  uint8_t* oct;                  // [I][nlevels][oct_stride] (only with oct_global_tab)
  size_t oct_stride;
  int oct_max_cells;             // most grid cells on one level (cell-prefix array in LDS)
  int oct_cand_cap;              // candidates per (image, level): CAND_CAP (keys in LDS) or CAND_CAP_BIG (keys in global scratch)
  int oct_global_keys;
  int oct_ln;                    // node-table capacity: max(N, 256) + 8 over the levels (N = per-level budget)
  int oct_global_tab;            // node tables in global scratch (budgets too large for LDS)
  int* lvl_ncand;                // [I][nlevels]
  int* sel_count;                // [I][nlevels]
  uint32_t* sel;                 // [I][nlevels][SEL_CAP] packed like cell_cand
  float* sel_angle;              // [I][nlevels][SEL_CAP]
  int* status;                   // [I] bit0: candidate overflow, bit1: node overflow, bit2: output overflow
  // outputs
  uint8_t* out_kps;              // [I][out_cap] x 28 bytes (ssx_keypoint)
  uint8_t* out_desc;             // [I][out_cap][32]
  int* out_n;                    // [I]
};

// what a plan depends on: a call whose key equals the workspace's runs on the plan it finds
struct PlanKey {
  int rows = 0, cols = 0, I = 0, nlevels = 0, nfeatures = 0, ini_th = 0, min_th = 0, has_mask = 0, detect_only = 0;   // nlevels AS PLANNED: 1 for ORBextractor::Detect
  float scale_factor = 0.f;
  bool operator==(const PlanKey& o) const {
    return rows == o.rows && cols == o.cols && I == o.I && nlevels == o.nlevels && nfeatures == o.nfeatures && ini_th == o.ini_th && min_th == o.min_th &&
           has_mask == o.has_mask && detect_only == o.detect_only && scale_factor == o.scale_factor;
  }
  // a detect-with-mask plan of this shape and these thresholds for at least n images (ssx_orb_detect_boxes_batch: a smaller batch runs on it)
  bool detects_masked(int rows_, int cols_, const ssx_orb_params& prm, int n) const {
    return detect_only && has_mask && rows == rows_ && cols == cols_ && nfeatures == prm.nfeatures && ini_th == prm.ini_th_fast && min_th == prm.min_th_fast && I >= n;
  }
};

// a FIFO of at most two slots, 0 and 1: the oldest entry sits in `first`, the next push goes to the other one (while count < 2)
struct Ring2 {
  int first = 0, count = 0;
  int push_slot() const { return (first + count) & 1; }
  int pop() { const int s = first; first ^= 1; --count; return s; }
};

void launch_octree(const OrbDev& o, hipStream_t s);   // octree.hip

}  // namespace ssxorb

// host-side plan + buffers (one per ctx; re-planned when the key changes)
struct OrbWorkspace {
  DevBuf arena;        // pyramids, candidates, octree scratch, outputs
  DevBuf input;        // uploaded host images (host-pointer entry points)
  DevBuf stereo;       // match / triangulation results of the batch entry points
  HostBuf stage;       // pinned staging
  HostBuf fetch;       // pinned: everything ssx_stereo_frame returns, fetched with ONE synchronisation
  ssxorb::PlanKey key; ssxorb::OrbDev dev{}; bool planned = false;   // the plan in force, and what it was made for
  // batch parameters (ssx_stereo_batch_dev / _run -> _enqueue / _fetch)
  const uint8_t* batch_imgs = nullptr;
  int batch_pairs = 0, batch_stride = 0;
  ssx_orb_params batch_orb{};
  ssx_match_params batch_mp{};
  ssx_stereo_rig batch_rig{};
  // stereo result views inside `stereo`
  int *match_idx = nullptr, *match_dist = nullptr, *pair_counts = nullptr;   // pair_counts: [pairs][4]
  double* xyz = nullptr;
  uint8_t* tri_ok = nullptr;
  // upload ring (ssx_stereo_batch_upload -> _run): two device buffers filled from the host on a copy stream of their own (batch k + 1 crosses PCIe while
  // batch k is processed).  Per slot: the buffer, the events "uploaded" and "level 0 of the batch that used the buffer is staged" (pending?), the batch's shape
  struct Upload { DevBuf buf; hipEvent_t ev_up = nullptr, ev_free = nullptr; bool free_pending = false; int pairs = 0, stride = 0, rows = 0, cols = 0; } up[2];
  ssxorb::Ring2 up_ring;        // uploaded batches waiting for ssx_stereo_batch_run
  hipStream_t copy_stream = nullptr;
  // counts ring (ssx_stereo_batch_run -> _counts).  Per slot: the event "the counts are in counts_pinned", the batch size, the run's status (a failed run owns a slot too)
  struct Counts { hipEvent_t ev = nullptr; int pairs = 0; ssx_status fail = SSX_OK; } cnt[2];
  ssxorb::Ring2 cnt_ring;       // batches that were run and not collected yet
  HostBuf counts_pinned;        // per slot: [pairs][4] counts + [2 pairs] status words
};

namespace ssxorb {
OrbWorkspace* get_ws(ssx_ctx* ctx);
// plan (allocate + upload the cell and resize tables) for I images of rows x cols; returns SSX_OK or an error
ssx_status plan(ssx_ctx* ctx, int rows, int cols, int I, const ssx_orb_params& prm, bool has_mask, bool detect_only);
// stage level 0 from a device / pinned buffer [I][rows][stride]; the masks likewise when a mask buffer is given
ssx_status stage_level0(ssx_ctx* ctx, const uint8_t* imgs_dev, int stride, size_t img_bytes, const uint8_t* masks_dev, int mask_stride, size_t mask_bytes);
// run the extraction pipeline on level-0 images already placed in the pyramid buffers
ssx_status run_pipeline(ssx_ctx* ctx);
// download the keypoints / descriptors of one image of the last run (synchronises the stream)
ssx_status fetch_image(ssx_ctx* ctx, int image, int cap, ssx_keypoint* kps_out, uint8_t* desc_out, int32_t* n);
// the brute-force matcher k_bf_match (stereo.hip) on device arrays: idx[i] / dist[i] = nearest of the nt <= 65535 train descriptors to query i
// (ssx_bf_match's launch; the keyframe database matches through launch_bf_match_jobs, kf_batch.hpp)
void launch_bf_match(hipStream_t stream, const uint8_t* dq, int nq, const uint8_t* dt, int nt, int* idx, int* dist);
// what describe_enqueue leaves on the device: per input keypoint the output keypoint and descriptor (valid where keep), inside the block at
// `base` of `total` bytes; and what it issued: launches, synchronisations (a new plan's two), bytes sent up
struct Described {
  char* base = nullptr; size_t total = 0;
  const ssx_keypoint* kps = nullptr; const uint8_t* desc = nullptr; const uint8_t* keep = nullptr;
  int n_in = 0, launches = 0, syncs = 0;
  size_t bytes_up = 0;
};
// ScreenAndComputeKPsParams + CalcDescriptors of `kps` on a host image, enqueued on the ctx stream (orb.hip).  levels > 0: every keypoint is
// replicated over that many pyramid levels first (octave = level, response = -1, class_id = its index); levels == 0: taken as they are
ssx_status describe_enqueue(ssx_ctx* ctx, const uint8_t* img, int stride, int rows, int cols, const ssx_orb_params& prm, const ssx_keypoint* kps, int n_kps,
                            int levels, Described* out);
// rows of `cols` bytes from the caller's pitch to the staging copy's
inline void copy_rows(uint8_t* dst, size_t dst_pitch, const uint8_t* src, size_t src_pitch, int rows, int cols)
{
  for (int y = 0; y < rows; ++y) memcpy(dst + (size_t)y * dst_pitch, src + (size_t)y * src_pitch, cols);
}
}  // namespace ssxorb
