// ssvio_amd/csrc/kf_batch.hpp -- the jobs of the keyframe database's chain (loop.hip): a device table of them for
// ssx_kfdb_process_keyframe_batch and ssx_kfdb_relocalize_query_batch, one by value as a kernel argument for the single calls; and the job-indexed launches the chain borrows
// from orb.hip (pyramid, blur, k_describe_at), voc.hip (k_voc_words) and stereo.hip (k_bf_match).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ctx.hpp"
#include "voc.hpp"

// One keyframe step of the call.  Pyramid keypoint k of job j is entry kp0 + k of every array that is concatenated over the jobs (the
// replicated keypoints, k_describe_at's outputs, the per-feature words and weights); the image of job j is image j of the ORB plan.
struct KfJobDev {
  int32_t kp0, n_in;              // first pyramid keypoint and their number (features x levels)
  int32_t n_elig;                 // stored keyframes k_kfdb_score scores (and k_kfdb_topk ranks), the one this job commits included; 0: the job's workgroups exit
  int32_t commit;                 // != 0: k_kfdb_commit moves c_* into c_blob first
  // the pending arrays in the database's own buffer, each of capacity n_in
  ssx_keypoint* p_kps; uint8_t* p_desc; int32_t* p_cls; int32_t* p_ids; double* p_vals;
  unsigned long long* bow_keys;   // global sort scratch of k_kf_bow (n_in > 4096), else null
  const char* arena; const void* rows; double* scores;   // the database and this job's scores
  // the commit: the previous pending arrays, their blob and their row
  const int32_t* c_ids; const double* c_vals; const int32_t* c_cls; const uint8_t* c_desc;
  char* c_blob; void* c_row_out;
  int64_t c_off; int32_t c_n_bow, c_n_desc;
};
static_assert(sizeof(KfJobDev) == 152, "the job table is counted against the call's upload budget");

// One found loop of the call: MatchFeatures of a job's pending keyframe (train) against its winner's stored descriptors (query)
struct KfMatchJob {
  const uint8_t* loop_desc; const int32_t* loop_cls; const uint8_t* cur_desc; const int32_t* cur_cls;
  int* idx; int* dist; unsigned long long* keys;   // scratch: nl, nl, and the global sort scratch (nl > 4096) or null
  int32_t* hdr; int32_t* pairs;                    // mapped pinned memory: (pair count, minimum distance), the pairs
  int32_t nl, n_cur;
};
static_assert(sizeof(KfMatchJob) == 80, "the match table is counted against the call's upload budget");

namespace ssxorb {
struct DescribeJob { const uint8_t* img; const ssx_keypoint* feats; int n_feats; };
// One block on the device and (pinned) on the host: [the caller's `extra` bytes | image pointers | replicated keypoints | images unless
// they are read in place] goes up in ONE copy by describe_batch_launch; [keypoints out | descriptors | keep flags], concatenated over the
// jobs, stay on the device.
struct DescribedBatch {
  char* host_extra = nullptr; char* dev_extra = nullptr;
  const ssx_keypoint* kps = nullptr; const uint8_t* desc = nullptr; const uint8_t* keep = nullptr;
  int launches = 0, syncs = 0;
  size_t bytes_up = 0;
  // (between prepare and launch)
  size_t o_ptr = 0, o_in = 0; int stride = 0, total = 0;
};
// plan for the next power of two of n images (a plan of the same shape for more stays), reserve and fill the block; nothing is enqueued
ssx_status describe_batch_prepare(ssx_ctx* ctx, int n, const DescribeJob* jobs, int stride, int rows, int cols, const ssx_orb_params& prm, int levels,
                                  bool images_on_device, size_t extra_bytes, DescribedBatch* out);
// the copy, level 0, pyramid, blur and k_describe_at of all jobs; `table` = the job table inside dev_extra, max_n_in the largest n_in
ssx_status describe_batch_launch(ssx_ctx* ctx, int n, const KfJobDev* table, int max_n_in, DescribedBatch* io);
// k_bf_match of every match job in one launch (stereo.hip); max_nl = the largest nl.  jobs == null (n_jobs == 1): the job is `one`, passed as a
// kernel argument
void launch_bf_match_jobs(hipStream_t stream, const KfMatchJob* jobs, const KfMatchJob& one, int n_jobs, int max_nl);
}  // namespace ssxorb

namespace ssxvoc {
// k_voc_words over the concatenated bound `total`: entry t belongs to the job with kp0 <= t < kp0 + n_in, is its descriptor t - kp0 in p_desc
// and exists while t - kp0 < counts[count_stride * job]
void launch_words_jobs(hipStream_t stream, const ssx_vocabulary* v, const KfJobDev* jobs, int n_jobs, const int32_t* counts, int count_stride, int total,
                       int32_t* word_out, double* weight_out);
}  // namespace ssxvoc
