// ssvio_amd/csrc/voc.hpp -- the vocabulary object and the launch of its tree descent, for voc.hip and the keyframe step of loop.hip.
#pragma once
#include "ctx.hpp"

struct ssx_vocabulary {
  ssx_ctx* ctx = nullptr;
  int k = 0, L = 0, scoring = 0, weighting = 0, n_nodes = 0, n_words = 0;
  DevBuf arena, io;
  HostBuf stage;
  const uint8_t* d_desc = nullptr;      // [n_nodes][32]
  const double* d_weight = nullptr;     // [n_nodes]
  const int32_t* d_child_ptr = nullptr; // [n_nodes + 1]
  const int32_t* d_child = nullptr;     // [n_nodes - 1] children of every node, id order
  const int32_t* d_word = nullptr;      // [n_nodes] word id of a leaf, -1 otherwise
};

namespace ssxvoc {
// k_voc_words (voc.hip) on device arrays: word_out[f] / weight_out[f] = the leaf of descriptor f (-1 / 0 with an empty vocabulary), for the
// first n descriptors; n = *n_dev when n_dev is given (n_bound >= that count sizes the grid), else n_bound.  Needs v->n_nodes >= 1.
void launch_words(hipStream_t stream, const ssx_vocabulary* v, const uint8_t* feat, int n_bound, const int32_t* n_dev, int32_t* word_out, double* weight_out);
}  // namespace ssxvoc
