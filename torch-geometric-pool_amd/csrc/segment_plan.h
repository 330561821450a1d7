// What the fp32 segment readout (segment_aggr.hip) and its 16-bit storage form (sparse_half.hip) must agree on for
// their results to have the same bits: how a batch is cut into row chunks, and how many runs the fold adds them in.
#pragma once
#include <stdint.h>

namespace tgp {

constexpr int SA_FOLD_PARTS = 64;  // split route: runs of consecutive chunk records the fold kernel adds per feature

// rows per chunk and chunks per segment; n_chunks == 1: no workspace, the items write the output themselves
void sa_plan(int64_t G, int64_t F, int64_t max_len, int64_t* chunk, int64_t* n_chunks);

}  // namespace tgp
