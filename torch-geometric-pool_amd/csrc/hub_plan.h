// The device side of a host hub plan (tgp/kernels.py: build_hub_plan), shared by the hub routes (hub_walk.hip,
// maxcut_hub.hip): hub_ids [H] ascending, chunk_ptr [H + 1]; chunk c of a hub covers entries b + c C ..
// min(b + (c + 1) C, e) of its group [b, e), C = HW_CHUNK: a function of the group alone.  Every file that walks chunks
// cuts them through hub_item, so they all cut exactly as the plan counted.
#pragma once

#include "common.h"
#include "edge_walk.h"

namespace tgp {

#ifndef TGP_HW_CHUNK
#define TGP_HW_CHUNK 256  // -DTGP_HW_CHUNK=...: the builds the chunk-size measurement of DESIGN 4.20 compared
#endif
constexpr int HW_CHUNK = TGP_HW_CHUNK;  // entries of a chunk (DESIGN 4.20 says what decided it)
static_assert(HW_CHUNK >= 64 && HW_CHUNK % 64 == 0, "a chunk is whole rounds of a wave");
constexpr int HW_TAIL_SLOTS = 16;

namespace {

struct HubPlan {
  const int32_t* hub_ids;    // [H] ascending
  const int32_t* chunk_ptr;  // [H + 1]
  int H, T;                  // hubs, chunks of all hubs (= records of the workspace)
};

struct HubItem {
  int64_t node, b, e;  // the hub node and the entries of this chunk
  int first, count;    // the hub's records: first .. first + count of the workspace
  int hub;             // its place in hub_ids
};

// the records of hub h, clamped to [0, T]
__device__ __forceinline__ bool hub_of(const HubPlan& pl, int h, int64_t n, HubItem* it) {
  const int64_t node = pl.hub_ids[h];
  int first = pl.chunk_ptr[h], last = pl.chunk_ptr[h + 1];
  if (first < 0) first = 0;
  if (last > pl.T) last = pl.T;
  it->node = node;
  it->hub = h;
  it->first = first;
  it->count = last > first ? last - first : 0;
  return static_cast<uint64_t>(node) < static_cast<uint64_t>(n);
}

// wave item w -> (hub, chunk) by bisection of chunk_ptr; false for an item that owns nothing
__device__ __forceinline__ bool hub_item(const HubPlan& pl, const int32_t* __restrict__ grp_ptr, int64_t w, int64_t n,
                                         int64_t E, HubItem* it) {
  int lo = 0, hi = pl.H;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pl.chunk_ptr[mid] <= w) lo = mid;
    else hi = mid;
  }
  if (!hub_of(pl, lo, n, it)) return false;
  const int64_t c = w - it->first;
  if (c < 0 || c >= it->count) return false;
  const Group g = group_of(grp_ptr, it->node, E);
  it->b = g.b + c * HW_CHUNK;
  it->e = it->b + HW_CHUNK < g.e ? it->b + HW_CHUNK : g.e;
  return true;
}

}  // namespace
}  // namespace tgp
