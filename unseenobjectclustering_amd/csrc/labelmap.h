// The label map, once: what every stage that reads one shares.  How many ids there are and which raw
// label is which id.  The wave-level pieces these stages use with it (for_each_wave_key, the reductions, lane_rank) are
// common.h's; the table grid is grid.h's, which builds on this file.
#pragma once
#include "common.h"

namespace uoc {

constexpr int NUM_IDS = 128;  // ids 0..127; 1..127 are objects

static_assert(NUM_IDS == UOC_MAX_SEEDS, "a label is a seed's number: include/uoc_hip.h");

// Three readings of a raw label, on purpose three functions.
//   obj_id       1..127 is that object, anything else (negatives included) is background, id 0: a table has a row 0
//   obj_key      the same rule for a wave-group key: background is -1, no key, and takes no part
//   label_row    0..127 is that row, anything else is -1.  confidence.hip alone: it summarises a value map per label and
//                the background's values are a row of its table like any other, so label 0 is a key there
__device__ __forceinline__ int obj_id(int l) { return ((unsigned)(l - 1) < (unsigned)(NUM_IDS - 1)) ? l : 0; }
__device__ __forceinline__ int obj_key(int l) { return ((unsigned)(l - 1) < (unsigned)(NUM_IDS - 1)) ? l : -1; }
__device__ __forceinline__ int label_row(int l) { return ((unsigned)l < (unsigned)NUM_IDS) ? l : -1; }

// The depth of a pixel in whole millimetres as relations.hip and identity.hip read it: -1 of an invalid one (NaN fails
// both comparisons).
__device__ __forceinline__ int depth_mm(float z) { return (z > 0.0f && z <= 65.0f) ? (int)rintf(z * 1000.0f) : -1; }

}  // namespace uoc
