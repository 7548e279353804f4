// greb_gram.h -- host interface of the covariance output (greb_gram.hip): the member-by-member Gram matrices of the records
// of x[n_members][n_records][len], one matrix per block of records.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace greb {

constexpr int kGramTile = 64;     // members along each side of the tile of G one workgroup of gram_tile_kernel owns
constexpr int kGramOwn = 4;       // ... of which a lane owns 4 x 4: 16 fp64 accumulators
constexpr int kGramThreads = 256; // (kGramTile / kGramOwn)^2
constexpr int kGramChunk = 32;    // elements of every member row of a tile staged through LDS at a time
constexpr int kGramMaxUsed = 1024;
constexpr int kGramMaxBlocks = 16;

// The plan's tables on the device.  The used members in ascending member index: member[k], control[k] beside it (null: no
// control map).  The records that enter a matrix, sorted by block and ascending inside each: record[q], block b's being
// q = offs[b] ... offs[b + 1] - 1.  partial: the per-record matrices [n_listed][n_used][n_used] between the two launches.
struct GramTables {
  const int* member;  // [n_used]
  const int* control; // [n_used] or null
  const int* record;  // [n_listed]
  const int* offs;    // [n_blocks + 1]
  const float* scale; // [len] or null
  double* partial;    // [n_listed][n_used][n_used]
  int n_used, n_listed, n_blocks, n_records;
};

// G[n_blocks][n_used][n_used] of x[n_members][n_records][len]: gram_tile_kernel, grid (tiles of the lower triangle,
// n_listed), then gram_sum_kernel, grid (ceil(n_used^2 / 256), n_blocks)
hipError_t launch_gram(const float* x, size_t len, const GramTables& t, double* G, hipStream_t s);

} // namespace greb
