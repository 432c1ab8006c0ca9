// gl3_chunked.h — the rank-chunked activation layout of tensor-parallel batched steps, shared by its writers and readers
// (gl3_prefill.hip: the layers, the output-row gather, the greedy scan; gl3_sample.hip: the batched sampler and the scorer).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

// Activation layout under tensor parallelism ("rank-chunked"): a [ntok][cols] activation that is produced by row-split
// matrices is kept as [tp][ntok][cols / tp], so every rank's output is one contiguous chunk and the all-gather is in
// place; element j of token b sits at (j / cc) * ntok * cc + b * cc + j % cc with cc = cols / tp (tp = 1: the plain layout).
__device__ __forceinline__ size_t chunked(int b, int j, int cc, int ntok) { return ((size_t)(j / cc) * ntok + b) * cc + (j % cc); }

// How a reader finds the rows of a gathered buffer: element i of row r is at chunked(r, i, cc, nrows).  cc = the row length: plain rows,
// whatever nrows is.  cc is a multiple of 16 in every buffer a plan gathers (gl3_create), so an aligned float4 never straddles two chunks.
struct RowLayout { int cc, nrows; };
