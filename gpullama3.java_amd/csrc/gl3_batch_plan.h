// gl3_batch_plan.h — the host-side plan of a mixed batched step (gl3_forward_batch): plain C++, no HIP, so the CPU suite checks it
// through gl3_debug_batch_plan.
//
// The n rows of a step are a list of RUNS: a run is a maximal stretch of consecutive rows with the same sequence id, at consecutive
// ascending positions; a sequence id belongs to at most one run.  A run of one row is a decode row, a longer one a prompt chunk
// (which may start anywhere: a continuation chunk).  From (seq_ids, positions, want_logits, n) the plan holds
//   runs      {first row, rows, sequence, position of the first row}
//   tiles     the same record for at most BP_TILE_ROWS rows: the unit of work of the run-table form of the one-launch prefill
//             attention (gl3_prefill_attn.h).  A tile never crosses a run boundary; tiles are ordered deepest last position first,
//             as the one-sequence kernels launch their heaviest tiles first (the triangular work profile leaves no tail)
//   out_rows  the rows whose logits the caller wants, in row order (want_logits == NULL: the last row of every run)
// batch_plan_split then divides the tiles by depth: a tile whose last position is <= fused_max_pos keeps its score rows in LDS (SHALLOW, the
// one-launch table form); the rows of the others (DEEP) are cut again, into records of at most BP_DEEP_ROWS rows for the table form of the
// long-context kernels (scores -> pf_softmax_rows_kernel -> weighted V sum over score rows in HBM).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace gl3 {

constexpr int BP_TILE_ROWS = 8;      // = FA_TB (gl3_prefill.hip asserts it)
constexpr int BP_DEEP_ROWS = 16;     // = PA_TB = SCM_TB = PVM_TB (gl3_prefill.hip asserts it)

struct BatchSpan { int32_t row0, rows, seq, pos0; };      // a run or a tile; 16 bytes: the kernels read a tile as one int4

struct BatchPlan {
    std::vector<BatchSpan> runs, tiles;
    std::vector<int32_t> out_rows;
    int max_pos = 0;                 // deepest row of the step
    bool single_rows = true;         // every run is one row: the step has the shape of a static-batched decode step
};

// Returns nullptr and fills bp, or the reason the step is refused (nothing of bp is to be used then).
// capacity = rows a step may have (max_batch), n_seqs / ctx = the plan's sequence slots and context length.
inline const char* batch_plan_build(const int32_t* seq_ids, const int32_t* positions, const int8_t* want_logits, int n, int n_seqs, int ctx,
                                    int capacity, BatchPlan& bp) {
    if (!seq_ids || !positions || n <= 0) return "bad batch arrays";
    if (n > capacity) return "batch larger than max_batch";
    bp.runs.clear(); bp.tiles.clear(); bp.out_rows.clear();
    bp.max_pos = 0; bp.single_rows = true;
    std::vector<char> seen((size_t)(n_seqs > 0 ? n_seqs : 0), 0);
    for (int i = 0; i < n; ++i) {
        if (seq_ids[i] < 0 || seq_ids[i] >= n_seqs) return "sequence id out of range";
        if (positions[i] < 0) return "position outside the KV cache (context length)";
        if (i > 0 && seq_ids[i] == seq_ids[i - 1]) {
            if (positions[i] != positions[i - 1] + 1) return "positions inside a run must be consecutive and ascending";
            ++bp.runs.back().rows;
        } else {
            if (seen[seq_ids[i]]) return "a sequence id belongs to at most one run of a step";
            seen[seq_ids[i]] = 1;
            bp.runs.push_back({i, 1, seq_ids[i], positions[i]});
        }
        if (positions[i] >= ctx) return "position outside the KV cache (context length)";      // also: a run ending past ctx
        bp.max_pos = std::max(bp.max_pos, (int)positions[i]);
    }
    for (const BatchSpan& r : bp.runs) {
        if (r.rows > 1) bp.single_rows = false;
        for (int o = 0; o < r.rows; o += BP_TILE_ROWS)
            bp.tiles.push_back({r.row0 + o, std::min(BP_TILE_ROWS, r.rows - o), r.seq, r.pos0 + o});
        if (!want_logits) bp.out_rows.push_back(r.row0 + r.rows - 1);
    }
    if (want_logits)
        for (int i = 0; i < n; ++i) if (want_logits[i]) bp.out_rows.push_back(i);
    std::stable_sort(bp.tiles.begin(), bp.tiles.end(),
                     [](const BatchSpan& a, const BatchSpan& b) { return a.pos0 + a.rows > b.pos0 + b.rows; });
    return nullptr;
}

// The tiles of a built plan by depth.  fused_max_pos = the largest last position a tile may have and still fit the one-launch table form (-1:
// the shape has none; >= ctx: every tile is shallow and `shallow` is bp.tiles unchanged).
//   shallow    the tiles with last position <= fused_max_pos, in bp.tiles' order (deepest last position first).  Positions ascend inside a
//              run, so they are a prefix of their run
//   deep       records {first row, rows <= BP_DEEP_ROWS, sequence, position of the first row} cut from each run's deep suffix, starting at its
//              first deep row, never across a run boundary; deepest last position first (stable).  A deep decode row is a one-row record
//   deep_rows  the step rows of the deep records, ascending: the rows pf_softmax_rows_kernel serves
struct BatchSplit {
    std::vector<BatchSpan> shallow, deep;
    std::vector<int32_t> deep_rows;
    int shallow_max_pos = -1;        // last position of the deepest shallow tile (-1: none)
};
inline void batch_plan_split(const BatchPlan& bp, int fused_max_pos, BatchSplit& sp) {
    sp.shallow.clear(); sp.deep.clear(); sp.deep_rows.clear(); sp.shallow_max_pos = -1;
    for (const BatchSpan& t : bp.tiles)
        if (t.pos0 + t.rows - 1 <= fused_max_pos) { sp.shallow.push_back(t); sp.shallow_max_pos = std::max(sp.shallow_max_pos, t.pos0 + t.rows - 1); }
    for (const BatchSpan& r : bp.runs) {
        int o = 0;                   // rows of the run's shallow prefix: whole tiles whose last position is within the limit
        while (o < r.rows && r.pos0 + std::min(o + BP_TILE_ROWS, r.rows) - 1 <= fused_max_pos) o = std::min(o + BP_TILE_ROWS, r.rows);
        for (; o < r.rows; o += BP_DEEP_ROWS) {
            const int rows = std::min(BP_DEEP_ROWS, r.rows - o);
            sp.deep.push_back({r.row0 + o, rows, r.seq, r.pos0 + o});
            for (int i = 0; i < rows; ++i) sp.deep_rows.push_back(r.row0 + o + i);      // runs ascend by first row: so does this list
        }
    }
    std::stable_sort(sp.deep.begin(), sp.deep.end(),
                     [](const BatchSpan& a, const BatchSpan& b) { return a.pos0 + a.rows > b.pos0 + b.rows; });
}

}  // namespace gl3
