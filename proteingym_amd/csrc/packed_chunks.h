// Packed rows of attention_prefix.hip's launches (PoET, ESM-IF1): the (segment, tile) lists of a launch and the rule that cuts a batch of
// sequences into workspace chunks.  Host integer logic only -- no HIP call, no device type -- so a plain C++ program can include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace pgmi {

// The segments of one launch, on the host and (after model.h upload_plan) on the device: segment b = packed rows seg_off[b] ..
// seg_off[b + 1] - 1, and one (segment, tile) entry per 32 query rows of a segment.
struct SegPlan {
    std::vector<int32_t> seg_off, ent_seg, ent_tile;
    int32_t *d_seg_off = nullptr, *d_ent_seg = nullptr, *d_ent_tile = nullptr;
    int n_seg() const { return (int)seg_off.size() - 1; }
    int n_ent() const { return (int)ent_seg.size(); }
    void add(int len) {
        if (seg_off.empty()) seg_off.push_back(0);
        const int b = n_seg();
        for (int j = 0; j * 32 < len; ++j) { ent_seg.push_back(b); ent_tile.push_back(j); }
        seg_off.push_back(seg_off.back() + len);
    }
};

// The padded key rows the own-segment planes of a workspace of max_rows rows hold: whole 32-key tiles.
inline size_t own_pitch(int max_rows) { return (size_t)max_rows / 32 * 32; }

// One chunk of a batch: sequences [b0, b1) as `rows` packed rows, plan.seg_off[b - b0] = the first row of sequence b.
struct PackedChunk {
    int b1 = 0, rows = 0;
    SegPlan plan;
};

// The chunk that starts at sequence b0 of B.  The model reads n = lens[b] (drop_last: lens[b] - 1, the inputs of a log-likelihood) rows
// of sequence b.  Sequences are taken while the packed rows fit the workspace (rows + n <= max_rows) and the key rows, every sequence
// padded to whole 32-key tiles, fit the own-segment planes (padded + roundup(n, 32) <= pitch); same_length: and while lens[b] ==
// lens[b0] (a dense B x T attention takes one length per launch).  b1 == b0: sequence b0 alone does not fit, the caller's error.
inline PackedChunk pack_chunk(const int32_t* lens, int b0, int B, bool drop_last, bool same_length, int max_rows, size_t pitch) {
    PackedChunk c;
    size_t rows = 0, padded = 0;
    for (c.b1 = b0; c.b1 < B; ++c.b1) {
        const int n = lens[c.b1] - (drop_last ? 1 : 0);
        const size_t pad = ((size_t)n + 31) / 32 * 32;
        if (same_length && lens[c.b1] != lens[b0]) break;
        if (rows + n > (size_t)max_rows || padded + pad > pitch) break;
        c.plan.add(n);
        rows += n; padded += pad;
    }
    c.rows = (int)rows;
    return c;
}

}  // namespace pgmi
