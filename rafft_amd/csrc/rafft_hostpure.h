// rafft_hostpure.h - host helpers that need neither HIP nor the global context: base codes, the dot-bracket parsers, the loop
// that encloses a region, the lane cut of a batch and the row layout of the scoring calls.  Plain C++ (g++ compiles it alone:
// tests/hostcheck/hostpure_check.cpp).  Part of the single translation unit of rafft_api.hip (included there, before the kernels).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace {

// base codes of rafft/utils.py:73-80 (N=0 A=1 C=2 G=3 U=4); bit 3 marks a character outside "AGCUN"
struct BaseCodeTable {
    uint8_t v[256];
    BaseCodeTable() { for (int i = 0; i < 256; i++) v[i] = 8; v['N'] = 0; v['A'] = 1; v['C'] = 2; v['G'] = 3; v['U'] = 4; }
    uint8_t operator[](unsigned char c) const { return v[c]; }
};
static const BaseCodeTable kBaseCode;

// pair table of a plain dot-bracket string (0-based partners, -1 = unpaired); false: malformed
static bool parse_db(const char *db, int L, std::vector<int16_t> &pt)
{
    pt.assign(L, -1);
    std::vector<int> stk;
    for (int i = 0; i < L; i++) {
        if (db[i] == '(') stk.push_back(i);
        else if (db[i] == ')') {
            if (stk.empty()) return false;
            int j = stk.back(); stk.pop_back();
            pt[i] = (int16_t)j; pt[j] = (int16_t)i;
        } else if (db[i] != '.') return false;
    }
    return stk.empty();
}

// the known structure's table as rafft/utils.py:53-67 pairs it: ( and < share a stack, [ has its own; 1-based partners, 0 = unpaired
static bool score_known_table(const char *db, int L, uint16_t *t, int *n_known, std::string &err)
{
    const size_t n = strlen(db);
    if (n != (size_t)L) { err = "known structure of length " + std::to_string(n) + " for a sequence of length " + std::to_string(L); return false; }
    std::vector<int> reg, pk;
    int pairs = 0;
    for (int i = 0; i < L; i++) {
        const char c = db[i];
        t[i] = 0;
        if (c == '(' || c == '<') reg.push_back(i);
        else if (c == '[') pk.push_back(i);
        else if (c == ')' || c == '>' || c == ']') {
            std::vector<int> &stk = c == ']' ? pk : reg;
            if (stk.empty()) { err = std::string("known structure: unmatched '") + c + "' at position " + std::to_string(i); return false; }
            const int j = stk.back(); stk.pop_back();
            t[i] = (uint16_t)(j + 1); t[j] = (uint16_t)(i + 1);
            pairs++;
        } else if (c != '.') { err = std::string("known structure: character '") + c + "' at position " + std::to_string(i); return false; }
    }
    if (!reg.empty() || !pk.empty()) { err = "known structure: unclosed bracket at position " + std::to_string(!reg.empty() ? reg.back() : pk.back()); return false; }
    *n_known = pairs;
    return true;
}

// the loop that encloses a region starting at pos0: the nearest pair (ci, cj) with ci < pos0 < cj (-1, L: the exterior loop),
// and the branch helices hanging in it as (i | j << 16)
struct LoopOf { int ci, cj; std::vector<uint32_t> br; };
static LoopOf enclosing_loop(const std::vector<int16_t> &pt, int pos0)
{
    LoopOf lp{-1, (int)pt.size(), {}};
    for (int x = pos0 - 1, depth = 0; x >= 0; x--) {
        if (pt[x] < 0) continue;
        if (pt[x] < x) { depth++; continue; }
        if (depth > 0) { depth--; continue; }
        if (pt[x] > pos0) { lp.ci = x; lp.cj = pt[x]; break; }
    }
    for (int x = lp.ci + 1; x < lp.cj;) {
        if (pt[x] < 0) { x++; continue; }
        lp.br.push_back((uint32_t)x | ((uint32_t)pt[x] << 16));
        x = pt[x] + 1;
    }
    return lp;
}

struct SeqIn { const char *s; int len; int idx; int bi; const uint8_t *c = nullptr; };   // bi: which member batch of the job the sequence belongs to; c: the bases as codes (encoded at submit, on the caller's thread), or null

// ---- lanes.  Folds are independent, so how the batch is cut cannot change any result.  The number of
// folding steps of a wave is set by its longest sequence, and the steps that only the long ones still need
// are latency-bound and nearly empty (the benchmark set: 24 steps for two 2.9-knt sequences, 12 for the rest).
// So a batch whose few longest sequences stand far out is cut in two jobs: the long tail starts first and runs
// beside the bulk (and beside the bulk of the next batch).  The workspaces of the bulk lane have a stream
// priority of their own, which gives them HW queues of their own - with all streams at one priority the waves
// share the process's four queues and the cut is a loss (17.3 ms against 15.2 for the benchmark batch; with it: 13.3 ms).
// RAFFT_SPLIT (`want`): -1 automatic, 0 never, > 0 cut at that length.  Returns the length to cut at, 0: no cut.
static int split_length(std::vector<int> lens, int want)
{
    if (lens.size() < 32 || want == 0 || (want < 0 && lens.size() >= 16384)) return 0;     // (very large batches amortise the tail anyway)
    if (want > 0) return want;
    // the sequences at least twice as long as the 99th percentile of the batch (leaving room for two)
    std::sort(lens.begin(), lens.end());
    const size_t top = std::max<size_t>(2, lens.size() / 100);
    const int ref = lens[lens.size() - top - 1];
    return lens.back() >= 2 * ref ? 2 * ref : 0;
}

// the jobs of a batch, in starting order: the long tail (lane 0) before the bulk (lane 1) when the cut leaves both, else one
// job - in the bulk lane from 256 sequences.  est: expected survivors per beam slot (~ folding steps in which a slot is
// renewed), grows with length; `cfg_est` > 0 (RAFFT_EST) replaces it
struct LaneJob { int lane; std::vector<SeqIn> seqs; double est; };
static std::vector<LaneJob> cut_lanes(const std::vector<SeqIn> &good, int split_len, double cfg_est)
{
    auto est_of = [&](const std::vector<SeqIn> &v) {
        size_t sl = 0;
        for (auto &sq : v) sl += sq.len;
        return cfg_est > 0 ? cfg_est : 6.0 + (v.empty() ? 0.0 : (double)sl / (double)v.size()) / 100.0;
    };
    std::vector<SeqIn> shorts, longs;
    for (auto &sq : good) (split_len > 0 && sq.len >= split_len ? longs : shorts).push_back(sq);
    std::vector<LaneJob> jobs;
    if (!longs.empty() && !shorts.empty()) {
        jobs.push_back(LaneJob{0, longs, est_of(longs)});
        jobs.push_back(LaneJob{1, shorts, est_of(shorts)});
    } else if (!good.empty())
        jobs.push_back(LaneJob{good.size() >= 256 ? 1 : 0, good, est_of(good)});
    return jobs;
}

struct ScoreSrc { const char *base; size_t bytes; size_t dev_off; };      // a host range of rows that goes to the device as it lies

// rows of every sequence packed into one host buffer (strides kept): rows that lie anywhere in pageable memory
static void score_pack(int n_seq, const int *lens, const int *n_rows, const char *const *rows, const int *stride, const int *pre_status,
                       std::vector<char> &pack, std::vector<unsigned long long> &rows_off)
{
    size_t tot = 0;
    for (int s = 0; s < n_seq; s++) {
        rows_off[s] = tot;
        if (n_rows[s] && !(pre_status && pre_status[s])) tot += (size_t)(n_rows[s] - 1) * stride[s] + lens[s];
    }
    pack.resize(tot);
    for (int s = 0; s < n_seq; s++) {
        const size_t end = s + 1 < n_seq ? rows_off[s + 1] : tot;
        if (end > rows_off[s]) memcpy(pack.data() + rows_off[s], rows[s], end - rows_off[s]);
    }
}

// rows that lie in the chunks [chunk_base[c], + chunk_cap[c]): per chunk, the range its sequences span goes up as one copy, each
// at a multiple of 256 bytes; rows_off[s] is where sequence s's first row lies in the device copy.  false: a range is not in chunks
static bool score_chunk_layout(int n_seq, const int *lens, const int *n_rows, const int *stride, const char *const *rows, size_t nc,
                               const char *const *chunk_base, const size_t *chunk_cap, std::vector<ScoreSrc> &src,
                               std::vector<unsigned long long> &rows_off, size_t &rows_bytes)
{
    std::vector<const char *> lo(nc, nullptr), hi(nc, nullptr);
    std::vector<int> chunk_of(n_seq, -1);
    for (int s = 0; s < n_seq; s++) {
        if (!n_rows[s]) continue;
        const char *a = rows[s], *b = a + (size_t)(n_rows[s] - 1) * stride[s] + lens[s];
        for (size_t c = 0; c < nc && chunk_of[s] < 0; c++)
            if (a >= chunk_base[c] && b <= chunk_base[c] + chunk_cap[c]) chunk_of[s] = (int)c;
        const int c = chunk_of[s];
        if (c < 0) return false;
        if (!lo[c] || a < lo[c]) lo[c] = a;
        if (!hi[c] || b > hi[c]) hi[c] = b;
    }
    std::vector<size_t> dev_off(nc, 0);
    src.clear();
    rows_bytes = 0;
    for (size_t c = 0; c < nc; c++) {
        if (!lo[c]) continue;
        dev_off[c] = rows_bytes;
        src.push_back(ScoreSrc{lo[c], (size_t)(hi[c] - lo[c]), rows_bytes});
        rows_bytes += ((size_t)(hi[c] - lo[c]) + 255) & ~(size_t)255;
    }
    for (int s = 0; s < n_seq; s++) rows_off[s] = chunk_of[s] >= 0 ? dev_off[chunk_of[s]] + (size_t)(rows[s] - lo[chunk_of[s]]) : 0;
    return true;
}

} // namespace
