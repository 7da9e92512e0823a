// rafft_hostpure.h - host helpers that need neither HIP nor the global context: base codes, the dot-bracket parsers, the loop
// that encloses a region, the lane cut of a batch, the row layout of the scoring calls and the planning of the batch drivers of
// rafft_batch.h: chunks within a budget, the sequence pack, the graph pack, the solve order, the scale of a partition function,
// and the layouts - every offset the drivers' kernels dereference, as records of rafft_batch_layout.h - with, for the drivers
// that need them, the moves and conflict masks of findpath, the row intake of descend, barriers and kinfold, the tree of
// barriers, the weight table and argument checks of kinfold, the constraint packs of the constrained MFE folds, the cuts of the
// dimer folds.
// Plain C++ (g++ compiles it alone: the programs of tests/hostcheck).  Part of the single translation unit of rafft_api.hip
// (included there, before the kernels).
#pragma once

#include "../../include/rafft_hip.h"
#include "rafft_batch_layout.h"

#include <algorithm>
#include <cmath>
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
// two base codes that form a canonical pair: CG GC GU UG AU UA
static bool fp_canonical(int a, int b) { return (a == 2 && b == 3) || (a == 3 && b == 2) || (a == 3 && b == 4) || (a == 4 && b == 3) || (a == 1 && b == 4) || (a == 4 && b == 1); }

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

// ---- planning of the batch drivers (rafft_batch.h)

// Chunks of consecutive items within a budget.  An item joins the open chunk unless the chunk is non-empty and the item would take
// the chunk's primary or secondary total over `budget`, or the chunk already holds `cap` items (0: no cap): a chunk holds one item
// at least, however large.  cost2 may be null.  off[i]: the primary bytes of the items before i in i's chunk.
struct ChunkPlan {
    struct Range { size_t a, b; };          // items [a, b)
    std::vector<Range> chunks;
    std::vector<size_t> off;
    size_t max_cost = 0, max_cost2 = 0;     // the largest totals of any chunk
};
static ChunkPlan plan_chunks(size_t n, const size_t *cost, const size_t *cost2, size_t budget, size_t cap)
{
    ChunkPlan p;
    p.off.resize(n);
    for (size_t a = 0; a < n;) {
        size_t w = 0, w2 = 0, b = a;
        while (b < n && !(cap && b - a >= cap)) {
            const size_t d2 = cost2 ? cost2[b] : 0;
            if (b > a && (w + cost[b] > budget || w2 + d2 > budget)) break;
            p.off[b] = w;
            w += cost[b]; w2 += d2; b++;
        }
        p.chunks.push_back(ChunkPlan::Range{a, b});
        p.max_cost = std::max(p.max_cost, w); p.max_cost2 = std::max(p.max_cost2, w2);
        a = b;
    }
    return p;
}

// The sequences of rafft_mfe_batch / rafft_pf_batch.  Per sequence: status (empty before too long before bad character), the
// length as reported (max(len, 0)), the folded length (0 for an error) and where its bases lie in `codes` (kBaseCode & 7, back to
// back, 16 zero bytes behind the last); `fold`: the sequences without an error, in input order; first_err: the first error's text (`limit`: the name it gives max_len).
struct SeqPack {
    std::vector<int> status, len, L, fold;
    std::vector<unsigned long long> code_off;
    std::vector<uint8_t> codes;
    std::string first_err;
};
static SeqPack pack_sequences(int n_seq, const char *const *seqs, const int *lens, int max_len, const char *limit = "RAFFT_MFE_MAX_LEN")
{
    SeqPack p;
    p.status.resize(n_seq); p.len.resize(n_seq); p.L.resize(n_seq); p.code_off.resize(n_seq);
    unsigned long long n_codes = 0;
    for (int s = 0; s < n_seq; s++) {
        int st = 0;
        if (lens[s] <= 0) st = RAFFT_ERR_EMPTY;
        else if (lens[s] > max_len) st = RAFFT_ERR_TOO_LONG;
        else for (int x = 0; x < lens[s] && !st; x++) if (kBaseCode[(unsigned char)seqs[s][x]] & 8) st = RAFFT_ERR_BAD_CHAR;
        p.status[s] = st;
        p.len[s] = lens[s] > 0 ? lens[s] : 0;
        p.L[s] = st ? 0 : p.len[s];
        p.code_off[s] = n_codes;
        if (st) {
            if (p.first_err.empty())
                p.first_err = "sequence " + std::to_string(s) + (st == RAFFT_ERR_EMPTY ? ": empty" : st == RAFFT_ERR_TOO_LONG ? std::string(": longer than ") + limit : ": character outside ACGUN");
            continue;
        }
        n_codes += (unsigned long long)p.L[s];
        p.fold.push_back(s);
    }
    p.codes.assign(n_codes + 16, 0);
    for (int s : p.fold)
        for (int x = 0; x < p.L[s]; x++) p.codes[p.code_off[s] + x] = (uint8_t)(kBaseCode[(unsigned char)seqs[s][x]] & 7);
    return p;
}

// ---- layouts of the sequence drivers: from a pack, the call's parameters and the workspace budget to the records the kernels read.
// A sequence with an error (L 0) takes no room anywhere.  Chunks hold up to 65535 sequences (gridDim.y of a launch).

// the longest of the sequences order[a .. b) of a chunk
static int chunk_lmax(const ChunkPlan::Range &c, const std::vector<int> &order, const std::vector<int> &L)
{
    int Lmax = 0;
    for (size_t k = c.a; k < c.b; k++) Lmax = std::max(Lmax, L[order[k]]);
    return Lmax;
}
// the widest band of the sequences order[a .. b) of a chunk of banded tables: the anti-diagonals its passes launch
template <class Seq>
static int chunk_wmax(const ChunkPlan::Range &c, const std::vector<int> &order, const std::vector<Seq> &qs)
{
    int Wmax = 0;
    for (size_t k = c.a; k < c.b; k++) Wmax = std::max(Wmax, qs[order[k]].W);
    return Wmax;
}

// What a layout of tables ends with.  The sequences of `order` own tab_bytes(record) bytes of tables each: the chunks of the order
// within the budget (cost2: a second cost per sequence of the order, or null), and in every record tab_off, the first element of
// the sequence's tables in its chunk's workspace, an element being `elem` bytes.
template <class Seq, class TabBytes>
static ChunkPlan plan_tables(const std::vector<int> &order, std::vector<Seq> &qs, TabBytes tab_bytes, size_t elem, const size_t *cost2, size_t budget)
{
    std::vector<size_t> cost(order.size());
    for (size_t k = 0; k < order.size(); k++) cost[k] = tab_bytes(qs[order[k]]);
    ChunkPlan plan = plan_chunks(order.size(), cost.data(), cost2, budget, 65535);
    for (size_t k = 0; k < order.size(); k++) qs[order[k]].tab_off = plan.off[k] / elem;
    return plan;
}

// rafft_mfe_batch: sequences up to lds_len in the LDS class, the longest first (the workgroups of a launch that run last are the
// short ones), the others in the HBM class in input order, in chunks (plan: over hbm_order) of three L x L int32 tables a sequence;
// order: the LDS class, then the HBM class.  n_stack words of traceback stacks, n_db bytes of rows.
struct MfeLayout {
    std::vector<MfeSeq> qs;
    std::vector<int> lds_order, hbm_order, order;
    ChunkPlan plan;
    unsigned long long n_stack = 0, n_db = 0;
};
static MfeLayout mfe_layout(const SeqPack &pk, int lds_len, size_t budget)
{
    MfeLayout y;
    const int n_seq = (int)pk.L.size();
    y.qs.resize(n_seq);
    for (int s = 0; s < n_seq; s++) {
        const int len = pk.L[s];
        y.qs[s] = MfeSeq{pk.code_off[s], 0, y.n_stack, y.n_db, len, 0};
        if (!len) continue;
        y.n_stack += (unsigned long long)len + 8; y.n_db += (unsigned long long)len + 1;
        (len <= lds_len ? y.lds_order : y.hbm_order).push_back(s);
    }
    std::stable_sort(y.lds_order.begin(), y.lds_order.end(), [&](int a, int b) { return pk.L[a] > pk.L[b]; });
    y.plan = plan_tables(y.hbm_order, y.qs, [](const MfeSeq &q) { return 3 * (size_t)q.L * q.L * 4; }, 4, nullptr, budget);
    y.order = y.lds_order;
    y.order.insert(y.order.end(), y.hbm_order.begin(), y.hbm_order.end());
    return y;
}

// rafft_cofold_batch: the cuts of a call as the kernels read them.  cut[s] = cuts[s] for a sequence without
// an error, 0 (a single strand) for one with an error and for all of them when cuts is null.  A cut outside 0 .. L[s] - 1 is
// RAFFT_ERR_STRUCT of that sequence (status[s]; first_seq, first_err: the first of them); L[s] = 0: the sequence has an error already.
struct CutPack {
    std::vector<int> status, cut;
    int first_seq = -1;
    std::string first_err;
};
static CutPack cut_pack(int n_seq, const int *L, const int *cuts)
{
    CutPack p;
    p.status.assign(n_seq, 0);
    p.cut.assign(n_seq, 0);
    for (int s = 0; s < n_seq; s++) {
        if (!L[s] || !cuts) continue;
        if (cuts[s] < 0 || cuts[s] >= L[s]) {
            p.status[s] = RAFFT_ERR_STRUCT;
            if (p.first_seq < 0) { p.first_seq = s; p.first_err = "sequence " + std::to_string(s) + ": cut outside 0 .. length - 1"; }
            continue;
        }
        p.cut[s] = cuts[s];
    }
    return p;
}

// rafft_mfe_constrained_batch: the constraint packs of a call, as the kernels read them (the layout is
// stated in rafft_batch_layout.h).  Per sequence s of L[s] positions (0: it has an error already and is not looked at) whose
// bases lie at codes + code_off[s]: constraints[s], a string of . x | < > ( ), soft_unpaired[s] and soft_stack[s], L[s] dcal values
// each; every one of the three arrays and every entry may be null.  A sequence with an error, or with no constraint at all, takes no
// space and points at nothing (off[s] = MFE_CON_NONE).  status[s] = RAFFT_ERR_STRUCT for a string of another length than the
// sequence, a character outside the seven, unbalanced brackets, a bracket pair that is not canonical or encloses fewer than 3
// positions: an error of that sequence (first_seq, first_err: the first of them).  param_seq >= 0: that sequence has a soft value
// beyond RAFFT_MFE_SOFT_MAX, an error of the call - nothing else of the pack is valid then.
struct ConstraintPack {
    std::vector<int> status;
    std::vector<unsigned long long> off;    // first int of the sequence's pack in `data`, or MFE_CON_NONE
    std::vector<int32_t> data;              // 16 bytes of zeros behind the last pack
    int first_seq = -1, param_seq = -1;
    std::string first_err;
};
static ConstraintPack constraint_pack(int n_seq, const int *L, const uint8_t *codes, const unsigned long long *code_off, const char *const *constraints,
                                      const int32_t *const *soft_unpaired, const int32_t *const *soft_stack)
{
    ConstraintPack p;
    p.status.assign(n_seq, 0);
    p.off.assign(n_seq, MFE_CON_NONE);
    std::vector<int> stk;
    for (int s = 0; s < n_seq; s++) {
        const int len = L[s];
        const char *con = constraints ? constraints[s] : nullptr;
        const int32_t *u = soft_unpaired ? soft_unpaired[s] : nullptr, *b = soft_stack ? soft_stack[s] : nullptr;
        if (!len || (!con && !u && !b)) continue;
        for (const int32_t *soft : {u, b})
            for (int k = 0; soft && k < len; k++)
                if (soft[k] > RAFFT_MFE_SOFT_MAX || soft[k] < -RAFFT_MFE_SOFT_MAX) {
                    p.param_seq = s;
                    p.first_err = "sequence " + std::to_string(s) + ": a soft constraint beyond RAFFT_MFE_SOFT_MAX at position " + std::to_string(k);
                    return p;
                }
        const size_t at = p.data.size();
        p.data.resize(at + (size_t)mfe_con_pack_ints(len), 0);
        int32_t *code = p.data.data() + at, *must = code + len, *usum = must + len + 1, *bb = usum + len + 1;
        const uint8_t *S = codes + code_off[s];
        const char *why = nullptr;
        if (con && strnlen(con, (size_t)len + 1) != (size_t)len) why = "a constraint string of another length than the sequence";
        stk.clear();
        for (int k = 0; k < len && !why; k++) {
            const char c = con ? con[k] : '.';
            code[k] = c == '.' ? MFE_CON_ANY : c == 'x' ? MFE_CON_UNPAIRED : c == '|' ? MFE_CON_PAIRED : c == '<' ? MFE_CON_DOWN : c == '>' ? MFE_CON_UP : 0;
            if (c == '(') stk.push_back(k);
            else if (c == ')') {
                if (stk.empty()) { why = "unbalanced brackets in the constraint"; break; }
                const int i = stk.back();
                stk.pop_back();
                if (!fp_canonical(S[i], S[k])) why = "a forced pair that is not canonical";
                else if (k - i - 1 < 3) why = "a forced pair that encloses fewer than 3 positions";
                code[i] = k; code[k] = i;
            } else if (!code[k]) why = "a constraint character outside . x | < > ( )";
        }
        if (!why && !stk.empty()) why = "unbalanced brackets in the constraint";
        if (why) {
            p.data.resize(at);
            p.status[s] = RAFFT_ERR_STRUCT;
            if (p.first_seq < 0) { p.first_seq = s; p.first_err = "sequence " + std::to_string(s) + ": " + why; }
            continue;
        }
        for (int k = 0; k < len; k++) {
            must[k + 1] = must[k] + (code[k] != MFE_CON_ANY && code[k] != MFE_CON_UNPAIRED);
            usum[k + 1] = usum[k] + (u ? u[k] : 0);
            bb[k] = b ? b[k] : 0;
        }
        p.off[s] = at;
    }
    p.data.resize(p.data.size() + 4, 0);
    return p;
}

// rafft_mfe_span_batch: every sequence has W = min(max_span, L) cells a row and MFE_SPAN_TABLES tables of L x W int32; chunks
// (plan: over pk.fold) of whole sequences in input order.  n_f ints of exterior energies, n_stack words of traceback stacks, n_db
// bytes of rows over the whole call.
struct MfeSpanLayout {
    std::vector<MfeSpanSeq> qs;
    ChunkPlan plan;
    unsigned long long n_f = 0, n_stack = 0, n_db = 0;
};
static MfeSpanLayout mfe_span_layout(const SeqPack &pk, int max_span, size_t budget)
{
    MfeSpanLayout y;
    const int n_seq = (int)pk.L.size();
    y.qs.resize(n_seq);
    for (int s = 0; s < n_seq; s++) {
        const int L = pk.L[s];
        y.qs[s] = MfeSpanSeq{pk.code_off[s], 0, y.n_f, y.n_stack, y.n_db, L, mfe_span_width(L, max_span)};
        if (!L) continue;
        y.n_f += (unsigned long long)L + 1; y.n_stack += (unsigned long long)L + 8; y.n_db += (unsigned long long)L + 1;
    }
    y.plan = plan_tables(pk.fold, y.qs, [](const MfeSpanSeq &q) { return (size_t)(MFE_SPAN_TABLES * mfe_span_table_ints(q.L, q.W) * 4); }, 4, nullptr, budget);
    return y;
}

// rafft_pf_batch / rafft_sample_batch: chunks (plan: over pk.fold) of n_tabs L x L fp64 tables a sequence and, with cost2, a second
// cost per sequence.  n_aux doubles of ps, pb, F, Fr, n_db bytes of rows.  mfe_dcal, scale and ln_scale of qs are left 0: they
// need the MFE, which the driver gets from the device.
struct PfLayout {
    std::vector<PfSeq> qs;
    ChunkPlan plan;
    unsigned long long n_aux = 0, n_db = 0;
};
static PfLayout pf_layout(const SeqPack &pk, int n_tabs, const size_t *cost2, size_t budget)
{
    PfLayout y;
    const int n_seq = (int)pk.L.size();
    y.qs.resize(n_seq);
    for (int s = 0; s < n_seq; s++) {
        const int L = pk.L[s];
        y.qs[s] = PfSeq{pk.code_off[s], 0, y.n_aux, y.n_db, L, 0, 0.0, 0.0};
        if (!L) continue;
        y.n_aux += 4 * ((unsigned long long)L + 1); y.n_db += (unsigned long long)L + 1;
    }
    y.plan = plan_tables(pk.fold, y.qs, [n_tabs](const PfSeq &q) { return (size_t)n_tabs * q.L * q.L * sizeof(double); }, sizeof(double), cost2, budget);
    return y;
}

// The scale of a sequence's partition function: kT in kcal/mol and 1 / (100 kT) per dcal of a call's temp;
// from the sequence's MFE, exp(-scale_factor MFE / (kT L)) a position (scale_factor 0: 1.07) into mfe_dcal, scale and ln_scale of
// its record - ln_scale the logarithm of the scale as stored, not the exponent it came from.
#define PF_GAS 1.98717e-3           // kcal / (mol K)
struct PfTemp { double kt, beta; };
static PfTemp pf_temp(double temp) { const double kt = (temp + 273.15) * PF_GAS; return PfTemp{kt, 1.0 / (100.0 * kt)}; }
template <class Seq>
static void pf_set_scale(Seq &q, int mfe_dcal, double kt, double scale_factor)
{
    const double sf = scale_factor > 0.0 ? scale_factor : 1.07;
    const double ln_scale = q.L ? -sf * ((double)mfe_dcal / 100.0) / (kt * (double)q.L) : 0.0;
    q.mfe_dcal = mfe_dcal; q.scale = std::exp(ln_scale); q.ln_scale = std::log(q.scale);
}

// rafft_pf_span_batch: every sequence has W = min(max_span, L) cells a row and PF_SPAN_TABLES tables of L x W fp64; chunks (plan:
// over pk.fold) of whole sequences in input order.  n_aux doubles and n_exp ints of the aux arrays, n_db bytes of rows over the
// whole call.  mfe_dcal, scale and ln_scale of qs are left 0: they need the span MFE, which the driver gets from the device.
struct PfSpanLayout {
    std::vector<PfSpanSeq> qs;
    ChunkPlan plan;
    unsigned long long n_aux = 0, n_exp = 0, n_db = 0;
};
static PfSpanLayout pf_span_layout(const SeqPack &pk, int max_span, size_t budget)
{
    PfSpanLayout y;
    const int n_seq = (int)pk.L.size();
    y.qs.resize(n_seq);
    for (int s = 0; s < n_seq; s++) {
        const int L = pk.L[s], W = mfe_span_width(L, max_span);
        y.qs[s] = PfSpanSeq{pk.code_off[s], 0, y.n_aux, y.n_exp, y.n_db, L, W, 0, 0, 0.0, 0.0};
        if (!L) continue;
        y.n_aux += pf_span_aux_doubles(L, W); y.n_exp += pf_span_exp_ints(L); y.n_db += (unsigned long long)L + 1;
    }
    y.plan = plan_tables(pk.fold, y.qs, [](const PfSpanSeq &q) { return (size_t)(PF_SPAN_TABLES * pf_span_table_doubles(q.L, q.W) * sizeof(double)); },
                         sizeof(double), nullptr, budget);
    return y;
}

// rafft_sample_batch.  The rows of pk.fold[k], n_samples of L + 1 bytes: the second cost of its plan
static std::vector<size_t> sample_row_costs(const SeqPack &pk, int n_samples)
{
    std::vector<size_t> row_bytes(pk.fold.size());
    for (size_t k = 0; k < pk.fold.size(); k++) row_bytes[k] = (size_t)n_samples * ((size_t)pk.L[pk.fold[k]] + 1);
    return row_bytes;
}
// ... and, the plan being made: per chunk the rows back to back from byte 0 of the row buffer, the energies of the chunk's k-th
// sequence from int k n_samples; max_seqs: the sequences of the largest chunk.  seeds may be null (every seed 0).
struct SampleLayout {
    std::vector<size_t> row_bytes;
    std::vector<SampleSeq> smp;
    size_t max_seqs = 0;
};
static SampleLayout sample_layout(const SeqPack &pk, const ChunkPlan &plan, int n_samples, const unsigned long long *seeds)
{
    SampleLayout y;
    y.row_bytes = sample_row_costs(pk, n_samples);
    y.smp.assign(pk.L.size(), SampleSeq{0, 0, 0});
    for (const ChunkPlan::Range &c : plan.chunks) {
        unsigned long long at = 0;
        for (size_t k = c.a; k < c.b; k++) {
            const int s = pk.fold[k];
            y.smp[s] = SampleSeq{seeds ? seeds[s] : 0ull, at, (unsigned long long)(k - c.a) * (unsigned long long)n_samples};
            at += y.row_bytes[k];
        }
        y.max_seqs = std::max(y.max_seqs, c.b - c.a);
    }
    return y;
}

// rafft_mea_batch: the records of mea's kernels over the tables of a pf_layout with six tables a sequence.  After pf_prob_kernel
// table 3 holds P and the others are dead: WT, E and ET go to tables 0, 1 and 2, q and the diversity over ps and pb (4 (L + 1)
// doubles of aux are there, mea_aux_doubles(L) are taken), the pair table lies where the sequence's bases lie in `codes` (what
// eval_kernel expects), the row where the centroid row lay.  n_stack: words of traceback stacks.
struct MeaLayout {
    std::vector<MeaSeq> qs;
    unsigned long long n_stack = 0;
};
static MeaLayout mea_layout(const std::vector<PfSeq> &pf)
{
    MeaLayout y;
    y.qs.resize(pf.size());
    for (size_t s = 0; s < pf.size(); s++) {
        const PfSeq &q = pf[s];
        const unsigned long long LL = (unsigned long long)q.L * (unsigned long long)q.L;
        y.qs[s] = MeaSeq{q.tab_off + 3 * LL, q.tab_off, q.tab_off + LL, q.tab_off + 2 * LL, q.aux_off, y.n_stack, q.code_off, q.db_off, q.L, 0};
        if (q.L) y.n_stack += mea_stack_words(q.L);
    }
    return y;
}

// rafft_mea_probs_batch: matrices of lens[s] x lens[s]; status (empty before too long), `order`: the matrices without an error in
// input order, chunks (plan: over order) of four L x L fp64 tables a matrix within the budget (one matrix at least): P, WT, E, ET
// in this order.  n_aux doubles of q and the diversity, n_stack words of stacks, n_pt int16 of pair tables, n_db bytes of rows.
struct MeaProbsLayout {
    std::vector<int> status, len, L, order;
    std::vector<MeaSeq> qs;
    ChunkPlan plan;
    unsigned long long n_aux = 0, n_stack = 0, n_pt = 0, n_db = 0;
    std::string first_err;
};
static MeaProbsLayout mea_probs_layout(int n, const int *lens, size_t budget)
{
    MeaProbsLayout y;
    y.status.resize(n); y.len.resize(n); y.L.resize(n); y.qs.resize(n);
    for (int s = 0; s < n; s++) {
        const int st = lens[s] <= 0 ? RAFFT_ERR_EMPTY : lens[s] > RAFFT_PF_MAX_LEN ? RAFFT_ERR_TOO_LONG : 0;
        y.status[s] = st;
        y.len[s] = lens[s] > 0 ? lens[s] : 0;
        const int L = y.L[s] = st ? 0 : lens[s];
        y.qs[s] = MeaSeq{0, 0, 0, 0, y.n_aux, y.n_stack, y.n_pt, y.n_db, L, 0};
        if (st) {
            if (y.first_err.empty()) y.first_err = "sequence " + std::to_string(s) + (st == RAFFT_ERR_EMPTY ? ": empty" : ": longer than RAFFT_PF_MAX_LEN");
            continue;
        }
        y.n_aux += mea_aux_doubles(L); y.n_stack += mea_stack_words(L); y.n_pt += (unsigned long long)L; y.n_db += (unsigned long long)L + 1;
        y.order.push_back(s);
    }
    std::vector<size_t> tab_bytes(y.order.size());
    for (size_t k = 0; k < y.order.size(); k++) tab_bytes[k] = 4 * (size_t)y.L[y.order[k]] * y.L[y.order[k]] * sizeof(double);
    y.plan = plan_chunks(y.order.size(), tab_bytes.data(), nullptr, budget, 65535);
    for (size_t k = 0; k < y.order.size(); k++) {
        MeaSeq &q = y.qs[y.order[k]];
        const unsigned long long LL = (unsigned long long)q.L * (unsigned long long)q.L;
        q.p_off = y.plan.off[k] / sizeof(double); q.wt_off = q.p_off + LL; q.e_off = q.wt_off + LL; q.et_off = q.e_off + LL;
    }
    return y;
}

// The first entry of a matrix that rafft_mea_probs_batch refuses, for i < j: one that is not finite, below 0 or above 1, or
// non-zero with j - i <= 3.  (i, j) and the reason, or false
static bool mea_probs_bad_entry(const double *P, int L, int &bi, int &bj, const char *&why)
{
    for (int i = 0; i < L; i++)
        for (int j = i + 1; j < L; j++) {
            const double x = P[(size_t)i * L + j];
            const char *w = !(x - x == 0.0) ? "is not finite" : (x < 0.0 || x > 1.0) ? "is outside [0, 1]" : (j - i <= 3 && x != 0.0) ? "is not 0 although j - i <= 3" : nullptr;
            if (w) { bi = i; bj = j; why = w; return true; }
        }
    return false;
}

// rafft_subopt_batch: chunks (plan: over pk.fold) of three L x L int32 tables a sequence as the primary cost, its two frontier
// buffers of max_structs states and its max_structs counts (rounded up to 256 bytes) as the second.  Per chunk the frontiers back to
// back from byte 0 of the frontier buffer; n_f ints of exterior energies over the whole call.  mq: what mfe_diag_kernel reads of a
// sequence (code_off, tab_off, L), for the table fill the enumeration shares with the MFE.
struct SuboptLayout {
    std::vector<size_t> tab_bytes, front_bytes;
    ChunkPlan plan;
    std::vector<SuboptSeq> qs;
    std::vector<MfeSeq> mq;
    unsigned long long n_f = 0;
    size_t max_seqs = 0;
};
static SuboptLayout subopt_layout(const SeqPack &pk, int max_structs, size_t budget)
{
    SuboptLayout y;
    const std::vector<int> &order = pk.fold;
    y.tab_bytes.resize(order.size()); y.front_bytes.resize(order.size());
    for (size_t k = 0; k < order.size(); k++) {
        const int L = pk.L[order[k]];
        y.tab_bytes[k] = 3 * (size_t)L * L * 4;
        y.front_bytes[k] = 2 * (size_t)max_structs * (size_t)subopt_state_bytes(L) + (((size_t)max_structs * 4 + 255) & ~(size_t)255);
    }
    y.plan = plan_chunks(order.size(), y.tab_bytes.data(), y.front_bytes.data(), budget, 65535);
    y.qs.assign(pk.L.size(), SuboptSeq{0, 0, 0, {0, 0}, 0, 0, 0});
    y.mq.assign(pk.L.size(), MfeSeq{0, 0, 0, 0, 0, 0});
    for (const ChunkPlan::Range &c : y.plan.chunks) {
        size_t at = 0;
        for (size_t k = c.a; k < c.b; k++) {
            const int s = order[k], L = pk.L[s];
            const size_t one = (size_t)max_structs * (size_t)subopt_state_bytes(L);
            y.mq[s] = MfeSeq{pk.code_off[s], y.plan.off[k] / 4, 0, 0, L, 0};
            y.qs[s] = SuboptSeq{pk.code_off[s], y.plan.off[k] / 4, y.n_f, {at, at + one}, (at + 2 * one) / 4, L, 0};
            y.n_f += (unsigned long long)L + 1;
            at += y.front_bytes[k];
        }
        y.max_seqs = std::max(y.max_seqs, c.b - c.a);
    }
    return y;
}

// ---- rafft_findpath_batch: a problem from its rows, and the layout of a call

// The moves of a direct path from row a to row b over the bases `codes` (kBaseCode, L of them): the pairs of A not in B, ascending
// 5' end, then the pairs of B not in A, ascending 5' end, as (i | j << 16); per addition the mask of the removals that cross it or
// share a base with it (fp_mask_words(d) words, bit m = move m) - the addition is legal once they are all applied.  Returns
// RAFFT_ERR_STRUCT for a row of another length than L, a character outside ( ) . , an unbalanced row or a non-canonical pair.
struct FpMoves {
    std::vector<int16_t> pt_a, pt_b;
    std::vector<uint32_t> moves;
    std::vector<uint64_t> conf;         // (d - n_rem) x fp_mask_words(d)
    int n_rem = 0, d = 0;
};
static int findpath_moves(const uint8_t *codes, int L, const char *a, const char *b, FpMoves &o)
{
    o = FpMoves{};
    if (!a || !b || strlen(a) != (size_t)L || strlen(b) != (size_t)L) return RAFFT_ERR_STRUCT;
    if (!parse_db(a, L, o.pt_a) || !parse_db(b, L, o.pt_b)) return RAFFT_ERR_STRUCT;
    for (int i = 0; i < L; i++) {
        if (o.pt_a[i] > i && !fp_canonical(codes[i], codes[o.pt_a[i]])) return RAFFT_ERR_STRUCT;
        if (o.pt_b[i] > i && !fp_canonical(codes[i], codes[o.pt_b[i]])) return RAFFT_ERR_STRUCT;
    }
    for (int i = 0; i < L; i++) if (o.pt_a[i] > i && o.pt_b[i] != o.pt_a[i]) o.moves.push_back((uint32_t)i | ((uint32_t)o.pt_a[i] << 16));
    o.n_rem = (int)o.moves.size();
    for (int i = 0; i < L; i++) if (o.pt_b[i] > i && o.pt_a[i] != o.pt_b[i]) o.moves.push_back((uint32_t)i | ((uint32_t)o.pt_b[i] << 16));
    o.d = (int)o.moves.size();
    const int mw = fp_mask_words(o.d);
    o.conf.assign((size_t)(o.d - o.n_rem) * mw, 0);
    for (int m = o.n_rem; m < o.d; m++) {
        const int i = (int)(o.moves[m] & 0xffffu), j = (int)(o.moves[m] >> 16);
        for (int r = 0; r < o.n_rem; r++) {
            const int p = (int)(o.moves[r] & 0xffffu), q = (int)(o.moves[r] >> 16);
            const bool share = p == i || p == j || q == i || q == j;
            const bool cross = (p < i && i < q && q < j) || (i < p && p < j && j < q);
            if (share || cross) o.conf[(size_t)(m - o.n_rem) * mw + (r >> 6)] |= 1ull << (r & 63);
        }
    }
    return 0;
}

// The problems `run` (those without an error, in input order) of a call: chunks of whole problems whose work areas (primary cost)
// and whose inputs and outputs together (second cost) fit the budget each, one problem at least.  Per chunk the inputs lie back to
// back from byte 0 of the input buffer, the outputs from byte 0 of the output buffer, the work areas from byte 0 of the workspace.
struct FpLayout {
    std::vector<FpProb> ps;             // one per problem of the call (zeros for a problem with an error)
    std::vector<size_t> ws_bytes, io_bytes;         // per problem of `run`
    ChunkPlan plan;                     // over `run`
    std::vector<size_t> chunk_in, chunk_out;        // bytes of a chunk's inputs / outputs
    std::vector<int> chunk_dmax;        // the levels of a chunk
    size_t max_in = 0, max_out = 0;
};
static FpLayout findpath_layout(int n_paths, const std::vector<int> &run, const int *L, const int *d, const int *n_rem, const int *W,
                                const unsigned long long *code_off, size_t budget)
{
    FpLayout y;
    y.ps.assign((size_t)n_paths, FpProb{0, 0, 0, 0, 0, 0, 0, 0});
    y.ws_bytes.resize(run.size()); y.io_bytes.resize(run.size());
    for (size_t k = 0; k < run.size(); k++) {
        const int p = run[k];
        y.ws_bytes[k] = (size_t)fp_ws_bytes(d[p], W[p]);
        y.io_bytes[k] = (size_t)(fp_in_bytes(L[p], d[p], n_rem[p]) + fp_out_bytes(d[p]));
    }
    y.plan = plan_chunks(run.size(), y.ws_bytes.data(), y.io_bytes.data(), budget, 65535);
    for (const ChunkPlan::Range &c : y.plan.chunks) {
        size_t in = 0, out = 0;
        int dmax = 0;
        for (size_t k = c.a; k < c.b; k++) {
            const int p = run[k];
            y.ps[p] = FpProb{code_off[p], in, out, y.plan.off[k], L[p], d[p], n_rem[p], W[p]};
            in += (size_t)fp_in_bytes(L[p], d[p], n_rem[p]);
            out += (size_t)fp_out_bytes(d[p]);
            dmax = std::max(dmax, d[p]);
        }
        y.chunk_in.push_back(in); y.chunk_out.push_back(out); y.chunk_dmax.push_back(dmax);
        y.max_in = std::max(y.max_in, in); y.max_out = std::max(y.max_out, out);
    }
    return y;
}

// ---- rafft_descend_batch: a walk's start from its row, and the layout of a call

// The pair table of a start row over the bases `codes` (kBaseCode, L of them); the row is the L bytes at `row` (it need not end
// in a NUL).  Returns RAFFT_ERR_STRUCT for a character outside ( ) . (a NUL before L among them: a row of the wrong length), an
// unbalanced row, a non-canonical pair (N pairs with nothing) or a pair (i, j) with j - i <= 3 - every hairpin of fewer than 3
// positions is one, and every such pair is or holds one.
static int descend_parse_row(const uint8_t *codes, int L, const char *row, std::vector<int16_t> &pt)
{
    if (!row || !parse_db(row, L, pt)) return RAFFT_ERR_STRUCT;
    for (int i = 0; i < L; i++)
        if (pt[i] > i && (pt[i] - i <= 3 || !fp_canonical(codes[i], codes[pt[i]]))) return RAFFT_ERR_STRUCT;
    return 0;
}

// ---- the row intake of the three row drivers (rafft_descend_batch, rafft_barriers_batch, rafft_kinfold_batch)

// row r of sequence s in the caller's blocks of rows
static const char *row_ptr(const char *const *rows, const int *row_stride, int s, size_t r) { return rows[s] + r * (size_t)row_stride[s]; }

// what descend_parse_row's RAFFT_ERR_STRUCT says, behind the name of the row
static const char *const ROW_PARSE_ERR = ": malformed, a non-canonical pair, or a hairpin of fewer than 3";

// a bad row comes back as it went in: its bytes up to L or an earlier NUL, and a NUL
static void copy_row_back(char *db, const char *row, int L)
{
    const size_t n = strnlen(row, (size_t)L);
    memcpy(db, row, n);
    db[n] = 0;
}

// The call's error text: that of the first erroneous item in input order, (sequence, item), item -1 for the sequence itself.
// Seeded with the pack's first error; a later note at the same place does not replace an earlier one.
struct FirstError {
    long long at = -1;
    std::string msg;
    explicit FirstError(const SeqPack &pk) : msg(pk.first_err)
    {
        for (size_t s = 0; s < pk.status.size() && at < 0; s++) if (pk.status[s]) at = (long long)s << 32;
    }
    void note(int s, long long item, const std::string &m)
    {
        const long long k = ((long long)s << 32) + item + 1;
        if (at < 0 || k < at) { at = k; msg = m; }
    }
    const std::string &text() const { return msg; }
};

// The walks that run (those without an error, in input order; walk k is over L[k] positions, may take bound[k] steps, its bases
// lie at code_off[k], want_moves[k]: the caller asked for its moves): chunks of whole walks whose rows and move buffers together fit
// the budget, one walk at least, DESCEND_CHUNK_WALKS at most.  Per chunk the rows lie back to back from byte 0 of the row buffer,
// the moves from byte 0 of the move buffer.
constexpr size_t DESCEND_CHUNK_WALKS = (size_t)1 << 22;
struct DsLayout {
    std::vector<DsWalk> ws;             // one per walk that runs
    std::vector<size_t> bytes;          // per walk: row and moves
    ChunkPlan plan;
    std::vector<size_t> chunk_io, chunk_mv;         // bytes of a chunk's rows / moves
    std::vector<int> chunk_lmax;
    size_t max_io = 0, max_mv = 0;
};
static DsLayout descend_layout(size_t n, const int *L, const int *bound, const unsigned long long *code_off, const unsigned char *want_moves,
                               size_t budget)
{
    DsLayout y;
    y.ws.resize(n); y.bytes.resize(n);
    for (size_t k = 0; k < n; k++) y.bytes[k] = (size_t)(descend_io_bytes(L[k]) + (want_moves[k] ? descend_moves_bytes(bound[k]) : 0ull));
    y.plan = plan_chunks(n, y.bytes.data(), nullptr, budget, DESCEND_CHUNK_WALKS);
    for (const ChunkPlan::Range &c : y.plan.chunks) {
        size_t io = 0, mv = 0;
        int lmax = 0;
        for (size_t k = c.a; k < c.b; k++) {
            y.ws[k] = DsWalk{code_off[k], io, want_moves[k] ? mv : DESCEND_NO_MOVES, L[k], bound[k]};
            io += (size_t)descend_io_bytes(L[k]);
            if (want_moves[k]) mv += (size_t)descend_moves_bytes(bound[k]);
            lmax = std::max(lmax, L[k]);
        }
        y.chunk_io.push_back(io); y.chunk_mv.push_back(mv); y.chunk_lmax.push_back(lmax);
        y.max_io = std::max(y.max_io, io); y.max_mv = std::max(y.max_mv, mv);
    }
    return y;
}

// ---- rafft_barriers_batch: the layout of a call, and the tree from the edges between basins

// The sequences that run (those without an error, in input order; sequence k has n[k] rows over L[k] positions, bases at
// code_off[k]): their work areas (barriers_area_bytes), chunks of whole sequences whose areas fit the budget together, one
// sequence at least - the caller refuses a sequence whose own area is above the budget before it gets here - and per chunk every
// offset the kernels dereference, each buffer from 0.
struct BarLayout {
    std::vector<BarSeq> qs;             // one per sequence that runs
    std::vector<size_t> bytes;          // per sequence: its work area
    ChunkPlan plan;
    std::vector<size_t> chunk_rows, chunk_pt, chunk_tab, chunk_edge;    // rows / pair-table bytes / row-table slots / edge-table slots of a chunk
    std::vector<int> chunk_lmax;
    size_t max_rows = 0, max_pt = 0, max_tab = 0, max_edge = 0, max_seqs = 0;
};
static BarLayout barriers_layout(size_t n_seq, const int *L, const int *n, const unsigned long long *code_off, int max_edges, size_t budget)
{
    BarLayout y;
    y.qs.resize(n_seq); y.bytes.resize(n_seq);
    for (size_t k = 0; k < n_seq; k++) y.bytes[k] = (size_t)barriers_area_bytes(L[k], n[k], barriers_edge_cap(n[k], max_edges));
    y.plan = plan_chunks(n_seq, y.bytes.data(), nullptr, budget, 65535);
    for (const ChunkPlan::Range &c : y.plan.chunks) {
        size_t rows = 0, pt = 0, tab = 0, edge = 0;
        int lmax = 0;
        for (size_t k = c.a; k < c.b; k++) {
            const long long cap = barriers_edge_cap(n[k], max_edges);
            const size_t ts = (size_t)barriers_row_slots(n[k]), es = (size_t)barriers_edge_slots(cap);
            y.qs[k] = BarSeq{code_off[k], pt, tab, edge, (unsigned)(ts - 1), (unsigned)(es - 1), (unsigned)cap, L[k], n[k], (int)rows, (int)barriers_pt_bytes(L[k]), 0};
            rows += (size_t)n[k]; pt += (size_t)n[k] * (size_t)barriers_pt_bytes(L[k]); tab += ts; edge += es;
            lmax = std::max(lmax, L[k]);
        }
        y.chunk_rows.push_back(rows); y.chunk_pt.push_back(pt); y.chunk_tab.push_back(tab); y.chunk_edge.push_back(edge); y.chunk_lmax.push_back(lmax);
        y.max_rows = std::max(y.max_rows, rows); y.max_pt = std::max(y.max_pt, pt); y.max_tab = std::max(y.max_tab, tab);
        y.max_edge = std::max(y.max_edge, edge); y.max_seqs = std::max(y.max_seqs, c.b - c.a);
    }
    return y;
}

// The barrier tree over n_minima minima (numbered by ascending rank) from the edges between their gradient basins, sorted by
// (saddle_rank, a, b): Kruskal with a union-find whose root is the lowest minimum index.  The edges of one saddle_rank are one
// group - the row of that rank may join several components at once: every component that loses its root in the group gets the
// lowest root of what it merged into as father and that rank as saddle.  A minimum that is never merged into a lower one stays a
// root (father = saddle_rank = -1).
static void barriers_tree(int n_minima, const std::vector<rafft_barriers_edge> &edges, std::vector<int32_t> &father, std::vector<int32_t> &saddle_rank)
{
    father.assign((size_t)n_minima, -1); saddle_rank.assign((size_t)n_minima, -1);
    std::vector<int32_t> up((size_t)n_minima), lost;
    for (int m = 0; m < n_minima; m++) up[m] = m;
    auto find = [&](int32_t m) {
        int32_t r = m;
        while (up[r] != r) r = up[r];
        while (up[m] != r) { const int32_t nx = up[m]; up[m] = r; m = nx; }
        return r;
    };
    for (size_t e = 0; e < edges.size();) {
        const int32_t t = edges[e].saddle_rank;
        lost.clear();
        for (; e < edges.size() && edges[e].saddle_rank == t; e++) {
            const int32_t ra = find(edges[e].a), rb = find(edges[e].b);
            if (ra == rb) continue;
            const int32_t lo = std::min(ra, rb), hi = std::max(ra, rb);
            up[hi] = lo;
            lost.push_back(hi);
        }
        for (int32_t m : lost) { father[m] = find(m); saddle_rank[m] = t; }
    }
}

// ---- rafft_kinfold_batch: the weight table, the call's own arguments and the layout of a call

#define KINFOLD_GAS 1.98717e-3      // kcal / (mol K), as PF_GAS

// kT of a call in kcal/mol: kt, or the gas constant times the absolute temperature when kt is 0
static double kinfold_kT(double temp, double kt) { return kt != 0.0 ? kt : KINFOLD_GAS * (temp + 273.15); }

// The weights of a call: W[0] = 2^32 (every dE <= 0), W[d] = floor(2^32 exp(-d / (100 kT)) + 0.5) for d dcal uphill; beyond the
// table the weight is 0.  false: kt negative or not finite, or a kT that is not above 0 and finite.
static bool kinfold_weights(double temp, double kt, uint64_t *out)
{
    if (!(kt >= 0.0) || !std::isfinite(kt)) return false;
    const double kT = kinfold_kT(temp, kt);
    if (!(kT > 0.0) || !std::isfinite(kT)) return false;
    out[0] = KINFOLD_W0;
    for (int d = 1; d < RAFFT_KINFOLD_NW; d++) out[d] = (uint64_t)std::floor(4294967296.0 * std::exp(-(double)d / (100.0 * kT)) + 0.5);
    return true;
}

// what is wrong with the arguments of a call that are not a sequence's own, or null
static const char *kinfold_check_call(int n_rep, double kt, double t_max, int max_steps, int n_times, const double *sample_times, long long workspace_bytes)
{
    if (n_rep < 1) return "n_rep below 1";
    if (!(kt >= 0.0) || !std::isfinite(kt)) return "kt negative or not finite";
    if (!(t_max >= 0.0) || !std::isfinite(t_max)) return "t_max negative or not finite";
    if (max_steps < 0 || workspace_bytes < 0 || n_times < 0) return "negative argument";
    if (n_times > 0 && !sample_times) return "null argument";
    for (int t = 0; t < n_times; t++) {
        if (!(sample_times[t] >= 0.0) || !(sample_times[t] <= t_max)) return "a sample time outside [0, t_max]";
        if (t > 0 && sample_times[t] < sample_times[t - 1]) return "sample times descend";
    }
    return nullptr;
}
static const char *kinfold_check_watch(int n_watch, int n_stop)
{
    if (n_watch < 0 || n_stop < 0) return "negative count";
    if (n_watch > RAFFT_KINFOLD_MAX_WATCH) return "more than 64 watched rows";
    if (n_stop > n_watch) return "more stop rows than watched rows";
    return nullptr;
}

// The trajectories that run (those without an error, in input order; trajectory t is over L[t] positions, the k[t]-th of its
// sequence, its bases at code_off[t], its sequence's watched tables at wt_off[t], want_log[t]: the caller asked for its moves and
// times): chunks of whole trajectories whose rows, sample records and logs together fit the budget, one at least,
// KINFOLD_CHUNK_TRAJ at most.  Per chunk the rows lie back to back from byte 0 of the row buffer, the logs from byte 0 of the log
// buffer, the sample records n_times apiece in the order of the trajectories.
constexpr size_t KINFOLD_CHUNK_TRAJ = (size_t)1 << 22;
struct KfLayout {
    std::vector<KfTraj> ws;             // one per trajectory that runs
    std::vector<size_t> bytes;          // per trajectory: row, samples and log
    ChunkPlan plan;
    std::vector<size_t> chunk_io, chunk_log;        // bytes of a chunk's rows / logs
    std::vector<int> chunk_lmax;
    size_t max_io = 0, max_log = 0, max_traj = 0;
};
static KfLayout kinfold_layout(size_t n, const int *L, const unsigned *k, const unsigned long long *code_off, const unsigned long long *wt_off,
                               const unsigned long long *seed, const int *n_watch, const int *n_stop, const unsigned char *want_log, int bound,
                               int n_times, size_t budget)
{
    KfLayout y;
    y.ws.resize(n); y.bytes.resize(n);
    const size_t log_bytes = (size_t)kinfold_log_bytes(bound), smp_bytes = (size_t)n_times * sizeof(KfSample);
    for (size_t t = 0; t < n; t++) y.bytes[t] = (size_t)kinfold_io_bytes(L[t]) + smp_bytes + (want_log[t] ? log_bytes : 0);
    y.plan = plan_chunks(n, y.bytes.data(), nullptr, budget, KINFOLD_CHUNK_TRAJ);
    for (const ChunkPlan::Range &c : y.plan.chunks) {
        size_t io = 0, lg = 0;
        int lmax = 0;
        for (size_t t = c.a; t < c.b; t++) {
            y.ws[t] = KfTraj{code_off[t], io, want_log[t] ? lg : KINFOLD_NO_LOG, wt_off[t], seed[t], k[t], L[t], bound, n_watch[t], n_stop[t], 0};
            io += (size_t)kinfold_io_bytes(L[t]);
            if (want_log[t]) lg += log_bytes;
            lmax = std::max(lmax, L[t]);
        }
        y.chunk_io.push_back(io); y.chunk_log.push_back(lg); y.chunk_lmax.push_back(lmax);
        y.max_io = std::max(y.max_io, io); y.max_log = std::max(y.max_log, lg); y.max_traj = std::max(y.max_traj, c.b - c.a);
    }
    return y;
}

// the step a step of a folding graph is compared with: the reference compares step 0 with the LAST step (fast_paths[-1], rafft_kin.py:75)
static int kin_prev_step(int i, int n_steps) { return i == 0 ? n_steps - 1 : i - 1; }

// The graphs of rafft_kin_batch, rows packed back to back without their strides.  Per graph: its rows, the number of its first
// row in the batch and the first byte of its rows; per row: its graph, and first row and size of the step it is compared with;
// `rows` (one spare byte behind the last) and `energy` in row order.  false: more than 2^31 - 1 rows (nothing is packed then).
struct KinPack {
    std::vector<int> n_rows, row0, row_graph, row_prev0, row_nprev;
    std::vector<unsigned long long> off;
    std::vector<char> rows;
    std::vector<double> energy;
    long long n = 0;                    // rows of the batch
    unsigned long long bytes = 0;       // of all rows
};
static bool kin_pack(int n_graphs, const int *lens, const int *n_steps, const int *const *step_size, const char *const *rows, const int *row_stride,
                     const double *const *energy, KinPack &p)
{
    p = KinPack{};
    p.n_rows.resize(n_graphs); p.row0.resize(n_graphs); p.off.resize(n_graphs);
    for (int g = 0; g < n_graphs; g++) {
        long long nr = 0;
        for (int i = 0; i < n_steps[g]; i++) nr += step_size[g][i];
        if (p.n + nr > 0x7fffffff) return false;
        p.n_rows[g] = (int)nr; p.row0[g] = (int)p.n; p.off[g] = p.bytes;
        p.n += nr;
        p.bytes += (unsigned long long)nr * (unsigned long long)lens[g];
    }
    p.rows.resize(p.bytes + 1);
    p.row_graph.resize(p.n); p.row_prev0.resize(p.n); p.row_nprev.resize(p.n);
    p.energy.resize(p.n);
    for (int g = 0; g < n_graphs; g++) {
        if (!p.n_rows[g]) continue;
        const size_t L = (size_t)lens[g];
        if (row_stride[g] == lens[g]) memcpy(p.rows.data() + p.off[g], rows[g], (size_t)p.n_rows[g] * L);
        else for (int r = 0; r < p.n_rows[g]; r++) memcpy(p.rows.data() + p.off[g] + (size_t)r * L, rows[g] + (size_t)r * row_stride[g], L);
        memcpy(p.energy.data() + p.row0[g], energy[g], (size_t)p.n_rows[g] * sizeof(double));
        std::vector<int> s0(n_steps[g]);
        int at = p.row0[g];
        for (int i = 0; i < n_steps[g]; i++) { s0[i] = at; at += step_size[g][i]; }
        for (int i = 0; i < n_steps[g]; i++) {
            const int pi = kin_prev_step(i, n_steps[g]);
            for (int r = s0[i]; r < s0[i] + step_size[g][i]; r++) { p.row_graph[r] = g; p.row_prev0[r] = s0[pi]; p.row_nprev[r] = step_size[g][pi]; }
        }
    }
    return true;
}

// The graphs [a, b) of a chunk in the order they are solved: those with 0 < S <= lds_states (their inverse fits LDS) first, in input
// order, then those above; S == 0 is not solved.  Written to order[a ...]; returns the two counts.
struct SolveCounts { int n_small, n_big; };
static SolveCounts kin_solve_order(const int *S, size_t a, size_t b, int lds_states, int *order)
{
    size_t at = a;
    for (size_t g = a; g < b; g++) if (S[g] && S[g] <= lds_states) order[at++] = (int)g;
    const int n_small = (int)(at - a);
    for (size_t g = a; g < b; g++) if (S[g] > lds_states) order[at++] = (int)g;
    return SolveCounts{n_small, (int)(at - a) - n_small};
}

} // namespace
