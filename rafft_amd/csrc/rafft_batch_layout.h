// rafft_batch_layout.h - what the host and the device of the batch drivers must agree on: the per-item records the kernels of
// rafft_mfe.hip, rafft_mfe_span.hip, rafft_pf.hip, rafft_pf_span.hip, rafft_mea.hip, rafft_sample.hip, rafft_subopt.hip,
// rafft_findpath.hip, rafft_descend.hip, rafft_barriers.hip and rafft_kinfold.hip read and write, and the sizes both sides compute:
// the LDS of the MFE and sampling kernels, the banded tables and aux arrays of the span folds, the aux and stack of an MEA
// structure, a state of the enumeration and its packed copy, the buffers of a findpath problem and of a gradient walk, the work
// area of a barrier tree, the buffers of a folding trajectory.  The layouts that fill the records are in rafft_hostpure.h.
// Plain C++, no HIP include: g++ compiles it with the programs of tests/hostcheck, hipcc with the kernels.
#pragma once

#ifdef __HIPCC__
#define RAFFT_HD __host__ __device__
#else
#define RAFFT_HD
#endif

// ---- minimum-free-energy folds (rafft_mfe.hip)

#define MFE_LDS_BYTES (128 << 10)
// LDS class: three triangular int32 tables of L (L + 1) / 2 cells, F (L + 1 ints) and the bases (L bytes, padded to 16) in 128 KiB
#define RAFFT_MFE_LDS_LEN 146
RAFFT_HD constexpr int mfe_lds_bytes(int L) { return (3 * (L * (L + 1) / 2) + L + 1) * 4 + ((L + 15) & ~15); }
static_assert(mfe_lds_bytes(RAFFT_MFE_LDS_LEN) <= MFE_LDS_BYTES && mfe_lds_bytes(RAFFT_MFE_LDS_LEN + 1) > MFE_LDS_BYTES, "RAFFT_MFE_LDS_LEN is what 128 KiB hold");

struct MfeSeq {
    unsigned long long code_off;    // bases in `codes`
    unsigned long long tab_off;     // HBM class: first int of the sequence's three L x L tables in the workspace
    unsigned long long stack_off;   // first word of its traceback stack (L + 8 words)
    unsigned long long db_off;      // its row in the output (L + 1 bytes)
    int L, pad;
};

// ---- the same under constraints and soft terms (the mfe_con_* kernels of rafft_mfe.hip)

// A sequence's constraint pack, mfe_con_pack_ints(L) int32 back to back: code[L] - the partner of a position with a bracket, else
// one of MFE_CON_*; must[L + 1] - must[k] = positions before k that have to pair (neither . nor x), so a..b may stay unpaired iff
// must[b + 1] == must[a]; usum[L + 1] - usum[k] = the sum of soft_unpaired before k; b[L] - soft_stack.  A sequence without any
// constraint has no pack: its offset is MFE_CON_NONE.
#define MFE_CON_ANY (-1)            // .
#define MFE_CON_UNPAIRED (-2)       // x
#define MFE_CON_PAIRED (-3)         // |
#define MFE_CON_DOWN (-4)           // <  paired with a partner downstream
#define MFE_CON_UP (-5)             // >  paired with a partner upstream
#define MFE_CON_NONE (~0ull)
RAFFT_HD constexpr int mfe_con_pack_ints(int L) { return 4 * L + 2; }
// LDS class: the pack behind the bases.  More than the 128 KiB of the unconstrained kernel at RAFFT_MFE_LDS_LEN, within the
// 160 KiB a workgroup may have: the LDS bound is the same for both entry points
#define MFE_CON_LDS_BYTES (160 << 10)
RAFFT_HD constexpr int mfe_con_lds_bytes(int L) { return mfe_lds_bytes(L) + ((4 * mfe_con_pack_ints(L) + 15) & ~15); }
static_assert(mfe_con_lds_bytes(RAFFT_MFE_LDS_LEN) <= MFE_CON_LDS_BYTES, "the constraint pack of RAFFT_MFE_LDS_LEN positions fits the LDS of a workgroup");

// ---- minimum-free-energy folds of two-strand dimers (rafft_cofold.hip)

// LDS class: G, the exterior energies of the two strand ends (L + 1 ints: FA[i] at i for i < c, FB[j] at j + 1 for j >= c, 0 at c
// for both), behind the bases.  The kernel takes a dynamic size of its own (130112 bytes at RAFFT_MFE_LDS_LEN), so the LDS bound
// stays rafft_mfe_lds_len() for both entry points whatever the two layouts grow by
#define COFOLD_LDS_BYTES (160 << 10)
RAFFT_HD constexpr int cofold_lds_bytes(int L) { return mfe_lds_bytes(L) + ((4 * (L + 1) + 15) & ~15); }
static_assert(cofold_lds_bytes(RAFFT_MFE_LDS_LEN) <= COFOLD_LDS_BYTES, "G of RAFFT_MFE_LDS_LEN positions fits the LDS of a workgroup");
// HBM class: G of a sequence lies in a buffer of its own, as long as the stacks, at the sequence's stack_off (MfeSeq): its L + 1
// ints fit the L + 8 words a stack has

// ---- minimum-free-energy folds under a base-pair span (rafft_mfe_span.hip)

// What a sequence of L positions folded with pairs of at most max_span positions has on the device.  W = min(max_span, L) cells
// d = j - i a row.  Four tables of L x W int32 back to back from tab_off: C and M as [i][d], M1 and X (C + exterior stem) by
// their 3' end as [j][d].  F: L + 1 ints.  A traceback stack of L + 8 words (i | d << 15 | table << 30), a row of L + 1 bytes.
#define MFE_SPAN_TABLES 4
RAFFT_HD constexpr int mfe_span_width(int L, int max_span) { return max_span < L ? max_span : L; }
RAFFT_HD constexpr unsigned long long mfe_span_table_ints(int L, int W) { return (unsigned long long)L * (unsigned long long)W; }
// dynamic LDS of the exterior and the traceback kernel for the longest sequence of a chunk: F, then the pair table over it
RAFFT_HD constexpr int mfe_span_lds_bytes(int L) { return (L + 1) * 4; }

struct MfeSpanSeq {
    unsigned long long code_off;    // bases in `codes`
    unsigned long long tab_off;     // first int of its four L x W tables in the workspace
    unsigned long long f_off;       // first int of its exterior energies (L + 1)
    unsigned long long stack_off;   // first word of its traceback stack (L + 8 words)
    unsigned long long db_off;      // its row in the output (L + 1 bytes)
    int L, W;
};

// ---- partition function and pair probabilities (rafft_pf.hip)

struct PfSeq {
    unsigned long long code_off;    // bases in `codes`
    unsigned long long tab_off;     // first double of the sequence's six L x L tables in the workspace
    unsigned long long aux_off;     // first double of ps, pb, F, Fr (L + 1 each)
    unsigned long long db_off;      // its row in the output (L + 1 bytes)
    int L, mfe_dcal;
    double scale, ln_scale;
};
struct PfRec {
    int status, n_pairs, bad, pad;  // bad: a probability that is not finite
    double energy, mfe_frequency;
};

// ---- partition function and pair probabilities under a base-pair span (rafft_pf_span.hip)

// What a sequence of L positions with pairs of at most max_span positions has on the device.  W = mfe_span_width(L, max_span)
// cells d = j - i a row.  Six tables of L x W fp64 back to back from tab_off: C, M, Co, Mo as [i][d], M1 and M1o by their 3' end
// as [j][d]; between the inside and the outside pass Co holds C w(exterior stem) by the 5' end and M1o the same by the 3' end
// (what the exterior sums read), after the probability kernel Mo holds P as [i][d].  From aux_off, pf_span_aux_doubles(L, W)
// doubles: ps and pb (W + 2 each), the mantissas of F and of Fr (L + 1 each), unpaired (L).  From exp_off, pf_span_exp_ints(L)
// ints: the binary exponents of F and of Fr (L + 1 each).  A row of L + 1 bytes.
//   bytes of a sequence = 48 L W + 8 (3 L + 2 W + 6) + 8 (L + 1) + L + 1
#define PF_SPAN_TABLES 6
#define PF_SPAN_RING 4096           // slots of the exterior kernel's LDS ring (a mantissa and an exponent each: 48 KiB), a power of two
RAFFT_HD constexpr unsigned long long pf_span_table_doubles(int L, int W) { return (unsigned long long)L * (unsigned long long)W; }
RAFFT_HD constexpr unsigned long long pf_span_aux_doubles(int L, int W) { return 2ull * ((unsigned long long)W + 2ull) + 2ull * ((unsigned long long)L + 1ull) + (unsigned long long)L; }
RAFFT_HD constexpr unsigned long long pf_span_exp_ints(int L) { return 2ull * ((unsigned long long)L + 1ull); }
RAFFT_HD constexpr unsigned long long pf_span_seq_bytes(int L, int W)
{
    return 8ull * (PF_SPAN_TABLES * pf_span_table_doubles(L, W) + pf_span_aux_doubles(L, W)) + 4ull * pf_span_exp_ints(L) + (unsigned long long)L + 1ull;
}

struct PfSpanSeq {
    unsigned long long code_off;    // bases in `codes`
    unsigned long long tab_off;     // first double of its six L x W tables in the workspace
    unsigned long long aux_off;     // first double of ps, pb, the mantissas of F and Fr, unpaired
    unsigned long long exp_off;     // first int of the exponents of F and Fr
    unsigned long long db_off;      // its row in the output (L + 1 bytes)
    int L, W, mfe_dcal, pad;
    double scale, ln_scale;
};

// ---- maximum-expected-accuracy structures (rafft_mea.hip)

// What a sequence of L positions has on the device.  Four L x L fp64 tables in the workspace: P (read for i < j only), WT (the
// weights, transposed), E and its transposed copy ET.  In the aux buffer from aux_off, mea_aux_doubles(L) doubles: q (L), the
// positions' shares of the diversity (L), the diversity.  A traceback stack of mea_stack_words(L) words (an interval is i | j << 16),
// a pair table of L int16 (-1 = unpaired), a row of L + 1 bytes.
RAFFT_HD constexpr unsigned long long mea_aux_doubles(int L) { return 2ull * (unsigned long long)L + 2ull; }
RAFFT_HD constexpr unsigned long long mea_stack_words(int L) { return (unsigned long long)L + 8ull; }

struct MeaSeq {
    unsigned long long p_off, wt_off, e_off, et_off;    // first double of each table in the workspace
    unsigned long long aux_off;     // first double of q
    unsigned long long stack_off;   // first word of its traceback stack
    unsigned long long pt_off;      // first int16 of its pair table
    unsigned long long db_off;      // its row in the output (L + 1 bytes)
    int L, pad;
};
struct MeaRec {
    int bad, n_pairs;               // bad: MEA_BAD_*
    double mea, diversity;
};

// ---- structures drawn from the ensemble (rafft_sample.hip)

#define SAMPLE_NT 256               // four wavefronts: four samples of one sequence per workgroup
#define RAFFT_SAMPLE_STACK(L) ((L) / 5 + 2)

struct SampleSeq {
    unsigned long long seed;
    unsigned long long row_off;     // first byte of the sequence's n_samples rows (L + 1 bytes each) in the chunk's row buffer
    unsigned long long dcal_off;    // first int of its n_samples energies
};

// a row (L + 1 bytes, padded to 16) and a stack of pending segments, as the sampling kernel's waves and the enumeration's states hold them
RAFFT_HD constexpr int row_bytes16(int L) { return (L + 1 + 15) & ~15; }
RAFFT_HD constexpr int seg_stack_words(int L) { return (RAFFT_SAMPLE_STACK(L) + 3) & ~3; }
// per-wave LDS of the sampling kernel for the longest sequence of a launch: the row and the stack
RAFFT_HD constexpr int sample_lds_bytes(int L) { return (SAMPLE_NT / 64) * (row_bytes16(L) + 4 * seg_stack_words(L)); }

// ---- every structure within an energy band (rafft_subopt.hip)

// a state of a sequence of L: e_fixed, e_pending, the number of pending segments, a spare word; the stack; the row and its NUL
RAFFT_HD constexpr int subopt_state_bytes(int L) { return 16 + 4 * seg_stack_words(L) + row_bytes16(L); }

struct SuboptSeq {
    unsigned long long code_off;    // bases in `codes`
    unsigned long long tab_off;     // first int of the sequence's three L x L tables in the table workspace
    unsigned long long f_off;       // first int of its exterior energies (L + 1)
    unsigned long long buf_off[2];  // first byte of its two frontier buffers (max_structs states each)
    unsigned long long cnt_off;     // first int of its counts / offsets (max_structs)
    int L, pad;
};
struct SuboptRec {
    int n[2];                       // states in buffer 0 / 1
    int state, bad;                 // SUBOPT_*; SUBOPT_BAD_*
    int final_buf, levels, mfe, pad;
    long long n_reached;
};

// the packed copy of n finished states, in the buffer that is not the final one: n rows of L + 1 bytes, then at this offset n energies
RAFFT_HD inline unsigned long long subopt_pack_dcal_off(int n, int L) { return ((unsigned long long)n * (unsigned long long)(L + 1) + 15ull) & ~15ull; }

// ---- folding barriers between structure pairs (rafft_findpath.hip)

#define FINDPATH_KEY_BITS 22                                // of the biased saddle and of the biased energy in a candidate's key
#define FINDPATH_BIAS (1 << (FINDPATH_KEY_BITS - 1))        // an energy e is held when -FINDPATH_BIAS < e < FINDPATH_BIAS
#define FINDPATH_INDEX_BITS 20                              // parent rank * d + move number: below RAFFT_FINDPATH_MAX_CANDIDATES

RAFFT_HD constexpr unsigned long long fp_align16(unsigned long long x) { return (x + 15ull) & ~15ull; }
// 64-bit words of a mask over d moves (one at least)
RAFFT_HD constexpr int fp_mask_words(int d) { return d > 64 ? (d + 63) / 64 : 1; }

// What a problem of L positions, d moves of which n_rem are removals, and width W has on the device.  Its inputs, in the chunk's
// input buffer from in_off: the pair tables of A and B (int16, -1 = unpaired), the moves as (i | j << 16), removals first, and per
// addition its conflict mask.  Its outputs, in the chunk's output buffer from out_off: d moves as (i, j) ints, d + 1 energies.
// Its work area, in the chunk's workspace from ws_off: two beams of W masks and W (energy, saddle) pairs, W d candidate keys,
// and per level W records (parent rank | move << 16, energy) of the kept states.
RAFFT_HD constexpr unsigned long long fp_in_pt_bytes(int L) { return fp_align16(2ull * (unsigned long long)L); }
RAFFT_HD constexpr unsigned long long fp_in_moves_off(int L) { return 2 * fp_in_pt_bytes(L); }
RAFFT_HD constexpr unsigned long long fp_in_conf_off(int L, int d) { return fp_in_moves_off(L) + fp_align16(4ull * (unsigned long long)d); }
RAFFT_HD constexpr unsigned long long fp_in_bytes(int L, int d, int n_rem)
{
    return fp_in_conf_off(L, d) + (unsigned long long)(d - n_rem) * (unsigned long long)fp_mask_words(d) * 8ull;
}
RAFFT_HD constexpr unsigned long long fp_out_dcal_off(int d) { return fp_align16(8ull * (unsigned long long)d); }
RAFFT_HD constexpr unsigned long long fp_out_bytes(int d) { return fp_out_dcal_off(d) + fp_align16(4ull * ((unsigned long long)d + 1)); }
RAFFT_HD constexpr unsigned long long fp_ws_mask_bytes(int d, int W) { return (unsigned long long)W * (unsigned long long)fp_mask_words(d) * 8ull; }
RAFFT_HD constexpr unsigned long long fp_ws_es_off(int d, int W) { return 2 * fp_ws_mask_bytes(d, W); }                 // two beams of W (energy, saddle)
RAFFT_HD constexpr unsigned long long fp_ws_keys_off(int d, int W) { return fp_ws_es_off(d, W) + 2ull * (unsigned long long)W * 8ull; }
RAFFT_HD constexpr unsigned long long fp_ws_back_off(int d, int W) { return fp_ws_keys_off(d, W) + (unsigned long long)W * (unsigned long long)d * 8ull; }
RAFFT_HD constexpr unsigned long long fp_ws_bytes(int d, int W) { return fp_ws_back_off(d, W) + (unsigned long long)W * (unsigned long long)d * 8ull; }

struct FpProb {
    unsigned long long code_off;    // bases in `codes`
    unsigned long long in_off;      // first byte of its inputs in the chunk's input buffer
    unsigned long long out_off;     // first byte of its outputs in the chunk's output buffer
    unsigned long long ws_off;      // first byte of its work area in the chunk's workspace
    int L, d, n_rem, W;
};
struct FpRec {
    int n_cur, n_keys;              // states of the current beam; candidate keys written in this level
    int flags;                      // FP_*
    int start, end, end_eval;       // energies of A and of survivor 0; of B as eval_kernel sums it (they must agree)
    int saddle, saddle_step;
};
#define FP_RANGE 1                  // an energy outside what a key holds
#define FP_BAD_PAIR 2               // a non-canonical pair met on the device (the host refuses them: cannot happen)
#define FP_STUCK 4                  // a level without a candidate (cannot happen: a legal move always exists)

// ---- gradient walks to local minima (rafft_descend.hip)

// What a walk over L positions has on the device.  Its row, in the chunk's row buffer from io_off: on the way in the pair table
// (int16, -1 = unpaired), on the way out the end row as L characters of ( ) . and a NUL, over the same bytes (L + 1 <= 2 L).  Its
// moves, when the caller asked for them, in the chunk's move buffer from mv_off: 2 x bound ints, (i, j) added, (-i-1, -j-1) removed.
#define DESCEND_NO_MOVES (~0ull)
RAFFT_HD constexpr unsigned long long descend_io_bytes(int L) { return fp_align16(2ull * (unsigned long long)L); }
RAFFT_HD constexpr unsigned long long descend_moves_bytes(int bound) { return fp_align16(8ull * (unsigned long long)bound); }
// the steps a walk may take: max_steps, or 2 L + 16 when max_steps is 0
RAFFT_HD constexpr int descend_bound(int L, int max_steps) { return max_steps > 0 ? max_steps : 2 * L + 16; }
// dynamic LDS of the kernel for the longest walk of a chunk: the pair table
RAFFT_HD constexpr int descend_lds_bytes(int L) { return (2 * L + 15) & ~15; }

struct DsWalk {
    unsigned long long code_off;    // bases in `codes`
    unsigned long long io_off;      // first byte of its row in the chunk's row buffer
    unsigned long long mv_off;      // first byte of its moves in the chunk's move buffer, or DESCEND_NO_MOVES
    int L, bound;
};
struct DsRec {
    int flags;                      // DS_*
    int n_steps;
    int start, end;                 // energies of the start row and of the row the walk reached
};
#define DS_MORE 1                   // the walk took `bound` steps and could take another
#define DS_BAD_PAIR 2               // a non-canonical pair met on the device (the host refuses them: cannot happen)

// ---- exact barrier trees of energy bands (rafft_barriers.hip)

// What a sequence of n rows over L positions has on the device, its work area.  Per row: its pair table (int16, -1 = unpaired;
// barriers_pt_bytes(L) bytes apart), its 128-bit key (two uint64), down and basin (int32 each: ranks within the sequence).  Per
// sequence: the row table, barriers_row_slots(n) slots of 8 bytes (tag << 32 | rank; BAR_EMPTY when free), and the edge table,
// barriers_edge_slots(cap) slots of a 64-bit key (a << 32 | b, a < b ranks of two minima) and a 32-bit value (the saddle rank).
// Rows are numbered through the chunk (row0 + rank); keys, down and basin are indexed by that number.
#define BAR_EMPTY (~0ull)
RAFFT_HD constexpr unsigned long long barriers_pt_bytes(int L) { return fp_align16(2ull * (unsigned long long)L); }
RAFFT_HD constexpr unsigned long long barriers_pow2(unsigned long long x) { unsigned long long p = 1; while (p < x) p <<= 1; return p; }
// a power of two >= 2 n: the table is never more than half full, so a probe sequence is short and always meets a free slot
RAFFT_HD constexpr unsigned long long barriers_row_slots(long long n) { return barriers_pow2(2ull * (unsigned long long)(n > 0 ? n : 1)); }
// the distinct edges a sequence may have: max_edges, or 4 n when it is 0; 1024 at least, 2^30 at most (slot numbers fit 31 bits)
RAFFT_HD constexpr long long barriers_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : v > hi ? hi : v; }
RAFFT_HD constexpr long long barriers_edge_cap(long long n, int max_edges) { return barriers_clamp(max_edges > 0 ? (long long)max_edges : 4 * n, 1024, 1ll << 30); }
RAFFT_HD constexpr unsigned long long barriers_edge_slots(long long cap) { return barriers_pow2(2ull * (unsigned long long)cap); }
RAFFT_HD constexpr unsigned long long barriers_area_bytes(int L, long long n, long long cap)
{
    return (unsigned long long)n * (barriers_pt_bytes(L) + 16ull + 4ull + 4ull) + 8ull * barriers_row_slots(n) + 12ull * barriers_edge_slots(cap);
}
// dynamic LDS of the neighbour kernels for the longest sequence of a chunk: the pair table
RAFFT_HD constexpr int barriers_lds_bytes(int L) { return (2 * L + 15) & ~15; }

struct BarSeq {
    unsigned long long code_off;    // bases in `codes`
    unsigned long long pt_off;      // first byte of its pair tables in the chunk's buffer
    unsigned long long tab_off;     // first slot of its row table in the chunk's
    unsigned long long edge_off;    // first slot of its edge table in the chunk's
    unsigned tab_mask, edge_mask;   // slots - 1
    unsigned edge_cap;              // distinct edges it may have
    int L, n_rows;
    int row0;                       // the chunk's number of its rank 0
    int pt_stride;                  // bytes from one pair table to the next
    int _pad;
};
struct BarRec {
    unsigned long long dup;         // (x << 32 | r) of the lowest-ranked row x with a twin r < x; BAR_EMPTY: none
    unsigned long long hits;        // neighbour probes of the down pass that found a row
    unsigned claims;                // slots of the edge table taken
    unsigned flags;                 // BAR_*
};
#define BAR_EDGES_FULL 1            // more distinct edges than edge_cap, or no free slot
#define BAR_TABLE_BAD 2             // a row table without a free slot, or a rank outside the sequence in it (cannot happen)

// ---- stochastic folding trajectories (rafft_kinfold.hip)

// What a trajectory over L positions has on the device.  Its row, in the chunk's row buffer from io_off, as a walk of descend has it:
// the pair table on the way in, the end row and a NUL on the way out.  Its log, when the caller asked for it, in the chunk's log
// buffer from log_off: 2 x bound ints (the moves, as descend's) and behind them bound doubles (the time of every jump).  Its sample
// records, n_times of them, in the chunk's sample buffer at (its number in the chunk) * n_times.  The watched rows of its sequence
// are n_watch pair tables of L int16 each, back to back from element wt_off of the call's watch buffer.
#define RAFFT_KINFOLD_NW 4096                   // entries of the weight table: dE of 0 .. NW - 1 dcal; weight 0 beyond it
#define RAFFT_KINFOLD_MAX_WATCH 64              // one lane of the wavefront per watched row
#define RAFFT_KINFOLD_DEFAULT_STEPS (1 << 20)   // the steps a trajectory may take when max_steps is 0
#define KINFOLD_NO_LOG (~0ull)
#define KINFOLD_W0 (1ull << 32)                 // the weight of a move with dE <= 0: rate 1
RAFFT_HD constexpr unsigned long long kinfold_io_bytes(int L) { return fp_align16(2ull * (unsigned long long)L); }
RAFFT_HD constexpr unsigned long long kinfold_log_bytes(int bound) { return 16ull * (unsigned long long)bound; }
RAFFT_HD constexpr int kinfold_bound(int max_steps) { return max_steps > 0 ? max_steps : RAFFT_KINFOLD_DEFAULT_STEPS; }
// dynamic LDS of the kernel for the longest trajectory of a chunk: the pair table and the weight subtotal of every position
RAFFT_HD constexpr int kinfold_pt_bytes(int L) { return (2 * L + 15) & ~15; }
RAFFT_HD constexpr int kinfold_lds_bytes(int L) { return kinfold_pt_bytes(L) + 8 * L; }

struct KfTraj {
    unsigned long long code_off;    // bases in `codes`
    unsigned long long io_off;      // first byte of its row in the chunk's row buffer
    unsigned long long log_off;     // first byte of its log in the chunk's log buffer, or KINFOLD_NO_LOG
    unsigned long long wt_off;      // first int16 of its sequence's watched pair tables
    unsigned long long seed;        // its sequence's
    unsigned k;                     // its number within the sequence: the first word of its Philox counters
    int L, bound;
    int n_watch, n_stop;
    int _pad;
};
struct KfSample {
    int dcal;                       // the energy of the state at that time; INT32_MIN: not reached (KF_MORE)
    int watch;                      // the lowest watched row the state equals, -1: none, -2: not reached
};
struct KfRec {
    int flags;                      // KF_*
    int n_steps;
    int start, end;                 // energies of the start row and of the row the trajectory ended in
    int stop;                       // the stop row it arrived at, or -1
    int _pad;
    double time;
};
#define KF_TIME 1                   // the next jump lies beyond t_max
#define KF_STOP 2                   // arrived at a stop row
#define KF_ABSORBED 4               // no neighbour has a weight above 0
#define KF_MORE 8                   // `bound` steps taken and another would be taken
#define KF_BAD_PAIR 16              // a non-canonical pair met on the device (the host refuses them: cannot happen)
#define KF_STUCK 32                 // the drawn number met no move (cannot happen: it is below the sum of the weights)
