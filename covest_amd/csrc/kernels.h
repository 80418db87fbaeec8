// kernels.h -- host-callable launchers of the gfx950 kernels (ll_direct.hip,
// argmin.hip, ...).  All launches are asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "device_model.h"
#include "handback.h"
#include "kmer_plan.h"
#include "tiles.h"

namespace covest {

// ---- The launch record (covest_grid_launch_record, covest_model_launch_record): what an evaluation launched ----
// Host bookkeeping only.  A launcher notes the instantiation it picked and how many launches it took into the record
// of the evaluation in progress on the calling thread (LaunchRecordScope; none: nothing is noted).  Nothing is read from
// the device and nothing waits for it.  The names come from the tables beside the instantiation lists (kVariantNames of
// ll_basic.hip, ll_fix.hip, argmin.hip and ll_deriv.hip; K-factored's: the table of factored_launch.h); covest_compiled_variants
// lists those tables.
struct LaunchRecord {
    struct Entry {
        const char *name;
        int64_t launches;
    };
    struct Plan { // a K-factored work description as the host built it (tiles.h FactoredPlan)
        int32_t n_threads, n_buf, ld, n_qblocks, shared_tiles, n_pass, list_mode;
        bool long_part; // a chunk of the long weight vectors (list_mode 3)
        int32_t col_floor; // tiles.h FactoredPlan::col_floor
    };
    Entry entries[16];
    int n_entries = 0;
    Plan plans[8];
    int n_plans = 0; // (plans beyond the room: counted, not kept)
    void clear() { n_entries = n_plans = 0; }
};
void record_launch(const char *name, int64_t launches = 1);
void record_factored_plan(const FactoredPlan &plan, int shared_tiles, bool long_part);
struct LaunchRecordScope { // notes go to `r` (cleared; append: kept and added to) until the scope ends
    explicit LaunchRecordScope(LaunchRecord &r);
    LaunchRecordScope(LaunchRecord &r, bool append);
    ~LaunchRecordScope();
    LaunchRecord *prev;
};
// The instantiations linked in, by family; a launcher records kXxxVariantNames[its index].
constexpr int kFactoredVariants = 10, kBasicVariants = 8, kFixVariants = 6, kArgminVariants = 3, kDerivVariants = 7;
// (K-factored's names: factored_launch.h kFactoredVariantTable, kFactoredVariants rows -- covest_amd/build.py reads the figure above)
extern const char *const kFactoredFinishNames[2];                   // ll_factored_launch.hip: ll_finish_dense, ll_finish_partials
extern const char *const kBasicVariantNames[kBasicVariants];       // ll_basic.hip
extern const char *const kFixVariantNames[kFixVariants];           // ll_fix.hip
extern const char *const kArgminVariantNames[kArgminVariants];     // argmin.hip
extern const char *const kDerivVariantNames[kDerivVariants];       // ll_deriv.hip: six ll_deriv<P,mode>, then ll_deriv_finish

// K-direct: one wavefront per grid point, one exp per pmf term (ll_direct.hip).
// out_ll[n]; when out_p != nullptr (n must be 1) also writes p_j for every bin
// of `m.bins`.
// ref_overflow: the reference's long-double overflow reproduced (direct_point.h REF_OVF; out_p must be nullptr).
hipError_t launch_ll_direct(const DevModel &m, const PointSource &src, int64_t n, double *out_ll,
                            double *out_p, hipStream_t stream, bool ref_overflow = false);

// K-basic: basic model, one lane per grid point, pmf recurrence (ll_basic.hip).
// Needs n_err == 8 and a tile table (keys in 1..16384).
// sub_list: the queue of points handed back (handback.h); run launch_ll_fix_list after this.
hipError_t launch_ll_basic(const DevModel &m, const TileView &tv, const PointSource &src, int64_t n,
                           double *out_ll, const SubList &sub_list, hipStream_t stream);

// K-factored: repeats model on a dense grid, one workgroup per (c, e)
// (ll_factored.hip).  out_ll is the block's LL buffer (index flat - plan.flat_begin).
// sub_list: the queue of points handed back (handback.h; dense grids -- list mode 1 hands the side words over
// in `partial`, list mode 2 leaves the strict evaluation to ll_finish_partials); run launch_ll_fix_list after this.
hipError_t launch_ll_factored(const DevModel &m, const TileView &tv, const FactoredPlan &plan,
                              double *out_ll, const SubList &sub_list, hipStream_t stream);

// Chunked point list (tiles.h FactoredPlan::list_mode 2): combine the chunks' shares of p_j per point and
// take the logs.  first_item[n_points + 1] delimits each point's chunks; point_par[5 n_points] and point_T[n_points]
// are the points' parameters and threshold_o.
hipError_t launch_ll_finish_partials(const DevModel &m, const TileView &tv, const double *partial,
                                     const int32_t *first_item, const double *point_par, const int32_t *point_T,
                                     int64_t n_points, double *out_ll, hipStream_t stream);

// Dense grids, long weight vectors (tiles.h FactoredPlan::list_mode 3): take the logs of the p_j that the chunk
// launches summed into `partial` ([n_ce][n_cols][n_items * 32], first row = (c, e) number ce_first); q_orig[n_cols] maps
// a slot to its index in the (q1, q2, q) product (-1: padding); values go to out_ll[flat - src.flat_begin].
hipError_t launch_ll_finish_dense(const DevModel &m, const TileView &tv, const PointSource &src, const double *partial,
                                  int64_t ce_first, int64_t n_ce, int64_t n_cols, const int32_t *q_orig, int64_t n_q,
                                  int64_t flat_end, double *out_ll, hipStream_t stream);

// The pass after every K-basic / K-factored launch (ll_fix.hip): one wave per point of the queue `list` (handback.h) adds
// the strict evaluation of the rows named in its side word to ll[], in place.  The queue's counter must be zero
// before the NEXT recurrence launch: launch_argmin resets it (grids), the host does for point lists.  list.count is
// whatever word holds the queue's length when the pass runs: the counter itself, or where the arg-min copied it to.
// n_points: how many points the launch before evaluated (the queue cannot be longer; 0: unknown) -- sizes the launch.
hipError_t launch_ll_fix_list(const DevModel &m, const TileView &tv, const PointSource &src, double *ll,
                              const SubList &list, hipStream_t stream, int64_t n_points = 0);

// (min -LL, lowest index) over ll[n]: two-stage reduction (argmin.hip).
// partial_val/partial_idx need kArgminBlocks entries; result[0] = {min, bits of idx}.
constexpr int kArgminBlocks = 1024; // (256: 7.4 us for the 10^6 points of C2; four workgroups a CU hide the loads better)
struct ArgminResult {
    double min_negll;
    int64_t index;  // local index, -1 if no value is < +inf
    double pair[2]; // {min_negll, GLOBAL flat index as a double (-1 if none)}: what the ranks exchange
    int64_t unproven; // launch_argmin_proving: 1 where the queued points' final values could still change the winner
};
// queue_count: the hand-back queue's counter to reset (nullptr: none); two words: the queue's length is copied to the
// second before the first is cleared.
constexpr int64_t kArgminSmall = 16384; // grids up to this size: one workgroup, one launch
// host_mirror: page-locked host memory the winner is stored to as well (nullptr: none)
hipError_t launch_argmin(const double *ll, int64_t n, int64_t flat_begin, double *partial_val, int64_t *partial_idx,
                         ArgminResult *result, ArgminResult *host_mirror, unsigned *queue_count, hipStream_t stream);

// The same over values of which the hand-back queue's points are still PROVISIONAL (the strict pass put off:
// abi_grid.cpp): queue_index[*queue_count] names them, and the kernel that has the winner also walks the queue and sets
// result->unproven unless no queued point's final value can change the winner (argmin.hip winner_unproven).  The
// queue's length is left in queue_count[1] for the pass that comes later, queue_count[0] is reset as above.
// queue_index == nullptr: launch_argmin (unproven = 0).
hipError_t launch_argmin_proving(const double *ll, int64_t n, int64_t flat_begin, double *partial_val, int64_t *partial_idx,
                                 ArgminResult *result, ArgminResult *host_mirror, unsigned *queue_count,
                                 const int64_t *queue_index, hipStream_t stream);

// The same reduction and, beside it, the selection scan of covest/grid.py:65-70 started from `start`: the strict
// running-minimum records below it, in index order, written to `scan` (page-locked host memory).  n <= kArgminSmall.
constexpr int kScanCap = 120;
struct ScanRecords {
    int32_t n;         // records listed (written LAST, behind a system-scope fence)
    int32_t truncated; // 1: there were more than kScanCap -- read the values back instead
    double start;      // the minimum the scan started from (echo)
    struct {
        int64_t index; // GLOBAL flat index
        double negll;
    } rec[kScanCap];
};
hipError_t launch_argmin_scan(const double *ll, int64_t n, int64_t flat_begin, double start, ArgminResult *result,
                              ArgminResult *host_mirror, ScanRecords *scan, unsigned *queue_count, hipStream_t stream);

// ---- K-axis-min (axis_min.hip): the same selection per cell of the product of the KEPT axes of a grid ----
// The launch description, built on the host by axis_min_plan.  Axes of length 1 dropped and adjacent axes of one side
// merged, the grid is at most three kept and three reduced groups that alternate; a point's flat index is
// sum coord * kstride over the kept groups plus sum coord * rstride over the reduced ones.
struct AxisMinPlan {
    int32_t n_kept, n_red;         // groups on either side (0..3)
    int32_t last_kept, first_kept; // the fastest / the slowest group is a kept one
    int64_t klen[3], kstride[3];   // kept groups in the axes' order: length, stride in the flat index
    int64_t rlen[3], rstride[3];   // reduced groups
    int64_t n_cells, n_red_total;  // product of the kept / the reduced lengths
    int64_t flat_begin, flat_end;  // the block the LL buffer holds (index flat - flat_begin)
    int64_t lead_lo, lead_hi;      // coordinates of the slowest group the block touches (lo > hi: none)
    int64_t r_begin, r_end;        // row-major numbers of the reduced coordinates a cell walks
    int64_t n_slices, per_slice;   // ... in n_slices runs of per_slice: one candidate per (cell, slice)
};
// keep_mask: bit d set = axis d is kept.  false: more groups than a plan holds (not with kMaxParams axes).
bool axis_min_plan(const int64_t *len, int n_axes, uint32_t keep_mask, int64_t flat_begin, int64_t flat_end, AxisMinPlan *out);
// out_val/out_idx[n_cells]: min -LL and the GLOBAL flat index of the lowest-index point attaining it, (+inf, -1)
// where no point of the block in the cell is < +inf.  partial_val/partial_idx need n_cells * n_slices entries when
// n_slices > 1 (else unused).  One launch, two with slices; not entered in the launch record.
hipError_t launch_axis_min(const AxisMinPlan &p, const double *ll, double *partial_val, int64_t *partial_idx, double *out_val,
                           int64_t *out_idx, hipStream_t stream);

// ---- K-grad, K-hess and K-opg (ll_deriv.hip): value, analytic gradient (order 1), closed-form Hessian (order 2), or the
// outer product of the per-k-mer scores beside order 1's value and gradient (order kDerivOpg: a mode, not a derivative) ----
// One workgroup per (point, segment of ll_deriv_segments(m) key segments) leaves compensated partial sums in `partial`
// (ll_deriv_partial_bytes(m, order, n) bytes): per segment 2 + 2P sums for order 1 (h log p, p, h d_k p / p, d_k p),
// P (P + 1) more for order 2 (the two second-order sums of each pair k <= l), each a (hi, lo) pair, and one double behind
// them; P (P + 1) / 2 more than order 1 for kDerivOpg (sum h (d_k p / p)(d_l p / p) of each pair).  A second launch adds
// a point's segments in ascending order and applies the tail terms.  out_ll[n], out_grad[n][P], and for order 2 or
// kDerivOpg out_hess[n][P][P], the Hessian or the outer product (symmetric: the upper triangle computed, mirrored; not
// read for order 1); src is a point list.  Two launches (per 16384 points), each noted in the launch record.
constexpr int kDerivOpg = 3;
int ll_deriv_segments(const DevModel &m);
size_t ll_deriv_partial_bytes(const DevModel &m, int order, int64_t n);
hipError_t launch_ll_deriv(const DevModel &m, int order, const PointSource &src, int64_t n, double *partial, double *out_ll,
                           double *out_grad, double *out_hess, hipStream_t stream);

// K-grad's walk (order 1) or K-hess's (order 2) with its per-key quantities stored on the way (DESIGN.md sections 6u, 6x): `m` is the batch's table
// model (the all-keys view, a zero count array, tail 1).  rows: per point P + 1 rows of n_keys doubles, point-major -- row
// (P + 1) i is log p_ij in launch_batch_table's conventions (+0.0 dead and nothing else, p = 1 as -0.0, NaN stays), rows
// (P + 1) i + 1 + k the scores d_k p_ij / p_ij, +0.0 at a dead key and throughout where the clamp moved parameter k;
// dead[i] the keys with p_ij <= 0.  With zero counts and tail 1 the finishing pass leaves the tail coefficients:
// out_ll[i] = log(1 - sp_i), out_grad[i][k] = -S_k / (1 - sp_i), all 0 where sp_i is not < 1, 0 for a moved parameter.
// Order 2: R2 = 1 + P + P (P + 1) / 2 rows a point -- behind the P + 1 above, at row R2 i + 1 + P + pair(k, l), k <= l row by
// row, c_kl(j) = d_k d_l p_ij / p_ij - (d_k p_ij / p_ij)(d_l p_ij / p_ij), +0.0 at a dead key and throughout where the clamp
// moved k or l -- and out_hess[i][P][P] the tail's second-order coefficients
// -(S_kl / (1 - sp_i) + S_k S_l / (1 - sp_i)^2), S_kl = sum_j d_k d_l p_ij, with the same zeros (not read at order 1).
// partial: ll_deriv_partial_bytes(m, order, n) bytes.  The launch cut is launch_ll_deriv's; not entered in the launch
// record.
hipError_t launch_ll_deriv_table(const DevModel &m, int order, const PointSource &src, int64_t n, double *partial, double *rows,
                                 int32_t *dead, double *out_ll, double *out_grad, double *out_hess, hipStream_t stream);

// ---- K-tp (tp_eval.hip): the truncated-Poisson pmf itself, c_src/covest_poissonmodule.c:7-35 ----
// Modes of the pairs kernel (include/covest_amd.h COVEST_TP_*): the finite value the formula defines (0 below the
// doubles' range, 0 at a rate that is 0 or NaN); the same with +inf where the extension's running long-double product
// overflows (direct_point.h REF_OVF's rule); the exponent itself (-inf where the value mode returns 0 for its rate).
constexpr int kTpValue = 0, kTpReference = 1, kTpLog = 2;
constexpr int64_t kTpMaxPairs = (int64_t)1 << 30; // pairs of one launch
// in: [4][n] doubles = rate | key | ln key! | ln m!, m = min(key, floor(rate)) (anything where rate < 1); out[n].
// K-direct's expressions in K-direct's order, one pair a lane.  One launch, not entered in the launch record.
hipError_t launch_tp_pairs(int mode, int64_t n, const double *in, double *out, hipStream_t stream);
// out[n_l][n_j] = TP(rates[i], key of bin b) in value mode BY THE RECURRENCE (streams.h), along the tiles of `tv`: a
// table built over the key list with counts that are not 0 and bin index = position in the list (tiles_host.cpp).
hipError_t launch_tp_table(const TileView &tv, int64_t n_l, const double *rates, int64_t n_j, double *out,
                           hipStream_t stream);

// ---- K-kmer: k-mer abundance histogram (kmer_count.hip), SURVEY 8(f) row F1 ----
// Open-addressing table in HBM, slots = 2^log2_slots, one 16-byte entry per slot: {key, count}
// (key all-ones = empty).  Key and count share a cache line on purpose: a k-mer costs ONE scattered
// line (relaxed load of the key + atomic add on the neighbouring count), not two.
struct KmerSlot {
    unsigned long long key;
    unsigned long long count;
};
struct KmerTable {
    KmerSlot *slots;
    unsigned long long mask;
    int log2_slots;
    int k; // bases per key (a key's first slot is a function of its minimizer: kmer_count.hip)
};
hipError_t launch_kmer_fill_empty(const KmerTable &t, hipStream_t stream);
// bases: ASCII acgt/ACGT; offsets[n_reads + 1] or nullptr with every read `fixed_len` long.  weights (device, a uint32
// a read) or nullptr: every occurrence of read r is added weights[r] times, and a read of weight 0 adds nothing.
hipError_t launch_kmer_count(const unsigned char *bases, const int64_t *offsets, int64_t n_reads,
                             int64_t fixed_len, int k, int canonical, const KmerTable &t, int *overflow,
                             hipStream_t stream, const uint32_t *weights = nullptr);
// kmer_remove.hip: launch_kmer_count's inverse on the same arguments -- every occurrence of read r is taken out once, or
// weights[r] times; no key is created or cleared.  *underflow (a word of its own, not the overflow word) is set to 1 where
// a key occupies no slot or its count was smaller than what was subtracted.
hipError_t launch_kmer_remove(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t fixed_len, int k,
                              int canonical, const KmerTable &t, int *underflow, hipStream_t stream,
                              const uint32_t *weights = nullptr);
// rehash: the keys HELD by src (kmer_table.h) into dst; stats: {max count, keys held, slots occupied}
hipError_t launch_kmer_rehash(const KmerTable &src, const KmerTable &dst, int *overflow, hipStream_t stream);
hipError_t launch_kmer_stats(const KmerTable &t, unsigned long long *stats, hipStream_t stream);
hipError_t launch_kmer_histogram(const KmerTable &t, unsigned long long *hist, unsigned long long hist_len,
                                 hipStream_t stream);
// kmer_join.hip: out[n_rows][n_cols] (device, zeroed by the call on `stream`) = the keys of a or b by their clipped
// counts in the two (kmer_join.h, whose cells_ok(n_rows, n_cols) the caller has checked); the tables share their k
hipError_t launch_kmer_join(const KmerTable &a, const KmerTable &b, int64_t n_rows, int64_t n_cols, int64_t *out,
                            hipStream_t stream);

// ---- K-kmer, partitioned (kmer_bulk.hip): minimizer buckets of super-k-mer records in HBM, counted in LDS ----
struct KmerBulk {
    int k, m, w;          // k-mer length, minimizer length, m-mers per k-mer (k - m + 1)
    int canonical;
    int log2_buckets;
    int max_run;          // windows per record: 32 - k + 1 (a record holds at most 32 bases)
    int sample;           // pass 0 looks at 1 block of tiles (1 read) in `sample`
    unsigned *sampled;    // [buckets] records pass 0 counted
    typedef unsigned long long fill_t; // (32-bit cursors are no faster -- measured)
    ulonglong2 *ctl;      // [buckets] {first, end}: the bucket's places in recs
    fill_t *fill;         // [buckets] records sent to the bucket (beyond its room: it overflowed, the surplus is in `overflow`)
    ulonglong2 *recs;     // {bases as 2-bit codes, base i at bits 2i; number of bases}
    // the overflow list, in kOvfShards parts with a counter each (ONE counter for all of it saturates at ~90 adds per
    // microsecond: 10 ms for the 9e5 records that overflow at 10 Gbp); a workgroup writes to the part of its number
    ulonglong2 *overflow;          // [kOvfShards][overflow_cap]
    unsigned long long *ovf_count; // [kOvfShards * kOvfStride] records sent to a part (beyond overflow_cap: lost -- the
                                   // caller starts over); a counter per 128-byte line
    unsigned long long overflow_cap; // per part
};
// The two control blocks of a call, as the host reserves and names them (the launch functions take pointers to their
// members).  BulkControl: zeroed before pass 0; the one-length probe of reads with offsets borrows its first word before.
struct BulkControl {
    unsigned long long one_length;   // the probe's flag: 1 on entry, 0 unless every read is as long as the first
    unsigned long long pad0_;
    unsigned long long room;         // pass 0: records the buckets were given places for, in all
    unsigned long long pad1_;
    unsigned long long stats[4];     // pass 2: see launch_kmer_bucket_count
    unsigned long long pad2_[8];
    unsigned long long ovf_count[kOvfShards * kOvfStride]; // KmerBulk::ovf_count, on 128-byte lines of their own
};
static_assert(offsetof(BulkControl, one_length) == 0 && offsetof(BulkControl, room) == 16 &&
                  offsetof(BulkControl, stats) == 32 && offsetof(BulkControl, ovf_count) == 128 &&
                  sizeof(BulkControl) == (16 + kOvfShards * kOvfStride) * 8,
              "BulkControl: the layout kmer_bulk.hip's kernels were measured with");
// BulkLists: the head is zeroed before pass 2; the two lists of bucket numbers, [buckets] words each, lie behind it.
struct BulkLists {
    unsigned later_n;                // buckets the wave-per-bucket kernel left to the workgroup-per-bucket one
    unsigned pad0_;
    unsigned long long to_table[2];  // buckets no LDS table could hold, and their k-mer occurrences
    unsigned pad1_[2];
    unsigned *later_list() { return reinterpret_cast<unsigned *>(this + 1); }
    unsigned *to_table_list(size_t n_buckets) { return later_list() + n_buckets; }
    static size_t bytes(size_t n_buckets) { return sizeof(BulkLists) + 2 * n_buckets * sizeof(unsigned); }
};
static_assert(offsetof(BulkLists, later_n) == 0 && offsetof(BulkLists, to_table) == 8 && sizeof(BulkLists) == 32,
              "BulkLists: later_list at byte 32, to_table_list at 32 + 4 * buckets");
// offsets != nullptr: reads of any length -- base0 = offsets[0], total_bytes = offsets[n_reads] - base0, first_read: room
// for kmer_plan::ragged_tiles(total_bytes, p.w) words
hipError_t launch_kmer_scatter(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t fixed_len,
                               int64_t base0, int64_t total_bytes, unsigned *first_read, const KmerBulk &p, bool count_only,
                               hipStream_t stream);
hipError_t launch_kmer_place_buckets(const KmerBulk &p, unsigned long long *partial, unsigned long long *total,
                                     hipStream_t stream);
// stats: [0] max count, [1] distinct keys, [2] entries of `big` (counts >= hist_len), [3] records pass 1 sent
// later: [0] buckets the wave-per-bucket kernel left to the workgroup-per-bucket one, later_list: [buckets]
// to_table: [0] buckets no LDS table could hold, [1] their k-mer occurrences, to_table_list: [buckets]
hipError_t launch_kmer_bucket_count(const KmerBulk &p, unsigned long long *hist, unsigned long long hist_len,
                                    unsigned long long *stats, unsigned long long *big, unsigned long long big_cap,
                                    unsigned *later, unsigned *later_list, unsigned long long *to_table, unsigned *to_table_list,
                                    bool small_buckets, int n_cu, hipStream_t stream);
// out[0] (1 on entry) = 0 unless every read is offsets[1] - offsets[0] bases long (n_reads >= 1)
hipError_t launch_kmer_one_length(const int64_t *offsets, int64_t n_reads, unsigned long long *out, hipStream_t stream);
// `ops` (rounded up to 64 per thread) returning atomic adds at pseudo-random places of words[slots]
hipError_t launch_kmer_scatter_rate(unsigned long long *words, unsigned long long slots, long long ops, unsigned long long *sink,
                                    hipStream_t stream);
// the overflow list's records and the listed buckets' into the table in HBM
hipError_t launch_kmer_to_table(const KmerBulk &p, bool any_overflowed, const KmerTable &t, int *overflow,
                                const unsigned long long *to_table, const unsigned *to_table_list, hipStream_t stream);

// ---- K-kmer for k > 31 (kmer_wide.hip): keys of w = 2, 4 or 8 words, slots of `stride` words {state/count, key[w]} ----
struct KmerWideTable {
    unsigned long long *words;
    unsigned long long mask; // slots - 1
    int log2_slots;
    int k;
    int w;      // 64-bit words per key
    int stride; // words per slot: 4, 8 or 16
};
hipError_t launch_kmer_wide_clear(const KmerWideTable &t, hipStream_t stream);
hipError_t launch_kmer_wide_count(const unsigned char *bases, const int64_t *offsets, int64_t n_reads, int64_t fixed_len,
                                  int canonical, const KmerWideTable &t, int *overflow, hipStream_t stream,
                                  const uint32_t *weights = nullptr); // (weights: as launch_kmer_count's)
hipError_t launch_kmer_wide_rehash(const KmerWideTable &src, const KmerWideTable &dst, int *overflow, hipStream_t stream);
hipError_t launch_kmer_wide_stats(const KmerWideTable &t, unsigned long long *stats, hipStream_t stream);
hipError_t launch_kmer_wide_histogram(const KmerWideTable &t, unsigned long long *hist, unsigned long long hist_len,
                                      hipStream_t stream);

// ---- K-thin: expected histogram after down-sampling by `factor` (thin_hist.hip), SURVEY 8(f) row F3 ----
struct ThinSource {
    int32_t i;     // source count
    int32_t pad;
    double count;  // its multiplicity h_i
    double a;      // i < 100: ln i!            i >= 100: ln(i / factor)
    double b;      // i < 100: unused           i >= 100: i / factor
};
// src[n] and lgam[m] = ln m! (m = 0 .. max(max key, out_len)) on the device; partial needs
// thin_hist_chunks() * out_len doubles; out[j-1], j = 1..out_len.
int thin_hist_chunks();
hipError_t launch_thin_hist(const ThinSource *src, int64_t n, const double *lgam, double factor, int64_t out_len,
                            double *partial, double *out, hipStream_t stream);

// ---- K-sim: the read simulator (sim_reads.hip; tools/simulator/ of the reference) ----
// out[n]: a random genome, upper-case ASCII.  Any alignment of `out`.
hipError_t launch_random_genome(int64_t n, uint64_t seed, unsigned char *out, hipStream_t stream);
// out[n_reads * read_len]: reads first_read .. first_read + n_reads of the stream of `seed`, back to back; origin
// (or nullptr)[n_reads] = pos << 1 | forward.  thr = floor(error_rate * 2^32), 2^32 included.  Any alignment of `out`;
// nothing outside the two arrays is written.  One launch per 4 GiB of output.
hipError_t launch_sim_reads(const unsigned char *genome, int64_t genome_len, int read_len, int64_t first_read,
                            int64_t n_reads, uint64_t thr, uint64_t seed, int both_strands, unsigned char *out,
                            int64_t *origin, hipStream_t stream);

// ---- K-repeat: a genome whose units are copies of families (sim_repeats.hip) ----
// out[n]: unit u = i / unit_len of the genome is family plan[u] >> 1, forward iff plan[u] & 1, substituted at
// thr = floor(divergence * 2^32) (2^32 included; 0: no divergence block is computed).  plan[ceil(n / unit_len)] on the
// device, entries >= 0 with (f + 1) * unit_len within 63 bits.  Any alignment of `out`; nothing outside it is written.
// One launch per 4 GiB of output.
hipError_t launch_repeat_genome(const int64_t *plan, int unit_len, int64_t n, uint64_t thr, uint64_t seed,
                                unsigned char *out, hipStream_t stream);

// ---- K-draw: replicate histograms drawn from a weight vector (draw_hist.hip) ----
// out[n_rep * m] (int64, overwritten: zeroed on `stream` first): row b - first_rep counts the draws d < n of replicate
// b by cell, the cell of a draw being #{i <= m - 2 : thr[i] <= u} (include/covest_amd.h).  thr[m] ascending, on the
// device.  1 <= m <= kDrawMaxCells, first_rep + n_rep <= 2^32; nothing outside out[0 .. n_rep * m) is written.
constexpr int kDrawMaxCells = 65536;      // the cap on m (COVEST_DRAW_MAX_CELLS of the header)
constexpr int kDrawLdsBothCells = 12288;  // up to here thresholds AND counters live in LDS (12 bytes a cell)
constexpr int kDrawLdsThrCells = 16384;   // up to here the thresholds do; beyond, they are read through L2
constexpr int kDrawGuideBits = 11;        // the guide table is indexed by the top 11 bits of a 63-bit draw
constexpr int kDrawGuide = 1 << kDrawGuideBits;
constexpr long long kDrawChunk = 1 << 17; // draws a workgroup takes
hipError_t launch_draw_hist(const uint64_t *thr, int64_t m, int64_t n, uint64_t first_rep, int64_t n_rep, uint64_t seed,
                            int64_t *out, hipStream_t stream);

// ---- K-batch: many histograms on one key set (ll_batch.hip) ----
// LL_b(theta_i) = sum_j h_bj log p_j(theta_i) + tail_b [sp_i < 1] log(1 - sp_i): p is evaluated once per point, into a
// table of log p over ALL keys, and the histograms enter through one fp64 contraction (v_mfma_f64_16x16x4_f64).
constexpr int64_t kBatchTableBytes = (int64_t)256 << 20; // the table of one chunk of points (the host loops over chunks)
constexpr int64_t kBatchMaxHist = (int64_t)1 << 20;      // histograms of a batch (the contraction's grid y stays < 65536)
// The table of n points (a list: src.params, src.t_list): one wave a point runs direct_point_ll<P, true> on `m`, whose
// bins must be the all-keys view with a zero count array and whose tail must be 1.  table[i][j] (row-major, n_keys a
// row) = log p_ij, +0.0 where p_ij <= 0 (such keys counted in dead[i]; a p_ij of exactly 1 is stored as -0.0, so that
// the bits of +0.0 mean "dead" and nothing else), NaN where p_ij is NaN; tl[i] = log(1 - sp_i) or 0.  keep_p: the row
// stays p_ij itself (what covest_probabilities(clamp = 1) returns), dead and tl as above.
hipError_t launch_batch_table(const DevModel &m, const PointSource &src, int64_t n, double *table, double *tl,
                              int32_t *dead, bool keep_p, hipStream_t stream);
// out[b * ld + i] = sum_j H[b][j] table[i][j] + tails[b] tl[i] for b < n_hist, i < n; H is n_hist x n_keys, row-major.
// Returns in *tiles (nullptr: not wanted) the 16 x 16 output tiles the launches cover.
hipError_t launch_batch_cross(const double *H, const double *tails, int64_t n_hist, const double *table, const double *tl,
                              int64_t n, int64_t n_keys, double *out, int64_t ld, int64_t *tiles, hipStream_t stream);
// One wave per (b, k): point i = dead_list[k] of the table has keys with p <= 0; where histogram b counts one of them
// (h_bj != 0), out[b * ld + i] = -inf unless it is NaN already.
hipError_t launch_batch_fix_dead(const double *H, int64_t n_hist, const double *table, int64_t n_keys,
                                 const int32_t *dead_list, int64_t n_dead, double *out, int64_t ld, hipStream_t stream);
// out[i * R + q] = sum_j H[index[i]][j] rows[i * R + q][j] + tails[index[i]] tc[i * R + q], one wave a request: the R dot
// products in one sweep over the keys; the dead-key rule inline (value -inf), and where the value is not finite the
// R - 1 derivative entries NaN.  R is 1 (the value form: rows and tc are launch_batch_table's table and tl) or, for the
// gradient's and the Hessian's tables below, 3 or 6, or 21 (the repeat model's second-order table; the basic model's has
// 6).
hipError_t launch_batch_pairs(const double *H, const double *tails, const int64_t *index, const double *rows,
                              const double *tc, int64_t n, int64_t n_keys, int rows_per_point, double *out,
                              hipStream_t stream);
// ---- the gradient and the Hessian of a batch (DESIGN.md sections 6u, 6x): `rows` is launch_ll_deriv_table's, R = P + 1
// or 1 + P + P (P + 1) / 2 rows a point ----
// tc[i * R + q] from the finishing pass's out_ll[i] (q = 0), out_grad[i][q - 1] (q <= P) and, where R > P + 1, the upper
// triangle of out_hess[i][P][P], k <= l row by row (fin_hess is not read otherwise): the array launch_batch_cross takes for
// tl when the table has R n rows.
hipError_t launch_batch_tail_pack(const double *fin_ll, const double *fin_grad, const double *fin_hess, int64_t n, int n_par,
                                  int rows_per_point, double *tc, hipStream_t stream);
// out is n_hist x (n * R) with row length ld (launch_batch_cross over R n rows, then launch_batch_fix_dead with the dead
// points' VALUE rows listed): where out[b * ld + i * R] is not finite, the R - 1 entries behind it become NaN.
hipError_t launch_batch_grad_specials(int64_t n_hist, int64_t n, int rows_per_point, double *out, int64_t ld,
                                      hipStream_t stream);
// Per histogram b, over ll[b * ld + i], i < n: the first i with the strictly smallest -ll (NaN never wins) against the
// running (run_val[b], run_idx[b]) of the chunks before, which a later chunk only beats with a strictly smaller value;
// a winner is stored as first + i.  Start the running pair at (+inf, -1).
hipError_t launch_batch_argmin(const double *ll, int64_t ld, int64_t n_hist, int64_t n, int64_t first, double *run_val,
                               int64_t *run_idx, hipStream_t stream);
hipError_t launch_batch_argmin_init(int64_t n_hist, double *run_val, int64_t *run_idx, hipStream_t stream);
// The rows of a draw (draw_hist.hip: n_hist x m int64, m = n_keys + has_tail) as double counts H[n_hist][n_keys] and
// tails[n_hist] (the last cell with a tail, else 0).
hipError_t launch_batch_from_draw(const int64_t *draw, int64_t n_hist, int64_t n_keys, bool has_tail, double *H,
                                  double *tails, hipStream_t stream);

} // namespace covest
