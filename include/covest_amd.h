/*
 * covest_amd.h -- C ABI of the MI355X (gfx950) likelihood grid-search library.
 *
 * This is the drop-in boundary for ONE path of mhozza/covest: the truncated-
 * Poisson mixture log-likelihood evaluated over a parameter grid and reduced to
 * its arg-min.  Plain C, caller-owned buffers, integer status codes, no torch or
 * C++ types.  Every entry point cites the reference interface it replaces
 * (paths relative to the reference checkout, v0.5.6).  The ctypes binding a
 * maintainer adds on the reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *   - All functions return 0 on success, a negative COVEST_E_* code on failure;
 *     covest_last_error() returns a thread-local message for the last failure.
 *   - Numeric outcomes are in-band IEEE values exactly as the reference returns
 *     them: -inf when a non-zero bin has p_j == 0 (covest/utils.py:32-35), NaN
 *     propagates, parameters outside the model bounds are clamped, never
 *     rejected (covest/models.py:60-69).
 *   - The library copies the histogram to the device at create time and keeps no
 *     pointer of the caller's past any call.
 *   - There is NO CPU fallback: without a usable HIP device every compute entry
 *     point fails with COVEST_E_NO_DEVICE.
 *   - A model handle is immutable after create; calls on one handle are
 *     serialised internally, distinct handles are independent.
 */
#ifndef COVEST_AMD_H
#define COVEST_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COVEST_ABI_VERSION 1

#define COVEST_MODEL_BASIC 0   /* covest/models.py:17  BasicModel   (coverage, error_rate)          */
#define COVEST_MODEL_REPEATS 1 /* covest/models.py:173 RepeatsModel (coverage, error_rate, q1,q2,q) */
#define COVEST_MAX_PARAMS 5
#define COVEST_MAX_ERROR_CLASSES 64

#define COVEST_OK 0
#define COVEST_E_INVALID (-1)   /* bad argument */
#define COVEST_E_NO_DEVICE (-2) /* no HIP device / HIP runtime error at init */
#define COVEST_E_HIP (-3)       /* HIP runtime error during a call */
#define COVEST_E_NOMEM (-4)
#define COVEST_E_UNSUPPORTED (-5) /* the request is valid but this entry point does not serve it (another one does) */

/* Kernel selection for covest_grid_eval / covest_eval_points (mostly for tests
 * and benchmarks; AUTO picks the fastest kernel valid for the request). */
#define COVEST_KERNEL_AUTO 0
#define COVEST_KERNEL_DIRECT 1   /* one wavefront per grid point, one exp per pmf term        */
#define COVEST_KERNEL_RECUR 2    /* one wavefront per grid point, pmf recurrence along j      */
#define COVEST_KERNEL_FACTORED 3 /* repeats, dense grids: (c,e)-outer / (q1,q2,q)-inner reuse */
/* K-direct with the reference's long-double OVERFLOW reproduced: truncated_poisson (c_src/covest_poissonmodule.c:19-24)
 * forms its whole product before scaling and returns +inf once it passes LDBL_MAX, the likelihood becomes +inf / NaN
 * (covest/models.py:100-107) and optimize_grid would select -(+inf) (covest/grid.py:65-70).  The other kernels
 * return the finite value the formula defines; this one returns what the reference returns, specials included. */
#define COVEST_KERNEL_DIRECT_REF 4

typedef struct covest_model covest_model; /* opaque */
typedef struct covest_grid covest_grid;   /* opaque */

/* Arguments of the reference model constructors:
 *   BasicModel.__init__   covest/models.py:19-31
 *   RepeatsModel.__init__ covest/models.py:175-183
 * `comb[s]` is the reference's self.comb[s] = comb(k, s) * 3**s (models.py:25),
 * passed in so that the caller's scipy decides its rounding, as in the reference.
 * `lo/hi` are self.bounds; NaN stands for Python None. */
typedef struct {
    int32_t kind;   /* COVEST_MODEL_* */
    int32_t k;      /* k-mer size */
    int32_t r;      /* read length */
    int32_t n_err;  /* self.max_error = min(k + 1, max_error): error classes summed, 1..64 */
    const double *comb;    /* [n_err] */
    int64_t n_keys;        /* len(hist) */
    const int32_t *keys;   /* hist keys j in dict order (zero-count keys included) */
    const double *counts;  /* hist values h_j as doubles */
    double tail;           /* self.tail */
    double lo[COVEST_MAX_PARAMS];
    double hi[COVEST_MAX_PARAMS];
    double threshold;      /* RepeatsModel threshold (1e-8) */
    int32_t has_threshold; /* 0: threshold is None */
    int32_t device;        /* HIP device ordinal; -1 = the calling thread's current device */
} covest_model_desc;

/* Library / device probes (no reference counterpart). */
int covest_abi_version(void);
int covest_device_count(void); /* >= 0, or COVEST_E_NO_DEVICE */
const char *covest_last_error(void);

/* Model(k, r, hist, tail, max_error=, max_cov=, ...): covest/covest.py:136-140. */
int covest_model_create(const covest_model_desc *desc, covest_model **out);
void covest_model_destroy(covest_model *m);
int covest_model_param_count(const covest_model *m); /* BasicModel.param_count, models.py:40-42 */
/* number of histogram bins the kernels evaluate: all keys when tail != 0, else
 * only keys with a non-zero count (the tail term of models.py:104 is then 0). */
int64_t covest_model_bins_evaluated(const covest_model *m);

/* RepeatsModel.get_hist_threshold(get_b_o(q1,q2,q), threshold): models.py:185-208.
 * q123 is [n][3] (already clamped to the model bounds); out[n]; hist_max is
 * max(self.hist); has_threshold == 0 stands for threshold None.  Pure host code
 * (no device needed): computed with libm pow, as Python does, so that the
 * integer cut-off cannot differ from the reference by a device ulp. */
int covest_threshold_o(int64_t n, const double *q123, double threshold, int32_t has_threshold,
                       int32_t hist_max, int32_t *out);

/* model.compute_loglikelihood(*params) for a list of points: covest/models.py:100-107,
 * batched like compute_loglikelihood_multi (models.py:109-117).
 * params is [n][param_count] on the HOST; out_ll[n] on the HOST.
 * COVEST_KERNEL_AUTO: basic model -> the recurrence kernel; repeats model -> up to 4096 points go to the
 * factored kernel's list mode (one workgroup per point and key segment, points whose threshold_o exceeds 513 in
 * chunks of 512 copy numbers: the latency path of scipy-driven refinements, ~85 us for one point), longer lists
 * to the direct kernel.  Within either range a point's value does not depend on what else is in the call. */
int covest_eval_points(covest_model *m, int64_t n, const double *params, double *out_ll,
                       int32_t kernel);

/* The same values and, beside them, the ANALYTIC gradient of the log-likelihood in the model's parameters: the
 * gradient of what the kernels evaluate, at the point after fit_to_bounds, with threshold_o held fixed (DESIGN.md
 * section 6e).  HOST arrays: params [n][param_count], out_ll[n], out_grad[n][param_count].  A component whose
 * parameter fit_to_bounds moved is 0 (the function is constant there); where the value is not finite every component
 * is NaN.  One kernel for both models (ll_deriv.hip, order 1) and a small finishing launch; a point's numbers do not depend on
 * what else is in the call. */
int covest_eval_points_grad(covest_model *m, int64_t n, const double *params, double *out_ll, double *out_grad);

/* Values, the analytic gradient and, beside them, the HESSIAN of the log-likelihood in closed form: second derivatives
 * of the same function (what the kernels evaluate, at the point after fit_to_bounds, threshold_o held fixed; DESIGN.md
 * section 6f).  HOST arrays: params [n][param_count], out_ll[n], out_grad[n][param_count],
 * out_hess[n][param_count][param_count].  The matrix is symmetric bit for bit (the upper triangle is computed and
 * mirrored).  A row and column whose parameter fit_to_bounds moved are 0, and so is that gradient component; where the
 * value is not finite every entry of gradient and Hessian is NaN.  One kernel for both models (ll_deriv.hip, order 2) and a small
 * finishing launch, neither entered in the launch record; a point's numbers do not depend on what else is in the
 * call.  Meant to be asked once per fit (the observed information at the optimum), not inside a search. */
int covest_eval_points_hess(covest_model *m, int64_t n, const double *params, double *out_ll, double *out_grad,
                            double *out_hess);

/* Values, the analytic gradient (the same bits covest_eval_points_grad returns) and, beside them, the OUTER PRODUCT OF
 * THE SCORES, the meat of the sandwich (robust) covariance A^-1 B A^-1: with
 * r_k(j) = d_k p_j / p_j, sp = sum_j p_j, S_k = sum_j d_k p_j over the evaluated keys and on = [tail != 0 and sp < 1],
 *     B_kl = sum_{h_j != 0} h_j r_k(j) r_l(j)  +  on tail S_k S_l / (1 - sp)^2,
 * the uncentred sum over k-mers of the outer product of their scores, the tail as one more class; of the function
 * covest_eval_points_grad differentiates.  HOST arrays: params [n][param_count], out_ll[n], out_grad[n][param_count],
 * out_opg[n][param_count][param_count].  The matrix is symmetric bit for bit (the upper triangle is computed and
 * mirrored).  A row and column whose parameter fit_to_bounds moved are 0; where the value is not finite every entry of
 * gradient and matrix is NaN.  The order-1 walk of ll_deriv.hip with one product per parameter pair in each key's
 * epilogue, and a small finishing launch, neither entered in the launch record; a point's numbers do not depend on
 * what else is in the call.  The unit is one distinct k-mer counted as independent of the others: B corrects the
 * covariance for misfit of the mixture, not for dependence between overlapping k-mers. */
int covest_eval_points_opg(covest_model *m, int64_t n, const double *params, double *out_ll, double *out_grad,
                           double *out_opg);

/* Documented divergence made visible: the reference forms its pmf product in x87 long double BEFORE
 * scaling it (c_src/covest_poissonmodule.c:19-24), so for large rates against large keys
 * (ln(l^i / i!) > 11356.5 at i = min(j, floor(l))) truncated_poisson returns +inf, the likelihood
 * becomes +inf or NaN, and optimize_grid would select it (covest/grid.py:65-70).  This library
 * returns the finite value the formula defines.  flags[i] = 1 where the reference itself would have
 * overflowed at params[i] (HOST arrays, [n][param_count] and [n]); pure host arithmetic, no device
 * work.  No benchmark configuration contains such a point. */
int covest_reference_overflow(const covest_model *m, int64_t n, const double *params, uint8_t *flags);

/* ---- the pmf itself: covest_poisson.truncated_poisson(l, j), c_src/covest_poissonmodule.c:7-35 ----
 * The function every likelihood value above is a mixture of, on its own.  No model handle;
 * HOST arrays owned by the caller; device < 0 = the calling thread's current device.
 *   COVEST_TP_VALUE      the finite value the formula defines: 0 where it lies below the doubles' range, never inf;
 *                        0.0 where l == 0 or l is NaN (:15), and for a negative l (no rate: the kernels' `x > 0`)
 *   COVEST_TP_REFERENCE  the same, but +inf exactly where the extension's running long-double product overflows
 *                        (:19-24; the rule of COVEST_KERNEL_DIRECT_REF): what the extension returns
 *   COVEST_TP_LOG        the logarithm of that value before the last exp: finite wherever l > 0 -- also where the
 *                        value underflows and where the extension overflows --, -inf where the value modes return 0
 *                        for the rate's sake
 * covest_truncated_poisson: out[i] = TP(l[i], j[i]), one pair a lane, the likelihood kernels' term-by-term arithmetic
 * (K-direct's), ln j! from the host's long-double table.  j >= 1, at most 4194304 (COVEST_E_INVALID otherwise, and
 * for an unknown mode or more than 2^30 pairs); n == 0 returns COVEST_OK without touching the device.  A pair's bits
 * do not depend on what else is in the call.
 * covest_truncated_poisson_table: out[n_l][n_j] (row-major) = TP(l[i], j[b]) in COVEST_TP_VALUE mode BY THE RECURRENCE
 * the fast likelihood kernels walk (one multiply a key along tiles of <= 32 keys, anchored by one exp where a rate's
 * terms enter the doubles' range): j strictly ascending integers in 1..16384, COVEST_E_INVALID otherwise. */
#define COVEST_TP_VALUE 0
#define COVEST_TP_REFERENCE 1
#define COVEST_TP_LOG 2
int covest_truncated_poisson(int32_t device, int64_t n, const double *l, const int64_t *j, int32_t mode, double *out);
int covest_truncated_poisson_table(int32_t device, int64_t n_l, const double *l, int64_t n_j, const int64_t *j, double *out);

/* ---- DIAGNOSTIC: the scalar primitives under the kernels, one element a thread (csrc/math_probe.hip) ----
 * Not part of the model's interface: it exists so that tests can hold the hand-written device math (csrc/fastmath.h,
 * point_fetch.h, grad_common.h) to a reference on its own.  out[i] = fn(x[i], y[i], z[i], iarg[i]) in one launch of
 * 256-thread workgroups; HOST arrays of n elements, n <= 65536; an array `fn` does not read may be NULL.  `fn`:
 *    0 exp_fast(x)                 1 exp_scaled(x, iarg), |iarg| <= 2048     2 the device library's exp(x)
 *    3 exp_neg_rn(x)               4 fast_log(x)                             5 fast_log_n<4>(x)
 *    6 fast_log_bits_n<1, 5, kBasicShift>(x)        7 fast_log_bits_n<4, 5, kScaleBits>(x)
 *    8 fast_log_bits_n<4, 3, kScaleBits, RAW>(x)    9 fast_log_bits_n<4, 4, kScaleBits>(x)
 *   10 log_trunc_norm(x, y), y = log x             11 the same with the log table
 *   12 trunc_norm_dlog(x)         13, 14 the first and the second output of trunc_norm_dlog2(x)
 *   15 error_class_rate(c = x, e = y, s = iarg)    16, 17 error_class_rate_mul(.., S = 8, 16)
 *   18, 19 error_class_rates<8>, <16>(c = x, e = y)[s = iarg]   -- all five on a model of (k, r), 1 <= k <= 63, r >= k
 *   20 copy_number_weight(q1 = x, q2 = y, q = z, o = iarg)      21 copy_number_weight_by_squaring, 1 <= o <= 16384
 * In 5 and 7 .. 9 a thread takes four consecutive elements, as the kernels do.  k and r are read by 15 .. 19 only.
 * COVEST_E_INVALID: an unknown fn, n outside 0 .. 65536, a NULL array that fn reads, an iarg outside the range above
 * (a class: 0 .. S - 1; 15: 0 .. 63).  n == 0: COVEST_OK, nothing launched.  Enters no launch record. */
int covest_math_probe(int32_t device, int32_t fn, int64_t n, const double *x, const double *y, const double *z,
                      const int32_t *iarg, int32_t k, int32_t r, double *out);

/* model.compute_probabilities(*params): models.py:81-98, :211-242.  out_p[n_keys]
 * in key order (host).  clamp != 0 applies fit_to_bounds first, which is how
 * compute_loglikelihood calls it (models.py:101-102); clamp == 0 is the raw
 * method as plot_probs calls it.  Used by --plot and by the parity tests. */
int covest_probabilities(covest_model *m, const double *params, int32_t clamp, double *out_p);

/* ---- what the fitted mixture says about the k-mers of abundance j: posterior classes, in the log domain ----
 * (DESIGN.md section 6ab).  The shares are the terms of the sum compute_probabilities adds up, before they are added.
 * A point is params[i][param_count], taken as given (clamp == 0) or clamped as fit_to_bounds clamps it (clamp != 0:
 * the meaning it has in covest_probabilities).  S = max_error classes; T = threshold_o of the point by the host rule of
 * covest_threshold_o (of the clamped point where clamp != 0), T = 2 in the basic model: one copy number, b_1 = 1.  With
 * x_os = o l_s, and a_os and b_o exactly as models.py:77, 87-90, 194-206, 221-233 forms them (1.0 - exp(-x), not expm1,
 * and fix_zero included), for every key j of the model, all keys, in the order of model.hist:
 *   ln w_os(j) = ln b_o + ln a_os + j ln x_os - D(x_os) - ln j!      (-inf where a_os b_o = 0 or x_os = 0)
 *   ln p_j     = logsumexp over (o, s) of ln w_os(j)
 *   E_s(j)     = sum_o w_os(j) / p_j        s = 0 .. S-1      error share: the k-mer has s wrong bases
 *   C_o(j)     = sum_s w_os(j) / p_j        o = 1 .. T-1      copy share
 *   M(j)       = sum_o o C_o(j)                               mean copy number
 * D is the reference's normaliser (c_src/covest_poissonmodule.c:20,25-31).  Each of the three is formed as
 * sum exp(ln w - max) over its own sum, never by a division by a p_j held as a double, so a share exists where p_j
 * itself is subnormal or 0 in double; each family is normalised by its own total.  These are shares of the model as
 * the reference evaluates it: a class whose 1.0 - exp(-x) is 0 in double has share exactly 0.
 * The copy shares come in copy_columns = Cc >= 1 columns: columns 0 .. Cc-2 are o = 1 .. Cc-1, the last column is
 * everything from o = Cc on; where T - 1 < Cc the columns beyond T - 1 are 0.  A key at which every component is -inf
 * has ln p_j = -inf, and NaN shares and NaN mean copy number: no posterior exists there.  The tail cell (mass at or
 * beyond the trim) is not covered: only keys are.
 * HOST arrays; an output that is NULL is not computed for the caller, the others do not change by it.  A point's numbers
 * do not depend on what else is in the call.  COVEST_E_INVALID for each of: a null model; n < 0; n > 0 with null params;
 * copy_columns < 1 or > 65536; all four outputs null with n > 0.  n == 0 or a model with no keys: COVEST_OK, nothing
 * written.  Two launches per chunk of points (posterior.hip), not entered in the launch record. */
int covest_posterior_classes(covest_model *m, int64_t n, const double *params, int32_t clamp, int32_t copy_columns,
                             double *out_log_p,        /* [n][n_keys]            or NULL */
                             double *out_error_share,  /* [n][n_keys][S]         or NULL */
                             double *out_copy_share,   /* [n][n_keys][Cc]        or NULL */
                             double *out_mean_copies); /* [n][n_keys]            or NULL */
/* The same call with the points walked in chunks of at most chunk_points (0: the library's own choice, which bounds the
 * device memory of a call; negative: COVEST_E_INVALID).  The chunk changes no number: it is here so that the chunk edge
 * can be tested on a short list. */
int covest_posterior_classes_chunked(covest_model *m, int64_t n, const double *params, int32_t clamp, int32_t copy_columns,
                                     int64_t chunk_points, double *out_log_p, double *out_error_share,
                                     double *out_copy_share, double *out_mean_copies);

/* Dense grid = itertools.product(*axes), last axis fastest (covest/grid.py:39-43,
 * notebooks/VisualiseLikelihood.ipynb cell 5).  n_axes must equal param_count; a
 * fixed parameter is an axis of length 1 (covest/grid.py:27-28).  The handle
 * evaluates flat indices [flat_begin, flat_end) of the product -- one contiguous
 * block per GPU (multi-GPU block partition); pass 0 and -1 for the whole grid.
 * Axes are copied to the device here.  A grid borrows its model: destroy the grid first. */
int covest_grid_create(covest_model *m, int32_t n_axes, const double *const *axes,
                       const int64_t *axis_len, int64_t flat_begin, int64_t flat_end,
                       covest_grid **out);
void covest_grid_destroy(covest_grid *g);
/* Give an existing handle other axes and/or another block (same meaning of the arguments as
 * covest_grid_create): the iterations of covest/grid.py:56-74 evaluate a new grid each time, and a
 * handle keeps its device memory.  Waits for the handle's last evaluation; what it uploads (axes, threshold_o
 * table, K-factored's plan) is staged in page-locked memory of the handle and copied asynchronously on the default
 * stream -- the next covest_grid_eval queues up behind the copies (on another stream: behind an event). */
int covest_grid_reset(covest_grid *g, int32_t n_axes, const double *const *axes, const int64_t *axis_len,
                      int64_t flat_begin, int64_t flat_end);
int64_t covest_grid_size(const covest_grid *g); /* flat_end - flat_begin */

/* Evaluate LL at every point of the block into a device buffer owned by the
 * handle and reduce it to (min -LL, lowest flat index attaining it) on the
 * device.  Asynchronous on `stream` (a hipStream_t, NULL = default stream).
 * Replaces the Pool.map + scan of covest/grid.py:63-70. */
int covest_grid_eval(covest_grid *g, int32_t kernel, void *stream);

/* THE STRICT RE-EVALUATION IS PUT OFF.  The recurrence kernels hand a few points back for a strict, term-by-term pass that
 * corrects their values (at most downwards: it adds non-positive terms).  A plain covest_grid_eval launches the
 * likelihood kernel and an arg-min that PROVES its winner against the handed-back points' provisional values, and
 * leaves the pass out; whatever exposes the values or describes the launches -- covest_grid_ll_host,
 * covest_grid_ll_device, covest_grid_axis_min, covest_grid_launch_record, covest_grid_argmin_pair_device -- runs it first
 * (and the arg-min again), so that they see exactly what an evaluation with the pass inside leaves, bit for bit.
 * covest_grid_argmin runs it only where the winner could not be proven.  covest_grid_eval_scan keeps the pass inside.
 * covest_grid_complete does it by hand: the pass and the arg-min on the evaluation's stream, asynchronously; nothing
 * if nothing is owed.  covest_grid_fix_eager(g, 1) keeps the pass inside every evaluation of the handle from then on
 * (0: puts it off again); covest_grid_argmin_pair_device switches a handle to that by itself.
 * covest_grid_ll_provisional_host, a diagnostic for the tests: the values as they are while the pass is owed;
 * COVEST_E_INVALID if none is. */
int covest_grid_complete(covest_grid *g);
int covest_grid_fix_eager(covest_grid *g, int32_t eager);
int covest_grid_ll_provisional_host(covest_grid *g, double *out_ll);

/* Wait for the last covest_grid_eval and return the reduction.  Selection is the
 * scan of covest/grid.py:65-70 with maximize=False starting from +inf: strict <,
 * lowest GLOBAL flat index wins ties, NaN never wins; argmin -1 if nothing is
 * < +inf. */
int covest_grid_argmin(covest_grid *g, double *min_negll, int64_t *argmin_flat);

/* The same selection PER CELL of the product of the axes named in keep_mask (bit d set = axis d is kept), over the
 * other axes, of the last evaluation: for every cell -- row-major in the kept axes' original order, n_cells = the
 * product of their lengths -- min -LL over the points of the handle's block that fall in the cell and the GLOBAL flat
 * index of the lowest-index point attaining it; (+inf, -1) where no point of the block in the cell is < +inf, cells
 * the block does not touch included.  keep_mask 0 is covest_grid_argmin's pair; all axes kept is -LL itself.  Waits
 * for the last covest_grid_eval, reduces on its stream and copies the pairs to the HOST arrays (n_cells entries
 * each); the LL buffer, the arg-min pair and the scan's records stay as they are, and any number of masks may be
 * asked of one evaluation.  COVEST_E_INVALID: no evaluation on this handle since it was created or reset, a mask bit
 * at or above n_axes, n_cells not that product.  The pairs of the blocks of one grid combine with the same rule
 * (covest_amd.grid.merge_axis_minima). */
int covest_grid_axis_min(covest_grid *g, uint32_t keep_mask, int64_t n_cells, double *min_negll, int64_t *argmin_flat);

/* covest_grid_eval and, in the same arg-min launch, the SELECTION SCAN of covest/grid.py:65-70 started from the
 * minimum the caller holds (`start_min`: what optimize_grid's `min_val` is when an iteration begins, :49,67-69):
 *     if sgn * val < min_val: diff += min_val - val; min_val = sgn * val; min_args = args
 * changes its state exactly at the strict running-minimum records below start_min, taken in flat-index order -- a
 * handful of points once a search is under way.  The device lists them (page-locked host memory, the kernel's own
 * stores) and covest_grid_scan hands them over: index[i] (GLOBAL flat index, ascending) and negll[i] = -LL there,
 * so the caller replays the loop over those alone instead of reading every value back (covest_grid_ll_host).
 * *truncated != 0: the list is incomplete (more records than `cap` or than the device keeps -- 120 --, a block beyond
 * 16384 points, or the last evaluation was a plain covest_grid_eval): read the values back instead.  A NaN never
 * passes `<`, as in the reference.  maximize=False only (sgn = 1). */
int covest_grid_eval_scan(covest_grid *g, int32_t kernel, void *stream, double start_min);
int covest_grid_scan(covest_grid *g, int32_t cap, int64_t *index, double *negll, int32_t *n_records, int32_t *truncated);

/* Device pointer of the reduction of the last covest_grid_eval as two doubles in HBM,
 * {min -LL, GLOBAL flat index of the arg-min as a double (-1 if none; flat indices stay
 * below 2^53)}: what the ranks of a multi-GPU search exchange (one all-gather of these 16
 * bytes) without a round trip through the host.  Valid until the next
 * covest_grid_reset (which may move the handle's device arena) or destroy; written by
 * covest_grid_eval on its stream. */
const double *covest_grid_argmin_pair_device(const covest_grid *g);

/* Device pointer of the block's LL values (double[grid_size], valid until the next
 * covest_grid_reset or destroy) and a copy to the host. */
const double *covest_grid_ll_device(const covest_grid *g);
int covest_grid_ll_host(covest_grid *g, double *out_ll);

/* Work accounting of the last covest_grid_eval, for roofline reporting:
 * pmf terms evaluated (bins_evaluated * n_err * sum(T-1)), log evaluations,
 * and the name of the kernel that ran. */
int covest_grid_work(const covest_grid *g, double *pmf_terms, double *flops, const char **kernel);

/* What the last evaluation launched, for tests: covest_grid_launch_record covers the last covest_grid_eval(_scan) of
 * the handle, covest_model_launch_record the last covest_eval_points of the model.  Text, one line each:
 *   "launch <instantiation> <launches>"   e.g. "launch ll_factored<512,tail,plain,ld290> 1"
 *   "plan n_threads=.. n_buf=.. ld=.. n_qblocks=.. shared_tiles=.. long=0|1 n_pass=.. list_mode=.. col_floor=.."
 *     (a K-factored work description: shared_tiles = q-tiles with shared steps, long = a chunk of the long
 *     weight vectors, col_floor = the largest copy number read by a unit that keeps its full range).
 * covest_compiled_variants lists every instantiation of the likelihood kernels linked into the library, one name a
 * line, from the tables the dispatchers record from (K-direct, the yardstick, is recorded as "ll_direct" or
 * "ll_direct_ref" and not listed).  All three are host bookkeeping: nothing is read from the device.  They write at
 * most cap - 1 characters and a NUL to buf (cap 0: nothing) and return the length of the whole text, or a negative
 * error. */
int64_t covest_grid_launch_record(const covest_grid *g, char *buf, int64_t cap);
int64_t covest_model_launch_record(covest_model *m, char *buf, int64_t cap);
int64_t covest_compiled_variants(char *buf, int64_t cap);

/* Device-side timing of the likelihood kernel alone (not the arg-min pass), for
 * roofline reporting: with profiling enabled every covest_grid_eval brackets its
 * likelihood launch with hipEvents on the launch stream; covest_grid_kernel_ms
 * waits for them and returns the summed duration and the number of launches
 * since profiling was (re-)enabled. */
int covest_grid_profile(covest_grid *g, int32_t enable);
int covest_grid_kernel_ms(covest_grid *g, double *total_ms, int64_t *launches);

/* ---- k-mer abundance histogram: bin/kmer_hist.py (BASELINE config 5) ----
 * The counter is the `counts` dict of compute_counts (bin/kmer_hist.py:34-41) as an
 * open-addressing hash table in HBM.  k <= 255 (the reference's Python integers have no limit: k <= 31 is the fast
 * path, one 64-bit word per key; 32..63, ..127, ..255 take keys of 2, 4, 8 words).  canonical != 0 counts a k-mer and its reverse
 * complement as one key (jellyfish -C; NOT reference behaviour, the reference is forward-strand). */
typedef struct covest_kmer covest_kmer; /* opaque */

int covest_kmer_create(int32_t k, int32_t canonical, int64_t min_slots, int32_t device, covest_kmer **out);
void covest_kmer_destroy(covest_kmer *c);
/* Grow the table to at least min_slots (power of two), re-inserting what it holds.  The caller
 * keeps the table at most half full: slots >= 2 * (DISTINCT k-mers held + those the next batch can
 * add).  Overflow contract: a covest_kmer_add / covest_kmer_histogram that returns COVEST_E_NOMEM has
 * counted PART of its batch; the counter is then only good for covest_kmer_clear (recount with a larger
 * table).  The overflow state is STICKY until covest_kmer_clear: covest_kmer_reserve waits for everything in
 * flight on the device, returns COVEST_E_NOMEM if an earlier (asynchronous) add overflowed, and otherwise
 * re-inserts into the larger table and reports its own outcome. */
int covest_kmer_reserve(covest_kmer *c, int64_t min_slots);
/* compute_counts(seq, prev_counts=counts, k) for n_reads preprocessed reads (bin/kmer_hist.py:44-54
 * already applied: only a/c/g/t in either case).  bases: the reads back to back; offsets[n_reads+1].
 * A read shorter than k contributes the hash of what there is, an empty read k-mer 0 (:36-37).
 * HOST buffers; the call copies them to the device and waits. */
int covest_kmer_add(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads);
/* Same with DEVICE buffers, asynchronous on `stream`: d_offsets may be NULL when every read is
 * read_len bases long. */
int covest_kmer_add_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets,
                           int64_t n_reads, int64_t read_len, void *stream);
/* The same with a WEIGHT PER READ (uint32, weights[n_reads], aligned to 4 bytes): every k-mer
 * occurrence of read r is added weights[r] times, in one atomic add.  A read of weight 0 adds nothing and creates no
 * key; a read shorter than k adds its one key weights[r] times.  All weights 1 is covest_kmer_add*.  Everything else --
 * the table, every key width (k = 1 .. 255), the overflow flag and its contract, the reserve rule (weights never add
 * DISTINCT keys: the caller sizes the table as for the unweighted add), the refusal on a counter that holds a
 * covest_kmer_count_reads_device result -- is covest_kmer_add_device's and covest_kmer_add's.  The _device form is
 * asynchronous on `stream` and reads d_weights there: weights written on the same stream (covest_bootstrap_weights_device)
 * need no synchronisation in between.  COVEST_E_INVALID also for NULL weights with n_reads > 0 and for a weights
 * pointer that is not aligned to 4 bytes.  The partitioned path takes no weights. */
int covest_kmer_add_weighted_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                                    int64_t read_len, const uint32_t *d_weights, void *stream);
int covest_kmer_add_weighted(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                             const uint32_t *weights);
/* The INVERSE of the four adds (k <= 31; no reference counterpart): every k-mer occurrence of
 * read r is taken out of the table once, or weights[r] times.  Same arguments, same read layout, same weight rules as
 * covest_kmer_add_device / _add_weighted_device / _add / _add_weighted: a read of weight 0 takes nothing out (also
 * where it was never added), a read shorter than k takes out the one key the add adds for it, an empty read k-mer 0.
 *   HELD and OCCUPIED.  A removal lowers a count and never clears a key.  A key is HELD if its slot carries it with a
 * count of at least 1; a slot is OCCUPIED if it carries a key at all.  covest_kmer_histogram (its distinct count, its
 * histogram: out[0] stays 0), covest_kmer_join_histogram* (a key held by neither table is in no cell) and the lookups
 * (0 already means "holds none") speak of held keys; how FULL the table is, is a matter of occupied slots:
 * covest_kmer_occupancy gives both, and the caller's reserve rule reads "slots >= 2 * (slots OCCUPIED + keys the next
 * batch can add)".  covest_kmer_reserve, when it rehashes, and covest_kmer_compact leave the keys of count 0 behind.
 *   UNDERFLOW.  A window whose key occupies no slot, or whose count was smaller than what is subtracted, sets a sticky
 * underflow state on the counter, separate from the overflow state (neither erases the other).  After it the counts
 * are unspecified.  Until covest_kmer_clear, every call that answers COVEST_E_NOMEM for a sticky overflow --
 * covest_kmer_histogram, covest_kmer_reserve when it would rehash, covest_kmer_compact, the host forms of the adds, the
 * removals, the lookups, the correction, the influence and the join -- answers COVEST_E_INVALID with "underflow" and
 * its own name in the message (an overflow, where both are set, is reported first).
 *   The _device forms are asynchronous on `stream`, which must be the stream of the adds whose counts they take back
 * (or ordered after them by the caller), read d_weights there, and never look at either state.  The host forms copy,
 * wait and report an underflow themselves.
 *   COVEST_E_UNSUPPORTED for k > 31: in the wide table the state word IS the count and 0 means empty, so a key cannot
 * survive a count of 0 there.  COVEST_E_INVALID on a counter that holds a covest_kmer_count_reads_device result, for
 * NULL weights with n_reads > 0 and for a weights pointer that is not aligned to 4 bytes.  Removal frees no slot. */
int covest_kmer_remove_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                              int64_t read_len, void *stream);
int covest_kmer_remove_weighted_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                                       int64_t read_len, const uint32_t *d_weights, void *stream);
int covest_kmer_remove(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads);
int covest_kmer_remove_weighted(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                                const uint32_t *weights);
/* out[0] = the keys held, out[1] = the slots occupied (k <= 31, not a partitioned result).  Waits for the device. */
int covest_kmer_occupancy(covest_kmer *c, int64_t out[2]);
/* Rehash into a fresh table of the same size: the keys of count 0 go, occupied == held afterwards (k <= 31, not a
 * partitioned result).  Waits for the device; the sticky states as covest_kmer_reserve. */
int covest_kmer_compact(covest_kmer *c);
/* compute_histogram(counts) (bin/kmer_hist.py:57-64): out[i] = number of distinct k-mers seen i
 * times, i = 0 .. max count.  Call with out == NULL to learn needed_len (= max count + 1) and the
 * number of distinct k-mers; fails with COVEST_E_NOMEM-like status if the table overflowed.  After removals
 * (covest_kmer_remove*) "distinct" are the keys HELD, and a removal that underflowed makes it fail with
 * COVEST_E_INVALID. */
int covest_kmer_histogram(covest_kmer *c, int64_t *out, int64_t out_len, int64_t *needed_len,
                          int64_t *distinct);
/* The WHOLE counting loop of main (bin/kmer_hist.py:77-89: compute_counts over every read) for reads resident in
 * HBM, into an EMPTY counter, by the partitioned path (kmer_bulk.hip): the k-mers are grouped by minimizer into
 * buckets of super-k-mer records and counted bucket by bucket in LDS -- an occurrence costs no scattered memory
 * operation.  The counts are not kept as a dict: afterwards the counter answers covest_kmer_histogram (count-of-counts,
 * distinct keys -- exact) and nothing else, until covest_kmer_clear.  d_offsets NULL: every read is read_len bases;
 * else offsets[n_reads + 1] (ascending, reads back to back; fewer than 2^32 reads); n_bases_total is a hint, the
 * offsets decide.  Blocks until done.
 * COVEST_E_UNSUPPORTED: k outside 19..31, or reads of one length (no offsets) shorter than k; COVEST_E_NOMEM: the
 * buckets do not fit the device, or the sample of the reads misjudged them beyond what the overflow list holds --
 * covest_kmer_clear, then count with covest_kmer_add_device (whatever the counter held before the call is not part
 * of the result either way: the call counts into an emptied counter). */
int covest_kmer_count_reads_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                                   int64_t read_len, int64_t n_bases_total, void *stream);
/* How the last covest_kmer_count_reads_device went (the counter still holds its result): out[0] buckets, [1] minimizer
 * length, [2] pass 0 sampled one block of reads in this many, [3] records the buckets had room for, [4] records that
 * found their bucket full, [5] buckets counted by a workgroup instead of a wave, [6] buckets counted through the table
 * in HBM, [7] records pass 1 wrote.  Diagnostics for the caller's log; no reference counterpart. */
int covest_kmer_partition_info(const covest_kmer *c, int64_t out[8]);
/* A cap on what the partitioned path may allocate for its buckets' records (bytes; 0 = no cap but the device's free
 * memory): a caller that shares the card names its budget, and covest_kmer_count_reads_device answers COVEST_E_NOMEM
 * where the buckets would pass it -- before it allocates them. */
int covest_kmer_memory_limit(covest_kmer *c, int64_t max_bytes);
/* ... and how long its steps took on the device, milliseconds (HIP events on the caller's stream): out[0] pass 0
 * (sample of the reads, room per bucket, their places), [1] pass 1 (records to their buckets), [2] pass 2 (the buckets
 * counted in LDS), [3] what was left for the table in HBM. */
int covest_kmer_partition_ms(const covest_kmer *c, double out[4]);
/* Measurement only: the rate at which THIS device retires returning 64-bit atomic adds at pseudo-random places of a
 * `slots`-word array (the 64 lanes of a wave instruction on 64 different lines) -- what bounds pass 1 of the
 * partitioned path (one such add per record) and, per occurrence, the table path.  `ops` adds are timed. */
int covest_kmer_scatter_rate(int32_t device, int64_t slots, int64_t ops, double *ops_per_s);
int64_t covest_kmer_slots(const covest_kmer *c);
/* Forget every count (counts = defaultdict(int) again), keeping the table's size; asynchronous on `stream`.  After
 * covest_kmer_count_reads_device it also frees the buckets' records (gigabytes the handle keeps from call to call). */
int covest_kmer_clear(covest_kmer *c, void *stream);
/* The per-read use of the table (k <= 31; no reference counterpart): for every window of every read the count the
 * table holds for its key, and reductions of those counts per read.  Read-only: nothing is written to the table.
 * Every output is optional (NULL: not wanted).
 *   abundance  uint32, indexed like the bases: the entry at a window's first base is min(count, 0xFFFFFFFE); the last
 *              k - 1 positions of a read (all of a read shorter than k) hold 0xFFFFFFFF, "no window starts here".
 *              Every position in [offsets[0], offsets[n_reads]) -- reads of one length: [0, n_reads * read_len) -- is
 *              written exactly once, nothing outside.
 *   summary    uint32[n_reads][4] = {min_abundance, weak, first_weak, last_weak}: weak = windows with abundance <
 *              cutoff, first_weak / last_weak their first and last window index.  A read without windows gives
 *              {0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF}; one without a weak window has both indices 0xFFFFFFFF;
 *              cutoff 0: no window is weak.  A read has fewer than 2^32 - 1 windows.
 *   score      double[n_reads] = sum over the windows of weights[min(count, n_weights - 1)], n_weights >= 1, summed in
 *              a fixed order (csrc/kmer_lookup.h): the same bits on every run.  A read without windows scores 0.0.
 * A read shorter than k has no window: the key covest_kmer_add counts for it (the hash of what there is) is
 * deliberately NOT looked up.
 * Device form: asynchronous on `stream`; d_bases at any alignment, the outputs naturally aligned (a summary row is
 * one 16-byte store); d_offsets NULL: every read is read_len bases.  The call must be ORDERED AFTER the adds it is to
 * see -- the same stream, or the caller's own synchronisation -- and never looks at the overflow flag.
 * Host form: copies, waits, and answers COVEST_E_NOMEM if an add overflowed (sticky until covest_kmer_clear: the
 * counts are then partial); `abundance` holds offsets[n_reads] - offsets[0] entries, indexed relative to offsets[0].
 * COVEST_E_UNSUPPORTED: k > 31.  COVEST_E_INVALID: a null counter, negative sizes, a score without weights or with
 * n_weights < 1, no offsets and read_len < 0, or a counter that holds a covest_kmer_count_reads_device result (its
 * keys are not in the table).  n_reads == 0: COVEST_OK, nothing launched. */
int covest_kmer_lookup_reads_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                                    int64_t read_len, uint32_t cutoff, const double *d_weights, int32_t n_weights,
                                    uint32_t *d_abundance, uint32_t *d_summary, double *d_score, void *stream);
int covest_kmer_lookup_reads(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                             uint32_t cutoff, const double *weights, int32_t n_weights, uint32_t *abundance,
                             uint32_t *summary, double *score);
/* Isolated substitutions corrected from the table (k <= 31; no reference counterpart; read-only on the table).  Per
 * read, last = len - k: a window is WEAK when the table's count for its key is below `cutoff` (0: none is); a RUN is a
 * maximal set of consecutive weak windows [f, l], judged against the original bytes whatever happens to other runs; its
 * CANDIDATE POSITIONS are the bases p whose covering windows [max(0, p - k + 1), min(p, last)] are exactly [f, l]
 * (none when the run is longer than k; p = f + k - 1 when f > 0, and only if l == min(p, last); p = l when f == 0 and
 * l < last; every p in [last, min(k - 1, len - 1)] when the run is the whole read).  An alternative -- a candidate
 * position and one of the three other bases -- is VALID when every window of the run, with that base replaced, has a
 * count >= cutoff.  Exactly one valid alternative: the run is CORRECTED, the byte becomes that base in the case of the
 * old byte; more than one: AMBIGUOUS; none: UNFIXABLE; the bytes then stay.  Two errors closer than k + 1 merge into one
 * run longer than k and stay.
 *   out  uint8, indexed like the bases: the input except at corrected positions; every byte of every read is stored
 *        exactly once, nothing outside.  It may be the very pointer of the bases (in place: only the corrected bytes are
 *        stored); otherwise it must not overlap them.
 *   fix  uint32[n_reads][4] = {runs, corrected, ambiguous, unfixable}, runs being the sum of the other three; optional
 *        (NULL).  A read shorter than k has no window: its bytes are copied, its row is {0, 0, 0, 0}.
 * Device form: asynchronous on `stream`; d_bases and d_out at any alignment, d_fix 16-byte aligned; d_offsets NULL:
 * every read is read_len bases.  It must be ORDERED AFTER the adds it is to see and never looks at the overflow flag.
 * A d_out that overlaps the reads without being d_bases is COVEST_E_INVALID where the host can see it: reads of one
 * length; with d_offsets the extent of the reads is known on the device alone, and it is the caller's to keep apart.
 * Host form: copies, waits, and answers COVEST_E_NOMEM if an add overflowed; `out` holds offsets[n_reads] -
 * offsets[0] bytes, indexed relative to offsets[0].
 * COVEST_E_UNSUPPORTED: k > 31.  COVEST_E_INVALID: a null counter, negative sizes, no offsets and read_len < 0, a null
 * out with n_reads > 0, a d_fix that is not 16-byte aligned, or a counter that holds a covest_kmer_count_reads_device
 * result.  n_reads == 0: COVEST_OK, nothing launched. */
int covest_kmer_correct_reads_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                                     int64_t read_len, uint32_t cutoff, uint8_t *d_out, uint32_t *d_fix, void *stream);
int covest_kmer_correct_reads(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                              uint32_t cutoff, uint8_t *out, uint32_t *fix);
/* The influence of ONE read on a sum over the distinct k-mers (k <= 31; no reference counterpart; read-only on the
 * table).  `table` is double[n_rows][n_cols] row-major, n_rows >= 1, 1 <= n_cols <= 8: row i is
 * the value at abundance i, and the row of an abundance a is min(a, n_rows - 1).  With a_x the count the table holds
 * for key x and m_x the number of windows of read r whose key is x, deleting r moves x from a_x to a_x - m_x, so
 *   rows[r][c] = sum over the DISTINCT keys x of r of  table[row(max(a_x - m_x, 0))][c] - table[row(a_x)][c],  c < n_cols,
 *   rows[r][n_cols] = the number of windows of r, as a double.
 * `rows` is double[n_reads][n_cols + 1].  a_x < m_x can only happen when the table was not counted from these reads;
 * it takes row 0.  A read shorter than k has every column +0.0: the key covest_kmer_add counts for it is NOT looked
 * up, as in covest_kmer_lookup_reads.  The sums are made in a fixed order (csrc/kmer_influence.h): the same bits on
 * every run.  The compare that finds m_x is quadratic in a read's windows: a read with more than 4096 windows gets
 * NaN in its value columns from the device form with d_offsets (its window count is still written), and
 * COVEST_E_UNSUPPORTED, before anything is launched, from the host form and from the device form with reads of one
 * length.
 * Device form: asynchronous on `stream`; d_bases at any alignment, d_table and d_rows aligned to 8 bytes; d_offsets
 * NULL: every read is read_len bases.  It must be ORDERED AFTER the adds it is to see and never looks at the overflow
 * flag.  Host form: copies, waits, and answers COVEST_E_NOMEM if an add overflowed.
 * COVEST_E_UNSUPPORTED: k > 31.  COVEST_E_INVALID: a null counter, negative sizes, bad offsets, no offsets and
 * read_len < 0, n_rows < 1, n_cols outside 1 .. 8, a null table or rows, or a counter that holds a
 * covest_kmer_count_reads_device result.  n_reads == 0: COVEST_OK, nothing launched. */
int covest_kmer_read_influence_device(covest_kmer *c, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                                      int64_t read_len, const double *d_table, int64_t n_rows, int32_t n_cols,
                                      double *d_rows, void *stream);
int covest_kmer_read_influence(covest_kmer *c, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                               const double *table, int64_t n_rows, int32_t n_cols, double *rows);
/* Two counters joined on their keys (k <= 31 on both sides, the same k, canonical flag and device; no reference
 * counterpart; read-only on both tables).  With a(x) the count counter `a` holds for key x (0:
 * it holds none), b(x) the same for `b`, and U the keys held by at least one of the two,
 *   out[i][j] = #{ x in U : min(a(x), n_rows - 1) == i  and  min(b(x), n_cols - 1) == j },
 * int64, row-major, n_rows * n_cols entries: the last row and the last column take every count from n_rows - 1, n_cols - 1
 * on.  Row 0 holds the keys of `b` alone, column 0 those of `a` alone; out[0][0] is 0 (n_rows, n_cols >= 2).  The sum of all entries is the
 * number of keys in U, the sums of rows i >= 1 are the clipped covest_kmer_histogram of `a`, those of columns j >= 1
 * that of `b`.  The two tables may be of different sizes; either may be empty.  The key covest_kmer_add counts for a
 * read shorter than k is a key like any other.  The counts are integers: the same result on every run.
 * Device form: asynchronous on `stream`; d_out aligned to 8 bytes and ZEROED BY THE CALL on `stream` before anything is
 * counted (it may hold anything); nothing outside its n_rows * n_cols entries is written.  The call must be ORDERED
 * AFTER the adds into BOTH counters that it is to see -- the same stream, or the caller's own synchronisation -- and
 * never looks at an overflow flag.
 * Host form: waits for the device, joins, waits, and answers COVEST_E_NOMEM if an add into either counter overflowed
 * (sticky until that counter's covest_kmer_clear: the counts are then partial); then copies the matrix to `out`.
 * Both counters' locks are held for the call, taken together: a join of (a, b) on one thread and of (b, a) on another
 * cannot wait for each other.
 * COVEST_E_UNSUPPORTED: k > 31 on either side.  COVEST_E_INVALID: a null counter, the same counter twice, counters
 * that differ in k, in the canonical flag or in their device, n_rows < 1, n_cols < 1, n_rows * n_cols > 2^22, a null
 * output, a d_out that is not aligned to 8 bytes, or a counter that holds a covest_kmer_count_reads_device result (its
 * keys are not in the table). */
int covest_kmer_join_histogram_device(covest_kmer *a, covest_kmer *b, int64_t n_rows, int64_t n_cols, int64_t *d_out,
                                      void *stream);
int covest_kmer_join_histogram(covest_kmer *a, covest_kmer *b, int64_t n_rows, int64_t n_cols, int64_t *out);
/* The first two moments of n rows of q doubles about `centre` (1 <= q <= 9), with d_r = rows[r] - centre:
 *   sum[k] = sum_r d_r[k];   cross[k q - k (k - 1) / 2 + (l - k)] = sum_r d_r[k] d_r[l] for k <= l
 * (the packed upper triangle, row by row: q (q + 1) / 2 entries).  No floating-point atomic: the shape of the reduction
 * is a function of n alone (csrc/kmer_influence.h), so the same rows give the same bits on every run.  n == 0: zeros.
 * Device form: asynchronous on `stream`, on the calling thread's current device; every array aligned to 8 bytes.
 * COVEST_E_INVALID: n < 0 or beyond 2^40, q outside 1 .. 9, a null array. */
int covest_rows_moments_device(const double *d_rows, int64_t n, int32_t q, const double *d_centre, double *d_sum,
                               double *d_cross, void *stream);
int covest_rows_moments(const double *rows, int64_t n, int32_t q, const double *centre, double *sum, double *cross);

/* ---- FASTA / FASTQ front-end of the k-mer histogram: bin/kmer_hist.py:44-54 preprocess, :67-74 load_reads ----
 * HOST code (the only HIP calls: a device count and the allocation of page-locked buffers): the mapped file
 * is parsed span by span into batches in the packed layout covest_kmer_add takes.  Format by extension, as the reference: ".fq" / ".fastq" = FASTQ (4-line records), anything else FASTA
 * (a record = a '>' header line and the concatenation of the lines up to the next header; the reference leaves
 * the parsing to Bio.SeqIO).  preprocess is applied on the way: lower case; 'n' dropped (n_strategy 0, IGNORE),
 * replaced by 'a' (1, SINGLE) or by a random base (2, RANDOM: a hash of `seed` and of the N's position in the
 * file -- the reference draws from Python's unseeded random, which nothing can reproduce).  Any other letter fails with COVEST_E_INVALID, where
 * the reference's single_hash raises KeyError (:15).  An empty record is a read (it counts k-mer 0, :36-37). */
typedef struct covest_reads covest_reads; /* opaque */
int covest_reads_open(const char *path, int32_t n_strategy, uint64_t seed, covest_reads **out);
void covest_reads_close(covest_reads *r);
/* The next batch: whole reads, about max_bases bases of them (the span of the file that holds that many, up to the
 * next record boundary; one read at least), parsed by several threads (COVEST_READER_THREADS, default: the
 * machine's, 16 at most).  Two batch buffers alternate: *bases / *offsets[*n_reads + 1] stay valid until the call
 * AFTER the next one on `r`, so batch i + 1 can be parsed while batch i is being counted.  The buffers are
 * page-locked when the process has a HIP device (COVEST_READER_PINNED=0: never).  *n_reads == 0: end of file. */
int covest_reads_next(covest_reads *r, int64_t max_bases, const uint8_t **bases, const int64_t **offsets,
                      int64_t *n_reads);
/* file bytes consumed so far */
int64_t covest_reads_bytes(const covest_reads *r);

/* ---- read simulator: tools/simulator/generate_sequence.py, read_simulator.py:60-88 ----
 * Reads of KNOWN coverage and error rate, written in the layout covest_kmer_add_device and
 * covest_kmer_count_reads_device take (upper-case ASCII, read_len bases each, back to back, no offsets).  Where the
 * reference draws from Python's unseeded `random`, every byte here is a function of (seed, read index, base index)
 * through Philox4x32-10 (Random123; key = seed's low and high word), so reads [first_read, first_read + n_reads) of
 * one call are the same slice of any other call with the same seed, genome and settings:
 *   genome base i: block (lo32(i>>2), hi32(i>>2), 0, 1), word i & 3, "ACGT"[word >> 30]
 *   read r:        header block (lo32(r), hi32(r), 0, 0) = w0..w3: pos = mulhi64(w0 | w1 << 32, genome_len - read_len)
 *                  -- randrange(genome_size - read_length), the last start never drawn (:75) --; the forward slice if
 *                  w2 & 1 or both_strands == 0, else its reverse complement (:77-78)
 *   base i of it:  block (lo32(r), hi32(r), 1 + (i >> 2), 0), w = word i & 3: substituted iff w < floor(error_rate *
 *                  2^32) by the base of code (code + 1 + w % 3) & 3, A C G T = 0 1 2 3: one of the other three (:16-20, :79)
 * origin (may be NULL)[n_reads] = pos << 1 | forward.  The genome is a/c/g/t in either case (-s, the IUPAC
 * substitution of :34-57, is not built): the host form answers COVEST_E_INVALID for any other byte; the device form
 * does not look, and takes (byte >> 1) & 3 for a code, so any byte is SOME base.
 * COVEST_E_INVALID: genome_len <= read_len, read_len < 1, n_reads < 0, first_read < 0, error_rate outside [0, 1] or
 * NaN.  n_reads == 0 (n == 0): COVEST_OK, nothing launched.  device < 0 = the calling thread's current device.
 * The _device forms take DEVICE buffers of any alignment and are asynchronous on `stream`; they write nothing outside
 * d_bases[0 .. n_reads * read_len) and d_origin[0 .. n_reads).  The others take HOST buffers, copy and wait;
 * COVEST_E_NOMEM where the device buffers of the call do not fit. */
int covest_random_genome_device(int32_t device, int64_t n, uint64_t seed, uint8_t *d_out, void *stream);
int covest_simulate_reads_device(int32_t device, const uint8_t *d_genome, int64_t genome_len, int32_t read_len,
                                 int64_t first_read, int64_t n_reads, double error_rate, uint64_t seed,
                                 int32_t both_strands, uint8_t *d_bases, int64_t *d_origin, void *stream);
int covest_random_genome(int32_t device, int64_t n, uint64_t seed, uint8_t *out);
int covest_simulate_reads(int32_t device, const uint8_t *genome, int64_t genome_len, int32_t read_len,
                          int64_t first_read, int64_t n_reads, double error_rate, uint64_t seed,
                          int32_t both_strands, uint8_t *bases, int64_t *origin);

/* ---- repeat-bearing genomes: a prescribed copy-number distribution of k-mers ----
 * covest_random_genome draws every base on its own, so every k-mer of it is single-copy and the repeat model's
 * (q1, q2, q) have no truth to find.  A REPEAT GENOME of n bases is n_units = ceil(n / unit_len) units of unit_len
 * bases (the last may be cut), each a copy of one FAMILY, forward or reverse-complemented, then mutated away from it
 * at rate `divergence`.  Philox4x32-10 as above, key = seed's low and high word; the last counter words 3 to 6 are
 * this section's (0: reads, 1: genome, 2: sampler), so everything here is independent of those under one seed.
 *   family base g (g = f * unit_len + offset, 64-bit): block (lo32(g>>2), hi32(g>>2), 0, 3), word g & 3,
 *                  "ACGT"[word >> 30]
 *   copy number of family f: u = word 0 of block (lo32(f), hi32(f), 0, 4); o_f = 1 + the number of o in
 *                  1 .. max_copies - 1 with t_o <= u, t_o = min(2^32, floor(cdf_o * 2^32)).  The cdf is formed in
 *                  double by basic IEEE operations only, in this order (no pow): cdf_1 = q1;
 *                  cdf_2 = cdf_1 + (1 - q1) * q2; b = ((1 - q1) * (1 - q2)) * q; cdf_3 = cdf_2 + b; from there
 *                  b = b * (1 - q), cdf_{o+1} = cdf_o + b.  This is RepeatsModel.get_b_o (covest/models.py:193-208)
 *                  as a distribution; the mass the thresholds leave lands on max_copies.
 *   unit list:     families 0, 1, 2, ... each repeated o_f times until n_units entries exist (the last family is cut
 *                  to fit; *n_families = families in the list).  Entry j gets block (lo32(j), hi32(j), 0, 5) = w0..w3;
 *                  the list is stably sorted by the 64-bit key w0 | w1 << 32, ties by j; the entry is forward iff
 *                  w2 & 1 or both_orientations == 0.  plan[slot] = f << 1 | forward.
 *   genome base i: u = i / unit_len, off = i % unit_len, (f, fwd) = plan[u].  Forward: the family base at
 *                  f * unit_len + off.  Reverse: 3 - code of the family base at f * unit_len + unit_len - 1 - off.
 *                  Then divergence: w = word i & 3 of block (lo32(i>>2), hi32(i>>2), 0, 6); the base is substituted
 *                  iff w < floor(divergence * 2^32), by code (code + 1 + w % 3) & 3 -- the reads' rule.  At
 *                  divergence 0 those blocks are not computed.
 * A plan is plain data: a caller may hand-write one (a tandem array, one family everywhere, all distinct).
 * covest_repeat_plan is host arithmetic and needs no device.  COVEST_E_INVALID: q1, q2 or q outside [0, 1] or NaN,
 * max_copies outside 1 .. 2^20, n_units < 0, a NULL output with n_units > 0.  n_units == 0: COVEST_OK, *n_families = 0.
 * COVEST_E_NOMEM: n_units beyond 2^40, or a unit list (16 bytes a unit while it is sorted) the host cannot hold.
 * covest_repeat_genome*: COVEST_E_INVALID for unit_len < 1, n < 0, n > n_units * unit_len, divergence outside [0, 1]
 * or NaN, a NULL buffer with n > 0, and -- host form only -- a negative plan entry or a family id whose bases leave 63
 * bits ((f + 1) * unit_len > 2^63 - 1); with the device form both are the caller's duty.  The host form looks at all
 * n_units entries of the plan, whatever n is (n == 0 included: a bad plan is refused before anything else), and copies
 * to the device only the ceil(n / unit_len) entries the genome uses.  n == 0 otherwise: COVEST_OK, nothing
 * launched.  The _device form takes DEVICE buffers (d_out of any alignment), is asynchronous on `stream` and writes
 * nothing outside d_out[0 .. n); the other takes HOST buffers, copies and waits.  device < 0 = the calling thread's
 * current device. */
int covest_repeat_plan(int64_t n_units, double q1, double q2, double q, int32_t max_copies, uint64_t seed,
                       int32_t both_orientations, int64_t *plan, int64_t *n_families);
int covest_repeat_genome_device(int32_t device, const int64_t *d_plan, int64_t n_units, int32_t unit_len, int64_t n,
                                double divergence, uint64_t seed, uint8_t *d_out, void *stream);
int covest_repeat_genome(int32_t device, const int64_t *plan, int64_t n_units, int32_t unit_len, int64_t n,
                         double divergence, uint64_t seed, uint8_t *out);

/* ---- read sampler: covest/data.py:57-63 sample_reads, bin/read_sampler.py ----
 * Keeps every read with probability 1 / factor and writes the kept reads, IN INPUT ORDER, in the layout they came in:
 * the packed layout of covest_kmer_add_device (bases back to back at any alignment; offsets[n_reads + 1] ascending, or
 * NULL when every read is read_len bases long).  Empty reads are reads: a kept one is an empty read of the output.
 * Where the reference draws from Python's unseeded `random`, the selection is a function of (seed, read index):
 *   read r = index within the call + first_read (64-bit);
 *   w = word 0 of Philox4x32-10 (as above; key = seed's low and high word) on the counter (lo32(r), hi32(r), 0, 2);
 *   the read is kept iff (uint64_t)w < thr, thr = floor((1.0 / factor) * 2^32) formed in double on the host
 *   (prob = 1.0 / factor of data.py:58, quantised as the simulator quantises error_rate); factor == 1: thr = 2^32,
 *   every read is kept.
 * The simulator's counters end in (.., 0, 1) (genome) and (.., j, 0) (reads), so the selection of simulated reads with
 * their own seed is independent of their content.  A chunk [a, a + m) sampled with first_read = a keeps exactly the
 * reads the whole run keeps among those rows.
 * Output: out_bases (any alignment), out_offsets[n_kept + 1] (may be NULL where offsets is), kept_index[n_kept] (may be
 * NULL): the global indices r; counts[2] = (reads kept, bases kept).  The caller sizes the outputs for the input (the
 * upper bound); nothing is written outside out_bases[0 .. bases_kept), out_offsets[0 .. n_kept], kept_index[0 .. n_kept)
 * and counts[0 .. 2).  Scratch is the library's own (8 bytes a read of the input).
 * COVEST_E_INVALID: factor < 1, NaN or infinite; n_reads < 0 or first_read < 0; offsets == NULL with read_len < 0;
 * offsets without out_offsets; a NULL counts.  n_reads == 0: COVEST_OK, no kernel launched, counts (0, 0) and
 * out_offsets[0] = 0 (the device form sets them by a memset on the stream).  COVEST_E_NOMEM where the device buffers of
 * the call do not fit.  device < 0 = the calling thread's current device.
 * The _device form takes DEVICE buffers, is asynchronous on `stream` and does not look at the offsets; the other takes
 * HOST buffers, copies and waits, and answers COVEST_E_INVALID for offsets that are negative or descend. */
int covest_sample_reads_device(int32_t device, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                               int64_t read_len, int64_t first_read, double factor, uint64_t seed,
                               uint8_t *d_out_bases, int64_t *d_out_offsets, int64_t *d_kept_index,
                               int64_t *d_counts, void *stream);
int covest_sample_reads(int32_t device, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                        int64_t read_len, int64_t first_read, double factor, uint64_t seed,
                        uint8_t *out_bases, int64_t *out_offsets, int64_t *kept_index,
                        int64_t *n_kept, int64_t *bases_kept);

/* ---- duplicate reads removed: the first copy kept, input order ----
 * Takes the copies out of a read set in the packed layout above (PCR and optical duplicates double the variance of the
 * k-mer abundances and make repeated misreads look like k-mers of abundance 2) and writes the kept reads, IN INPUT
 * ORDER, in the layout they came in.  The result is a function of the input; scheduling does not change it.
 *   Equality: reads x and y are equal if they have the same length and the same bytes; with reverse_complement != 0 also
 *   if x is the reverse complement of y (a <-> t, c <-> g in either case, the case kept; every other byte is its own
 *   complement).  Case is not folded.  Two empty reads are equal.
 *   Fingerprint: mix64(z) is the finaliser of SplitMix64 (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *   z *= 0x94D049BB133111EB; z ^= z >> 31); salt = mix64(seed + 0x9E3779B97F4A7C15); S(x) = the sum mod 2^64 over the
 *   positions j of mix64(salt + 256 * j + x[j]); F(x) = mix64(mix64(S(x) + seed) + len(x)).  A read's fingerprint is
 *   F(x), with reverse_complement min(F(x), F(rc(x))); its KEY the low fp_bits bits of that, fp_bits in 1 .. 63 (so the
 *   table's empty sentinel, ~0, is no key).  fp_bits below 63 only makes more reads collide: it is there for tests of
 *   the collision route.  Pass 63.
 *   rep(r) = the lowest read index among the call's reads that have r's key.  Read r is KEPT iff rep(r) == r, or read r
 *   is not equal to read rep(r) (a fingerprint collision: kept and counted as collided), or its insert into the table
 *   ran out of probes (2^16; counted alike).  Otherwise it is DROPPED and is one more copy of rep(r).
 * So every dropped read is equal to an earlier read that is kept, a read without an equal is never dropped, and a
 * duplicate survives only beside a collision: where counts[2] > 0, the call run again on its own output with another
 * seed removes the remainder.
 * Output: out_bases (any alignment), out_offsets[n_kept + 1] (may be NULL where offsets is), kept_index[n_kept] (may be
 * NULL): first_read + the index within the call; copies[n_kept] (may be NULL): 1 + the reads dropped onto that read;
 * counts[3] = (reads kept, bases kept, reads kept as collided).  The caller sizes the outputs for the input; nothing is
 * written outside out_bases[0 .. bases_kept), out_offsets[0 .. n_kept], kept_index[0 .. n_kept), copies[0 .. n_kept)
 * and counts[0 .. 3).  Scratch is the library's own: 16 bytes a slot of a table of the power of two of slots that is
 * at least 2 * n_reads, and 20 bytes a read.  The compared read must be resident: one call, one resident set.
 * COVEST_E_INVALID: fp_bits outside 1 .. 63; n_reads < 0 or first_read < 0; offsets == NULL with read_len < 0; offsets
 * without out_offsets; a NULL counts.  n_reads == 0: COVEST_OK, no kernel launched, counts (0, 0, 0) and out_offsets[0]
 * = 0 (the device form sets them by a memset on the stream).  COVEST_E_NOMEM where the device buffers of the call do not
 * fit.  device < 0 = the calling thread's current device.
 * The _device form takes DEVICE buffers, is asynchronous on `stream` and does not look at the offsets; the other takes
 * HOST buffers, copies and waits, and answers COVEST_E_INVALID for offsets that are negative or descend. */
int covest_dedup_reads_device(int32_t device, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                              int64_t read_len, int64_t first_read, int32_t reverse_complement, int32_t fp_bits,
                              uint64_t seed, uint8_t *d_out_bases, int64_t *d_out_offsets, int64_t *d_kept_index,
                              int32_t *d_copies, int64_t *d_counts /* 3 */, void *stream);
int covest_dedup_reads(int32_t device, const uint8_t *bases, const int64_t *offsets, int64_t n_reads, int64_t read_len,
                       int64_t first_read, int32_t reverse_complement, int32_t fp_bits, uint64_t seed,
                       uint8_t *out_bases, int64_t *out_offsets, int64_t *kept_index, int32_t *copies,
                       int64_t *n_kept, int64_t *bases_kept, int64_t *n_collided);

/* ---- read groups: a stable G-way split of the packed reads ----
 * Deals every read into one of `groups` = G groups (1 <= G <= 256) and writes the reads group by group -- group 0's
 * first, then group 1's, ... --, IN INPUT ORDER WITHIN A GROUP (a stable partition), in the layout they came in: the
 * packed layout of covest_kmer_add_device (bases back to back at any alignment; offsets[n_reads + 1] ascending, or NULL
 * when every read is read_len bases long).  Every group is then one contiguous run of reads: "all reads but group g"
 * is two sub-ranges of one buffer (the delete-a-group jackknife over reads, covest_amd/jackknife.py).  Empty reads are
 * reads.  The group is a function of (seed, read index) alone:
 *   read r = index within the call + first_read (64-bit);
 *   w = word 0 of Philox4x32-10 (as above; key = seed's low and high word) on the counter (lo32(r), hi32(r), 0, 8)
 *   (stream 8, `group`: the next row of the table of streams above);
 *   group(r) = (w * G) >> 32, the product formed in 64-bit integer arithmetic.
 * So the group does not depend on the read's content, on the sampler's stream (.., 0, 2) or the simulator's, or on how
 * a run is cut into chunks: a chunk [a, a + m) split with first_read = a gives its reads the groups the whole run gives
 * those rows.
 * Output: out_bases (any alignment, the size of the input), out_offsets[n_reads + 1] absolute into out_bases (may be
 * NULL where offsets is), read_index[n_reads] (may be NULL): the global index r of the read at each output rank;
 * group_first[G + 1]: the output rank at which each group starts, group_first[G] = n_reads; an empty group has
 * group_first[g] == group_first[g + 1].  Nothing is written outside out_bases[0 .. bases in all), out_offsets[0 ..
 * n_reads], read_index[0 .. n_reads) and group_first[0 .. G].  Scratch is the library's own: at most 24 bytes a read of
 * the input plus a constant, at every G.
 * COVEST_E_INVALID: groups outside 1 .. 256; n_reads < 0 or first_read < 0; offsets == NULL with read_len < 0; offsets
 * without out_offsets; a NULL group_first.  n_reads == 0: COVEST_OK, no kernel launched, group_first[0 .. G] = 0 and
 * out_offsets[0] = 0 (the device form sets them by a memset on the stream).  COVEST_E_NOMEM where the device buffers of
 * the call do not fit.  device < 0 = the calling thread's current device.
 * The _device form takes DEVICE buffers, is asynchronous on `stream` and does not look at the offsets; the other takes
 * HOST buffers, copies and waits, and answers COVEST_E_INVALID for offsets that are negative or descend. */
int covest_split_reads_device(int32_t device, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                              int64_t read_len, int64_t first_read, int32_t groups, uint64_t seed,
                              uint8_t *d_out_bases, int64_t *d_out_offsets, int64_t *d_read_index,
                              int64_t *d_group_first, void *stream);
int covest_split_reads(int32_t device, const uint8_t *bases, const int64_t *offsets, int64_t n_reads,
                       int64_t read_len, int64_t first_read, int32_t groups, uint64_t seed,
                       uint8_t *out_bases, int64_t *out_offsets, int64_t *read_index, int64_t *group_first);

/* ---- read bootstrap: how often each read is drawn in a replicate ----
 * The bootstrap over reads resamples whole reads with replacement.  Here it is the POISSON bootstrap: the multiplicity
 * of every read is Poisson(1), drawn on its own, so a replicate holds n reads on average (relative spread 1 / sqrt(n))
 * rather than exactly n, and the multiplicity is a function of (seed, replicate, read index) alone:
 *   read r = index within the call + first_read (64-bit); replicate b (uint32);
 *   w = word 0 of Philox4x32-10 (as above; key = seed's low and high word) on the counter (lo32(r), hi32(r), b, 9)
 *   (stream 9, `bootstrap`: the next row of the table of streams below);
 *   m(r, b) = #{ i in 0 .. 12 : w >= T_i },  T_i = floor(2^32 P(Poisson(1) <= i)):
 *   T = 1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463,
 *       4294966817, 4294967252, 4294967292, 4294967295.
 * The largest m is 13; the mass beyond 12 is 0.27 * 2^-32, so the table is complete at 32 bits.  Rows [a, a + m) drawn
 * with first_read = a equal the same rows of the whole run.  out[n_reads] (uint32, aligned to 4 bytes) is what
 * covest_kmer_add_weighted* takes for its weights; nothing is written outside out[0 .. n_reads).
 * COVEST_E_INVALID: n_reads < 0 or first_read < 0, first_read + n_reads beyond 64-bit reach, a NULL or misaligned out
 * with n_reads > 0.  n_reads == 0: COVEST_OK, nothing launched.  device < 0 = the calling thread's current device.
 * The _device form takes a DEVICE buffer and is asynchronous on `stream`; the other takes a HOST buffer, copies and
 * waits (COVEST_E_NOMEM where its device buffer does not fit). */
int covest_bootstrap_weights_device(int32_t device, int64_t n_reads, int64_t first_read, uint64_t seed, uint32_t replicate,
                                    uint32_t *d_out, void *stream);
int covest_bootstrap_weights(int32_t device, int64_t n_reads, int64_t first_read, uint64_t seed, uint32_t replicate,
                             uint32_t *out);

/* ---- replicate histograms drawn from a weight vector: the parametric bootstrap's generator ----
 * INPUT: m >= 1 weights w_0 .. w_{m-1} (doubles, finite, >= 0, sum > 0) and a number of draws n >= 0.  A call covers
 * the replicates first_rep .. first_rep + n_rep - 1, every replicate index < 2^32, under a 64-bit seed.
 * THRESHOLDS, by basic IEEE double operations only, in this order (no pow, no compensated sum, no reordering; numpy's
 * cumsum of a one-dimensional double array restates it bit for bit):
 *   cdf_0 = w_0, cdf_i = cdf_{i-1} + w_i strictly left to right; total = cdf_{m-1}; r_i = cdf_i / total;
 *   t_i = floor(r_i * 2^63) as a uint64 -- the product is an exact scaling, and r_i <= 1, so t_i <= 2^63.
 * DRAWS: Philox4x32-10 as above, key = (lo32(seed), hi32(seed)).  Draw d of replicate b takes the block
 *   (lo32(d>>1), hi32(d>>1), b, 7) = w0..w3; an even d uses u = (w0 | w1 << 32) >> 1, an odd d u = (w2 | w3 << 32) >> 1.
 *   The draw's cell is the number of i in 0 .. m - 2 with t_i <= u.  u < 2^63, so a cell whose r_i is 1, and every
 *   cell after it, is never reached from above; a cell of weight 0 (t_i == t_{i-1}) never counts.
 * The streams of the generators, by the counter's last word (the key is always the seed's two words):
 *   0 read (c2: 0 the header, 1 + j the bases 4j .. 4j + 3)   1 genome   2 keep (the sampler)   3 family   4 copies
 *   5 shuffle   6 divergence   7 draw (c2: the replicate)   8 group (covest_split_reads)
 *   9 bootstrap (c2: the replicate; covest_bootstrap_weights) -- c2 is 0 in all but `read`, `draw` and `bootstrap`.
 * OUTPUT: counts[b - first_rep][i] (int64, row-major n_rep x m) = the number of draws d < n of replicate b in cell i.
 * The call OVERWRITES the output: the caller does not zero it.  A run of replicates [a, a + k) equals the same rows
 * of a larger run, and the row for n equals the row for n' > n restricted to its first n draws.  All arithmetic on the
 * device is integer and every atomic an integer one: the counts are exact, whatever the order.
 * COVEST_E_INVALID, before any device work: a weight that is negative, NaN or infinite; a total that is 0 or not
 * finite; m < 1; n_draws < 0; n_rep < 0; first_rep < 0 or a replicate index >= 2^32 (first_rep + n_rep > 2^32); a NULL
 * buffer; and, for covest_draw_histograms*, m > COVEST_DRAW_MAX_CELLS.  n_rep == 0: COVEST_OK, nothing written;
 * n_draws == 0: COVEST_OK, all-zero rows.
 * covest_draw_thresholds is host arithmetic and needs no device (any m).  covest_draw_histograms takes HOST buffers,
 * forms the thresholds, copies and waits (COVEST_E_NOMEM where its device buffers do not fit); the _device form takes
 * DEVICE buffers -- d_thresholds[m] ascending, as covest_draw_thresholds gives them; d_out[n_rep * m] --, is
 * asynchronous on `stream` and writes nothing outside d_out.  device < 0 = the calling thread's current device. */
#define COVEST_DRAW_MAX_CELLS 65536
int covest_draw_thresholds(int64_t m, const double *weights, uint64_t *out_thresholds);
int covest_draw_histograms(int32_t device, int64_t m, const double *weights, int64_t n_draws, int64_t first_rep,
                           int64_t n_rep, uint64_t seed, int64_t *out_counts);
int covest_draw_histograms_device(int32_t device, int64_t m, const uint64_t *d_thresholds, int64_t n_draws,
                                  int64_t first_rep, int64_t n_rep, uint64_t seed, int64_t *d_out, void *stream);

/* ---- histogram batches: many histograms on ONE model's key set, scored in one pass ----
 * A batch is n_hist histograms (rows of n_keys counts in the model's key order, and a tail each) that share the model's
 * keys, k, r, comb, bounds and threshold.  For a fixed key set p_j(theta) does not depend on the counts, so
 *   LL_b(theta_i) = sum_j h_bj log p_j(theta_i) + tail_b [sp_i < 1] log(1 - sp_i),   sp_i = min(1, fsum(p_j(theta_i)))
 * is ONE evaluation of p per point -- K-direct's arithmetic at the point after fit_to_bounds, bit for bit what
 * covest_probabilities(clamp = 1) returns -- and a contraction with the counts.  Every key of the model enters sp_i,
 * whatever the model's own tail is; a key with h_bj = 0 contributes nothing; a key with h_bj != 0 and p_j <= 0 makes the
 * value -inf (the reference's h * safe_log(0); NaN where another counted key's p_j is NaN).
 *   covest_batch_create     counts[n_hist * n_keys] and tails[n_hist] (NULL: all 0) are HOST doubles, finite and >= 0.
 *   covest_batch_draw       n_hist replicates (first_rep .. of the stream of `seed`) of n_draws draws over the model's
 *                           cells at `params`: p_j at every key and, where the model's tail != 0, one more cell
 *                           max(0, 1 - fsum(p)) whose count becomes the replicate's tail -- the rows covest_draw_histograms
 *                           gives for these weights, bit for bit.  The histograms never leave the device.
 *   covest_batch_counts     the histograms back: out_counts[n_hist * n_keys], out_tails[n_hist].
 *   covest_batch_eval_cross every histogram at every point: out_ll[b * n + i], row-major [n_hist][n].
 *   covest_batch_eval_pairs histogram hist_index[i] at point i: out_ll[n].  One launch pair for many requests.
 *   covest_batch_argmin_cross  per histogram the first index with the strictly smallest -LL over the points (NaN never
 *                           wins: covest/grid.py:65-70) and that value; (-1, +inf) where nothing is below +inf.  The
 *                           values never leave the device.
 *   covest_batch_info       out[8], of the last evaluation on the batch: points tabled, table chunks, 16 x 16 output
 *                           tiles the cross contraction covered, points with keys of p <= 0, fix-up waves launched
 *                           (one per such point and histogram), pairs requests, and the device time in nanoseconds of
 *                           the table kernels and of the contraction kernels.
 *   covest_batch_eval_cross_grad, covest_batch_eval_pairs_grad  the same two forms with the analytic gradient (DESIGN.md
 *                           section 6u): per (histogram, point) param_count + 1 doubles, [0] the log-likelihood and
 *                           [1 + k] its derivative in parameter k at the point after fit_to_bounds (0 for a parameter the
 *                           clamp moved; every derivative NaN where the value is not finite).  The per-key score
 *                           r_k(j) = d_k p_j / p_j does not depend on the counts either:
 *                             d_k LL_b = sum_j h_bj r_k(j) - tail_b [sp < 1] S_k / (1 - sp),   S_k = sum_j d_k p_j,
 *                           so the table has param_count + 1 rows a point, written by the derivative kernel's walk
 *                           (covest_eval_points_grad's arithmetic), and the value returned here is THAT kernel's: it
 *                           agrees with covest_batch_eval_cross / _pairs to 1e-11 relative, not to the bit.
 *   covest_batch_score_table  that table itself: out_rows[n][param_count + 1][n_keys] -- row 0 log p_ij (+0.0 where
 *                           p_ij <= 0 and nowhere else: p = 1 is stored as -0.0; NaN stays NaN), rows 1 + k the scores
 *                           (+0.0 at such a key, and throughout where the clamp moved parameter k) -- and
 *                           out_tail[n][param_count + 1]: log(1 - sp_i), then -S_k / (1 - sp_i); all 0 where sp_i is
 *                           not < 1.  It does not depend on the histograms.
 *   covest_batch_eval_cross_hess, covest_batch_eval_pairs_hess  the same two forms with the closed-form Hessian
 *                           (DESIGN.md section 6x): per (histogram, point) R2 = 1 + P + P (P + 1) / 2 doubles
 *                           (P = param_count: 6 for the basic model, 21 for repeats), [0] the log-likelihood, [1 + k] its
 *                           gradient, [1 + P + pair(k, l)] the entry d_k d_l LL -- of LL, not of -LL -- for k <= l, row by
 *                           row (pair(k, l) = k P - k (k - 1) / 2 + l - k); a row and a column of a parameter the clamp
 *                           moved are 0, every entry behind the value NaN where the value is not finite.  The curvature
 *                           of log p_j does not depend on the counts either:
 *                             d_k d_l LL_b = sum_j h_bj c_kl(j) - tail_b [sp < 1] (S_kl / (1 - sp) + S_k S_l / (1 - sp)^2),
 *                             c_kl(j) = d_k d_l p_j / p_j - r_k(j) r_l(j),   S_kl = sum_j d_k d_l p_j,
 *                           so the table has R2 rows a point, written by the derivative kernel's walk at order 2
 *                           (covest_eval_points_hess's arithmetic); value and gradient are that walk's.
 *   covest_batch_score_table2  that table: out_rows[n][R2][n_keys] -- rows 0 .. P as covest_batch_score_table's, rows
 *                           1 + P + pair(k, l) the c_kl (+0.0 at a key with p_ij <= 0, and throughout where the clamp
 *                           moved k or l) -- and out_tail[n][R2]: the P + 1 coefficients above, then
 *                           -(S_kl / (1 - sp_i) + S_k S_l / (1 - sp_i)^2); all 0 where sp_i is not < 1.
 * params is [n][param_count] as for covest_eval_points.  The table of log p is built for at most 256 MiB of points at
 * a time (the gradient's table holds param_count + 1 rows a point, the Hessian's R2, so a chunk has that many times fewer
 * points); the chunking changes no value.  In covest_batch_info a gradient or Hessian call counts points (not rows) as
 * tabled and its requests as pairs requests; the time fields cover its kernels.
 * A batch borrows its model: destroy the batch first.  Every call takes the model's lock and runs on the model's
 * device.  COVEST_E_INVALID: a NULL argument, a negative size, a count or tail that is negative, NaN or infinite, more
 * than 2^20 histograms, an index outside 0 .. n_hist - 1, a model without keys, and for covest_batch_draw what
 * covest_draw_histograms refuses.  An empty point list or an empty batch: COVEST_OK, nothing written. */
typedef struct covest_batch covest_batch; /* opaque */
int covest_batch_create(covest_model *m, int64_t n_hist, const double *counts, const double *tails, covest_batch **out);
int covest_batch_draw(covest_model *m, const double *params, int64_t n_draws, int64_t first_rep, int64_t n_hist,
                      uint64_t seed, covest_batch **out);
int covest_batch_counts(covest_batch *b, double *out_counts, double *out_tails);
int covest_batch_eval_cross(covest_batch *b, int64_t n, const double *params, double *out_ll);
int covest_batch_eval_pairs(covest_batch *b, int64_t n, const int64_t *hist_index, const double *params, double *out_ll);
int covest_batch_argmin_cross(covest_batch *b, int64_t n, const double *params, double *out_min_negll, int64_t *out_arg);
int covest_batch_eval_cross_grad(covest_batch *b, int64_t n, const double *params, double *out);
    /* out: B x n x (P+1); [..][0] the log-likelihood, [..][1+k] its derivative in parameter k */
int covest_batch_eval_pairs_grad(covest_batch *b, int64_t n, const int64_t *hist_index, const double *params, double *out);
    /* out: n x (P+1) */
int covest_batch_score_table(covest_batch *b, int64_t n, const double *params, double *out_rows, double *out_tail);
    /* out_rows: n x (P+1) x n_keys as the device holds them; out_tail: n x (P+1) */
int covest_batch_eval_cross_hess(covest_batch *b, int64_t n, const double *params, double *out);
    /* out: B x n x R2; [..][0] the log-likelihood, [..][1+k] the gradient, [..][1+P+pair(k,l)] d_k d_l LL, k <= l */
int covest_batch_eval_pairs_hess(covest_batch *b, int64_t n, const int64_t *hist_index, const double *params, double *out);
    /* out: n x R2 */
int covest_batch_score_table2(covest_batch *b, int64_t n, const double *params, double *out_rows, double *out_tail);
    /* out_rows: n x R2 x n_keys as the device holds them; out_tail: n x R2 */
int covest_batch_info(covest_batch *b, int64_t *out);
void covest_batch_destroy(covest_batch *b);

/* ---- histogram down-sampling: covest/histogram.py:47-70 sample_histogram ----
 * Expected counts of the histogram after keeping every read with probability 1/factor, BEFORE the
 * reference's randomised rounding (:71-74, host side): out[j-1] = sum_i counts_i * pmf_i(j) for
 * j = 1 .. out_len, with pmf_i = binomial(i, 1/factor) for i < 100 and Poisson(i/factor) for i >= 100.
 * keys[n] >= 1 are the (already trimmed) source counts i, counts[n] their multiplicities.  HOST buffers.
 * factor must be > 1.  (Where i/factor > 200 the reference's poisson_dist is itself wrong -- see
 * DESIGN.md -- and this returns the correct Poisson pmf.) */
int covest_thin_histogram(int32_t device, int64_t n, const int32_t *keys, const double *counts, double factor,
                          int64_t out_len, double *out);
/* The same, launched `repeats` times with inputs resident in HBM; *kernel_ms = mean device time of one
 * launch pair (hipEvents on the launch stream).  For benchmarks. */
int covest_thin_histogram_timed(int32_t device, int64_t n, const int32_t *keys, const double *counts, double factor,
                                int64_t out_len, double *out, int32_t repeats, double *kernel_ms);

/* PROFILING AID: with the environment variable COVEST_FACTORED_DIAG set at
 * covest_grid_create, the factored kernel accumulates s_memtime stamps per wave
 * ([workgroup][wave][8] int64: build, contract, log, barrier cycles); this copies
 * up to n of them to the host and returns how many exist.  Not part of the
 * reference's interface. */
int64_t covest_grid_diag(covest_grid *g, int64_t *out, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* COVEST_AMD_H */
