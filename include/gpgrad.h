/* gpgrad.h -- C ABI of the MI355X-native gradient-enhanced GP likelihood hot path.
 *
 * This is the drop-in boundary: every entry point replaces one step of the reference
 * (marchildon/gpgradpy @ v2; citations are file:line in that tree).  Plain pointers and sizes only;
 * the caller owns every host buffer, the library owns every device allocation.
 *
 * Return convention (all int-returning functions):
 *    0   success
 *   >0   LAPACK-style info: 1-based index of the first non-positive pivot met by the Cholesky
 *        factorisation -> the caller treats it like the `except` branch of Kernel.py:253-264
 *        (Kcov_chofac = None, b_chofac_good = False)
 *   <0   argument / HIP runtime error; text via gpg_last_error()
 *
 * Threading: one context = one device + one HIP stream, not re-entrant (the reference object is not
 * thread-safe either: memoised `_last_hp_vec`, mutable `_time_chofac`).
 *
 * Matrix layout: derivative-major blocks (KernelSqExp.py:381-408, CommonFun.py:151-173): row
 * r = blk * n + a, blk 0 = function value, blk i+1 = d/dx_i at point a.  Device storage is
 * column-major, lower triangle, padded to a multiple of 128.
 */
#ifndef GPGRAD_H
#define GPGRAD_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpg_ctx gpg_ctx;

/* RatQu = the rational quadratic kernel of KernelRatQuad.py, with its own hyperparameter alpha (gpg_hp.hp_kernel). */
enum { GPG_KERNEL_SQEXP = 0, GPG_KERNEL_MA5F2 = 1, GPG_KERNEL_RATQU = 2 };
enum { GPG_WELLCOND_BASE = 0, GPG_WELLCOND_PRECON = 1 };

/* Hyperparameters + regularisation of ONE evaluation.
 * Mirrors HparaOptzVal (GpHpara.py:12-19) plus the scalars calc_all_K_w_chofac reads from the object
 * (Kernel.py:186-236: theta, varK, noise, self._etaK, self.wellcond_mtd). */
typedef struct {
  const double* theta; /* [d] > 0                                                              */
  double varK_mat;     /* varK the matrix is built with: 1 for noise-free data and for          */
                       /* b_normlz_w_varK (Kernel.py:137-138,196-197), hp_vals.varK otherwise   */
  double var_fval;     /* >= 0: noise variance of every function value (unknown-noise case,     */
                       /*       Kernel.py:348); < 0: use the per-row vector given to set_data   */
  double var_fgrad;    /* same for every gradient entry (Kernel.py:355)                         */
  double eta;          /* nugget etaK (GpWellCond.py:116-154, Kernel.py:229-236)                */
  int wellcond;        /* GPG_WELLCOND_PRECON (Kernel.py:220-266) or _BASE (Kernel.py:268-302)  */
  int closed_form_varK;/* 1: noise-free path, varK = max(1e-32, r'K^-1 r / N) (CalcLkd.py:159); */
                       /* 0: noisy path, ln_lkd = -(ln_det + r'K^-1 r)/2 (CalcLkd.py:226)       */
  double hp_kernel;    /* hyperparameter of the kernel itself (HparaOptzVal.kernel): alpha > 0   */
                       /* of GPG_KERNEL_RATQU (KernelRatQuad.py:468); ignored by the others      */
} gpg_hp;

/* Result of one likelihood evaluation = the scalar fields of LkdInfo (CalcLkd.py:14-26). */
typedef struct {
  double ln_lkd;  /* marginal log-likelihood, without the N ln(2 pi) constant (CalcLkd.py:168,226) */
  double ln_det;  /* 2 sum log diag(P L)                               (CalcLkd.py:165,225)       */
  double beta;    /* GLS constant mean; beta[0] with mean order 1       (GpMeanFun.py:103-107)     */
  double varK;    /* closed-form varK, or varK_mat on the noisy path    (CalcLkd.py:159)           */
  double rKr;     /* r' Kcov^-1 r with r = y - V beta                   (CalcLkd.py:154,221)       */
  int info;       /* 0, or first non-positive pivot (1-based)                                      */
  int pad_;
} gpg_lkd_out;

/* Lifetime --------------------------------------------------------------------------------------- */

/* Replaces GaussianProcess.__init__ + the shape part of set_data (GaussianProcess.py:138-190,
 * 244-262).  n_eval points of dimension dim; use_grad != 0 -> N = n_eval * (dim + 1) rows.
 * Allocates the (N_pad + 128) x N_pad fp64 workspace once.  dim <= 16. */
int gpg_create(gpg_ctx** out, int device, int n_eval, int dim, int use_grad, int kernel);
void gpg_destroy(gpg_ctx* ctx);
const char* gpg_last_error(const gpg_ctx* ctx); /* ctx may be NULL: error of the last failed create */

/* Optional, before gpg_set_data: replaces the bvec_use_grad handling of set_data / calc_KernGrad
 * (GaussianProcess.py:246-262, KernelSqExp.py:349-377).  use_grad_pt [n_eval] != 0 marks the points whose
 * gradient enters the model; NULL restores "all".  N becomes n_eval + n_grad * dim and data_vec / noise_var
 * of gpg_set_data are [N] with the gradient part laid out [n_grad, dim] column-major (CommonFun.py:170-171). */
int gpg_set_grad_mask(gpg_ctx* ctx, const unsigned char* use_grad_pt);

/* Replaces the data ingest of set_data (GaussianProcess.py:296-302,363) and make_data_vec
 * (CommonFun.py:151-173).  x [n_eval, dim] row-major; data_vec [N] = [f, d1 f(all pts), ...];
 * noise_var [N] = known noise variances in the same ordering (Kernel.py:343-353) or NULL (zeros).
 * The [d, n, n] Rtensor of the reference is never materialised. */
int gpg_set_data(gpg_ctx* ctx, const double* x, const double* data_vec, const double* noise_var);

/* Replace the per-row noise variances only (host [N], NULL = zeros): what calc_all_K_w_chofac(..., noise_vec = ...) passes in
 * (Kernel.py:140-143, 207-208, 218).  Likelihood-side state is invalidated; a posterior set up by gpg_setup_eval keeps its factor. */
int gpg_set_noise(gpg_ctx* ctx, const double* noise_var);

/* Mean function (GpMeanFun.py).
 *   0 (default): constant mean, V = [1_n; 0] (GpMeanFun.py:160-163).
 *   1: first-order polynomial ('poly_ord_1', universal kriging), n_beta = dim + 1, V = calc_aug_vand (GpMeanFun.py:172-191):
 *      value row a: [1, x_a]; gradient row (i, a): e_(i+1) (points masked by gpg_set_grad_mask have no gradient rows).
 * x is the x given to gpg_set_data (with a data-rescaling method the caller passes the scaled x, as the reference uses
 * get_scl_x_w_dist).  The dim + 1 columns of V P^-1 and y P^-1 ride through every factorisation schedule as right-hand-side
 * rows (dim + 2 <= 18 of the 128), so L^-1 P^-1 [V, y] costs no extra N^3 work; the (dim+1) x (dim+1) GLS system
 * (calc_model_max_lkd_poly, GpMeanFun.py:69-122) is formed, factorised and solved by one workgroup per matrix on the device.
 * Invalidates likelihood- and posterior-side state; callable before or after gpg_set_data.  With order 1:
 *   - gpg_lkd, gpg_lkd_grad, gpg_lkd_batch, gpg_lkd_grad_batch, gpg_multi_lkd_batch and gpg_lkd_alpha use the GLS optimum beta
 *     [n_beta]; gpg_lkd_out.beta is beta[0] (gpg_lkd_beta gives the vector).  The adjoint gradient formulas are unchanged
 *     (V' alpha = 0 still holds).  A singular V' Kcov^-1 V (no gradients and fewer than dim + 1 points, or points that are not
 *     affinely independent) gives info = N + 1 + j, j the 0-based pivot of the small system, and NaN results.  The call then
 *     counts as a failed factorisation in every respect: although the Cholesky factor of the matrix itself is good, the context
 *     marks it invalid (gpg_get_matrix 3 and gpg_factor_apply refuse until the next successful call).
 *   - gpg_predict* add the mean and its gradient: mu += beta_0 + xq . beta_1..d, dmudx += beta_1..d; d2mudx2 is unchanged (the
 *     Hessian of the mean is zero).  sig, dsigdx, d2sigdx2 and gpg_predict_var are unchanged by the mean order: as in the reference,
 *     the posterior variance treats the mean coefficients as known unless gpg_set_mean_uncertainty switches their uncertainty in.
 *   - gpg_get_matrix, gpg_factor_apply, gpg_dcov_quadform, gpg_cond_fro, gpg_abs_rowsum and gpg_kern_* do not depend on the mean. */
int gpg_set_mean_order(gpg_ctx* ctx, int order);

/* Likelihood ------------------------------------------------------------------------------------- */

/* Replaces CalcLkd.calc_lkd_all(hp, calc_lkd=True, calc_cond=False, calc_grad=False)
 * (CalcLkd.py:270-346): assembly + noise + preconditioner + nugget (Kernel.py:213-237), Cholesky
 * (Kernel.py:251), GLS mean (GpMeanFun.py:69-122), alpha-free evaluation of r'K^-1 r and ln det
 * (CalcLkd.py:149-181 / 185-251).  Returns out->info as well. */
int gpg_lkd(gpg_ctx* ctx, const gpg_hp* hp, gpg_lkd_out* out);

/* Replaces CalcLkd.calc_lkd_all(hp, calc_grad=True) with the adjoint method (CalcLkd.py:170-177, 230-235;
 * kernel derivatives GpHparaGrad.py:13-155, KernelSqExp.py:470-568, KernelMatern5f2.py:532-642).
 * out as gpg_lkd.  g_aa, g_inv hold dim + 4 entries: hyperparameter slot k = theta_0..theta_(dim-1), varK, var_fval,
 * var_fgrad, hp_kernel (the last one zero unless the kernel has a hyperparameter of its own: alpha of GPG_KERNEL_RATQU,
 * KernelRatQuad.py:752-843):
 *   g_aa[k]  = sum_{r,c} G_k[r,c] alpha_r alpha_c,    g_inv[k] = sum_{r,c} G_k[r,c] (-1/2 Kcov^-1)[r,c],
 * G_k = d Kcov / d hp_k, alpha = Kcov^-1 (y - V beta).  The caller forms ln_lkd_grad = s g_aa + g_inv with
 * s = 1/2 (noisy, CalcLkd.py:233) or pnlt'/N + 1/(2 varK) (noise-free, CalcLkd.py:173-175).  Neither the
 * [n_hp, N, N] derivative tensor nor a dense identity solve is formed; costs two more N^3/3 sweeps. */
int gpg_lkd_grad(gpg_ctx* ctx, const gpg_hp* hp, gpg_lkd_out* out, double* g_aa, double* g_inv);

/* Replaces the serial restart loop of GpHparaX0.select_hp_optz_x0 (GpHparaX0.py:33-59) on ONE
 * device: m hyperparameter rows, hp_rows [m, row_len] with row = [theta(d), varK_mat, var_fval,
 * var_fgrad (, hp_kernel if row_len >= d + 4: alpha of GPG_KERNEL_RATQU)] already decoded from log10
 * (GpHpara.py:56-103); eta / wellcond / closed_form_varK are shared (row_len > dim + 4: column dim + 4 carries a nugget per row instead).  out [m].  Rows whose factorisation fails get info > 0 and NaN ln_lkd (GpHparaX0.py:34,
 * 43-45).  Returns 0 unless an argument / runtime error occurred.  All m evaluations are queued on
 * the stream back-to-back and synchronised once. */
int gpg_lkd_batch(gpg_ctx* ctx, int m, const double* hp_rows, int row_len, double eta, int wellcond,
                  int closed_form_varK, gpg_lkd_out* out);

/* beta [n_beta] (1 or dim + 1 entries, gpg_set_mean_order) of the most recent successful gpg_lkd / gpg_lkd_grad on this context
 * (no batched call in between); gpg_lkd_out.beta stays beta[0].  Replaces LkdInfo.hp_beta (CalcLkd.py:14-26). */
int gpg_lkd_beta(gpg_ctx* ctx, double* beta);

/* Value AND adjoint gradient of m restart rows in one call: what m SLSQP runs of the reference's multi-start
 * (OptzLkd.py:249-290, one calc_store_likelihood per iterate: OptzLkd.py:15-100) ask for when they advance in lock step.
 * Rows as gpg_lkd_batch; out [m]; g_aa, g_inv [m, dim + 4] row-major with the slots of gpg_lkd_grad.  Rows whose
 * factorisation fails get info > 0 and NaN gradients.  The factorisations, the two N^3/3 sweeps of the explicit inverse
 * (W = L^-T, -(W W^T)) run as ONE dataflow launch each per group of up to 8 rows; results are bit-identical to m calls
 * of gpg_lkd_grad. */
int gpg_lkd_grad_batch(gpg_ctx* ctx, int m, const double* hp_rows, int row_len, double eta, int wellcond,
                       int closed_form_varK, gpg_lkd_out* out, double* g_aa, double* g_inv);

/* Several devices, one process -------------------------------------------------------------------- */

/* The restart table of GpHparaX0.select_hp_optz_x0 (GpHparaX0.py:33-59) sharded over the devices of ONE process: one
 * context per listed device (devices == NULL: 0 .. ndev-1; a device may be listed more than once), one host thread per
 * context, contiguous row blocks (rows differ by at most one between devices), the results gathered in `out` [m] and
 * the row of the highest ln_lkd among the successfully factorised ones in *best (-1 if none; may be NULL).  The data
 * set is replicated by gpg_multi_set_data.  This is the in-library form of the partition DESIGN.md section 5 runs with
 * one process per GPU over torch.distributed / RCCL. */
typedef struct gpg_multi gpg_multi;
int gpg_multi_create(gpg_multi** out, int ndev, const int* devices, int n_eval, int dim, int use_grad, int kernel);
void gpg_multi_destroy(gpg_multi* m);
const char* gpg_multi_last_error(const gpg_multi* m); /* m may be NULL: error of the last failed create */
int gpg_multi_count(const gpg_multi* m);
int gpg_multi_set_data(gpg_multi* m, const double* x, const double* data_vec, const double* noise_var);
int gpg_multi_set_mean_order(gpg_multi* m, int order);   /* gpg_set_mean_order on every context */
int gpg_multi_lkd_batch(gpg_multi* m, int nrows, const double* hp_rows, int row_len, double eta, int wellcond,
                        int closed_form_varK, gpg_lkd_out* out, int* best);

/* Posterior -------------------------------------------------------------------------------------- */

/* Replaces GpEvalModel.setup_eval_model (GpEvalModel.py:17-57): factorises the matrix for hp (the
 * caller passes varK_mat = 1, noise undivided: the b_normlz_w_varK quirk of Kernel.py:196-197,218)
 * and keeps the factor plus alpha = Kcov^-1 (y - V beta) on the device.  alpha_out [N] may be NULL.
 * The factor lives in a workspace of its own (allocated by the first call: one more (N_pad + 128) x N_pad fp64
 * array): gpg_lkd / gpg_lkd_grad / gpg_lkd_batch / gpg_get_matrix calls that follow do NOT disturb it, and
 * gpg_predict* keep answering from it until the next gpg_setup_eval / gpg_set_data -- as KernEta_chofac of the
 * reference survives later calc_lkd_all calls. */
int gpg_setup_eval(gpg_ctx* ctx, const gpg_hp* hp, double beta, double* alpha_out);
/* The same with a coefficient vector beta [n_beta] (eval_mean_fun_poly, GpMeanFun.py:14-67).  With mean order 1 this is the call
 * to use: gpg_setup_eval (scalar beta) then returns -1 and says so; with order 0 it reads beta[0]. */
int gpg_setup_eval_mean(gpg_ctx* ctx, const gpg_hp* hp, const double* beta, double* alpha_out);

/* Replaces GpEvalModel.eval_model(x, calc_grad=False) (GpEvalModel.py:59-198): cross-kernel
 * (GpEvalModel.py:133-139), K^-1 Kyx (GpEvalModel.py:154), mu = beta + Kyx' alpha (:168),
 * sig = sqrt(max(0, 1 - diag(Kxy K^-1 Kyx))) * sqrt(varK) (:162-166).  xq [nx, dim] row-major.
 * sig2_raw [nx] (may be NULL) receives the unclipped 1 - diag(...) that the reference asserts to be
 * non-negative (GpEvalModel.py:163).  As in the reference, sig treats the mean coefficients as known; with
 * gpg_set_mean_uncertainty on, sig2_raw (and with it sig) gains u' (V' Kcov^-1 V)^-1 u of that switch. */
int gpg_predict(gpg_ctx* ctx, int nx, const double* xq, double varK, double* mu, double* sig,
                double* sig2_raw);

/* Replaces eval_model(x, calc_grad=True) (GpEvalModel.py:133-140,170-172,319-354): additionally returns
 * dmudx, dsigdx [nx, dim] row-major.  The derivative blocks of the cross-kernel are recomputed on the fly
 * (the [N, nx*dim] matrix dKxy_dx is never formed); K^-1 Kyx costs one extra triangular sweep per query. */
int gpg_predict_grad(gpg_ctx* ctx, int nx, const double* xq, double varK, double* mu, double* sig,
                     double* sig2_raw, double* dmudx, double* dsigdx);

/* Replaces GpEvalModel.eval_model_var(x, calc_grad) (GpEvalModel.py:200-317): the variance form of the posterior,
 * sig2 [nx] = varK (1 - diag(Kxy K^-1 Kyx)) (:297, NOT clipped at zero: the reference asserts min >= 0 on it) and, when
 * dsig2dx != NULL, its gradient [nx, dim] row-major = -2 varK sum_r dKxy_dx[., r] (K^-1 Kyx)[r] (calc_dsig2dx :327-337;
 * defined where sig = 0, unlike dsigdx). */
int gpg_predict_var(gpg_ctx* ctx, int nx, const double* xq, double varK, double* sig2, double* dsig2dx);

/* Posterior Hessians at ONE query point xq[d] (the reference evaluates them one point per call):
 * d2mudx2[d*d], d2sigdx2[d*d] row-major, plus everything gpg_predict_grad returns for that point.
 * Replaces eval_model(calc_grad=True, calc_hess=True) -- GpEvalModel.py:170-181, calc_d2mudx2 :355-363,
 * calc_d2sigdx2 :365-380, calc_Kern_hess_x (KernelSqExp.py:48-88,412-468, KernelMatern5f2.py:54-94,453-530).
 * d2sigdx2 is NaN where sig == 0, as in the reference. */
int gpg_predict_hess(gpg_ctx* ctx, const double* xq, double varK, double* mu, double* sig, double* dmudx,
                     double* dsigdx, double* d2mudx2, double* d2sigdx2);

/* Joint posterior at nx query points, from the factor kept by gpg_setup_eval.
 * with_grad = 0: m = nx rows (function values).
 * with_grad = 1: m = nx (dim + 1) rows, derivative-major like the training data:
 *   row r = blk * nx + j, blk 0 = f(x_j), blk k+1 = d f / d x_k at x_j.
 * mean [m]; cov [m, m] row-major, exactly symmetric:
 *   cov = varK (Kqq - Kqy Kcov^-1 Kyq)
 * Kqq: the kernel matrix of the query points with themselves (no nugget, no noise: the latent function).
 * Kqy: the cross-covariance that gpg_predict_grad already uses (training-side gradient mask honoured); it also works for a
 *   model built without training gradients (use_grad = 0) and with_grad = 1.
 * Kcov: the matrix gpg_setup_eval factorised.
 * mean includes the mean function: beta_0 (+ xq . beta_1..d, and beta_k on the gradient rows, with mean order 1).
 * As in the reference, the mean coefficients count as known: cov does not hold their uncertainty unless gpg_set_mean_uncertainty is
 * on, which adds varK U (V' Kcov^-1 V)^-1 U^T (exactly symmetric as well; mean is the same bits either way).
 * Not clipped: tiny negative diagonal entries are returned as computed.
 * mean or cov may be NULL.  m padded to a multiple of 64 must be <= 4096 (-1 beyond), and gpg_setup_eval must have succeeded (-1).
 * On the device: the cross-covariance rows of all points and blocks, one multi-row forward sweep Z = Kqy P^-1 L^-T, then
 * G = Z Z^T by a split-K fp64 MFMA kernel on the lower 64 x 64 tiles (partials added in fixed chunk order by a second launch,
 * which also subtracts from Kqq and mirrors the tile): ordinary grids, no atomics, so the result is the same bits from run to
 * run and under any gpg_set_max_workgroups. */
int gpg_predict_joint(gpg_ctx* ctx, int nx, const double* xq, double varK, int with_grad, double* mean, double* cov);

/* Uncertainty of the GLS mean coefficients beta in the posterior (universal kriging; the reference has no counterpart: it treats beta
 * as known).  on = 0 (default): every output is what it was without this switch, bit for bit.  on = 1: with
 *   V [N, n_beta]  the augmented Vandermonde matrix of the model (gpg_set_mean_order),
 *   H = V' Kcov^-1 V,  Kcov the matrix gpg_setup_eval factorised (varK := 1),
 *   u_r = v_r - V' Kcov^-1 k_r,  k_r the cross-covariance column of query row r and v_r its mean basis: [1] or [1, x_j] on a value
 *         row, 0 or e_(k+1) on the row of d/dx_k,
 * the joint covariance becomes varK (Kqq - Kqy Kcov^-1 Kyq + U H^-1 U'), U [m, n_beta] = rows u_r, and
 *   gpg_predict, gpg_predict_grad, gpg_predict_var, gpg_predict_hess: sig, sig2_raw, sig2, dsigdx, dsig2dx, d2sigdx2 are those of
 *       sig2 = varK (1 - k' Kcov^-1 k + u' H^-1 u)  (sig = sqrt(max(0, .)), dsigdx = 0 where sig = 0, as without the switch);
 *   gpg_predict_joint: cov gains varK U H^-1 U'.
 * mu, dmudx, d2mudx2 and the joint mean do not change.  Callable before or after gpg_setup_eval*; values other than 0 / 1 return -1.
 * Cost: W_V = L^-1 P^-1 V and K^-1 V (n_beta forward and backward rows, O(n_beta N^2)) once per gpg_setup_eval, by the first call
 * that needs them; per query row one more pass over its swept row (O(n_beta N)).  If H is not positive definite (the pivot rule of
 * the GLS solve: a pivot not above 1e-12 of its diagonal entry) the predict call returns -1 and names the pivot.  Ordinary grids,
 * no atomics: the same bits from run to run and under any gpg_set_max_workgroups. */
int gpg_set_mean_uncertainty(gpg_ctx* ctx, int on);

/* H = V' Kcov^-1 V [n_beta, n_beta] (row-major, symmetric) of the posterior kept by gpg_setup_eval*: varK H^-1 is the covariance of
 * the GLS coefficients.  Independent of gpg_set_mean_uncertainty.  -1 with a message before a successful gpg_setup_eval*, and -1
 * with the pivot named if H is not positive definite by the rule above (H is written all the same). */
int gpg_mean_gram(gpg_ctx* ctx, double* H);

/* Leave-one-out cross-validation of the posterior kept by gpg_setup_eval*, point by point and without a refit (the reference has
 * no counterpart).  The unit left out is the point: its value row a and, if it carries a gradient, its rows n + k ng + gpos[a],
 * k = 0..dim-1 (the row layout of gpg_set_data; gpg_set_grad_mask honoured).  bs = dim + 1 with use_grad, else 1.  With
 *   B = Kcov^-1, Kcov the matrix gpg_setup_eval factorised (varK := 1, noise and nugget included), alpha = Kcov^-1 (y - V beta):
 *   prec  [n, bs, bs] row-major, exactly symmetric: the block of B on the rows of point a; with gpg_set_mean_uncertainty on the
 *         block of Q = B - B V (V' B V)^-1 V' B (the mean coefficients are re-estimated without the point: Dubrule's formulas).
 *         A point without gradient rows has entry [0, 0] only, the rest of its block is 0.0.
 *   qy    [N]: alpha, the same bits as alpha_out of gpg_setup_eval*; with the switch on Q y = alpha - B V (V' B V)^-1 V' alpha
 *         (the correction is formed even though it vanishes in exact arithmetic when beta is the GLS optimum).
 *   resid [N] in data_vec order: on the rows of a, prec_a^-1 qy_a = the observed data minus their prediction from all other points.
 *   cov   [n, bs, bs] = varK prec_a^-1, exactly symmetric, laid out as prec: the covariance of that prediction of the OBSERVED rows
 *         (noise and nugget are part of it).
 * Each block is inverted through its Cholesky factor on the device, with the pivot rule of the GLS solve: a pivot not above
 * 1e-12 of the diagonal entry it started from marks the block bad -- NaN in that point's resid and cov; *n_bad counts the bad
 * blocks and the call still returns 0.  Any output pointer may be NULL.  -1 with a message before a successful gpg_setup_eval*;
 * with mean uncertainty on, -1 naming the pivot if V' B V is not positive definite; -2 out of memory.
 * On the device: W = L^-T by the one-launch dataflow sweep of the gradient path (N^3/3 flops), then only the n point-diagonal
 * blocks of W W^T -- one pass over the upper triangle of W (4 N^2 bytes, N^2 (dim + 2) / 2 flops) instead of the second N^3/3
 * sweep behind the full inverse -- as K-chunk partials added in chunk order, and one thread per point for the block algebra.
 * Ordinary grids, no atomics: the same bits from run to run and under any gpg_set_max_workgroups.  Likelihood-side state
 * (gpg_lkd*, gpg_cond_fro) is neither read nor invalidated. */
int gpg_loo(gpg_ctx* ctx, double varK, double* resid, double* cov, double* prec, double* qy, int* n_bad);

/* Number of K-chunks of the Gram kernel of gpg_predict_joint: 0 = automatic, a function of (m, N_pad) only -- never of the
 * device, the grid or gpg_set_max_workgroups; n >= 1: that many, capped at N_pad / 64.  Different chunk counts add the same
 * products in a different order: results agree to rounding, not bitwise. */
int gpg_set_gram_splits(gpg_ctx* ctx, int n);

/* Per-point covariance of [f, grad f] and batched Hessians of the posterior at nx query points (any nx >= 1), from the factor kept
 * by gpg_setup_eval* (the reference has no counterpart: its Hessians are one point per call and it has no gradient covariance).
 * bs = dim + 1; index 0 is f(x_j), index k + 1 is d f / d x_k at x_j.  Every output pointer may be NULL (not all of them); what
 * is not asked for is not computed (no sweep without gcov or a Hessian; no backward sweep and no contraction without a Hessian).
 *   mu      [nx], dmudx [nx, dim]: posterior mean and its gradient, mean function included (beta_0 (+ xq . beta_1..d) on mu,
 *           beta_k+1 on dmudx with mean order 1): the rows gpg_predict_joint puts in `mean`.
 *   gcov    [nx, bs, bs] row-major: gcov_j = varK (K0 - Z_j Z_j'), Z_j the bs forward-swept cross-covariance rows of x_j and K0
 *           the prior block of one point with itself from the kernel table (the numbers gpg_predict_joint uses): the j-th
 *           point-diagonal block of the cov of gpg_predict_joint(with_grad = 1) without the rest of that matrix.  gcov_j[0, 0] =
 *           sig^2, gcov_j[0, k + 1] = 1/2 d sig^2 / d x_k, gcov_j[1.., 1..] = Cov(grad f).  Exactly symmetric, not clipped.  The
 *           training-side gradient mask is honoured, and a model built with use_grad = 0 is fine, as for gpg_predict_joint.
 *   d2mudx2, d2sigdx2 [nx, dim, dim]: what gpg_predict_hess returns for each point, with sig and dsigdx taken from the block:
 *           sig = sqrt(max(0, gcov_00)), dsigdx_k = gcov_0,k+1 / sig, d2sig2 = -2 varK (H2 + T), T = (Z_j Z_j')[1.., 1..],
 *           d2sigdx2 = (d2sig2 - 2 dsigdx dsigdx') / (2 sig); NaN where sig == 0.
 * With gpg_set_mean_uncertainty on, every block gains varK U_j H^-1 U_j' and d2sigdx2 the terms gpg_predict_hess adds; mu, dmudx
 * and d2mudx2 do not change.
 * The host loops over chunks of points whose rows fit the row buffer of the posterior calls: at most 4096 rows, the automatic
 * point count the largest multiple of 64 with points * bs <= 4096 (192 points at dim 16, 448 at dim 8), and the last chunk
 * everything that is left once its rows fit (so nx <= 4096 / bs is one chunk).  Per chunk: the cross rows
 * and the mean as gpg_predict_joint, ONE forward sweep over all rows, a per-point Gram kernel (lane <-> query point, K-chunk
 * partials added in chunk order by a finishing kernel, which also subtracts from K0, scales and mirrors), and for the Hessians
 * one backward sweep of the value rows and one contraction launch with a grid over (row, point); one device-to-host copy per
 * output and one synchronisation.  The K-chunk count is min(N_pad / 64, 64), or gpg_set_gram_splits when set: never a function of
 * nx or of the chunk's point count.  Ordinary grids, no atomics: the same bits from run to run and under any
 * gpg_set_max_workgroups.  -1 with a message before a successful gpg_setup_eval*, for nx < 1 and when every output is NULL.
 * Measured on one MI355X (tools/second_time.py; n = 2000, d = 8 | n = 500, d = 4):
 *   gcov alone at the largest nx gpg_predict_joint takes (455 | 819): 26.5 ms | 0.87 ms = forward sweep 26.1 | 0.74 ms + Gram kernel
 *   0.122 ms (0.591 GB of Z: 4.8 TB/s) | 20.8 us (4.0 TB/s) + 0.25 | 0.11 ms for the rest, against 37.3 | 4.37 ms of gpg_predict_joint;
 *   Hessians of 64 points in one call 8.7 | 1.05 ms against 267 | 41.5 ms for 64 gpg_predict_hess calls. */
int gpg_predict_second(gpg_ctx* ctx, int nx, const double* xq, double varK, double* mu, double* dmudx, double* gcov,
                       double* d2mudx2, double* d2sigdx2);
/* Diagnostic, like gpg_set_gram_splits: query points per chunk of gpg_predict_second.  0 = automatic (above); points >= 1: that
 * many (a multiple of 64 keeps the reads of the Gram kernel aligned), so that tests reach several chunks with a small nx.
 * points < 0 and points (dim + 1) > 4096 return -1.  Chunked and unchunked results agree to rounding at least. */
int gpg_set_second_chunk(gpg_ctx* ctx, int points);

/* Posterior sample paths: functions drawn from the posterior kept by gpg_setup_eval*, by pathwise conditioning (Matheron's rule) on
 * a random-Fourier-feature prior (the reference has no counterpart).  For path s
 *     f_s(x) = m(x) + k(x, X) c_s + sqrt(varK) phi(x)' w_s,       c_s = alpha - sqrt(varK) Kcov^-1 (Phi_X w_s + D^(1/2) z_s),
 * m the mean function, alpha = Kcov^-1 (y - V beta) and Kcov of gpg_setup_eval*, k(x, X) the cross-covariance rows of gpg_predict_joint,
 * phi(x)_m = sqrt(2 / M) cos(omega_m . x + phase_m), Phi_X [N, M] its values on the value rows and d phi / d x_k on the gradient rows of
 * the training data (row layout of gpg_set_data, gpg_set_grad_mask honoured), D [N] = diag(Kcov) - diag(Kern): noise / varK_mat plus
 * the nugget as the well-conditioning method adds it (eta dvec for PRECON, eta for BASE), taken as the difference of the two diagonals
 * as gpg_get_matrix(1) and (0) return them.  With omega drawn from the spectral density of the kernel (the host's business: the device
 * never needs the law) and w, z standard normal, f_s is a draw from the posterior up to the random-feature approximation of the prior.
 * Given (omega, phase, w, z) a path is ONE smooth function: gpg_paths_eval at any points, in any number of calls, evaluates the same
 * function, and dfdx is its exact gradient.
 * Cost: the set-up is the feature rows of the training data plus one forward and one backward multi-row sweep of S rows through the kept
 * factor, O(S N^2), no factorisation; an evaluation is the cross rows plus an [nx (dim + 1)] x N x S product on fp64 MFMA and the feature
 * rows of the query points: no sweep, no N^2 work, no row cap (the host loops over chunks of points as gpg_predict_second does,
 * gpg_set_second_chunk applies), one device-to-host copy per output and one synchronisation per call.  The mean part m(x) + k(x, X) alpha
 * is summed with compensation by the kernels of gpg_predict_joint and is the same bits as its `mean`; the deviation is a split-K sum
 * with min(N_pad / 64, 64) K-chunks (gpg_set_gram_splits overrides) added in chunk order, the features are added in one fixed order.
 * Ordinary grids, no atomics: the same bits from run to run, under any gpg_set_max_workgroups, and whichever other points share the call.
 * Likelihood-side state is neither read nor invalidated.
 * The automatic chunk of gpg_paths_eval holds 4096 / (S_pad / 64) rows (at least 256), a function of S and dim only, so the split-K
 * partials stay within 128 MB for any S.
 * Registers (-Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / scratch bytes / waves per SIMD): rows_coeff_splitk_kernel
 * 50 / 0 / 5; feature_rows_kernel d = 1: 60 / 0 / 8, d = 4: 64 / 0 / 8, d = 8: 77 / 0 / 6, d = 16: 131 / 0 / 3; paths_finish_kernel
 * 40 / 0 / 8.  No kernel of paths.hip uses scratch.
 * Measured on one MI355X (tools/paths_time.py, S = 64, M = 4096; n = 2000, d = 8 | n = 500, d = 4; the full table is in README.md,
 * "Posterior sample paths"):
 *   gpg_paths_setup 11.2 | 2.6 ms = feature kernel 0.77 | 0.46 ms + two sweeps 6.45 | 0.89 ms + host transposition, uploads, launches;
 *   gpg_paths_eval with gradients at nx = 64: 0.57 | 0.43 ms = cross rows 18 | 8 us + product kernel 46 | 11 us (29.0 | 9.6 TFLOP/s,
 *   Wt read at 1.8 | 0.6 TB/s) + feature kernel 368 | 327 us + mean, finishing kernel, copies; at nx = 448: 1.22 | 0.55 ms (product
 *   kernel 228 | 25 us: 40.8 | 29.2 TFLOP/s, 2.6 | 1.9 TB/s; feature kernel 484 | 345 us);
 *   for scale, same points, same build: gpg_predict_grad 6.54 | 0.95 ms (nx = 64), 8.81 | 1.04 ms (nx = 448); gpg_predict_joint
 *   5.03 | 0.61 ms and 35.6 | 1.70 ms.
 * An evaluation pays no sweep (11x below gpg_predict_grad at N = 18000), but it is not "about the cost of the cross rows": two thirds
 * of it is the feature kernel on the query rows (one workgroup per point over all M features). */

/* S paths on the posterior kept by gpg_setup_eval*.  omega [M, dim] row-major, phase [M], w [S, M], z [S, N] (NULL = zeros:
 * no noise/nugget draw), all host.  1 <= S <= 1024, 1 <= M <= 65536, varK >= 0 (what gpg_predict* take as varK).  -1 with a message
 * before a successful gpg_setup_eval*, for arguments out of range, and with gpg_set_mean_uncertainty on (paths with re-drawn mean
 * coefficients are out of scope); -2 out of memory. */
int gpg_paths_setup(gpg_ctx* ctx, int n_paths, int n_feat, const double* omega, const double* phase,
                    const double* w, const double* z, double varK);
/* f [S, nx]; dfdx [S, nx, dim] (NULL = not computed, and then no derivative rows are built).  Any nx >= 1.  -1 with a message when no
 * paths are set up, or when gpg_setup_eval*, gpg_set_data, gpg_set_grad_mask or gpg_set_mean_order ran since gpg_paths_setup: the paths
 * belong to that posterior. */
int gpg_paths_eval(gpg_ctx* ctx, int nx, const double* xq, double* f, double* dfdx);
/* c [S, N] (the coefficient vectors above) and, if not NULL, ddiag [N] = the diagonal D that was used (either may be NULL, not both).
 * Errors as gpg_paths_eval. */
int gpg_paths_coeff(gpg_ctx* ctx, double* c, double* ddiag);

/* Materialisation on request (the 7-tuple of Kernel.py:307 carries N x N arrays; the fast path never
 * copies them).  out is [N, N] column-major == row-major (symmetric) for which = 0..2:
 *   0 Kern (Kernel.py:213-216), 1 Kcov (Kernel.py:237 / 277), 2 the matrix that is factorised
 *   (Kcov_precon, Kernel.py:236; equals Kcov for wellcond = base);
 *   3 the Cholesky factor of the most recent factorisation (gpg_lkd / gpg_lkd_grad / gpg_setup_eval), as the
 *     lower-triangular P L of Kernel.py:252 (row-major [N, N], zeros above the diagonal) usable with
 *     scipy.linalg.cho_solve((out, True), b);
 *   4 the same for the factor KEPT by the last successful gpg_setup_eval, whatever likelihood calls came after it
 *     (hp ignored for 3 and 4). */
int gpg_get_matrix(gpg_ctx* ctx, const gpg_hp* hp, int which, double* out);

/* Kernel table of the reference (Kernel.py:27-126): calc_KernBase / calc_KernGrad as functions of the difference
 * tensor, exactly as the reference's bound attributes take it -- replaces sq_exp_calc_KernBase / _KernGrad
 * (KernelSqExp.py:16-46, 320-410), matern_5f2_calc_KernBase / _KernGrad (KernelMatern5f2.py:16-52, 352-450),
 * rat_quad_calc_KernBase / _KernGrad (KernelRatQuad.py:439-554).  rtensor [dim, n1, n2] row-major with
 * R[k, a, b] = X1[a, k] - X2[b, k] (CommonFun.py:56-84); two DIFFERENT point sets are fine.  use_grad = 0: out
 * [n1, n2] = KernBase.  use_grad != 0: out [n1 + n1g dim, n2 + n2g dim] row-major = KernGrad in the derivative-major
 * block layout, where use_grad1 [n1] / use_grad2 [n2] (NULL = all) are bvec_use_grad1 / 2 and n1g, n2g their counts.
 * No context: a self-contained call on `device` (uploads the tensor, downloads the matrix); errors through
 * gpg_last_error(NULL). */
int gpg_kern_rtensor(int device, int kernel, int dim, int n1, int n2, const double* rtensor, const double* theta,
                     double hp_kernel, int use_grad, const unsigned char* use_grad1, const unsigned char* use_grad2,
                     double* out);

/* Products with the matrix that was factorised last (gpg_lkd / gpg_setup_eval), through its factor in HBM:
 * op 0: out = (L L^T) v, op 1: out = (L L^T)^-1 v; v, out host [N].  L L^T is Kcov_precon = varK (Kcor + eta I)
 * for 'precon' and Kcov for 'base' -- the matrices whose 2-norm condition number Kernel.py:239-245, 279-285 report.
 * The host side runs a Lanczos iteration on these two operators to get lambda_max and 1 / lambda_min
 * (gpgradpy_amd/cond_number.py; replaces np.linalg.cond of an N x N matrix). */
int gpg_factor_apply(gpg_ctx* ctx, int op, const double* v, double* out);

/* d K / d theta_k [dim, N, N] and, for GPG_KERNEL_RATQU, d K / d alpha [N, N] (either may be NULL) of the kernel matrix of ONE point
 * set with itself from its difference tensor rtensor [dim, n, n] (R[k, a, b] = x[a, k] - x[b, k]); N = n (dim + 1) with use_grad, n
 * without; host arrays, row-major.  Replaces the kernel-table entries calc_KernBase_grad_th / calc_KernGrad_grad_th /
 * calc_Kern*_grad_alpha (Kernel.py:43-48, 69-75, 96-102; KernelSqExp.py:91-123, 470-568, KernelMatern5f2.py:100-135, 532-642,
 * KernelRatQuad.py:133-163, 640-840) for callers that want the tensors themselves (the reference's unit_test/test_grad_Kmat.py,
 * calc_KernGrad_hp / calc_Kcov_grad_hp); the likelihood gradient never forms them (gpg_lkd_grad). */
int gpg_kern_rtensor_grad_hp(int device, int kernel, int dim, int n, const double* rtensor, const double* theta, double hp_kernel,
                             int use_grad, double* out_theta, double* out_alpha);

/* The x-derivative entries of the kernel table, from the difference tensor rtensor [dim, n1, n2] of two point sets (R = X1 - X2):
 * out [dim, n1 dim, n2 (+ n2g dim with use_grad)], out[k][i n1 + a][b] = d2 K(a, b) / d x1_i d x1_k and, in gradient column (j, b),
 * d3 K / d x1_i d x1_k d x2_j; use_grad2 [n2] masks the gradient columns (NULL = all).  Replaces calc_KernBase_hess_x (use_grad = 0) /
 * calc_KernGrad_grad_x (use_grad = 1) (Kernel.py:56-57, 82-83, 109-110; KernelSqExp.py:48-88, 412-468); the posterior Hessian itself
 * (gpg_predict_hess) never forms the tensor. */
int gpg_kern_rtensor_hess_x(int device, int kernel, int dim, int n1, int n2, const double* rtensor, const double* theta, double hp_kernel,
                            int use_grad, const unsigned char* use_grad2, double* out);

/* The reference's matrix-dependent nugget (cond_eta_is_const = False, i.e. wellcond_mtd 'rescale_eta_vary'; Kernel.py:229-236,
 * 269-276): rowsum[i] = sum_j |M_ij| over the N rows of M = Kcor = P^-1 (K + diag(noise / varK)) P^-1 (wellcond PRECON) or of the
 * kernel matrix K itself (BASE), host [N]; hp->eta is ignored.  The caller takes argmax / max and sets
 * eta = rowsum[argmax] / (cond_max_target - 1) in the gpg_hp of the evaluation that follows. */
int gpg_abs_rowsum(gpg_ctx* ctx, const gpg_hp* hp, double* rowsum);

/* alpha = Kcov^-1 (y - V beta), host [N], of the most recent successful gpg_lkd_grad on this context (no likelihood call in between):
 * with gpg_factor_apply and gpg_dcov_quadform it gives the remaining outputs of the reference's gradient code without the
 * [n_hp, N, N] tensors -- hp_beta_grad_k = -u' G_k alpha with u = Kcov^-1 V / (V' Kcov^-1 V) (GpMeanFun.py:114-117, as the polarisation
 * (q_k(u + alpha) - q_k(u - alpha)) / 4 of the quadratic form), hp_varK_grad_k = -alpha' G_k alpha / N (CalcLkd.py:112-113; V' alpha = 0),
 * ln_det_Kmat_grad_k = tr(Kcov^-1 G_k) = -2 g_inv[k] (CalcLkd.py:361-365). */
int gpg_lkd_alpha(gpg_ctx* ctx, double* alpha);

/* eta >= 0: the derivatives d Kcov / d hp_k (gpg_lkd_grad, gpg_lkd_grad_batch, gpg_dcov_quadform, gpg_cond_fro) are formed with
 * this nugget instead of gpg_hp.eta -- the reference differentiates with self._etaK even when the matrix was built with the
 * row-sum nugget above (GpHparaGrad.py:43,107,126).  eta < 0 (default): use gpg_hp.eta. */
int gpg_set_gradient_nugget(gpg_ctx* ctx, double eta);

/* out[k] = v^T (d Kcov / d hp_k) v for the dim + 4 hyperparameter slots of gpg_lkd_grad (theta, varK, var_fval,
 * var_fgrad, hp_kernel), v host [N]; call after a successful gpg_lkd / gpg_setup_eval with the same hp (it uses that
 * call's preconditioner vector).  With the extreme eigenvectors of the host-side Lanczos runs this gives the
 * gradient of the condition number, d cond / d hp_k = (q_k(v_max) - cond q_k(v_min)) / lambda_min
 * (GpHparaCon.py:163-207), without the [n_hp, N, N] derivative tensor or a dense eigendecomposition. */
int gpg_dcov_quadform(gpg_ctx* ctx, const gpg_hp* hp, const double* v, double* out);

/* Frobenius-norm condition number of the matrix that is factorised for hp -- cond_norm = 'fro' of the reference:
 * np.linalg.cond(Kcov_precon | Kcov, 'fro') = ||K||_F ||K^-1||_F (Kernel.py:239-245, 279-285; calc_cond_fronorm_w_grad,
 * GpHparaCon.py:209-236) -- and, when cond_grad != NULL (dim + 4 slots as gpg_lkd_grad; wellcond 'base' only, as in the
 * reference), its gradient sum_{r,c} (frac K - K^-3 / frac)[r,c] (d K / d hp_k)[r,c], frac = ||K^-1||_F / ||K||_F.
 * Everything stays on the device: the norms are reductions over the assembled matrix and over the explicit inverse of
 * the adjoint-gradient path, K^-2 and K^-3 are two full MFMA products, the contraction recomputes d K / d hp_k on the fly.
 * Returns > 0 (first non-positive pivot) when the Cholesky fails. */
int gpg_cond_fro(gpg_ctx* ctx, const gpg_hp* hp, double* cond, double* cond_grad);

/* Instrumentation (replaces the wall-clock accumulator _time_chofac, Kernel.py:247,304-305) ------- */

enum {
  GPG_PROF_ASSEMBLY = 0,   /* fused kernel build: algorithmic bytes 8 N (N+1) / 2                   */
  GPG_PROF_POTRF = 1,      /* diagonal-block factorisations                                         */
  GPG_PROF_TRSM = 2,       /* panel triangular solves                                               */
  GPG_PROF_GEMM_PANEL = 3, /* kept for the layout of the arrays below (GPG_PROF_NCAT): always reads zero,
                            * the panel solve is one fused launch counted under GPG_PROF_TRSM          */
  GPG_PROF_GEMM_TRAIL = 4, /* fp64 MFMA factorisation kernel (dataflow Cholesky launch, or the trailing
                            * update of the blocked schedule): algorithmic flops                      */
  GPG_PROF_REDUCE = 5,     /* log-det / GLS reductions                                              */
  GPG_PROF_NCAT = 6
};
/* mask: bit c enables HIP-event timing of category c launches on the context's stream. */
int gpg_prof_enable(gpg_ctx* ctx, unsigned mask);
/* Synchronises, then returns per category: ms[c] summed event time, count[c] launches,
 * work[c] algorithmic units (bytes for ASSEMBLY, flops otherwise) since the last call; resets. */
int gpg_prof_read(gpg_ctx* ctx, double ms[GPG_PROF_NCAT], long long count[GPG_PROF_NCAT],
                  double work[GPG_PROF_NCAT]);

/* Tuning knobs (defaults are the measured best): panel width (multiple of 128 in [128, 1024]). */
int gpg_set_panel(gpg_ctx* ctx, int nb_outer);
/* bit 0 = 1 (default): look-ahead Cholesky (the next diagonal block is factorised on a second,
 * high-priority stream under the trailing update); 0: single stream.  Only bit 0 is read: bits 1 and 2
 * selected kernel variants that no longer exist and are accepted and ignored. */
int gpg_set_lookahead(gpg_ctx* ctx, int on);

/* Factorisation schedule.  GPG_FACTOR_AUTO (default): one dataflow launch -- the 64 x 64-tile kernel up to
 * 12288 padded columns, the 128 x 128-tile kernel above (batched launches of gpg_lkd_batch switch to the 128-tile
 * kernel much earlier, see gpg_set_batch).  GPG_FACTOR_BLOCKED: right-looking blocked
 * algorithm (panel solve + trailing update per panel, look-ahead on a second stream; the fallback after a
 * timed-out dataflow launch and the reference point for the parity tests).  GPG_FACTOR_TILE64 / GPG_FACTOR_TILE128 force one kernel. */
enum gpg_factor_mode { GPG_FACTOR_AUTO = 0, GPG_FACTOR_BLOCKED = 1, GPG_FACTOR_TILE64 = 2, GPG_FACTOR_TILE128 = 3 };
int gpg_set_factor_mode(gpg_ctx* ctx, int mode);
/* Two dataflow launches sharing one device (two processes / contexts on the same GPU) can starve each other: every
 * wait inside the launch is bounded (0.25 s), the launch then drains, and the library repeats the call with the
 * blocked schedule and keeps the context on it until gpg_set_factor_mode is called again.  Returns how often that
 * happened (results are unaffected; rc -4 is only returned if the blocked repeat fails too). */
int gpg_factor_fallbacks(gpg_ctx* ctx);
/* The same bounded waits guard the overlapped inverse of gpg_lkd_grad / gpg_lkd_grad_batch (W = L^-T launched behind the
 * factorisation it waits for) and the dataflow triangular solves.  A timeout there does NOT cost the dataflow factorisation:
 * the call is repeated once without the overlap (the context stops overlapping), respectively with the blocked solve sweeps
 * (the context keeps them for its solves), until gpg_set_factor_mode re-arms both.  These return how often each happened. */
int gpg_overlap_fallbacks(gpg_ctx* ctx);
int gpg_solve_fallbacks(gpg_ctx* ctx);
/* Schedule of the most recent factorisation launch (for logs / bench): *kernel = 0 blocked, 1 dataflow with 64 x 64
 * tiles, 2 dataflow with 128 x 128 tiles, 3 dataflow with pairs of 128 x 128 tiles per workgroup (batched launches of large
 * matrices); *matrices = how many matrices that launch factorised.  Either may be NULL. */
int gpg_last_factor(gpg_ctx* ctx, int* kernel, int* matrices);
/* Batched launches of the 128 x 128-tile schedule (gpg_lkd_batch on large matrices) can give every 512-thread workgroup a PAIR of tiles of
 * one tile column: both tiles then share the row panel they read as the second operand (a quarter less memory traffic), at the
 * price of finalisations that are not hidden behind another workgroup's MFMA loop; measured 1-3 % faster for every batched size.
 * mode 0: never, 1: always (also for one matrix per launch, where it is 1-2 % slower), 2 (default): whenever a launch holds at
 * least two matrices.  Results are bit-identical in all three modes. */
int gpg_set_pair_mode(gpg_ctx* ctx, int mode);

/* Caps the number of persistent workgroups of every dataflow launch (0 = default: as many as the device holds at once).  The
 * launches are correct for ANY number >= 1 -- a workgroup only ever waits for tasks with smaller tickets, all of which are held
 * by running workgroups or finished -- which is what tests/test_gpu_smoke.py checks with 1, 3 and 17 workgroups; also a way to
 * leave part of the device to another tenant. */
int gpg_set_max_workgroups(gpg_ctx* ctx, int n);

/* Diagnostic switches of the dataflow factorisation (tests/test_gpu_factor.py reaches every schedule at small sizes with them).  With
 * the tile size and the fuse setting fixed the factor is the same bits under either task order.
 * gpg_set_fuse_max_tiles: a single matrix on 64 x 64 tiles lets each diagonal task also compute the sub-diagonal tile below the previous
 * diagonal tile ("fused") while the matrix has at most n 64-column tile columns; n >= 0, 0 = never fuse, default 48 (-1 if n < 0).
 * gpg_set_task_order: ticket order of the factorisation's tasks -- 0 tile column by tile column, 1 critical path first (the next diagonal
 * tile ahead of the rest of its column), -1 (default) the measured choice: 1 for batched launches and below 16384 padded columns, 0
 * above; any other value returns -1 with an error text. */
int gpg_set_fuse_max_tiles(gpg_ctx* ctx, int n);
int gpg_set_task_order(gpg_ctx* ctx, int order);

/* gpg_lkd_batch: up to max_matrices restart rows are assembled into separate workspaces and factorised by ONE
 * dataflow launch (task lists interleaved tile column by tile column).  A single small factorisation is
 * latency-bound and leaves most of the chip idle; a large one does so at its two ends.  Results are bit-identical to
 * the one-at-a-time path.  -1 (default): automatic (8 .. 64 rows, fewer the larger the matrix, 8 from ~18000 padded
 * columns up to 32768, 1 above, where 2 .. 3 can be asked for explicitly); 0 / 1: off.  With enough rows per launch (rows x Npad / 128 >= 320, Npad >= 2048)
 * the 128 x 128-tile kernel is used whatever the single-matrix choice of GPG_FACTOR_AUTO would be. */
int gpg_set_batch(gpg_ctx* ctx, int max_matrices);
/* Allocates the batch workspaces a gpg_lkd_batch call with `rows` rows will use (otherwise done by the first such
 * call): setup, like gpg_set_data, for callers that time gpg_lkd_batch. */
int gpg_reserve_batch(gpg_ctx* ctx, int rows);

/* Library / device facts for logs: writes "gfx950 MI355X ..." style text. */
int gpg_device_info(int device, char* buf, int buflen);

#ifdef __cplusplus
}
#endif
#endif /* GPGRAD_H */
