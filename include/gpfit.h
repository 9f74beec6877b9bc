/*
 * libgpfit — MI355X (gfx950) fp64 Gaussian-process fit/predict kernels behind a C ABI.
 *
 * Drop-in boundary for timghill/GladsGP's GP hot path.  The reference is pure Python: its GP
 * arithmetic lives in the un-vendored SEPIA fork (requirements-cc.txt:55) and GPmodule
 * (requirements-cc.txt:20), called from src/model.py and the analysis drivers.  There is no FFI
 * in the reference, so each entry point below names the reference call it replaces; the
 * Python-side binding is gladsgp_amd/_capi.py (ctypes) and is shown in INTEGRATION.md.
 *
 * Conventions (all entry points):
 *  - every pointer is caller-owned DEVICE memory.  The library allocates nothing persistent:
 *    workspaces are sized by the *_ws_bytes() functions and passed in (256-byte aligned); the
 *    only library-owned objects are the streams/events of an explicit gp_ctx (gp_ctx_create /
 *    gp_ctx_destroy).  The two convenience forms gp_potrf_inv and gp_potrf take no workspace
 *    and use stream-ordered scratch of gp_potrf_inv_ws_bytes / gp_potrf_ws_bytes bytes instead
 *    (hipMallocAsync / hipFreeAsync inside the call, freed on every path); their _ws forms and
 *    every other entry point allocate nothing;
 *  - matrices are column-major with a leading dimension (LAPACK layout), element (i,j) at
 *    A[i + j*ld]; design matrices X (n x d) are row-major with row stride ldx >= d;
 *  - beta holds ARD precisions, beta >= 0 (the kernels take sqrt(beta); a negative entry
 *    yields NaN, which the factorisation reports through info);
 *  - accuracy of a kernel value k = s exp(-sum_k beta_k (a_k - b_k)^2) (gp_gram_ardse,
 *    gp_cross_ardse, the prediction's cross-covariance).  The coordinates are scaled by
 *    q_k = sqrt(beta_k) before they are subtracted, so the rounding of q_k a_k and q_k b_k enters
 *    with the size of the coordinates, not of their difference.  With t_k = q_k (a_k - b_k),
 *    acc = sum_k t_k^2 and eps = 2^-52, relative to the exact value
 *      |dk| / k <= eps ( sum_k |t_k| q_k (|a_k| + |b_k|) + (2 + d/2) acc + 2 ),
 *    plus 2^-1074 absolute where k is below the normal range.  That last figure holds for
 *    2^-1021 <= |s| < 2^1023: the scale is applied before the result is rounded into the
 *    subnormal range, which needs 1.42 s finite and 0.70 s normal; with a smaller s such a
 *    result is rounded twice, a larger s overflows.  On the unit cube with beta <= 5 the bound
 *    is a few eps; it grows like sqrt(beta) |x| sqrt(acc), e.g. 2e-11 at |x| = 64, beta = 800,
 *    acc = 700.  A value whose exact size is below 2^-1075 is +0; acc is clamped at 1100.
 *    tests/test_gpu_extremes.py holds the three kernels to twice this bound over acc = 0 ... 1200;
 *  - accuracy of the factorisation and what is built on it.  No entry point back-substitutes:
 *    the factorisation inverts every diagonal block and multiplies (L_ik = A_ik D_k^T with
 *    D_k = L_kk^-1, on 64 x 64 blocks and, in the persistent kernel, on 16 x 16 blocks inside
 *    them), and z, alpha, the predictive mean and variance are products with the explicit L^-1.
 *    A product with a computed inverse is not backward stable: its error is that of a
 *    substitution times cond(L_kk).  Where the diagonal blocks are well conditioned -- every
 *    regime of the sampler on a scattered design -- the results are within a small multiple of
 *    what LAPACK's potrf / trsm give (measured: at most 7x their spread over orderings).  On
 *    blocks that are themselves near-singular (a smooth kernel on a fine 1-D grid with a jitter
 *    of 1e-7: cond(A) = 5e8, cond(L_kk) ~ 1e4) L, L^-1, z, alpha, mean and var are 30 ... 600
 *    times further from the exact values than LAPACK's, e.g. mean to 4e-11 instead of 1e-13 of
 *    its scale; info stays 0 and the results stay finite.  DESIGN.md §7 has the measured table;
 *    tests/_mp_ref.py (explicit_inverse_term) restates the arithmetic and derives the term.
 *    gp_predict_cov inherits this through V = L^-1 K*: on scattered designs C is within its own
 *    fp64 noise of the exact value (a few eps s_pred, also where test points coincide with
 *    training points or each other), on that grid from n = 64 on 20 ... 320 times the noise, at
 *    most 2e-12 s (tests/_mp_joint_ref.py, FINDINGS_COV);
 *  - `batch` independent problems share X / Xs; per-problem operands advance by the given
 *    stride (matrices), by ldbeta (beta rows), by 1 (s, delta, s_pred, info, logdet) and by
 *    ldw / ldo (w_hat, mean, var columns);
 *  - layout contract: an operand may be a sub-view of a larger array.  Any naturally aligned
 *    base (8 bytes for doubles, 4 for a float32 operand or output) and any leading dimension /
 *    row stride / batch stride at or above the stated minimum are accepted, odd values included;
 *    only the elements the function's comment names are read or written (never the rows between
 *    the logical extent and ld, nor the gap between two problems), and the results do not depend
 *    on the layout bit for bit: alignment only selects wider loads and stores where it allows
 *    them ("Operand layouts and the branches they select").  The exceptions, each
 *    reported by its argument number before anything is launched:
 *      - the L^-1 the prediction READS (gp_predict, gp_predict_ex, gp_predict_z,
 *        gp_predict_solve, gp_predict_cov, gp_fit_predict's Linv) and both buffers of gp_pack_linv /
 *        gp_unpack_linv: 16-byte aligned base, even ldinv, even strideInv (gp_potrf_inv,
 *        gp_trtri, gp_trmv, gp_nll, gp_xval, gp_alpha and gp_nll_grad take any L^-1 layout);
 *      - every workspace `ws`: 256-byte aligned (gp_dgemm / gp_gemm_ex's split-K scratch and
 *        the `work` vectors of gp_nll / gp_mean_var: 8 bytes);
 *  - stream-ordered and asynchronous on `stream`; no host synchronisation, so calls can be
 *    captured into a hipGraph;
 *  - return 0 on success, -k when argument k is invalid (LAPACK style), or
 *    GPFIT_ERR_HIP - hipError_t for a launch failure.  A non-positive-definite pivot is not an
 *    error return: it is reported per problem in info[b] (LAPACK potrf semantics); info[b] = -1
 *    reports an internal error of the factorisation (a bounded wait of the persistent kernel
 *    gave up), never a pivot: the problem's outputs are then unspecified.
 */
#ifndef GPFIT_H
#define GPFIT_H

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPFIT_ERR_HIP (-1000)
#define GPFIT_ERR_RCCL (-3000)  /* gp_comm_*: GPFIT_ERR_RCCL - ncclResult_t; RCCL not loadable */
#define GPFIT_ERR_INTERNAL (-2000)  /* a factorisation reported info = -1 (gp_loglik_status) */
#define GPFIT_MAX_DIM 32      /* largest input dimension d supported by the kernels      */
#define GPFIT_TILE 128        /* row padding of the L^-1 buffer (predict MFMA tile edge) */

/* Library version (major*10000 + minor*100 + patch). */
int gp_version(void);

/* Rows/columns of the L^-1 buffer gp_potrf_inv fills: n rounded up to GPFIT_TILE. */
int gp_padded_n(int n);

/*
 * ARD squared-exponential Gram with jitter, per problem b:
 *   G_b[i + j*ldg] = s[b] * exp(-sum_k beta_b[k] (X[i,k] - X[j,k])^2) + delta[b] * (i == j)
 * Replaces SEPIA SepiaDistCov.compute_cov_mat(beta, lamz, lams) (s = 1/lamUz,
 * delta = 1/lamWs + 1/(lamWOs*LamSim)) as used by SepiaModel.logLik and
 * SepiaEmulatorPrediction (src/model.py:106, analysis/time_predictions.py:76), the explicit
 * Gram of examples/01_Gaussian_random_fields.ipynb:135-141 and GPmodule's
 * squared_exponential (examples/02_univariate_GP_regression.ipynb:80).
 */
int gp_gram_ardse(const double* X, int n, int d, int ldx,
                  const double* beta, int ldbeta, const double* s, const double* delta,
                  double* G, int ldg, long long strideG, int batch, hipStream_t stream);

/*
 * Cross-covariance, transposed so each test point's column is contiguous:
 *   Kt_b[i + j*ldk] = s[b] * exp(-sum_k beta_b[k] (X[i,k] - Xs[j,k])^2),  i < n, j < m.
 * Replaces the Kvec / SigWWb cross-covariance of SepiaEmulatorPrediction and
 * examples/02...ipynb:226.
 */
int gp_cross_ardse(const double* X, int n, int ldx, const double* Xs, int m, int ldxs, int d,
                   const double* beta, int ldbeta, const double* s,
                   double* Kt, int ldk, long long strideK, int batch, hipStream_t stream);

/*
 * Blocked Cholesky with simultaneous triangular inverse, per problem b:
 *   A_b = L_b L_b^T (L_b overwrites the lower triangle of A_b; the strict upper triangle is
 *   left untouched, as LAPACK dpotrf('L')), Linv_b = L_b^-1 (lower; the upper triangle and the
 *   padding rows/cols n..gp_padded_n(n)-1 are zeroed), logdet[b] = log|A_b| = 2 sum log L_ii,
 *   info[b] = 0, or j (1-based) when the leading minor of order j is not positive definite
 *   (then L_b / Linv_b / logdet[b] are unspecified), or -1 for an internal error (above).
 * Linv_b needs ldinv >= gp_padded_n(n) and gp_padded_n(n) columns.  info / logdet may be NULL.
 * Replaces the dense SPD factorisation / solve inside SEPIA's likelihood and prediction
 * (LAPACK potrf/gesv), scipy.linalg.cholesky in examples/01...ipynb:66,144 and GPmodule's
 * K_inv (examples/02...ipynb:232).
 * gp_potrf_inv_ws is the same with caller-owned scratch `ws` of gp_potrf_inv_ws_bytes(n, batch)
 * bytes (the persistent factorisation's task list and flags; 0 bytes when n is beyond its
 * range); gp_potrf_inv allocates that scratch stream-ordered itself.
 */
long long gp_potrf_inv_ws_bytes(int n, int batch);
int gp_potrf_inv_ws(double* A, int n, int lda, long long strideA,
                    double* Linv, int ldinv, long long strideInv,
                    int batch, int* info, double* logdet, void* ws, long long ws_bytes,
                    hipStream_t stream);
int gp_potrf_inv(double* A, int n, int lda, long long strideA,
                 double* Linv, int ldinv, long long strideInv,
                 int batch, int* info, double* logdet, hipStream_t stream);

/*
 * Plain blocked Cholesky, LAPACK dpotrf('L') per problem: A_b = L_b L_b^T with L_b in the lower
 * triangle of A_b (strict upper triangle untouched), logdet[b] = log|A_b|, info[b] = 0 or the
 * 1-based order of the first non-positive-definite leading minor.  Same sweep and arithmetic as
 * gp_potrf_inv without the inverse (L is bit-identical to gp_potrf_inv's).  info / logdet may
 * be NULL.  Replaces the factorisation SURVEY §8b names gp_potrf (LAPACK potrf inside SEPIA's
 * likelihood, scipy.linalg.cholesky in examples/01...ipynb:66,144).  gp_potrf_ws takes the
 * scratch (the D_k = L_kk^-1 blocks and the persistent kernel's task list / flags) from the
 * caller: gp_potrf_ws_bytes(n, batch) bytes.
 */
long long gp_potrf_ws_bytes(int n, int batch);
int gp_potrf_ws(double* A, int n, int lda, long long strideA, int batch, int* info,
                double* logdet, void* ws, long long ws_bytes, hipStream_t stream);
int gp_potrf(double* A, int n, int lda, long long strideA, int batch, int* info,
             double* logdet, hipStream_t stream);

/*
 * Triangular inverse of a lower Cholesky factor, LAPACK dtrtri('L','N') into a padded buffer:
 * Linv_b = L_b^-1 (lower; upper triangle and padding to gp_padded_n(n) zeroed), so a caller
 * that already holds a LAPACK factor can call gp_predict without re-factorising.  info[b] =
 * 0, or the 1-based index of the first zero (or non-finite) diagonal entry (then Linv_b is
 * unspecified).  info may be NULL.
 */
int gp_trtri(const double* L, int n, int ldl, long long strideL, double* Linv, int ldinv,
             long long strideInv, int batch, int* info, hipStream_t stream);

/* Bytes of device workspace gp_predict needs for (n, m, batch) with test-point chunk m_chunk
 * (0 = library default).  Workspace contents are scratch (no state between calls).         */
long long gp_predict_ws_bytes(int n, int m, int batch, int m_chunk);

/*
 * Posterior mean and marginal variance of `batch` GPs at m test points:
 *   z_b = Linv_b w_b,  V = Linv_b Kt_b (never stored),
 *   mean_b[j] = sum_i V[i,j] z_b[i]          = k*_j^T A_b^-1 w_b
 *   var_b[j]  = s_pred[b] - sum_i V[i,j]^2   = s_pred[b] - k*_j^T A_b^-1 k*_j
 * with w_b = w_hat + b*ldw (n values), mean_b = mean + b*ldo, var_b = var + b*ldo (m values).
 * Linv comes from gp_potrf_inv with the same X, beta, s.  Replaces SepiaEmulatorPrediction's
 * predictive mean / covariance diagonal (analysis/time_predictions.py:76-78,
 * assess_all_models.py:489, sensitivity_indices.py:85) and examples/02...ipynb:232-233.
 */
int gp_predict(const double* Linv, int ldinv, long long strideInv,
               const double* X, int ldx, const double* Xs, int ldxs, int n, int m, int d,
               const double* beta, int ldbeta, const double* s, const double* s_pred,
               const double* w_hat, int ldw, double* mean, double* var, int ldo,
               int batch, void* ws, long long ws_bytes, int m_chunk, hipStream_t stream);

/*
 * gp_predict with the L^-1 layout and z = L^-1 w as options (the sharded single-GP path,
 * ranks >= 1 predict straight from the broadcast payload, no unpack and no trmv):
 *   layout GPFIT_LINV_PADDED: Linv as gp_predict (column k at Linv + k*ldinv);
 *   layout GPFIT_LINV_PACKED: Linv tile-packed (gp_pack_linv), ldinv ignored, strideInv >=
 *          gp_linv_packed_elems(n) between problems;
 *   z != NULL: z_b = z + b*ldz (gp_padded_n(n) values, from gp_predict_z) is used as L^-1 w and
 *          w_hat is not read; z == NULL: computed as gp_predict does.
 * Results are bit-identical to gp_predict's for every layout and z option.  Argument numbers
 * 1-23 as gp_predict; -24 layout, -26 ldz.  Workspace: gp_predict_ws_bytes.
 */
#define GPFIT_LINV_PADDED 0
#define GPFIT_LINV_PACKED 1
int gp_predict_ex(const double* Linv, int ldinv, long long strideInv,
                  const double* X, int ldx, const double* Xs, int ldxs, int n, int m, int d,
                  const double* beta, int ldbeta, const double* s, const double* s_pred,
                  const double* w_hat, int ldw, double* mean, double* var, int ldo,
                  int batch, void* ws, long long ws_bytes, int m_chunk, int layout,
                  const double* z, long long ldz, hipStream_t stream);

/*
 * z_b = Linv_b w_b (gp_padded_n(n) rows, zero past n) with exactly the arithmetic gp_predict
 * applies internally, into z + b*ldz: what rank 0 ships with L^-1 so the other ranks skip it.
 * `ws` holds gp_predict_z_ws_bytes(n, batch) bytes.  layout as gp_predict_ex.
 */
long long gp_predict_z_ws_bytes(int n, int batch);
int gp_predict_z(const double* Linv, int ldinv, long long strideInv, int layout, int n,
                 const double* w_hat, int ldw, double* z, long long ldz, int batch, void* ws,
                 long long ws_bytes, hipStream_t stream);

/*
 * The tile-packed L^-1: column c of the padded buffer from row 16*floor(c/16) on (every stored
 * run starts on a 16-row tile and is a multiple of 16 doubles, so the prediction's 16-B loads
 * and 16-row MFMA tiles read it in place), columns one after another:
 * gp_linv_packed_elems(n) = npad^2 - 128 q (q - 1) doubles, q = npad / 16, npad =
 * gp_padded_n(n) -- about half the padded square (67 MB at n = 4096).  Both buffers 16-B
 * aligned; gp_unpack_linv writes only the stored elements.
 */
long long gp_linv_packed_elems(int n);
int gp_pack_linv(const double* Linv, int n, int ldinv, double* P, hipStream_t stream);
int gp_unpack_linv(const double* P, int n, double* Linv, int ldinv, hipStream_t stream);

/*
 * gp_predict from the Cholesky factor L itself (the §8b form, LAPACK layout, lower): L^-1 by
 * gp_trtri into the head of `ws`, then gp_predict.  `ws` holds
 * gp_predict_chol_ws_bytes(n, m, batch, m_chunk) bytes; info as gp_trtri (mean / var of a
 * problem with info[b] != 0 are unspecified).
 */
long long gp_predict_chol_ws_bytes(int n, int m, int batch, int m_chunk);
int gp_predict_chol(const double* L, int ldl, long long strideL,
                    const double* X, int ldx, const double* Xs, int ldxs, int n, int m, int d,
                    const double* beta, int ldbeta, const double* s, const double* s_pred,
                    const double* w_hat, int ldw, double* mean, double* var, int ldo,
                    int batch, int* info, void* ws, long long ws_bytes, int m_chunk,
                    hipStream_t stream);

/*
 * Two-phase form of gp_predict.  The cross-covariance of every test-point chunk does not depend
 * on the factorisation, so it can be built on a second stream while gp_potrf_inv runs:
 *   gp_predict_cross : Kt chunks for all m points into ws (X, Xs, beta, s only)
 *   gp_predict_solve : z = Linv w, TRMM + mean/var per chunk from the prepared ws
 * Both take the same (n, m, batch, m_chunk) and a workspace of
 * gp_predict_prepared_ws_bytes(n, m, batch, m_chunk) bytes; results equal gp_predict's.
 */
long long gp_predict_prepared_ws_bytes(int n, int m, int batch, int m_chunk);
int gp_predict_cross(const double* X, int ldx, const double* Xs, int ldxs, int n, int m, int d,
                     const double* beta, int ldbeta, const double* s, int batch,
                     void* ws, long long ws_bytes, int m_chunk, hipStream_t stream);
int gp_predict_solve(const double* Linv, int ldinv, long long strideInv, int n, int m,
                     const double* s_pred, const double* w_hat, int ldw, double* mean,
                     double* var, int ldo, int batch, void* ws, long long ws_bytes,
                     int m_chunk, hipStream_t stream);

/*
 * z_b = Linv_b w_b (lower-triangular gemv, n rows), z_b = z + b*ldz.
 * Building block of the likelihood (quadratic form w^T A^-1 w = ||z||^2).
 */
int gp_trmv(const double* Linv, int ldinv, long long strideInv, int n,
            const double* w, int ldw, double* z, int ldz, int batch, hipStream_t stream);

/*
 * GP negative log-likelihood per problem:  nll[b] = 1/2 ||Linv_b w_b||^2 + 1/2 logdet[b]
 * (no 2*pi term), with Linv / logdet from gp_potrf_inv; `work` holds batch*n doubles.
 * Replaces GPmodule's MLE objective (examples/02_univariate_GP_regression.ipynb:80-83, known
 * answer fun = -3.989954265337257 at :70-72) and the per-PC Gaussian term of SEPIA's logLik
 * evaluated by SepiaModel.do_mcmc (src/model.py:234-235).
 */
int gp_nll(const double* Linv, int ldinv, long long strideInv, int n,
           const double* w, int ldw, const double* logdet, double* nll, double* work,
           int batch, hipStream_t stream);

/*
 * Execution context of gp_fit_predict, created and destroyed by the caller on the current
 * device: one stream for the cross-covariance (the factorisation and the prediction run on the
 * caller's stream) and its events (one per test-point chunk after its cross-covariance,
 * created on the first call that needs them).
 *   cross_start  : fraction of the factorisation's n/64 block steps after which the
 *                  cross-covariance starts (< 0: default 0.4; 0 = at once);
 *   aux_free_cus : CUs the cross-covariance stream leaves to the factorisation (CU mask;
 *                  < 0: default 0 = no mask).
 * gp_ctx_destroy drains the streams and frees them; call it before the HIP runtime is torn
 * down (e.g. before process exit).  A context serves one host thread at a time.
 */
int gp_ctx_create(double cross_start, int aux_free_cus, void** ctx);
int gp_ctx_destroy(void* ctx);
/*
 * How many test-point chunks' cross-covariance gp_fit_predict runs on the context's aux stream
 * (beside the factorisation and the earlier chunks' TRMMs); the remaining chunks' run on the
 * prediction stream just before their TRMM.  -1 (default): all chunks, the C3 schedule; a batch
 * of small GPs (C4) hides one chunk beside its factorisation and keeps the rest out of the
 * TRMMs' way.  Returns 0, -1 (ctx NULL), -2 (nchunks < -1).  Results are bit-identical for
 * every value.
 */
int gp_ctx_set_aux_chunks(void* ctx, int nchunks);

/*
 * Fit + predict in one call:
 *   G = gram(X) (caller buffer, L on return) -> L, L^-1, info, logdet (as gp_potrf_inv) ->
 *   mean / var at the m test points (as gp_predict).
 * With ctx == NULL every step runs in order on `stream`.  With a context the cross-covariance
 * of every chunk forks onto the context's stream, beside the factorisation (CU-masked if
 * asked), while `stream` runs the Gram + factorisation, z = L^-1 w and per chunk, once that
 * chunk's cross-covariance is done, its TRMM, then one mean/var pass: the caller sees one
 * stream-ordered operation.  `ws` holds
 * gp_fit_predict_ws_bytes(n, m, batch, m_chunk) bytes (the factorisation's scratch included).
 * The prediction runs whatever info says: mean / var of a problem with info[b] != 0 are
 * unspecified (check info; -1 is an internal error, see the conventions).
 * Replaces the reference's fit-then-predict sequence per GP (SEPIA likelihood factorisation +
 * SepiaEmulatorPrediction, time_predictions.py:76-79) at the bench configuration.
 */
long long gp_fit_predict_ws_bytes(int n, int m, int batch, int m_chunk);
int gp_fit_predict(const double* X, int ldx, const double* Xs, int ldxs, int n, int m, int d,
                   const double* beta, int ldbeta, const double* s, const double* delta,
                   const double* s_pred, const double* w_hat, int ldw, double* G, int ldg,
                   long long strideG, double* Linv, int ldinv, long long strideInv, int* info,
                   double* logdet, double* mean, double* var, int ldo, int batch, void* ws,
                   long long ws_bytes, int m_chunk, void* ctx, hipStream_t stream);

/*
 * Batched GP log-likelihood in one stream-ordered call: Gram (gp_gram_ardse) -> Cholesky
 * (gp_potrf_inv) -> ll[b] = -(1/2 ||L_b^-1 w_b||^2 + 1/2 log|G_b|), no 2*pi term, with
 * ll[b] = -inf where G_b is not positive definite (info[b] > 0: a proposal the sampler rejects)
 * and ll[b] = NaN where the factorisation gave up (info[b] = -1), which also raises a sticky
 * status word in `ws` (info optionally copied out to `info`).  `ws` is caller-owned device
 * scratch of gp_loglik_ws_bytes(n, batch) bytes, zero-filled before its first use.  Never
 * syncs, so a Metropolis sweep can be stream-ordered (and graph-captured) end to end;
 * gp_loglik_status reads the status word afterwards (it synchronises `stream`): 0, or
 * GPFIT_ERR_INTERNAL when any gp_loglik on this workspace since the last reset had an internal
 * factorisation error; `reset` clears the word.
 * Replaces the per-PC term of SEPIA's logLik evaluated by SepiaModel.do_mcmc /
 * tune_step_sizes (src/model.py:234-235): Sigma_j = s_j R(beta_j) + delta_j I, w = w_hat_j.
 */
long long gp_loglik_ws_bytes(int n, int batch);
int gp_loglik(const double* X, int n, int d, int ldx, const double* beta, int ldbeta,
              const double* s, const double* delta, const double* w, int ldw, int batch,
              void* ws, long long ws_bytes, double* ll, int* info, hipStream_t stream);
int gp_loglik_status(void* ws, int n, int batch, int reset, hipStream_t stream);

/*
 * Metropolis sweep steps around gp_loglik (the GPU sampler's speculative groups; replaces the
 * proposal / accept logic of SEPIA's SepiaModel.do_mcmc / tune_step_sizes that src/model.py:
 * 225-235 drives).  The chain state and its priors are described by a gp_mcmc_state of device
 * pointers (row-major: betaU and step_betaU (d+1) x P; lamUz, lamWs, ll, lam, step_lamUz,
 * step_lamWs P; lamWOs, step_lamWOs 1; acc (d+4) x P acceptance counters indexed by update
 * code; u the sweep's 2 ((d+1) P + 2 P + 1) uniforms, an update's proposal uniforms then its
 * acceptance uniforms, in update order; scratch 3 * GPFIT_MCMC_MAX_GROUP * P doubles) plus the
 * prior family / parameters / bounds and step type of each of betaU, lamUz, lamWs, lamWOs.
 * Update codes: 1..d betaU row, d+1 lamUz, d+2 lamWs, d+3 lamWOs (code c reads u[2 P c ..]: P
 * proposal then P acceptance uniforms; lamWOs one of each).  A code may appear at most once in
 * a group.  A proposal outside [lo, hi] (a BetaRho one also: rho' outside (0, 1]) is rejected:
 * its candidate is the current value.  An update is accepted when log(u_acc) < the difference
 * of its log likelihood + log prior; a NaN difference (ll_all NaN, or -inf against -inf)
 * rejects.  scratch holds three planes of GPFIT_MCMC_MAX_GROUP rows of P (candidates, in-range
 * flags as 0 / 1, prior differences), row i = update i of the group prepared last (lamWOs:
 * element 0 only); prep writes those rows and nothing else of it, decide reads them.  Only the
 * accepted elements of the state and of ll, the counters of the group's codes (and of code 0
 * when first != 0) and, when last != 0, lp are written.  For a group of g updates:
 *   gp_mcmc_group_prep   proposes them (first != 0: also the prior-only move of betaU row 0)
 *                        and writes the Gram inputs of the 2^g - 1 state sets, set
 *                        2^i - 1 + pat = update i proposed after the outcomes `pat` (bit q =
 *                        update q accepted) of updates 0..i-1, rows set * P + j of beta
 *                        (x d), s and delta: the batch for gp_loglik;
 *   gp_mcmc_group_decide takes the decisions in order from gp_loglik's ll_all (per GP; lamWOs
 *                        once on the sum over the GPs in index order, its outcome entering
 *                        every GP's `pat`), updates state, ll and counters in place and
 *                        (last != 0) writes the log posterior to lp: the sum over the GPs of
 *                        ll + that GP's d + 3 log priors, plus lamWOs' log prior;
 *   gp_mcmc_group_step   gp_mcmc_group_decide of one group (S, kinds, g, last, ll_all) then
 *                        gp_mcmc_group_prep of the next (S_next, kinds_next, g_next, first,
 *                        beta, s, delta) in one launch (one kernel boundary less per group);
 *                        the same results as the two calls in turn.  Argument errors of the
 *                        second group are its prep's codes - 10; S_next->P must equal S->P
 *                        (-18).
 * Single-workgroup launches (P <= 1024), stream-ordered, graph-capturable; 0 or < 0 (argument).
 * Each of the three forwards to the gp_mcmc_ens_* call of the same name below with nchains = 1
 * and zeroed strides: one set of kernels serves both families, and the return codes are that
 * call's (-1 .. -7 for prep and decide, and for step also -11 .. -18; the ensemble-only -8, -9
 * and -19 cannot occur with one chain).
 */
#define GPFIT_MCMC_MAX_GROUP 4
#define GPFIT_MCMC_GAMMA 0        /* (a - 1) log x - b x                                      */
#define GPFIT_MCMC_BETA 1         /* Beta(a, b) on rho = min(exp(-x / 4), 0.999)              */
#define GPFIT_MCMC_NORMAL 2       /* -1/2 ((x - a) / b)^2                                     */
#define GPFIT_MCMC_UNIFORM 3      /* 0 (the bounds)                                           */
#define GPFIT_MCMC_STEP_UNIFORM 0 /* x' = x + step (u - 1/2)                                  */
#define GPFIT_MCMC_STEP_BETARHO 1 /* the same move on rho = exp(-x / 4)                       */
typedef struct {
  double* betaU;
  double* lamUz;
  double* lamWs;
  double* lamWOs;
  double* ll;
  const double* lam;
  const double* u;
  const double* step_betaU;
  const double* step_lamUz;
  const double* step_lamWs;
  const double* step_lamWOs;
  double* acc;
  double* lp;
  double* scratch;
  int P, d;
  int dist[4];        /* per parameter: betaU, lamUz, lamWs, lamWOs */
  int steptype[4];
  double pa[4], pb[4], lo[4], hi[4];
} gp_mcmc_state;
int gp_mcmc_group_prep(const gp_mcmc_state* S, const int* kinds, int g, int first,
                       double* beta, double* s, double* delta, hipStream_t stream);
int gp_mcmc_group_decide(const gp_mcmc_state* S, const int* kinds, int g, int last,
                         const double* ll_all, hipStream_t stream);
int gp_mcmc_group_step(const gp_mcmc_state* S, const int* kinds, int g, int last,
                       const double* ll_all, const gp_mcmc_state* S_next, const int* kinds_next,
                       int g_next, int first, double* beta, double* s, double* delta,
                       hipStream_t stream);

/*
 * The three steps for an ensemble of `nchains` chains that share X, P, d, the priors, the
 * bounds and the step types (C repeat chains of one model, or C models on one design: equal or
 * different w_hat behind gp_loglik): the kernels behind both families (gp_mcmc_group_* above
 * forwards here with nchains = 1).  S describes chain 0; `strides` holds, for each pointer
 * field of gp_mcmc_state, the distance in doubles from one chain's buffer to the next chain's.
 * Workgroup c runs the step described above on chain c's buffers: a fixed arithmetic order per
 * chain (no FMA contraction, the in-order sums of lamWOs' decision and of lp), no atomics, and
 * it touches no other chain's memory, so a chain's results do not depend on the other chains of
 * the call: chain c's bits are those of a call with nchains = 1 on its buffers alone, whatever
 * the strides of that call hold.
 * The batch is chain-major: chain c's rows of beta / s / delta / ll_all start at row
 * c (2^g - 1) P and are laid out within the chain as above, so any run of whole chains is one
 * contiguous gp_loglik batch (gp_mcmc_ens_step: ll_all with the decided group's g, beta / s /
 * delta with the next group's).
 * Strides: 0 = every chain reads the same buffer, allowed for the buffers the kernels never
 * write (lam, u, step_betaU, step_lamUz, step_lamWs, step_lamWOs; any stride >= 0 is accepted
 * for them).  For a written buffer the stride must be at least its per-chain extent: betaU
 * (d+1) P, lamUz, lamWs, ll P, lamWOs, lp 1, acc (d+4) P, scratch 3 GPFIT_MCMC_MAX_GROUP P.
 * With nchains = 1 the strides are not read (the struct must still be given).
 * gp_mcmc_ens_step applies the one `strides` to S and to S_next.
 * nchains <= GPFIT_MCMC_MAX_CHAINS = 4096.  The launch grid would take far more; the limit
 * keeps the row count of a whole ensemble's batch, nchains (2^GPFIT_MCMC_MAX_GROUP - 1) P <=
 * 4096 * 15 * 1024 < 2^26, well inside gp_loglik's int `batch`, and is already beyond what one
 * device factorises at a time (the caller slices the batch by whole chains).
 * Return codes (argument checks in this order, before any launch):
 *   gp_mcmc_ens_prep / gp_mcmc_ens_decide
 *     -1 S null; -2 P outside 1..1024; -3 d outside 1..GPFIT_MAX_DIM; -4 g outside
 *     1..GPFIT_MCMC_MAX_GROUP or kinds null; -5 a null pointer in S; -6 an update code outside
 *     1..d+3; -7 beta, s or delta null (prep), ll_all null (decide); -8 nchains outside
 *     1..GPFIT_MCMC_MAX_CHAINS; -9 strides null, or (nchains > 1) a negative stride or a written
 *     buffer's stride below its per-chain extent;
 *   gp_mcmc_ens_step
 *     -1 .. -6, -7 (ll_all), -8, -9 for the decided group as above; then the next group's prep
 *     codes - 10: -11 .. -16 for S_next / kinds_next / g_next, -17 beta, s or delta null, -18
 *     S_next->P != S->P, -19 the strides against S_next's extents.
 * 0 on success; GPFIT_ERR_HIP - e for a launch error.
 */
#define GPFIT_MCMC_MAX_CHAINS 4096
typedef struct {
  long long betaU, lamUz, lamWs, lamWOs, ll, lam, u, step_betaU, step_lamUz, step_lamWs,
      step_lamWOs, acc, lp, scratch;
} gp_mcmc_strides;
int gp_mcmc_ens_prep(const gp_mcmc_state* S, const gp_mcmc_strides* strides, int nchains,
                     const int* kinds, int g, int first, double* beta, double* s, double* delta,
                     hipStream_t stream);
int gp_mcmc_ens_decide(const gp_mcmc_state* S, const gp_mcmc_strides* strides, int nchains,
                       const int* kinds, int g, int last, const double* ll_all,
                       hipStream_t stream);
int gp_mcmc_ens_step(const gp_mcmc_state* S, const gp_mcmc_strides* strides, int nchains,
                     const int* kinds, int g, int last, const double* ll_all,
                     const gp_mcmc_state* S_next, const int* kinds_next, int g_next, int first,
                     double* beta, double* s, double* delta, hipStream_t stream);

/*
 * Host-side (no device, no stream): `count` float32 deviates of numpy's legacy global
 * generator exactly as src/svd.py:51 draws randomized_svd's test matrix,
 * np.random.normal(size=...).astype(np.float32) -- MT19937 + the polar Box-Muller method
 * (numpy's legacy_gauss), bit-identical -- continued from and advancing the caller's state:
 * key[624] / pos (np.random.get_state()[1:3]) and the cached deviate has_gauss / gauss
 * ([3:5]).  Twist and candidate tests vectorised, the accepted pairs' log / sqrt on `nthreads`
 * host threads.  Returns 0, -1 (a state pointer NULL), -2 (pos outside [0, 624]), -5 (count < 0),
 * -6 (out NULL), -7 (a host thread or buffer could not be created; the state is then
 * undefined: restore it from a copy).
 */
int gp_host_legacy_normal_f32(unsigned int* key, int* pos, int* has_gauss, double* gauss,
                              long long count, float* out, int nthreads);

/*
 * One marginal realisation per entry: out[i] = mean[i] + sqrt(max(var[i], 0)) z_i, z_i ~ N(0,1)
 * from counter-based Philox4x32-10 keyed by `seed` (counter (i/2, offset); Box-Muller pairs),
 * so the draws depend only on (seed, offset, i).  out may alias mean.  The opt-in realize mode
 * of the prediction: SepiaEmulatorPrediction's .w is a random draw of the PC weights, whose
 * spread the reference's quantile / coverage statistics use (assess_all_models.py:489-500).
 */
int gp_realize(const double* mean, const double* var, long long N, unsigned long long seed,
               unsigned long long offset, double* out, hipStream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fit-side dense kernels (src/model.py init_model and src/svd.py randomized_svd).
 * ---------------------------------------------------------------------------------------- */

/* C = alpha op(A) op(B) + beta C, column-major fp64 on MFMA; op = transpose when trans = 1.
 * Large-K products are split over K into `ws` (gp_dgemm_ws_bytes(m, n, k) bytes; with a smaller
 * or NULL ws the product runs unsplit).  Replaces the numpy GEMMs of src/svd.py:52-64
 * (X Omega, X X^T Y, Q^T X, Q U) and of src/model.py:101, 219-220. */
long long gp_dgemm_ws_bytes(int m, int n, int k);
int gp_dgemm(int transa, int transb, int m, int n, int k, double alpha,
             const double* A, int lda, const double* B, int ldb, double beta,
             double* C, int ldc, void* ws, long long ws_bytes, hipStream_t stream);

/* gp_dgemm with either operand stored as float32 (a_f32 / b_f32 = 1): the float32 elements are
 * widened to fp64 as they are loaded (exactly), the products and sums are fp64, so the result
 * is bit-identical to gp_dgemm on an fp64 copy of the operand -- from half its bytes and
 * without the copy.  src/svd.py:51-64 receives the float32 ensemble of fit_models /
 * load_model (src/model.py:184, 136) and multiplies it as stored; this is that product in fp64.
 * Same workspace rule as gp_dgemm; argument numbers as listed. */
int gp_gemm_ex(int transa, int transb, int m, int n, int k, double alpha,
               const void* A, int a_f32, int lda, const void* B, int b_f32, int ldb,
               double beta, double* C, int ldc, void* ws, long long ws_bytes, hipStream_t stream);

/* Per-location statistics over simulations of a C-order ensemble Y (n x ny, row stride ldy):
 * mu = mean over rows, sd = std(ddof=1) floored at sd_floor — src/model.py:60-64.  n = 1 has no
 * sample deviation (numpy's ddof = 1 gives NaN there): sd is then the floor, mu the row itself. */
int gp_sim_stats(const double* Y, int n, int ny, long long ldy, double sd_floor,
                 double* mu, double* sd, hipStream_t stream);

/* out = (Y - mu) / sd (inverse = 0, src/model.py:72) or out = Y sd + mu (inverse = 1, the
 * back-transform of SepiaEmulatorPrediction.get_y), both C-order n x ny with row strides. */
int gp_standardize(const double* Y, int n, int ny, long long ldy, const double* mu,
                   const double* sd, double* out, long long ldo, int inverse,
                   hipStream_t stream);

/* Field reconstruction, SepiaEmulatorPrediction.get_y() (time_predictions.py:79-90,
 * assess_all_models.py:489-500) in one pass:
 *   Y[r*ldy + c] = ((sum_j W[r*ldw + j] K[j*ldk + c]) + err[r]) * sd[c] + mu[c]
 * for r < rows (samples x test points), c < ncols (field nodes), j < P <= gp_field_max_pcs()
 * PCs; fp64 MFMA products, the back-transform and the optional error term (one scalar per row,
 * err may be NULL) in the epilogue, stored once as float32 (out_f32 = 1, the reference's
 * .w.astype(float32) path) or fp64.  sd and mu NULL together: Y = W K (+ err), the
 * standardised field.  Equal bit for bit to gp_dgemm (K <= 64) + gp_standardize(inverse = 1)
 * + a float32 cast.  Returns -4 for P outside [1, gp_field_max_pcs()]. */
int gp_field_max_pcs(void);
int gp_field(const double* W, long long ldw, int rows, int P, const double* K, long long ldk,
             int ncols, const double* sd, const double* mu, const double* err, void* Y,
             long long ldy, int out_f32, hipStream_t stream);

/* Predictive summary of the reconstructed field over the posterior samples, the reduction every
 * consumer of get_y() applies at once (assess_all_models.py:489-500, 510-521,
 * plot_test_error.py:77-87, include_trunc_error.py:84-90), in one pass that never stores the
 * (S, m, ncols) field.  With a_s = sum_j W[s*lds + i*ldw + j] K[j*ldk + c] (gp_field's MFMA chain,
 * bit for bit), y_s = a_s sd[c] + mu[c] and z_s = (a_s + err[s*m + i]) sd[c] + mu[c] (z_s = y_s
 * when err is NULL; sd and mu NULL together: the standardised field), for i < m, c < ncols:
 *   mean[i*ldo + c] = fp64 mean of y_s over s < S (no error term, as in the reference),
 *   lo / hi[i*ldo + c] = the q_lo / q_hi quantile of z_s over s, numpy's default ("linear") rule:
 *     pos = q (S - 1), j = floor(pos), t = pos - j, z_(j) + (z_(j+1) - z_(j)) t for t < 0.5,
 *     z_(j+1) - (z_(j+1) - z_(j)) (1 - t) otherwise, z_(j) at j = S - 1,
 * each rounded once to float32 (out_f32 = 1) or stored as fp64.  The order statistics are
 * selections kept in registers: the lower tail needs the min(floor(q_lo (S-1)) + 2, S) smallest
 * values, the upper one the S - floor(q_hi (S-1)) largest, each at most
 * gp_field_summary_max_tail() = 8 (q = 0.025 up to S = 128); a deeper request returns the
 * argument number of its q (-13 / -14) with nothing launched, as does q outside [0, 1] and
 * q_lo > q_hi (-14).  -6 for P outside [1, gp_field_max_pcs()], -3 for lds < (m - 1) ldw + P;
 * NaN samples are not ordered (unspecified quantiles).  m = 0 or ncols = 0: no launch. */
int gp_field_summary_max_tail(void);
int gp_field_summary(const double* W, long long ldw, long long lds, int S, int m, int P,
                     const double* K, long long ldk, int ncols, const double* sd,
                     const double* mu, const double* err, double q_lo, double q_hi, void* mean,
                     void* lo, void* hi, long long ldo, int out_f32, hipStream_t stream);

/* Test-error scores of the reconstructed field against a truth, the numbers the assessment drivers
 * reduce the summary to (assess_all_models.py:524-552: RMSE, MAPE, mean quantiles, coverage;
 * plot_integrated_RMSE.py:108-116: per-node RMSE; assess_all_models.py:504-521, 538: the band
 * width where there is no truth), in gp_field_summary's one pass and without its three (m, ncols)
 * arrays.  Arguments 1-14 are gp_field_summary's, with the same limits and the same codes.  Let
 * mu, l, h be what gp_field_summary stores at (i, c) as mean, lo, hi -- with out_f32 = 1 the
 * float32 values, widened again -- and y = Y[i*ldy + c] (float32 when y_f32 = 1, else fp64,
 * widened exactly; ldy >= ncols).  An element is valid when Y is given and y is not NaN (the
 * reference's nanmean).  Every term is formed in fp64 with each operation rounded on its own
 * ((mu - y)^2 is a rounded difference, squared and rounded: numpy's terms bit for bit), then
 *   rows[i*8 + k], summed over c < ncols:                       cols[c*4 + k], summed over i < m:
 *     GPFIT_SCORE_ROW_SQERR   sum (mu - y)^2 over valid           GPFIT_SCORE_COL_SQERR  the same
 *     GPFIT_SCORE_ROW_VALID   number of valid elements            GPFIT_SCORE_COL_VALID  the same
 *     GPFIT_SCORE_ROW_APE     sum |(mu - y) / y| over valid       GPFIT_SCORE_COL_COVERED
 *                             elements with !(y < mape_floor)     GPFIT_SCORE_COL_WIDTH  sum (h - l)
 *     GPFIT_SCORE_ROW_APE_N   the number of those elements
 *     GPFIT_SCORE_ROW_LO / _HI / _MEAN   sum of l / h / mu over all c
 *     GPFIT_SCORE_ROW_COVERED number of valid elements with l <= y <= h (both inclusive)
 * counts as doubles (exact).  mape_floor is the reference's inner_mape[y_test < lq] = nan: -inf
 * counts every valid element, +inf none but y = +inf; a NaN floor compares false like numpy's
 * mask and so counts every valid element too.  Y NULL: no element is valid (the widths and the
 * sums of l, h, mu remain: the integration-point loop).  mean, lo, hi are optional outputs, each
 * NULL or m x ncols with row stride ldo >= ncols in the out_f32 dtype: what gp_field_summary
 * stores there, bit for bit.  cols may be NULL.  ws: gp_field_score_ws_bytes(S, m, P, ncols)
 * bytes, 256-B aligned (8 doubles per (128-column panel, point) and 4 x 128 per (workgroup, panel)
 * segment; -1 for an invalid size, 0 for an empty problem).  A second small kernel on the same
 * stream adds the partials in a fixed order: no floating-point atomics, no hand-off between
 * workgroups, equal inputs give equal bits.  The new arguments are checked after the shared ones,
 * each by its own number: -16 ldy, -17 y_f32, -22 ldo (when an output is given), -23 out_f32,
 * -24 rows, -26 ws (NULL or misaligned), -27 ws_bytes.  m = 0 or ncols = 0: no launch, ws unused. */
#define GPFIT_SCORE_ROW_SQERR 0
#define GPFIT_SCORE_ROW_VALID 1
#define GPFIT_SCORE_ROW_APE 2
#define GPFIT_SCORE_ROW_APE_N 3
#define GPFIT_SCORE_ROW_LO 4
#define GPFIT_SCORE_ROW_HI 5
#define GPFIT_SCORE_ROW_COVERED 6
#define GPFIT_SCORE_ROW_MEAN 7
#define GPFIT_SCORE_COL_SQERR 0
#define GPFIT_SCORE_COL_VALID 1
#define GPFIT_SCORE_COL_COVERED 2
#define GPFIT_SCORE_COL_WIDTH 3
long long gp_field_score_ws_bytes(int S, int m, int P, int ncols);
int gp_field_score(const double* W, long long ldw, long long lds, int S, int m, int P,
                   const double* K, long long ldk, int ncols, const double* sd, const double* mu,
                   const double* err, double q_lo, double q_hi, const void* Y, long long ldy,
                   int y_f32, double mape_floor, void* mean, void* lo, void* hi, long long ldo,
                   int out_f32, double* rows, double* cols, void* ws, long long ws_bytes,
                   hipStream_t stream);

/* Saltelli estimators of the Sobol' sensitivity indices for R replicates of the design rows: the
 * statistic that saltelli_sensitivity_indices / PCA_saltelli_sensitivity_indices evaluate once
 * for the point estimate and then 9,999 times per scipy.stats.bootstrap call, plus N jackknife
 * evaluations for BCa (src/utils.py:27-256, called from sensitivity_indices.py:96,214), here one
 * asynchronous launch per set of replicates.  Operands are output-major: output j at design row k
 * is fA[j*ldf + k], fB[j*ldf + k] and, with input i taken from A, fAB[i*strideAB + j*ldf + k]
 * (ldf >= N, strideAB >= (p-1) ldf + N).  Replicate r uses the M = n_draw rows i_0 .. i_{M-1}:
 *   GPFIT_SOBOL_IDENTITY   i_k = k                         (R = 1, n_draw = N: the point estimate)
 *   GPFIT_SOBOL_INDEX      i_k = idx[r*ldi + k], ldi >= n_draw, clamped into [0, N)
 *   GPFIT_SOBOL_PHILOX     i_k = (x N) >> 32, x = word k & 3 of Philox4x32-10 (gp_realize's) with
 *                          key seed and counter (k >> 2, r, offset_lo, offset_hi)
 *   GPFIT_SOBOL_JACKKNIFE  i_k = k + (k >= r)              (R = N, n_draw = N - 1: leave r out)
 * the same rows for every output and input.  With a_k, b_k, c_k = fA, fB, fAB_i at row i_k:
 *   mu = (sum a + sum b) / (2M),  var = (sum (a-mu)^2 + sum (b-mu)^2) / (2M)   (two-pass),
 *   V = sum a (c - b) / M  (V < 0 -> 0 when clamp != 0, as the reference's bootstrap statistic
 *   does and its point estimate does not),  E = sum (b - c)^2 / (2M),
 *   first[r*ldr + j*d + i] = V / var,  total[r*ldr + j*d + i] = E / var,  ldr >= p d,
 * and, when pcvar is given, the general indices of the whole field
 *   gfirst[r*ldg + i] = sum_j pcvar[j] first[r, j, i] (increasing j), gtotal likewise, ldg >= d;
 * pcvar, gfirst and gtotal are NULL together or not at all.  fp64 throughout, no atomics: equal
 * inputs give equal bits, and so do two modes that select the same rows.  Allocates nothing and
 * can be captured into a hipGraph.  2 <= N <= 2^20, 1 <= d <= GPFIT_MAX_DIM, p >= 1, R >= 0
 * (R = 0: no launch); a violation returns its argument number (a mode's R / n_draw rule: -13 /
 * -12; a NULL pointer: its own number) before any launch.  gp_sobol_lds_points(d): the largest N
 * whose (d + 2) N working set the kernel keeps in LDS (0 for d out of range); above it the same
 * kernel gathers from global memory. */
#define GPFIT_SOBOL_IDENTITY 0
#define GPFIT_SOBOL_INDEX 1
#define GPFIT_SOBOL_PHILOX 2
#define GPFIT_SOBOL_JACKKNIFE 3
int gp_sobol_replicates(
    const double* fA, const double* fB, const double* fAB, long long ldf, long long strideAB,
    int N, int p, int d, int mode, const int* idx, long long ldi, int n_draw, int R,
    unsigned long long seed, unsigned long long offset, const double* pcvar, int clamp,
    double* first, double* total, long long ldr, double* gfirst, double* gtotal, long long ldg,
    hipStream_t stream);
long long gp_sobol_lds_points(int d);

/* Cross-validated predictions of the training simulations (leave-one-out or K-fold) from the
 * L^-1 of gp_potrf_inv, with no refit: what SEPIA's SepiaXvalEmulatorPrediction(leave_out_inds=)
 * (imported by assess_all_models.py:32 and include_trunc_error.py:15) computes by refitting one
 * sub-model per fold.  Per problem b, with A = G + delta I, Q = A^-1 = L^-T L^-1, z = L^-1 w and,
 * for a fold F of f indices, the n x f column panel P_F = L^-1[:, F]:
 *   Q_FF = P_F^T P_F,  alpha_F = P_F^T z,
 *   mean[F] = w[F] - Q_FF^-1 alpha_F     = E[w_F | w outside F],
 *   var[F]  = diag(Q_FF^-1) - shift[b]   (leave-one-out: w_i - alpha_i / Q_ii, 1 / Q_ii - shift).
 * shift = s + delta - s_pred gives the variance gp_predict reports at a new point placed at x_i
 * (s_pred on the diagonal); shift NULL or 0: the variance of the observed w_i.
 *   Linv      the padded L^-1 of gp_potrf_inv (GPFIT_LINV_PADDED), ldinv >= gp_padded_n(n),
 *             strideInv >= ldinv * gp_padded_n(n); any naturally aligned layout (a 16-B aligned
 *             base with even ldinv and strideInv selects 16-B loads).  Column c is taken as
 *             zero above row c and below row n - 1 whatever the buffer holds there.
 *   w_hat     n values at w_hat + b * ldw.
 *   fold_ptr  nfolds + 1 device ints, fold k = fold_idx[fold_ptr[k] .. fold_ptr[k + 1] - 1];
 *   fold_idx  nidx <= n device ints, 0-based, in any order; both shared by all problems.  Both
 *             NULL with nfolds = nidx = 0: leave-one-out over all n.  An index should appear in
 *             one fold at most (otherwise which fold's value is kept is unspecified).
 *   mean, var written at + b * ldo + i for every i in a fold; other elements are not touched.
 *   info      (may be NULL) info[b] = 0, or k + 1 for the first fold k whose Q_FF is not positive
 *             definite (that fold's outputs are NaN, the other folds are produced), or -2 when a
 *             fold holds more than GPFIT_XVAL_MAX_FOLD indices, an index lies outside [0, n) or
 *             fold_ptr is not a non-decreasing sequence within [0, nidx]: such a fold is skipped,
 *             nothing is read or written for it.
 *   ws        gp_xval_ws_bytes(n, nfolds, nidx, batch) bytes, 256-B aligned (z of every problem).
 * Leave-one-out reads the lower triangle once (4 n^2 bytes per problem); a fold reads its panel
 * from row min(F) down (8 (n - min F) f bytes).  Stream-ordered, allocates nothing, can be
 * captured into a hipGraph.  n = 0 or batch = 0: no launch. */
#define GPFIT_XVAL_MAX_FOLD 64
int gp_xval_max_fold(void);
long long gp_xval_ws_bytes(int n, int nfolds, int nidx, int batch);
int gp_xval(const double* Linv, int ldinv, long long strideInv, int n, const double* w_hat,
            int ldw, const int* fold_ptr, const int* fold_idx, int nfolds, int nidx,
            const double* shift, double* mean, double* var, int ldo, int* info, int batch,
            void* ws, long long ws_bytes, hipStream_t stream);

/* alpha_b = A_b^-1 w_b = Linv_b^T (Linv_b w_b) from the L^-1 of gp_potrf_inv: the weights of the
 * posterior mean, mean(x) = sum_n alpha_n k(x, x_n), which gp_mean_response contracts in closed
 * form (the reference never forms them: mean_response.py:126,200 predict point by point).
 *   Linv   the padded L^-1 of gp_potrf_inv under gp_xval's layout rules: ldinv >= gp_padded_n(n),
 *          strideInv >= ldinv * gp_padded_n(n), any naturally aligned layout (a 16-B aligned base
 *          with even ldinv and strideInv selects 16-B loads); column c is taken as zero above
 *          row c and below row n - 1 whatever the buffer holds there.
 *   w      n values at w + b * ldw;  alpha: n values written at alpha + b * lda.
 *   ws     gp_alpha_ws_bytes(n, batch) bytes, 256-B aligned (z = L^-1 w of every problem; -1 for
 *          a negative size).
 * Two launches per 65535 problems: z by the masked triangular gemv, then one wave per column for
 * sum_{k >= i} L^-1[k,i] z_k (fixed order: equal inputs give equal bits).  Stream-ordered,
 * allocates nothing, can be captured into a hipGraph.  n = 0 or batch = 0: no launch.  A
 * violation returns minus its argument position before anything is launched. */
long long gp_alpha_ws_bytes(int n, int batch);
int gp_alpha(const double* Linv, int ldinv, long long strideInv, int n, const double* w, int ldw,
             double* alpha, int lda, int batch, void* ws, long long ws_bytes, hipStream_t stream);

/* Analytic gradient of NLL = 1/2 w^T K^-1 w + 1/2 log|K| (the value gp_nll returns) from the L^-1
 * of gp_potrf_inv: what scipy takes by forward differences of GPmodule's objective in
 * GPmodule.GP.fit (examples/02...ipynb:80-85: d + 1 further factorisations per gradient, each only
 * cond(K) eps accurate).  Per problem b, with K = s R + delta I, R_ij = exp(-sum_k beta_k D_ijk^2),
 * D_ijk = X[i,k] - X[j,k], alpha = K^-1 w and W = K^-1 - alpha alpha^T:
 *   grad_b[0]     = dNLL/ds      =  1/2 sum_ij W_ij R_ij
 *   grad_b[1]     = dNLL/ddelta  =  1/2 sum_i  W_ii
 *   grad_b[2 + k] = dNLL/dbeta_k = -1/2 s sum_ij W_ij R_ij D_ijk^2,   k < d
 * written at grad + b * ldg (d + 2 values, ldg >= d + 2).
 *   Linv   the padded L^-1 of gp_potrf_inv under gp_alpha's layout rules: ldinv >= gp_padded_n(n),
 *          strideInv >= ldinv * gp_padded_n(n), any naturally aligned layout (a 16-B aligned base
 *          with even ldinv and strideInv selects 16-B loads); column c is taken as zero above
 *          row c and below row n - 1 whatever the buffer holds there.
 *   X      the n x d design shared by all problems (row i at X + i * ldx, ldx >= d);
 *          1 <= d <= GPFIT_MAX_DIM.  beta: d values at beta + b * ldbeta; s: one value per problem.
 *   alpha  n values at alpha + b * lda, from gp_alpha with the same Linv and w.
 *   ws     gp_nll_grad_ws_bytes(n, d, batch) bytes, 256-B aligned (the tiles' partial sums; -1
 *          for a negative size).
 * No n x n matrix is stored: one workgroup per lower 64 x 64 tile forms its tile of K^-1 = L^-T
 * L^-1 on fp64 MFMA over k >= the tile's first row (n^3 / 3 flop in all, the factorisation's count
 * without its dependency chain), subtracts alpha_i alpha_j, recomputes R_ij from X and beta and
 * writes its d + 2 partial sums; a second launch adds them in ascending tile order.  No atomics:
 * equal inputs give equal bits, whatever the layout and the problem's position in the batch.
 * Two launches per 65535 problems.  Stream-ordered, allocates nothing, can be captured into a
 * hipGraph.  n = 0 or batch = 0: no launch.  A violation returns minus its argument position
 * before anything is launched.  A problem whose factorisation reported info != 0 has an
 * unspecified gradient. */
long long gp_nll_grad_ws_bytes(int n, int d, int batch);
int gp_nll_grad(const double* Linv, int ldinv, long long strideInv, const double* X, int ldx,
                int n, int d, const double* beta, int ldbeta, const double* s,
                const double* alpha, int lda, double* grad, int ldg, int batch, void* ws,
                long long ws_bytes, hipStream_t stream);

/* Mean-response surfaces of the posterior mean: main effects (nfree = 1) and input pairs
 * (nfree = 2), the GP arithmetic of mean_response.py's compute_mean_response (lines 82-138:
 * per input dimension 11 targets x 20 Latin-hypercube integration points predicted and averaged)
 * and compute_mean_response_pairs (lines 159-208: one SepiaEmulatorPrediction of 10 points per
 * node of an 11 x 11 grid).  The kernel is a product over dimensions, so with alpha of gp_alpha
 * the average over the integration points has a closed form and no test point is materialised.
 * Per problem b and effect e, freeing d1 = effects[e*nfree] (and d2 = effects[e*nfree + 1]):
 *   M_n = (1/I) sum_i exp(-sum_{k not free} beta_b[k] (X[n,k] - Xint[i*ldi + col(k)])^2)
 *   out[b*ldb + e*lde + a2*T1 + a1] = s[b] sum_n alpha_b[n] M_n
 *          exp(-beta_b[d1] (X[n,d1] - t1[a1])^2) exp(-beta_b[d2] (X[n,d2] - t2[a2])^2)
 * (the d2 factor and a2 absent when nfree = 1): the posterior mean at x_d1 = t1[a1],
 * x_d2 = t2[a2] averaged over the I integration points placed in the other dimensions.
 *   effects  HOST array of E * nfree ints, read at enqueue (a captured graph keeps the values);
 *            d1 != d2, both in [0, d), in either order; E <= GPFIT_RESP_MAX_EFFECTS.
 *   order    which dimension integration column c takes: GPFIT_RESP_CYCLIC (d1 + 1 + c) mod d
 *            (compute_mean_response's dnums rule, nfree = 1 only), GPFIT_RESP_ASCENDING the
 *            non-free dimensions in ascending order (compute_mean_response_pairs's dim_int).
 *   t1, t2   T1 / T2 device values, 1 <= T <= gp_mean_response_max_grid(); t2 / T2 are ignored
 *            when nfree = 1 (T2 is taken as 1).
 *   Xint     device, row-major I x (d - nfree), row stride ldi >= d - nfree, I >= 1 and
 *            I (d - nfree) <= gp_mean_response_max_int_elems() (kept in LDS).  d == nfree:
 *            nothing to integrate, M_n = 1, Xint may be NULL and I is ignored.
 *   alpha    n values at alpha + b * lda;  X, beta, s, ldx, ldbeta as for gp_gram_ardse.
 *   out      lde >= T1 T2, ldb >= (E - 1) lde + T1 T2; nothing else of out is written.
 * One workgroup per (problem, effect); fp64 throughout, no atomics, one summation order fixed by
 * (n, I, T1, T2): equal inputs give equal bits, and the value of (b, e) does not depend on batch,
 * on E or on the other effects requested.  The error of a value is bounded by a small multiple of
 * eps s sum_n |alpha_n| M_n E1 E2: it scales with |alpha|, i.e. with the conditioning of A
 * ("Mean-response surfaces").  Stream-ordered, allocates nothing, can be captured into
 * a hipGraph.  E = 0, batch = 0 or n = 0: validated, nothing launched, nothing written.  A
 * violation returns minus its argument position (1 = X ... 24 = ldb) before any launch: a bad
 * effect -11, E above the limit -13, GPFIT_RESP_CYCLIC with nfree = 2 -14. */
#define GPFIT_RESP_CYCLIC 0      /* integration column c -> dimension (d1 + 1 + c) mod d     */
#define GPFIT_RESP_ASCENDING 1   /* integration columns -> the non-free dimensions, ascending */
#define GPFIT_RESP_MAX_EFFECTS 64
int gp_mean_response_max_grid(void);        /* 64 */
int gp_mean_response_max_int_elems(void);   /* 2048: largest I * (d - nfree) kept in LDS */
int gp_mean_response(const double* X, int n, int d, int ldx, const double* alpha, int lda,
                     const double* beta, int ldbeta, const double* s, int batch,
                     const int* effects, int nfree, int E, int order,
                     const double* t1, int T1, const double* t2, int T2,
                     const double* Xint, int I, int ldi,
                     double* out, long long lde, long long ldb, hipStream_t stream);

/* Closed-form Sobol' ingredients of the posterior mean under uniform inputs on the box
 * prod_k [lo_k, hi_k]: what utils.py:27-256 (saltelli_sensitivity_indices) estimates by sampling
 * the emulator's mean.  The U = G * M units (one (sample, PC) GP each: alpha of gp_alpha, beta,
 * s) are G groups of M consecutive units, unit u = g * M + a.  With w_k = hi_k - lo_k and
 *   I_k(u,n)       = (1/w_k) int exp(-beta_uk (x - X[n,k])^2) dx
 *   J_k(u,n;v,n')  = (1/w_k) int exp(-beta_uk (x - X[n,k])^2 - beta_vk (x - X[n',k])^2) dx
 * (finite sums of erf and exp) the call returns
 *   E[u*incE]                         = s_u sum_n alpha_un prod_k I_k(u,n)          (the mean)
 *   Q[g*ldqg + a*ldqa + b*ldq + 0]     = s_u s_v sum_nn' alpha_un alpha_vn' prod_k J_k
 *   Q[.. + 1 + i]                     = s_u s_v sum_nn' alpha_un alpha_vn' J_i
 *                                       prod_{k != i} I_k(u,n) I_k(v,n')
 *   Q[.. + 1 + d + i]                 = s_u s_v sum_nn' alpha_un alpha_vn' I_i(u,n) I_i(v,n')
 *                                       prod_{k != i} J_k
 * for every pair u = g M + a, v = g M + b of one group (pairs across groups are not computed):
 * E[f_u f_v], E[E[f_u|x_i] E[f_v|x_i]] and E[E[f_u|x_~i] E[f_v|x_~i]].  For the mean function of
 * a group, f = (1/M) sum_a f_a, with Eb = mean_a E and Qb = mean_ab Q: V = Qb_tot - Eb^2,
 * S_i = (Qb_main_i - Eb^2) / V, T_i = (Qb_tot - Qb_not_i) / V.
 *   X        row-major n x d, ldx >= d;  alpha: n values at alpha + u * lda;  beta: d values at
 *            beta + u * ldbeta;  s: one value per unit.  1 <= d <= GPFIT_MAX_DIM, M >= 1.
 *   lo, hi   d device values each, or both NULL for the unit box.  hi_k <= lo_k cannot be seen
 *            from the host: the result is then unspecified.
 *   Q        ldq >= 2 d + 1, ldqa >= (M - 1) ldq + 2 d + 1, ldqg >= (M - 1) (ldqa + ldq) +
 *            2 d + 1; both triangles are written, with the same bits; nothing else is.
 *   ws       gp_sobol_exact_ws_bytes(n, d, G, M) bytes, 256-B aligned (0 when n = 0 or G = 0;
 *            -1 for a negative size).
 * fp64 throughout, no atomics, every summation order fixed by (n, d) alone: equal inputs give
 * equal bits whatever G, M, the unit's position and the strides; a pair is computed once, as
 * (a, b) with a <= b, and mirrored; the (a, a) entry of a grouped call is the M = 1 call's.  The leave-one-out products
 * are prefix / suffix products, never quotients, so an underflowed J_i leaves Q_not_i finite.
 * The error of a value is a small multiple of eps times the same sum with |alpha_un alpha_vn'|
 * (DESIGN.md 4.6h).  Stream-ordered, allocates nothing, can be captured into a hipGraph.
 * n = 0: E and Q are written as 0.  G = 0: validated, nothing launched, nothing written.  A
 * violation returns minus its argument position (1 = X ... 21 = ws_bytes) before any launch;
 * lo without hi -13, hi without lo -12. */
long long gp_sobol_exact_ws_bytes(int n, int d, int G, int M);
int gp_sobol_exact(const double* X, int n, int d, int ldx, int G, int M, const double* alpha,
                   int lda, const double* beta, int ldbeta, const double* s, const double* lo,
                   const double* hi, double* E, long long incE, double* Q, long long ldq,
                   long long ldqa, long long ldqg, void* ws, long long ws_bytes,
                   hipStream_t stream);

/* Joint predictive covariance of the m test points of a call, per problem b, from the L^-1 of
 * gp_potrf_inv: what SepiaEmulatorPrediction forms for every (sample, PC) GP before it draws the
 * PC weights jointly.  With V_b = Linv_b K*_b (n x m; K* the cross-covariance gp_predict uses):
 *   C_b[i,j] = s_b exp(-sum_k beta_bk (xs_ik - xs_jk)^2) - sum_{r<n} V_b[r,i] V_b[r,j]   (i != j)
 *   C_b[i,i] = s_pred_b + jitter_b - sum_{r<n} V_b[r,i]^2
 * (the diagonal's prior term is s_pred_b itself), written column-major at C + b*strideC + i +
 * j*ldc for i, j < m, both triangles with the same bits (the tiles with J <= I are computed and
 * mirrored); every other element of the buffer (rows m .. ldc-1, the gaps between problems) is
 * left untouched.
 *   Linv     gp_predict's padded contract: 16-B aligned, ldinv >= gp_padded_n(n) and even,
 *            strideInv even and >= ldinv * gp_padded_n(n).  Column c is taken as zero above row c
 *            and for rows >= n whatever the buffer holds there.
 *   X, Xs, beta, s, ldx, ldxs, ldbeta as for gp_predict; 1 <= d <= GPFIT_MAX_DIM.
 *   jitter   one value per problem added to the diagonal, or NULL (= 0).
 *   ws       gp_predict_cov_ws_bytes(n, m, batch) bytes, 256-B aligned (K* and V, k-major; 0 when
 *            n, m or batch is 0, -1 for a negative size).
 * Each element is one k-ordered fp64 MFMA chain in one workgroup: no atomics, no split-K, equal
 * inputs give equal bits and a problem's result does not depend on the rest of the batch.
 * n = 0: the prior, nothing subtracted.  m = 0 or batch = 0: no launch.  Stream-ordered, allocates
 * nothing, can be captured into a hipGraph.  Argument checks run on the host, in argument order,
 * before anything is enqueued and return minus the argument's position (-1 .. -19); the
 * workspace answers with gp_predict's codes, -21 (NULL or misaligned) then -22 (too small). */
long long gp_predict_cov_ws_bytes(int n, int m, int batch);
int gp_predict_cov(const double* Linv, int ldinv, long long strideInv, const double* X, int ldx,
                   const double* Xs, int ldxs, int n, int m, int d, const double* beta,
                   int ldbeta, const double* s, const double* s_pred, const double* jitter,
                   double* C, int ldc, long long strideC, int batch, void* ws,
                   long long ws_bytes, hipStream_t stream);

/* Joint draws from N(mean_b, R_b R_b^T), R_b the lower factor gp_potrf left in C_b (column-major,
 * ldr, strideR):
 *   out[(b*nsamp + r)*ldo + i] = mean[b*ldm + i] + sum_{k<=i} R_b[i,k] xi_e,
 *   e = ((unit0 + b)*nsamp + r)*m + k,
 * xi_e element e of gp_realize's normal stream for (seed, offset): Philox4x32-10 at counter
 * (e/2, offset), Box-Muller, cos for even e and sin for odd e.  unit0 is the index of problem 0
 * in the caller's stream of problems, so a batch split over several calls with matching unit0
 * gives the bits of one call.  The strict upper triangle of R is never read (gp_potrf leaves the
 * upper half of C there).  mean may be NULL (= 0).  0 <= nsamp <= 262144; R is read once per
 * group of 8 draws.  m = 0, nsamp = 0 or batch = 0: no launch.  Stream-ordered, allocates
 * nothing, can be captured into a hipGraph.  A violation returns minus its argument position. */
int gp_mvn_draw(const double* R, int ldr, long long strideR, int m, const double* mean, int ldm,
                int nsamp, unsigned long long seed, unsigned long long offset, long long unit0,
                double* out, long long ldo, int batch, hipStream_t stream);

/* PCA truncation-error curve: the residual sums of every requested truncation rank in one pass
 * over the ensemble (plot_PC_RMSE.py:25-46,84-108: compute_truncation_error of the rank-k field
 * U_k S_k Vh_k for each of 26 ranks; include_trunc_error.py:41-49: np.var of the same residual).
 * With C = U diag(S) (n x pmax, row-major), V = Vh (pmax x ncols, row-major), pmax = ranks[nlev-1]:
 *   e_r[i,j]       = (Y[i*ldy + j] - mu[j]) - sd[j] * sum_{k < ranks[r]} C[i*ldc + k] V[k*ldv + j]
 *   tot[2r]        = sum_ij e_r^2          (RMSE = sqrt(tot[2r] / (n ncols)))
 *   tot[2r+1]      = sum_ij e_r            (np.var = tot[2r]/N - (tot[2r+1]/N)^2, N = n ncols)
 *   node[r*ldn + j] = sum_i e_r[i,j]^2     (node may be NULL)
 * for r < nlev.  Y is float32 (y_f32 = 1, widened exactly as it is loaded: the reference's
 * ensembles are float32 and are not copied) or fp64, row stride ldy >= ncols; everything else and
 * all arithmetic is fp64.  mu and sd (ncols each) are NULL together: 0 and 1.
 *   ranks  HOST array of nlev ints, 0 <= ranks[0] < ranks[1] < ... <= gp_pca_trunc_max_rank(),
 *          nlev <= gp_pca_trunc_max_levels(); read at enqueue (a captured graph keeps the values).
 *   ws     gp_pca_trunc_ws_bytes(n, ncols, nlev) bytes, 256-B aligned: 0 for an empty problem,
 *          -1 for a negative size or nlev above the limit.
 * Every level's sums are those of one k-ordered fp64 MFMA chain over k < ranks[r] per element (a
 * level's values do not depend on which other levels are requested), reduced without atomics in
 * an order fixed by (n, ncols) alone: equal inputs give equal bits, with or without node.
 * Argument checks run on the host before any launch and return minus the argument's position:
 * n, ncols, nlev and ranks first, then the other arguments in the order listed.  n = 0, ncols = 0
 * or nlev = 0: validated, nothing launched, nothing written.  Stream-ordered, allocates nothing,
 * can be captured into a hipGraph. */
int gp_pca_trunc_max_rank(void);
int gp_pca_trunc_max_levels(void);
long long gp_pca_trunc_ws_bytes(int n, int ncols, int nlev);
int gp_pca_trunc(const void* Y, long long ldy, int y_f32, int n, int ncols, const double* mu,
                 const double* sd, const double* C, long long ldc, const double* V,
                 long long ldv, const int* ranks, int nlev, double* tot, double* node,
                 long long ldn, void* ws, long long ws_bytes, hipStream_t stream);

/* out[0] = mean(x), out[1] = var(x, ddof) of a length-N vector (two-pass, deterministic);
 * work holds 1024 doubles.  np.var of the PC truncation residual, src/model.py:222. */
int gp_mean_var(const double* x, long long N, int ddof, double* out, double* work,
                hipStream_t stream);

/* A[i][i] += factor * trace(A) (shifted CholeskyQR); row i of M scaled by f[i] or 1/f[i]. */
int gp_shift_diag(double* A, int r, int lda, double factor, hipStream_t stream);
int gp_rowscale(double* M, int rows, int cols, int ld, const double* f, int inv,
                hipStream_t stream);

/* Symmetric eigendecomposition A = V diag(W) V^T by cyclic Jacobi (r <= 1024, one workgroup),
 * eigenvalues descending (want_sqrt = 1: W = sqrt(max(eig, 0)), the singular values when
 * A = B B^T); A is destroyed.  `sweeps` (device int, may be NULL) receives the sweep count.
 * The r x r core of np.linalg.svd(B) in src/svd.py:63 (via B B^T).  Sweeps stop at
 * off(A) <= tol ||A||_F, measured on entries normalised by a power of two taken from max|a| of
 * the input: A 2^k gives W 2^k, the same V and the same sweep count bit for bit wherever the
 * entries and the rotations' products stay in the normal range (no absolute threshold). */
int gp_syevj(double* A, int r, int lda, double* W, double* V, int ldv, int max_sweeps,
             double tol, int* sweeps, int want_sqrt, hipStream_t stream);

/* ------------------------------------------------------------------------------------------
 * RCCL over xGMI for the sharded emulator: one communicator per process /
 * GPU.  The (sample, PC) GPs are independent, so the only exchanges are one broadcast of the
 * inputs (X, X*, w_hat, hyperparameters) from rank 0 and one gather of the (mean, var) shards
 * to rank 0.  librccl is opened at run time (dlopen); where it cannot be loaded these return
 * GPFIT_ERR_RCCL and the rest of the library is unaffected.  The reference has no distributed
 * code: a C caller uses these instead of torch.distributed (gladsgp_amd.dist.NativeComm).
 *   gp_comm_unique_id: rank 0 writes the 128-byte id every rank passes to gp_comm_init (the
 *                      caller ships it out of band);
 *   gp_bcast:          `bytes` from `root`'s buf to every rank's buf (stream-ordered);
 *   gp_gather:         every rank's `bytes` at `send` land at recv + rank * bytes on `root`.
 * ---------------------------------------------------------------------------------------- */
int gp_comm_available(void);
int gp_comm_unique_id(void* id128);
int gp_comm_init(int nranks, int rank, const void* id128, void** comm);
int gp_comm_destroy(void* comm);
int gp_bcast(void* comm, void* buf, long long bytes, int root, hipStream_t stream);

/* Lower triangle of a column-major n x n matrix (leading dimension ld; column c from row c
 * on) to / from a contiguous vector of n (n + 1) / 2 doubles, column after column (round 4's
 * single-GP broadcast payload; the payload is now gp_pack_linv's tile-packed layout, which the
 * prediction reads in place).
 * gp_unpack_tril writes only the lower triangle (the strict upper part of A is left as it
 * is: zero in a buffer prepared for gp_predict). */
int gp_pack_tril(const double* A, int n, int ld, double* out, hipStream_t stream);
int gp_unpack_tril(const double* in, int n, double* A, int ld, hipStream_t stream);
int gp_gather(void* comm, const void* send, long long bytes, void* recv, int root,
              hipStream_t stream);

/*
 * Optional kernel timing (diagnostics; not part of the reference surface).  When enabled with
 * capacity > 0, instrumented launches record a hipEvent pair on their own stream; after the
 * stream has drained, gp_profile_read returns the number of recorded launches of kernel `id`
 * and their summed / largest device time in milliseconds.  A run of back-to-back launches of
 * one kernel on one stream (gp_fit_predict's and gp_predict_solve's TRMM chunks, the cross-
 * covariance chunks) is bracketed by one pair and counted as that many launches, so the
 * events do not add stream time between them; `max_ms` is then the largest per-launch mean of
 * a run.  Host-side, single-threaded use.
 */
#define GP_PROF_GRAM 0        /* gram / cross-covariance build (ardse_kernel)            */
#define GP_PROF_POTRF 1       /* whole gp_potrf_inv sequence                             */
#define GP_PROF_TRMM 2        /* predict: trmm_pair_kernel (dominant kernel)             */
#define GP_PROF_CROSS 3       /* predict: per-chunk cross-covariance build               */
#define GP_PROF_NUM 4
int gp_profile_enable(int capacity);
/* Which kernels record (bit GP_PROF_* set; default all): a timed run can keep only the
 * dominant kernel's event pair on the critical path.  Returns the previous mask. */
unsigned gp_profile_select(unsigned mask);
int gp_profile_reset(void);
int gp_profile_read(int id, int* count, double* total_ms, double* max_ms);

/* Test / diagnostics hook, process-wide (the library's one mutable setting): the number of
 * polls a wait of the persistent factorisation makes before it gives up and reports info = -1
 * for the launches enqueued afterwards.  polls > 0 sets it, 0 restores the default (2^22, far
 * beyond any legitimate wait), < 0 makes every later factorisation start with its problems
 * given up (info = -1 deterministically: the tests of the internal-error path).  The value
 * is read when a factorisation is enqueued, so a captured HIP graph keeps the one it was
 * captured with.  Returns the previous setting. */
long long gp_set_poll_budget(long long polls);

/* Test / A-B hook, process-wide: the factorisation path of gp_potrf_inv / gp_potrf /
 * gp_fit_predict / gp_loglik enqueued afterwards.  0 = automatic (the persistent dataflow
 * kernel where eligible -- with per-XCD task queues for batches that are multiples of 8 --,
 * else the blocked sweep), 1 = always the blocked right-looking sweep, 2 = the persistent
 * kernel with one shared task queue for every batch.  Returns the previous setting. */
int gp_set_potrf_path(int path);

/*
 * Test hooks: the persistent factorisation's task schedule, so that its order and the launch
 * rule can be checked without running a factorisation (tests/test_pp_sched_cpu.py checks them
 * against a dependence model, tests/test_gpu_pp_sched.py the device's list against the host's).
 * A task is (kind, i, j) on the 64 x 64 tiles of one problem, N = ceil(n / 64) tile rows:
 */
#define GP_PP_TASK_CHAIN 0  /* list entries only: the problem's chain (diagonal + subdiagonal)   */
#define GP_PP_TASK_LT 1     /* L tile (i, j), i >= j + 2                                         */
#define GP_PP_TASK_DP 2     /* partial sums of diagonal tile j (i = 0)                           */
#define GP_PP_TASK_SP 3     /* partial sums of subdiagonal tile (i, j), i = j + 1                */
#define GP_PP_TASK_XT 4     /* L^-1 tile (i, j), i > j                                           */
#define GP_PP_TASK_Z 5      /* zero the L^-1 tiles (r, i), r = j .. min(j + 8, i) - 1            */
#define GP_PP_TASK_XT2 6    /* L^-1 tiles (i, j) and (i, j + 1), i > j + 1                       */
#define GP_PP_TASK_ZP 7     /* zero the padding tile row N, tile columns i .. i + 7 (j = 0)      */

/*
 * gp_pp_schedule_host: the tasks of one problem of order n (inv = 1: with L^-1) in the order
 * the schedule kernel emits them with dequeue lead `lead` (0 .. 8), the chain entry not
 * included: task t as out[3t .. 3t+2] = (kind, i, j), for the first `cap` tasks.  Returns the
 * number of tasks (cap = 0: the size to allocate), the same for every lead.  Makes no HIP call.
 * n beyond the persistent kernel's range (n > 64 * 240) returns -1.
 */
long long gp_pp_schedule_host(int n, int inv, int lead, int* out, long long cap);

/*
 * gp_pp_plan: what a factorisation of (n, batch, inv) enqueued on a stream with `resident`
 * persistent workgroup slots would launch, from the same function the entry points use
 * (gp_set_potrf_path applies).  lead = -1: the library's own dequeue lead; 0 .. 8: that one
 * instead.  out[GP_PP_PLAN_*], GP_PP_PLAN_NUM words.  Makes no HIP call.  n beyond the
 * persistent kernel's range is no error: ELIGIBLE = 0 and GROUPS, GRID, TASKS are 0.
 * gp_pp_plan_stream is the same with `resident` taken from `stream` (its CU mask and the
 * persistent kernel's occupancy on the current device), reported in out[GP_PP_PLAN_RESIDENT].
 */
#define GP_PP_PLAN_ELIGIBLE 0      /* 1: the persistent kernel runs; 0: the blocked sweep        */
#define GP_PP_PLAN_N 1             /* tile rows, ceil(n / 64)                                    */
#define GP_PP_PLAN_LEAD 2          /* dequeue lead of this launch: 0 or KLEAD (or the given one) */
#define GP_PP_PLAN_KLEAD 3         /* the library's lead where the rule allows one               */
#define GP_PP_PLAN_KLEAD_BLOCKED 4 /* the rule's bound on blocked tasks per problem at KLEAD     */
#define GP_PP_PLAN_KXDELAY 5       /* chain steps the L^-1 tasks are dequeued behind their row   */
#define GP_PP_PLAN_KMAXN 6         /* largest N of the persistent kernel                         */
#define GP_PP_PLAN_GROUPS 7        /* dequeue queues: 1, or 8 (queue g: list entries 8k + g)     */
#define GP_PP_PLAN_GRID 8          /* workgroups launched                                        */
#define GP_PP_PLAN_TASKS 9         /* tasks per problem, its chain entry not counted             */
#define GP_PP_PLAN_RESIDENT 10     /* the residency the plan was made for                        */
#define GP_PP_PLAN_NKEYS 11        /* schedule keys (one schedule-kernel thread each, <= 1024)   */
#define GP_PP_PLAN_NUM 12
int gp_pp_plan(int n, int batch, int inv, int resident, int lead, long long* out);
int gp_pp_plan_stream(int n, int batch, int inv, int lead, long long* out, hipStream_t stream);

/*
 * gp_pp_schedule: enqueues the schedule kernel alone, as a factorisation of (n, batch, inv)
 * with dequeue lead `lead` (0 .. 8) does ahead of its persistent launch, into the 256-byte
 * aligned scratch `ws` of gp_pp_schedule_ws_bytes(n, batch, inv) bytes (the persistent part of
 * gp_potrf_inv_ws_bytes / gp_potrf_ws_bytes), and writes nothing past that size.  Needs n <=
 * 64 * 240.  Scratch layout, with T = out[GP_PP_PLAN_TASKS] tasks per problem:
 *   task list   batch * (T + 1) entries of two 32-bit ints, (kind | b << 4, i | j << 16) for
 *               problem b: first the batch chain entries (b = 0 .. batch-1), then each of the T
 *               tasks of gp_pp_schedule_host's order in turn for b = 0 .. batch-1; padded to a
 *               multiple of 256 bytes
 *   header      256 bytes, the dequeue counters: all 0 after the schedule kernel
 *   flag words  batch * fstride ints, fstride = 2 N^2 + 2 N + 1 rounded up to a multiple of 32:
 *               all 0 after the schedule kernel; padded to a multiple of 256 bytes
 * An invalid argument returns minus its position before any launch (-1: n, -2: batch, also a
 * task list of 2^30 entries or more, -3: inv, -4: lead, -5: ws null or not 256-byte aligned,
 * -6: ws_bytes too small).
 */
long long gp_pp_schedule_ws_bytes(int n, int batch, int inv);
int gp_pp_schedule(int n, int batch, int inv, int lead, void* ws, long long ws_bytes,
                   hipStream_t stream);

/* A-B hook, process-wide: the prediction path of gp_predict / gp_predict_ex / gp_fit_predict /
 * gp_predict_solve enqueued afterwards.  0 = automatic (at gp_padded_n(n) <= 512 the
 * column-resident kernel, the cross-covariance produced inside it when d <= 8 and read from
 * materialised chunks otherwise; above, cross-covariance chunks + the row-pair TRMM), 1 = always
 * cross-covariance chunks + the row-pair TRMM, 2 = the column-resident kernel from materialised
 * chunks at every d.  Paths 0 and 2 give the same bits; path 1 agrees to rounding.  Returns the
 * previous setting.  (Python: GPFIT_TRMM_RES=0 / 2 in the environment sets 1 / 2 at load.) */
int gp_set_predict_path(int path);

#ifdef __cplusplus
}
#endif
#endif /* GPFIT_H */
