/*
 * spadot_model.h -- C-ABI of libspadot_model.so: the hand-written HIP kernels (gfx950) behind the
 * model side of SpaDOT's training step.  All pointers are DEVICE pointers unless named *_host;
 * `stream` is a hipStream_t passed as void*; every function returns 0 or a negative errno-style
 * code and only ENQUEUES work (no host synchronisation).  No torch types appear here; the Python
 * host (spadot_amd/model) passes tensor.data_ptr() values.
 *
 * Reference interfaces replaced (all under /root/reference/SpaDOT):
 *   spadot_gat_*       torch_geometric GATConv's edge phase as called at model/encoder.py:56-58
 *                      (scatter-softmax over incoming edges + weighted scatter-add)
 *   spadot_kernel_matrix   model/svgp.py:110-125 (Kernel.forward: cdist + Gaussian/Cauchy/Quadratic)
 *   spadot_rowdot_*    the diag(A B^T) pattern of svgp.py:80, :98 and the trace identity replacing
 *                      the (b,m,m) tensor of svgp.py:99-101
 *   spadot_elbo_*      the scalar reductions of svgp.py:102-104 and model/SpaDOT.py:67-77,:125-142
 *   spadot_vae_*       model/SpaDOT.py:78-93 (reparameterisation, GAT KL, reconstruction, alignment)
 *   spadot_kmeans_*    utils/_train_utils.py:240-253 (loss) and sklearn KMeans.predict (labels, :266-269)
 *   spadot_adamw_*     utils/_train_utils.py:214-217 (clip_grad_norm_(0.3) + AdamW.step)
 *   spadot_pre_*, spadot_sparkx_*  utils/_utils.py:121-414 (SPARK-X) and utils/_preprocess_utils.py:11-49 (the preprocess stage)
 *   spadot_mk_*        no counterpart in the reference: scipy.stats.mannwhitneyu per (time point, gene, domain)
 *   spadot_silhouette  no counterpart in the reference: sklearn.metrics.silhouette_samples per (data set, labeling)
 *   spadot_gmm_*       no counterpart in the reference: sklearn.mixture.GaussianMixture(covariance_type="full") per (data set, K)
 *   spadot_weighted_moments  no counterpart in the reference: X_csc.T @ W of the log-normalised counts, three moments
 *   spadot_nhood_counts      no counterpart in the reference: the label-pair edge counts of squidpy's gr.nhood_enrichment
 *   spadot_territory_counts  no counterpart in the reference: the connected pieces of every domain (scipy's csgraph.connected_components)
 *   spadot_hop_sums          no counterpart in the reference: hop distances from every domain and every spot (squidpy's gr.centrality_scores)
 *   spadot_cooccur_counts    no counterpart in the reference: the label-pair counts by distance of squidpy's gr.co_occurrence
 *   spadot_cooccur_null      no counterpart in the reference: the same counts under relabelings (a random-labelling null)
 *   spadot_ripley_*          no counterpart in the reference: the pair, nearest-neighbour and empty-space counts of squidpy's gr.ripley
 *   spadot_local_lag         no counterpart in the reference: the neighbour sums and permutation counts of esda's Moran_Local
 *   spadot_cross_*           no counterpart in the reference: the cross sums of a bivariate Moran's I between genes (esda's Moran_BV)
 *   spadot_corr_sums         no counterpart in the reference: the band sums of a spatial correlogram (spdep's sp.correlogram)
 *   spadot_sepal_steps       no counterpart in the reference: the diffusion steps and the entropy stop of squidpy's gr.sepal, on the graph
 *   spadot_autocorr_sums     no counterpart in the reference: the edge sums of squidpy's gr.spatial_autocorr (Moran's I, Geary's C)
 *   spadot_ligrec_*          no counterpart in the reference: the per-domain sums and comparison counts of squidpy's gr.ligrec
 */
#ifndef SPADOT_MODEL_H
#define SPADOT_MODEL_H

#ifdef __cplusplus
extern "C" {
#endif

enum { SPADOT_DT_F32 = 0, SPADOT_DT_BF16 = 1, SPADOT_DT_F64 = 2 };
enum { SPADOT_KERNEL_GAUSSIAN = 0, SPADOT_KERNEL_CAUCHY = 1, SPADOT_KERNEL_QUADRATIC = 2 };

const char *spadot_model_version(void);

/* ---------------------------------------------------------------- GAT edge phase
 * Graph in CSR by TARGET node: rowptr[n+1], col[E] = source node of each incoming edge (self loops
 * already present exactly once per node, as GATConv(add_self_loops=True) leaves them).
 * h: [n, H*C] features after the layer's linear map (dtype = SPADOT_DT_F32 or _BF16);
 * s_src, s_dst: [n, H] fp32 attention logits (h . att_src, h . att_dst per head).
 *
 * forward:  e_ij = leaky_relu(s_src[j] + s_dst[i], 0.2); alpha = softmax over incoming edges of i
 *           (exp(e - max) / (sum + 1e-16)); agg_i = sum_j alpha_ij h_j
 *           concat != 0: out[i, H*C] = act(agg + bias[H*C])      (act = leaky_relu(0.01) if act != 0)
 *           concat == 0: out[i, C]   = act(mean_h agg + bias[C])
 *           alpha_out [E, H] fp32 is kept for the backward pass.
 */
int spadot_gat_forward(const void *h, int dtype, const float *s_src, const float *s_dst,
                       const int *rowptr, const int *col, const float *bias, int n, int H, int C,
                       int concat, int act, void *out, float *alpha_out, void *stream);

/* backward, target-side half: from g_out (gradient w.r.t. `out`, same shape/dtype as out) and the
 * saved forward tensors computes
 *   g_pre [n, H*C] (dtype) = gradient w.r.t. agg (activation and head-mean undone)
 *   dz    [E, H] fp32      = gradient w.r.t. the pre-leaky logits s_src[j] + s_dst[i]
 *   ds_dst[n, H] fp32      = sum over incoming edges of dz
 */
int spadot_gat_backward_target(const void *g_out, const void *out, const void *h, int dtype,
                               const float *s_src, const float *s_dst, const float *alpha,
                               const int *rowptr, const int *col, int n, int H, int C, int concat,
                               int act, void *g_pre, float *dz, float *ds_dst, void *stream);

/* backward, source-side half (no atomics): transposed CSR rowptr_t[n+1], col_t[E] = TARGET of each
 * outgoing edge, eid_t[E] = position of that edge in the target-ordered arrays (alpha, dz).
 *   dh[j]     = sum_{j->i} alpha_ij g_pre[i]      [n, H*C] (dtype)
 *   ds_src[j] = sum_{j->i} dz_ij                  [n, H] fp32
 */
int spadot_gat_backward_source(const void *g_pre, int dtype, const float *alpha, const float *dz,
                               const int *rowptr_t, const int *col_t, const int *eid_t, int n, int H,
                               int C, void *dh, float *ds_src, const float *ds_dst, const float *att_src,
                               const float *att_dst, void *stream);
/*   If att_src / att_dst ([H, C] fp32) are given (not NULL), the logits were produced by spadot_gat_logits
 *   and their gradient is folded into dh in the same pass:
 *       dh[j,h,c] += ds_src[j,h] att_src[h,c] + ds_dst[j,h] att_dst[h,c]        (ds_dst from the target half). */

/* Attention logits from h: s_src[j,h] = sum_c h[j,h,c] att_src[h,c], s_dst[j,h] likewise (h read once). */
int spadot_gat_logits(const void *h, int dtype, const float *att_src, const float *att_dst, int n, int H,
                      int C, float *s_src, float *s_dst, void *stream);
/* Gradient of the attention vectors: datt_src[h,c] = sum_j ds_src[j,h] h[j,h,c] (datt_dst with ds_dst).
 * datt_src and datt_dst must be the two halves of ONE [2, H*C] fp32 buffer (datt_dst == datt_src + H*C);
 * scratch: fp32 work space of scratch_floats >= 2*H*C entries (more = more parallel slabs).
 * With g_pre ([n_pre, H*C], n_pre <= n; else NULL) the buffer is [3, H*C] (scratch >= 3*H*C) and its third
 * block receives sum_i g_pre[i, :], the bias gradient before any head reduction, from the same pass. */
int spadot_gat_att_grad(const void *h, int dtype, const float *ds_src, const float *ds_dst, int n, int H,
                        int C, float *scratch, int scratch_floats, float *datt_src, float *datt_dst,
                        const void *g_pre, int n_pre, void *stream);

/* out[c] = sum_r x[r, c] for a row-major fp32 [rows, width] array, rows added in a fixed order (bias gradients of the
 * dense maps: no semaphore-based library reduction inside the replayed graphs). */
int spadot_colsum(const float *x, int rows, int width, float *out, void *stream);

/* ---------------------------------------------------------------- SVGP pieces */

/* K[i,j] = k(|x_i - z_j|^2 / scale), x [n,d], z [m,d], K [n,m]; dtype F32 or F64 for all three.
 * Gaussian exp(-d2/scale); Cauchy 1/(1+d2/scale); Quadratic 1 - d2/(d2+scale)  (svgp.py:116-124). */
int spadot_kernel_matrix(const void *x, const void *z, int n, int m, int d, double scale, int kind,
                         int dtype, void *K, void *stream);

/* Batched SPD inverse and log-determinant (fp64): A [L, m, m] symmetric positive definite ->
 * Ainv [L, m, m], logdet [L].  One workgroup per matrix, symmetric sweep operator, matrix resident in
 * registers + LDS (m <= 310; returns -34 beyond: the host splits larger matrices into blocks, spadot_amd/ops.py).  Replaces the
 * torch.linalg.inv / cholesky calls of svgp.py:50,75,87-88 on the L latent dimensions at once. */
int spadot_spd_inverse_logdet(const double *A, int L, int m, double *Ainv, double *logdet, void *stream);
/* Same for L matrices read as A[b mod Lsrc] + add0 (+ add1 for b >= Lsrc) (add0 / add1: m x m or NULL; Lsrc = 0: plain).
 * The SVGP step stores G_l = c K_mn diag(1/var_l) K_nm once and inverts Sigma_l = G_l + (K_mm + jI) and
 * Sigma_l + K_mm^2 / j (svgp.py:65-75 and the Sylvester form of :88) for every latent dimension in this one launch. */
int spadot_spd_inverse_logdet2(const double *A, int Lsrc, int L, int m, const double *add0, const double *add1, double *Ainv,
                               double *logdet, void *stream);

/* Batched row-wise dot products: out[l, i] = sum_k A[l, i, k] * B[i, k]   (A [L,n,m], B [n,m]).
 * dtype F32 or F64. */
int spadot_rowdot_forward(const void *A, const void *B, int L, int n, int m, int dtype, void *out,
                          void *stream);
/* gA[l,i,k] = g[l,i] * B[i,k]   (B is a constant of the step: no gradient) */
int spadot_rowdot_backward(const void *g, const void *B, int L, int n, int m, int dtype, void *gA,
                           void *stream);

/* ELBO scalar reductions over a [b, L] batch (row-major, L latent dims):
 *   l3 = -0.5 * sum_{i,l} [ (ktilde_i + tr_{i,l}) / var_{i,l} + log var_{i,l} + log(2 pi)
 *                           + (mu_{i,l} - mv_{i,l})^2 / var_{i,l} ]                (svgp.py:97-104)
 *   ce = sum_{i,l} -0.5 * [ log(2 pi) + log var + (pv + pm^2 - 2 pm mu + mu^2) / var ]  (SpaDOT.py:125-142)
 * out2[0] = l3, out2[1] = ce (fp64 accumulators written as `dtype`).
 * inputs: mu, var (encoder mean / variance), mv (K_nm K_mm^-1 mu_hat), tr (trace term), pm, pv
 * (posterior mean / variance): all [b, L]; ktilde [b]. */
int spadot_elbo_forward(const void *mu, const void *var, const void *mv, const void *tr, const void *pm,
                        const void *pv, const void *ktilde, int b, int L, int dtype, void *out2,
                        void *stream);
/* element-wise gradients given g2 = (dLoss/dl3, dLoss/dce) on the device: g_mu, g_var, g_mv, g_tr, g_pm,
 * g_pv, each [b, L]. */
int spadot_elbo_backward(const void *g2, const void *mu, const void *var, const void *mv, const void *tr,
                         const void *pm, const void *pv, const void *ktilde, int b, int L, int dtype,
                         void *g_mu, void *g_var, void *g_mv, void *g_tr, void *g_pm, void *g_pv,
                         void *stream);

/* ---------------------------------------------------------------- small-MLP stages (encoder.py:7-34, decoder.py:3-20)
 * BatchNorm1d in training mode + LeakyReLU(slope) in one launch: y = leaky((x + lin_bias - mean) invstd gamma + beta);
 * x [b, F] fp32 or bf16 (the preceding Linear's output WITHOUT its bias; lin_bias [F] or NULL is added here), batch
 * statistics over the b rows, running_mean / running_var / num_batches_tracked updated as nn.BatchNorm1d does
 * (momentum; unbiased running variance).  save_mean / save_invstd [F] feed the backward, which returns dx (dtype of x),
 * dgamma, dbeta (the gradient of lin_bias is identically zero: the batch mean removes it).
 * LayerNorm over the F features + LeakyReLU likewise (fp32; save_mean / save_invstd [b]). */
int spadot_bn_act_forward(const void *x, int x_dtype, const float *lin_bias, const float *gamma, const float *beta,
                          float *running_mean, float *running_var, long long *num_batches_tracked, int b, int F,
                          double momentum, double eps, double slope, float *y, float *save_mean, float *save_invstd,
                          void *stream);
int spadot_bn_act_backward(const float *dy, const float *y, const void *x, int x_dtype, const float *lin_bias,
                           const float *gamma, const float *save_mean, const float *save_invstd, int b, int F,
                           double slope, void *dx, float *dgamma, float *dbeta, void *stream);
int spadot_ln_act_forward(const float *x, const float *gamma, const float *beta, int b, int F, double eps, double slope,
                          float *y, float *save_mean, float *save_invstd, void *stream);
int spadot_ln_act_backward(const float *dy, const float *y, const float *x, const float *gamma, const float *save_mean,
                           const float *save_invstd, int b, int F, double slope, float *dx, float *dgamma, float *dbeta,
                           void *stream);

/* SVGP branch after the batched inverse, all latent dimensions, fp64 (svgp.py:62-104, SpaDOT.py:72-77).
 * forward: raw = X2 r^T [2b, L] (X2 = [K_nm; K_nm K^-1 K_mm]), rd = rowdot(X2 S, X2) [L, 2b], r and Mr = r M [L, m],
 * ld [2L] log-determinants, sm [L] = <S_l, M>, mu / var [b, L] encoder output, ktilde [b]  ->  p_m, mv, p_v, tr [b, L]
 * and out4 = (l3, ce, KL sum, SVGP_KL = -|ce - (l3 - (b/N) KL)| / L); kl_const = log|K| - m log j - m.
 * backward: g_skl fp32 device scalar, G_pm / G_pv upstream gradients or NULL -> direct g_mu, g_var [b, L], the operands
 * G1 [2b, L] and G2T [L, 2b] of the algebra's backward, g_kl, gMr = g_kl c^2 Mr [L, m], gM = g_kl/2 M [m, m].
 * grad_tail: the last element-wise step of that backward (see model/svgp.py:_SVGPCore). */
int spadot_svgp_post_forward(const double *raw, const double *rd, const double *r, const double *Mr, const double *ld,
                             const double *sm, const double *mu, const double *var, const double *ktilde, int b, int L,
                             int m, double c, double kl_const, double b_over_N, double *p_m, double *mv, double *p_v,
                             double *tr, double *out4, float *skl32 /* may be NULL: SVGP_KL once more in fp32 */, void *stream);
int spadot_svgp_post_backward(const float *g_skl, const double *out4, const double *G_pm, const double *G_pv,
                              const double *mu, const double *var, const double *mv, const double *tr, const double *p_m,
                              const double *p_v, const double *ktilde, const double *Mr, const double *M, int b, int L,
                              int m, double c, double b_over_N, double *g_mu, double *g_var, double *G1, double *G2T,
                              double *g_kl, double *gMr, double *gM, void *stream);
/* q1[l, i] = sum_n G2T[l, n] T[l, n, i]^2 + g_kl / 2 * m0[l, i]: the diag(K_nm dSigma K_mn) term of _SVGPCore.backward
 * (svgp.py:62-104 differentiated) from T_l = X2 S_l K_mn, given as its two halves Ta = K_nm S_l K_mn and Tb = P S_l K_mn
 * (each [L, nh, b]; G2T [L, 2 nh]), and m0 [L, b], all formed ahead of the backward pass. */
int spadot_svgp_q1t(const double *Ta, const double *Tb, const double *G2T, const double *m0, const double *g_kl, int L, int nh,
                    int b, double *q1, void *stream);
/* p_m = c raw[:b] and p_v = k~ + rd_a^T (rd_a [L, b] = diag(K_nm S_l K_mn)): what the loss tail needs of
 * spadot_svgp_post_forward (svgp.py:62-84), which may then run later. */
int spadot_svgp_post_pm_pv(const double *raw, const double *rd_a, const double *ktilde, int b, int L, double c, double *p_m,
                           double *p_v, void *stream);
int spadot_svgp_grad_tail(const double *q1, const double *q2, const double *Kdt, const double *p_v, const double *ktilde,
                          const double *p_m, const double *mu, const double *w, const double *g_kl, const double *g_mu,
                          const double *g_var, int b, int L, double c, double *dmu, double *dvar, float *dz,
                          void *stream);
/* z [b, 2L] fp32 = SVGP_fc output (mu | logvar) -> mu, var = exp(logvar), w = 1/var, mu w, each [b, L] fp64
 * (encoder.py:31-34 + the first element-wise steps of svgp.py:62-70).  grad_tail's dz [b, 2L] fp32 is the matching
 * gradient (d/dlogvar = d/dvar * var); dmu/dvar may then both be NULL (one of the pair alone is refused: -22). */
int spadot_svgp_pre(const float *z, int b, int L, double *mu, double *var, double *w, double *muw, void *stream);
/* ... and A[l, i, :] = K_nm[i, :] / var[i, l]  ([L, b, m] fp64) in the same launch */
int spadot_svgp_pre2(const float *z, const double *Kn, int b, int L, int m, double *mu, double *var, double *w, double *muw,
                     double *A, void *stream);
/* The small products behind the inverse for all L latent dimensions in two launches: r_l = S_l t_l, Mr_l = M r_l,
 * raw[:, l] = X2 r_l (X2 [rows2, m]) and sm_l = <S_l, M>; smpart: scratch of >= L * 4 * ceil(m / 4) doubles. */
int spadot_svgp_mid(const double *S, const double *t, const double *M, const double *X2, int L, int m, int rows2,
                    double *r, double *Mr, double *raw, double *sm, double *smpart, int smpart_doubles, void *stream);

/* ---------------------------------------------------------------- loss tail of a training step
 * Single-workgroup kernels for the b x 20 / 10 x 10 arithmetic after the encoders (each replaces a few dozen
 * library launches; reductions in a fixed order, fp64 accumulators).
 *
 * latent head (SpaDOT.py:78-93): zg [b, 2 Lg] fp32 = GAT_fc output (mu | logvar), p_m / p_v [b, Ls] fp64 = SVGP
 * posterior, eps [b, Ls+Lg] fp32 standard normal.  latent [b, Ls+Lg] = (p_m + eps sqrt(p_v) | mu + eps
 * sqrt(exp(logvar))); scal2 = (GAT_KL = -1/2 sum(1 + logvar - mu^2 - var) / Lg,
 * alignment = sum_i (|s_i| / Ls - |g_i| / Lg)^2); Ls + Lg <= 32; partials: 2 * ceil(b/8) doubles of work space, counter: one
 * unsigned that is 0 before the first launch (the kernel leaves it 0).  rng_state NULL: eps is an input; else eps is
 * WRITTEN by the kernel (counter-based standard normals from rng_state = (seed, launch count); the count advances by
 * one per launch), so that no library RNG launch sits in the replayed graph.  backward: g_latent [b, Ls+Lg] or NULL, g_kl / g_align device
 * scalars or NULL -> d_zg [b, 2 Lg], d_pm, d_pv [b, Ls] fp64. */
int spadot_latent_head_forward(const float *zg, const double *p_m, const double *p_v, float *eps, int b, int Ls,
                               int Lg, float *latent, float *scal2, double *partials, unsigned *counter,
                               unsigned long long *rng_state, void *stream);
int spadot_latent_head_backward(const float *zg, const double *p_v, const float *eps, const float *latent,
                                const float *g_latent, const float *g_kl, const float *g_align, int b, int Ls, int Lg,
                                float *d_zg, double *d_pm, double *d_pv, void *stream);
/* K-means loss (_train_utils.py:240-253) and OT loss (_train_utils.py:272-307) of one batch.  z [b, D] fp32;
 * labels_all[seed_ids[i]] (int64) = cluster of seed i; centres [K, D]; prev_centres [Kp, D]; gamma [Kp, Kl]
 * row-normalised plan; cluster_list [Kl] int64 = clusters of the time point, ascending.  K <= 64, D <= 64.
 * out2 = (||z - c[label]||^2 / D / #distinct labels, mean(gamma * cdist(prev, batch means or stored centre))).
 * work: K*D + K + 1 + b floats, written by forward, read by backward.  do_km / do_ot switch the terms. */
int spadot_cluster_losses_forward(const float *z, const long long *labels_all, const long long *seed_ids,
                                  const float *centres, const float *prev_centres, const float *gamma,
                                  const long long *cluster_list, int b, int D, int K, int Kp, int Kl, int do_km,
                                  int do_ot, float *out2, float *work, void *stream);
int spadot_cluster_losses_backward(const float *z, const float *centres, const float *prev_centres, const float *gamma,
                                   const long long *cluster_list, const float *work, const float *g_km,
                                   const float *g_ot, int b, int D, int K, int Kp, int Kl, int do_km, int do_ot,
                                   float *dz, void *stream);
/* forward AND dz = d(g_km[0] * km + g_ot[0] * ot) / dz in ONE launch, for gradient seeds known when the forward runs (the loss
 * weights of _train_utils.py:205-212, device scalars).  Same arithmetic as forward + backward.  Returns -95 when the shape
 * does not take the kernel's one-chunk fast path (K <= 16, K * D <= 512, b * D <= 10240): call forward / backward then. */
int spadot_cluster_losses_fb(const float *z, const long long *labels_all, const long long *seed_ids, const float *centres,
                             const float *prev_centres, const float *gamma, const long long *cluster_list, int b, int D, int K,
                             int Kp, int Kl, int do_km, int do_ot, const float *g_km, const float *g_ot, float *out2,
                             float *work, float *dz, void *stream);
/* elbo = sum_k w6[k] * *terms6[k] (_train_utils.py:205-212); out7 [8 floats] = (elbo, the six terms, elbo again).
 * terms6 is a HOST array of six device pointers.  backward: g6[k] = g_elbo[0] * w6[k]. */
int spadot_mix_losses_forward(const float *const *terms6, const float *w6, float *out7, void *stream);
int spadot_mix_losses_backward(const float *g_elbo, const float *w6, float *g6, void *stream);

/* ---------------------------------------------------------------- VAE head losses (SpaDOT.py:78-93)
 * out1[0] = inv_scale * sum_k (y[k] - yhat[k])^2 over `count` elements (recon: inv_scale = 1/G),
 * deterministic two-stage reduction through `scratch` (>= 2048 doubles).
 * backward writes g_yhat[k] = -2 inv_scale (y[k] - yhat[k]) * g1[0]. */
int spadot_sqerr_forward(const void *y, const void *yhat, long long count, double inv_scale, int dtype,
                         double *scratch, void *out1, void *stream);
int spadot_sqerr_backward(const void *g1, const void *y, const void *yhat, long long count,
                          double inv_scale, int dtype, void *g_yhat, void *stream);

/* ---------------------------------------------------------------- k-means glue */
/* labels[i] = argmin_c |x_i - c_c|^2 (first minimum wins), x [n,d], centers [k,d], int32 labels.
 * Distances are accumulated in fp64 whatever `dtype` (F32/F64) the inputs have. */
int spadot_kmeans_assign(const void *x, const void *centers, int n, int k, int d, int dtype, int *labels,
                         void *stream);

/* Small fp32 products of the MLP stages with a small footprint (32 x 32 tiles, 256 threads, 8 KB of LDS): they find room on a
 * compute unit beside the GAT branch's GEMMs, where the library's 256 x 64 macro tiles waited 150-185 us for a whole unit.
 *   C [M x N] (row stride ldc) = sum_k a(m, k) b(k, n) (+ bias[n] when bias != NULL), k ascending (fixed order):
 *   mode 0: a = A[m * lda + k], b = B[k * ldb + n]   (dx = g W)
 *   mode 1: a = A[m * lda + k], b = B[n * ldb + k]   (y = x W^T + bias: the forward map of nn.Linear)
 *   mode 2: a = A[k * lda + m], b = B[k * ldb + n]   (dW = g^T x)
 * `batch` such products in one launch, entry z using A + z strideA, B + z strideB, C + z strideC (elements): a long
 * contraction (mode 2 over hundreds of rows) is cut into row slices whose partial results the caller adds in slice order.
 * Meant for products of at most a few hundred MFLOP. */
int spadot_sgemm_small(int mode, const float *A, int lda, const float *B, int ldb, float *C, int ldc, int M, int N, int K,
                       const float *bias, int batch, long long strideA, long long strideB, long long strideC, void *stream);

/* ---- The SVGP encoder behind its first map as three launches (csrc/enc_fused.hip, round 5; encoder.py:7-34 in training mode) ----
 * h1 [b x F1] (fp32, the first map's output without its bias) -> BatchNorm1d + LeakyReLU -> y1 -> hidden map -> h2 [b x F2] ->
 * BatchNorm1d + LeakyReLU -> y2 -> SVGP_fc -> z [b x Q].  The two maps cross workgroups as PARTIAL PRODUCTS in a caller-owned
 * workspace (spadot_enc_fused_workspace floats: part [F1 / 16][b][F2], then pz [F2 / 4][b][Q]), summed in group order by the
 * next launch: spadot_enc_bn_map (statistics of 16 columns of h1, y1, running statistics, part), spadot_enc_bn_fc (h2 = sum of
 * part -- stored without the map's bias, which BatchNorm's lin_bias carries --, y2, running statistics, pz), and either
 * spadot_enc_sum_z (z = bias + sum of pz) or spadot_svgp_pre2_partials (spadot_svgp_pre2 reading z from pz; it also stores z).
 * b <= 512, F1 % 16 == 0, F2 % 4 == 0, F2 <= 128, Q <= 32; both readers of pz take 1 .. 64 partials.  y1 is bit for bit what
 * spadot_bn_act_forward writes. */
int spadot_enc_fused_supported(int b, int F1, int F2, int Q);
long long spadot_enc_fused_workspace(int b, int F1, int F2, int Q);
int spadot_enc_bn_map(const float *h1, const float *lin_bias, const float *gamma, const float *beta, float *running_mean,
                      float *running_var, long long *num_batches_tracked, int b, int F1, double momentum, double eps, double slope,
                      float *y1, float *save_mean, float *save_invstd, const float *W2, int F2, float *part, void *stream);
int spadot_enc_bn_fc(const float *part, int nparts, const float *lin_bias, const float *gamma, const float *beta, float *running_mean,
                     float *running_var, long long *num_batches_tracked, int b, int F2, double momentum, double eps, double slope,
                     float *h2, float *y2, float *save_mean, float *save_invstd, const float *Wfc, int Q, float *pz, void *stream);
int spadot_enc_sum_z(const float *pz, int nparts, const float *bias, int b, int Q, float *z, void *stream);
int spadot_svgp_pre2_partials(const float *pz, int nparts, const float *bias, const double *Kn, int b, int L, int m, float *z,
                              double *mu, double *var, double *w, double *muw, double *A, void *stream);

/* ---- The decoder's output map, the reconstruction term and their backward as one launch (csrc/recon_fb.hip, round 5) ----------
 * decoder.py:3-20 (last Linear: hidden K = 256 -> G) + SpaDOT.py:89 (recon = inv_scale * sum (y - (h W^T + bias))^2) forward AND
 * backward for a gradient seed known at forward time: grad_weight[0] = d loss / d recon (the loss weight lambda1,
 * _train_utils.py:205-212, a device scalar).  h_bf16 [b x K], W_bf16 [G x K] (bf16 images of h and of the weight), y [b x G] fp32.
 * Leaves: g_bf16 [b x G] = -2 inv_scale grad_weight (y - o - bias) in bf16 (the weight gradient g^T h is the caller's GEMM),
 * dh [b x K] fp32 = g W (gene blocks summed in block order), in `workspace` (spadot_recon_fb_workspace floats) behind the
 * per-gene-block partials of dh the bias-gradient partials dbp [ceil(b / 64)][G] (sum them: spadot_colsum), and in loss_parts
 * (ceil(b / 64) * ceil(G / 128) doubles) the partial sums of (y - o - bias)^2 (spadot_sum_parts with scale = inv_scale gives the
 * term's value).  The fp32 image of o = h W^T is never formed.  WT_bf16 [K x ldt]: the TRANSPOSED bf16 image of the weight, rows
 * padded to ldt >= G rounded up to 128 (the second product reads it like the first reads W: 16 bytes per lane straight from
 * memory, no weight tile in LDS -- the workgroups stay small enough to be placed beside another stream's GEMMs).
 * K == 256, G % 8 == 0, G >= 128. */
int spadot_recon_fb_supported(int b, int K, int G);
long long spadot_recon_fb_workspace(int b, int K, int G);
int spadot_recon_fb(const void *h_bf16, const void *W_bf16, const void *WT_bf16, int ldt, const float *bias, const float *y, int b, int K,
                    int G, double inv_scale, const float *grad_weight, void *g_bf16, float *workspace, double *loss_parts, float *dh,
                    void *stream);
int spadot_sum_parts(const double *part, int n, double scale, float *out, void *stream);

/* Measurement aid: buf[slot] = the device's constant-rate timestamp counter (100 MHz: 10 ns units) when the launch runs.
 * Launched at the head and the end of a captured stage it dates the stage on the GPU with no profiler attached. */
int spadot_stamp(unsigned long long *buf, int slot, void *stream);

/* One Lloyd iteration of K-means for R restarts at once, over several data sets and cluster counts in one launch pair (fp64,
 * no atomics: two fits of the same data are bitwise identical).  Restart r belongs to set rgroup[r] (rows xoff[g] .. xoff[g] +
 * npts[g] - 1 of the centred data X [sum npts, D], stopping threshold tol[g]) and has Kr[r] <= K_max clusters; C [R, K_max, D]
 * keeps its first Kr[r] rows, updated in place unless done[r] (the rest is padding, never read or written).  Each restart sums
 * over its own clusters and points only, so its result does not depend on the other restarts of the launch.  done [R] int
 * flags (set when the squared centre shift <= tol[g]), inertia [R] = inertia of the centres the iteration started from.  n_max
 * = the largest npts (grid size); part: work space of R * ceil(n_max / 256) * (K_max (D + 1) + 1) doubles.  skip_done != 0:
 * restarts whose done flag is set are left alone entirely (their centres are final; inertia[r] then still belongs to the
 * centres of the iteration that froze them -- measure the final one with a call that has skip_done = 0 and every done flag
 * set).  xoff, npts: int32 device arrays [sets]; rgroup, Kr: int32 device arrays [R]; tol: fp64 device array [sets].
 * K_max <= 32 and (K_max + 256) * D <= 7936 (K_max centres and 256 points in LDS), hence D <= 30; R <= 65535; anything else
 * returns -22 and launches nothing.  An EMPTY cluster keeps its centre (sklearn relocates it).  (KMeans of
 * _train_utils.py:255-269 and _analyze_utils.py:42-105.) */
int spadot_lloyd_step(const double *X, double *C, const int *xoff, const int *npts, int n_max, int R, const int *rgroup,
                      const int *Kr, int K_max, int D, const double *tol, double *part, int *done, double *inertia, int skip_done,
                      void *stream);
/* k-means++ seeding (sklearn's rule: 2 + int(log k) candidates per further centre, drawn
 * by potential; the candidate whose new potential is smallest wins, first on ties) for P problems in one launch, one workgroup
 * each.  Problem p seeds pK[p] <= K_max centres on group pset[p] (rows xoff[g] .. xoff[g] + npts[g] - 1 of the centred data
 * X, npts[g] <= n_max), starting from row pfirst[p]; round c (1 <= c < pK[p]) reads its uniforms from
 * U[puoff[p] + (c - 1) * trials ...].  Candidate = first index whose prefix sum of the current distances is >= u * potential
 * (clamped to n - 1); distances in the expanded form xsq - 2 x.c + csq clamped at 0.  The prefix sums are a fixed-order
 * workgroup scan (bitwise reproducible), rounded in a different order from torch.cumsum: a candidate can differ from the torch
 * path's only when a draw lies within rounding distance of a boundary.  Outputs: idx [P, K_max] int32 row indices (-1 in
 * padding rows and for an invalid problem), centers [P, K_max, D] fp64 (zero padding).  closest: work space of P * n_max
 * doubles.  D <= 32, K_max <= 32 (two more dimensions than spadot_lloyd_step holds). */
int spadot_kmeanspp_seed(const double *X, const int *xoff, const int *npts, int D, int P, const int *pset, const int *pK,
                         const int *pfirst, const int *puoff, const double *U, int K_max, int n_max, double *closest, int *idx,
                         double *centers, void *stream);

/* Exact kk nearest neighbours of every point among all n points (self included), brute force in fp64, ordered by
 * (squared distance, index): out [n, kk] int32.  x [n, d] fp64, d <= 4, kk <= min(n, 128).  Replaces the host
 * NearestNeighbors call of _Cal_Spatial_Net (_utils.py:66-75) when the coordinates already live in HBM. */
int spadot_knn(const double *x, int n, int d, int kk, int *out, void *stream);

/* ---------------------------------------------------------------- GAT edge phase on the matrix cores (bf16 rows)
 * Same arithmetic as spadot_gat_forward / _backward_target / _backward_source (GATConv message passing of
 * /root/reference/SpaDOT/model/encoder.py:41-58) for bf16 rows with C = 512 channels per head, H in
 * {1, 2, 4, 8} and head concat, organised by BLOCK PLANS (spadot_amd/graph.py: BlockPlan): blocks of 32 rows, each
 * with the list of its distinct columns (plan_cols, padded to a multiple of 32, offsets plan_sptr).  Every distinct
 * source row of a block is fetched once (LDS-DMA) and the weighted sum is a dense product on v_mfma_f32_32x32x16_bf16.
 * The weights travel as a dense image `acell` [chunk of 16 columns][head][hi | lo][512] of bf16 (weights = hi + lo, 16
 * significant bits; zero where the tile has no edge; the 512 positions of a 32 x 16 tile are in MFMA fragment order),
 * which the per-node kernels fill through cellq[e] = chunk * 512 + position of edge e.  The image must be ZERO before
 * its first use and may then be reused: edges always overwrite the same cells.
 *   spadot_gat_alpha             alpha[e, hd] = softmax over the incoming edges of each of the n_tgt targets, written as
 *                                fp32 [E, H] and into the by-target plan's image (cellq = plan's cellq) and, optionally, into
 *                                the by-SOURCE plan's image (cellq_s indexed by by-target edge position): round 5, the
 *                                backward product's weights are gradient-independent and are written by the forward pass
 *   spadot_gat_aggregate         mode 0: out[row] = act?(sum_cols w x[col] + vec_a (bias));              plan by target
 *                                mode 1: out[row] = sum_cols w x[col] + ds_src[row] vec_a + ds_dst[row] vec_b  (att_src,
 *                                att_dst: the logits' own gradient path);                                plan by source
 *                                with att_part (mode 1; h_rows = the layer's input h): block b also leaves the partial sums
 *                                sum_rows ds_src[row] h[row] at att_part[b * part_width + 0 ..] and the ds_dst ones at
 *                                [.. + H C ..] -- the attention-vector gradients up to a column sum over the blocks;
 *                                rows pad_from .. pad_to - 1 of `out` (allocated past the last node so that the next GEMM
 *                                sees a row count that is a multiple of 128) are written as zeros; with dz (mode 1) the
 *                                workgroup sums dz over the outgoing edges of its own rows itself (transposed CSR rowptr_t /
 *                                eid_t: what spadot_gat_ds_src computes in a launch of its own), ds_src may then be NULL and
 *                                ds_src_out (may be NULL) receives the sums
 *   spadot_gat_edge_dot          g_pre = g_out * (act ? LeakyReLU'(out) : 1) (written), dz[e] = <g_pre[row], h[col]> through
 *                                plan_cell [chunk][32 rows][16] -> edge position or -1; with bias_part block b leaves the
 *                                column sums of its 32 rows of g_pre at bias_part[b * part_width + part_col ..] (the bias
 *                                gradient up to a column sum over the blocks: spadot_colsum, fixed order)
 *   spadot_gat_softmax_backward  dz (raw d alpha) -> d logits in place, ds_dst[i] = sum over incoming edges; with cellq_s /
 *                                acell_s (both or neither) alpha is also written into the by-SOURCE plan's image
 *   spadot_gat_ds_src            ds_src[j] = sum of dz over the outgoing edges of j (transposed CSR)
 * spadot_gat_mfma_supported(dtype, H, C, max_cols) tells whether a plan whose longest column list is max_cols can run. */
int spadot_gat_mfma_supported(int dtype, int H, int C, int max_cols);

/* ---- The last GAT layer for the seeds only, aggregate-first (csrc/gat_tail.hip, round 4) -----------------------------
 * Replaces, for gat3 = GATConv(H*C -> C, heads = H, concat = False) (encoder.py:45,58; PyG GATConv semantics)
 * whose targets are the first n_tgt << n nodes (only the seeds' rows reach the loss, SpaDOT.py:82), the dense map over
 * ALL n source rows by dense maps over the n_tgt aggregated rows:
 *     out_i = 1/H sum_h ( sum_j alpha_ij^h x_j ) W_h^T + bias,   e_ij^h = leaky_relu_0.2( x_j . w_src^h + x_i . w_dst^h ),
 *     w_src^h = W_h^T att_src^h, w_dst^h = W_h^T att_dst^h          (W_h = rows h C .. h C + C - 1 of lin.weight [H C, K]).
 * dtype: 0 = fp32, 1 = bf16 rows (x, A, dA, dx, O); K <= 2048, K % 8 == 0, H in {1, 2, 4, 8}; everything else fp32.
 * s [n][2 H]: s[j][2 h] = x_j . w_src^h, s[j][2 h + 1] = x_j . w_dst^h.  CSR by target (rowptr [n_tgt + 1], col) and by
 * source (rowptr_t [n + 1], col_t = target, eid_t = position of the edge in the by-target order), self loops included.
 *   spadot_gat_tail_wvec             wv [2 H][K] from W, att (part: workspace of slices * 2 H * K floats); whi / wlo (both or neither
 *                                    NULL): bf16 images [2 H][K] with wv = whi + wlo to 16 bits, for the matrix-core logits
 *   spadot_gat_tail_logits           s = x wv^T for all n rows (bf16 rows with whi / wlo and K % 32 == 0: on the matrix cores)
 *   spadot_gat_tail_aggregate        alpha [E][H] (softmax over the incoming edges of each target: exp(e - max) / (sum + 1e-16))
 *                                    and A [H][n_tgt][K] = sum_j alpha x_j
 *   spadot_gat_tail_headmean         out [n_tgt][C] = 1/H sum_h O[h] + bias            (O [H][n_tgt][C] = A_h W_h^T, a library GEMM)
 *   spadot_gat_tail_colsum_rows      column sums of g [rows][C] in fp32 (the bias gradient)
 *   spadot_gat_tail_edge_backward    dz [E][H] = d logit per edge (through aggregation, softmax and leaky_relu), ds_dst [n_tgt][H]
 *   spadot_gat_tail_source_backward  dx [rows_out][lddx] (rows n .. rows_out - 1 zero), ds_src [n][H]; with act_out (the layer's
 *                                    input rows [rows_out][ldm], may be NULL) dx is multiplied by `slope` where act_out <= 0
 *   spadot_gat_tail_dwvec            per-block partials [spadot_gat_tail_dwvec_rows(n)][2 H][K] of d wv (spadot_colsum adds them)
 *   spadot_gat_tail_wvec_backward    dW (+)= att (x) d wv per row of W, datt = W d wv
 * All sums in fixed orders, no atomics: repeated calls are bit-identical. */
int spadot_gat_tail_supported(int dtype, int H, int K);
int spadot_gat_tail_wvec(const float *W, int ldw, const float *att_src, const float *att_dst, int H, int C, int K, float *part,
                         int slices, float *wv, void *whi, void *wlo, void *stream);
int spadot_gat_tail_logits(const void *x, int dtype, int ldx, const float *wv, const void *whi, const void *wlo, int n, int H, int K,
                           float *s, void *stream);
int spadot_gat_tail_aggregate(const void *x, int dtype, int ldx, const float *s, const int *rowptr, const int *col, int n_tgt, int H,
                              int K, void *A, float *alpha, void *stream);
int spadot_gat_tail_headmean(const void *O, int dtype, const float *bias, int n_tgt, int H, int C, void *out, void *stream);
int spadot_gat_tail_colsum_rows(const void *g, int dtype, int rows, int C, float *out, void *stream);
/* ... and gs = scale * g (same dtype) in the same pass: the backward's d O_h = g / H and the bias gradient in one launch */
int spadot_gat_tail_scale_colsum(const void *g, int dtype, int rows, int C, double scale, void *gs, float *out, void *stream);
int spadot_gat_tail_edge_backward(const void *x, int dtype, int ldx, const void *dA, const float *s, const float *alpha, const int *rowptr,
                                  const int *col, int n_tgt, int H, int K, float *dz, float *ds_dst, void *stream);
int spadot_gat_tail_source_backward(const void *dA, int dtype, const float *alpha, const float *dz, const float *ds_dst, const float *wv,
                                    const int *rowptr_t, const int *col_t, const int *eid_t, int n, int n_tgt, int rows_out, int H, int K,
                                    void *dx, int lddx, float *ds_src, const void *act_out, int ldm, double slope, void *stream);
int spadot_gat_tail_dwvec_rows(int n);
int spadot_gat_tail_dwvec(const void *x, int dtype, int ldx, const float *ds_src, const float *ds_dst, int n, int n_tgt, int H, int K,
                          float *part, void *stream);
int spadot_gat_tail_wvec_backward(const float *W, int ldw, const float *att_src, const float *att_dst, const float *dwv, int H, int C, int K,
                                  float *dW, int lddw, int accumulate, float *datt_src, float *datt_dst, void *stream);
/* (cellq_s / acell_s, both or neither: the by-SOURCE plan's cell map and image -- the same weights once more, for the backward
 * product; a layer that will not be differentiated passes NULL) */
int spadot_gat_alpha(const float *s_src, const float *s_dst, const int *rowptr, const int *col, const int *cellq, int n_tgt,
                     int H, float *alpha, void *acell, const int *cellq_s, void *acell_s, void *stream);
int spadot_gat_aggregate(const void *x, int dtype, const void *acell, const int *plan_rows, const int *plan_sptr,
                         const int *plan_cols, int nb, int max_cols, int H, int C, int mode, const float *vec_a,
                         const float *vec_b, int act, const float *ds_src, const float *ds_dst, void *out,
                         const void *h_rows, float *att_part, int part_width, int pad_from, int pad_to, const float *dz,
                         const int *rowptr_t, const int *eid_t, float *ds_src_out, void *stream);
int spadot_gat_edge_dot(const void *g_out, const void *out, const void *h, int dtype, const int *plan_rows,
                        const int *plan_sptr, const int *plan_cols, const int *plan_cell, int nb, int max_cols, int H,
                        int C, int act, void *g_pre, float *dz, float *bias_part, int part_width, int part_col, void *stream);
/* (ds_dst has n_all >= n_tgt rows: the rows of nodes that are sources only are written as zeros) */
int spadot_gat_softmax_backward(const float *alpha, const float *s_src, const float *s_dst, const int *rowptr,
                                const int *col, const int *cellq_s, int n_tgt, int n_all, int H, float *dz, float *ds_dst,
                                void *acell_s, void *stream);
int spadot_gat_ds_src(const float *dz, const int *rowptr_t, const int *eid_t, int n, int H, float *ds_src, void *stream);

/* ---- dense map of a GAT layer on the matrix cores (csrc/gemm_bf16.hip) -------------------------------------------------
 * C [M x N] (bf16, row stride ldc) = A [M x K] (bf16, lda) . B^T with B stored [N x K] (bf16, ldb); fp32 accumulation.
 * Replaces the library GEMM under GATConv's `lin` (/root/reference/SpaDOT/model/encoder.py:41-58 -> torch_geometric
 * GATConv.lin) at the training shapes.  Requires N % 256 == 0, K % 32 == 0, 16-byte aligned pointers and strides that are
 * multiples of 8 elements; returns -22 otherwise (the caller then uses the library).  One 320 x 256 tile per workgroup. */
int spadot_gemm_tn_bf16(const void *A, int lda, const void *B, int ldb, void *C, int ldc, int M, int N, int K, void *stream);
/* The same kernel with B stored [K x N] (contraction index = row; transposed LDS reads for that operand): C = A . B, the
 * input gradient of a dense map (dx = g W with W the [N_out x K_in] weight image).  Same shape conditions. */
int spadot_gemm_nn_bf16(const void *A, int lda, const void *B, int ldb, void *C, int ldc, int M, int N, int K, void *stream);
/* ... with C[m][n] multiplied by `slope` wherever act_out[m][n] <= 0 (act_out [M x N] bf16, row stride ldm): the input gradient
 * of a dense map, dx = g W, times the LeakyReLU' of the activation that produced the map's INPUT (encoder.py:56-57) -- handed
 * to the layer below already masked, so that its edge backward neither reads its own output nor writes a masked copy. */
int spadot_gemm_nn_bf16_masked(const void *A, int lda, const void *B, int ldb, void *C, int ldc, int M, int N, int K,
                               const void *act_out, int ldm, double slope, void *stream);
/* spadot_gemm_tn_bf16 with the LAST `tail_row_tiles` row panels (320 rows each) cut into `slices` (2..8) slices of the
 * contraction; fp32 partial tiles in the caller's `workspace` (spadot_gemm_bf16_split_workspace floats, 16-byte aligned),
 * added in slice order and rounded once to bf16 by a second launch: bit-reproducible.  For a map whose grid is exactly one
 * round of workgroups and that shares the chip with another stream's long kernel (the second GAT layer beside the SVGP
 * branch's inverse: 40 of 256 compute units busy): 216 whole + 160 quarter tiles take 1.25 tile times instead of 2. */
long long spadot_gemm_bf16_split_workspace(int M, int N, int tail_row_tiles, int slices);
int spadot_gemm_tn_bf16_split(const void *A, int lda, const void *B, int ldb, void *C, int ldc, int M, int N, int K,
                              int tail_row_tiles, int slices, float *workspace, void *stream);


/* ---- weight gradient of a GAT layer's dense map on the matrix cores (csrc/gemm_wgrad_bf16.hip) ---------------------------
 * dW [N x K] (fp32, row stride ldw) = G^T X with G [M x N] (bf16, ldg) and X [M x >= K] (bf16, ldx; columns K .. the next
 * multiple of 256 must be readable -- the padded gene axis of the batch cache is).  256 x 256 output tiles x `slices`
 * slices of the M rows (0: one), partial tiles added in slice order by a second launch: bit-reproducible.
 * Requires N % 256 == 0, 16-byte aligned operands, strides % 8 == 0, operand images below 4 GiB; -22 otherwise.
 * The library keeps NO state: `workspace` (fp32, spadot_gemm_wgrad_bf16_workspace(M, N, K, slices) floats, 16-byte aligned;
 * may be NULL when that is 0) and `zero_row` (512 bytes of zeros, 16-byte aligned: the source of rows past M) belong to the
 * caller, so that calls on different streams, or captured into different graphs, never share scratch. */
long long spadot_gemm_wgrad_bf16_workspace(int M, int N, int K, int slices);
int spadot_gemm_wgrad_bf16(const void *G, int ldg, const void *X, int ldx, float *dW, int ldw, int M, int N, int K,
                           int slices, float *workspace, const void *zero_row, void *stream);
/* The same with the tile width along K chosen by the caller: tile_k = 256 (the entry points above) or 192 (256 x 192 tiles:
 * for shapes whose square-tile grid leaves the chip partly empty, e.g. 2048 x 3072 -- 96 square tiles x 2 slices = 192
 * workgroups, but 128 x 2 = 256 of these).  X columns up to the next multiple of tile_k must be readable. */
long long spadot_gemm_wgrad_bf16_workspace_tiled(int M, int N, int K, int slices, int tile_k);
int spadot_gemm_wgrad_bf16_tiled(const void *G, int ldg, const void *X, int ldx, float *dW, int ldw, int M, int N, int K,
                                 int slices, int tile_k, float *workspace, const void *zero_row, void *stream);

/* ---- hidden stages of the decoder as one launch each way (csrc/mlp_chain.hip) -------------------------------------------
 * /root/reference/SpaDOT/model/decoder.py:3-20: [Linear, LayerNorm, LeakyReLU] x n_layers on x [b, dims[0]] (fp32);
 * stage l maps dims[l] -> dims[l + 1].  forward keeps, per stage, a (linear output), y (stage output), mean, invstd.
 * backward: dy = gradient at the last stage's output; writes dx [b, dims[0]] (may be NULL) and `grads`, laid out per stage
 * as [dW (dout x din) | dbias (dout) | dgamma (dout) | dbeta (dout)] (spadot_mlp_chain_workspace gives that width and the
 * number of workspace rows; workspace = rows x width floats of scratch).  Fixed summation order.
 * supported: <= 4 stages, widths <= 256, input widths % 4 == 0, output widths % 8 == 0; all pointers 16-byte aligned. */
int spadot_mlp_chain_supported(int n_layers, const int *dims);
int spadot_mlp_chain_workspace(int b, int n_layers, const int *dims, int *n_rows, int *width);
int spadot_mlp_chain_forward(const float *x, int b, int n_layers, const int *dims, const float *const *W,
                             const float *const *bias, const float *const *gamma, const float *const *beta, const double *eps,
                             const double *slope, float *const *a, float *const *y, float *const *mean, float *const *invstd,
                             void *stream);
/* ... the same launch, also leaving a bf16 copy of the LAST stage's output [b, dims[n_layers]] in y_last_bf16 (may be NULL):
 * the operand of the output map's matrix-core GEMM (decoder.py:20), so that no cast launch sits between them. */
int spadot_mlp_chain_forward_bf16(const float *x, int b, int n_layers, const int *dims, const float *const *W,
                                  const float *const *bias, const float *const *gamma, const float *const *beta,
                                  const double *eps, const double *slope, float *const *a, float *const *y, float *const *mean,
                                  float *const *invstd, void *y_last_bf16, void *stream);
/* grads may be NULL: the per-workgroup partials stay in `workspace` and the caller adds them later (spadot_colsum).
 * spadot_mlp_chain_backward_add: dx = (the chain's input gradient) + dx_add [b, dims[0]] (may be NULL) -- a gradient that
 * reaches the chain's input by another path, added here instead of by a launch of its own. */
int spadot_mlp_chain_backward(const float *dy, const float *x, int b, int n_layers, const int *dims, const float *const *W,
                              const float *const *gamma, const double *slope, float *const *a, float *const *y,
                              float *const *mean, float *const *invstd, float *dx, float *workspace, float *grads, void *stream);
int spadot_mlp_chain_backward_add(const float *dy, const float *x, int b, int n_layers, const int *dims, const float *const *W,
                                  const float *const *gamma, const double *slope, float *const *a, float *const *y,
                                  float *const *mean, float *const *invstd, float *dx, const float *dx_add, float *workspace,
                                  float *grads, void *stream);

/* ---- reconstruction term on the output map's GEMM result (csrc/mlp_chain.hip) -------------------------------------------
 * out[0] = inv_scale * sum_{r,c} (y[r,c] - (o[r,c] + bias[c]))^2   (/root/reference/SpaDOT/model/SpaDOT.py:89 on the
 * decoder's output map, decoder.py:20), o = h W^T [b x G] fp32 without the bias: two launches (b <= 4096; scratch: >= 4096 doubles).  backward: g (bf16 [b x G]) = g1[0] * d out / d o and
 * dbias[c] = sum_r of the same values in fp32, fixed order. */
int spadot_bias_sqerr_forward(const float *o, const float *bias, const float *y, int b, int G, double inv_scale, double *scratch,
                              float *out, void *stream);
int spadot_bias_sqerr_backward(const float *g1, const float *o, const float *bias, const float *y, int b, int G,
                               double inv_scale, void *g_bf16, float *dbias, void *stream);

/* ---- GAT_fc on the bf16 rows of the last GAT layer (csrc/mlp_chain.hip) -------------------------------------------------
 * out [b x N] (fp32) = h [b x K] (bf16) . W^T [N x K] (fp32) + bias, N <= 32, K % 8 == 0: the (mu | logvar) head of
 * /root/reference/SpaDOT/model/encoder.py:59-61.  The forward is a cast + library GEMM; backward (fixed order): dh (bf16) and
 * per-8-row partials of dW, db in one launch, summed by a second. */
int spadot_headfc_backward(const float *g, const void *h_bf16, const float *W, int b, int K, int N, void *dh_bf16,
                           float *workspace /* ceil(b / 8) x (N K + N) floats */, float *grads /* [dW (N x K) | db (N)] */,
                           void *stream);

/* dst[t][r, 0:K[t]] = (bf16) src[t][r, 0:K[t]] for n <= 4 row-major matrices in one launch (fp32 weights -> their
 * compute-dtype images; dst rows have Kp[t] >= K[t] elements, the padding is not touched; K, Kp multiples of 4). */
int spadot_cast_rows_multi(const float *const *src, void *const *dst, const int *rows, const int *K, const int *Kp, int n,
                           void *stream);

/* ---------------------------------------------------------------- optimiser (one flat fp32 buffer)
 * sumsq[0] = sum g^2 over `count` gradients (deterministic two-stage reduction; scratch >= 2048 doubles). */
int spadot_grad_sumsq(const float *grad, long long count, double *scratch, float *sumsq, void *stream);
/* clip_grad_norm_(max_norm) folded into AdamW (torch semantics: decoupled weight decay, bias
 * correction, eps outside the sqrt):  coef = min(1, max_norm / (sqrt(sumsq) + 1e-6)); g = coef * grad;
 * p -= lr*wd*p; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr/(1-b1^t) * m / (sqrt(v/(1-b2^t)) + eps).
 * sumsq is read on the device (no host round trip). */
/* clip_grad_norm_ + AdamW with the step count on the device, TWO launches: the gradient's sum of squares (per-workgroup
 * partials in `scratch` (>= 2048 doubles), the last workgroup adds them in order, writes sumsq[0] and advances
 * step_dev[0]; `counter` is one unsigned that is 0 before the first call and left 0), then the update. */
int spadot_clip_adamw_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long long count, double lr,
                          double beta1, double beta2, double eps, double weight_decay, double max_norm, double *scratch,
                          float *sumsq, int *step_dev, unsigned *counter, const float *grad_scale_dev, void *stream);
/* grad_scale_dev (device scalar, may be NULL = 1): `grad` stands for grad_scale * grad -- the data-parallel step
 * all-reduces a SUM over replicas and passes 1 / (number of replicas that had a batch in this step), so that the clip
 * threshold and the update see the MEAN gradient, as a single replica would (spadot_amd/parallel.py). */
/* The same two-stage clip + AdamW, with the update ALSO keeping bf16 images of registered weight matrices current: image w
 * is the row-major [rows x Kp] bf16 copy (columns K .. Kp-1 are padding the kernel never writes) of the fp32 weight that
 * occupies flat elements [offset, offset + rows * K).  The GAT layers' dense maps read such images; casting them took a
 * launch at the head of every step.  Requires count % 4 == 0, 16-byte aligned buffers, K, Kp, offset % 4 == 0,
 * rows * K < 2^31, at most 8 images; -22 otherwise. */
typedef struct spadot_weight_image {
    long long offset;
    int rows, K, Kp, reserved;
    void *image;
} spadot_weight_image;
typedef struct spadot_weight_images {
    int n, reserved;
    spadot_weight_image w[8];
} spadot_weight_images;
int spadot_clip_adamw_images_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long long count, double lr,
                                 double beta1, double beta2, double eps, double weight_decay, double max_norm, double *scratch,
                                 float *sumsq, int *step_dev, const float *grad_scale_dev, const spadot_weight_images *images,
                                 void *stream);
/* The same update in two parts: the gradient norm + step count (once per step), then the element update of a RANGE
 * [offset, offset + count) of the flat buffers (offset, count multiples of 4; `images` may be NULL; image offsets refer to
 * the whole buffer).  A caller can update the parameters something is waiting for first and the rest afterwards: same
 * arithmetic per element, bit-identical to the one-call form (_train_utils.py:214-217). */
int spadot_grad_norm_step_dev(const float *grad, long long count, double *scratch, float *sumsq, int *step_dev, void *stream);
int spadot_adamw_range_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long long offset, long long count,
                           double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                           const float *sumsq, const int *step_dev, const float *grad_scale_dev, const spadot_weight_images *images,
                           void *stream);

int spadot_adamw_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                      const float *sumsq, long long count, double lr, double beta1, double beta2,
                      double eps, double weight_decay, double max_norm, int step, void *stream);

/* Same update with the step count kept ON THE DEVICE (step_dev[0] is incremented, then used for the bias
 * corrections): nothing in the launch depends on a host-side counter, so a captured hipGraph of a whole
 * training step can be replayed. */
int spadot_adamw_step_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                          const float *sumsq, long long count, double lr, double beta1, double beta2,
                          double eps, double weight_decay, double max_norm, int *step_dev, void *stream);

/* ---------------------------------------------------------------- preprocess stage (csrc/preprocess.hip)
 * SPARK-X gene statistics and the log-normalise + scale of the output (SpaDOT/utils/_utils.py:121-414,
 * _preprocess_utils.py:11-49).  Counts are fp32 in CSR (indptr [n+1], cidx, val: spots x genes) and CSC (colptr [G+1], ridx
 * sorted within each column, val: genes x spots), rows in output order: time point t owns rows [tp_off[t], tp_off[t+1]).
 * Every sum is fp64, owned by one wavefront in a fixed order (no atomics: bitwise repeatable).
 *
 * gene_detect:  cnt[t, g] = #{rows of t: x >= thr}, colsum[t, g] = sum of x over the rows of t              (CSC)
 * row_total:    total[r] = sum of x[r, g] over the genes with mask[t(r), g] != 0, rows tp_off[0] .. + nrows   (CSR)
 * sparkx_moments: per pair p = (pair_t, pair_g): mom[p, 24] = sum y, sum y^2, sum y * xt[rowmap[r], 0 .. 21]; xt [*, 22]
 *               fp64 centred kernel coordinates of the kept spots, rowmap[r] = its row or -1                  (CSC)
 * sparkx_pvals: per pair: stat[p, 11], pval[p, 11] (two-term chi^2_1 survival, trapezoid on `nodes` points; ylam = 0 -> 1),
 *               comb[p] (ACAT).  inv [T, 11, 4] = (X^T X)^-1, lam [T, 11, 2] its eigenvalues of X^T X (X^T X)^-1,
 *               nkeep[t] kept spots
 * lognorm_stats: v = log1p(x * target / total[r]); mean[t, j], std[t, j] (ddof 1, 0 -> 1) of column cols[j] over the rows
 *               of t                                                                                             (CSC)
 * scale_write:  out[(r - tp_off[0]) * S + colpos[g]] = clip((v - mean) / std) as fp32 (clip 0: none), dense rows
 *               tp_off[0] .. + nrows                                                                             (CSR) */
int spadot_pre_gene_detect(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int T, int G,
                           double thr, int *cnt, double *colsum, void *stream);
int spadot_pre_row_total(const long long *indptr, const int *cidx, const float *val, const int *tp_off, int T, int G,
                         const unsigned char *mask, int nrows, double *total, void *stream);
int spadot_sparkx_moments(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int P,
                          const int *pair_t, const int *pair_g, const int *rowmap, const double *xt, double *mom, void *stream);
int spadot_sparkx_pvals(const double *mom, int P, const int *pair_t, const int *nkeep, const double *inv, const double *lam,
                        int nodes, double *stat, double *pval, double *comb, void *stream);
int spadot_pre_lognorm_stats(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int T, int S,
                             const int *cols, const double *total, double target, double *mean, double *stdv, void *stream);
int spadot_pre_scale_write(const long long *indptr, const int *cidx, const float *val, const int *tp_off, int T, int S,
                           const int *colpos, const double *total, double target, const double *mean, const double *stdv,
                           double clip, int nrows, float *out, void *stream);

/* ---------------------------------------------------------------- SCTransform (csrc/sctransform.hip)
 * The per-gene work of SpaDOT/utils/sctransform (vst with method='poisson', theta.ml, Pearson residuals) on one time point t,
 * counts in the CSC layout above.  The N spots t keeps (non-zero total) are given as lu[k] (log10 total, row order), krow[k]
 * (their rows), and per row lur[r] (log10 total, 0 elsewhere) and rowmap[r] (k, or -1).  One wavefront per gene, fp64 sums in
 * a fixed order (bitwise repeatable).  pars[i] = (theta, b0, b1).
 *
 * sct_gene_stats:  out[i, 3] = sum log1p(y), sum y, sum (y - mean)^2 over the N spots, gene genes[i]
 * sct_fit:         per step-1 gene: Poisson IRLS of y ~ 1 + log_umi (tol, maxit), then theta.ml (limit, eps) on the fitted
 *                  mu of the last iteration; out[i, 8] = theta, b0, b1, fitted b0, fitted b1, iterations, theta iterations,
 *                  sum y
 * sct_resid_stats: r = (y - mu) / sqrt(mu + mu^2 / theta), mu = exp(b0 + b1 x); out[i, 3] = mean, variance (ddof 1) of
 *                  clip(r, +-clip_hi), mean of clip(r, +-clip_lo)
 * sct_resid_write: out[i * N + k] = clip(r, +-clip_lo) - center[i], fp64 dense
 * sct_polygamma:   psi[i], psi1[i] = digamma, trigamma of x[i] (the device functions sct_fit uses) */
int spadot_sct_gene_stats(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int t, int Gk,
                          const int *genes, int N, double *out, void *stream);
int spadot_sct_fit(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int t, int G1,
                   const int *genes, const double *lur, const double *lu, int N, double tol, int maxit, int limit, double eps,
                   double *out, void *stream);
int spadot_sct_resid_stats(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int t, int Gk,
                           const int *genes, const double *lur, const double *lu, int N, const double *pars, double clip_hi,
                           double clip_lo, double *out, void *stream);
int spadot_sct_resid_write(const long long *colptr, const int *ridx, const float *val, const int *tp_off, int t, int S,
                           const int *genes, const double *lur, const double *lu, const int *krow, const int *rowmap, int N,
                           const double *pars, const double *center, double clip_lo, double *out, void *stream);
int spadot_sct_polygamma(const double *x, int n, double *psi, double *psi1, void *stream);

/* ---------------------------------------------------------------- markers stage (csrc/markers.hip)
 * Per (time point, gene, domain) Wilcoxon rank-sum tests of v = float(log1p(x * target / total[r])), all spots of the time point
 * ranked together with average ranks, fp32 bit patterns defining ties: scipy.stats.mannwhitneyu(in, out, 'two-sided',
 * method='asymptotic', use_continuity=True).  Same CSC layout as the preprocess stage; labels[r] in 0 .. K-1 is the domain of
 * row r inside its time point, nk[t, k] the size of domain k.  Limits (return -7): K <= 32, nmax <= 2097151.
 *
 * mk_lognorm:  v[p] per stored entry p of the CSC arrays
 * mk_ranksum:  per (t, g): r2[t, g, K] int64 TWICE the rank sum of each domain, ties[t, g] int64 sum of t^3 - t over the tie
 *              runs (the zeros included), nnz_k[t, g, K] int32 entries with v > 0, vsum[t, g, K] fp64 sum of v (fixed order).
 *              Segments of up to spadot_mk_lds_capacity() entries are sorted in LDS, longer ones through `scratch`
 *              (spadot_mk_ranksum_scratch_bytes(T, G, nmax) bytes, nmax >= the spots of every time point)
 * mk_finish:   u1, score, pval [t, g, K] fp64; score 0 and p 1 where the variance is 0, a side is empty or U1 = n1 n2 / 2 */
int spadot_mk_lds_capacity(void);
long long spadot_mk_ranksum_scratch_bytes(int T, int G, int nmax);
int spadot_mk_lognorm(const int *ridx, const float *val, const double *total, long long nnz, double target, float *v,
                      void *stream);
int spadot_mk_ranksum(const long long *colptr, const int *ridx, const float *v, const int *tp_off, const int *labels,
                      const int *nk, int T, int G, int K, int nmax, void *scratch, long long scratch_bytes, long long *r2,
                      long long *ties, int *nnz_k, double *vsum, void *stream);
int spadot_mk_finish(const long long *r2, const long long *ties, const int *tp_off, const int *nk, int T, int G, int K,
                     double *u1, double *score, double *pval, void *stream);

/* ---------------------------------------------------------------- silhouette coefficients (csrc/silhouette.hip)
 * sklearn.metrics.silhouette_samples of P (data set, labeling) problems in one launch, fp64, no n x n matrix, no atomics (two
 * runs, and a problem alone or in a batch, give the same bits).  x: [rows, d] fp64, the data sets one after the other.
 * prob[p, 4] int64: first row of the problem's set in x, offset of the problem in order / the outputs, n (points), K (label
 * values).  order[offset + j]: the set's row at position j of the problem's points sorted by (label, row); coff[p, 33] int32:
 * cluster k holds the sorted positions coff[p, k] .. coff[p, k + 1] (coff[p, K] = n; an empty cluster is skipped).
 * With dist(i, j) = sqrt(sum_c (x_ic - x_jc)^2) and S_i(k) the sum of dist(i, j) over cluster k, per row i of cluster c:
 *   a = S_i(c) / (n_c - 1) (0 if n_c = 1),  b = min over non-empty k != c of S_i(k) / n_k,  nearest = that k (first minimum),
 *   s = (b - a) / max(a, b), 0 if n_c = 1 or max(a, b) = 0;  a single non-empty cluster leaves b = inf, nearest = -1, s = NaN.
 * Outputs a, b, s fp64 and nearest int32 at [offset + row], the caller's row order.
 * Limits (return -7, nothing launched): 1 <= d <= 32, 2 <= k_min <= k_max <= 32 (the range of the K column), P <= 65535
 * (gridDim.y), n_max <= 2147483391 (int32 positions; n_max >= the n of every problem sizes gridDim.x). */
int spadot_silhouette(const double *x, int d, int P, const long long *prob, const int *order, const int *coff, int n_max,
                      int k_min, int k_max, double *a, double *b, int *nearest, double *s, void *stream);

/* ---------------------------------------------------------------- Gaussian mixtures (csrc/gmm.hip)
 * EM for full-covariance Gaussian mixtures of P (data set, component count) problems at once, pinned to sklearn 1.7's
 * GaussianMixture(covariance_type="full"): fp64, no atomics, every sum in a fixed order that depends on the problem alone (a
 * problem gives the same bits alone, in any batch, run after run, for any grouping of iterations into calls).
 * x: [rows, d] fp64, the CENTRED data sets one after the other.  prob[p, 4] int64: first row of the problem's set in x, first row of
 * the problem in the per-point arrays (resp_init, norm, labels, resp, lp), n (points), K (components, 1 <= K <= K_max).
 * With DP = 4 ceil(d / 4), T = DP (DP + 1) / 2, S = DP + T + 2, M = 1 + DP + T, nblk = ceil(n_max / 256):
 *   par  [P, K_max, S]   mu_k (zero padding), then P_k = L_k^-T (Sigma_k = L_k L_k^T) packed by columns (P[a, j], a <= j, at
 *                        j (j + 1) / 2 + a; identity padding), then sum_j log P_k[j, j], then log w_k -- stored per problem as the K_max means
 *                        [K_max, DP] first and the K_max blocks of T + 2 doubles after them
 *   w    [P, K_max]      w_k = nk / n;   cov [P, K_max, d, d]  Sigma_k;   mom [P, K_max, M] (may be null): sum r, sum r u_a,
 *                        sum r u_a u_b (a <= b, packed like P) of the last M-step, u = x - the mean
 *                        the iteration started from (resp_init: the raw moments, u = x, of its first pass)
 *   part                 work space of P * nblk * (K_max * M + 1) doubles
 *   done, n_iter [P] int32, lb [P] fp64: the stop flag, the iteration count and the lower bound (mean log-likelihood per
 *                        point of the last E-step) of every problem; the caller starts them at 0, 0 and -inf
 * spadot_gmm_em_step: if resp_init ([sum n, K_max] fp64, rows at the problem's offset) is not null, first one M-step from those
 * responsibilities (nk = sum r + 10 eps, mu = sum r x / nk, Sigma = sum r (x - mu)(x - mu)^T / nk + reg_covar I, w = nk / n),
 * in two passes over the points: raw moments for the means, then moments about those means.  Then
 * `steps` iterations of E-step (lp_ik = (-(d log 2 pi + |(x_i - mu_k) P_k|^2) / 2 + log det P_k) + log w_k, norm_i =
 * logsumexp_k lp_ik, r_ik = exp(lp_ik - norm_i)), M-step, and the stop rule: lb = mean norm, n_iter += 1, done = |lb - lb_prev|
 * < tol (the M-step of the stopping iteration has been applied).  A problem whose done flag is set is left alone entirely.
 * spadot_gmm_estep: one E-step with the parameters in par: norm [sum n], and where not null labels [sum n] int32 (argmax_k of
 * lp - norm, first maximum), resp and lp [sum n, K_max].
 * Return -22 for null or empty arguments and -7, before any launch, outside the limits: 1 <= d <= 32, 1 <= K_max <= 32,
 * P <= 65535, n_max <= 2147483391 and 8 (max(K_max S, (K_max + 256) DP) + 256 (K_max | 1)) + 2048 <= 163840 bytes of LDS
 * (d <= 24: K_max <= 32; d <= 28: K_max <= 29; d <= 32: K_max <= 24). */
int spadot_gmm_em_step(const double *x, int d, int P, const long long *prob, int K_max, int n_max, double *par, double *w,
                       double *cov, double *mom, const double *resp_init, double reg_covar, double tol, int steps, double *part,
                       int *done, int *n_iter, double *lb, void *stream);
int spadot_gmm_estep(const double *x, int d, int P, const long long *prob, int K_max, int n_max, const double *par, double *norm,
                     int *labels, double *resp, double *lp, void *stream);

/* ---------------------------------------------------------------- neighbourhood enrichment (csrc/nhood.hip)
 * Count matrices C[a, b] = #{edges i -> j : lab[i] = a, lab[j] = b} of many (graph, labeling) problems in ONE launch: integers
 * only, integer LDS atomics, no global atomics (a problem gives the same integers alone, in any batch, run after run).
 * src, dst: int32 edge ends of the G graphs back to back (no self loops expected; duplicates are counted); labels: uint8, per
 * graph either L labelings [L, n] (GIVEN) or one base labeling [n] (PERM).  desc [G, 12] int64, once in host memory (checked
 * here) and once on the device (read by the kernel), per graph:
 *   0 first edge   1 n   2 E   3 K   4 first label byte   5 L (labelings, or permutations)   6 first permutation index p0
 *   (-1: GIVEN)   7 graph id g of the permutation keys   8 first output matrix (the sum of L over the graphs before; checked)
 *   9 seed   10 the smallest and 11 the largest edge end of the graph (ignored where E = 0)
 * PERM labeling l is base[pi(i)] with pi the permutation of (seed, g, p0 + l, n): a six-round balanced Feistel network on b
 * bits (b = ceil(log2 n) rounded up to even, at least 2) with round function mix32(R ^ key_r) & mask, keys from splitmix64 of
 * seed ^ (g << 32) ^ p, cycle-walked into 0 .. n-1 (tests/nhood_ref.py).
 * out: int32 [sum L, K_max, K_max], matrix item0 + l of graph g in its top-left K x K corner, written completely (zeros too).
 * A graph keeps its labeling in LDS where 16 K^2 + (n rounded up to 16) <= lds_limit (at most 163840; larger values mean
 * 163840) and reads its labels from global memory otherwise.
 * Return -22 for null or inconsistent arguments and -7, before any launch, outside the limits: 1 <= K <= K_max <= 32,
 * 1 <= n <= 2147483647, E <= 2147483647, every edge end in 0 .. n-1, sum L <= 2147483647 (gridDim.x), p0 + L <= 2^32,
 * g <= 2147483647.  A label >= K is the caller's to refuse (its edges are not counted). */
int spadot_nhood_counts(const int *src, const int *dst, const unsigned char *labels, const long long *desc_host,
                        const long long *desc_dev, int G, int K_max, long long lds_limit, int *out, void *stream);

/* ---------------------------------------------------------------- territories (csrc/territories.hip)
 * The connected pieces of every domain of many (graph, labeling) problems in ONE launch, one workgroup per (problem,
 * labeling).  A territory is a connected component of the subgraph that keeps only the edges whose two ends carry the same
 * label (direction ignored; duplicates, two-way edges and self loops change nothing); its id is the smallest node it contains.
 * Integers only: integer min / add / max atomics inside one workgroup, none across workgroups (a problem gives the same
 * integers alone, in any batch, on either path, run after run; tests/territories_ref.py).
 * src, dst, labels and the columns 0 .. 11 of desc [G, 14] int64 (once on the host, checked here; once on the device) are those
 * of spadot_nhood_counts, the permuted labelings included.  Further columns:
 *   12 first node of the problem in ids / sizes (-1: not asked for; otherwise the n ids and sizes of its FIRST labeling are written)
 *   13 first int of the problem's slabs in scratch (checked: the sum of the slabs of the problems before; ignored on the LDS path)
 * out: int64 [sum L, K_max, 4] per label value (count of territories, size of the largest, territories of one node, sum of
 * size^2), zeros for a label value without nodes or >= K; written completely.  ids, sizes: int32 [n_ids] (may be null when no
 * problem asks).  status: int32 [sum L, 2] = (0, or 1 when the round cap n + 1 was reached: the other outputs of that item are
 * then meaningless; rounds run).
 * A problem keeps its parents, sizes and labels in LDS where 1024 + 8 n + (n rounded up to 16) <= lds_limit (at most 163840;
 * larger values mean 163840: n <= 18 090) and otherwise in a slab of 2 n + ceil(n / 4) ints per labeling of `scratch` (int32
 * [n_scratch]; may be null when every problem fits); the work stays inside the workgroup's own slab.
 * Return -22 for null or inconsistent arguments and -7, before any launch, outside the limits of spadot_nhood_counts. */
int spadot_territory_counts(const int *src, const int *dst, const unsigned char *labels, const long long *desc_host,
                            const long long *desc_dev, int G, int K_max, long long lds_limit, long long *out, int *ids,
                            int *sizes, long long n_ids, int *status, int *scratch, long long n_scratch, void *stream);

/* ---------------------------------------------------------------- hop distances (csrc/hops.hip)
 * Level-synchronous breadth-first search from up to 32 source sets at once (one bit of a 32-bit mask per set) of many
 * (graph, labeling) problems in ONE launch, one workgroup per item.  Direction is ignored; duplicates, two-way edges and self
 * loops change nothing.  Integers only: integer or / add atomics inside one workgroup, none across workgroups, and two mask
 * arrays so that a round reads only what the round before left (a problem gives the same integers, the round counts
 * included, alone, in any batch, on either path, run after run; tests/hops_ref.py).
 * src, dst, labels and the columns 0 .. 11 of desc [G, 15] int64 (once on the host, checked here; once on the device) are those
 * of spadot_nhood_counts, the permuted labelings included.  Further columns:
 *   12 first int of the problem in hops (-1: not asked for; otherwise the [n, K] hop distances of its FIRST labeling are written)
 *   13 first int of the problem's slabs in scratch (checked: the sum of the slabs of the problems before; ignored on the LDS path)
 *   14 kind: 0 label items -- item l of the problem is labeling l, set a = the nodes that carry label a, the class of a node its
 *      label; 1 source items -- p0 = -1, ONE explicit labeling of n labels, L = ceil(n / 32), column 12 = -1 and K_max = 32:
 *      item l has the sets {32 l + j}, j = 0 .. 31 (those past n empty), the class of a node is its label
 * out: int64 [sum L, K_max, K_max, 3] per (set, class): the nodes of the class at a distance >= 1 of the set (reached), the
 * sum of those distances (sumdist), those at distance 1 (adjacent); zeros for an empty set and outside the sets and classes of
 * the item; written completely.  ecc: int32 [sum L, K_max] the largest distance from a set (0: nothing reached).  hops: int32
 * [n_hops] (may be null when no problem asks): 0 for the members of a set, the distance for the nodes it reaches, -1 for the
 * others.  status: int32 [sum L, 2] = (0, or 1 when the round cap n + 1 was reached: the other outputs of that item are then
 * meaningless; rounds run: the largest distance + 1).
 * A problem keeps its two mask arrays and its classes in LDS where 16640 + 8 n + (n rounded up to 16) <= lds_limit (at most
 * 163840; larger values mean 163840: n <= 16 354) and otherwise in a slab of 2 n + ceil(n / 4) ints per item of `scratch`
 * (int32 [n_scratch]; may be null when every problem fits); the work stays inside the workgroup's own slab.
 * Return -22 for null or inconsistent arguments and -7, before any launch, outside the limits of spadot_nhood_counts. */
int spadot_hop_sums(const int *src, const int *dst, const unsigned char *labels, const long long *desc_host,
                    const long long *desc_dev, int G, int K_max, long long lds_limit, long long *out, int *ecc, int *hops,
                    long long n_hops, int *status, unsigned *scratch, long long n_scratch, void *stream);

/* ---------------------------------------------------------------- co-occurrence by distance (csrc/cooccur.hip)
 * N[a, b, t] = #{ordered pairs (i, j), i != j : lab[i] = a, lab[j] = b, d2(i, j) <= r2[t]} of P (spot set, labeling,
 * thresholds) problems in ONE counting launch, with d2 = fl(fl(dx dx) + fl(dy dy)), dx = x_i - x_j, dy = y_i - y_j: five
 * correctly rounded fp64 operations, no fused multiply-add (what dx*dx + dy*dy <= r2 does in numpy; tests/cooccur_ref.py).  Two
 * spots at the same coordinates are a pair at distance 0.  Integers only: register counters, 64-bit integer LDS and global adds
 * onto the output, which the call zeroes itself (a problem gives the same integers alone, in any batch, run after run, under a
 * larger K_max or B_max).  No n x n array, no floating-point sum.
 * xy: fp64 [sum n, 2], per problem its spots ORDERED BY (label, index), the problems back to back.  desc [P, 40] int64, once in
 * host memory (checked here) and once on the device (read by the kernel), per problem:
 *   0 first spot in xy (the sum of n over the problems before; checked)   1 n   2 K   3 B
 *   4 .. 4 + K   the cluster offsets: label k holds the sorted positions desc[4 + k] .. desc[5 + k] (desc[4] = 0, desc[4 + K] = n)
 * r2 [P, BP] fp64 with BP = B_max rounded up to a multiple of 16, once in host memory (checked here) and once on the device: the
 * problem's B squared thresholds, strictly increasing, finite and >= 0, then -1.0 in every padded place (no d2 is <= -1).
 * out: int64 [P, K_max, K_max, B_max], problem p in its corner [K, K, B], written completely (zeros too).
 * Return -22 for null or inconsistent arguments and -7, before any launch, outside the limits: 1 <= K <= K_max <= 32,
 * 1 <= B <= B_max <= 64, 1 <= n <= 2147483391 (int32 positions of a 256-wide tile), P <= 65535 (gridDim.y), a threshold that is
 * negative, not finite or not above the one before.  Non-finite coordinates and labels outside 0 .. K-1 are the caller's to
 * refuse (the labels never reach the library: the offsets do). */
int spadot_cooccur_counts(const double *xy, const long long *desc_host, const long long *desc_dev, const double *r2_host,
                          const double *r2_dev, int P, int K_max, int B_max, long long *out, void *stream);

/* The random-labelling null of the counts above (restated in numpy in tests/cooccur_null_ref.py): the same
 * counts of the observed labeling and of relabelings of every problem in ONE launch.  Pattern 0 is the observed labeling;
 * pattern s >= 1 leaves the labels on the sorted positions and gives position j the coordinates xy[pi^-1(j)], pi the
 * permutation of spadot_nhood_counts with (seed, g, s - 1, n) -- the convention of spadot_ripley_counts under null "labels".
 * pi^-1 is evaluated per element while the spots are read: no permuted copy of xy and no table of pi exists.  The domain
 * sizes are those of the observed labeling in every pattern.
 * xy, desc, r2 as for spadot_cooccur_counts, with the problem number g of a problem in column 37 of its descriptor (K <= 32
 * leaves the columns 37 .. 39 free).  The call counts pattern 0 where observed = 1, then the patterns 1 + first ..
 * first + n_perms.
 * out: int64 [P, observed + n_perms, K_max, K_max, B_max], written completely (zeros too).  Integers only: a problem gives the
 * same integers alone, in any batch, run after run, under a larger K_max or B_max and under any split of the relabelings
 * into calls with `first` advanced.
 * Return as spadot_cooccur_counts, and -22 for observed not 0 or 1, -7 for observed + n_perms outside 1 .. 65535 (gridDim.y;
 * the problems are gridDim.z), first < 0, first + n_perms > 2^31, or g outside 0 .. 2147483647. */
int spadot_cooccur_null(const double *xy, const long long *desc_host, const long long *desc_dev, const double *r2_host,
                        const double *r2_dev, int P, int K_max, int B_max, int observed, long long first, int n_perms,
                        long long seed, long long *out, void *stream);

/* ---------------------------------------------------------------- Ripley's L, G and F per domain (csrc/ripley.hip)
 * The integers behind Ripley's functions of every (problem, domain, pattern) of a call in ONE counting launch; the definition
 * is restated in numpy in tests/ripley_ref.py.  Domain c of a problem holds n_c spots and 1 + S patterns of n_c points each:
 * pattern 0 its own spots; pattern s >= 1, under null 0 ("labels"), the spots that receive label c under the permutation of
 * spadot_nhood_counts with (seed, g, s - 1, n) acting on the sorted positions (point i is xy[pi^-1(off_c + i)]), under null 1
 * ("csr") the points 0 .. n_c - 1 of stream 1 + c S + s - 1 generated in the window.  Stream 0 holds the M probe points.  Per
 * pattern and threshold t, with d2 the unfused squared distance of spadot_cooccur_counts:
 *   stat 0  Lc = #{ordered pairs i != j of the pattern : d2 <= r2[t]}
 *   stat 1  Gc = #{points of the pattern whose nearest other point has d2 <= r2[t]}   (a lone point is never counted)
 *   stat 2  Fc = #{probe points whose nearest point of the pattern has d2 <= r2[t]}
 * A generated point is a pure function of (seed, g, stream, i): key = splitmix(seed ^ (g << 32) ^ stream) ^ 0x52504C5953494D31,
 * w_j = splitmix(key + (3 i + j) 0x9E3779B97F4A7C15), u_j = (w_j >> 11) 2^-53; the triangle is the first k with
 * fl(u_0 cum[V - 3]) < cum[k] (the last where there is none); where u_1 + u_2 > 1 both are replaced by 1 - u; the point is
 * (A + u_1 (B - A)) + u_2 (C - A) with (A, B, C) = (V0, V_{k+1}, V_{k+2}), every operation rounded once.
 * xy: fp64 [sum n, 2], per problem its spots ORDERED BY (label, index), the problems back to back.  desc [P, 48] int64, once in
 * host memory (checked here) and once on the device (read by the kernel), per problem:
 *   0 first spot in xy (checked)   1 n   2 K   3 B   4 S   5 M   6 null (0 labels, 1 csr)   7 modes (1 L | 2 G | 4 F)
 *   8 g   9 first row of its window in hull / cum   10 V, the window's vertices   11 0
 *   12 .. 12 + K   the cluster offsets (desc[12] = 0, desc[12 + K] = n)
 * r2 [P, BP] fp64 as for spadot_cooccur_counts (padded with -1.0), on the host and on the device.  hull [hull_rows, 2] fp64: the
 * windows' vertices, counter-clockwise; cum [hull_rows] fp64: beside the first V - 2 vertices of a window the cumulative areas
 * of its fan triangles (V0, V_{k+1}, V_{k+2}) (a sliver whose area rounding makes negative counts 0: cum never descends), then
 * two places that are not read; both on the host and on the device.
 * out: int64 [P, K_max, 1 + S_max, 3, B_max], problem p in its corner [K, 1 + S, 3, B], written completely (zeros too; a
 * statistic outside `modes` stays zero).  Integers only reach memory: a problem gives the same integers alone, in any batch,
 * run after run, under a larger K_max, S_max or B_max.
 * Return -22 for null or inconsistent arguments (a window that turns right, goes round more than once, has fewer than 3
 * vertices, non-finite coordinates or descending areas among them) and -7, before any launch, outside the limits:
 * 1 <= K <= K_max <= 32, 1 <= B <= B_max <= 64, 1 <= S <= S_max <= 9999, 1 <= M <= 1048576, V <= 256, 1 <= n <= 2147483391,
 * P <= 65535 (gridDim.z), K (1 + S) <= 65535 (gridDim.y), thresholds as for spadot_cooccur_counts.  Non-finite coordinates
 * are the caller's to refuse. */
int spadot_ripley_counts(const double *xy, const long long *desc_host, const long long *desc_dev, const double *r2_host,
                         const double *r2_dev, const double *hull_host, const double *hull_dev, const double *cum_host,
                         const double *cum_dev, long long hull_rows, int P, int K_max, int S_max, int B_max, long long seed,
                         long long *out, void *stream);

/* The points 0 .. count - 1 of stream `stream_id` of problem g under seed, generated in one window by the device function that
 * spadot_ripley_counts uses: hull [V, 2] and cum [V - 2] on the host (checked as above) and on the device, out fp64 [count, 2].
 * Return -22 / -7 as above; 1 <= count <= 2147483391, 0 <= stream_id <= 1 + 32 * 9999. */
int spadot_ripley_points(const double *hull_host, const double *hull_dev, const double *cum_host, const double *cum_dev, int V,
                         long long seed, long long g, long long stream_id, long long count, double *out, void *stream);

/* ---------------------------------------------------------------- spatial autocorrelation (csrc/autocorr.hip)
 * The two edge sums behind Moran's I and Geary's C of every (time point, gene, labeling) in ONE launch.  Time point t is a
 * directed edge list over its n spots (src, dst: int32 edge ends of the T time points back to back; no self loops expected,
 * duplicates count) and the rows row0 .. row0 + n - 1 of a CSC matrix (colptr [G + 1] int64, ridx [nnz] int32 ascending inside
 * a column, v [nnz] fp32: the layout of the preprocess, markers and trends stages).  Gene g of time point t has the value v of
 * its stored entries and 0 elsewhere, and the centre c = centre[t * G + g] (fp64 [T, G], absolute gene index).  Labeling 0 (only
 * with observed = 1) is the identity; the P labelings after it give spot i the value of spot pi_p(i), p = first .. first + P - 1,
 * with pi_p the permutation of spadot_nhood_counts under (seed, graph id, p, n).  With x the labeled values promoted to fp64:
 *   N[t, g - g0, l] = sum over edges i -> j of (x_i - c)(x_j - c)     D[t, g - g0, l] = sum over edges of (x_i - x_j)^2
 * for the genes g0 .. g0 + ng - 1, fp64 [T, ng, observed + P], written completely.  One fp64 subtraction per centring and per
 * difference, one fma per term; thread u of a workgroup adds the edges u, u + threads, ... in that order, the partial sums are
 * added by shuffles inside the wavefront and across the wavefronts in wavefront order: no atomics, and the bits of a sum depend
 * on the time point's edges, the gene's values, c, the labeling and `threads` alone (two runs, a gene alone, another batch,
 * either path, either gs: the same bits).
 * desc [T, 7] int64, once in host memory (checked here) and once on the device (read by the kernel), per time point:
 *   0 first edge   1 n   2 E   3 row0   4 graph id of the permutation keys   5 the smallest and 6 the largest edge end (ignored
 *   where E = 0)
 * ridx_lo, ridx_hi: the smallest and the largest row index in ridx (ignored where nnz = 0).
 * A workgroup handles one (time point, labeling, group of gs consecutive genes) and keeps a dense fp32 image [n, gs] of its
 * labeled values in LDS where 2048 + 4 gs n <= lds_limit (at most 163840; larger values mean 163840); otherwise the image lives
 * in scratch, fp32 [items, slab] with items = T (observed + P) ceil(ng / gs) and slab = the largest such gs n rounded up to a
 * multiple of 4 (scratch_floats: how many floats scratch holds; scratch may be null where every image fits).
 * threads: 256, 512 or 1024 (0: the default, 1024); gs: 2 or 4 (0: the default, 2).
 * Return -22 for null, negative or inconsistent arguments (a scratch buffer that is too small among them) and -7, before any
 * launch, outside the limits: 1 <= n <= 2147483647, E <= 2147483647, nnz <= 2147483647, every edge end in 0 .. n-1, every row
 * index in 0 .. max(row0 + n) - 1, g0 + ng <= G, first + P <= 2^32, graph id <= 2147483647, items <= 2147483647 (gridDim.x),
 * threads and gs as above. */
int spadot_autocorr_sums(const int *src, const int *dst, const long long *colptr, const int *ridx, const float *v, long long nnz,
                         long long ridx_lo, long long ridx_hi, const double *centre, const long long *desc_host,
                         const long long *desc_dev, int T, int G, int g0, int ng, int observed, long long first, long long P,
                         long long seed, long long lds_limit, float *scratch, long long scratch_floats, int threads, int gs,
                         double *N, double *D, void *stream);

/* ---------------------------------------------------------------- ligand-receptor test (csrc/ligrec.hip)
 * spadot_ligrec_sums: the per-domain expression sums of selected genes under the identity labeling and / or a run of
 * permutations, for all time points in ONE launch.  Time point t is the rows row0 .. row0 + n - 1 of a CSC matrix (colptr
 * [G + 1] int64, ridx [nnz] int32 ascending inside a column, v [nnz] fp32: the layout of the preprocess, markers and trends
 * stages) and labels[row0 .. row0 + n - 1], one byte per row in 0 .. K-1 (label_hi: the largest byte in labels).  Labeling 0
 * (only with observed = 1) is the label itself; the P labelings after it give spot i the label of spot pi_p(i), p = first ..
 * first + P - 1, with pi_p the permutation of spadot_nhood_counts under (seed, graph id, p, n).  For the selected genes
 * genes[0 .. ng-1] (int32, any order, repeats allowed; gene_lo, gene_hi: the smallest and the largest), with v promoted to fp64:
 *   S[t, l, j, k] = sum of v over the stored entries of gene genes[j] in time point t whose row has label k under labeling l
 * fp64 [T, observed + P, ng, K], written completely, and with observed = 1
 *   cnt[t, j, k]  = the number of those entries with v > 0 under labeling 0                       int32 [T, ng, K].
 * One workgroup per (time point, labeling, chunk of gc selected genes); a wavefront takes a gene at a time, lane u adds the
 * entries u, u + 64, ... of the gene's segment in ascending order, the 64 lane sums are added by shuffles at offsets 32, 16,
 * .. 1: no atomics, and the bits of a sum depend on the segment and the labels of its rows alone (two runs, a gene alone, any
 * batch, any gc, either thread count, either path: the same bits).
 * desc [T, 3] int64, once in host memory (checked here) and once on the device (read by the kernel), per time point:
 *   0 n   1 row0   2 graph id of the permutation keys
 * ridx_lo, ridx_hi: the smallest and the largest row index in ridx (ignored where nnz = 0).
 * A workgroup keeps its accumulators in LDS (512 K threads / 64 bytes) and, where 512 K threads / 64 + n rounded up to 16 <=
 * lds_limit (at most 163840; larger values mean 163840), the n label bytes of its labeling beside them; otherwise it evaluates
 * pi_p per stored entry and reads the labels from global memory.
 * threads: 256 or 512 (0: the default, 512); gc >= 1 (0: the default, 128).
 * Return -22 for null, negative or inconsistent arguments (no labeling at all among them) and -7, before any launch, outside
 * the limits: 1 <= K <= 32, label_hi < K, 1 <= n <= 2147483647, nnz <= 2147483647, every row index in 0 .. max(row0 + n) - 1,
 * every selected gene in 0 .. G-1, first + P <= 2^32, graph id <= 2147483647, T (observed + P) ceil(ng / gc) <= 2147483647
 * (gridDim.x), threads as above. */
int spadot_ligrec_sums(const long long *colptr, const int *ridx, const float *v, long long nnz, long long ridx_lo,
                       long long ridx_hi, const unsigned char *labels, int label_hi, const long long *desc_host,
                       const long long *desc_dev, int T, int G, int K, const int *genes, int ng, int gene_lo, int gene_hi,
                       int observed, long long first, long long P, long long seed, long long lds_limit, int threads, int gc,
                       double *S, int *cnt, void *stream);

/* spadot_ligrec_count: the comparisons behind the p-values, one launch.  S0 fp64 [T, ns, K]: the sums of labeling 0; S fp64
 * [T, L, ns, K]: the sums of a run of L labelings, of which the first `skip` (0 or 1: the observed one) are not compared; wk
 * fp64 [T, K]: 1 / n_k (0 for an empty domain); pairs int32 [M, 2]: (source, target) as positions in the ns selected genes
 * (pair_lo, pair_hi: the smallest and the largest); mask uint8 [T, M, K, K]: the cells to test.  With
 *   stat_l(m, a, b) = 0.5 * (S[t, l, src_m, a] * wk[t, a] + S[t, l, tgt_m, b] * wk[t, b])
 * (two products and one sum, each rounded once: no fused multiply-add), every masked cell adds #{l >= skip : stat_l >= stat_0}
 * to ge[t, m, a, b] (int32 [T, M, K, K]; the caller zeroes it; several runs accumulate exactly).  One workgroup per (time
 * point, interaction), one thread per cell.
 * Return -22 for null or inconsistent arguments and -7 outside the limits: K <= 32, T M <= 2147483647, pairs inside 0 .. ns-1. */
int spadot_ligrec_count(const double *S0, const double *S, const double *wk, const int *pairs, int pair_lo, int pair_hi,
                        const unsigned char *mask, int T, int M, int ns, int K, long long L, int skip, int *ge, void *stream);

/* ---------------------------------------------------------------- local Moran's I (csrc/localmoran.hip)
 * The neighbour sums behind local Moran's I of every (time point, selected gene, spot) and their comparison with the sums under
 * conditional permutations, in ONE launch.  Time point t is a CSR over its n spots (rowptr: int32 [n + 1] ascending from 0 to E,
 * the T arrays back to back; col: int32 [E] out-neighbours in row order, back to back; no self loops expected, duplicates count)
 * and the rows row0 .. row0 + n - 1 of a CSC matrix (colptr [G + 1] int64, ridx [nnz] int32 ascending inside a column, v [nnz]
 * fp32).  Gene g of time point t has the value v of its stored entries and 0 elsewhere, and the centre c = centre[t * G + g]
 * (fp64 [T, G], absolute gene index).  With x the shown values promoted to fp64, the neighbour sum of spot i is
 *   lag_i = ((0 + (x_j1 - c)) + (x_j2 - c)) + ...      over the row of i in row order (subtractions and additions only).
 * Observed: x = v.  Permutation p = first .. first + P - 1 shows x_j = v[pi_p(j)], pi_p the permutation of spadot_nhood_counts
 * under (seed, graph id, p, n), except that while spot i is evaluated the neighbour j* = pi_p^-1(i) shows v[pi_p(i)].  For the
 * selected genes genes[0 .. ng-1] (int32, any order, repeats allowed; gene_lo, gene_hi: the smallest and the largest) and with
 * time point t's spot i at column row0 + i of `rows` columns:
 *   lag[j, row0 + i] = the observed sum (fp64 [ng, rows], written for the spots of the time points)
 *   ge[j, row0 + i] += #{p : lag^p >= lag^0}     le[j, row0 + i] += #{p : lag^p <= lag^0}      (int32 [ng, rows])
 * ge and le are ADDED to with integer atomics (exact in any order): the caller zeroes them, and several runs over disjoint
 * permutations accumulate.  The bits of lag and the integers depend on the row, the gene's values, c and the permutations alone
 * (two runs, a gene alone, another batch, any threads, gs, perm_chunk, either path: the same).
 * desc [T, 8] int64, once in host memory (checked here) and once on the device (read by the kernel), per time point:
 *   0 first entry of col   1 n   2 E   3 row0   4 graph id of the permutation keys   5 first entry of rowptr   6 the smallest
 *   and 7 the largest entry of col (ignored where E = 0)
 * ridx_lo, ridx_hi: the smallest and the largest row index in ridx (ignored where nnz = 0).
 * A workgroup handles one (time point, chunk of perm_chunk permutations, group of gs selected genes): the identity first, then
 * its permutations.  It keeps a dense fp32 image [n, gs] of the shown values in LDS where 256 + 4 gs n <= lds_limit (at most
 * 163840; larger values mean 163840), otherwise in scratch.  The observed sums and the counters of its spots live in scratch:
 * bytes [items, stride] with items = T ceil(P / perm_chunk) ceil(ng / gs) and stride = 16 gs max n + 4 slab, slab = the largest
 * gs n of the time points whose image does not fit, rounded up to a multiple of 4 (0 if all fit); scratch_bytes: its size.
 * threads: 256, 512 or 1024 (0: the default, 1024); gs: 2 or 4 (0: the default, 4); perm_chunk >= 1 (0: the default, 128).
 * Return -22 for null, negative or inconsistent arguments (a scratch buffer that is too small, rows < max(row0 + n) among them)
 * and -7, before any launch, outside the limits: P >= 1, 1 <= n <= 2147483647, E <= 2147483647, nnz <= 2147483647, every entry of
 * col in 0 .. n-1, every row index in 0 .. max(row0 + n) - 1, every selected gene in 0 .. G-1, first + P <= 2^32, graph id <=
 * 2147483647, items <= 2147483647 (gridDim.x), threads and gs as above.  That rowptr ascends from 0 to E is the caller's to
 * refuse (the kernel clamps what it reads). */
int spadot_local_lag(const int *rowptr, const int *col, const long long *colptr, const int *ridx, const float *v, long long nnz,
                     long long ridx_lo, long long ridx_hi, const double *centre, const long long *desc_host,
                     const long long *desc_dev, int T, int G, const int *genes, int ng, int gene_lo, int gene_hi, long long first,
                     long long P, long long seed, long long lds_limit, void *scratch, long long scratch_bytes, int threads, int gs,
                     long long perm_chunk, long long rows, double *lag, int *ge, int *le, void *stream);

/* ---------------------------------------------------------------- bivariate Moran's I (csrc/crossmoran.hip)
 * The cross sums of every pair of selected genes of every time point, observed and under relabelings of the spots.  Both entries
 * work on two dense fp64 images Z and Y [zrows, GP], GP = ng rounded up to a multiple of 16, in which time point t owns the rows
 * zoff .. zoff + npad - 1, npad = n rounded up to a multiple of 4.  With gene j = genes[j] of the CSC of spadot_local_lag, its
 * fp32 values v (0 where nothing is stored) and the centre c = centre[t * G + genes[j]]:
 *   Z[zoff + i, j] = (double)v_i - c                                   (0.0 in the rows i >= n and the columns j >= ng)
 *   Y[zoff + i, j] = ((0 + Z[zoff + j1, j]) + Z[zoff + j2, j]) + ...   over the row of i in the CSR, in row order
 * (subtractions and additions only: Y has the bits of the lag of spadot_local_lag).
 * desc [T, 9] int64, once in host memory (checked here) and once on the device (read by the kernels), per time point:
 *   0 first entry of col   1 n   2 E   3 row0   4 graph id of the permutation keys   5 first entry of rowptr   6 the smallest
 *   and 7 the largest entry of col (ignored where E = 0)   8 zoff
 * spadot_cross_dense(): writes Z (fill, then the stored entries: no atomics) and Y.  With colptr NULL, Z is the caller's (dense
 * columns: the padding must be zero) and only Y is written; ridx, v, centre and genes are not read then.  rowptr, col, colptr,
 * ridx, v, nnz, ridx_lo, ridx_hi, genes, gene_lo, gene_hi as in spadot_local_lag.
 * spadot_cross_sums(): for the labelings l = 0 .. observed + P - 1 (the identity first if observed, then the permutations first ..
 * first + P - 1 of spadot_nhood_counts under (seed, graph id, p, n)):
 *   M[t, l, g, h] = sum_i Z[zoff + pi_l(i), g] Y[zoff + i, h]        (fp64 [T, observed + P, ng, ng])
 * on the fp64 matrix cores.  One workgroup of 256 threads per (t, l, 64 x 64 tile of M); every wavefront runs over all the spots
 * of the time point in ascending order, four per v_mfma_f64_16x16x4_f64, so the bits of an element depend on n, its two columns
 * and the permutation alone (two runs, a pair alone, another batch, another split over `first`: the same).  No permuted copy of Z
 * is made; LDS: 1 KiB of permuted spot numbers.
 * Return -22 for null, negative or inconsistent arguments (n < 1, ng < 1, GP other than ng rounded up to 16, rows of a time
 * point outside zrows among them) and -7, before any launch, outside the limits: ng <= 4096, n, E, nnz, row0 and graph id <=
 * 2147483647, first + P <= 2^32, T (observed + P) ceil(ng / 64)^2 <= 2147483647 (gridDim.x) for the sums; T <= 65535 (gridDim.y),
 * ceil(max npad GP / 256) <= 2147483647, every entry of col in 0 .. n-1, every row index in 0 .. max(row0 + n) - 1 and every
 * selected gene in 0 .. G-1 for the images. */
int spadot_cross_dense(const int *rowptr, const int *col, const long long *colptr, const int *ridx, const float *v, long long nnz,
                       long long ridx_lo, long long ridx_hi, const double *centre, const long long *desc_host,
                       const long long *desc_dev, int T, int G, const int *genes, int ng, int gene_lo, int gene_hi, int GP,
                       long long zrows, double *Z, double *Y, void *stream);
int spadot_cross_sums(const double *Z, const double *Y, long long zrows, int GP, const long long *desc_host,
                      const long long *desc_dev, int T, int ng, int observed, long long first, long long P, long long seed,
                      double *M, void *stream);

/* ---------------------------------------------------------------- spatial correlogram (csrc/correlogram.hip)
 * The sums behind Moran's I by distance band of every (time point, selected gene, labeling); the definition is restated in numpy
 * in tests/correlogram_ref.py.  A time point is n spots and B squared thresholds r2[0] < .. < r2[B-1]; band b holds the ordered
 * pairs (i, j), i != j, with r2[b-1] < d2(i, j) <= r2[b] (r2[-1] below 0: coincident spots are in band 0; pairs beyond r2[B-1] are
 * in no band), d2 the unfused squared distance of spadot_cooccur_counts.  cnt_b(i): the partners of spot i in band b.  With
 * x_i = Z[zoff + pi_l(i), j], Z the image of spadot_cross_dense and pi_l the identity (l = 0 if observed) or the permutation
 * first + .. of spadot_nhood_counts under (seed, graph id, p, n):
 *   W[t, b] = sum_i cnt_b(i)      S2c[t, b] = sum_i cnt_b(i)^2                                   (int64, exact; see below)
 *   N[t, j, l, b] = sum over the pairs of band b of x_i x_j      Q[t, j, l, b] = sum_i cnt_b(i) x_i^2      (fp64)
 * xy: fp64 [sum n, 2], per time point its spots in ANY order that keeps near spots near (the Morton order of graph.morton_key),
 * the time points back to back; order: int32 [sum n], per position the original index 0 .. n-1 of its spot (a permutation: the
 * caller's to refuse; the kernel clamps).  desc [T, 6] int64, once in host memory (checked here) and once on the device:
 *   0 first spot in xy (checked)   1 n   2 B   3 graph id of the permutation keys   4 zoff   5 the blocks of 256 spots of the
 *   time points before (checked)
 * r2 [T, 16] fp64, once on the host (checked here) and once on the device: the B squared thresholds, finite, >= 0 and strictly
 * increasing, then +inf in every padded place.
 * One 256-thread workgroup per (256 positions, labeling and chunk of cs genes, time point); tiles of 256 spots stream through LDS
 * and a tile whose bounding box lies further than r2[B-1] from that of the query block is skipped where cull = 1 (no bit of any
 * output changes: DESIGN 7o).  A thread adds its partners in ascending position, the workgroup its threads in a fixed order into
 * a partial per (block, column, band) in scratch, and a second launch adds the partials in ascending block order: the bits of one
 * (time point, gene, labeling, band) depend on nothing else of the call, neither on cs, cull nor the split over `first`.  No
 * floating-point atomics; W and S2c are 64-bit integer atomics from the workgroups of column chunk 0.
 * S2c is exact while sum_i cnt_b(i)^2 < 2^63 (always for n <= 2097152); a larger time point with a dense band can wrap it, and
 * is not refused.
 * cs: 2 or 4 (0: the default, 2).  scratch: fp64 [scratch_doubles] with scratch_doubles >= 4 blocks + 2 blocks (observed + P) ng
 * B_max, blocks = sum ceil(n / 256).  skipped: NULL or int64 [1], the (query block, tile) pairs that were culled.
 * out: W, S2c int64 [T, B_max]; N, Q fp64 [T, ng, observed + P, B_max]; written completely (zeros in the bands >= B).
 * Return -22 for null or inconsistent arguments (GP other than ng rounded up to 16, a scratch buffer that is too small, rows of a
 * time point outside zrows, padding other than +inf among them) and -7, before any launch, outside the limits: 1 <= B <= B_max <=
 * 16, ng <= 4096, 1 <= n <= 2147483391, T <= 65535 (gridDim.z), (observed + P) ceil(ng / cs) <= 65535 (gridDim.y), first + P <=
 * 2^32, graph id <= 2147483647, a threshold that is negative, not finite or not above the one before. */
int spadot_corr_sums(const double *xy, const int *order, const double *Z, long long zrows, int GP, const long long *desc_host,
                     const long long *desc_dev, const double *r2_host, const double *r2_dev, int T, int ng, int B_max, int observed,
                     long long first, long long P, long long seed, int cull, int cs, double *scratch, long long scratch_doubles,
                     long long *W, long long *S2c, double *N, double *Q, long long *skipped, void *stream);

/* ---------------------------------------------------------------- embed stage (csrc/embed.hip)
 * t-SNE of P problems (sets of n points in d dimensions, fp64) with sklearn's objective and optimiser, Barnes-Hut's sparse input
 * affinities and EXACT repulsion over all pairs in fp64.  The problems lie back to back in every array; prob [P, 10] int64, once in
 * host memory (checked here) and once on the device:
 *   0 first point (checked)   1 n   2 k = min(n - 1, floor(3 u))   3 first entry of the neighbour lists, sum n k before (checked)
 *   4 S, the slices of the partner range, 1 .. 65535   5 sum n S before (checked)   6 first entry of rowptr, the points
 *   before plus the problems before (checked)   7 first stored entry of the CSR (checked)   8 sum ceil(n / 256) before (checked)
 *   9 stored entries of the problem
 * spadot_latent_knn reads the columns 0 .. 3, spadot_tsne_affinities too; spadot_tsne_steps reads all.
 *
 * spadot_latent_knn: per point the k nearest OTHER points by (squared distance, index) ascending; idx int32 and d2 fp64
 * [sum n k], row i of a problem at column 3 + i k.  The squared distance is sum_c (x_ic - x_jc)^2, c ascending, UNFUSED: every
 * subtraction, product and addition is rounded once.  Self is left out by index; a duplicate of a point is its neighbour at
 * distance 0.  One 64-thread workgroup per 64 queries, a query's list in LDS as [slot][lane] (12 k 64 bytes).
 *
 * spadot_tsne_affinities: per row, with e_j = d2_j - min_j d2_j, p_j = exp(-(beta e_j)), s = sum p_j and H = log s + beta
 * (sum e_j p_j) / s: from beta = 1, 200 steps (H > log u: beta goes up, doubled while it has no upper bracket, else to the middle
 * of the bracket; otherwise down, halved or to the middle), no early stop; then cond_j = p_j / s at the last beta.  A row whose e
 * are all 0 is uniform and reports beta = 0.  perp [P] fp64 on the host (checked) and on the device; cond fp64 [sum n k], beta
 * fp64 [sum n].  One wavefront per row.
 *
 * spadot_tsne_steps queues the iterations it0 .. it0 + steps - 1 without a host synchronisation.  Iteration `it` reads Y from
 * (it odd ? Y1 : Y0) and writes the other buffer; with eps = exaggeration and mu = 0.5 while it < early, else eps = 1, mu = 0.8:
 *   q_ij = 1 / (1 + |y_i - y_j|^2) (IEEE division, the distance unfused), j != i by a select;  z_i = sum_j q_ij,  r_i = sum_j
 *   q_ij^2 (y_i - y_j), j ascending inside each of the S slices of whole 256-tiles (slice s: the tiles floor(s T / S) ..
 *   floor((s + 1) T / S) - 1 of T = ceil(n / 256); a slice without tiles adds exact zeros), the slices in their order;
 *   Z = sum_i z_i: a fixed tree per block of 256 points, the blocks ascending;  a_i = sum over row i of the CSR, in stored order,
 *   of ((eps P_ij) q_ij) (y_i - y_j);  g_i = 4 (a_i - r_i / Z);  per component: gain += 0.2 where update g < 0, else gain *= 0.8,
 *   at least 0.01;  update = mu update - lr (gain g);  y += update  (unfused: numpy on `grad` repeats them bit for bit);
 *   kl[p, it] = sum over the stored entries with P_ij > 0 of P_ij (log P_ij - log q_ij) + log Z (unexaggerated P).
 * rowptr int64 [sum (n + 1)], per problem ascending from 0; col int32 in 0 .. n-1 (the caller's to refuse: the kernel clamps),
 * val fp64.  Y0, Y1, upd, gains, grad, att fp64 [sum n, 2]; lr fp64 [P] on the device; part fp64 [sum n S, 3] and blk fp64
 * [sum ceil(n / 256), 2]: scratch; zr fp64 [sum n, 3] (z_i, r_i), att (a_i), grad (g_i) and Z fp64 [P] hold the last iteration's;
 * kl fp64 [P, kl_stride].  two: 1 gives a thread two query points (the same bits).  No atomics.
 *
 * All three return -22 for null or inconsistent arguments and -7, before any launch, outside the limits: 1 <= d <= 32, at most
 * 65535 problems, 2 <= n <= 2147483135, 1 <= k <= min(n - 1, 150), 2 <= u <= 50, n >= u + 2, 1 <= S <= 65535,
 * exaggeration >= 1. */
int spadot_latent_knn(const double *x, int d, int P, const long long *prob_host, const long long *prob_dev, int *idx, double *d2,
                      void *stream);
int spadot_tsne_affinities(const double *d2, int P, const long long *prob_host, const long long *prob_dev, const double *perp_host,
                           const double *perp_dev, double *cond, double *beta, void *stream);
int spadot_tsne_steps(const long long *prob_host, const long long *prob_dev, int P, const long long *rowptr, const int *col,
                      const double *val, double *Y0, double *Y1, double *upd, double *gains, const double *lr, double *part,
                      double *zr, double *att, double *blk, double *grad, double *Z, double *kl, long long kl_stride, long long it0,
                      int steps, long long early, double exaggeration, int two, void *stream);

/* ---------------------------------------------------------------- sepal stage (csrc/sepal.hip)
 * The diffusion time of every (time point, selected gene) on the spatial graph; the definition is restated in numpy in
 * tests/sepal_ref.py.  Time point t is a SYMMETRIC CSR over its n spots (rowptr: int32 [n + 1] ascending from 0 to M, the T arrays
 * back to back; col: int32 [M], back to back: for row i first the targets of i's own edges, then the sources of the edges that end
 * in i, so that an edge in both directions counts twice; M = 2 E), the rows row0 .. row0 + n - 1 of the CSC matrix of
 * spadot_local_lag and a rate a = rate[t] = dt n / M (fp64, formed by the caller).  Item (t, j), j = 0 .. ng-1, is gene genes[j] in
 * time point t, number t ng + j.  Its image c is fp64 [n]: at first the fp32 values of the stored entries widened, 0 elsewhere.
 * One step, Jacobi, every operation rounded once (no fused multiply-add), deg_i the length of row i:
 *   s_i = ((0 + c_j1) + c_j2) + ..  over row i in row order     l_i = s_i - deg_i c_i     c'_i = c_i + a l_i, 0 where that is < 0
 * The entropy of an image, over the spots with c_i > 0:  S = sum c_i, Q = sum c_i log c_i, H = (log S - Q / S) / n, both sums in a
 * fixed order that depends on n alone (csrc/sepal.hip's header).  The image has the bits of numpy after any number of steps; H is
 * bit-reproducible (an item alone or in a batch, either path, any split over launches) and within rounding of any other order.
 * State per item, on the device, updated in place:
 *   image [items, stride] fp64: the image in the first n places of a row; stride >= max n + (the largest n of the time points
 *   whose image does not fit in LDS, 0 if all fit), the place behind max n being the second slab of that path; image_doubles: its size
 *   H_prev fp64, iterations int32, done int32 [items]: the entropy after the last step, the steps taken, and 0 running, 1 stopped
 *   by the rule, 2 degenerate (no positive value, n < 2 or M = 0: H_prev and H0 are NaN and no step is ever run)
 *   H0 fp64 [items]: the entropy of the first image, written with init = 1
 * init = 1: the image is built from the CSC column and H0, H_prev, iterations = 0 and done are written first; init = 0: the state
 * of an earlier launch is read.  Every item that is not done then takes min(steps, n_iter - iterations) further steps; with stop =
 * 1 it ends behind the first step t with |H^t - H^(t-1)| <= thresh (done = 1).  trace: NULL or fp64 [items, trace_len]: H after
 * step number it goes to column it < trace_len, H0 to column 0.
 * One 1024-thread workgroup per item, all items in ONE launch; no host round trip per step, no atomics, no workgroup waits for
 * another.  The image lives in LDS where 512 + 8 n <= lds_limit (at most 98816, n <= 12288: what the registers of the workgroup
 * hold between the two barriers of a step; larger values mean 98816), otherwise in the item's row of `image`.
 * desc [T, 8] int64 as for spadot_local_lag (column 2 holds M, column 4 is not read), once on the host (checked here) and once on
 * the device; rate once on the host (checked) and once on the device.
 * Return -22 for null, negative or inconsistent arguments (an image that is too small among them) and -7, before any launch,
 * outside the limits: 1 <= steps, n_iter <= 2147483647, thresh >= 0 and finite, 0 < a and finite where M > 0, 1 <= n <=
 * 2147483647, M, nnz and row0 <= 2147483647, every entry of col in 0 .. n-1, every row index in 0 .. max(row0 + n) - 1, every
 * selected gene in 0 .. G-1, T ng <= 2147483647 (gridDim.x).  That rowptr ascends from 0 to M, that no value is negative and that
 * a max deg < 1 are the caller's to refuse (the kernel clamps what it reads). */
int spadot_sepal_steps(const int *rowptr, const int *col, const long long *colptr, const int *ridx, const float *v, long long nnz,
                       long long ridx_lo, long long ridx_hi, const long long *desc_host, const long long *desc_dev,
                       const double *rate_host, const double *rate_dev, int T, int G, const int *genes, int ng, int gene_lo,
                       int gene_hi, int init, int stop, long long steps, long long n_iter, double thresh, long long lds_limit,
                       double *image, long long image_doubles, long long stride, double *H_prev, double *H0, int *iterations,
                       int *done, double *trace, long long trace_len, void *stream);

/* ---------------------------------------------------------------- trends stage (csrc/trends.hip)
 * The log-normalised counts of every time point, transposed, times a dense row-major fp64 W[n, C] (rows in the permuted order of
 * the CSC arrays), as three weighted moments in one pass over the stored entries.  Same CSC layout as the preprocess and markers
 * stages; v: the fp32 values of spadot_mk_lognorm in CSC order.  With vd = (double)v and vv = vd * vd, over the stored entries
 * (i, g) whose row i lies in time point t:
 *   S0[t, g, c] = sum W[i, c],   S1[t, g, c] = sum vd W[i, c],   S2[t, g, c] = sum vv W[i, c]      (fp64 [T, G, C])
 * A stored entry with v = 0 adds W to S0 and nothing to S1, S2; W may be negative.  One workgroup per (t, g); wavefront w of its
 * four adds the segment's entries w, w + 4, ... in that order and the four partial sums are added as ((p0 + p1) + p2) + p3: no
 * atomics, and the bits of an output element depend only on its segment and its column of W, not on C, T, G or the other
 * columns (two runs, a column alone, a problem in another batch: the same bits).  No temporaries in global memory.
 * spadot_weighted_moments_chunk(): the stored entries staged in LDS at a time (segments of any length are taken).
 * Limits (return -7, nothing launched): 1 <= C <= 1024, n <= 2147483647, T * G <= 2147483647 (gridDim.x). */
int spadot_weighted_moments_chunk(void);
int spadot_weighted_moments(const long long *colptr, const int *ridx, const float *v, const int *tp_off, int T, int G,
                            const double *W, long long n, int C, double *S0, double *S1, double *S2, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPADOT_MODEL_H */
