/*
 * sigsvgd_hip.h -- C ABI of libsigsvgd_hip.so: the MI355X (gfx950) implementation of the
 * signature-kernel SVGD hot path of lubaroli/sigsvgd.
 *
 * What each entry point replaces in the reference (Python; there is no native code there):
 *
 *   sigsvgd_gram_fwd       sigkernel.SigKernel.compute_Gram(X, Y) forward
 *                          call sites: src/kernels/_traj_kernels.py:203-206,
 *                                      src/inference/trajectory_svgd.py:60-63
 *                          static kernel fused in: src/kernels/_traj_kernels.py:176-195
 *   sigsvgd_gram_fwd_bwd   the same forward + its autograd backward for grad_output
 *                          (d sum(grad_out*K) / dX, first argument only), triggered by
 *                          src/inference/score.py:68-69, src/inference/trajectory_svgd.py:65
 *   sigsvgd_svgd_phi       SVGD._velocity dense part: v = -((K @ score - grad_k)/N) [* mask]
 *                          src/inference/svgd.py:82-83, src/inference/trajectory_svgd.py:84
 *                          optionally fused with the optimizer=None update X - lr*v (svgd.py:115)
 *   sigsvgd_svgd_step      the same with the adaptive_gradient=True scaling fused (svgd.py:110-113)
 *   sigsvgd_svgd_adam_step the same with the update of the reference's DEFAULT optimizer fused: torch.optim.Adam
 *                          stepped through a closure that sets X.grad to the velocity (svgd.py:20,100-107)
 *   sigsvgd_svgd_update    the three update rules above (optimizer=None, adaptive_gradient=True, Adam) and the mask on a
 *                          velocity that is given: the particle-sharded step, after its reduction over ranks
 *   sigsvgd_vec_sqdist     src/utils/math.py:69-86 pw_dist_sq, :116-144 scaled_pw_dist_sq
 *   sigsvgd_vec_kernel     src/kernels/_kernels.py:64-299 GaussianKernel / ScaledGaussianKernel /
 *                          IMQKernel / ScaledIMQKernel: K and d_K.sum(1) without the [A,B,D] tensor
 *   sigsvgd_obstacle_cost  batch_cost_fn of examples/script_planning_obstacle_field.py:113-126 (spline samples,
 *                          obstacle field, path length) and its gradient w.r.t. the knots (torch autograd there)
 *   sigsvgd_vec_kernel_fused  the same classes with a fixed bandwidth: distance, kernel and summed gradient in one launch
 *   sigsvgd_signature      signatory.signature(path, depth, basepoint) [third-party, absent] as
 *                          called by PathSigKernel, src/kernels/_traj_kernels.py:124-125
 *   sigsvgd_signature_backward  its autograd backward: PathSigKernel has analytic_grad=False (:92), so the reference
 *                          differentiates K THROUGH the signature (src/inference/score.py:50-55, svgd.py:41-43)
 *   sigsvgd_pde_fwd        the PDE of sigkernel.SigKernel on a static kernel the CALLER evaluated (any object with
 *   sigsvgd_pde_fwd_bwd    Gram_matrix / batch_kernel): K per grid, and the adjoint with respect to the grid
 *   sigsvgd_gram_long_fwd  sigsvgd_gram_fwd / _fwd_bwd for the long paths those refuse (built-in static kernels,
 *   sigsvgd_gram_long_fwd_bwd  static kernel evaluated inside the PDE sweep)
 *   sigsvgd_pair_fwd       sigkernel.SigKernel.compute_kernel(X, Y) with a built-in static kernel: k_sig(X_i, Y_i) per
 *   sigsvgd_pair_fwd_bwd   pair, and the gradients of both paths from one solve per pair
 *   sigsvgd_gram_long_fwd_bwd2  sigsvgd_gram_long_fwd_bwd with the gradients of both slots from one solve per pair
 *                          (sigkernel's compute_mmd with a trainable Y), and with Y = X each unordered pair once (SVGD)
 *   sigsvgd_sqdist_select  torch.median of the [A,B,TX,TY] distance tensor inside bw_median (src/utils/math.py:28-34), the
 *                          default bandwidth of BatchGaussianKernel (src/kernels/_traj_kernels.py:186-194): an exact order
 *                          statistic of the point distances without that tensor
 *
 * Conventions
 *   - all pointers are DEVICE pointers (HIP), row-major contiguous; the caller owns every buffer
 *     and keeps it alive until the work queued on `stream` has completed;
 *   - inputs are read-only; outputs are fully overwritten; nothing persistent is allocated;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue work
 *     (no host synchronisation, graph-capturable);
 *   - return value 0 = ok, negative = error (see SIGSVGD_E_*); sigsvgd_last_error() gives text;
 *   - `dtype` selects the I/O element type of X, Y, grad_out, K_out, gradX_out:
 *     SIGSVGD_F32 or SIGSVGD_F64.  Arithmetic of the register-resident and quadrant kernels
 *     (dyadic order 0, T <= 128) and of the refined-grid kernels (T <= 33 with dyadic refinement to
 *     64 .. 256 cells per side: the reference's own call shapes): fp64 static kernel + 4-corner
 *     increments, fp32 PDE sweeps in difference form, fp32 storage of per-pair intermediates, fp32
 *     gradient contraction, fp64 reduction over pairs; the coverage kernel (other refinements, longer
 *     paths, more than 16 channels -- except RBF paths of 17 to 32 channels at dyadic order 0, 3 <= T <= 64 with
 *     SIGSVGD_FLAG_FP32_SWEEPS, which take the register-resident kernel: see the flag --, linear kernel, naive solver,
 *     SIGSVGD_FLAG_FORCE_GENERIC) is fp64 end to end (DESIGN.md
 *     "precision plan").  The fp32 route is checked PER PAIR and a pair that fails a check has its K solved
 *     again by the coverage kernel in fp64 (static kernel, increments, sweeps) inside the same call:
 *       (1) cancellation -- the largest |K| on the pair's PDE grid exceeds 2x .. 8x max(|K|, 0.1)
 *           (oscillating discrete solutions of rough paths in few channels);
 *       (2) conditioning, paths in <= 3 channels, dyadic order 0 -- the first-order condition number of K
 *           in the increments, sum |K_fwd U D| / max(|K|, 0.1), exceeds 150 (forward-only launches: the bound
 *           sum |K_fwd D| max(grid maximum, 1) / max(|K|, 0.1) exceeds 300): there the fp32 STORAGE of the
 *           increments limits K whatever the precision of the sweeps.
 *     The rule is defined once, in sigsvgd_amd/csrc/sweep_scaffold.h.  The exact pass ENFORCES the bound below for paths
 *     in d <= 4 channels on the register-resident kernel (T <= 64) and d <= 3 on the quadrant, refined-grid and band
 *     kernels; for d >= 5 the bound is measured, not enforced.  sigsvgd_gram_fwd and sigsvgd_gram_fwd_bwd apply (2) in
 *     its two forms (the bound 300 forward-only, the condition number 150 with the gradient), so for a flagged pair the
 *     two may return different bits, both within the bound.
 *     Measured bound (DESIGN.md sections 2, 3): every entry of K_out within 1e-5 RELATIVE of the fp64
 *     reference's (plain |K - K_ref| / |K_ref|, no floor) over the committed rough-path cases and 18,000
 *     random soak cases; unflagged pairs of the calibration study are within 2.5e-6.  (The 8- / 16-channel
 *     kernels for T <= 64 have no exact pass: their cancelled pairs repeat the sweep in fp64 on fp32
 *     increments; tests/test_gpu_precision.py::test_rough_wide_paths_default_dispatch holds d = 5 .. 16,
 *     T = 32 .. 128, steps 0.2 / 0.5, h = 0.1 .. 1 to 1e-5 in every launch form.)  Only K is repaired: the
 *     gradient of a flagged pair keeps the fp32 solution (its error is relative to the largest gradient entry
 *     of the launch and stayed below 5e-6 of it in every regime measured).  Gram + gradient launches of paths
 *     in ONE channel at dyadic order 0 run on the coverage kernel (fp64 sweeps): very smooth one-channel paths
 *     (K = 1 + O(1e-4)) left the fp32 sweeps' gradient at up to 2.0e-5; now <= 4.2e-6
 *     (test_smooth_one_channel_order0).  SIGSVGD_FLAG_FORCE_GENERIC returns 6e-8 anywhere.
 *   - results are bit-reproducible: every reduction over pairs runs in an order fixed by the launch
 *     geometry (no floating-point atomics), so two calls on the same inputs return the same bits.
 *     sigsvgd_vec_kernel_fused is reproducible when it is given its workspace (sigsvgd_vec_fused_workspace_bytes);
 *     without one its column splits meet in fp32 atomics and the last bits of dK_out may differ between calls.
 *   - environment, read per launch, for tests and measurements only (results do not depend on any of them, bit for bit):
 *     SIGSVGD_BAND_MODE=serial|parallel pins the schedule of the refined-grid launches;
 *     SIGSVGD_PAIR_MODE=serial|bands pins the schedule of the paired launches (sigsvgd_pair_*): one wavefront per pair, or a
 *     workgroup per pair with the pair's 64-row bands dealt to its wavefronts, wherever that plan has two or more
 *     (sigsvgd_pair_schedule tells which one a launch would run; any other value is ignored);
 *     SIGSVGD_SWEEP_WINDOWS=table keeps Gram + gradient launches of 64-point paths on the register-resident kernel
 *     whose PDE sweeps read their lane windows from the constant table (what every other path length runs) instead
 *     of its twin with the windows as immediates, so that the two can be compared on one build;
 *     SIGSVGD_WAVE_BALANCE=off sends symmetric Gram + gradient launches of 64-point paths in up to 8 channels to the
 *     fixed-window kernel without the per-half wave priorities instead of the twin that sets them.
 */
#ifndef SIGSVGD_HIP_H
#define SIGSVGD_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIGSVGD_ABI_VERSION 10

/* dtype */
#define SIGSVGD_F32 0
#define SIGSVGD_F64 1

/* static kernel kinds */
#define SIGSVGD_STATIC_RBF 0    /* k(x,y) = exp(-|x-y|^2 * inv_h)   (reference: exp(-dist/h)) */
#define SIGSVGD_STATIC_LINEAR 1 /* k(x,y) = <x,y>                                              */
/* The heavy-tailed radial kinds, s = |x-y|^2 * inv_h with inv_h > 0 as for RBF.  Accepted from the
 * second revision of ABI 10 on (no new symbol, no changed signature: a library of the first revision answers
 * SIGSVGD_E_BADARG).  They run on the fp64 kernels: sigsvgd_gram_fwd / _fwd_bwd wherever the coverage kernel's plan fits,
 * and the long-path entry points (sigsvgd_gram_long_*, sigsvgd_pair_*) with the default stencil only --
 * SIGSVGD_FLAG_NAIVE_SOLVER with them is SIGSVGD_E_UNSUPPORTED there.  sigsvgd_gram_sym_partial refuses them unless
 * SIGSVGD_FLAG_FP32_SWEEPS sends them to the register-resident kernel (3 <= T <= 64; see the flag). */
#define SIGSVGD_STATIC_IMQ 2    /* k(x,y) = (1 + s)^(-1/2)          (inverse multiquadric)     */
#define SIGSVGD_STATIC_RQ 3     /* k(x,y) = (1 + s)^(-1)            (rational quadratic)       */
/* The Matern kinds, accepted by a later revision of ABI 10 (again no new symbol and no changed
 * signature: an earlier library answers SIGSVGD_E_BADARG).  Same s and the same routes, refusals and workspace figures as IMQ / RQ above; a Matern kernel of lengthscale l
 * is inv_h = 1 / l^2.  s is clamped at 0 before the square root, and -dk/ds is finite at s = 0 (3/2 and 5/6), so coincident
 * points contribute a zero gradient term.  Kinds 4 and 5 are reserved and stay SIGSVGD_E_BADARG.  Matern-1/2 (exp(-sqrt(s)),
 * whose slope is unbounded at 0) is not provided.  The sigsvgd_*_h entry points take both kinds. */
#define SIGSVGD_STATIC_MATERN32 6 /* k(x,y) = (1 + u) exp(-u),           u = sqrt(3 s);  -dk/ds = (3/2) exp(-u)         */
#define SIGSVGD_STATIC_MATERN52 7 /* k(x,y) = (1 + u + u^2/3) exp(-u),   u = sqrt(5 s);  -dk/ds = (5/6) (1 + u) exp(-u) */

/* vector kernels (sigsvgd_vec_kernel) */
#define SIGSVGD_VEC_GAUSSIAN 0 /* k = exp(-sq / (2 h^2))          src/kernels/_kernels.py:106 */
#define SIGSVGD_VEC_IMQ 1      /* k = (1 + sq / (2 h^2))^(-1/2)     src/kernels/_kernels.py:229-230 */
#define SIGSVGD_VEC_UNIT 2     /* k = sq, w = 1: dK = grad_scale * sum_j grad_out_ij (XM_i - YM_j),
                                  the adjoint of sigsvgd_vec_sqdist (autograd through the distance) */

/* flags
 *
 * Which entry point takes which flag (one row per family; a family's workspace, plan and schedule queries answer as its
 * launches do).  Columns, in the order of the bits: NV NAIVE_SOLVER, SYM, YX Y_IS_X, FG FORCE_GENERIC, WC WS_CLEAN,
 * SF STORED_FORWARD, FOLD FOLD_TILES, FP32 FP32_SWEEPS, EX EXACT_ADJOINT, NT NAN_TAILS, LK LOG_K, NM NORMALIZED,
 * NF NORMALIZED_FUSED.  Cells:
 *   T  taken: the flag means what its paragraph below says        i  taken and ignored: the bit changes nothing
 *   G  taken by the gradient forms (a launch with a gradient output, a query with want_grad / want_gradX / want_gradY),
 *      B otherwise
 *   U  SIGSVGD_E_UNSUPPORTED ahead of every other check of the flags: the entry point has no kernels for the bit
 *   R  SIGSVGD_E_UNSUPPORTED from the choice of kernel: the partial solve has the fp32-sweep kernels only
 *   B  an unknown bit: SIGSVGD_E_BADARG, the message states the refused bits in hex and lists the ones taken
 *                        NV  SYM YX  FG  WC  SF  FOLD FP32 EX  NT  LK  NM  NF
 * gram_workspace_bytes   T   i   T   T   i   i   i    T    U   i   i   i   T
 * gram_fwd               T   T   T   T   i   i   i    T    i   i   i   i   T
 * gram_fwd_bwd           T   T   T   T   i   i   i    T    U   i   i   i   T
 * gram_sym_partial       R   T   i   R   i   i   T    T    U   i   i   i   U
 * pde                    T   B   B   B   B   B   B    B    G   B   B   B   B
 * gram_long              T   T   i   B   B   B   B    B    G   U   B   B   B
 * pair                   T   B   B   B   B   B   B    B    G   T   T   B   B
 * gram_long2             T   T   T   B   B   B   B    B    G   T   T   T   B
 * gram_long_h            T   T   T   B   B   B   B    B    T   U   B   B   B
 * pair_h                 T   B   B   B   B   B   B    B    T   U   B   B   B
 * gram_long_partial      T   T   i   B   B   B   T    B    U   U   B   B   B
 * sqdist_select          B   B   T   B   B   B   B    B    B   B   B   B   B
 * Rows: pde = sigsvgd_pde_fwd, _fwd_bwd; gram_long = sigsvgd_gram_long_fwd, _fwd_bwd; pair = sigsvgd_pair_fwd, _fwd_bwd,
 * _schedule; gram_long2 = sigsvgd_gram_long_fwd_bwd2; gram_long_h = sigsvgd_gram_long_fwd_bwd_h; pair_h =
 * sigsvgd_pair_fwd_bwd_h; gram_long_partial = sigsvgd_gram_long_sym_partial and its plan; the others are named in full.
 * Pairs that are not built -- SIGSVGD_E_UNSUPPORTED wherever the first flag is taken, checked after the U cells and before
 * the unknown bits, the message names both flags: NT with EX; LK with NV, EX or NT; NM with NV, EX, NT or LK; NF with NV.
 * On the long route (the six rows from gram_long to gram_long_partial) NV with IMQ, RQ or a Matern kind is
 * SIGSVGD_E_UNSUPPORTED.  SYM needs A == B (and TX == TY) where it is T; YX needs them in sigsvgd_gram_fwd_bwd, in
 * sigsvgd_gram_fwd with NF, in gram_long2, gram_long_h and sqdist_select; with either, gram_long2 and gram_long_h take no
 * gradY_out.  (tests/test_flag_contract_cpu.py runs every flag word against this table.) */
#define SIGSVGD_FLAG_NAIVE_SOLVER 1u /* first-order stencil (sigkernel _naive_solver=True)      */
#define SIGSVGD_FLAG_SYM 2u          /* sigkernel sym=True backward weighting: go + go^T (A==B) */
#define SIGSVGD_FLAG_Y_IS_X 4u       /* caller guarantees Y aliases X (same values): lets the   */
                                     /* library solve each unordered pair once                  */
#define SIGSVGD_FLAG_STORED_FORWARD 32u /* accepted and ignored: every kernel of this library keeps the forward solution   */
                                       /* (ABI 4-6 used it to route long paths away from a kernel that regenerated it)     */
#define SIGSVGD_FLAG_WS_CLEAN 16u     /* accepted and ignored since ABI 8: no launch needs a zeroed workspace any more */
                                      /* (partial sums are stored, not accumulated), none issues a memset, and a        */
                                      /* captured graph of an iteration consists of kernel nodes only                   */
#define SIGSVGD_FLAG_FOLD_TILES 64u    /* sigsvgd_gram_sym_partial: this launch owns the row tiles tile_offset + k*tile_stride AND  */
                                      /* their mirror images ntile-1 - (tile_offset + k*tile_stride): a tile and its mirror image  */
                                      /* together always hold the same number of pairs of the upper triangle, so every rank of   */
                                      /* the sharded step gets the same share (cyclic ownership alone: +5.4 % on the first rank)    */
#define SIGSVGD_FLAG_FP32_SWEEPS 128u  /* IMQ / rational-quadratic static kernel (SIGSVGD_STATIC_IMQ, _RQ) at dyadic order 0, 3 <= T <= 64,   */
                                      /* d <= 16, default stencil: run the register-resident fp32-sweep kernel RBF runs there instead of  */
                                      /* the fp64 coverage kernel.  Opt-in because it selects that kernel's        */
                                      /* accuracy contract (above: every entry of K within 1e-5 relative, the gradient within 1e-5 of its  */
                                      /* largest entry; the per-pair checks and the fp64 repair of K apply) where the default holds these  */
                                      /* kinds to fp64 results.  sigsvgd_gram_fwd / _fwd_bwd / _workspace_bytes and                         */
                                      /* sigsvgd_gram_sym_partial take it.  One-channel Gram + gradient launches stay on the coverage      */
                                      /* kernel as for RBF; with any other kind, shape, order, SIGSVGD_FLAG_NAIVE_SOLVER or                */
                                      /* SIGSVGD_FLAG_FORCE_GENERIC the bit is accepted and ignored (as it was before this revision of     */
                                      /* ABI 10, which adds no symbol and changes no signature).                                            */
                                      /* RBF: at dyadic order 0, 3 <= T <= 64, default stencil, 17 <= d <= 32 the   */
                                      /* bit sends sigsvgd_gram_fwd / _fwd_bwd (and their _workspace_bytes query) to the same kernel's      */
                                      /* 32-channel layout, at the same contract, instead of the coverage kernel; opt-in because K and the  */
                                      /* gradient then are fp32-sweep results where the default route's are fp64 ones.  RBF at d <= 16 runs  */
                                      /* that kernel by default and the bit changes nothing there; sigsvgd_gram_sym_partial and              */
                                      /* sigsvgd_gram_sym_tile_rows (which has no flags argument) keep refusing d > 16 with or without it   */
#define SIGSVGD_FLAG_EXACT_ADJOINT 256u /* gradient launches of the long route (sigsvgd_pde_fwd_bwd, sigsvgd_gram_long_fwd_bwd, _fwd_bwd2,     */
                                      /* _fwd_bwd_h, sigsvgd_pair_fwd_bwd, _fwd_bwd_h): every gradient -- dG_out,      */
                                      /* gradX_out, gradY_out, dK_dinvh_out -- is the exact derivative of the discrete K the launch returns, */
                                      /* the adjoint of the default (second-order) stencil itself, instead of the reference's GG convention  */
                                      /* K_fwd[p][q] K_rev[p+1][q+1], which is that derivative for the first-order stencil only and differs  */
                                      /* from it by per cents otherwise.  K_out is bit-identical to the unflagged launch, the workspace is   */
                                      /* the same bytes, the cost is the same sweeps.  With SIGSVGD_FLAG_NAIVE_SOLVER the bit is accepted    */
                                      /* and the launch is the unflagged one (GG is exact there).  Paired launches run one wavefront per     */
                                      /* pair with it (sigsvgd_pair_schedule says so).  Forward-only launches and their queries refuse it    */
                                      /* as an unknown bit (SIGSVGD_E_BADARG); sigsvgd_gram_long_sym_partial with its plan and workspace     */
                                      /* queries, sigsvgd_gram_fwd_bwd, sigsvgd_gram_sym_partial and sigsvgd_gram_workspace_bytes, whose     */
                                      /* routes have GG kernels only, return SIGSVGD_E_UNSUPPORTED.  A later revision of ABI 10: no new      */
                                      /* symbol, no changed signature; an earlier library answers SIGSVGD_E_BADARG                           */
#define SIGSVGD_FLAG_NAN_TAILS 512u   /* variable-length batches on the long route: a path of X[A][TX][d] or        */
                                      /* Y[B][TY][d] ends before its first point whose channel 0 is NaN (length L = that index, T where     */
                                      /* there is none).  The path is its points 0 .. L-1 and pair (i, j) is solved on its own                */
                                      /* r (L_i - 1) x r (L_j - 1) grid: K and the gradients have the bits of the unflagged 1 x 1 launch on    */
                                      /* the truncated paths.  Rows m >= L of every gradient output are exact zeros, row L-1 is the end        */
                                      /* point's whole gradient.  L = 1 is a one-point path: K = 1 exactly, no gradient.  L = 0 (a path that   */
                                      /* starts with NaN) is the caller's error: it is treated as L = 1, the result is unspecified, nothing     */
                                      /* is read or written out of bounds.  The lengths are found on the device by a pass of its own ahead of  */
                                      /* the launch, on its stream (no read-back, no host sync: capturable), into int arrays at the head of    */
                                      /* the workspace, which grows by them (padded to 256 B) and by nothing else; with SIGSVGD_FLAG_Y_IS_X     */
                                      /* Y's lengths are X's.  Taken by sigsvgd_gram_long_fwd_bwd2 (every output combination, forward only     */
                                      /* included) with sigsvgd_gram_long2_workspace_bytes, and by sigsvgd_pair_fwd, sigsvgd_pair_fwd_bwd,      */
                                      /* sigsvgd_pair_workspace_bytes and sigsvgd_pair_schedule; paired launches run one wavefront per pair    */
                                      /* with it (sigsvgd_pair_schedule says so).  SIGSVGD_E_UNSUPPORTED before any device work from           */
                                      /* sigsvgd_gram_long_fwd, _fwd_bwd, _fwd_bwd_h, sigsvgd_pair_fwd_bwd_h, sigsvgd_gram_long_sym_partial     */
                                      /* and their queries, and from every entry point when SIGSVGD_FLAG_EXACT_ADJOINT is set too.  Every       */
                                      /* other entry point treats it as the unknown bit it was.  A later revision of ABI 10: no new symbol,     */
                                      /* no changed signature; an earlier library answers SIGSVGD_E_BADARG                                     */
#define SIGSVGD_FLAG_LOG_K 1024u      /* log-domain solve on the long route.  K_out holds the natural logarithm      */
                                      /* ln K(X_i, Y_j) (same layout, same mirror store with SIGSVGD_FLAG_Y_IS_X) and every gradient output   */
                                      /* sum_ij w_ij grad ln K_ij = sum_ij w_ij grad K_ij / K_ij in the GG convention; grad_out,              */
                                      /* SIGSVGD_FLAG_SYM, SIGSVGD_FLAG_Y_IS_X and NULL outputs mean what they mean without the bit.  The     */
                                      /* sweeps carry a running power-of-two scale (mantissas are those of the unscaled solve), the stored    */
                                      /* forward solution and the fp32 S partials are scaled too, so nothing overflows while ln K itself is   */
                                      /* representable: the signature kernel of long rough paths passes fp32 from about T = 300 and fp64      */
                                      /* from about T = 1600.  A pair whose discrete K is <= 0 gets NaN in K_out and in its gradient          */
                                      /* contribution.  All six static kinds, both dtypes, any dyadic order, default stencil.  Taken by       */
                                      /* sigsvgd_gram_long_fwd_bwd2 (every output combination, forward only included) with                    */
                                      /* sigsvgd_gram_long2_workspace_bytes, and by sigsvgd_pair_fwd, sigsvgd_pair_fwd_bwd,                   */
                                      /* sigsvgd_pair_workspace_bytes and sigsvgd_pair_schedule; paired launches run one wavefront per pair   */
                                      /* with it (sigsvgd_pair_schedule says so).  The workspace grows by one int per band and block of 64    */
                                      /* sweep steps and wave (forward-only launches need that much too), the LDS by one int per block.       */
                                      /* SIGSVGD_E_UNSUPPORTED before any device work from those entry points when                            */
                                      /* SIGSVGD_FLAG_NAIVE_SOLVER, SIGSVGD_FLAG_EXACT_ADJOINT or SIGSVGD_FLAG_NAN_TAILS is set too.  Every   */
                                      /* other entry point treats it as the unknown bit it was.  A later revision of ABI 10: no new symbol,   */
                                      /* no changed signature; an earlier library answers SIGSVGD_E_BADARG                                    */
#define SIGSVGD_FLAG_NORMALIZED 2048u /* normalised signature kernel and its gradient from one call on the long route (DESIGN.md section      */
                                      /* 5.22).  With l_ij = ln K(X_i, Y_j), a_i = ln K(X_i, X_i), b_j = ln K(Y_j, Y_j), all from the          */
                                      /* log-domain solve of SIGSVGD_FLAG_LOG_K (which the bit implies and is not combined with), K_out holds   */
                                      /* K^_ij = exp(l_ij - (a_i / 2 + b_j / 2)), kept in fp64 until the one rounding to the I/O type (same     */
                                      /* layout, same mirror store with SIGSVGD_FLAG_Y_IS_X, whose diagonal is exactly 1).  With w = grad_out   */
                                      /* (NULL: ones; SIGSVGD_FLAG_SYM: w + w^T) and U = w * K^ entry by entry, in the GG convention            */
                                      /*   gradX_out[i] = sum_j U_ij d1 l_ij - 1/2 (sum_j U_ij) grad a_i,                                      */
                                      /*   gradY_out[j] = sum_i U_ij d2 l_ij - 1/2 (sum_i U_ij) grad b_j,                                      */
                                      /* grad a_i the derivative of ln K(X_i, X_i) in both slots; each row summed in fp64 and rounded once.     */
                                      /* SIGSVGD_FLAG_Y_IS_X, SIGSVGD_FLAG_SYM, NULL outputs and forward-only launches mean what they mean      */
                                      /* without the bit: with Y_IS_X and no SYM gradX_out[i] is the derivative of sum_j w_ij K^(X_i, Y_j) in   */
                                      /* X_i at fixed Y = X, the first-slot gradient SVGD uses; the diagonal pairs of a Y_IS_X launch, whose    */
                                      /* K^ is the constant 1, are left out of both terms.  Every pair is solved once; the diagonals are        */
                                      /* a paired pass ahead of the launch on the same stream, no host synchronisation, no allocation.  A pair  */
                                      /* whose discrete K is <= 0 gives NaN in its K^ and the gradient rows it touches, a diagonal K <= 0 in    */
                                      /* its whole row or column.  All six static kinds, both dtypes, any dyadic order, default stencil.        */
                                      /* Taken by sigsvgd_gram_long_fwd_bwd2 and sigsvgd_gram_long2_workspace_bytes only.  The workspace is     */
                                      /* the SIGSVGD_FLAG_LOG_K launch's plus the diagonals' logarithms (8 (A + B) bytes, 8 A with Y_IS_X,   */
                                      /* padded to 256 B) and, with a gradient output, the pairs' fp64 weights w K^ (8 A B bytes), per side  */
                                      /* whose gradient is wanted that side's fp64 diagonal gradients ([A][TX][d] or [B][TY][d]) and sums       */
                                      /* ([A] or [B]); never less than the LOG_K launch's.  The weights stay fp64: with fp32 I/O a K^ below     */
                                      /* fp32's range is stored as 0 and still counts in the gradient under a large grad_out.                   */
                                      /* SIGSVGD_E_UNSUPPORTED before any device work when SIGSVGD_FLAG_NAIVE_SOLVER,                           */
                                      /* SIGSVGD_FLAG_EXACT_ADJOINT, SIGSVGD_FLAG_NAN_TAILS or SIGSVGD_FLAG_LOG_K is set too.  Every other      */
                                      /* entry point treats it as the unknown bit it was.  A later revision of ABI 10: no new symbol, no        */
                                      /* changed signature; an earlier library answers SIGSVGD_E_BADARG                                         */
#define SIGSVGD_FLAG_NORMALIZED_FUSED 4096u /* normalised signature kernel and its first-slot gradient on the fused Gram route (DESIGN.md */
                                      /* section 5.23): sigsvgd_gram_fwd, sigsvgd_gram_fwd_bwd and sigsvgd_gram_workspace_bytes (bit 2048  */
                                      /* stays the ignored bit it always was there).  SIGSVGD_FLAG_NORMALIZED's semantics restricted to    */
                                      /* what this route has, one T for both batches and the first-slot gradient: a_i = ln K(X_i, X_i) and */
                                      /* b_j = ln K(Y_j, Y_j) from the paired log-domain solve (fp64, unrounded), s_ij = exp(-(a_i + b_j)  */
                                      /* / 2) in fp64, K_out[i][j] = K_ij s_ij with K_ij what the unflagged launch of the same route       */
                                      /* returns, the product formed in fp64 and rounded once to the I/O type; with SIGSVGD_FLAG_Y_IS_X     */
                                      /* the diagonal is stored as exactly 1 and K_out stays bit-symmetric.  With w = grad_out (NULL:      */
                                      /* ones; SIGSVGD_FLAG_SYM: w + w^T) and U = w * K^ entry by entry, in the GG convention               */
                                      /*   gradX_out[i] = sum_j w_ij s_ij d1 K_ij - 1/2 (sum_j U_ij) grad a_i,                             */
                                      /* grad a_i the derivative of ln K(X_i, X_i) in both slots; with Y_IS_X the diagonal pair is left    */
                                      /* out of both terms (weight 0, U 0): its two terms would come from an fp32-sweep and an fp64 solve  */
                                      /* and cancel to 1e-5 of |grad a_i| only.  Pipeline, all on the caller's stream without host         */
                                      /* synchronisation or allocation (capturable): the diagonal pass of SIGSVGD_FLAG_NORMALIZED, a       */
                                      /* kernel that writes W' = (I/O type)(w s) (always, also for grad_out == NULL; SYM applied there),   */
                                      /* the unflagged launch with grad_out = W' on whatever route it takes -- no pair kernel differs, and */
                                      /* SIGSVGD_FLAG_FORCE_GENERIC and SIGSVGD_FLAG_FP32_SWEEPS mean what they mean without the bit --,   */
                                      /* and one wavefront per row that scales K_out in place, adds U_i in fp64 in a fixed order (no       */
                                      /* atomics: two runs give the same bits) and adds the diagonal term to gradX_out in one fma per      */
                                      /* entry.  The accuracy is the unflagged route's: K^ per entry as K, the gradient within that        */
                                      /* route's bound of max|first term| + max|second term|.  Defined where K(X_i, X_i) and K(Y_j, Y_j)   */
                                      /* fit the I/O type, as the unflagged launch's K_out is (a 64-point walk's is 1e7 .. 1e12); past     */
                                      /* that use SIGSVGD_FLAG_NORMALIZED on the long route.  A diagonal K <= 0 gives NaN in its row or    */
                                      /* column.  All six static kinds, both dtypes, every dyadic order and route of these entry points.  */
                                      /* Workspace: the unflagged query's bytes plus the logarithms (8 (A + B) bytes, 8 A with Y_IS_X),    */
                                      /* the diagonal pass's scratch (sigsvgd_pair_workspace_bytes with SIGSVGD_FLAG_LOG_K) and, for a     */
                                      /* gradient launch, W' [A][B] (sized for fp64 I/O: the query has no dtype), the fp64 diagonal        */
                                      /* gradients [A][T][d] and the sums [A]; each padded to 256 B; never less than the unflagged         */
                                      /* query's.  A shape whose diagonal pass the paired plan refuses is refused as a whole, with that    */
                                      /* plan's message, and every refusal comes before any device work.  SIGSVGD_E_UNSUPPORTED with       */
                                      /* SIGSVGD_FLAG_NAIVE_SOLVER (the diagonal pass has the default stencil only) and from               */
                                      /* sigsvgd_gram_sym_partial; SIGSVGD_FLAG_EXACT_ADJOINT keeps its answer.  Every other entry point   */
                                      /* treats it as the unknown bit it is.  A later revision of ABI 10: no new symbol, no changed        */
                                      /* signature; an earlier library ignores the bit here and returns the unnormalised K                 */
#define SIGSVGD_FLAG_FORCE_GENERIC 8u /* use the coverage kernel: fp64 end to end (every entry of K is the fp64 reference's up to */
                                      /* the store in `dtype`, in any regime): whole-grid fp64 tables where they fit LDS, per-band */
                                      /* fp64 increments beyond that (dyadic order 0, T <= ~200); one wavefront per pair; tests,   */
                                      /* and callers who want the gradient of rough few-channel paths from fp64 sweeps as well     */

/* errors */
#define SIGSVGD_OK 0
#define SIGSVGD_E_BADARG -1
#define SIGSVGD_E_UNSUPPORTED -2 /* shape does not fit the device limits (LDS) */
#define SIGSVGD_E_WORKSPACE -3   /* workspace too small */
#define SIGSVGD_E_HIP -4         /* a HIP runtime call failed */

int sigsvgd_abi_version(void);
const char *sigsvgd_last_error(void);

/* The workspace contract of every entry point below that takes `workspace, workspace_bytes`:
 *   1. a buffer of exactly the bytes the entry point's *_workspace_bytes query reports is enough;
 *   2. the pointer may have any alignment: every reported total includes 256 B of slack, and the launcher aligns the pointer
 *      up to 256 B itself;
 *   3. the contents do not matter: no launch needs a zeroed (or otherwise prepared) workspace, and the results have the same
 *      bits whatever it held.
 * A size below the query's is refused with SIGSVGD_E_WORKSPACE (sigsvgd_last_error names the required bytes) before any
 * device work: nothing is enqueued and no output is written.  A query of 0 bytes: the launch takes workspace = NULL.
 * tests/test_gpu_workspace.py holds this for every launch form (exact size, misaligned, poisoned, between guard areas). */

/* Bytes of scratch the two Gram entry points need for this problem.  Forward-only launches need some too
 * (accumulation buffers, scratch of the persistent grids), so always query.  The size is the largest of the launches the
 * arguments can reach: with SIGSVGD_FLAG_Y_IS_X and A == B the symmetric launch and (want_grad = 1) the symmetric partial
 * solve of the shape; otherwise the ordered launch and, when A == B, the symmetric one -- either value of
 * SIGSVGD_FLAG_SYM.  `static_kind` and `flags` are the ones of the launch
 * (ABI 9: the static kernel decides which solver runs -- the linear kernel always takes the coverage kernel --, so the
 * query needs it; ABI <= 8 sized for RBF whatever the launch asked for).
 * want_grad = 0 for sigsvgd_gram_fwd, 1 for sigsvgd_gram_fwd_bwd.  Returns 0 and sets *bytes. */
/* (flags with SIGSVGD_FLAG_EXACT_ADJOINT: SIGSVGD_E_UNSUPPORTED -- the fused kernels have the GG gradient only; see the flag.) */
int sigsvgd_gram_workspace_bytes(int A, int B, int T, int d, int dyadic_order, int static_kind, int want_grad,
                                 unsigned flags, size_t *bytes);

/* K_out[A,B] = signature-kernel Gram matrix of paths X[A,T,d], Y[B,T,d]. */
int sigsvgd_gram_fwd(const void *X, const void *Y, int A, int B, int T, int d, int dtype,
                     double inv_h, int dyadic_order, int static_kind, unsigned flags,
                     void *K_out, void *workspace, size_t workspace_bytes, void *stream);

/* As above, plus gradX_out[A,T,d] = d( sum_ij grad_out[i,j] K[i,j] ) / dX  (first slot only;
 * Y receives no gradient, as in the reference).  grad_out == NULL means all ones (the only case
 * the reference produces: callers differentiate K.sum()). */
/* SIGSVGD_FLAG_EXACT_ADJOINT: SIGSVGD_E_UNSUPPORTED before any device work (GG kernels only on this route; the long-path entry
 * points below take it). */
int sigsvgd_gram_fwd_bwd(const void *X, const void *Y, int A, int B, int T, int d, int dtype,
                         double inv_h, int dyadic_order, int static_kind, unsigned flags,
                         const void *grad_out, void *K_out, void *gradX_out, void *workspace,
                         size_t workspace_bytes, void *stream);

/* Multi-GPU building block (particles sharded over ranks; new design, the reference has no
 * distributed code -- SURVEY.md §8e).  Solves the unordered pairs {i <= j} whose row tile
 * (sigsvgd_gram_sym_tile_rows(T, d) consecutive rows i) has index tile_offset + k*tile_stride for some k >= 0
 * -- with SIGSVGD_FLAG_FOLD_TILES also the mirror images of those tiles, see the flag -- on the full gathered
 * particle tensor X[N,T,d]:
 *   K_partial[N,N]      (dtype)  caller-ZEROED; receives both orientations K[i,j], K[j,i] of every owned pair
 *   grad_partial[N,T,d] (fp64)   OVERWRITTEN with this launch's share of d sum(grad_out*K)/dX (row- and
 *                                column-side; rows the owned pairs do not touch get 0)
 * Summing the buffers over tile_offset = 0..tile_stride-1 gives sigsvgd_gram_fwd_bwd's outputs (K exactly, the
 * gradient up to the fp64 rounding of the sum).  Shapes of the register-resident and quadrant kernels
 * (dyadic_order 0, 3 <= T <= 128, d <= 16, RBF, no SIGSVGD_FLAG_NAIVE_SOLVER / SIGSVGD_FLAG_FORCE_GENERIC).
 * `workspace` as sized by sigsvgd_gram_workspace_bytes(N, N, T, d, 0, static_kind, 1, SIGSVGD_FLAG_Y_IS_X). */
/* SIGSVGD_FLAG_EXACT_ADJOINT: SIGSVGD_E_UNSUPPORTED before any device work (GG kernels only). */
int sigsvgd_gram_sym_partial(const void *X, int N, int T, int d, int dtype, double inv_h,
                             int static_kind, unsigned flags, int tile_offset, int tile_stride,
                             const void *grad_out, void *K_partial, double *grad_partial,
                             void *workspace, size_t workspace_bytes, void *stream);

/* Rows per tile of the symmetric / partial solve for paths of T points in d channels: 4 for T <= 64 with d > 8, else 8
 * (0 for shapes sigsvgd_gram_sym_partial does not take).  The unit of ownership of the sharded solve. */
int sigsvgd_gram_sym_tile_rows(int T, int d);

/* v_out[N,D] = -((K[N,N] @ score[N,D] - grad_k[N,D]) / N) * (mask ? mask[N,D] : 1)   (fp32)
 * If X_in and X_out are non-NULL additionally X_out = X_in - lr * v_out (optimizer=None update).
 * The N x N x D product runs on the fp32 MFMA (exact fp32 FMA chain). */
int sigsvgd_svgd_phi(const float *K, const float *score, const float *grad_k, const float *mask,
                     int N, int D, float *v_out, const float *X_in, float *X_out, float lr,
                     void *stream);

/* The same launch with the reference's "simple Adagrad" (SVGD(adaptive_gradient=True), svgd.py:110-113)
 * fused into the epilogue when adagrad_state[N,D] is non-NULL:
 *   state += v^2;  v_out = v / sqrt(state + 1e-12);  X_out = X_in - lr * v_out
 * (v already multiplied by the mask).  adagrad_state is read and written in place; zero it before the
 * first iteration.  With adagrad_state == NULL this is sigsvgd_svgd_phi. */
int sigsvgd_svgd_step(const float *K, const float *score, const float *grad_k, const float *mask,
                      int N, int D, float *v_out, const float *X_in, float *X_out, float lr,
                      float *adagrad_state, void *stream);

/* The same launch with torch.optim.Adam's update (amsgrad=False, weight_decay=0, maximize=False) in the epilogue:
 *   t = *step_dev + 1;  m = m + (1-beta1)(v - m);  q = beta2 q + (1-beta2) v^2;
 *   X_out = X_in - lr/(1-beta1^t) * m / (sqrt(q)/sqrt(1-beta2^t) + eps);   then *step_dev = t
 * exp_avg (m) and exp_avg_sq (q) are [N,D] fp32, updated in place; step_dev is an int on the DEVICE (the bias
 * corrections are formed in the kernel, so the launch can be replayed from a captured HIP graph); it is
 * incremented by a one-thread launch behind the update.  lr, beta1, beta2 and eps are doubles as torch holds them
 * (1 - beta and the bias corrections are formed in fp64 and rounded once, as torch does).  v_out receives the velocity (what the reference stores
 * in X.grad and in iter_dict["grad"]). */
int sigsvgd_svgd_adam_step(const float *K, const float *score, const float *grad_k, const float *mask,
                           int N, int D, float *v_out, const float *X_in, float *X_out, double lr, double beta1,
                           double beta2, double eps, float *exp_avg, float *exp_avg_sq, int *step_dev, void *stream);

/* The update rules of the three launches above on a velocity the caller ALREADY HAS, v_in[N,D] = -((K @ score - grad_k)/N)
 * (what sigsvgd_svgd_phi writes without a mask): the particle-sharded step, whose velocity is a sum over ranks, applies
 * mask, Adagrad and Adam -- none of them linear -- to its own rows after the reduction.  One elementwise launch, the same
 * device function as the fused epilogues, so the results have their bits:
 *   v = v_in * (mask ? mask : 1)
 *   adagrad_state != NULL:  state += v^2;  v = v / sqrt(state + 1e-12)            (sigsvgd_svgd_step)
 *   v_out (may be NULL) = v      -- the velocity after mask and Adagrad, what sigsvgd_svgd_step writes to v_out
 *   exp_avg != NULL:        torch.optim.Adam's update of X along v, the counter on the device and incremented by a
 *                           one-thread launch behind the update                    (sigsvgd_svgd_adam_step)
 *   else, X given:          X_out = X_in - lr * v
 * X_in and X_out are given both or neither and may be the same buffer, as may v_in and v_out (every element is read and
 * then written by the same thread).  Adam needs exp_avg, exp_avg_sq, step_dev and X (any one of the three state pointers
 * asks for Adam), with beta1, beta2 in [0, 1) and eps >= 0; Adam together with adagrad_state is an error, as is a call
 * with nothing to write (v_out, X_out and the state all NULL): SIGSVGD_E_BADARG, before any device work.  beta1, beta2
 * and eps are ignored without Adam.  16-byte accesses where D % 4 == 0 and every pointer is 16-byte aligned. */
int sigsvgd_svgd_update(const float *v_in, const float *mask, int N, int D, float *v_out, const float *X_in,
                        float *X_out, double lr, float *adagrad_state, float *exp_avg, float *exp_avg_sq,
                        int *step_dev, double beta1, double beta2, double eps, void *stream);

/* ---- vector kernels on particles X[A,D], Y[B,D] ---------------------------------
 * sq[i,j] = max(0, sum_c (XM[i,c] - YM[j,c]) * (X[i,c] - Y[j,c])).  XM = X @ M, YM = Y @ M for a metric
 * M[D,D] (scaled_pw_dist_sq); XM = YM = NULL means M = I, i.e. |x_i - y_j|^2 (pw_dist_sq).  Arithmetic
 * in `dtype`.  Differences are formed directly, so sq >= 0 up to rounding and the clamp is a no-op. */
int sigsvgd_vec_sqdist(const void *X, const void *Y, const void *XM, const void *YM, int A, int B, int D,
                       int dtype, void *sq_out, void *stream);

/* From sq[A,B]:  K_out[i,j] = f(sq[i,j])  (kind: SIGSVGD_VEC_GAUSSIAN / SIGSVGD_VEC_IMQ, inv_h2 = 1/h^2)
 * and, if dK_out != NULL,
 *   dK_out[i,c] = grad_scale * sum_j (grad_out ? grad_out[i,j] : 1) * w(sq[i,j]) * (XM[i,c] - YM[j,c]),
 * w = f for the Gaussian, f^3 = (1 + sq/(2h^2))^(-3/2) for the IMQ: the reference's `d_K.sum(1)`
 * with grad_scale = -1/h^2 (Gaussian kernels), +1/(2h^2) (IMQKernel: its (Y - X) sign convention,
 * _kernels.py:232) or -1/(2h^2) (ScaledIMQKernel, _kernels.py:297).  For M = I pass XM = X, YM = Y.
 * K_out may be NULL when only the gradient is wanted (it must be with SIGSVGD_VEC_UNIT). */
int sigsvgd_vec_kernel(const void *sq, const void *XM, const void *YM, const void *grad_out, int A, int B,
                       int D, int dtype, int kind, double inv_h2, double grad_scale, void *K_out,
                       void *dK_out, void *stream);

/* The same in ONE launch when the bandwidth is known in advance (no sq[A,B] round trip through HBM; both
 * GEMM-shaped sums on the fp32 matrix cores).  X, Y [.,D]; XM, YM = X M, Y M or both NULL (M = I); K_out / dK_out
 * nullable (not both).  fp32 and D <= 512 only (else SIGSVGD_E_UNSUPPORTED: use the two calls above).  Operands
 * are centred on the first row of Y (differences are unchanged); dK_out is fully overwritten. */
int sigsvgd_vec_kernel_fused(const void *X, const void *Y, const void *XM, const void *YM, const void *grad_out, int A,
                             int B, int D, int dtype, int kind, double inv_h2, double grad_scale, void *K_out,
                             void *dK_out, void *workspace, size_t workspace_bytes, void *stream);
/* Scratch for the reproducible route of sigsvgd_vec_kernel_fused (ABI 9): the launch splits the columns over the grid, and
 * with a workspace of this size every split stores its partial dK in a block of its own, added in split order by a second
 * small launch -- bits that depend on the launch geometry only.  workspace = NULL keeps the one-launch route whose splits
 * meet in fp32 atomics (last bits of dK_out may differ between calls).  0 bytes: a single split, nothing to join.
 * Otherwise splits * A * D * 4 bytes and the 256 B of alignment slack (the launcher aligns the pointer up, as everywhere). */
int sigsvgd_vec_fused_workspace_bytes(int A, int B, int D, size_t *bytes);

/* ---- trajectory cost in front of the path -----------------------------------------------
 * The reference's planning cost, examples/script_planning_obstacle_field.py:113-126, with its analytic gradient:
 *   knots_i = [start, x_i[0..knots-1], target]  ->  traj_i = basis[samples, knots+2] @ knots_i   (natural cubic
 *   spline samples for fixed knot times, :18-23; pass the identity for use_splines=False)
 *   cost_i  = w_obstacle * sum_t p(traj_i[t]) + || w_length * (traj_i[1:] - traj_i[:-1]) ||_F
 *   p(z)    = sum_m exp(log_weights[m]) prod_c Normal(z_c; mean[m,c], std[m,c])   (the script's obstacle field, :363-370)
 * Outputs: cost[N], traj[N,samples,d] (nullable), grad_x[N,knots,d] = d cost_i / d x_i (nullable; samples <= 128).
 * All fp32; d <= 16, knots + 2 <= 64, samples <= 1024. */
int sigsvgd_obstacle_cost(const float *x, int N, int knots, int d, const float *start, const float *target,
                          const float *basis, int samples, const float *log_weights, const float *mean, const float *std,
                          int components, float w_obstacle, float w_length, float *cost, float *traj, float *grad_x,
                          void *stream);

/* ---- truncated path signature ----------------------------------------------------
 * out[N, C + C^2 + ... + C^depth] = signature of the piecewise-linear path X[N,L,C] (levels
 * concatenated, each level row-major), with a zero point prepended when basepoint != 0.  Chen's
 * identity, fp64 accumulation, I/O in `dtype`.  *channels (if non-NULL) receives the output width;
 * with out == NULL only that query is performed. */
int sigsvgd_signature(const void *X, int N, int L, int C, int depth, int basepoint, int dtype, void *out,
                      long long *channels, void *stream);

/* grad_X[N,L,C] = d( sum_{n,e} grad_sig[n,e] * signature(X)[n,e] ) / dX: the adjoint of sigsvgd_signature for the same
 * (depth, basepoint).  grad_sig is [N, channels]; fp64 arithmetic (the signature is rebuilt forwards, then unwound point by
 * point with the group inverse exp(-increment): nothing per point is stored), I/O in `dtype`.  depth <= 8 and
 * 6 * channels doubles of LDS (channels <= ~3000), else SIGSVGD_E_UNSUPPORTED. */
int sigsvgd_signature_backward(const void *X, const void *grad_sig, int N, int L, int C, int depth, int basepoint, int dtype,
                               void *grad_X, void *stream);

/* ---- signature PDE on a caller's static-kernel grid (ABI 10; user static kernels) -----------------
 * Replaces the PDE part of sigkernel.SigKernel.compute_Gram / compute_kernel for a static kernel the library does not
 * evaluate itself: the caller passes the static kernel's values G[npairs][M][N] (contiguous, fp32 or fp64 by `dtype`;
 * Gram_matrix(X, Y) -> [A, B, M, N] is A*B pairs, batch_kernel(X, Y) -> [A, M, N] is A pairs; M != N allowed).  Per pair:
 * the 4-corner increments D[a][b] = G[a+1][b+1] + G[a][b] - G[a+1][b] - G[a][b+1] in fp64 (fp32 input too), refined to
 * g[p][q] = D[p >> n][q >> n] / r^2 on the P x Q grid (r = 2^dyadic_order, P = r (M-1), Q = r (N-1)), one Goursat sweep
 * in fp64 with the second-order stencil (SIGSVGD_FLAG_NAIVE_SOLVER: the first-order one):
 *   K_out[pair] = sol[P][Q]
 * and, sigsvgd_pde_fwd_bwd, dG_out[pair][M][N] = d( sum_pair grad_out[pair] K[pair] ) / dG in the reference's convention
 * (exact for the naive stencil; the one the built-in kernels return): GG[p][q] = K_fwd[p][q] K_rev[p+1][q+1],
 * S[a][b] = r^-2 sum of GG over block (a, b), dG[m][n] = grad_out (S[m-1][n-1] + S[m][n] - S[m-1][n] - S[m][n-1]), S = 0
 * outside.  grad_out == NULL means ones.  The stored forward solution and S are fp32, the sweeps fp64.
 * Any flag bit other than SIGSVGD_FLAG_NAIVE_SOLVER is SIGSVGD_E_BADARG.  P and Q up to 8192 (upstream's GPU path takes
 * P + 1, Q + 1 <= 1023); beyond that SIGSVGD_E_UNSUPPORTED.  Bit-reproducible (no floating-point atomics).
 * The workspace is sized by the resident wavefronts, not by npairs (one pair per wavefront; forward-only launches need
 * none and report 0 bytes); want_grad = 1 for sigsvgd_pde_fwd_bwd. */
/* flags: SIGSVGD_FLAG_NAIVE_SOLVER, and for sigsvgd_pde_fwd_bwd and its query (want_grad = 1) SIGSVGD_FLAG_EXACT_ADJOINT: dG_out
 * is then the exact derivative of the discrete K_out in G for the default stencil too.  K_out is
 * bit-identical to the unflagged launch and the workspace the same bytes; together with SIGSVGD_FLAG_NAIVE_SOLVER the launch is
 * the unflagged one.  sigsvgd_pde_fwd and the query with want_grad = 0 refuse the bit like any unknown one (SIGSVGD_E_BADARG). */
int sigsvgd_pde_workspace_bytes(int npairs, int M, int N, int dyadic_order, int want_grad, unsigned flags, size_t *bytes);
int sigsvgd_pde_fwd(const void *G, int npairs, int M, int N, int dtype, int dyadic_order, unsigned flags, void *K_out,
                    void *workspace, size_t workspace_bytes, void *stream);
int sigsvgd_pde_fwd_bwd(const void *G, int npairs, int M, int N, int dtype, int dyadic_order, unsigned flags,
                        const void *grad_out, void *K_out, void *dG_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- long paths with the built-in static kernels (added in ABI 10) --------------------------------
 * The same K[A,B] and gradX[A,TX,d] = d sum(grad_out*K)/dX (first argument only) as sigsvgd_gram_fwd / sigsvgd_gram_fwd_bwd,
 * for the launches those refuse with SIGSVGD_E_UNSUPPORTED: paths whose per-pair tables outgrow the LDS (from about T = 250
 * at dyadic order 0, and refined grids such as T = 200 at order 2).  X [A,TX,d] and Y [B,TY,d] keep their own lengths.
 * The static kernel (SIGSVGD_STATIC_RBF or _LINEAR) is evaluated inside the kernel, in fp64, and its 4-corner increments are
 * formed as the sweep needs them: nothing of size A*B*TX*TY exists.  Increments, sweeps and the gradient are fp64; the stored
 * forward solution and the block sums S are fp32 (per-wave scratch).  Backward in the reference's GG convention, as
 * sigsvgd_pde_fwd_bwd, chained through dk/dx.  Every ordered pair (i, j) is solved (sigsvgd_gram_long_fwd_bwd2 below solves
 * Y = X once per unordered pair, and gives the gradient of Y).
 * Flags: SIGSVGD_FLAG_NAIVE_SOLVER; SIGSVGD_FLAG_SYM (weights grad_out + grad_out^T, needs A == B and TX == TY);
 * SIGSVGD_FLAG_Y_IS_X is accepted and has no effect; any other bit is SIGSVGD_E_BADARG.  Limits: P = 2^n (TX-1) and
 * Q = 2^n (TY-1) up to 8192, and the per-wave LDS (boundary row of Q + 2 doubles, 64 KB of increments, the band's points)
 * within 160 KB; beyond them SIGSVGD_E_UNSUPPORTED.  Bit-reproducible: each work item (i, chunk of columns) adds its pairs
 * into its own gradient slab in j order and the slabs are summed in a fixed order; no floating-point atomics.
 * Workspace: per-wave scratch of 2 x P x (Q + 63) floats for the resident wavefronts (at most 1 GiB, fewer waves beyond)
 * plus A x ceil(B / JC) x TX x d doubles of slabs; forward-only launches need none and report 0 bytes. */
int sigsvgd_gram_long_workspace_bytes(int A, int B, int TX, int TY, int d, int dyadic_order, int static_kind, int want_grad,
                                      unsigned flags, size_t *bytes);
int sigsvgd_gram_long_fwd(const void *X, const void *Y, int A, int B, int TX, int TY, int d, int dtype, double inv_h,
                          int dyadic_order, int static_kind, unsigned flags, void *K_out, void *workspace,
                          size_t workspace_bytes, void *stream);
/* sigsvgd_gram_long_fwd_bwd (and the query with want_grad = 1) takes SIGSVGD_FLAG_EXACT_ADJOINT: gradX_out is the exact
 * derivative of the discrete K_out (every static kernel); K_out is bit-identical to the unflagged launch,
 * the workspace the same bytes, and with SIGSVGD_FLAG_NAIVE_SOLVER the launch is the unflagged one.  sigsvgd_gram_long_fwd and the
 * query with want_grad = 0: SIGSVGD_E_BADARG, as for any unknown bit. */
int sigsvgd_gram_long_fwd_bwd(const void *X, const void *Y, int A, int B, int TX, int TY, int d, int dtype, double inv_h,
                              int dyadic_order, int static_kind, unsigned flags, const void *grad_out, void *K_out,
                              void *gradX_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- paired signature kernels with the built-in static kernels (ABI 10) -------------------------
 * Replaces sigkernel.SigKernel.compute_kernel(X, Y) -> [A]: K_out[i] = k_sig(X_i, Y_i) for X [A,TX,d] and Y [A,TY,d]
 * (TX != TY allowed; X and Y may be the same buffer), A solves instead of the A*A of a Gram launch.  It is the paired mode
 * of the long-path kernel: the same fp64 static kernel, increments and sweeps, so K_out[i] is bit-identical to
 * sigsvgd_gram_long_fwd(X_i, Y_i), and the same limits (P, Q up to 8192, per-wave LDS within 160 KB; beyond them
 * SIGSVGD_E_UNSUPPORTED).  sigsvgd_pair_fwd_bwd: from the one reverse sweep of each pair (the reference's GG convention,
 * as sigsvgd_gram_long_fwd_bwd), with w = grad_out (NULL = ones),
 *   gradX_out[i][m] = w_i sum_n dG[m][n] dk(x_m, y_n)/dx_m     and     gradY_out[i][n] = w_i sum_m dG[m][n] dk(x_m, y_n)/dy_n,
 * each in the I/O dtype; either may be NULL (not both).  Flags: SIGSVGD_FLAG_NAIVE_SOLVER only; any other bit, both
 * gradient outputs NULL, bad shapes, kinds, orders, dtypes, inv_h <= 0 with RBF or null pointers are SIGSVGD_E_BADARG.
 * One pair per wavefront, each gradient entry written by one lane in a fixed order: bit-reproducible, no floating-point
 * atomics.  Workspace: per-wave scratch of 2 x P x (Q + 63) floats for min(resident wavefronts, A) waves (at most 1 GiB,
 * fewer waves beyond); forward-only launches need none and report 0 bytes.
 *
 * Schedule (third revision of ABI 10, additive): where a pair has enough 64-row bands for it to pay
 * (the rule counts both schedules' dependent steps over the rounds the launch takes), each pair gets a workgroup of up to 8
 * wavefronts that sweep the pair's bands as a pipeline (pair_bands.hip).  Same arithmetic per cell in the same order: K and both gradients are
 * bit-identical to the one-wavefront schedule, and the workspace is the same (fewer of its per-pair slots are used).
 * sigsvgd_pair_schedule (host only; the argument checks and refusals of sigsvgd_pair_workspace_bytes) reports what a launch
 * with these arguments would run now, SIGSVGD_PAIR_MODE included: wavefronts per pair (1: the one-wavefront kernel), the
 * grid, and the LDS bytes of a workgroup. */
int sigsvgd_pair_workspace_bytes(int A, int TX, int TY, int d, int dyadic_order, int static_kind, int want_grad,
                                 unsigned flags, size_t *bytes);
/* SIGSVGD_FLAG_EXACT_ADJOINT (sigsvgd_pair_fwd_bwd, and the queries with want_grad = 1): gradX_out and gradY_out are the exact
 * derivatives of the discrete K_out; K_out is bit-identical to the unflagged launch and the workspace the same bytes.  The
 * launch runs one wavefront per pair whatever the shape (the band-parallel kernel has the GG sweep only), and
 * sigsvgd_pair_schedule reports waves_per_pair = 1 with the bit.  With SIGSVGD_FLAG_NAIVE_SOLVER the launch -- and the schedule
 * reported -- is the unflagged one.  sigsvgd_pair_fwd and the queries with want_grad = 0: SIGSVGD_E_BADARG. */
int sigsvgd_pair_schedule(int A, int TX, int TY, int d, int dyadic_order, int static_kind, int want_grad, unsigned flags,
                          int *waves_per_pair, int *grid, size_t *lds_bytes);
int sigsvgd_pair_fwd(const void *X, const void *Y, int A, int TX, int TY, int d, int dtype, double inv_h,
                     int dyadic_order, int static_kind, unsigned flags, void *K_out, void *workspace,
                     size_t workspace_bytes, void *stream);
int sigsvgd_pair_fwd_bwd(const void *X, const void *Y, int A, int TX, int TY, int d, int dtype, double inv_h,
                         int dyadic_order, int static_kind, unsigned flags, const void *grad_out /* [A] or NULL = ones */,
                         void *K_out, void *gradX_out /* may be NULL */, void *gradY_out /* may be NULL */,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---- long-path Gram, both slots and Y = X (ABI 10, additive) ---------------------------------------
 * The two-sided launch of the long-path kernel: the K[A,B] of sigsvgd_gram_long_fwd, bit for bit, and from each pair's one
 * reverse sweep
 *   gradX_out[i][m] = sum_j w_ij sum_n dG_ij[m][n] dk(x_im, y_jn)/dx_im     (first slot, as sigsvgd_gram_long_fwd_bwd)
 *   gradY_out[j][n] = sum_i w_ij sum_m dG_ij[m][n] dk(x_im, y_jn)/dy_jn     (second slot, the same GG convention),
 * w = grad_out (NULL = ones).  Either output may be NULL; both NULL is a forward-only launch.
 * SIGSVGD_FLAG_Y_IS_X (A == B, TX == TY, gradY_out == NULL; the caller guarantees Y holds X's values): only the pairs i <= j
 * are solved, K_out[j][i] is a copy of K_out[i][j], and gradX_out is the first-slot gradient of the ordered launch: pair
 * (i, j), i < j, gives w_ij d1 k(X_i, X_j) to row i and w_ji d2 k(X_i, X_j) = w_ji d1 k(X_j, X_i) to row j.
 * SIGSVGD_FLAG_SYM (A == B, TX == TY, gradY_out == NULL): weights w_ij + w_ji.  SIGSVGD_FLAG_NAIVE_SOLVER as elsewhere;
 * any other bit is SIGSVGD_E_BADARG.  Limits and refusals are sigsvgd_gram_long_fwd's.
 * Work items are tiles of IC rows x JC columns (with Y_IS_X: the tiles of the upper triangle); a tile adds its pairs into
 * one fp64 slab per row and one per column in a fixed order, and the slabs of a row (a column) are summed in tile order:
 * bit-reproducible, no floating-point atomics.  Workspace: the per-wave scratch of sigsvgd_gram_long_fwd_bwd plus at most
 * (A ceil(B / JC) TX + B ceil(A / IC) TY) d doubles of slabs; forward-only launches need none and report 0 bytes. */
int sigsvgd_gram_long2_workspace_bytes(int A, int B, int TX, int TY, int d, int dyadic_order, int static_kind,
                                       int want_gradX, int want_gradY, unsigned flags, size_t *bytes);
/* SIGSVGD_FLAG_EXACT_ADJOINT (with a gradient output, and the query with want_gradX or want_gradY): gradX_out and gradY_out are
 * the exact derivatives of the discrete K_out, with SIGSVGD_FLAG_Y_IS_X, SIGSVGD_FLAG_SYM and weights as without it; K_out is
 * bit-identical to the unflagged launch, the workspace the same bytes; with SIGSVGD_FLAG_NAIVE_SOLVER the launch is the
 * unflagged one.  Forward only (both outputs NULL / neither wanted): SIGSVGD_E_BADARG. */
int sigsvgd_gram_long_fwd_bwd2(const void *X, const void *Y, int A, int B, int TX, int TY, int d, int dtype, double inv_h,
                               int dyadic_order, int static_kind, unsigned flags, const void *grad_out, void *K_out,
                               void *gradX_out /* may be NULL */, void *gradY_out /* may be NULL */, void *workspace,
                               size_t workspace_bytes, void *stream);

/* ---- long-path route, derivative in the static kernel's bandwidth (ABI 10, additive) --------------
 * sigsvgd_gram_long_fwd_bwd2 and sigsvgd_pair_fwd_bwd with one more output: for the static kernels k = phi(|x - y|^2 inv_h)
 * (SIGSVGD_STATIC_RBF, _IMQ, _RQ) every pair's derivative of K in inv_h, from the pair's one reverse sweep,
 *   dK_dinvh_out[i][j] = - sum_{m,n} R_ij[m][n] slope(dist inv_h) dist,     dist = |x_im - y_jn|^2,
 * with R = dG / w the 4-corner scatter of the pair's S and slope = -phi' (exp(-s) for RBF, k^3 / 2 for IMQ, k^2 for the
 * rational quadratic kernel): the contraction of the coordinate gradients with the scalar dist in place of (x - y).  It is the
 * reference's GG convention chained exactly through the static kernel (the exact derivative of K for the first-order stencil;
 * for the default stencil GG is not the exact adjoint, and the value differs from a finite difference of K by per cents, as
 * the coordinate gradients do).  dK / d sigma = -inv_h^2 dK / d inv_h for k(x, y) = phi(|x - y|^2 / sigma).
 * dK_dinvh_out is required, [A][B] (sigsvgd_gram_long_fwd_bwd_h) or [A] (sigsvgd_pair_fwd_bwd_h) in the I/O dtype, and is
 * unweighted: grad_out and SIGSVGD_FLAG_SYM weight the coordinate gradients only.  With SIGSVGD_FLAG_Y_IS_X the pair (i, j),
 * i <= j, stores its value at [i][j] and [j][i], as K's mirror does.  gradX_out and gradY_out may both be NULL: the launch
 * still runs the reverse sweep and needs the per-wave scratch, and no slabs.  K_out and the gradients returned are
 * bit-identical to those of sigsvgd_gram_long_fwd_bwd2 / sigsvgd_pair_fwd_bwd on the same arguments.  The paired launch always
 * runs the one-wavefront schedule.  Lanes own points of X and add their terms in fp64; a fixed-shape reduction over the
 * wavefront and a fixed order over the passes of 63 points follow, and one lane stores the pair's value: bit-reproducible, no
 * floating-point atomics.
 * SIGSVGD_E_BADARG: SIGSVGD_STATIC_LINEAR (it has no bandwidth), dK_dinvh_out == NULL, inv_h <= 0, unknown flag bits, and what
 * the launches without the output refuse; limits and SIGSVGD_E_UNSUPPORTED are theirs too (SIGSVGD_FLAG_NAIVE_SOLVER: RBF
 * only).  Workspace: sigsvgd_gram_long_h_workspace_bytes = the scratch plus the slabs of the gradients wanted (what
 * sigsvgd_gram_long2_workspace_bytes reports where one is wanted; the scratch alone where neither is);
 * sigsvgd_pair_h_workspace_bytes = sigsvgd_pair_workspace_bytes with the gradient. */
/* SIGSVGD_FLAG_EXACT_ADJOINT (both launches and both queries): gradX_out, gradY_out and dK_dinvh_out are the exact derivatives of
 * the discrete K_out -- dK_dinvh_out then agrees with a finite difference of K_out in inv_h, which the GG value misses by per
 * cents; K_out is bit-identical to the unflagged launch, the workspace the same bytes; with SIGSVGD_FLAG_NAIVE_SOLVER the launch
 * is the unflagged one. */
int sigsvgd_gram_long_h_workspace_bytes(int A, int B, int TX, int TY, int d, int dyadic_order, int static_kind,
                                        int want_gradX, int want_gradY, unsigned flags, size_t *bytes);
int sigsvgd_gram_long_fwd_bwd_h(const void *X, const void *Y, int A, int B, int TX, int TY, int d, int dtype, double inv_h,
                                int dyadic_order, int static_kind, unsigned flags, const void *grad_out, void *K_out,
                                void *gradX_out /* may be NULL */, void *gradY_out /* may be NULL */,
                                void *dK_dinvh_out /* [A][B], required */, void *workspace, size_t workspace_bytes,
                                void *stream);
int sigsvgd_pair_h_workspace_bytes(int A, int TX, int TY, int d, int dyadic_order, int static_kind, unsigned flags,
                                   size_t *bytes);
int sigsvgd_pair_fwd_bwd_h(const void *X, const void *Y, int A, int TX, int TY, int d, int dtype, double inv_h,
                           int dyadic_order, int static_kind, unsigned flags, const void *grad_out /* [A] or NULL = ones */,
                           void *K_out, void *gradX_out /* may be NULL */, void *gradY_out /* may be NULL */,
                           void *dK_dinvh_out /* [A], required */, void *workspace, size_t workspace_bytes, void *stream);

/* ---- long-path Gram, one rank's share of the Y = X solve (ABI 10, additive) -----------------------
 * The partial mode of the two-sided Y-is-X launch, for the sharded SVGD step: the launch of rank tile_offset of tile_stride
 * owns the row tiles tile_offset + k tile_stride of tile_rows rows each -- with SIGSVGD_FLAG_FOLD_TILES also their mirror
 * images ntile - 1 - t (the ownership of sigsvgd_gram_sym_partial) -- and a row tile owns the pairs (i, j), i in the tile,
 * j >= i.  For the owned pairs K_partial[i][j] = K_partial[j][i] = the K of sigsvgd_gram_long_fwd, bit for bit (I/O dtype;
 * entries of other pairs are not touched: the caller zeroes the buffer), and grad_partial [N, T, d], always fp64 and fully
 * overwritten (zero in rows that received nothing), holds the owned pairs' contributions to the first-slot gradient of
 * sigsvgd_gram_long_fwd_bwd2 with Y_IS_X: w_ij d1 k(X_i, X_j) to row i and w_ji d1 k(X_j, X_i) to row j, w = grad_out (NULL =
 * ones), SIGSVGD_FLAG_SYM: w_ij + w_ji.  Summed over tile_offset = 0 .. tile_stride - 1 they give that launch's K and
 * gradient.  SIGSVGD_FLAG_NAIVE_SOLVER as elsewhere; SIGSVGD_FLAG_Y_IS_X is implied; any other bit, tile_stride < 1 or
 * tile_offset outside [0, tile_stride) is SIGSVGD_E_BADARG.  Limits and refusals are sigsvgd_gram_long_fwd's.  A rank that
 * owns no tile (more ranks than tiles) is a valid launch: grad_partial is zeroed, K_partial not touched.
 * Work items are rectangles of tile_rows x tile_cols pairs of an owned row tile, from the tile's first row on;
 * sigsvgd_gram_long_partial_plan reports the two, which depend on (N, T, d, dyadic_order, tile_stride) and the device only,
 * never on tile_offset or the fold flag: every rank of a step has the same tiles.  An item adds its pairs into one fp64 slab
 * per row and one per column in a fixed order, and a row's slabs are summed in a fixed order: bit-reproducible, no
 * floating-point atomics.  Workspace (sigsvgd_gram_long_partial_workspace_bytes, per rank): the per-wave scratch of
 * sigsvgd_gram_long_fwd_bwd plus the slabs of the owned tiles only; 0 bytes for a rank without tiles.  The query is exact
 * per rank.  The tile is chosen for the folded ownership on the device's resident wavefronts: there a share's slabs are at
 * most N N / 4 x T d doubles where it holds more than 16 pairs per resident wavefront and (2 pairs + N) x T d doubles below,
 * and its schedule keeps at least 0.9 of the resident waves busy.  Cyclic ownership (its first rank owns more) and launches
 * whose grid the 1 GiB scratch cap lowers run on the same tile without those two guarantees. */
int sigsvgd_gram_long_partial_plan(int N, int T, int d, int dyadic_order, int static_kind, unsigned flags, int tile_stride,
                                   int *tile_rows, int *tile_cols);
int sigsvgd_gram_long_partial_workspace_bytes(int N, int T, int d, int dyadic_order, int static_kind, unsigned flags,
                                              int tile_offset, int tile_stride, size_t *bytes);
/* SIGSVGD_FLAG_EXACT_ADJOINT: SIGSVGD_E_UNSUPPORTED from the launch and from both queries above, before any device work (the
 * partial mode has the GG sweep only; the message names the flag). */
int sigsvgd_gram_long_sym_partial(const void *X, int N, int T, int d, int dtype, double inv_h, int dyadic_order,
                                  int static_kind, unsigned flags, int tile_offset, int tile_stride,
                                  const void *grad_out /* [N,N] or NULL = ones */, void *K_partial, double *grad_partial,
                                  void *workspace, size_t workspace_bytes, void *stream);

/* ---- order statistic of the point distances (ABI 10, additive) ------------------------------------
 * out_device[0] = the element of rank `rank` (zero-based, ascending) of the multiset
 *   { |X_ip - Y_jq|^2 : i < A, j < B, p < TX, q < TY },     n = A B TX TY elements,
 * X [A, TX, d], Y [B, TY, d] in `dtype`.  rank = (n - 1) / 2 is the lower median, which the reference's default bandwidth
 * takes of the [A, B, TX, TY] tensor (bw_median, src/utils/math.py:28-34); nothing of that size is stored here.  Each value
 * is computed in fp64 as sum_k (x_k - y_k)^2 in channel order (fp32 inputs converted exactly): never negative, and the same
 * bits for (i, j, p, q) and (j, i, q, p).  The select is exact on those values: counting passes over the 64-bit pattern, at
 * most six, each recomputing the distances until the remaining candidates fit a buffer in the workspace.  The state stays
 * on the device: no host synchronisation, no allocation, graph-capturable; integer counts only, so the result does not
 * depend on the order of arrival.  With non-finite inputs the call ends and returns some value.
 * SIGSVGD_FLAG_Y_IS_X (A == B, TX == TY; the caller guarantees Y holds X's values): each unordered pair of paths is visited
 * once and counted twice; the result is the unflagged call's, bit for bit.  Any other flag bit, a shape below 1, a bad
 * dtype, null pointers, rank >= n or n >= 2^63 are SIGSVGD_E_BADARG, a workspace below the query's size is
 * SIGSVGD_E_WORKSPACE, all before any device work.  The workspace (a constant size, independent of the shape) needs no
 * zeroing: the call clears its counters on the stream. */
int sigsvgd_sqdist_select_workspace_bytes(int A, int B, int TX, int TY, int d, unsigned flags, size_t *bytes);
int sigsvgd_sqdist_select(const void *X, const void *Y, int A, int B, int TX, int TY, int d, int dtype, unsigned flags,
                          unsigned long long rank, double *out_device, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGSVGD_HIP_H */
