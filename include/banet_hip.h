/* banet_hip.h -- C ABI of libbanet_hip.so: the MI355X (gfx950) bundle-adjustment hot path.
 *
 * This is the drop-in boundary for the one native component of frobelbest/BANet, the
 * TensorFlow custom-op library `utils.so` (reference: utils.cu, loaded by
 * bundlenet.py:76-82 and legacy/ba.py:11-13), plus fused entry points that replace the
 * TF-graph portion of the same path (bundlenet.py:122-278, legacy/ba.py:148-345).
 *
 * Conventions (all entry points):
 *   - plain C, no C++/torch types; every pointer is a DEVICE pointer owned by the caller;
 *   - row-major contiguous float32 tensors with the reference's axis order;
 *   - asynchronous: work is enqueued on the caller's hipStream_t; nothing synchronises,
 *     allocates or frees; scratch comes from the caller-supplied workspace `ws`
 *     (size from the matching *_workspace_bytes query; 256-byte aligned);
 *   - the workspace is pure scratch: on entry its contents are ARBITRARY (it need not be zeroed and
 *     may hold another call's leftovers -- one arena can be recycled by calls of any shape); no call
 *     reads a workspace byte it did not write itself, with one documented exception,
 *     BANET_ADJOINT_REUSE_DEPTH_SEED, which reads what the previous banet_dense_adjoint_ex_f32 call
 *     left; no call touches a byte outside [ws, ws + workspace_bytes); a NULL, misaligned or too
 *     small `ws` is BANET_ERR_WORKSPACE wherever the query is non-zero (the one optional workspace,
 *     banet_equation_construction_grad_f32's, selects the kernel that needs none instead);
 *   - stateless and re-entrant: no globals (the reference keeps per-GPU static scratch
 *     sized by the first call, utils.cu:214-216,259-264 -- not reproduced);
 *   - return value: BANET_OK or a negative BANET_ERR_* code; never throws.
 *   - deterministic: reductions use fixed-order partials, no float atomics.
 */
#ifndef BANET_HIP_H_
#define BANET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef BANET_STREAM_T
#define BANET_STREAM_T
typedef void* banet_stream_t; /* a hipStream_t (NULL = default stream) */
#endif

#define BANET_VERSION 150 /* 0.1.5: BANET_ADJOINT_FOLD_TARGET, banet_small_step_adjoint_f32; 0.1.4: banet_dense_adjoint_f32 / banet_target_map_adjoint_f32; 0.1.3: banet_lm_params_t / banet_lm_level_ex_f32 (0.1.2: banet_sample_stats[_grad]_f32; 0.1.1: banet_level_t.pairs) */

enum {
  BANET_OK = 0,
  BANET_ERR_INVALID_ARG = -1, /* null pointer, non-positive size, bad enum        */
  BANET_ERR_WORKSPACE = -2,   /* ws too small or misaligned                       */
  BANET_ERR_UNSUPPORTED = -3, /* shape outside the compiled kernel set (see docs) */
  BANET_ERR_LAUNCH = -4       /* hipGetLastError() != hipSuccess after enqueue    */
};

int banet_version(void);
const char* banet_error_string(int code);

/* ---------------------------------------------------------------------------------------
 * (1) EquationConstruction  -- replaces the TF op registered at utils.cu:150-171 and its
 *     kernel utils.cu:219-417 (5 cuBLAS sgemmBatched + 2 column reductions).
 *       jacobian   J [B,N,2,P]     gradient G [B,N,C,2]     difference d [B,N,C,1]
 *       left  AtA [B,P,P] = sum_n J_n^T (G_n^T G_n) J_n
 *       right Atb [B,P,1] = sum_n J_n^T  G_n^T d_n
 *     Never materialises the per-pixel PxP products (utils.cu:356-365 does: 22 GB/item at
 *     640x480, P=134).  Supported: 1 <= P <= 304, any C >= 1, any N >= 1 (all on the matrix-pipe kernels; 272 < P <= 304, cfg-5's P = 298: the 17-block pass + three jobs, round 5).
 * ------------------------------------------------------------------------------------- */
size_t banet_equation_construction_workspace_bytes(int B, int N, int C, int P);
int banet_equation_construction_f32(const float* jacobian, const float* gradient,
                                    const float* difference, float* left, float* right,
                                    int B, int N, int C, int P, void* ws, size_t ws_bytes,
                                    banet_stream_t stream);

/* (2) EquationConstructionGrad -- replaces utils.cu:420-428 (op) / :465-694 (kernel),
 *     bound as the op's gradient at bundlenet.py:79-82.
 *       left_grad g0 [B,P,P], right_grad g1 [B,P,1]
 *       A_n = G_n J_n ; dA_n = 2 A_n g0 + d_n g1^T   (alpha = 2.0 as utils.cu:651)
 *       jacobian_grad = G^T dA [B,N,2,P]; gradient_grad = dA J^T [B,N,C,2];
 *       difference_grad = A g1 [B,N,C,1]
 *     Workspace: optional.  With ws_bytes >= banet_equation_construction_grad_workspace_bytes (P <= 304, 256-byte
 *     aligned) the matrix-pipe kernels run; with ws = NULL (or for shapes whose size is 0) the first-generation
 *     kernel, same results to rounding.                                                   */
size_t banet_equation_construction_grad_workspace_bytes(int B, int N, int C, int P);
int banet_equation_construction_grad_f32(const float* jacobian, const float* gradient,
                                         const float* difference, const float* left_grad,
                                         const float* right_grad, float* jacobian_grad,
                                         float* gradient_grad, float* difference_grad, int B,
                                         int N, int C, int P, void* ws, size_t ws_bytes,
                                         banet_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Fused path.  One "level problem" = B independent windows at one pyramid level.
 * ------------------------------------------------------------------------------------- */
enum { /* banet_level_t.variant: which reference iteration is restated */
  BANET_LEGACY_LM = 0,     /* legacy/ba.py:226-345 CameraIteration2 (MLP, exponent 1+y,
                              N/sum(mask) scaling, QR, V, accept/reject)                  */
  BANET_LEGACY_FIXED = 1,  /* legacy/ba.py:148-214 CameraIteration (lambda=|avg|^2, no V)  */
  BANET_BUNDLE_CAMERA = 2, /* bundlenet.py:122-191 CameraIteration (pose only)            */
  BANET_BUNDLE = 3         /* bundlenet.py:193-278 BundleIteration (pose + depth basis)   */
};

/* banet_level_t.flags -- named overrides of the kernel / arithmetic-form selection (0 in production).  The BANET_FLAG_* bits are the
 * documented ones; every other bit is development A/B plumbing (tools/, profiles/) and must be 0 in a caller's code.
 *   BANET_FLAG_FORCE_PATCH_GATHER / _STRIP_GATHER / _QUAD_GATHER, BANET_FLAG_NO_QUAD_GATHER : run (never run) that C = 128 gather kernel
 *       at any launch size (parity tests compare the kernels at oracle sizes; banet_gather_selection reports what a level runs);
 *   BANET_FLAG_SYRK_F16 / BANET_FLAG_NO_SYRK_F16 : the arithmetic FORM of the depth-block contraction.  Default (neither bit): the LM loop
 *       (banet_lm_level_f32) runs the fp16 two-piece form -- fp32 operands as two scaled fp16 pieces, three products, ~2^-21 per
 *       product, <= 2e-7 per entry of the matrix's own scale; an absolute 2^-25 of the column bound for entries more than 17 octaves
 *       below it -- on throughput-bound launches (N * B >= 32 * 76 800 pixels; banet_level_t.policy decides whether B counts), and the
 *       exact form (three bf16 pieces, six products, fp32-exact) elsewhere; the single pass banet_ba_assemble_f32 always runs the
 *       exact form.  _SYRK_F16: the fp16 form at any launch size and in the single pass too; _NO_SYRK_F16: the exact form everywhere.
 *       banet_syrk_selection reports the form;
 *   BANET_FLAG_SYRK_THREE_PRODUCTS : OPT-IN, reduced precision -- the K = 128 depth-block contraction with the three largest
 *       bf16 products only (~2^-16 per product instead of fp32-exact).  Never the default, never what bench.py's `value`
 *       is measured with.
 * (Until round 4 this field was called `reserved_` and the bits BANET_DEV_*: same offset, same values.  The BANET_DEV_* ENUM names stay
 * as aliases; the STRUCT FIELDS were renamed -- `reserved_` -> `flags`, `pad_` -> `policy` -- which is source-breaking for a C / C++
 * caller that named them (binary layout unchanged; the Python ctypes mirror keeps a `reserved_` property).) */
enum {
  BANET_FLAG_FORCE_PATCH_GATHER = 1 << 9,
  BANET_FLAG_FORCE_STRIP_GATHER = 1 << 18,
  BANET_FLAG_FORCE_QUAD_GATHER = 1 << 25,   /* the 4x4-pixel-item gather of latency-bound launches, at any size */
  BANET_FLAG_NO_QUAD_GATHER = 1 << 30,      /* ... never (the tile kernels instead) */
  BANET_FLAG_SYRK_THREE_PRODUCTS = 1 << 29,
  BANET_FLAG_SYRK_F16 = 1 << 24,             /* the fp16 two-piece SYRK also in banet_ba_assemble_f32 and at any launch size */
  BANET_FLAG_NO_SYRK_F16 = (int)0x80000000,  /* ... never: the exact bf16 form everywhere */
  BANET_DEV_FORCE_PATCH_GATHER = BANET_FLAG_FORCE_PATCH_GATHER,
  BANET_DEV_FORCE_STRIP_GATHER = BANET_FLAG_FORCE_STRIP_GATHER,
  BANET_DEV_FORCE_QUAD_GATHER = BANET_FLAG_FORCE_QUAD_GATHER,
  BANET_DEV_NO_QUAD_GATHER = BANET_FLAG_NO_QUAD_GATHER,
  BANET_DEV_SYRK_THREE_PRODUCTS = BANET_FLAG_SYRK_THREE_PRODUCTS,
  BANET_DEV_SYRK_F16 = BANET_FLAG_SYRK_F16,
  BANET_DEV_NO_SYRK_F16 = BANET_FLAG_NO_SYRK_F16
};

/* banet_level_t.policy -- what the kernel / form selection may depend on.
 *   BANET_POLICY_THROUGHPUT (0, default): kernels, the SYRK form and the number of partial rows are chosen from the whole LAUNCH
 *       (N, K, pairs AND the batch B): fastest, and results are within rounding (<= 1e-5 relative on a solve, tested) of any other
 *       batching of the same windows -- but not bit-identical to them: a window solved in a batch of 8 and in a batch of 32 may run
 *       different gather kernels, SYRK forms and summation splits.
 *   BANET_POLICY_BATCH_INVARIANT (1): every such decision is taken from the LEVEL alone (N, K, pairs, as if B = BANET_CANONICAL_BATCH),
 *       so a window's bits do not depend on how many windows share its launch or on how a batch is sharded over GPUs (tested:
 *       batches of 1 / 8 / 32 bit-identical).  Small batches then run the kernels tuned for 32 windows: slower below ~8 windows.
 *       The reference has no such dependence either way (utils.cu:181-198 reduces per item).                                        */
enum { BANET_POLICY_THROUGHPUT = 0, BANET_POLICY_BATCH_INVARIANT = 1 };
#define BANET_CANONICAL_BATCH 32

typedef struct banet_level {
  int32_t B;            /* windows                                                        */
  int32_t N;            /* points per window                                              */
  int32_t C;            /* feature channels (C <= 256)                                    */
  int32_t K;            /* depth-basis coefficients; 0 for the pose-only variants; <= 256
                           (P = 6 pairs + K > ~190: the solve keeps its matrix in a workspace:
                           banet_lm_level_f32's, or banet_ba_solve_update_ws_f32's;
                           banet_ba_solve_update_f32 alone then returns BANET_ERR_UNSUPPORTED) */
  int32_t H, W;         /* target map height / width at this level                        */
  int32_t variant;      /* BANET_LEGACY_LM ... BANET_BUNDLE                               */
  int32_t dense;        /* 1: the N = H*W points are this level's own pixel grid          */
  int32_t tgt_has_grad; /* 1: target map is the reference's [f|gx|gy] 3C layout
                              (legacy/ba.py:116-118); 0: C channels, gradient computed in
                              the kernel from the map (same arithmetic as grad_fixed)      */
  int32_t normalize_rays; /* dense only: 1 = bundlenet.py:119, 0 = legacy/ba.py:33-34     */
  float scale;          /* dense only: level scale s (points, intrinsics = full-res / s)  */
  int32_t pairs;        /* target frames per window (F - 1); 0 or 1 = the reference's 2-frame
                           case.  pairs > 1 (bundle variants only) is the multi-frame window
                           of SURVEY.md 8(d): the key frame carries depth / basis / Wc, every
                           other frame its own pose; P = 6 pairs + K, parameter order
                           [pose_1 .. pose_pairs, depth]                                     */
  int32_t flags;        /* 0 in production; BANET_FLAG_* overrides of the kernel / arithmetic-form selection
                           (above); was `reserved_` until round 4 (same offset)                */
  int32_t policy;       /* BANET_POLICY_THROUGHPUT (0) or BANET_POLICY_BATCH_INVARIANT (1); was `pad_`,
                           which had to be 0: existing callers get the default                  */
  const float* src;     /* dense: source map [B,H,W,C];  sparse: conv1 [B,N,C]            */
  const float* tgt;     /* target maps [B,pairs,H,W,C] or [B,pairs,H,W,3C]                */
  const float* depth;   /* D  [B,N]   (legacy: z-depth; bundle: range along the ray)      */
  const float* basis;   /* Bs [B,N,K] or NULL when K == 0                                 */
  const float* rays;    /* sparse: p [B,3,N] (bundlenet.py:115-119); dense: NULL          */
  const float* fx;      /* sparse: per-point level intrinsics [B,N] each                  */
  const float* fy;
  const float* ox;
  const float* oy;
  const float* intr;    /* dense: full-resolution (fx,fy,ox,oy) per window [B,4]          */
} banet_level_t;

/* Five k=1 conv layers of the lambda predictor (bundlenet.py:168-172): filters [Cin,Cout]
 * row-major (the reference's [1,Cin,Cout] variable), biases [Cout]; C->2C->4C->2C->C->1. */
typedef struct banet_mlp {
  const float* w[5];
  const float* b[5];
} banet_mlp_t;

/* Per-window LM state carried across iterations and levels (device memory, caller-owned).
 *   R [B,pairs,9]  T [B,pairs,3]  Wc [B,K]   current estimate (input and output)
 *   iters [B] int32                 iterations executed at the current level
 *   ratio [B]                       legacy "keep ratio" (legacy/ba.py:214 / :344)
 *   lambda_out [B]                  last lambda (diagnostic)
 *   delta [B,P]                     last solved update (diagnostic / parity tests)       */
typedef struct banet_state {
  float* R;
  float* T;
  float* Wc;
  int32_t* iters;
  float* ratio;
  float* lambda_out;
  float* delta;
} banet_state_t;

/* (3) one fused assembly pass: warp -> sample -> residual/gradient -> Jacobians -> normal
 *     equations, for all B windows at the pose (R,T,Wc) -- replaces the TF graph of
 *     bundlenet.py:206-263 / legacy/ba.py:238-283 plus the EquationConstruction op.
 *       AtA [B,P,P], Atb [B,P]  (P = 6 pairs + K), absres [B,C] = sum over pairs and n of
 *       |d_nc|, nvalid [B] = sum over pairs of the in-image point counts                 */
size_t banet_ba_assemble_workspace_bytes(const banet_level_t* lv);
int banet_ba_assemble_f32(const banet_level_t* lv, const float* R, const float* T,
                          const float* Wc, float* AtA, float* Atb, float* absres,
                          float* nvalid, void* ws, size_t ws_bytes, banet_stream_t stream);
/* The same pass, additionally writing the in-image mask bit (bundlenet.py:155,231 / utils_python.py:61-117) the kernel decided
 * for every pixel: mask_out [B * pairs][N] bytes, 1 = in the image.  A parity diagnostic (bench.py's sweep gate compares it
 * bit by bit with the float64 oracle's mask, so that a float32-vs-float64 disagreement on a pixel sitting on the image border is
 * demonstrated, not assumed); same kernels, same sums.                                                                        */
int banet_ba_assemble_mask_f32(const banet_level_t* lv, const float* R, const float* T,
                               const float* Wc, float* AtA, float* Atb, float* absres, float* nvalid,
                               unsigned char* mask_out, void* ws, size_t ws_bytes, banet_stream_t stream);

/* (3b) residual evaluation: what the level costs at the state (R, T, Wc), per pixel -- the reference's CheckUpdate
 *     (legacy/ba.py:306-324: the masked average residual at a pose) as an op of its own, for every variant and per target frame.
 *     For every window b, target frame f (pairs, as in banet_level_t) and point n:
 *       D = depth[b,n] + basis[b,n,:] . Wc[b,:]  (K > 0), geometry and in-image mask by the float32 statements of the assembly
 *       pass (3), F2w = the bilinear sample of the first C channels of target frame f (the +1 taps clamped to the image,
 *       utils_python.py:96-99), d_c = F2w_c - F1_c with F1 the source row:
 *         sq[b,f,n] = sum_c d_c^2     ab[b,f,n] = sum_c |d_c|     mask[b,f,n] = 1 in the image / 0
 *         proj[b,f,n] = (px, py) as computed; unspecified where mask = 0           (optional)
 *         sums[b,f,0..3] = sum_n sq, sum_n ab, sum_n mask (an integer count stored as float), max_n sq   (optional; a second
 *                          launch over the three maps, one workgroup per (b, f), fixed order)
 *     Every element of sq / ab / mask is written, zeros where mask = 0 (such a point, also one with a NaN projection, reads no
 *     tap).  A window's bits -- sums included -- do not depend on the batch it is evaluated in: neither launch's arithmetic
 *     depends on B, which is also why the entry takes NO workspace.  absres of (3) is sum over f and n of ab, per channel instead
 *     of per pixel; nvalid of (3) is sum_f sums[b,f,2].
 *     Accepts exactly the levels banet_ba_assemble_f32 accepts and refuses the others with its code (all four variants, dense
 *     and sparse, pairs >= 1 for the bundle variants); a NULL lv / R / T / out / sq / ab / mask, or Wc with K > 0:
 *     BANET_ERR_INVALID_ARG, decided before any launch.  lv->flags and lv->policy are accepted and ignored (a policy value (3)
 *     refuses is refused here too).  Enqueue only: no
 *     allocation, no synchronisation, no global state, one stream.  16-byte loads where C = 128 (K = 128) and src / tgt (basis)
 *     are 16-byte aligned.  BANET_VERSION is unchanged by this addition: detect the entry by its symbol.                    */
typedef struct banet_residual_out {
  float* sq;            /* [B,pairs,N]   required */
  float* ab;            /* [B,pairs,N]   required */
  unsigned char* mask;  /* [B,pairs,N]   required */
  float* proj;          /* [B,pairs,N,2] or NULL  */
  float* sums;          /* [B,pairs,4]   or NULL  */
} banet_residual_out_t;
int banet_ba_residual_f32(const banet_level_t* lv, const float* R, const float* T, const float* Wc,
                          const banet_residual_out_t* out, banet_stream_t stream);

/* (3c) backward of (3b): the per-pixel maps as differentiable losses.  With upstream gradients gsq, gab [B,pairs,N] and
 *     gproj [B,pairs,N,2] (each may be NULL = zeros; at least one is given) the loss is
 *         L = sum_{b,f,n} gsq sq + gab ab + gproj . proj
 *     with the forward's mask and the forward's floor of the projection held fixed (the one-sided derivative at an integer
 *     coordinate, as banet_resample_grad_f32).  e_c = mask (2 gsq d_c + gab sgn d_c), sgn 0 = 0; a point with mask = 0 (also one
 *     with a NaN projection) contributes nothing to any output and reads no tap, gproj is ignored there.
 *       dsrc   [B,N,C]            = - sum_f e
 *       dtgt   [B,pairs,H,W,C]    = per texel, the sum over the points' four taps of tap weight x e row (the +1 taps clamped as in
 *                                   the forward; two clamped taps on one texel each add their own weight), in ascending
 *                                   (point, tap) order -- the resampler gradient of (6b) in clamp mode with B pairs as its batch
 *       ddepth [B,N] = dD_n       dbasis [B,N,K] = dD_n Wc_k       dWc [B,K] = sum_n dD_n basis[b,n,k]
 *       dR [B,pairs,9], dT [B,pairs,3] = dL/dR (matrix entries, as dpose of (7b)), dL/dT
 *     through (dpx, dpy) = sum_c e_c dF2w_c/d(px,py) + mask gproj and the forward's own float32 geometry statements.  No gradient
 *     for rays or intrinsics.
 *     Every output pointer may be NULL (not computed); a subset gives the same bits for that subset.  dR / dT / dWc are WRITTEN;
 *     dsrc / ddepth / dbasis are accumulated (+=) unless flags has BANET_ADJOINT_OVERWRITE, dtgt unless BANET_ADJOINT_OVERWRITE_MAP
 *     (overwriting writes every element, zeros where nothing lands: the same bits as accumulating into zeros); any other flag bit:
 *     BANET_ERR_INVALID_ARG.  dbasis / dWc with K = 0 are ignored.
 *     Accepts exactly the levels (3b) accepts, with its codes, decided before any launch; NULL lv / R / T / g / out, all three of
 *     g's pointers NULL, or Wc NULL with K > 0: BANET_ERR_INVALID_ARG.  dtgt: C-channel target maps only (tgt_has_grad = 0) and
 *     within the limits of (6b) with batch B pairs (C <= 256, B pairs H W C < 2^32), else BANET_ERR_UNSUPPORTED when out->dtgt is
 *     given and workspace_bytes(lv, 1) = 0; the other outputs of such a level still work.
 *     Workspace: required (the scratch contract at the top of this file), size by the query (want_dtgt = whether out->dtgt will be
 *     given); NULL, misaligned or too small: BANET_ERR_WORKSPACE.  Enqueue only: no allocation, no synchronisation, no global
 *     state, one stream, capturable.  No float atomics; bit-reproducible; every summation order depends on N, H, W and pairs, never
 *     on B: a window's bits are the same alone and in any batch.  BANET_VERSION is unchanged: detect the entry by its symbol.
 *     (BANET_ADJOINT_OVERWRITE / _OVERWRITE_MAP: the enum of (7b) below.)                                                      */
typedef struct banet_residual_grad_in {
  const float* gsq;   /* [B,pairs,N]   or NULL */
  const float* gab;   /* [B,pairs,N]   or NULL */
  const float* gproj; /* [B,pairs,N,2] or NULL */
} banet_residual_grad_in_t;
typedef struct banet_residual_grad_out { /* every pointer may be NULL */
  float* dsrc;
  float* dtgt;
  float* ddepth;
  float* dbasis;
  float* dWc;
  float* dR;
  float* dT;
} banet_residual_grad_out_t;
size_t banet_ba_residual_grad_workspace_bytes(const banet_level_t* lv, int want_dtgt);
int banet_ba_residual_grad_f32(const banet_level_t* lv, const float* R, const float* T, const float* Wc,
                               const banet_residual_grad_in_t* g, const banet_residual_grad_out_t* out,
                               int flags, void* ws, size_t workspace_bytes, banet_stream_t stream);

/* (3d) posterior marginals: how well the normal equations determine their answer.  From the normal matrix AtA [B,P,P] of (3)
 *     (P = 6 max(pairs, 1) + K, parameter order [pose_1 .. pose_pairs, depth]; only the lower triangle is read), per window b with
 *     mu = damping[b] (damping == NULL: 0) and s2 = sigma2[b] (sigma2 == NULL: 1):
 *         H = AtA[b] + mu diag(diag(AtA[b]) + 1e-5)         Sigma = s2 H^-1         H = L L^T
 *     The damping has the form of bundlenet.py:264-266, but -- UNLIKE the bundle solve of (4), which leaves the last coefficient
 *     undamped -- it is applied to EVERY diagonal entry, the last one included.
 *       pose_cov[b]  = the leading 6 pairs x 6 pairs block of Sigma: the joint marginal of all poses with the depth coefficients
 *                      marginalised out; written exactly symmetric
 *       wfactor[b]   = T = L_WW^-1, L_WW the trailing K x K block of L, so that Sigma_WW = s2 T^T T (the depth block comes last:
 *                      marginalising the poses costs nothing); lower triangular, the strict upper triangle written as zeros
 *       depth_var[b,n] = s2 |T basis[b,n,:]|^2: the variance of D_n = depth + basis . Wc under Sigma; non-negative by construction
 *       logdet[b]    = log det H = 2 sum_i log L_ii
 *       status[b]    = 0, or 1 where the factorisation met a pivot <= 0 or a non-finite value (H not positive definite): that
 *                      window gets depth_var = +inf everywhere, pose_cov = +inf on the diagonal and 0 elsewhere, wfactor = 0,
 *                      logdet = -inf; the other windows of the batch are unaffected.
 *     Two launches: a factorisation kernel (one workgroup per window: Cholesky and L^-1 by forward substitution, in float64 on
 *     the float32 inputs, outputs rounded once -- a float32 factorisation would lose cond(H) 2^-24 of every output; the matrix
 *     in LDS up to P = 199, in the workspace above) and, when depth_var is asked for, one pass over the basis on the f32-input
 *     matrix instructions (every product an exact float32 fma; one read of the basis, 4 bytes written per pixel).
 *     The entry reads lv->B, N, K, pairs and basis and NOTHING else of the level (N and basis only for depth_var), so a level with
 *     only those fields set is a valid argument.  BANET_ERR_INVALID_ARG, decided before any launch: NULL lv / AtA / out /
 *     out->pose_cov / out->status; B < 1 (or a negative K / pairs); with depth_var given and K > 0: basis == NULL or N < 1.
 *     K > 256 or P > 304: workspace_bytes = 0 and BANET_ERR_UNSUPPORTED.  Workspace: required (the scratch contract at the top of
 *     this file; the query is never 0 for a supported shape), size by the query (want_depth_var = whether out->depth_var will be
 *     given); NULL, misaligned or too small: BANET_ERR_WORKSPACE.  Enqueue only: no allocation, no synchronisation, no global
 *     state, one stream.  No float atomics; every summation order depends on N, K and pairs, never on B: a window's bits are the
 *     same alone and in any batch; a subset of the optional outputs gives the same bits for that subset.  BANET_VERSION is
 *     unchanged by this addition: detect the entry by its symbol.                                                              */
typedef struct banet_marginals_out {
  float* pose_cov;   /* [B][6 pairs][6 pairs]  required */
  float* depth_var;  /* [B][N]        or NULL; ignored when K == 0 */
  float* wfactor;    /* [B][K][K]     or NULL; lower-triangular T; ignored when K == 0 */
  float* logdet;     /* [B]           or NULL: log det H */
  int32_t* status;   /* [B]           required: 0 = ok, 1 = H not positive definite */
} banet_marginals_out_t;
size_t banet_ba_marginals_workspace_bytes(const banet_level_t* lv, int want_depth_var);
int banet_ba_marginals_f32(const banet_level_t* lv, const float* AtA, const float* damping, const float* sigma2,
                           const banet_marginals_out_t* out, void* ws, size_t workspace_bytes, banet_stream_t stream);

/* (3d') the backward of (3d): pose_cov, depth_var and logdet as differentiable losses.  From the upstream gradients g_pose_cov
 *     [B,m,m] (m = 6 max(pairs, 1); need not be symmetric), g_depth_var [B,N] (either sign) and g_logdet [B] -- each or NULL = zeros
 *     -- with A = AtA[b] as a symmetric matrix, H, L, T, mu, s2 as in (3d), Hinv = H^-1:
 *         M    = sum_n g_depth_var[n] b_n b_n^T               Gbar = blockdiag(1/2 (g_pose_cov + g_pose_cov^T), M)
 *         dH   = g_logdet Hinv - s2 Hinv Gbar Hinv             (symmetric)
 *       gAtA[b]     = dH off the diagonal, (1 + mu) dH on it: the gradient with respect to a SYMMETRIC AtA (through 1/2 (A + A^T)),
 *                     written in full and exactly symmetric -- the form banet_dense_adjoint_ex_f32 takes as its upstream gAtA
 *       gdamping[b] = sum_i dH_ii (A_ii + 1e-5)               gsigma2[b] = trace(Hinv Gbar)
 *       gbasis[b,n] = 2 s2 g_depth_var[n] T^T (T b_n)
 *       status[b]   = as (3d), by the same test; a window with status 1 gets zeros in every output, and its upstream values are
 *                     not used; the other windows of the batch are unaffected.
 *     wfactor has no gradient.  The entry recomputes the factorisation from AtA, damping and sigma2 (float64 on the float32 inputs,
 *     outputs rounded once): it takes no saved state from (3d).  Every requested output is written in every element: no
 *     accumulation, no need to pre-zero.  A NULL upstream gives the same bits as a zero-filled one.  Launches: M on the f32-input
 *     matrix instructions and its fold (with g_depth_var and K > 0), the factor kernel (one workgroup per window), one pass over
 *     the basis (with gbasis and K > 0: one read of the basis, one write of [N,K]).
 *     The entry reads lv->B, N, K, pairs and basis and NOTHING else of the level; N and basis only when g_depth_var or gbasis is
 *     given and K > 0 (gbasis of a level without a basis: ignored).  BANET_ERR_INVALID_ARG, decided before any launch: NULL lv /
 *     AtA / in / out / out->status; B < 1 (or a negative K / pairs); basis == NULL or N < 1 where they are read.  K > 256 or
 *     P > 304: workspace_bytes = 0 and BANET_ERR_UNSUPPORTED.  Workspace: required, pure scratch (the contract at the top of this
 *     file; the query is never 0 for a supported shape), size by the query with the lv of the call (want_gbasis = whether
 *     out->gbasis will be given); NULL, misaligned or too small: BANET_ERR_WORKSPACE.  Enqueue only, one stream.  No float atomics;
 *     every summation order depends on N, K and pairs, never on B: a window's bits are the same alone and in any batch; a subset
 *     of the outputs gives the same bits for that subset.  BANET_VERSION is unchanged: detect the entry by its symbol.          */
typedef struct banet_marginals_grad_in {
  const float* g_pose_cov;   /* [B][6 pairs][6 pairs]  or NULL = zeros */
  const float* g_depth_var;  /* [B][N]                 or NULL = zeros; ignored when K == 0 */
  const float* g_logdet;     /* [B]                    or NULL = zeros */
} banet_marginals_grad_in_t;
typedef struct banet_marginals_grad_out {
  float* gAtA;       /* [B][P][P]   or NULL */
  float* gdamping;   /* [B]         or NULL */
  float* gsigma2;    /* [B]         or NULL */
  float* gbasis;     /* [B][N][K]   or NULL; ignored when K == 0 */
  int32_t* status;   /* [B]         required: 0 = ok, 1 = H not positive definite */
} banet_marginals_grad_out_t;
size_t banet_ba_marginals_grad_workspace_bytes(const banet_level_t* lv, int want_gbasis);
int banet_ba_marginals_grad_f32(const banet_level_t* lv, const float* AtA, const float* damping, const float* sigma2,
                                const banet_marginals_grad_in_t* in, const banet_marginals_grad_out_t* out,
                                void* ws, size_t workspace_bytes, banet_stream_t stream);

/* (3e) depth transfer to a new key frame: what a window learned about the scene, carried into another frame.  Two entries.
 *   banet_depth_reproject_f32: the key frame's depth map D = depth + basis . Wc (Wc == NULL or K == 0: D = depth) reprojected
 *     into the pixel grid of every target frame f (F = max(pairs, 1); R [B,F,9], T [B,F,3]) with a z-buffer.  Per source pixel n
 *     and frame f, by the float32 statements of the assembly pass (3): the ray p_n from the pixel index, the level scale and intr
 *     (normalised iff normalize_rays), X = R_f (p_n D) + T_f, (px, py) with the level intrinsics intr / scale, and the point's
 *     depth in the target frame in the level's own convention, d' = |X| if normalize_rays (range along the ray, bundlenet.py:119)
 *     else X_z (legacy/ba.py:33-34).  The point is valid iff 0 <= px <= W-1 and 0 <= py <= H-1 (the in-image mask of (3); a NaN
 *     fails it), X_z > 0 and d' is finite and > 0; it lands on texel (floor(px + 0.5), floor(py + 0.5)).  Per texel the winner is
 *     the landed point with the smallest (bits of d' as uint32, n), lexicographically:
 *       depth[b,f,y,x] = the winner's d', bit for bit; 0 where nothing lands
 *       index[b,f,y,x] = the winner's n;               -1 where nothing lands
 *     Every element of both outputs is written.  No splatting over neighbours: holes under magnification are reported as -1.
 *     Three launches (key init, splat with an unsigned 64-bit integer atomic min on (d' bits << 32) | n, decode); integer atomics
 *     only, so the result does not depend on the order in which points arrive: bit-reproducible, and a window's bits are the same
 *     alone and in any batch.  16-byte loads of the basis rows where K % 4 == 0 and basis is 16-byte aligned, 4-byte loads
 *     otherwise: the same bits.  Dense levels (dense = 1) of any variant; the entry reads B, N, K, H, W, dense, normalize_rays,
 *     scale, pairs, depth, basis, intr and NOTHING else of the level (src, tgt and C are not read).  BANET_ERR_INVALID_ARG, decided
 *     before any launch: NULL lv / R / T / out / out->depth / out->index / lv->depth / lv->intr (lv->basis with K > 0 and Wc
 *     given), B, N, H or W < 1, a negative K / pairs, N != H W, scale <= 0; dense = 0: BANET_ERR_UNSUPPORTED and a query of 0.
 *     Workspace: required, B F H W 8 bytes (the keys) rounded up to 256; NULL, misaligned or too small: BANET_ERR_WORKSPACE.
 *   banet_basis_fit_f32: a weighted, damped least-squares fit of a depth map on a level's basis -- the new key frame's
 *     coefficients from the reprojected map, or a depth observation (RGB-D, a prior) as normal equations.  Per window b, with
 *     target, weight [B,N] (weight == NULL: 1), mu = damping[b] (damping == NULL: 0) and r_n = target_n - depth_n, over the points
 *     with a finite w_n > 0 and a finite target_n (texels of the reprojection with index = -1 go in with w = 0):
 *         G = sum_n w_n b_n b_n^T     g = sum_n w_n r_n b_n     H = G + mu diag(diag(G) + 1e-5)     Wc = H^-1 g
 *     (the damping on every diagonal entry, as (3d)).  G and g are exactly what such a depth term adds to the depth block of AtA /
 *     Atb in front of (4).
 *       Wc[b]      = the solution; 0 where status = 1
 *       normal[b]  = G, full and exactly symmetric            rhs[b] = g
 *       stats[b]   = (sum_n w_n, sum_n w_n r_n^2) over the contributing points
 *       status[b]  = 0, or 1 where the factorisation met a pivot <= 0 or a non-finite value (H not positive definite): that window
 *                    gets Wc = 0; the other windows of the batch are unaffected.
 *     Three launches: the Gram pass (one read of the basis on the f32-input matrix instructions, every product an exact float32
 *     fma; partial rows per contiguous pixel range in the workspace), a fold that adds the rows in a fixed order, and one
 *     workgroup per window for the Cholesky factorisation and the two substitutions in float64 on the float32 H, Wc rounded once
 *     (the matrix in LDS up to K = 199, in the workspace above).  The entry reads lv->B, N, K, depth and basis and NOTHING else of
 *     the level: a level with only those fields set is a valid argument, sparse N included.  BANET_ERR_INVALID_ARG, decided before
 *     any launch: NULL lv / target / out / out->Wc / out->status / lv->depth / lv->basis, B < 1.  K outside 1 .. 256 or N < 1:
 *     workspace_bytes = 0 and BANET_ERR_UNSUPPORTED.  Workspace: required, size by the query; NULL, misaligned or too small:
 *     BANET_ERR_WORKSPACE.
 *   Both: enqueue only -- no allocation, no synchronisation, no global state, one stream.  No float atomics; the number of
 *   partial rows and every summation order depend on N and K only, never on B: a window's bits are the same alone and in any
 *   batch; a subset of the optional outputs gives the same bits for that subset.  BANET_VERSION is unchanged by this addition:
 *   detect the entries by their symbols.                                                                                        */
typedef struct banet_reproject_out {
  float* depth;    /* [B,F,H,W]  required: depth of the winning point in the TARGET frame, 0 where nothing lands */
  int32_t* index;  /* [B,F,H,W]  required: the winning source pixel n, -1 where nothing lands */
} banet_reproject_out_t;
size_t banet_depth_reproject_workspace_bytes(const banet_level_t* lv);
int banet_depth_reproject_f32(const banet_level_t* lv, const float* R, const float* T, const float* Wc,
                              const banet_reproject_out_t* out, void* ws, size_t workspace_bytes, banet_stream_t stream);
typedef struct banet_basis_fit_out {
  float* Wc;        /* [B,K]    required */
  float* normal;    /* [B,K,K]  or NULL: G, full and exactly symmetric */
  float* rhs;       /* [B,K]    or NULL: g */
  float* stats;     /* [B,2]    or NULL: sum_n w_n, sum_n w_n r_n^2 */
  int32_t* status;  /* [B]      required: 0 ok, 1 H not positive definite (that window: Wc = 0; others unaffected) */
} banet_basis_fit_out_t;
size_t banet_basis_fit_workspace_bytes(const banet_level_t* lv);
int banet_basis_fit_f32(const banet_level_t* lv, const float* target, const float* weight, const float* damping,
                        const banet_basis_fit_out_t* out, void* ws, size_t workspace_bytes, banet_stream_t stream);

/* (4) lambda prediction + damping + solve + SE(3)/W update for all B windows
 *     (bundlenet.py:165-190,241-276; legacy/ba.py:187-213,266-302).  Consumes the outputs
 *     of (3); updates `st` in place.  l2_base: bundlenet.py:252-253 (pass 1.0 for none). */
int banet_ba_solve_update_f32(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base,
                              const float* AtA, const float* Atb, const float* absres,
                              const float* nvalid, banet_state_t* st, banet_stream_t stream);
/*     The same with a caller workspace for the systems whose matrix does not fit the LDS
 *     (P > ~190, e.g. K = 256): workspace_bytes = 0 means (4) alone is enough (ws may be NULL). */
size_t banet_ba_solve_update_workspace_bytes(const banet_level_t* lv);
int banet_ba_solve_update_ws_f32(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base,
                                 const float* AtA, const float* Atb, const float* absres,
                                 const float* nvalid, banet_state_t* st, void* ws, size_t ws_bytes,
                                 banet_stream_t stream);

/* (5) the LM loop at one level, entirely enqueued (no host sync): max_iters iterations of
 *     (3)+(4).  For BANET_LEGACY_LM with early_termination != 0 the accept/reject test and
 *     the update-norm thresholds of legacy/ba.py:132-140,343-345 are evaluated on the
 *     device per window (the CheckUpdate pass of iteration k is the assembly pass of
 *     iteration k+1); st->iters receives the reference's iteration count.               */
size_t banet_lm_level_workspace_bytes(const banet_level_t* lv);
int banet_lm_level_f32(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base,
                       int max_iters, int early_termination, banet_state_t* st, void* ws,
                       size_t ws_bytes, banet_stream_t stream);

/* (5b) the same loop with the reference's run-time LM configuration.  legacy/ba.py:5-9 keeps
 *     early_termination / angle_change / translation_change / residual_ratio / qr as module
 *     globals that its drivers overwrite (legacy/example.py:8, legacy/eval.py:9); here they are
 *     arguments.  banet_lm_level_f32 == banet_lm_level_ex_f32 with params = NULL (the
 *     reference's defaults, banet_lm_params_default).
 *       angle_change, translation_change : loop continues while both update norms exceed them
 *                                          (legacy/ba.py:133); only read with early_termination
 *       residual_ratio                   : accept iff avg' < residual_ratio * avg (ba.py:343)
 *       solver (legacy variants only)    : BANET_SOLVER_QR  = tf.qr + triangular solve
 *                                          (ba.py:205-206,292-293, `qr = True`);
 *                                          BANET_SOLVER_INVERSE = tf.matrix_inverse (LU with
 *                                          partial pivoting) then a product (ba.py:203,290,
 *                                          `qr = False`).  The bundlenet variants always use
 *                                          tf.matrix_solve's algorithm class (bundlenet.py:183,
 *                                          267) and ignore this field.                        */
enum { BANET_SOLVER_QR = 0, BANET_SOLVER_INVERSE = 1 };
typedef struct banet_lm_params {
  float angle_change;       /* legacy/ba.py:6  default 0.002 * (3.14 / 180)                   */
  float translation_change; /* legacy/ba.py:7  default 0.0002                                 */
  float residual_ratio;     /* legacy/ba.py:8  default 1.0                                    */
  int32_t solver;           /* legacy/ba.py:9  default BANET_SOLVER_QR                        */
} banet_lm_params_t;
void banet_lm_params_default(banet_lm_params_t* params);
int banet_lm_level_ex_f32(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base,
                          int max_iters, int early_termination, const banet_lm_params_t* params,
                          banet_state_t* st, void* ws, size_t ws_bytes, banet_stream_t stream);

/* (5c) the whole coarse -> fine schedule in one call.  The reference's layer runs every level inside one graph and returns the
 *     per-level rotations, translations and depths of all of them (bundlenet.py:376-399: the loop over the pyramid and its
 *     output_rotations / output_translations / output_depths lists; legacy/ba.py:106-145: trackTF's three levels and their
 *     iteration counts).  banet_lm_solve_f32 is exactly the sequence
 *         banet_lm_level_ex_f32(&levels[l], mlps[l], l2_base, max_iters[l], early_termination, params, st,
 *                               workspace, workspace_bytes, stream)        for l = 0 .. n_levels - 1
 *     on one stream, with the state after each level copied into row l of the trace -- bit-identical to that sequence plus
 *     copies after every level.  The levels are PREPARED levels, dense or sparse (the per-level resampling of (6) is the
 *     caller's); they share B, K, pairs, variant and policy (the state's layout) and may differ in H, W, N, C, scale, flags.
 *       - all or nothing: every level, the state, params, each level's launch plan and workspace need are checked on the host
 *         before the first launch; a bad level -- also the last one -- returns the code banet_lm_level_ex_f32 would return for
 *         it and nothing has been enqueued.  Levels that disagree in B / K / pairs / variant / policy, n_levels outside 1 .. 16,
 *         trace->depth with a variant other than BANET_BUNDLE: BANET_ERR_INVALID_ARG;
 *       - workspace: the MAXIMUM of the levels' banet_lm_level_workspace_bytes (banet_lm_solve_workspace_bytes; 0 = a level is
 *         invalid or unsupported, or the levels disagree).  Each level runs on the previous level's leftovers (the scratch
 *         contract at the top of this file); the trace needs none;
 *       - trace: every pointer optional (NULL = not recorded); one small kernel per level (no memcpy nodes), the per-level depth
 *         through the kernel of banet_depth_output_f32;
 *       - no allocation, no synchronisation, no global state, one stream: capturable into a HIP graph as a linear chain.
 *     BANET_VERSION is unchanged by this addition: detect the entry by its symbol (dlsym / hasattr).                          */
typedef struct banet_solve_trace { /* state AFTER each level; every pointer may be NULL */
  float* R;            /* [n_levels][B][pairs][9]                                                */
  float* T;            /* [n_levels][B][pairs][3]                                                */
  float* Wc;           /* [n_levels][B][K]   (ignored when K == 0)                               */
  float* lambda_out;   /* [n_levels][B]                                                          */
  float* delta;        /* [n_levels][B][P]                                                       */
  float* ratio;        /* [n_levels][B]                                                          */
  int32_t* iters;      /* [n_levels][B]      the reference's iteration count at that level       */
  float* const* depth; /* n_levels HOST-array entries, entry l NULL or a device buffer [B][N_l]:
                          levels[l].depth + levels[l].basis . Wc after level l (bundlenet.py:397
                          output_depths); BANET_BUNDLE only                                      */
} banet_solve_trace_t;

typedef struct banet_schedule {
  const banet_level_t* levels;       /* n_levels prepared levels, coarse -> fine                 */
  int32_t n_levels;                  /* 1 .. 16                                                  */
  int32_t early_termination;         /* as banet_lm_level_f32's                                  */
  const banet_mlp_t* const* mlps;    /* n_levels pointers (entries NULL where the variant has no
                                        MLP: BANET_LEGACY_FIXED; the array itself may then be NULL) */
  const int32_t* max_iters;          /* n_levels counts, each >= 0                               */
  float l2_base;                     /* bundlenet.py:252-253 (1.0 for none)                      */
  const banet_lm_params_t* params;   /* NULL = the reference's defaults                          */
  void* workspace;                   /* >= banet_lm_solve_workspace_bytes, 256-byte aligned      */
  size_t workspace_bytes;
  const banet_solve_trace_t* trace;  /* NULL = nothing recorded                                  */
} banet_schedule_t;

size_t banet_lm_solve_workspace_bytes(const banet_schedule_t* s); /* reads levels / n_levels only */
int banet_lm_solve_f32(const banet_schedule_t* s, banet_state_t* st, banet_stream_t stream);

/* (5d) depth observations and coefficient priors inside the LM loop.  BANET_BUNDLE levels with K >= 1, dense or sparse, any pairs.
 *     Per window the solve additionally minimises
 *         scale (1/2 Wc^T Lambda Wc - eta^T Wc + 1/2 sum_n w_n (obs_n - depth_n - b_n . Wc)^2)
 *     -- a Gaussian prior on the coefficients in information form (what banet_basis_fit_f32 returns as normal / rhs for the
 *     previous window's transferred depth) and / or a depth observation per point (RGB-D, sparse LiDAR; w = obs_weight, NULL: 1),
 *     the sum over the points banet_basis_fit_f32 counts: a finite w_n > 0 and a finite obs_n.  With G, g that fit's normal and rhs
 *     for target = obs:
 *         Le = fl(scale fl(G + Lambda))      ee = fl(scale fl(g + eta))      (a half that is not given is left out, not added as 0)
 *         AtA[m+i, m+j] += Le[i,j]           Atb[m+i] += ee[i] - sum_j Le[i,j] Wc[j]          m = 6 max(pairs, 1), row stride P
 *     between (3) and (4) of every iteration: before the damping, which therefore sees the prior on the diagonal.  lambda is still
 *     predicted from the feature residuals alone (absres / nvalid).  D = depth + b . Wc is linear in Wc, so G and g are constant
 *     over a level's iterations: Le and ee are formed once per level (the Gram pass and fold of banet_basis_fit_f32 -- G, g bit-equal
 *     to its normal / rhs -- and one combine launch), and every iteration costs one more launch, ba_prior_add_kernel, one wave per
 *     row of Le, no atomics, every output element written by exactly one lane.  Every summation order depends on N and K only: a
 *     window's bits are the same alone and in any batch.
 *     The EMPTY prior: pr == NULL, all four pointers NULL, or scale == 0.  banet_prior_apply_f32 then launches nothing;
 *     banet_lm_level_prior_f32 is then exactly banet_lm_level_ex_f32 with early_termination = 0 (same launches, same bits, same
 *     workspace need) and banet_lm_solve_prior_f32 exactly banet_lm_solve_f32.
 *     BANET_ERR_INVALID_ARG, decided before any launch: eta without Lambda, obs_weight without obs_depth, a scale that is negative
 *     or not finite, reserved_ != 0 (whatever the scale); NULL Wc / AtA / Atb (banet_prior_apply_f32); everything
 *     banet_lm_level_ex_f32 / banet_lm_solve_f32 refuse, with their codes; s->early_termination != 0.  A prior that is not empty on
 *     a variant other than BANET_BUNDLE or with K == 0 (K > 256, N < 1): BANET_ERR_UNSUPPORTED, and a query of 0.
 *     Workspace: the queries read which pointers of pr are NULL and the level's shape, nothing else (not the scale);
 *     banet_lm_level_prior_workspace_bytes = banet_lm_level_workspace_bytes plus the prior's regions behind it,
 *     banet_lm_solve_prior_workspace_bytes the maximum over the levels (priors == NULL: no level has one).  NULL, misaligned or too
 *     small: BANET_ERR_WORKSPACE.  banet_prior_apply_f32 is one iteration's step on the caller's AtA / Atb, in place (the once-per-
 *     level launches included); it reads lv->B, N, K, pairs, variant, depth and basis and nothing else of the level.
 *     banet_lm_solve_prior_f32: priors[l] belongs to levels[l]; all or nothing like banet_lm_solve_f32 -- a bad prior on the last
 *     level enqueues nothing; bit-identical to the sequence of banet_lm_level_prior_f32 calls plus the trace copies.
 *     Enqueue only: no allocation, no synchronisation, no global state, one stream, capturable.  BANET_VERSION is unchanged by this
 *     addition: detect the entries by their symbols.                                                                           */
typedef struct banet_prior {
  const float* Lambda;      /* [B,K,K] symmetric, or NULL */
  const float* eta;         /* [B,K], or NULL = 0; only with Lambda */
  const float* obs_depth;   /* [B,N], or NULL */
  const float* obs_weight;  /* [B,N], or NULL = 1; only with obs_depth */
  float scale;              /* finite, >= 0 */
  int32_t reserved_;        /* 0 */
} banet_prior_t;

size_t banet_prior_workspace_bytes(const banet_level_t* lv, const banet_prior_t* pr);
int banet_prior_apply_f32(const banet_level_t* lv, const banet_prior_t* pr, const float* Wc, float* AtA, float* Atb, void* ws,
                          size_t workspace_bytes, banet_stream_t stream);

size_t banet_lm_level_prior_workspace_bytes(const banet_level_t* lv, const banet_prior_t* pr);
int banet_lm_level_prior_f32(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, int max_iters,
                             const banet_lm_params_t* params, const banet_prior_t* pr, banet_state_t* st, void* ws,
                             size_t workspace_bytes, banet_stream_t stream);

size_t banet_lm_solve_prior_workspace_bytes(const banet_schedule_t* s, const banet_prior_t* priors);
int banet_lm_solve_prior_f32(const banet_schedule_t* s, const banet_prior_t* priors /* n_levels entries, or NULL */,
                             banet_state_t* st, banet_stream_t stream);

/* (5e) the backward of (5d): training through a solve that carries a prior.  With gAtA', gAtb' the gradients with respect to the
 *     matrices one iteration's solve was given (the post-prior ones), Wc that iteration's coefficients, m = 6 max(pairs, 1):
 *         gAtA = gAtA', gAtb = gAtb'                               (pass through to the dense adjoint, unchanged)
 *         gLe[i,j] += gAtA'[m+i, m+j] - gAtb'[m+i] Wc[j]           (raw, not symmetrised)
 *         gee[i]   += gAtb'[m+i]          gWc[j] -= sum_i Le[i,j] gAtb'[m+i]
 *     and once per level, after the iterations have accumulated gLe and gee:
 *         gLambda = scale gLe     geta = scale gee     gscale = (sum gLe.Le + sum gee.ee) / scale
 *         Gh = scale 1/2 (gLe + gLe^T)    gh = scale gee        (G is a mirrored sum: it takes the symmetrised gradient)
 *         per counted point n, r = obs - depth, y = Gh b_n, p = b_n . gh, q = b_n . y:
 *         gweight_n = q + r p     gobs_n = w p     gdepth_n -= w p     gbasis_n += w (2 y + r gh)
 *     A point is counted as in (5d); the others get zeros, or are left untouched in accumulate mode.
 *   banet_prior_terms_f32       the once-per-level launches of (5d) alone: Le [B,K,K] and ee [B,K] into the caller's memory, bit-equal
 *       to what banet_prior_apply_f32 forms in its workspace (so banet_prior_apply_f32 with {Lambda = Le, eta = ee, scale = 1} adds
 *       the bits of the original prior: fl(1 x) = x).  Workspace: banet_prior_workspace_bytes.  Errors as banet_prior_apply_f32
 *       (NULL Le / ee: BANET_ERR_INVALID_ARG).  The empty prior writes nothing and returns BANET_OK.
 *   banet_prior_add_grad_f32    one iteration's step, one launch, no workspace.  BANET_PRIOR_GRAD_OVERWRITE: gLe and gee are written
 *       (the first call of a level), otherwise accumulated into; gWc always accumulates.  It reads lv->B, K, pairs and variant only.
 *       The column sums of gWc are fixed-order fma chains joined by the wave butterfly; 16-byte accesses where K % 4 == 0 and gLe
 *       and Wc are 16-byte aligned, 4-byte accesses of the same elements otherwise: equal bits.  NULL pointer, unknown flag bit:
 *       BANET_ERR_INVALID_ARG; a level the term does not exist on: BANET_ERR_UNSUPPORTED.
 *   banet_prior_terms_grad_f32  the once-per-level step.  Every output pointer is optional and a subset gives the same bits.
 *       BANET_PRIOR_GRAD_ACCUMULATE: gdepth and gbasis are read-modify-write (the term adds into the dense adjoint's ddepth /
 *       dbasis); without it they are written, zeros at the points that are not counted.  gLambda, geta, gscale, gobs and gweight
 *       are always written.  An output whose input the prior does not have (gLambda / geta / gobs / gweight without Lambda / eta /
 *       obs_depth / obs_weight; gdepth / gbasis without obs_depth), NULL gLe / gee, gscale without Le / ee, no output at all, an
 *       unknown flag bit, an empty prior: BANET_ERR_INVALID_ARG before any launch.  gscale: one workgroup per window, float64 on
 *       the float32 inputs, fixed order.  One preparation launch (Gh, gh into the workspace; gLambda, geta, gscale), then -- only
 *       with observations and one of the four per-pixel outputs -- the per-pixel kernel: y = Gh b for 32-pixel tiles on
 *       v_mfma_f32_32x32x2_f32, Gh's lower 32 x 32 blocks resident in LDS, one read of the basis row, one read-modify-write of
 *       the gbasis row.  Workspace: Gh [B,K,K] and gh [B,K], each at a 256-byte boundary.
 *     Enqueue only: no allocation, no synchronisation, no global state, one stream, capturable.  No float atomics; every output
 *     element is written by exactly one lane; every summation order is a function of N, K and pairs alone: a window's bits are the
 *     same alone and in any batch.  BANET_VERSION is unchanged by this addition: detect the entries by their symbols.          */
#define BANET_PRIOR_GRAD_OVERWRITE 1   /* banet_prior_add_grad_f32: write gLe / gee instead of accumulating */
#define BANET_PRIOR_GRAD_ACCUMULATE 2  /* banet_prior_terms_grad_f32: gdepth / gbasis += instead of = */

typedef struct banet_prior_grad_in {
  const float* gLe;  /* [B,K,K] accumulated by banet_prior_add_grad_f32 */
  const float* gee;  /* [B,K] */
  const float* Le;   /* [B,K,K] of banet_prior_terms_f32; only gscale reads it (else may be NULL) */
  const float* ee;   /* [B,K] */
  int32_t flags;     /* BANET_PRIOR_GRAD_ACCUMULATE or 0 */
  int32_t reserved_; /* 0 */
} banet_prior_grad_in_t;

typedef struct banet_prior_grad_out { /* each or NULL */
  float* gLambda; /* [B,K,K] */
  float* geta;    /* [B,K] */
  float* gscale;  /* [B] */
  float* gobs;    /* [B,N] */
  float* gweight; /* [B,N] */
  float* gdepth;  /* [B,N] */
  float* gbasis;  /* [B,N,K] */
} banet_prior_grad_out_t;

int banet_prior_terms_f32(const banet_level_t* lv, const banet_prior_t* pr, float* Le, float* ee, void* ws, size_t workspace_bytes,
                          banet_stream_t stream);
int banet_prior_add_grad_f32(const banet_level_t* lv, const float* Le, const float* Wc, const float* gAtA, const float* gAtb, float* gLe,
                             float* gee, float* gWc, int flags, banet_stream_t stream);
size_t banet_prior_terms_grad_workspace_bytes(const banet_level_t* lv, const banet_prior_t* pr);
int banet_prior_terms_grad_f32(const banet_level_t* lv, const banet_prior_t* pr, const banet_prior_grad_in_t* in,
                               const banet_prior_grad_out_t* out, void* ws, size_t workspace_bytes, banet_stream_t stream);

/* (5f) a pose prior inside the LM loop: a motion-model, odometry or IMU pose, or the previous window's posterior on the frames it
 *     shares with this one (banet_ba_marginals_f32's pose_cov, inverted).  BANET_BUNDLE levels (K >= 1) and the pose-only
 *     BANET_BUNDLE_CAMERA (K == 0), dense or sparse, up to 8 target frames.  The update convention is the solve's: delta = [w; t],
 *     R' = exp(w) R, T' = V(w) t + exp(w) T, i.e. T' = Exp(delta) o T with Exp([phi; rho]) = (exp(phi), V(phi) rho) -- a left
 *     perturbation, the tangent pose_cov is expressed in.  Per window, with prior poses (R0_i, T0_i), i < pairs, and a joint
 *     information matrix Lambda [m,m], m = 6 max(pairs, 1) (symmetric; positive semi-definite expected, not checked), the solve
 *     additionally minimises scale 1/2 r^T Lambda r:
 *         E_i = T_i o T0_i^-1:  Re = R_i R0_i^T,  te = T_i - Re T0_i        r_i = Log(E_i) = [phi; rho],  rho = V(phi)^-1 te
 *         Jr  = blockdiag_i J_l(r_i)^-1,   J_l^-1 = [[J^-1, 0], [-J^-1 Q J^-1, J^-1]],   J = V(phi),   Q = Q(rho, phi) of the
 *               SE(3) left Jacobian in closed form (Barfoot, State Estimation for Robotics), rotation first
 *         AtA[0:m, 0:m] += scale Jr^T Lambda Jr         Atb[0:m] -= scale Jr^T Lambda r           (Gauss-Newton; row stride P)
 *     between (3) and (4) of every iteration at that iteration's R, T: before the damping, which therefore sees the prior on the
 *     diagonal.  lambda is still predicted from the feature residuals alone.  The angle is atan2(|vee(Re - Re^T)| / 2,
 *     (tr Re - 1) / 2); series below |phi| = 1e-3 (theta / sin theta) and 0.5 (the coefficients of J^-1 and Q).  Supported range:
 *     |phi| <= 3.0; beyond it the outputs are finite and nothing more.  At Re = I and te = 0 exactly (R = R0 = I, T = T0):
 *     Jr = I and r = 0 exactly, the block gets fl(scale Lambda) and Atb keeps its bits.
 *     One launch per iteration, ba_pose_prior_add_kernel: one workgroup of four waves per window whatever the shape, r_i and
 *     Jr_i in LDS, no workspace, no once-per-level pass, no atomics, every output element written by exactly one lane, 4-byte
 *     accesses to AtA.  Every summation order depends on pairs only: a window's bits are the same alone and in any batch.
 *     The EMPTY pose prior: pp == NULL, all three pointers NULL, or scale == 0.  banet_pose_prior_apply_f32 then launches
 *     nothing; banet_lm_level_pose_prior_f32 is then exactly banet_lm_level_prior_f32 and banet_lm_solve_pose_prior_f32 exactly
 *     banet_lm_solve_prior_f32 (same launches, same bits, same workspace need).
 *     BANET_ERR_INVALID_ARG, decided before any launch: some but not all of R0 / T0 / Lambda; a scale that is negative or not
 *     finite; reserved_ != 0 (whatever the scale); NULL R / T / AtA / Atb (banet_pose_prior_apply_f32); everything
 *     banet_lm_level_prior_f32 / banet_lm_solve_prior_f32 refuse, with their codes (pr keeps the rules of (5d): a coefficient
 *     prior on a camera level is still BANET_ERR_UNSUPPORTED); s->early_termination != 0.  A pose prior that is not empty on a
 *     legacy variant or a window of more than 8 target frames: BANET_ERR_UNSUPPORTED, and a query of 0.
 *     Workspace: none of its own -- banet_lm_level_pose_prior_workspace_bytes(lv, pr, pp) == banet_lm_level_prior_workspace_bytes(lv,
 *     pr) wherever the entry accepts pp's pointers (the scale is not read), and the solve query is the maximum over the levels.
 *     banet_pose_prior_apply_f32 is one iteration's step on the caller's AtA [B,P,P] / Atb [B,P] at R [B,pairs,3,3], T [B,pairs,3],
 *     in place; it reads lv->B, K, pairs and variant and nothing else of the level.
 *     banet_lm_solve_pose_prior_f32: priors[l] and pose_priors[l] belong to levels[l] (either array may be NULL: no level has
 *     one); all or nothing -- a bad prior on the last level enqueues nothing; bit-identical to the sequence of
 *     banet_lm_level_pose_prior_f32 calls plus the trace copies.
 *     Enqueue only: no allocation, no synchronisation, no global state, one stream, capturable.  BANET_VERSION is unchanged by this
 *     addition: detect the entries by their symbols.                                                                           */
typedef struct banet_pose_prior {
  const float* R0;      /* [B,pairs,3,3] */
  const float* T0;      /* [B,pairs,3] */
  const float* Lambda;  /* [B,m,m] symmetric, m = 6 max(pairs, 1) */
  float scale;          /* finite, >= 0 */
  int32_t reserved_;    /* 0 */
} banet_pose_prior_t;

int banet_pose_prior_apply_f32(const banet_level_t* lv, const banet_pose_prior_t* pp, const float* R, const float* T, float* AtA,
                               float* Atb, banet_stream_t stream);

size_t banet_lm_level_pose_prior_workspace_bytes(const banet_level_t* lv, const banet_prior_t* pr, const banet_pose_prior_t* pp);
int banet_lm_level_pose_prior_f32(const banet_level_t* lv, const banet_mlp_t* mlp, float l2_base, int max_iters,
                                  const banet_lm_params_t* params, const banet_prior_t* pr, const banet_pose_prior_t* pp,
                                  banet_state_t* st, void* ws, size_t workspace_bytes, banet_stream_t stream);

size_t banet_lm_solve_pose_prior_workspace_bytes(const banet_schedule_t* s, const banet_prior_t* priors,
                                                 const banet_pose_prior_t* pose_priors);
int banet_lm_solve_pose_prior_f32(const banet_schedule_t* s, const banet_prior_t* priors /* n_levels entries, or NULL */,
                                  const banet_pose_prior_t* pose_priors /* n_levels entries, or NULL */, banet_state_t* st,
                                  banet_stream_t stream);

/* (5g) the backward of (5f): training through a solve that carries a pose prior.  With G = gAtA'[0:m, 0:m] (raw, not symmetrised; row
 *     stride P) and g = gAtb'[0:m] the gradients with respect to the post-prior matrices of one iteration, r, Jr, Lambda and
 *     s = scale the quantities of (5f) at that iteration's R, T:
 *         gAtA = gAtA', gAtb = gAtb'                               (pass through to the dense adjoint, unchanged; not written)
 *         y = Jr g     X = Lambda Jr     Xt = Lambda^T Jr     u = Lambda r
 *         gLambda += s (Jr G Jr^T - y r^T)                         (Lambda differentiated as the full matrix the forward reads)
 *         gscale  += <G, Jr^T Lambda Jr> - <g, Jr^T Lambda r>      (float64 on the float32 values, fixed order)
 *         gr = -s Lambda^T y      gJr_i = s (X G^T + Xt G)[block i] - s u_i g_i^T       (the 6 x 6 diagonal blocks only)
 *         (gR_i, gT_i, gR0_i, gT0_i) += (d(r_i, Jr_i) / d(R_i, T_i, R0_i, T0_i))^T (gr_i, gJr_i)
 *     the last line being the derivative of the chain of (5f) as the forward evaluates it, R and R0 as nine free entries each (the
 *     convention of the dense adjoint's dpose[:, 0:9]).  Every 0 / 0 of the chain is taken analytically: at R = R0, T = T0
 *     exactly the gradients are finite and equal the limit.  The derivative's coefficients of J^-1 and Q are series in theta^2
 *     over the whole supported range (|phi| <= 3.0), with their own orders; the branch of theta / sin theta is the forward's.
 *   banet_pose_prior_add_grad_f32   one iteration's step: one launch, ba_pose_prior_grad_kernel, one workgroup of four waves per
 *       window whatever the shape, no workspace, no atomics; r_i and Jr_i are recomputed with the forward's own function (its
 *       bits); the pose outputs in forward mode, one lane per (pose, input entry) and output element.  Every output pointer of
 *       banet_pose_prior_grad_t is optional (NULL: not wanted, and not computed where that saves work); a subset gives the bits of
 *       the full call.  All outputs accumulate (read-modify-write) unless BANET_POSE_PRIOR_GRAD_OVERWRITE_STATE (gR / gT are
 *       written) / BANET_POSE_PRIOR_GRAD_OVERWRITE_PRIOR (gR0 / gT0 / gLambda / gscale are written).  It reads lv->B, K, pairs
 *       and variant only.  BANET_ERR_INVALID_ARG before any launch: a struct (5f) refuses, the empty pose prior (it has no
 *       backward), an unknown flag bit, reserved_ != 0, NULL lv / pp / R / T / gAtA / gAtb / out, no output at all;
 *       BANET_ERR_UNSUPPORTED: a level (5f) refuses.
 *     Enqueue only: no allocation, no synchronisation, no global state, one stream, capturable.  Every output element is written
 *     by exactly one lane; every summation order is a function of pairs alone: a window's bits are the same alone and in any
 *     batch.  BANET_VERSION is unchanged by this addition: detect the entry by its symbol.                                      */
#define BANET_POSE_PRIOR_GRAD_OVERWRITE_STATE 1 /* write gR / gT instead of accumulating */
#define BANET_POSE_PRIOR_GRAD_OVERWRITE_PRIOR 2 /* write gR0 / gT0 / gLambda / gscale instead of accumulating */

typedef struct banet_pose_prior_grad { /* each pointer or NULL */
  float* gR;         /* [B,pairs,3,3] */
  float* gT;         /* [B,pairs,3] */
  float* gR0;        /* [B,pairs,3,3] */
  float* gT0;        /* [B,pairs,3] */
  float* gLambda;    /* [B,m,m] */
  float* gscale;     /* [B] */
  int32_t flags;     /* BANET_POSE_PRIOR_GRAD_OVERWRITE_* or 0 */
  int32_t reserved_; /* 0 */
} banet_pose_prior_grad_t;

int banet_pose_prior_add_grad_f32(const banet_level_t* lv, const banet_pose_prior_t* pp, const float* R, const float* T,
                                  const float* gAtA, const float* gAtb, const banet_pose_prior_grad_t* out, banet_stream_t stream);

/* (6) per-level preparation -- the step immediately before the LM loop.
 *   banet_resample_f32   data [B,H,W,C], warp [B,N,2] (x,y) -> out [B,N,C]
 *       mode BANET_RESAMPLE_ZERO_PAD : tf.contrib.resampler.resampler as called at
 *            bundlenet.py:290,320,343-344,385 (bilinear, taps outside the image contribute 0,
 *            points with x <= -1, y <= -1, x >= W or y >= H give 0)
 *       mode BANET_RESAMPLE_CLAMP    : interpolate2d2, legacy/utils_python.py:177-232
 *            (legacy/ba.py:115): weights from the unclamped floor, indices clamped
 *   banet_target_map_f32 img [B,H,W,C] -> [B,H,W,3C] = [f | gx | gy], grad_fixed with REFLECT
 *            padding (bundlenet.py:92-100,323-324; legacy/ba.py:17-25,116-118)
 *   banet_depth_output_f32 out [B,N] = init_depth [B,N] + basis [B,N,K] . Wc [B,K]
 *            (bundlenet.py:397)                                                            */
enum { BANET_RESAMPLE_ZERO_PAD = 0, BANET_RESAMPLE_CLAMP = 1 };
int banet_resample_f32(const float* data, const float* warp, float* out, int B, int N, int C,
                       int H, int W, int mode, banet_stream_t stream);
int banet_target_map_f32(const float* img, float* out, int B, int H, int W, int C,
                         banet_stream_t stream);
int banet_depth_output_f32(const float* init_depth, const float* basis, const float* Wc,
                           float* out, int B, int N, int K, banet_stream_t stream);

/* (6b) gradients of the per-level preparation (what tf.gradients derives for bundlenet.py:320,343-344,385,397).
 *   banet_resample_grad_f32   adjoint of banet_resample_f32 (same mode): given gout [B,N,C] = dL/dout,
 *       ddata [B,H,W,C] = sum over the points' taps of tap weight x gout row (mode 0: taps outside the image and points
 *            that are not sampled contribute nothing; mode 1: clamped taps on one texel each add their own weight);
 *            summed per texel in ascending (point, tap) order with no float atomics: bit-reproducible;
 *       dwarp [B,N,2] = sum_c gout . d out / d (x, y) with the forward's floor held fixed (the one-sided derivative at an
 *            integer coordinate); 0 for a point mode 0 does not sample.  dwarp is always written.
 *   banet_depth_output_grad_f32  adjoint of banet_depth_output_f32: dinit [B,N] = gout, dbasis [B,N,K] = gout Wc^T,
 *       dWc [B,K] = sum_n gout basis (per-block partials in the workspace, folded in a fixed order).
 *   Outputs may be NULL (not computed).  flags: BANET_ADJOINT_OVERWRITE (below) writes every entry of ddata / dinit / dbasis /
 *   dWc, zeros where nothing lands; without it they are accumulated (+=).  Same bits as accumulating into zeros.
 *   Limits (resampler): C <= 256 and B H W C < 2^32, else workspace_bytes = 0 and BANET_ERR_UNSUPPORTED.  The workspace
 *   (256-byte aligned, at least workspace_bytes) is required.  Everything is enqueued on `stream` (graph-capturable).        */
size_t banet_resample_grad_workspace_bytes(int B, int N, int C, int H, int W, int mode); /* 0 = unsupported */
int banet_resample_grad_f32(const float* data, const float* warp, const float* gout,
                            float* ddata /* [B,H,W,C] or NULL */, float* dwarp /* [B,N,2] or NULL */,
                            int B, int N, int C, int H, int W, int mode, int flags,
                            void* ws, size_t ws_bytes, banet_stream_t stream);
size_t banet_depth_output_grad_workspace_bytes(int B, int N, int K);
int banet_depth_output_grad_f32(const float* basis, const float* Wc, const float* gout,
                                float* dinit, float* dbasis, float* dWc, /* each may be NULL */
                                int B, int N, int K, int flags, void* ws, size_t ws_bytes,
                                banet_stream_t stream);

/* (6c) dense level preparation: a map resampled onto the PIXEL GRIDS of up to 8 pyramid levels, and the adjoint of all of them --
 *     what bundlenet.py:343-344 and their gradients become when every pixel of a level is a BA point (the decoder's depth
 *     and basis maps at every level's own resolution).  Level l's pixel (i, j) samples the map at
 *         x = j sx + ox,  y = i sy + oy      (two float32 roundings each, never an fma: numpy float32 j * sx + ox)
 *     with the mode, the footprint and the tap sum of banet_resample_f32; no warp tensor exists.
 *   banet_grid_resample_f32       data [B,H,W,C] -> levels[l].out [B,Ho,Wo,C], every level in one launch.
 *   banet_grid_resample_grad_f32  ddata [B,H,W,C] (= or +=) sum over the levels and over the output pixels whose taps include
 *       the texel of tap weight x levels[l].out[b,i,j,:] (here the level's gout, read only); CLAMP: taps clamped onto one texel
 *       each add their own weight.  One launch over the texels, each summed in a fixed order (levels ascending, then i, then j,
 *       then the forward's tap order): no float atomics, bit-reproducible.  flags: BANET_ADJOINT_OVERWRITE writes every texel
 *       (zeros where nothing lands); without it the sums are added to ddata.  Same bits as accumulating into zeros.
 *   `levels` is a HOST array, copied into the kernel arguments.  Neither entry takes a workspace.  Supported geometry:
 *   1 <= n_levels <= 8, 1 <= C <= 256, B <= 65535, 1/4 <= sx, sy <= 64, every sample coordinate of every level inside
 *   [-1, W] x [-1, H], H W C and every Ho Wo C below 2^30 -- else BANET_ERR_UNSUPPORTED (BANET_ERR_INVALID_ARG for a NULL
 *   pointer, a non-positive size or count, a non-finite or non-positive step, a non-finite offset, a bad mode or flag).
 *   Every check happens before the launch.  16-byte accesses where C % 4 == 0 and every pointer is 16-byte aligned.          */
typedef struct banet_grid_level {
  int32_t Ho, Wo;      /* the level's grid */
  float sx, sy, ox, oy;
  float* out;          /* [B,Ho,Wo,C]; grad call: the level's gout, read only */
} banet_grid_level_t;
int banet_grid_resample_f32(const float* data, int B, int H, int W, int C, int mode,
                            const banet_grid_level_t* levels, int n_levels, banet_stream_t stream);
int banet_grid_resample_grad_f32(float* ddata, int B, int H, int W, int C, int mode,
                                 const banet_grid_level_t* levels, int n_levels, int flags, banet_stream_t stream);

/* (7) differentiable layer support -- the C-wide part of one BundleIteration / CameraIteration in the reference's
 *     own tensor layout (bundlenet.py:230-243) and its adjoint (what TF autodiff derives from the same statements),
 *     so that a training graph never materialises samp [B,N,3C], diff, grad or J [B,N,2,P]:
 *   banet_sample_stats_f32      conv1 [B,N,C], conv2 [B,H,W,3C] = [f|gx|gy], px, py [B,N] ->
 *       stats [B,N,8] = (M11, M12, M22, g1, g2, mask, 0, 0) with M = G^T G, g = G^T d,
 *       d = (conv1 - samp_f) mask, G = [samp_gx, samp_gy] mask, mask = px in [0,W-1] and py in [0,H-1];
 *       absd_part [B, banet_sample_stats_blocks(N), C] = per-block sums of |d| (add them in order for sum_n |d|)
 *   banet_sample_stats_grad_f32 dstats [B,N,8] (first five used), dabs [B,C] = dL/d(sum_n |d|) ->
 *       dconv1 [B,N,C], dconv2 [B,H,W,3C] (ACCUMULATED with float atomics: zero it first), dpos [B,N,2] = dL/d(px,py)
 *     C <= 256, B H W 3C < 2^32.                                                                                   */
int banet_sample_stats_blocks(int N);
int banet_sample_stats_f32(const float* conv1, const float* conv2, const float* px, const float* py, int B, int N, int C,
                           int H, int W, float* stats, float* absd_part, banet_stream_t stream);
int banet_sample_stats_grad_f32(const float* conv1, const float* conv2, const float* px, const float* py, int B, int N,
                                int C, int H, int W, const float* dstats, const float* dabs, float* dconv1,
                                float* dconv2, float* dpos, banet_stream_t stream);

/*   banet_sample_stats_grad_det_f32: the same gradients with dconv2 accumulated WITHOUT float atomics -- every point
 *     writes its 3C contribution row and (target cell, bilinear fractions); per texel the contributions are then gathered
 *     in a fixed order (cells row-major, ascending point index): bit-reproducible training gradients.  Workspace from
 *     banet_sample_stats_grad_workspace_bytes (3C + 12 floats per point, 16 bytes per texel).                            */
size_t banet_sample_stats_grad_workspace_bytes(int B, int N, int C, int H, int W);
int banet_sample_stats_grad_det_f32(const float* conv1, const float* conv2, const float* px, const float* py, int B, int N,
                                    int C, int H, int W, const float* dstats, const float* dabs, float* dconv1,
                                    float* dconv2, float* dpos, void* ws, size_t ws_bytes, banet_stream_t stream);

/* (7b) backward of the fused dense assembly (3) -- SURVEY.md 8(f1).  Given the upstream gradients of ONE assembly pass at
 *     the state (R, T, Wc),
 *       gAtA [B,P,P] (any matrix: symmetrised internally, utils.cu:648-657 assumes symmetry), gAtb [B,P],
 *       gabs [B,C] = dL/d(sum_n |d_nc|)  (= dL/d avg / N for bundlenet.py:243),
 *     it ACCUMULATES (+=, so that the iterations of a level share one buffer; zero them first)
 *       dsrc [B,N,C], dmap3 [B,H,W,3C] = adjoint of the target's [f|gx|gy] map (bundlenet.py:323-324), ddepth [B,N],
 *       dbasis [B,N,K]
 *     and WRITES dpose [B, 12 + K] = (dL/dR [9], dL/dT [3], dL/dWc [K]) through the assembly (the caller adds the
 *     direct dependence of the update step on R, T, Wc).  What TF autodiff + EquationConstructionGrad (bundlenet.py:79-82,
 *     utils.cu:465-694) compute for bundlenet.py:206-263, per pixel, without J / G / d in memory.  Bit-reproducible:
 *     the target-map adjoint is gathered per texel in a fixed order (integer atomics only build the cell lists).
 *     Supported: dense = 1 with tgt_has_grad = 0 -- or (round 5) the reference's own sparse layout, dense = 0 with tgt_has_grad = 1:
 *     src = conv1 [B,N,C] at N sampled points, rays / fx / fy / ox / oy per point, tgt = the [f|gx|gy] map [B,H,W,3C]
 *     (bundlenet.py:332-399, what the reference trains on); dmap3 is then the gradient of that map itself --, pairs <= 1,
 *     C <= 256 (sparse: not C > 128 together with K > 128), and BANET_BUNDLE with 1 <= K <= 256 or the pose-only
 *     BANET_BUNDLE_CAMERA (bundlenet.py:122-191: K = 0, P = 6; basis / Wc / dbasis are not touched and may be NULL); else
 *     workspace_bytes = 0 and BANET_ERR_UNSUPPORTED.  A multi-frame window (pairs > 1) is the sum of its frames' two-frame
 *     terms: call once per target frame with the frame's sub-blocks of gAtA / gAtb (banet_amd/dense_train.py does).
 *   banet_target_map_adjoint_f32: dimg [B,H,W,C] += dmap3_f + grad_fixed^T (dmap3_gx, dmap3_gy) -- the adjoint of
 *     banet_target_map_f32 (REFLECT rim: zero gradient on the 1-px border, bundlenet.py:92-100); once per level.      */
size_t banet_dense_adjoint_workspace_bytes(const banet_level_t* lv);
/*   banet_spd_solve_f32: x [B,P] = A^-1 rhs for B symmetric positive definite systems A [B,P,P] (the blocked LDL^T of (4) as an op
 *     of its own; the matrix must fit the LDS: 32 <= P <= ~190, else BANET_ERR_UNSUPPORTED).  The backward of the layer calls it
 *     twice per iteration -- the damped system of bundlenet.py:264-267 again, then lam = A^-T g for the implicit-function gradient
 *     of tf.matrix_solve (dA = -lam x^T, db = lam).                                                                      */
int banet_spd_solve_f32(const float* A, const float* rhs, float* x, int B, int P, banet_stream_t stream);
int banet_dense_adjoint_f32(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const float* gAtA,
                            const float* gAtb, const float* gabs, float* dsrc, float* dmap3, float* ddepth,
                            float* dbasis, float* dpose, void* ws, size_t ws_bytes, banet_stream_t stream);
/*   banet_dense_adjoint_ex_f32: the same with flags.  BANET_ADJOINT_OVERWRITE: dsrc / ddepth / dbasis are WRITTEN -- every
 *     entry, zeros where nothing contributes -- instead of accumulated; BANET_ADJOINT_OVERWRITE_MAP: the same for dmap3.  The first
 *     call of a level (its last iteration; per target frame for dmap3, the first frame only for the buffers the frames share)
 *     then needs no zero-filled buffers and reads none (25 GB of fills + 25 GB of reads per 32-window 640x480 level).  Same bits
 *     as accumulating into zeros.  banet_target_map_adjoint_ex_f32 with BANET_ADJOINT_OVERWRITE: dimg is written, not added to. */
/*   BANET_ADJOINT_FOLD_TARGET (round 6; dense layout only -- dense = 1, tgt_has_grad = 0): `dmap3` is the gradient of the TARGET MAP
 *     itself, [B,H,W,C] -- the adjoint of the bilinear sampling AND of grad_fixed (bundlenet.py:92-100, REFLECT rim -> 0) in one
 *     step, accumulated (BANET_ADJOINT_OVERWRITE_MAP: written, every texel) per small texel tile in LDS by the one wave that owns the
 *     tile, pixels in a fixed order (cells row-major, ascending pixel index): still no float atomics between waves, still
 *     bit-reproducible.  Neither the per-pixel 3C adjoint rows nor the [f|gx|gy] map adjoint exist, and banet_target_map_adjoint_f32
 *     is not called: 3C (N + HW) floats less memory per window, about a third of the backward's traffic.  The workspace layout
 *     differs: size it with banet_dense_adjoint_workspace_bytes_ex(lv, flags) (0 = unsupported: a window's H W C must stay below 2^30,
 *     the tile kernels use 32-bit byte offsets inside a window).  BANET_ADJOINT_TILE_SHAPE(k), k = 1 .. 13: development
 *     switch (A/B) -- the tile kernel and its tile shape (csrc/adjoint_plan.hpp: choose_adj_tile and its shape lists); 0 = the default.                    */
/*   BANET_ADJOINT_REUSE_DEPTH_SEED (multi-frame windows: the calls for target frames 2 .. of one iteration): the caller states that
 *     the depth block of gAtA, the depth part of gAtb, lv->basis and the workspace are those of the PREVIOUS call -- then z2 = 2 S_dd b,
 *     zeta = b.S_dd b and e = gAtb_d.b of that call are still in the workspace and only the frame's q = S_cd b is computed (one
 *     column block of the GEMM-shaped piece instead of K/16 + 1).  Same bits as without the flag; ignored where it does not apply.   */
enum { BANET_ADJOINT_OVERWRITE = 1, BANET_ADJOINT_OVERWRITE_MAP = 2, BANET_ADJOINT_FOLD_TARGET = 4, BANET_ADJOINT_REUSE_DEPTH_SEED = 8 };
#define BANET_ADJOINT_TILE_SHAPE(k) (((k) & 15) << 4)
size_t banet_dense_adjoint_workspace_bytes_ex(const banet_level_t* lv, int flags);
int banet_dense_adjoint_ex_f32(const banet_level_t* lv, const float* R, const float* T, const float* Wc, const float* gAtA,
                               const float* gAtb, const float* gabs, float* dsrc, float* dmap3, float* ddepth,
                               float* dbasis, float* dpose, int flags, void* ws, size_t ws_bytes, banet_stream_t stream);
int banet_target_map_adjoint_f32(const float* dmap3, float* dimg, int B, int H, int W, int C, banet_stream_t stream);
int banet_target_map_adjoint_ex_f32(const float* dmap3, float* dimg, int B, int H, int W, int C, int flags,
                                    banet_stream_t stream);

/* (7c) backward of the SMALL part of one BundleIteration / CameraIteration (round 6) -- what tf.gradients derives for
 *     bundlenet.py:165-190 / :241-276 after the EquationConstruction op: avg = sum|d| / (N pairs) -> lambda MLP -> lambda = l2
 *     ||avg||^(2 + y) -> damping (bundle: last coefficient undamped, :264-266; bundle_camera: all six, no l2, :181-182) ->
 *     tf.matrix_solve -> SE(3) / W update (AngleaAxisRotation :17-37, VMatrix :39-46).  Four launches instead of a ~150-launch
 *     framework graph.  Inputs: the assembly outputs AtA [B,P,P], Atb [B,P], absres [B,C] (= sum |d|), the forward's solution
 *     delta [B,P] (banet_state_t.delta), the state BEFORE the update R [B,pairs,9], T [B,pairs,3], and the upstream gradients of
 *     the updated state gR [B,pairs,9], gT [B,pairs,3], gW [B,K].  Outputs (written): gAtA [B,P,P] (not symmetrised -- (7b) does
 *     that), gAtb [B,P], gabs [B,C] = dL/d absres, dR [B,pairs,9], dT [B,pairs,3] = the direct dependence of (R', T') on (R, T);
 *     dL/dWc = gW (W' = W + sol) is the caller's.  gmlp: the ten lambda-weight gradients, ACCUMULATED (+=, summed over the
 *     windows in window order: bit-reproducible) -- zero them before the first iteration of a level.  The damped system is solved
 *     by implicit differentiation on banet_spd_solve_f32's kernel (lam = A^-1 dL/dsol, dL/dA = -lam sol^T, dL/dAtb = lam): P must
 *     fit it (32 <= P <= ~190) or be < 32 (pose only: in-kernel Cholesky); C <= 256; variant BANET_BUNDLE (K >= 1) or
 *     BANET_BUNDLE_CAMERA (K = 0); else workspace_bytes = 0 and BANET_ERR_UNSUPPORTED.                                        */
size_t banet_small_step_adjoint_workspace_bytes(int variant, int B, int N, int C, int K, int pairs);
int banet_small_step_adjoint_f32(int variant, int B, int N, int C, int K, int pairs, float l2_regularizer_base,
                                 const banet_mlp_t* mlp, const float* AtA, const float* Atb, const float* absres,
                                 const float* delta, const float* R, const float* T, const float* gR, const float* gT,
                                 const float* gW, float* gAtA, float* gAtb, float* gabs, float* dR, float* dT,
                                 const banet_mlp_t* gmlp, void* ws, size_t ws_bytes, banet_stream_t stream);

/* (8) optional kernel timing, used by bench.py for the roofline figure.  Between
 *     banet_profile_begin and banet_profile_end every launch of the fused assembly kernel
 *     (from banet_ba_assemble_f32 / banet_lm_level_f32) is bracketed by two hipEvents recorded
 *     on its stream.  banet_profile_end synchronises those events and returns, per distinct
 *     level size (tag = points per window N), the number of launches and the summed kernel
 *     time in milliseconds.  Process-global and NOT thread-safe: a measurement aid, not part
 *     of the data path; events are created in _begin, never inside the timed region.       */
int banet_profile_begin(int max_launches);
int banet_profile_end(int max_tags, int32_t* tag_points, int32_t* tag_launches, double* tag_ms,
                      int32_t* ntags);
/*   banet_build_id: a 16-hex-digit digest of the kernel sources + compile flags this library was built from (build.sh).
 *     Measurement provenance only: bench.py refuses a PMC traffic file (profiles/pmc_traffic.json) recorded on another build.
 *   banet_profile_ranges: 1 = wrap every kernel launch of the assembly / solve path in a roctx range ("banet.gather N=...",
 *     "banet.syrk", "banet.fold", "banet.reduce", "banet.solve") so that `rocprofv3 --marker-trace` groups the kernels by
 *     role (the reference has no tracing hooks at all).  Returns 0 when the roctx library could not be
 *     loaded.  Off by default; also enabled by the environment variable BANET_ROCTX=1.                                     */
const char* banet_build_id(void);
/*   banet_gather_selection: which assembly (gather) kernel a level of this shape runs -- 0 = ba_gather_kernel (generic),
 *     1 = ba_gather128_kernel (C = 128, 8x8 tiles, direct taps), 2 = ba_gather128p_kernel (wave-private LDS patches),
 *     3 = ba_gather128s_kernel (16x16 strip segments, rolling LDS window), 4 = ba_gather128q_kernel (4x4-pixel items, one step
 *     per item: latency-bound launches); negative = error code.  The selection depends on
 *     the batch (work items per resident wave), so bench.py / the tests use this to run a one-window parity check on the
 *     kernel the full batch runs (the BANET_FLAG_FORCE_* / _NO_QUAD_GATHER bits of banet_level_t.flags).                */
int banet_gather_selection(const banet_level_t* lv);
/*   banet_syrk_selection: which depth-block contraction (SYRK) kernel banet_lm_level_f32 runs for this level AND batch size --
 *     0 = ba_syrk_kernel (LDS-tiled fp32 MFMA), 1 = ba_syrk_direct_kernel (fp32 MFMA, A/B), 2 = ba_syrk_bf16x6_kernel (fp32 operands
 *     split exactly into three bf16 pieces, six products), 3 = the syrk_wide.hip jobs (K = 256 / many frames), 4 =
 *     ba_syrk_bf16x6_kernel's fp16 two-piece form (three products, per-column power-of-two scales: throughput-bound launches of
 *     the LM loop; BANET_DEV_SYRK_F16 runs it in a single assembly pass too, BANET_DEV_NO_SYRK_F16 never); -1000 = no depth block
 *     (K = 0); other negative = error code.                                                                                    */
int banet_syrk_selection(const banet_level_t* lv);
int banet_profile_ranges(int enable);

#ifdef __cplusplus
}
#endif
#endif /* BANET_HIP_H_ */
