"""ctypes binding of libbanet_hip.so (the C ABI declared in include/banet_hip.h).

PyTorch is used only as plumbing here: device memory (`tensor.data_ptr()`), the current
HIP stream and the caching allocator for workspaces.  There is NO fallback: if the shared
library is missing or a call fails, an exception is raised.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# BANET_HIP_LIB: development override (same-box A/B of two builds of the library, tools/ab_builds.sh); the in-tree build otherwise
LIB_PATH = os.environ.get("BANET_HIP_LIB") or os.path.join(_HERE, "lib", "libbanet_hip.so")

LEGACY_LM, LEGACY_FIXED, BUNDLE_CAMERA, BUNDLE = 0, 1, 2, 3

_FP = ctypes.c_void_p


class BanetError(RuntimeError):
    pass


class Level(ctypes.Structure):
    """mirror of banet_level_t"""
    _fields_ = [("B", ctypes.c_int32), ("N", ctypes.c_int32), ("C", ctypes.c_int32), ("K", ctypes.c_int32),
                ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("variant", ctypes.c_int32),
                ("dense", ctypes.c_int32), ("tgt_has_grad", ctypes.c_int32), ("normalize_rays", ctypes.c_int32),
                ("scale", ctypes.c_float), ("pairs", ctypes.c_int32), ("flags", ctypes.c_int32), ("policy", ctypes.c_int32),
                ("src", _FP), ("tgt", _FP), ("depth", _FP), ("basis", _FP), ("rays", _FP),
                ("fx", _FP), ("fy", _FP), ("ox", _FP), ("oy", _FP), ("intr", _FP)]

    # the field's name until round 4 (tools/ and older tests still say `reserved_`): same storage
    reserved_ = property(lambda self: self.flags, lambda self, v: setattr(self, "flags", v))


POLICY_THROUGHPUT, POLICY_BATCH_INVARIANT = 0, 1   # banet_hip.h: BANET_POLICY_*
CANONICAL_BATCH = 32


# banet_level_t.flags: every bit a source of the library consults, under the names of banet_amd/csrc/dev_flags.hpp (kDevFooBar ->
# DEV_FOO_BAR; tests/test_plan_cpu.py compares the values).  0 in production.  As Level.flags
# is an int32, bit 31 is the negative number.
DEV_ABLATE_TAPS = 1 << 0           # every tap reads one fixed interior texel / point (generic kernel; BANET_ABLATE builds of the tile kernels)
DEV_ABLATE_SOURCE_ROWS = 1 << 1    # patch kernel, BANET_ABLATE builds: every source row = pixels 0..3
DEV_SPARSE_ITEMS64 = 1 << 1        # plan: sparse points stay 64 per wave item, never 16 (A/B; the bit's meaning outside BANET_ABLATE builds)
DEV_ABLATE_DEPTH_DOT = 1 << 2      # no depth dot (generic kernel; BANET_ABLATE builds of the patch kernel)
DEV_ABLATE_GATHER = 1 << 3         # no gather loop (generic kernel) / no tap arithmetic (BANET_ABLATE builds of the patch kernel)
DEV_NO_QUARTER_TILES = 1 << 4      # direct tile kernel: never quarter-tile work items (A/B)
DEV_GENERIC_GATHER = 1 << 5        # force the generic kernel where the C = 128 kernels would run (A/B experiments only)
DEV_DIRECT_GATHER = 1 << 6         # the direct tile kernel instead of the patch kernel (A/B); also keeps the 4x4-item kernel off
DEV_PATCH_NO_STAGING = 1 << 7      # patch kernel: no pixel group stages its bounding box in LDS (A/B)
DEV_SYRK_NO_BF16X6 = 1 << 8        # SYRK: ba_syrk_direct_kernel (fp32 MFMA) / the LDS-tiled kernel instead of the bf16x6 / wide kernels (A/B)
DEV_FORCE_PATCH_GATHER = 1 << 9    # the patch kernel at any size (parity tests)
DEV_QUARTER_TILES = 1 << 10        # force quarter-tile work items (A/B); with kDevForceStripGather: 8-row strip segments (parity tests)
DEV_PATCH_NO_STAGGER = 1 << 11     # patch kernel: the waves of a workgroup start together (A/B)
DEV_PATCH_PAIR_LOOP = 1 << 12      # patch kernel: force the loop over a window's target frames inside a tile (parity tests)
DEV_PATCH_ONE_PER_CU = 1 << 13     # patch kernel: 60 KB of unused dynamic LDS -> one workgroup per CU (A/B experiment, experiments/README.md)
DEV_PATCH_UNITS4 = 1 << 14         # patch kernel: 4-step units (A/B, experiments/README.md)
DEV_MLP_IN_SOLVE = 1 << 15         # LM loop: the lambda MLP inside the solve kernel, no role workgroups in the SYRK launch (A/B)
DEV_PATCH_PACKED = 1 << 16         # patch kernel: the packed patch with flat loads (A/B)
DEV_PATCH_COLUMN_MAJOR = 1 << 17   # patch kernel, 2-step units: column-major unit order (experiment)
DEV_FORCE_STRIP_GATHER = 1 << 18   # the strip kernel at any size (parity tests)
DEV_NO_STRIP_GATHER = 1 << 19      # never the strip kernel (A/B)
DEV_STRIP_DIRECT_ROWS = 1 << 20    # strip kernel: every pixel row takes the direct (window-less) path (parity tests)
DEV_STRIP_ROWS32 = 1 << 21         # strip kernel: 32-row segments (A/B, parity tests)
DEV_STRIP_FRAME_LOOP = 1 << 22     # strip kernel: a window's frames looped over inside one wave, no frame-parallel workgroups (A/B)
DEV_SOLVE_LDLT_ONLY = 1 << 23      # solve: blocked LDL^T only, no conjugate gradients (A/B and parity tests)
DEV_SYRK_F16 = 1 << 24             # the fp16 two-piece SYRK also in a single assembly pass and at any launch size
DEV_FORCE_QUAD_GATHER = 1 << 25    # the 4x4-pixel-item kernel at any size (parity tests, A/B)
DEV_ADJ_FP32_MFMA = 1 << 26        # the fp32-MFMA kernel instead of the bf16x6 form of the GEMM-shaped piece (A/B)
DEV_ADJ_PIXEL_PER_WAVE = 1 << 27   # one pixel per wave (A/B)
DEV_ADJ_TEXEL_PER_WAVE = 1 << 28   # target-map kernel: one texel per wave (A/B)
DEV_SYRK_THREE_PRODUCTS = 1 << 29  # opt-in, K = 128: the three largest of the six bf16 products only
DEV_NO_QUAD_GATHER = 1 << 30       # never the 4x4-pixel-item kernel
DEV_NO_SYRK_F16 = -(1 << 31)       # never the fp16 two-piece SYRK (A/B)


class Mlp(ctypes.Structure):
    """mirror of banet_mlp_t"""
    _fields_ = [("w", _FP * 5), ("b", _FP * 5)]


class State(ctypes.Structure):
    """mirror of banet_state_t"""
    _fields_ = [("R", _FP), ("T", _FP), ("Wc", _FP), ("iters", _FP), ("ratio", _FP), ("lambda_out", _FP),
                ("delta", _FP)]


class LmParams(ctypes.Structure):
    """mirror of banet_lm_params_t (the run-time LM configuration of legacy/ba.py:5-9)"""
    _fields_ = [("angle_change", ctypes.c_float), ("translation_change", ctypes.c_float),
                ("residual_ratio", ctypes.c_float), ("solver", ctypes.c_int32)]


SOLVER_QR, SOLVER_INVERSE = 0, 1


class SolveTrace(ctypes.Structure):
    """mirror of banet_solve_trace_t: the state after every level, [n_levels][B]... rows (every pointer optional); `depth` is a
    host array of n_levels device pointers"""
    _fields_ = [("R", _FP), ("T", _FP), ("Wc", _FP), ("lambda_out", _FP), ("delta", _FP), ("ratio", _FP), ("iters", _FP),
                ("depth", ctypes.POINTER(_FP))]


class Schedule(ctypes.Structure):
    """mirror of banet_schedule_t (banet_lm_solve_f32: all levels of a solve in one call)"""
    _fields_ = [("levels", ctypes.POINTER(Level)), ("n_levels", ctypes.c_int32), ("early_termination", ctypes.c_int32),
                ("mlps", ctypes.POINTER(ctypes.POINTER(Mlp))), ("max_iters", ctypes.POINTER(ctypes.c_int32)),
                ("l2_base", ctypes.c_float), ("params", ctypes.POINTER(LmParams)), ("workspace", _FP),
                ("workspace_bytes", ctypes.c_size_t), ("trace", ctypes.POINTER(SolveTrace))]


class GridLevel(ctypes.Structure):
    """mirror of banet_grid_level_t (banet_grid_resample[_grad]_f32: one level's pixel grid over the map)"""
    _fields_ = [("Ho", ctypes.c_int32), ("Wo", ctypes.c_int32), ("sx", ctypes.c_float), ("sy", ctypes.c_float),
                ("ox", ctypes.c_float), ("oy", ctypes.c_float), ("out", _FP)]


class ResidualOut(ctypes.Structure):
    """mirror of banet_residual_out_t (banet_ba_residual_f32: per-pixel error maps, mask and their sums; proj / sums optional)"""
    _fields_ = [("sq", _FP), ("ab", _FP), ("mask", _FP), ("proj", _FP), ("sums", _FP)]


class ResidualGradIn(ctypes.Structure):
    """mirror of banet_residual_grad_in_t (banet_ba_residual_grad_f32: the upstream gradients of sq / ab / proj, each optional)"""
    _fields_ = [("gsq", _FP), ("gab", _FP), ("gproj", _FP)]


class ResidualGradOut(ctypes.Structure):
    """mirror of banet_residual_grad_out_t (every output optional)"""
    _fields_ = [("dsrc", _FP), ("dtgt", _FP), ("ddepth", _FP), ("dbasis", _FP), ("dWc", _FP), ("dR", _FP), ("dT", _FP)]


class MarginalsOut(ctypes.Structure):
    """mirror of banet_marginals_out_t (banet_ba_marginals_f32: pose_cov and status required, the others optional)"""
    _fields_ = [("pose_cov", _FP), ("depth_var", _FP), ("wfactor", _FP), ("logdet", _FP), ("status", _FP)]


class MarginalsGradIn(ctypes.Structure):
    """mirror of banet_marginals_grad_in_t (banet_ba_marginals_grad_f32: the upstream gradients, each optional = zeros)"""
    _fields_ = [("g_pose_cov", _FP), ("g_depth_var", _FP), ("g_logdet", _FP)]


class MarginalsGradOut(ctypes.Structure):
    """mirror of banet_marginals_grad_out_t (status required, the others optional)"""
    _fields_ = [("gAtA", _FP), ("gdamping", _FP), ("gsigma2", _FP), ("gbasis", _FP), ("status", _FP)]


class ReprojectOut(ctypes.Structure):
    """mirror of banet_reproject_out_t (banet_depth_reproject_f32: both required)"""
    _fields_ = [("depth", _FP), ("index", _FP)]


class BasisFitOut(ctypes.Structure):
    """mirror of banet_basis_fit_out_t (banet_basis_fit_f32: Wc and status required, the others optional)"""
    _fields_ = [("Wc", _FP), ("normal", _FP), ("rhs", _FP), ("stats", _FP), ("status", _FP)]


class Prior(ctypes.Structure):
    """mirror of banet_prior_t (banet_prior_apply_f32 and the *_prior_ LM entries: every pointer optional, reserved_ = 0)"""
    _fields_ = [("Lambda", _FP), ("eta", _FP), ("obs_depth", _FP), ("obs_weight", _FP), ("scale", ctypes.c_float),
                ("reserved_", ctypes.c_int32)]


class PriorGradIn(ctypes.Structure):
    """mirror of banet_prior_grad_in_t (banet_prior_terms_grad_f32: gLe / gee required, Le / ee for gscale, reserved_ = 0)"""
    _fields_ = [("gLe", _FP), ("gee", _FP), ("Le", _FP), ("ee", _FP), ("flags", ctypes.c_int32), ("reserved_", ctypes.c_int32)]


class PriorGradOut(ctypes.Structure):
    """mirror of banet_prior_grad_out_t (every pointer optional)"""
    _fields_ = [("gLambda", _FP), ("geta", _FP), ("gscale", _FP), ("gobs", _FP), ("gweight", _FP), ("gdepth", _FP), ("gbasis", _FP)]


class PosePrior(ctypes.Structure):
    """mirror of banet_pose_prior_t (banet_pose_prior_apply_f32 and the *_pose_prior_ LM entries: all three pointers or none,
    reserved_ = 0)"""
    _fields_ = [("R0", _FP), ("T0", _FP), ("Lambda", _FP), ("scale", ctypes.c_float), ("reserved_", ctypes.c_int32)]


class PosePriorGrad(ctypes.Structure):
    """mirror of banet_pose_prior_grad_t (banet_pose_prior_add_grad_f32: every pointer optional, at least one; reserved_ = 0)"""
    _fields_ = [("gR", _FP), ("gT", _FP), ("gR0", _FP), ("gT0", _FP), ("gLambda", _FP), ("gscale", _FP), ("flags", ctypes.c_int32),
                ("reserved_", ctypes.c_int32)]


POSE_PRIOR_GRAD_OVERWRITE_STATE, POSE_PRIOR_GRAD_OVERWRITE_PRIOR = 1, 2  # banet_hip.h: BANET_POSE_PRIOR_GRAD_OVERWRITE_STATE / _PRIOR
PRIOR_GRAD_OVERWRITE, PRIOR_GRAD_ACCUMULATE = 1, 2  # banet_hip.h: BANET_PRIOR_GRAD_OVERWRITE / _ACCUMULATE

ADJOINT_OVERWRITE, ADJOINT_OVERWRITE_MAP = 1, 2  # banet_hip.h: BANET_ADJOINT_OVERWRITE / _OVERWRITE_MAP

EXPORTS = {
    "banet_version": (ctypes.c_int, []),
    "banet_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    "banet_equation_construction_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "banet_equation_construction_f32": (ctypes.c_int, [_FP] * 5 + [ctypes.c_int] * 4 + [_FP, ctypes.c_size_t, _FP]),
    "banet_equation_construction_grad_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "banet_equation_construction_grad_f32": (ctypes.c_int, [_FP] * 8 + [ctypes.c_int] * 4 + [_FP, ctypes.c_size_t, _FP]),
    "banet_resample_f32": (ctypes.c_int, [_FP] * 3 + [ctypes.c_int] * 6 + [_FP]),
    "banet_target_map_f32": (ctypes.c_int, [_FP] * 2 + [ctypes.c_int] * 4 + [_FP]),
    "banet_depth_output_f32": (ctypes.c_int, [_FP] * 4 + [ctypes.c_int] * 3 + [_FP]),
    "banet_resample_grad_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 6),
    "banet_resample_grad_f32": (ctypes.c_int, [_FP] * 5 + [ctypes.c_int] * 7 + [_FP, ctypes.c_size_t, _FP]),
    "banet_grid_resample_f32": (ctypes.c_int, [_FP] + [ctypes.c_int] * 5 + [ctypes.POINTER(GridLevel), ctypes.c_int, _FP]),
    "banet_grid_resample_grad_f32": (ctypes.c_int, [_FP] + [ctypes.c_int] * 5 + [ctypes.POINTER(GridLevel), ctypes.c_int, ctypes.c_int, _FP]),
    "banet_depth_output_grad_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 3),
    "banet_depth_output_grad_f32": (ctypes.c_int, [_FP] * 6 + [ctypes.c_int] * 4 + [_FP, ctypes.c_size_t, _FP]),
    "banet_sample_stats_blocks": (ctypes.c_int, [ctypes.c_int]),
    "banet_sample_stats_f32": (ctypes.c_int, [_FP] * 4 + [ctypes.c_int] * 5 + [_FP] * 3),
    "banet_sample_stats_grad_f32": (ctypes.c_int, [_FP] * 4 + [ctypes.c_int] * 5 + [_FP] * 6),
    "banet_ba_assemble_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Level)]),
    "banet_ba_assemble_f32": (ctypes.c_int, [ctypes.POINTER(Level)] + [_FP] * 7 + [_FP, ctypes.c_size_t, _FP]),
    "banet_ba_assemble_mask_f32": (ctypes.c_int, [ctypes.POINTER(Level)] + [_FP] * 8 + [_FP, ctypes.c_size_t, _FP]),
    "banet_ba_residual_f32": (ctypes.c_int, [ctypes.POINTER(Level)] + [_FP] * 3 + [ctypes.POINTER(ResidualOut), _FP]),
    "banet_ba_residual_grad_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Level), ctypes.c_int]),
    "banet_ba_residual_grad_f32": (ctypes.c_int, [ctypes.POINTER(Level)] + [_FP] * 3 + [ctypes.POINTER(ResidualGradIn), ctypes.POINTER(ResidualGradOut),
                                                  ctypes.c_int, _FP, ctypes.c_size_t, _FP]),
    "banet_ba_marginals_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Level), ctypes.c_int]),
    "banet_ba_marginals_f32": (ctypes.c_int, [ctypes.POINTER(Level)] + [_FP] * 3 + [ctypes.POINTER(MarginalsOut), _FP, ctypes.c_size_t, _FP]),
    "banet_ba_marginals_grad_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Level), ctypes.c_int]),
    "banet_ba_marginals_grad_f32": (ctypes.c_int, [ctypes.POINTER(Level)] + [_FP] * 3 + [ctypes.POINTER(MarginalsGradIn), ctypes.POINTER(MarginalsGradOut),
                                                   _FP, ctypes.c_size_t, _FP]),
    "banet_depth_reproject_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Level)]),
    "banet_depth_reproject_f32": (ctypes.c_int, [ctypes.POINTER(Level)] + [_FP] * 3 + [ctypes.POINTER(ReprojectOut), _FP, ctypes.c_size_t, _FP]),
    "banet_basis_fit_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Level)]),
    "banet_basis_fit_f32": (ctypes.c_int, [ctypes.POINTER(Level)] + [_FP] * 3 + [ctypes.POINTER(BasisFitOut), _FP, ctypes.c_size_t, _FP]),
    "banet_ba_solve_update_f32": (ctypes.c_int, [ctypes.POINTER(Level), ctypes.POINTER(Mlp), ctypes.c_float] + [_FP] * 4 +
                                  [ctypes.POINTER(State), _FP]),
    "banet_ba_solve_update_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Level)]),
    "banet_ba_solve_update_ws_f32": (ctypes.c_int, [ctypes.POINTER(Level), ctypes.POINTER(Mlp), ctypes.c_float] + [_FP] * 4 +
                                     [ctypes.POINTER(State), _FP, ctypes.c_size_t, _FP]),
    "banet_lm_level_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Level)]),
    "banet_lm_level_f32": (ctypes.c_int, [ctypes.POINTER(Level), ctypes.POINTER(Mlp), ctypes.c_float, ctypes.c_int,
                                          ctypes.c_int, ctypes.POINTER(State), _FP, ctypes.c_size_t, _FP]),
    "banet_lm_params_default": (None, [ctypes.POINTER(LmParams)]),
    "banet_lm_level_ex_f32": (ctypes.c_int, [ctypes.POINTER(Level), ctypes.POINTER(Mlp), ctypes.c_float, ctypes.c_int,
                                             ctypes.c_int, ctypes.POINTER(LmParams), ctypes.POINTER(State), _FP,
                                             ctypes.c_size_t, _FP]),
    "banet_lm_solve_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Schedule)]),
    "banet_lm_solve_f32": (ctypes.c_int, [ctypes.POINTER(Schedule), ctypes.POINTER(State), _FP]),
    "banet_prior_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Level), ctypes.POINTER(Prior)]),
    "banet_prior_apply_f32": (ctypes.c_int, [ctypes.POINTER(Level), ctypes.POINTER(Prior)] + [_FP] * 3 + [_FP, ctypes.c_size_t, _FP]),
    "banet_lm_level_prior_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Level), ctypes.POINTER(Prior)]),
    "banet_lm_level_prior_f32": (ctypes.c_int, [ctypes.POINTER(Level), ctypes.POINTER(Mlp), ctypes.c_float, ctypes.c_int,
                                                ctypes.POINTER(LmParams), ctypes.POINTER(Prior), ctypes.POINTER(State), _FP,
                                                ctypes.c_size_t, _FP]),
    "banet_lm_solve_prior_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Schedule), ctypes.POINTER(Prior)]),
    "banet_lm_solve_prior_f32": (ctypes.c_int, [ctypes.POINTER(Schedule), ctypes.POINTER(Prior), ctypes.POINTER(State), _FP]),
    "banet_prior_terms_f32": (ctypes.c_int, [ctypes.POINTER(Level), ctypes.POINTER(Prior)] + [_FP] * 2 + [_FP, ctypes.c_size_t, _FP]),
    "banet_prior_add_grad_f32": (ctypes.c_int, [ctypes.POINTER(Level)] + [_FP] * 7 + [ctypes.c_int, _FP]),
    "banet_prior_terms_grad_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Level), ctypes.POINTER(Prior)]),
    "banet_prior_terms_grad_f32": (ctypes.c_int, [ctypes.POINTER(Level), ctypes.POINTER(Prior), ctypes.POINTER(PriorGradIn),
                                                  ctypes.POINTER(PriorGradOut), _FP, ctypes.c_size_t, _FP]),
    "banet_pose_prior_apply_f32": (ctypes.c_int, [ctypes.POINTER(Level), ctypes.POINTER(PosePrior)] + [_FP] * 4 + [_FP]),
    "banet_pose_prior_add_grad_f32": (ctypes.c_int, [ctypes.POINTER(Level), ctypes.POINTER(PosePrior)] + [_FP] * 4 +
                                      [ctypes.POINTER(PosePriorGrad), _FP]),
    "banet_lm_level_pose_prior_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Level), ctypes.POINTER(Prior), ctypes.POINTER(PosePrior)]),
    "banet_lm_level_pose_prior_f32": (ctypes.c_int, [ctypes.POINTER(Level), ctypes.POINTER(Mlp), ctypes.c_float, ctypes.c_int,
                                                     ctypes.POINTER(LmParams), ctypes.POINTER(Prior), ctypes.POINTER(PosePrior),
                                                     ctypes.POINTER(State), _FP, ctypes.c_size_t, _FP]),
    "banet_lm_solve_pose_prior_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Schedule), ctypes.POINTER(Prior), ctypes.POINTER(PosePrior)]),
    "banet_lm_solve_pose_prior_f32": (ctypes.c_int, [ctypes.POINTER(Schedule), ctypes.POINTER(Prior), ctypes.POINTER(PosePrior),
                                                     ctypes.POINTER(State), _FP]),
    "banet_sample_stats_grad_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 5),
    "banet_sample_stats_grad_det_f32": (ctypes.c_int, [_FP] * 4 + [ctypes.c_int] * 5 + [_FP] * 5 + [_FP, ctypes.c_size_t, _FP]),
    "banet_spd_solve_f32": (ctypes.c_int, [_FP] * 3 + [ctypes.c_int] * 2 + [_FP]),
    "banet_dense_adjoint_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(Level)]),
    "banet_dense_adjoint_workspace_bytes_ex": (ctypes.c_size_t, [ctypes.POINTER(Level), ctypes.c_int]),
    "banet_dense_adjoint_f32": (ctypes.c_int, [ctypes.POINTER(Level)] + [_FP] * 11 + [_FP, ctypes.c_size_t, _FP]),
    "banet_dense_adjoint_ex_f32": (ctypes.c_int, [ctypes.POINTER(Level)] + [_FP] * 11 + [ctypes.c_int, _FP, ctypes.c_size_t, _FP]),
    "banet_small_step_adjoint_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 6),
    "banet_small_step_adjoint_f32": (ctypes.c_int, [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.POINTER(Mlp)] + [_FP] * 14 +
                                     [ctypes.POINTER(Mlp), _FP, ctypes.c_size_t, _FP]),
    "banet_target_map_adjoint_f32": (ctypes.c_int, [_FP] * 2 + [ctypes.c_int] * 4 + [_FP]),
    "banet_target_map_adjoint_ex_f32": (ctypes.c_int, [_FP] * 2 + [ctypes.c_int] * 5 + [_FP]),
    "banet_build_id": (ctypes.c_char_p, []),
    "banet_gather_selection": (ctypes.c_int, [_FP]),
    "banet_syrk_selection": (ctypes.c_int, [_FP]),
    "banet_profile_ranges": (ctypes.c_int, [ctypes.c_int]),
    "banet_profile_begin": (ctypes.c_int, [ctypes.c_int]),
    "banet_profile_end": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                         ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]),
}

_lib = None


def lib():
    """Load libbanet_hip.so (once).  Raises BanetError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BanetError("%s not found: build it with banet_amd/csrc/build.sh (or __graft_entry__.build())"
                             % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise BanetError("libbanet_hip: %s (%d)" % (lib().banet_error_string(rc).decode(), rc))


def ptr(t):
    """device pointer of a contiguous float32/int32 CUDA(HIP) tensor (None -> NULL)"""
    if t is None:
        return None
    if not t.is_cuda:
        raise BanetError("banet_amd runs on the GPU only: got a %s tensor" % t.device)
    if not t.is_contiguous():
        raise BanetError("tensor must be contiguous")
    if t.dtype not in (torch.float32, torch.int32):
        raise BanetError("tensor must be float32/int32, got %s" % t.dtype)
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(nbytes, device):
    """256-byte aligned scratch from the caching allocator"""
    n = max(int(nbytes), 256)
    buf = torch.empty(n + 256, dtype=torch.uint8, device=device)
    off = (-buf.data_ptr()) % 256
    return buf[off:off + n]


def f32c(t):
    return t.contiguous().to(torch.float32)
