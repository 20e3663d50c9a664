"""Operator layer: the reference's custom ops (`util.equation_construction`,
`util.equation_construction_grad`, bundlenet.py:76-82) and the fused entry points, each a
thin call into libbanet_hip.so through its C ABI.  GPU only -- no CPU / eager fallback.
"""
import collections
import ctypes
from typing import Tuple

import torch

from . import _capi as capi

_VARIANT_OF = {"legacy_lm": capi.LEGACY_LM, "legacy_fixed": capi.LEGACY_FIXED,
               "bundle_camera": capi.BUNDLE_CAMERA, "bundle": capi.BUNDLE}


# --------------------------------------------------------------------------------------
# EquationConstruction (+Grad)                      utils.cu:150-171 / :420-428
# --------------------------------------------------------------------------------------
def _eq_shapes(jacobian, gradient, difference):
    B, N, two, P = jacobian.shape
    Bg, Ng, C, two2 = gradient.shape
    if two != 2 or two2 != 2 or (Bg, Ng) != (B, N) or tuple(difference.shape) != (B, N, C, 1):
        raise capi.BanetError("equation_construction: expected J[B,N,2,P], G[B,N,C,2], d[B,N,C,1]; got %s %s %s"
                              % (tuple(jacobian.shape), tuple(gradient.shape), tuple(difference.shape)))
    return B, N, C, P


def equation_construction_forward(jacobian, gradient, difference):
    J, G, d = capi.f32c(jacobian), capi.f32c(gradient), capi.f32c(difference)
    B, N, C, P = _eq_shapes(J, G, d)
    L = capi.lib()
    left = torch.empty((B, P, P), dtype=torch.float32, device=J.device)
    right = torch.empty((B, P, 1), dtype=torch.float32, device=J.device)
    nb = L.banet_equation_construction_workspace_bytes(B, N, C, P)
    if nb == 0:
        raise capi.BanetError("equation_construction: unsupported shape B=%d N=%d C=%d P=%d" % (B, N, C, P))
    ws = capi.workspace(nb, J.device)
    capi.check(L.banet_equation_construction_f32(capi.ptr(J), capi.ptr(G), capi.ptr(d), capi.ptr(left), capi.ptr(right),
                                                 B, N, C, P, ctypes.c_void_p(ws.data_ptr()),
                                                 ws.numel(), capi.stream()))
    return left, right


def equation_construction_grad(jacobian, gradient, difference, left_grad, right_grad):
    """`util.equation_construction_grad` (bundlenet.py:78,81)."""
    J, G, d = capi.f32c(jacobian), capi.f32c(gradient), capi.f32c(difference)
    g0, g1 = capi.f32c(left_grad), capi.f32c(right_grad)
    B, N, C, P = _eq_shapes(J, G, d)
    L = capi.lib()
    gJ, gG, gd = torch.empty_like(J), torch.empty_like(G), torch.empty_like(d)
    nb = L.banet_equation_construction_grad_workspace_bytes(B, N, C, P)      # 0: no workspace needed for this shape
    ws = capi.workspace(nb, J.device) if nb else None
    capi.check(L.banet_equation_construction_grad_f32(capi.ptr(J), capi.ptr(G), capi.ptr(d), capi.ptr(g0), capi.ptr(g1),
                                                      capi.ptr(gJ), capi.ptr(gG), capi.ptr(gd), B, N, C, P,
                                                      ctypes.c_void_p(ws.data_ptr()) if nb else None, ws.numel() if nb else 0,
                                                      capi.stream()))
    return gJ, gG, gd


class _EquationConstruction(torch.autograd.Function):
    """forward = EquationConstruction, backward = EquationConstructionGrad: the pairing the
    reference registers with @ops.RegisterGradient (bundlenet.py:79-82)."""

    @staticmethod
    def forward(ctx, jacobian, gradient, difference, symmetric_grad):
        ctx.save_for_backward(jacobian, gradient, difference)
        ctx.symmetric_grad = bool(symmetric_grad)
        return equation_construction_forward(jacobian, gradient, difference)

    @staticmethod
    def backward(ctx, left_grad, right_grad):
        J, G, d = ctx.saved_tensors
        if ctx.symmetric_grad:
            left_grad = 0.5 * (left_grad + left_grad.transpose(1, 2))
        return equation_construction_grad(J, G, d, left_grad, right_grad) + (None,)


def equation_construction(jacobian, gradient, difference, symmetric_grad=False):
    """`util.equation_construction(jacobian=, gradient=, difference=)` -> (AtA [B,P,P], Atb [B,P,1]).
    The registered gradient is the reference's (utils.cu:648-657: dA = 2 A g0 + d g1^T), which is the
    true gradient only for a symmetric upstream g0 = dL/dAtA.  symmetric_grad=True feeds it
    (g0 + g0^T)/2 instead -- the exact gradient for any g0, identical to the reference's whenever the
    reference's is exact."""
    return _EquationConstruction.apply(jacobian, gradient, difference, symmetric_grad)


# torch.ops.banet.equation_construction / equation_construction_grad: the same two kernels registered with the
# dispatcher (the counterpart of REGISTER_OP + @ops.RegisterGradient, utils.cu:150-171,420-428 and
# bundlenet.py:79-82).  Device type "cuda" only (= HIP here): a CPU tensor raises NotImplementedError.
@torch.library.custom_op("banet::equation_construction", mutates_args=(), device_types="cuda")
def _eq_op(jacobian: torch.Tensor, gradient: torch.Tensor, difference: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return equation_construction_forward(jacobian, gradient, difference)


@_eq_op.register_fake
def _eq_op_fake(jacobian, gradient, difference):
    B, _, _, P = jacobian.shape
    return jacobian.new_empty((B, P, P)), jacobian.new_empty((B, P, 1))


@torch.library.custom_op("banet::equation_construction_grad", mutates_args=(), device_types="cuda")
def _eq_grad_op(jacobian: torch.Tensor, gradient: torch.Tensor, difference: torch.Tensor, left_grad: torch.Tensor,
                right_grad: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return equation_construction_grad(jacobian, gradient, difference, left_grad, right_grad)


@_eq_grad_op.register_fake
def _eq_grad_op_fake(jacobian, gradient, difference, left_grad, right_grad):
    return torch.empty_like(jacobian), torch.empty_like(gradient), torch.empty_like(difference)


def _eq_op_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _eq_op_backward(ctx, left_grad, right_grad):
    J, G, d = ctx.saved_tensors
    return torch.ops.banet.equation_construction_grad(J, G, d, left_grad.contiguous(), right_grad.contiguous())


_eq_op.register_autograd(_eq_op_backward, setup_context=_eq_op_setup)


# --------------------------------------------------------------------------------------
# fused path
# --------------------------------------------------------------------------------------
class MlpWeights:
    """Device copies of the five k=1 conv layers lambda_<level>_<i>_{filters,biases}
    (bundlenet.py:102-110,168-172): filters [Cin,Cout] row-major, biases [Cout]."""

    def __init__(self, layers, device, C=None):
        if len(layers) != 5:
            raise capi.BanetError("the lambda predictor has 5 layers, got %d" % len(layers))
        self.w = [torch.as_tensor(w, dtype=torch.float32).reshape(w.shape[-2], w.shape[-1]).contiguous().to(device)
                  for w, _ in layers]
        self.b = [torch.as_tensor(b, dtype=torch.float32).reshape(-1).contiguous().to(device) for _, b in layers]
        self.C = int(self.w[0].shape[0])
        self.check(self.C if C is None else C)
        self.c = capi.Mlp()
        for i in range(5):
            self.c.w[i] = self.w[i].data_ptr()
            self.c.b[i] = self.b[i].data_ptr()


    def check(self, C):
        """The solve kernel reads the layers with the fixed extents C -> 2C -> 4C -> 2C -> C -> 1
        (bundlenet.py:168-172): anything else would be an out-of-bounds device read, so refuse it here."""
        dims = [C, 2 * C, 4 * C, 2 * C, C, 1]
        for i in range(5):
            if tuple(self.w[i].shape) != (dims[i], dims[i + 1]) or tuple(self.b[i].shape) != (dims[i + 1],):
                raise capi.BanetError("lambda MLP layer %d: expected filters [%d,%d] and biases [%d] for C = %d feature "
                                      "channels, got %s and %s" % (i + 1, dims[i], dims[i + 1], dims[i + 1], C,
                                                                   tuple(self.w[i].shape), tuple(self.b[i].shape)))


class MlpCache:
    """Device copies of per-level lambda weights, rebuilt whenever a level's weights are replaced or modified in place
    (checkpoint reload, optimizer step): keyed on the identity and autograd version counter of every weight tensor;
    weights held as numpy arrays (no version counter) are re-uploaded on every call."""

    def __init__(self):
        self._d = {}

    def get(self, lambda_weights, level, device):
        level = str(level)
        if level not in lambda_weights:
            raise KeyError("no lambda weights for level %r (set lambda_weights[level])" % (level,))
        layers = lambda_weights[level]
        flat = [t for pair in layers for t in pair]
        versioned = all(torch.is_tensor(t) for t in flat)
        sig = tuple((id(t), t._version) for t in flat) if versioned else None
        key = (level, str(device))
        hit = self._d.get(key)
        if hit is None or sig is None or hit[0] != sig:
            # the entry keeps the source tensors alive: their id()s cannot be recycled by new tensors (del + reload from a
            # checkpoint at the same addresses with _version 0) while the signature still names them
            hit = (sig, MlpWeights(layers, device), flat)
            self._d[key] = hit
        return hit[1]

    def clear(self):
        self._d.clear()


def lm_params(angle_change=None, translation_change=None, residual_ratio=None, qr=None):
    """banet_lm_params_t: the reference's module globals legacy/ba.py:5-9 as a value (None = the reference's default)."""
    p = capi.LmParams()
    capi.lib().banet_lm_params_default(ctypes.byref(p))
    if angle_change is not None:
        p.angle_change = float(angle_change)
    if translation_change is not None:
        p.translation_change = float(translation_change)
    if residual_ratio is not None:
        p.residual_ratio = float(residual_ratio)
    if qr is not None:
        p.solver = capi.SOLVER_QR if qr else capi.SOLVER_INVERSE
    return p


class LmState:
    """Per-window LM state (banet_state_t): R [B,3,3], T [B,3,1], Wc [B,K,1] + diagnostics.
    Multi-frame windows (pairs > 1): R [B,pairs,3,3], T [B,pairs,3,1]."""

    def __init__(self, R, T, Wc=None, P=6, pairs=1):
        dev = R.device
        B = R.shape[0]
        shape = (B,) if pairs == 1 else (B, pairs)
        self.R = capi.f32c(R).clone().reshape(*shape, 3, 3)
        self.T = capi.f32c(T).clone().reshape(*shape, 3, 1)
        self.Wc = capi.f32c(Wc).clone() if Wc is not None else None
        self.iters = torch.zeros(B, dtype=torch.int32, device=dev)
        self.ratio = torch.zeros(B, dtype=torch.float32, device=dev)
        self.lambda_out = torch.zeros(B, dtype=torch.float32, device=dev)
        self.delta = torch.zeros(B, P, dtype=torch.float32, device=dev)
        self.c = capi.State()
        self.c.R = self.R.data_ptr()
        self.c.T = self.T.data_ptr()
        self.c.Wc = self.Wc.data_ptr() if self.Wc is not None else None
        self.c.iters = self.iters.data_ptr()
        self.c.ratio = self.ratio.data_ptr()
        self.c.lambda_out = self.lambda_out.data_ptr()
        self.c.delta = self.delta.data_ptr()


class LevelProblem:
    """One banet_level_t plus the tensors it points at (kept alive here)."""

    def __init__(self, variant, src, tgt, depth, H, W, C, basis=None, rays=None, fx=None, fy=None, ox=None, oy=None,
                 intr=None, scale=1.0, dense=False, tgt_has_grad=True, normalize_rays=False, pairs=1):
        """pairs > 1: multi-frame window, tgt [B,pairs,H,W,C(3C)] (banet_level_t.pairs)"""
        v = _VARIANT_OF[variant] if isinstance(variant, str) else int(variant)
        keep = [capi.f32c(x) if x is not None else None for x in (src, tgt, depth, basis, rays, fx, fy, ox, oy, intr)]
        src, tgt, depth, basis, rays, fx, fy, ox, oy, intr = keep
        self.keep = keep
        B = tgt.shape[0]
        N = depth.numel() // B
        K = 0 if basis is None else basis.shape[-1]
        lv = capi.Level()
        lv.B, lv.N, lv.C, lv.K, lv.H, lv.W = B, N, C, K, H, W
        lv.variant, lv.dense, lv.tgt_has_grad = v, int(dense), int(tgt_has_grad)
        lv.normalize_rays, lv.scale = int(normalize_rays), float(scale)
        lv.pairs = int(pairs)
        for name, t in (("src", src), ("tgt", tgt), ("depth", depth), ("basis", basis), ("rays", rays), ("fx", fx),
                        ("fy", fy), ("ox", ox), ("oy", oy), ("intr", intr)):
            setattr(lv, name, None if t is None else t.data_ptr())
            if t is not None and not t.is_cuda:
                raise capi.BanetError("banet_amd runs on the GPU only (%s is on %s)" % (name, t.device))
        expect_tgt = B * int(pairs) * H * W * C * (3 if tgt_has_grad else 1)
        if tgt.numel() != expect_tgt or src.numel() != B * N * C:
            raise capi.BanetError("level tensors have inconsistent sizes")
        self.c = lv
        self.B, self.N, self.C, self.K, self.P, self.pairs = B, N, C, K, 6 * int(pairs) + K, int(pairs)
        self.device = tgt.device


GATHER_KERNELS = {0: "ba_gather_kernel", 1: "ba_gather128_kernel", 2: "ba_gather128p_kernel", 3: "ba_gather128s_kernel",
                  4: "ba_gather128q_kernel"}
FORCE_QUAD_GATHER, NO_QUAD_GATHER = capi.DEV_FORCE_QUAD_GATHER, capi.DEV_NO_QUAD_GATHER   # banet_hip.h: BANET_DEV_FORCE_QUAD_GATHER / _NO_QUAD_GATHER
FORCE_PATCH_GATHER, FORCE_STRIP_GATHER = capi.DEV_FORCE_PATCH_GATHER, capi.DEV_FORCE_STRIP_GATHER     # banet_hip.h: BANET_DEV_FORCE_PATCH_GATHER / _STRIP_GATHER (parity checks at small batch sizes)
SYRK_THREE_PRODUCTS = capi.DEV_SYRK_THREE_PRODUCTS   # banet_hip.h: BANET_DEV_SYRK_THREE_PRODUCTS -- opt-in: the K = 128 SYRK with the three largest bf16 products only (~2^-16 per product instead of fp32-exact)


SYRK_F16, NO_SYRK_F16 = capi.DEV_SYRK_F16, capi.DEV_NO_SYRK_F16          # banet_hip.h: BANET_DEV_SYRK_F16 / BANET_DEV_NO_SYRK_F16
SYRK_KERNELS = {0: "ba_syrk_kernel", 1: "ba_syrk_direct_kernel", 2: "ba_syrk_bf16x6_kernel (bf16 x 3 pieces, 6 products)",
                3: "syrk_wide.hip jobs", 4: "ba_syrk_bf16x6_kernel (fp16 x 2 pieces, 3 products, scaled)", -1000: "none (K = 0)"}


def syrk_selection(level):
    """banet_syrk_selection: the depth-block contraction kernel banet_lm_level_f32 runs for this level AND batch size"""
    rc = capi.lib().banet_syrk_selection(ctypes.byref(level.c))
    if rc < 0 and rc != -1000:
        capi.check(rc)
    return rc


def gather_selection(level):
    """banet_gather_selection: 0 generic / 1 C=128 direct / 2 LDS patches / 3 strip segments / 4 4x4-pixel items, for this level AND batch size"""
    rc = capi.lib().banet_gather_selection(ctypes.byref(level.c))
    if rc < 0:
        capi.check(rc)
    return rc


def ba_assemble(level, R, T, Wc=None, return_mask=False):
    """banet_ba_assemble_f32 -> (AtA [B,P,P], Atb [B,P], absres [B,C], nvalid [B]); return_mask: banet_ba_assemble_mask_f32,
    additionally the in-image mask bit the kernel decided for every pixel, uint8 [B, pairs, N] (parity diagnostics)."""
    L = capi.lib()
    dev = level.device
    B, P, C = level.B, level.P, level.C
    AtA = torch.empty((B, P, P), dtype=torch.float32, device=dev)
    Atb = torch.empty((B, P), dtype=torch.float32, device=dev)
    absres = torch.empty((B, C), dtype=torch.float32, device=dev)
    nvalid = torch.empty((B,), dtype=torch.float32, device=dev)
    nb = L.banet_ba_assemble_workspace_bytes(ctypes.byref(level.c))
    if nb == 0:
        raise capi.BanetError("ba_assemble: unsupported level shape")
    ws = capi.workspace(nb, dev)
    R, T = capi.f32c(R), capi.f32c(T)
    Wc = capi.f32c(Wc) if Wc is not None else None
    if return_mask:
        pairs = max(int(level.c.pairs), 1)
        mask = torch.full((B, pairs, int(level.c.N)), 255, dtype=torch.uint8, device=dev)
        capi.check(L.banet_ba_assemble_mask_f32(ctypes.byref(level.c), capi.ptr(R), capi.ptr(T), capi.ptr(Wc), capi.ptr(AtA),
                                                capi.ptr(Atb), capi.ptr(absres), capi.ptr(nvalid), ctypes.c_void_p(mask.data_ptr()),
                                                ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
        return AtA, Atb, absres, nvalid, mask
    capi.check(L.banet_ba_assemble_f32(ctypes.byref(level.c), capi.ptr(R), capi.ptr(T), capi.ptr(Wc), capi.ptr(AtA),
                                       capi.ptr(Atb), capi.ptr(absres), capi.ptr(nvalid),
                                       ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
    return AtA, Atb, absres, nvalid


Residual = collections.namedtuple("Residual", "sq ab mask proj sums")


def ba_residual(problem, R, T, Wc=None, proj=False, sums=True):
    """banet_ba_residual_f32: what the level costs at the state (R, T, Wc), per window, target frame and point ->
    Residual(sq [B,pairs,N] = sum_c d^2, ab [B,pairs,N] = sum_c |d|, mask [B,pairs,N] uint8 (1 = in the image; sq = ab = 0 elsewhere),
    proj [B,pairs,N,2] = (px, py) or None, sums [B,pairs,4] = (sum sq, sum ab, in-image count, max sq) or None).  sums may also be
    a contiguous float32 device tensor of B * pairs * 4 elements to write into (it is returned).  Device tensors, no host sync, no
    workspace; a window's bits do not depend on the batch."""
    dev = problem.device
    B, N, pairs = problem.B, problem.N, max(int(problem.c.pairs), 1)
    R, T = capi.f32c(R), capi.f32c(T)
    Wc = capi.f32c(Wc) if Wc is not None else None
    pR, pT, pW = capi.ptr(R), capi.ptr(T), capi.ptr(Wc)      # (CPU tensors: BanetError, before anything is allocated)
    if R.numel() != B * pairs * 9 or T.numel() != B * pairs * 3 or (Wc is not None and Wc.numel() != B * problem.K):
        raise capi.BanetError("ba_residual: expected R [B,pairs,3,3], T [B,pairs,3,1], Wc [B,K,1] for B = %d, pairs = %d, K = %d"
                              % (B, pairs, problem.K))
    out = Residual(torch.empty((B, pairs, N), dtype=torch.float32, device=dev), torch.empty((B, pairs, N), dtype=torch.float32, device=dev),
                   torch.empty((B, pairs, N), dtype=torch.uint8, device=dev),
                   torch.empty((B, pairs, N, 2), dtype=torch.float32, device=dev) if proj else None,
                   sums if torch.is_tensor(sums) else torch.empty((B, pairs, 4), dtype=torch.float32, device=dev) if sums else None)
    if out.sums is not None and out.sums.numel() != B * pairs * 4:
        raise capi.BanetError("ba_residual: sums must hold B * pairs * 4 = %d floats" % (B * pairs * 4))
    c = capi.ResidualOut()
    c.sq, c.ab, c.mask = out.sq.data_ptr(), out.ab.data_ptr(), out.mask.data_ptr()
    c.proj = out.proj.data_ptr() if proj else None
    c.sums = capi.ptr(out.sums).value if out.sums is not None else None
    capi.check(capi.lib().banet_ba_residual_f32(ctypes.byref(problem.c), pR, pT, pW, ctypes.byref(c), capi.stream()))
    return out


MARGINALS_OUTPUTS = ("pose_cov", "depth_var", "wfactor", "logdet")
Marginals = collections.namedtuple("Marginals", "pose_cov depth_var wfactor logdet status")


def _per_window(v, name, B, dev, who):
    """damping / sigma2 of the marginals entries: None, a float or a tensor of 1 or B values -> None or a float32 tensor [B]"""
    if v is None:
        return None
    t = v if torch.is_tensor(v) else torch.full((B,), float(v), dtype=torch.float32, device=dev)
    t = capi.f32c(t).reshape(-1)
    if t.numel() == 1 and B > 1:
        t = t.expand(B).contiguous()
    if t.numel() != B:
        raise capi.BanetError("%s: %s must be a float or hold B = %d values" % (who, name, B))
    return t


def ba_marginals_workspace_bytes(problem, want_depth_var=True):
    """banet_ba_marginals_workspace_bytes (0 = unsupported: K > 256 or P > 304)"""
    return int(capi.lib().banet_ba_marginals_workspace_bytes(ctypes.byref(problem.c), int(bool(want_depth_var))))


def ba_marginals(problem, AtA, damping=None, sigma2=None, want=("pose_cov", "depth_var"), ws=None):
    """banet_ba_marginals_f32: how well the normal equations AtA [B,P,P] (ba_assemble) determine their answer.  With
    H = AtA + damping diag(diag(AtA) + 1e-5) (every diagonal entry) and Sigma = sigma2 H^-1 ->
    Marginals(pose_cov [B,6 pairs,6 pairs] = the poses' joint marginal, depth_var [B,N] = the variance of depth + basis . Wc per
    point, wfactor [B,K,K] = T lower triangular with Sigma_WW = sigma2 T^T T, logdet [B] = log det H, status [B] int32: 0, or 1
    where H is not positive definite (that window: depth_var = +inf, pose_cov = +inf on the diagonal, wfactor = 0, logdet = -inf)).
    damping, sigma2: None (0 and 1), a float, or a tensor [B].  `want` names the optional outputs to compute (pose_cov and status
    always are; depth_var / wfactor of a level without a basis are None); the others are None.  `problem` needs .c (a
    banet_level_t with B, N, K, pairs and basis set) only.  Device tensors, no host sync; a window's bits do not depend on the
    batch nor on `want`."""
    L = capi.lib()
    lv = problem.c
    B, N, K, pairs = int(lv.B), int(lv.N), int(lv.K), max(int(lv.pairs), 1)
    m, P = 6 * pairs, 6 * pairs + K
    AtA = capi.f32c(AtA)
    pA = capi.ptr(AtA)                      # (a CPU tensor: BanetError, before anything is allocated)
    dev = AtA.device
    if AtA.numel() != B * P * P:
        raise capi.BanetError("ba_marginals: AtA must be [B,P,P] = [%d,%d,%d]" % (B, P, P))
    unknown = [w for w in want if w not in MARGINALS_OUTPUTS]
    if unknown:
        raise capi.BanetError("ba_marginals: unknown outputs %s" % unknown)

    damping, sigma2 = _per_window(damping, "damping", B, dev, "ba_marginals"), _per_window(sigma2, "sigma2", B, dev, "ba_marginals")
    pD, pS = capi.ptr(damping), capi.ptr(sigma2)
    res = dict(pose_cov=torch.empty((B, m, m), dtype=torch.float32, device=dev),
               depth_var=torch.empty((B, N), dtype=torch.float32, device=dev) if "depth_var" in want and K > 0 else None,
               wfactor=torch.empty((B, K, K), dtype=torch.float32, device=dev) if "wfactor" in want and K > 0 else None,
               logdet=torch.empty((B,), dtype=torch.float32, device=dev) if "logdet" in want else None,
               status=torch.empty((B,), dtype=torch.int32, device=dev))
    c = capi.MarginalsOut()
    for name, t in res.items():
        setattr(c, name, None if t is None else t.data_ptr())
    nb = ba_marginals_workspace_bytes(problem, res["depth_var"] is not None)
    if nb == 0:
        raise capi.BanetError("ba_marginals: unsupported shape (K <= 256 and P <= 304)")
    if ws is None or ws.numel() < nb:
        ws = capi.workspace(nb, dev)
    capi.check(L.banet_ba_marginals_f32(ctypes.byref(lv), pA, pD, pS, ctypes.byref(c), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                        capi.stream()))
    return Marginals(**res)


MARGINALS_GRAD_OUTPUTS = ("gAtA", "gdamping", "gsigma2", "gbasis")
MarginalsGrad = collections.namedtuple("MarginalsGrad", "gAtA gdamping gsigma2 gbasis status")


def ba_marginals_grad(problem, AtA, damping=None, sigma2=None, g_pose_cov=None, g_depth_var=None, g_logdet=None,
                      want=("gAtA", "gbasis"), ws=None):
    """banet_ba_marginals_grad_f32: the backward of ba_marginals.  g_pose_cov [B,6 pairs,6 pairs] (need not be symmetric),
    g_depth_var [B,N], g_logdet [B]: dL/dpose_cov, dL/ddepth_var, dL/dlogdet (None = zeros) ->
    MarginalsGrad(gAtA [B,P,P] = the gradient with respect to a symmetric AtA, exactly symmetric (the upstream gAtA of
    dense_train.dense_adjoint), gdamping [B], gsigma2 [B], gbasis [B,N,K], status [B] int32 as ba_marginals); the outputs not named
    in `want` (and gbasis of a level without a basis) are None.  The factorisation is recomputed from AtA / damping / sigma2
    (None, a float or a tensor [B], as ba_marginals); a window with status 1 gets zeros.  Every element is written.  Device tensors,
    no host sync; a window's bits do not depend on the batch nor on `want`."""
    L = capi.lib()
    lv = problem.c
    B, N, K, pairs = int(lv.B), int(lv.N), int(lv.K), max(int(lv.pairs), 1)
    m, P = 6 * pairs, 6 * pairs + K
    AtA = capi.f32c(AtA)
    pA = capi.ptr(AtA)                      # (a CPU tensor: BanetError, before anything is allocated)
    dev = AtA.device
    if AtA.numel() != B * P * P:
        raise capi.BanetError("ba_marginals_grad: AtA must be [B,P,P] = [%d,%d,%d]" % (B, P, P))
    unknown = [w for w in want if w not in MARGINALS_GRAD_OUTPUTS]
    if unknown:
        raise capi.BanetError("ba_marginals_grad: unknown outputs %s" % unknown)
    damping = _per_window(damping, "damping", B, dev, "ba_marginals_grad")
    sigma2 = _per_window(sigma2, "sigma2", B, dev, "ba_marginals_grad")
    gin, keep = capi.MarginalsGradIn(), []
    for name, g, n in (("g_pose_cov", g_pose_cov, B * m * m), ("g_depth_var", g_depth_var, B * N), ("g_logdet", g_logdet, B)):
        if g is not None and not (name == "g_depth_var" and K == 0):
            g = capi.f32c(g)
            if g.numel() != n:
                raise capi.BanetError("ba_marginals_grad: %s must hold %d floats" % (name, n))
            keep.append(g)
            setattr(gin, name, capi.ptr(g).value)
    shapes = dict(gAtA=(B, P, P), gdamping=(B,), gsigma2=(B,), gbasis=(B, N, K))
    res = {name: torch.empty(shapes[name], dtype=torch.float32, device=dev) if name in want and not (name == "gbasis" and K == 0) else None
           for name in MARGINALS_GRAD_OUTPUTS}
    res["status"] = torch.empty((B,), dtype=torch.int32, device=dev)
    c = capi.MarginalsGradOut()
    for name, t in res.items():
        setattr(c, name, None if t is None else t.data_ptr())
    nb = int(L.banet_ba_marginals_grad_workspace_bytes(ctypes.byref(lv), int(res["gbasis"] is not None)))
    if nb == 0:
        raise capi.BanetError("ba_marginals_grad: unsupported shape (K <= 256 and P <= 304)")
    if ws is None or ws.numel() < nb:
        ws = capi.workspace(nb, dev)
    capi.check(L.banet_ba_marginals_grad_f32(ctypes.byref(lv), pA, capi.ptr(damping), capi.ptr(sigma2), ctypes.byref(gin), ctypes.byref(c),
                                             ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
    del keep
    return MarginalsGrad(**res)


class _MarginalsDiff(torch.autograd.Function):
    """ba_marginals with banet_ba_marginals_grad_f32 as its backward; the basis enters as an input so that autograd sees it"""

    @staticmethod
    def forward(ctx, problem, want, AtA, damping, sigma2, basis):
        m = ba_marginals(problem, AtA, damping=damping, sigma2=sigma2, want=want)
        ctx.problem = problem
        ctx.scalars = (None if torch.is_tensor(damping) else damping, None if torch.is_tensor(sigma2) else sigma2)
        ctx.has = (torch.is_tensor(damping), torch.is_tensor(sigma2))
        ctx.shapes = [t.shape if torch.is_tensor(t) else None for t in (AtA, damping, sigma2, basis)]
        ctx.save_for_backward(AtA, *[t for t in (damping, sigma2) if torch.is_tensor(t)])
        ctx.mark_non_differentiable(*[t for t in (m.wfactor, m.status) if t is not None])
        ctx.set_materialize_grads(False)      # an output the loss does not use arrives as None = a NULL upstream gradient
        return m.pose_cov, m.depth_var, m.wfactor, m.logdet, m.status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cov, g_dv, _g_wf, g_ld, _g_status):
        saved = list(ctx.saved_tensors)
        AtA = saved.pop(0)
        damping = saved.pop(0) if ctx.has[0] else ctx.scalars[0]
        sigma2 = saved.pop(0) if ctx.has[1] else ctx.scalars[1]
        need = ctx.needs_input_grad[2:]
        want = tuple(n for n, k in zip(MARGINALS_GRAD_OUTPUTS, need) if k and not (n == "gbasis" and int(ctx.problem.c.K) == 0))
        if not want or (g_cov is None and g_dv is None and g_ld is None):
            return (None,) * 6
        g = ba_marginals_grad(ctx.problem, AtA, damping, sigma2, g_cov, g_dv, g_ld, want=want)
        out = []
        for n, shape in zip(MARGINALS_GRAD_OUTPUTS, ctx.shapes):
            t = getattr(g, n) if n in want else None
            if t is not None and t.numel() != shape.numel():       # one damping / sigma2 value shared by the windows
                t = t.sum()
            out.append(None if t is None else t.reshape(shape))
        return (None, None) + tuple(out)


def ba_marginals_diff(problem, AtA, damping=None, sigma2=None, want=("pose_cov", "depth_var")):
    """ba_marginals attached to the autograd graph -> Marginals: pose_cov, depth_var and logdet are differentiable with respect to
    AtA (as a symmetric matrix), the basis the problem was built from, and damping / sigma2 where they are tensors that require
    grad; wfactor and status are not.  The backward is one banet_ba_marginals_grad_f32 call that asks only for the gradients some
    input needs; a window with status 1 (depth_var = +inf) sends zeros."""
    basis = problem.keep[3] if hasattr(problem, "keep") else getattr(problem, "basis", None)
    res = _MarginalsDiff.apply(problem, tuple(want), AtA, damping, sigma2, basis)
    return Marginals(*res)


Reprojection = collections.namedtuple("Reprojection", "depth index")


def depth_reproject(problem, R, T, Wc=None, ws=None):
    """banet_depth_reproject_f32: the key frame's depth map depth + basis . Wc (Wc None: depth) of a dense level reprojected into
    the pixel grid of every target frame at the poses R [B,F,3,3], T [B,F,3,1] (F = max(pairs, 1)), z-buffered ->
    Reprojection(depth [B,F,H,W] = the depth IN THE TARGET FRAME (range along the ray on normalize_rays levels, else z) of the
    nearest point that lands on the texel, 0 where nothing lands; index [B,F,H,W] int32 = that point's source pixel, -1 where
    nothing lands).  Device tensors, no host sync; integer atomics only: bit-reproducible, a window's bits do not depend on the
    batch."""
    L = capi.lib()
    lv = problem.c
    B, N, K, F = int(lv.B), int(lv.N), int(lv.K), max(int(lv.pairs), 1)
    H, W = int(lv.H), int(lv.W)
    R, T = capi.f32c(R), capi.f32c(T)
    Wc = capi.f32c(Wc) if (Wc is not None and K > 0) else None
    pR, pT, pW = capi.ptr(R), capi.ptr(T), capi.ptr(Wc)      # (CPU tensors: BanetError, before anything is allocated)
    if R.numel() != B * F * 9 or T.numel() != B * F * 3 or (Wc is not None and Wc.numel() != B * K):
        raise capi.BanetError("depth_reproject: expected R [B,F,3,3], T [B,F,3,1], Wc [B,K,1] for B = %d, F = %d, K = %d" % (B, F, K))
    dev = R.device
    nb = int(L.banet_depth_reproject_workspace_bytes(ctypes.byref(lv)))
    if nb == 0:
        raise capi.BanetError("depth_reproject: a dense level with N = H W is needed")
    out = Reprojection(torch.empty((B, F, H, W), dtype=torch.float32, device=dev), torch.empty((B, F, H, W), dtype=torch.int32, device=dev))
    c = capi.ReprojectOut()
    c.depth, c.index = out.depth.data_ptr(), out.index.data_ptr()
    if ws is None or ws.numel() < nb:
        ws = capi.workspace(nb, dev)
    capi.check(L.banet_depth_reproject_f32(ctypes.byref(lv), pR, pT, pW, ctypes.byref(c), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                           capi.stream()))
    return out


BASIS_FIT_OUTPUTS = ("Wc", "normal", "rhs", "stats")
BasisFit = collections.namedtuple("BasisFit", "Wc normal rhs stats status")


def basis_fit(depth, basis, target, weight=None, damping=None, want=("Wc",), ws=None):
    """banet_basis_fit_f32: the weighted, damped least-squares fit of a depth map on a basis.  depth [B,N] (any shape with B
    leading), basis [B,N,K], target and weight like depth (weight None: 1), damping None (0), a float or a tensor [B].  With
    r = target - depth over the points with a finite weight > 0 and a finite target:
        G = sum w b b^T    g = sum w r b    H = G + damping diag(diag(G) + 1e-5)    Wc = H^-1 g
    -> BasisFit(Wc [B,K], normal [B,K,K] = G (exactly symmetric), rhs [B,K] = g, stats [B,2] = (sum w, sum w r^2), status [B]
    int32: 0, or 1 where H is not positive definite (that window: Wc = 0)).  `want` names the optional outputs (Wc and status
    always are); the others are None.  Device tensors, no host sync; a window's bits do not depend on the batch nor on `want`."""
    L = capi.lib()
    depth, basis, target = capi.f32c(depth), capi.f32c(basis), capi.f32c(target)
    weight = capi.f32c(weight) if weight is not None else None
    pd, pb, pt, pw = capi.ptr(depth), capi.ptr(basis), capi.ptr(target), capi.ptr(weight)   # (CPU tensors: BanetError)
    B, K = int(basis.shape[0]), int(basis.shape[-1])
    N = basis.numel() // max(B * K, 1)
    if depth.numel() != B * N or target.numel() != B * N or (weight is not None and weight.numel() != B * N):
        raise capi.BanetError("basis_fit: expected depth / target / weight [B,N] and basis [B,N,K] with B = %d, N = %d" % (B, N))
    unknown = [w for w in want if w not in BASIS_FIT_OUTPUTS]
    if unknown:
        raise capi.BanetError("basis_fit: unknown outputs %s" % unknown)
    dev = basis.device
    if damping is not None:
        damping = damping if torch.is_tensor(damping) else torch.full((B,), float(damping), dtype=torch.float32, device=dev)
        damping = capi.f32c(damping).reshape(-1)
        if damping.numel() == 1 and B > 1:
            damping = damping.expand(B).contiguous()
        if damping.numel() != B:
            raise capi.BanetError("basis_fit: damping must be a float or hold B = %d values" % B)
    lv = capi.Level()                                     # a bare level: the entry reads B, N, K, depth and basis only
    lv.B, lv.N, lv.K = B, N, K
    lv.depth, lv.basis = pd.value, pb.value
    nb = int(L.banet_basis_fit_workspace_bytes(ctypes.byref(lv)))
    if nb == 0:
        raise capi.BanetError("basis_fit: unsupported shape (1 <= K <= 256, N >= 1)")
    res = dict(Wc=torch.empty((B, K), dtype=torch.float32, device=dev),
               normal=torch.empty((B, K, K), dtype=torch.float32, device=dev) if "normal" in want else None,
               rhs=torch.empty((B, K), dtype=torch.float32, device=dev) if "rhs" in want else None,
               stats=torch.empty((B, 2), dtype=torch.float32, device=dev) if "stats" in want else None,
               status=torch.empty((B,), dtype=torch.int32, device=dev))
    c = capi.BasisFitOut()
    for name, t in res.items():
        setattr(c, name, None if t is None else t.data_ptr())
    if ws is None or ws.numel() < nb:
        ws = capi.workspace(nb, dev)
    capi.check(L.banet_basis_fit_f32(ctypes.byref(lv), pt, pw, capi.ptr(damping), ctypes.byref(c), ctypes.c_void_p(ws.data_ptr()),
                                     ws.numel(), capi.stream()))
    return BasisFit(**res)


RESIDUAL_GRAD_OUTPUTS = ("dsrc", "dtgt", "ddepth", "dbasis", "dWc", "dR", "dT")
ResidualGrad =collections.namedtuple("ResidualGrad", RESIDUAL_GRAD_OUTPUTS)


def _residual_grad_shapes(problem):
    B, N, C, K, pairs = problem.B, problem.N, problem.C, problem.K, max(int(problem.c.pairs), 1)
    H, W = int(problem.c.H), int(problem.c.W)
    return dict(dsrc=(B, N, C), dtgt=(B, pairs, H, W, C), ddepth=(B, N), dbasis=(B, N, K), dWc=(B, K), dR=(B, pairs, 9), dT=(B, pairs, 3))


def ba_residual_grad(problem, R, T, Wc, gsq=None, gab=None, gproj=None, want=RESIDUAL_GRAD_OUTPUTS, overwrite=True, into=None, ws=None):
    """banet_ba_residual_grad_f32: the backward of ba_residual.  gsq, gab [B,pairs,N], gproj [B,pairs,N,2]: dL/dsq, dL/dab, dL/dproj
    (None = zeros; at least one) -> ResidualGrad(dsrc [B,N,C], dtgt [B,pairs,H,W,C], ddepth [B,N], dbasis [B,N,K], dWc [B,K],
    dR [B,pairs,9], dT [B,pairs,3]); the outputs not named in `want` (and dbasis / dWc of a level without a basis) are None.
    overwrite=True: fresh tensors, every element written.  overwrite=False: dsrc / dtgt / ddepth / dbasis are ACCUMULATED into the
    tensors given in `into` (a dict by output name; also with overwrite=True, to choose the destination); dR / dT / dWc are always
    written.  dtgt needs a C-channel target map.  Device tensors, no host sync; bit-reproducible, a window's bits do not depend
    on the batch."""
    L = capi.lib()
    dev = problem.device
    B, N, K, pairs = problem.B, problem.N, problem.K, max(int(problem.c.pairs), 1)
    R, T = capi.f32c(R), capi.f32c(T)
    Wc = capi.f32c(Wc) if Wc is not None else None
    pR, pT, pW = capi.ptr(R), capi.ptr(T), capi.ptr(Wc)
    if R.numel() != B * pairs * 9 or T.numel() != B * pairs * 3 or (Wc is not None and Wc.numel() != B * K):
        raise capi.BanetError("ba_residual_grad: expected R [B,pairs,3,3], T [B,pairs,3,1], Wc [B,K,1] for B = %d, pairs = %d, K = %d"
                              % (B, pairs, K))
    gin = capi.ResidualGradIn()
    keep = []
    for name, g, n in (("gsq", gsq, B * pairs * N), ("gab", gab, B * pairs * N), ("gproj", gproj, B * pairs * N * 2)):
        if g is not None:
            g = capi.f32c(g)
            if g.numel() != n:
                raise capi.BanetError("ba_residual_grad: %s must hold %d floats" % (name, n))
            keep.append(g)
            setattr(gin, name, capi.ptr(g).value)
    unknown = [w for w in want if w not in RESIDUAL_GRAD_OUTPUTS]
    if unknown:
        raise capi.BanetError("ba_residual_grad: unknown outputs %s" % unknown)
    shapes = _residual_grad_shapes(problem)
    into = dict(into or {})
    res, gout = {}, capi.ResidualGradOut()
    for name in RESIDUAL_GRAD_OUTPUTS:
        res[name] = None
        if name not in want or (K == 0 and name in ("dbasis", "dWc")):
            continue
        t = into.get(name)
        if t is None:
            if not overwrite and name in ("dsrc", "dtgt", "ddepth", "dbasis"):
                raise capi.BanetError("ba_residual_grad: overwrite=False accumulates into into[%r]" % name)
            t = torch.empty(shapes[name], dtype=torch.float32, device=dev)
        elif t.numel() != int(torch.Size(shapes[name]).numel()):
            raise capi.BanetError("ba_residual_grad: into[%r] must hold %s" % (name, shapes[name]))
        res[name] = t
        setattr(gout, name, capi.ptr(t).value)
    want_dtgt = res["dtgt"] is not None
    nb = L.banet_ba_residual_grad_workspace_bytes(ctypes.byref(problem.c), int(want_dtgt))
    if nb == 0 and want_dtgt and L.banet_ba_residual_grad_workspace_bytes(ctypes.byref(problem.c), 0) != 0:
        raise capi.BanetError("ba_residual_grad: dtgt needs a C-channel target map (tgt_has_grad = 0) with C <= 256 and B pairs H W C < 2^32")
    if ws is None or ws.numel() < nb:
        ws = capi.workspace(nb, dev)
    flags = (capi.ADJOINT_OVERWRITE | capi.ADJOINT_OVERWRITE_MAP) if overwrite else 0
    capi.check(L.banet_ba_residual_grad_f32(ctypes.byref(problem.c), pR, pT, pW, ctypes.byref(gin), ctypes.byref(gout), flags,
                                            ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
    return ResidualGrad(**res)


class _ResidualDiff(torch.autograd.Function):
    """ba_residual with banet_ba_residual_grad_f32 as its backward; the level tensors enter as inputs so that autograd sees them"""

    @staticmethod
    def forward(ctx, problem, want_proj, R, T, Wc, src, tgt, depth, basis):
        r = ba_residual(problem, R, T, Wc, proj=True, sums=False)
        ctx.problem = problem
        ctx.shapes = [None if t is None else t.shape for t in (R, T, Wc, src, tgt, depth, basis)]
        ctx.save_for_backward(R, T, *([Wc] if Wc is not None else []))
        ctx.mark_non_differentiable(r.mask)
        ctx.set_materialize_grads(False)      # an output the loss does not use arrives as None = a NULL upstream gradient
        return r.sq, r.ab, r.mask, r.proj

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gsq, gab, _gmask, gproj):
        problem = ctx.problem
        saved = ctx.saved_tensors
        R, T, Wc = saved[0], saved[1], (saved[2] if len(saved) > 2 else None)
        need = ctx.needs_input_grad[2:]
        names = ("dR", "dT", "dWc", "dsrc", "dtgt", "ddepth", "dbasis")
        want = tuple(n for n, k in zip(names, need) if k)
        if not want or (gsq is None and gab is None and gproj is None):
            return (None,) * 9
        g = ba_residual_grad(problem, R, T, Wc, gsq, gab, gproj, want=want, overwrite=True)
        out = []
        for n, k, shape in zip(names, need, ctx.shapes):
            t = getattr(g, n) if k else None
            out.append(None if t is None else t.reshape(shape))
        return (None, None) + tuple(out)


def ba_residual_diff(problem, R, T, Wc=None, proj=False):
    """ba_residual attached to the autograd graph -> (sq, ab, mask, proj): sq, ab [B,pairs,N] and proj [B,pairs,N,2] (None unless
    proj=True) are differentiable with respect to R, T, Wc and the tensors the problem was built from (src, tgt, depth, basis);
    mask [B,pairs,N] uint8 is not.  The backward is one banet_ba_residual_grad_f32 call that asks only for the gradients some
    input needs.  A level whose target map is the [f|gx|gy] layout has no target-map gradient: BanetError if that map requires
    grad."""
    src, tgt, depth, basis = problem.keep[0], problem.keep[1], problem.keep[2], problem.keep[3]
    if tgt.requires_grad and int(problem.c.tgt_has_grad):
        raise capi.BanetError("ba_residual_diff: no gradient for a [f|gx|gy] target map (tgt_has_grad = 1); detach it or pass the C-channel map")
    R, T = capi.f32c(R), capi.f32c(T)
    Wc = capi.f32c(Wc) if (Wc is not None and problem.K > 0) else None
    sq, ab, mask, pr = _ResidualDiff.apply(problem, bool(proj), R, T, Wc, src, tgt, depth, basis)
    return sq, ab, mask, (pr if proj else None)


def ba_solve_update(level, mlp, l2_base, AtA, Atb, absres, nvalid, state, ws=None):
    """banet_ba_solve_update_f32: lambda, damping, solve, SE(3)/W update (in place on `state`).  Systems whose matrix does
    not fit the LDS (P > ~190) go through banet_ba_solve_update_ws_f32 with a workspace (`ws`, or one allocated here)."""
    L = capi.lib()
    if mlp is not None:
        mlp.check(level.C)
    nb = L.banet_ba_solve_update_workspace_bytes(ctypes.byref(level.c))
    if nb == 0:
        capi.check(L.banet_ba_solve_update_f32(ctypes.byref(level.c), ctypes.byref(mlp.c) if mlp is not None else None,
                                               float(l2_base), capi.ptr(AtA), capi.ptr(Atb), capi.ptr(absres),
                                               capi.ptr(nvalid), ctypes.byref(state.c), capi.stream()))
        return None
    if ws is None or ws.numel() < nb:
        ws = capi.workspace(nb, level.device)
    capi.check(L.banet_ba_solve_update_ws_f32(ctypes.byref(level.c), ctypes.byref(mlp.c) if mlp is not None else None,
                                              float(l2_base), capi.ptr(AtA), capi.ptr(Atb), capi.ptr(absres),
                                              capi.ptr(nvalid), ctypes.byref(state.c), ctypes.c_void_p(ws.data_ptr()),
                                              ws.numel(), capi.stream()))
    return ws


class Prior:
    """banet_prior_t plus the tensors it points at: what a level's solve additionally minimises, per window,
        scale (1/2 Wc^T Lambda Wc - eta^T Wc + 1/2 sum_n w_n (obs_n - depth_n - b_n . Wc)^2)
    Lambda [B,K,K] symmetric with eta [B,K] (None: 0) -- a Gaussian prior on the coefficients in information form, e.g.
    basis_fit(...).normal / .rhs -- and / or obs_depth [B,N] (any shape with B leading) with obs_weight like it (None: 1), summed
    over the points with a finite weight > 0 and a finite observation.  Each half may be None; a prior without tensors, or with
    scale = 0, is the empty prior (the solve without it, bit for bit).  eta needs Lambda and obs_weight needs obs_depth."""

    def __init__(self, Lambda=None, eta=None, obs_depth=None, obs_weight=None, scale=1.0):
        keep = [capi.f32c(x) if x is not None else None for x in (Lambda, eta, obs_depth, obs_weight)]
        self.Lambda, self.eta, self.obs_depth, self.obs_weight = keep
        self.scale = float(scale)
        self.c = capi.Prior()
        for name, t in zip(("Lambda", "eta", "obs_depth", "obs_weight"), keep):
            setattr(self.c, name, None if t is None else capi.ptr(t).value)   # (CPU tensors: BanetError)
        self.c.scale = self.scale

    def check(self, B, N, K):
        for name, t, n in (("Lambda", self.Lambda, B * K * K), ("eta", self.eta, B * K), ("obs_depth", self.obs_depth, B * N),
                           ("obs_weight", self.obs_weight, B * N)):
            if t is not None and t.numel() != n:
                raise capi.BanetError("Prior: %s holds %d values, the level (B = %d, N = %d, K = %d) needs %d" % (name, t.numel(), B, N, K, n))


def prior_workspace_bytes(level, prior):
    """banet_prior_workspace_bytes (0: the empty prior, or a level the term does not exist on)"""
    return capi.lib().banet_prior_workspace_bytes(ctypes.byref(level.c), ctypes.byref(prior.c) if prior is not None else None)


def prior_apply(level, prior, Wc, AtA, Atb, ws=None):
    """banet_prior_apply_f32: one iteration's step of a Prior between ba_assemble and ba_solve_update, IN PLACE on AtA [B,P,P] and
    Atb [B,P] at the coefficients Wc [B,K]: the depth block gets Le = fl(scale fl(G + Lambda)), Atb's depth rows
    fl(scale fl(g + eta)) - Le Wc.  level: a LevelProblem (B, N, K, pairs, variant, depth and basis are read).  The empty prior
    launches nothing.  -> the workspace used (None for the empty prior)."""
    L = capi.lib()
    lv = level.c
    if prior is not None:
        prior.check(int(lv.B), int(lv.N), int(lv.K))
    pw, pa, pb = capi.ptr(Wc), capi.ptr(AtA), capi.ptr(Atb)
    pc = ctypes.byref(prior.c) if prior is not None else None
    nb = int(L.banet_prior_workspace_bytes(ctypes.byref(lv), pc))
    if nb and (ws is None or ws.numel() < nb):
        ws = capi.workspace(nb, AtA.device)
    capi.check(L.banet_prior_apply_f32(ctypes.byref(lv), pc, pw, pa, pb, ctypes.c_void_p(ws.data_ptr()) if ws is not None else None,
                                       ws.numel() if ws is not None else 0, capi.stream()))
    return ws


def _prior_is_empty(prior):
    return prior is None or prior.scale == 0.0 or (prior.Lambda is None and prior.eta is None and prior.obs_depth is None and
                                                   prior.obs_weight is None)


def prior_terms(level, prior, ws=None):
    """banet_prior_terms_f32: the once-per-level part of a Prior on its own -> (Le [B,K,K], ee [B,K]), bit-equal to what prior_apply
    forms in its workspace: Prior(Lambda=Le, eta=ee, scale=1) applies the bits of `prior`.  The empty prior: (None, None)."""
    L = capi.lib()
    lv = level.c
    B, N, K = int(lv.B), int(lv.N), int(lv.K)
    if _prior_is_empty(prior):
        return None, None
    prior.check(B, N, K)
    nb = int(L.banet_prior_workspace_bytes(ctypes.byref(lv), ctypes.byref(prior.c)))
    if nb == 0:
        raise capi.BanetError("prior_terms: a `bundle` level with 1 <= K <= 256 is needed (and N >= 1 with observations)")
    dev = level.device
    if ws is None or ws.numel() < nb:
        ws = capi.workspace(nb, dev)
    Le = torch.empty((B, K, K), dtype=torch.float32, device=dev)
    ee = torch.empty((B, K), dtype=torch.float32, device=dev)
    capi.check(L.banet_prior_terms_f32(ctypes.byref(lv), ctypes.byref(prior.c), capi.ptr(Le), capi.ptr(ee), ctypes.c_void_p(ws.data_ptr()),
                                       ws.numel(), capi.stream()))
    return Le, ee


def prior_add_grad(level, Le, Wc, gAtA, gAtb, gLe=None, gee=None, gWc=None):
    """banet_prior_add_grad_f32: the backward of one iteration's prior_apply.  gAtA [B,P,P], gAtb [B,P]: the gradients with
    respect to the post-prior matrices (they pass through to the assembly unchanged); Le from prior_terms; Wc [B,K] that iteration's
    coefficients.  gLe [B,K,K] / gee [B,K]: None = written (the first call of a level), else accumulated into, in place;
    gWc [B,K]: None = zeros, and the call subtracts Le^T gAtb[m:] from it in place.  -> (gLe, gee, gWc)"""
    lv = level.c
    B, K = int(lv.B), int(lv.K)
    dev = gAtA.device
    if (gLe is None) != (gee is None):
        raise capi.BanetError("prior_add_grad: gLe and gee are given together")
    flags = capi.PRIOR_GRAD_OVERWRITE if gLe is None else 0
    if gLe is None:
        gLe = torch.empty((B, K, K), dtype=torch.float32, device=dev)
        gee = torch.empty((B, K), dtype=torch.float32, device=dev)
    if gWc is None:
        gWc = torch.zeros((B, K), dtype=torch.float32, device=dev)
    P = 6 * max(int(lv.pairs), 1) + K
    for name, t, n in (("Le", Le, B * K * K), ("Wc", Wc, B * K), ("gAtA", gAtA, B * P * P), ("gAtb", gAtb, B * P), ("gLe", gLe, B * K * K),
                       ("gee", gee, B * K), ("gWc", gWc, B * K)):
        if t.numel() != n:
            raise capi.BanetError("prior_add_grad: %s must hold %d floats" % (name, n))
    capi.check(capi.lib().banet_prior_add_grad_f32(ctypes.byref(lv), capi.ptr(Le), capi.ptr(Wc), capi.ptr(gAtA), capi.ptr(gAtb), capi.ptr(gLe),
                                                   capi.ptr(gee), capi.ptr(gWc), flags, capi.stream()))
    return gLe, gee, gWc


PRIOR_GRAD_OUTPUTS = ("gLambda", "geta", "gscale", "gobs", "gweight", "gdepth", "gbasis")
PriorGrad = collections.namedtuple("PriorGrad", PRIOR_GRAD_OUTPUTS)


def prior_terms_grad(level, prior, gLe, gee, Le=None, ee=None, want=PRIOR_GRAD_OUTPUTS, accumulate=False, into=None, ws=None):
    """banet_prior_terms_grad_f32: the once-per-level backward of a Prior, from the gLe / gee that prior_add_grad accumulated ->
    PriorGrad(gLambda [B,K,K], geta [B,K], gscale [B], gobs / gweight / gdepth [B,N], gbasis [B,N,K]); the outputs not named in
    `want` are None, and naming one whose input the prior lacks is refused.  gscale needs Le / ee (prior_terms).  accumulate:
    gdepth / gbasis are added into into["gdepth"] / into["gbasis"] (the dense adjoint's ddepth / dbasis; points that are not
    counted stay untouched); otherwise they are written, zeros at those points.  A window's bits depend neither on the batch nor
    on `want`."""
    L = capi.lib()
    lv = level.c
    B, N, K = int(lv.B), int(lv.N), int(lv.K)
    unknown = [w for w in want if w not in PRIOR_GRAD_OUTPUTS]
    if unknown:
        raise capi.BanetError("prior_terms_grad: unknown outputs %s" % unknown)
    if _prior_is_empty(prior):
        raise capi.BanetError("prior_terms_grad: the empty prior has no backward")
    prior.check(B, N, K)
    dev = gLe.device
    into = into or {}
    gin = capi.PriorGradIn()
    gin.gLe, gin.gee = capi.ptr(gLe).value, capi.ptr(gee).value
    gin.Le = None if Le is None else capi.ptr(Le).value
    gin.ee = None if ee is None else capi.ptr(ee).value
    gin.flags = capi.PRIOR_GRAD_ACCUMULATE if accumulate else 0
    shapes = dict(gLambda=(B, K, K), geta=(B, K), gscale=(B,), gobs=(B, N), gweight=(B, N), gdepth=(B, N), gbasis=(B, N, K))
    res, out = {}, capi.PriorGradOut()
    for name in PRIOR_GRAD_OUTPUTS:
        t = None
        if name in want:
            t = into.get(name)
            if t is None:
                if accumulate and name in ("gdepth", "gbasis"):
                    raise capi.BanetError("prior_terms_grad: accumulate=True adds into into[%r]" % name)
                t = torch.empty(shapes[name], dtype=torch.float32, device=dev)
            elif t.numel() != int(torch.Size(shapes[name]).numel()):
                raise capi.BanetError("prior_terms_grad: into[%r] must hold %s" % (name, shapes[name]))
        res[name] = t
        setattr(out, name, None if t is None else capi.ptr(t).value)
    nb = int(L.banet_prior_terms_grad_workspace_bytes(ctypes.byref(lv), ctypes.byref(prior.c)))
    if nb == 0:
        raise capi.BanetError("prior_terms_grad: a `bundle` level with 1 <= K <= 256 is needed (and N >= 1 with observations)")
    if ws is None or ws.numel() < nb:
        ws = capi.workspace(nb, dev)
    capi.check(L.banet_prior_terms_grad_f32(ctypes.byref(lv), ctypes.byref(prior.c), ctypes.byref(gin), ctypes.byref(out),
                                            ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
    return PriorGrad(**res)


def _prior_grad_want(prior, need):
    """need: needs-grad flags of (Lambda, eta, obs_depth, obs_weight, depth, basis) -> the outputs to ask for"""
    names = ("gLambda", "geta", "gobs", "gweight", "gdepth", "gbasis")
    has = (prior.Lambda is not None, prior.eta is not None, prior.obs_depth is not None, prior.obs_weight is not None,
           prior.obs_depth is not None, prior.obs_depth is not None)
    return tuple(n for n, k, h in zip(names, need, has) if k and h)


class _PriorApplyDiff(torch.autograd.Function):
    """prior_apply, out of place, with banet_prior_add_grad_f32 + banet_prior_terms_grad_f32 as its backward; the prior's and the
    level's tensors enter as inputs so that autograd sees them"""

    @staticmethod
    def forward(ctx, level, prior, Wc, AtA, Atb, Lambda, eta, obs, weight, depth, basis):
        Le, ee = prior_terms(level, prior)
        A2, b2 = AtA.clone(), Atb.clone()
        prior_apply(level, Prior(Lambda=Le, eta=ee, scale=1.0), Wc, A2, b2)     # fl(1 x) = x: the bits of `prior`
        ctx.level, ctx.prior = level, prior
        ctx.shapes = [None if t is None else t.shape for t in (Wc, Lambda, eta, obs, weight, depth, basis)]
        ctx.save_for_backward(Le, Wc)
        ctx.set_materialize_grads(False)
        return A2, b2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gA, gb):
        if gA is None and gb is None:
            return (None,) * 11
        level, prior = ctx.level, ctx.prior
        Le, Wc = ctx.saved_tensors
        B, K = level.B, level.K
        P = 6 * max(level.pairs, 1) + K
        dev = Le.device
        gA = torch.zeros(B, P, P, device=dev) if gA is None else capi.f32c(gA)
        gb = torch.zeros(B, P, device=dev) if gb is None else capi.f32c(gb)
        gLe, gee, gWc = prior_add_grad(level, Le, Wc, gA, gb)
        want = _prior_grad_want(prior, ctx.needs_input_grad[5:])
        g = prior_terms_grad(level, prior, gLe, gee, want=want) if want else PriorGrad(*([None] * len(PRIOR_GRAD_OUTPUTS)))
        sW, sL, se, so, sw, sd, sb = ctx.shapes
        rs = lambda t, s: None if (t is None or s is None) else t.reshape(s)           # noqa: E731
        return (None, None, rs(gWc, sW) if ctx.needs_input_grad[2] else None, gA if ctx.needs_input_grad[3] else None,
                gb if ctx.needs_input_grad[4] else None,
                rs(g.gLambda, sL), rs(g.geta, se), rs(g.gobs, so), rs(g.gweight, sw), rs(g.gdepth, sd), rs(g.gbasis, sb))


def prior_apply_diff(level, prior, Wc, AtA, Atb):
    """prior_apply attached to the autograd graph, OUT of place -> (AtA', Atb'): the inputs are not modified.  Differentiable with
    respect to AtA, Atb, Wc, the prior's Lambda / eta / obs_depth / obs_weight and the depth and basis the level was built from.
    The backward is one banet_prior_add_grad_f32 call and one banet_prior_terms_grad_f32 call that asks only for what some input
    needs.  Composes with dense_train.assemble_differentiable and ba_marginals_diff (marginals of the posterior with the prior as a
    loss).  The empty prior returns (AtA, Atb) themselves."""
    if _prior_is_empty(prior):
        return AtA, Atb
    depth, basis = level.keep[2], level.keep[3]
    return _PriorApplyDiff.apply(level, prior, capi.f32c(Wc), capi.f32c(AtA), capi.f32c(Atb), prior.Lambda, prior.eta, prior.obs_depth,
                                 prior.obs_weight, depth, basis)


class PosePrior:
    """banet_pose_prior_t plus the tensors it points at: what a level's solve additionally minimises, per window,
        scale 1/2 r^T Lambda r,   r = [Log(T_i o T0_i^-1)]_i in [phi; rho] ordering
    R0 [B,pairs,3,3] and T0 [B,pairs,3] (any shape with these element counts) the prior poses, Lambda [B,6 pairs,6 pairs] symmetric
    their joint information in the solve's left tangent (the inverse of ba_marginals' pose_cov).  All three or none; without
    tensors, or with scale = 0, it is the empty pose prior (the solve without it, bit for bit)."""

    def __init__(self, R0=None, T0=None, Lambda=None, scale=1.0):
        keep = [capi.f32c(x) if x is not None else None for x in (R0, T0, Lambda)]
        self.R0, self.T0, self.Lambda = keep
        self.scale = float(scale)
        self.c = capi.PosePrior()
        for name, t in zip(("R0", "T0", "Lambda"), keep):
            setattr(self.c, name, None if t is None else capi.ptr(t).value)   # (CPU tensors: BanetError)
        self.c.scale = self.scale

    def check(self, B, pairs):
        m = 6 * max(int(pairs), 1)
        for name, t, n in (("R0", self.R0, B * m // 6 * 9), ("T0", self.T0, B * m // 6 * 3), ("Lambda", self.Lambda, B * m * m)):
            if t is not None and t.numel() != n:
                raise capi.BanetError("PosePrior: %s holds %d values, the level (B = %d, pairs = %d) needs %d" % (name, t.numel(), B, pairs, n))


def _pose_prior_is_empty(pp):
    return pp is None or pp.scale == 0.0 or (pp.R0 is None and pp.T0 is None and pp.Lambda is None)


def pose_prior_apply(level, pose_prior, R, T, AtA, Atb):
    """banet_pose_prior_apply_f32: one iteration's step of a PosePrior between ba_assemble and ba_solve_update, IN PLACE on the pose
    block of AtA [B,P,P] and on Atb[:, :6 pairs] at the poses R [B,pairs,3,3], T [B,pairs,3]:  AtA += scale Jr^T Lambda Jr,
    Atb -= scale Jr^T Lambda r.  level: a LevelProblem (B, K, pairs and variant are read; `bundle` and `bundle_camera`).  No
    workspace; the empty pose prior launches nothing."""
    lv = level.c
    if pose_prior is not None:
        pose_prior.check(int(lv.B), int(lv.pairs))
    capi.check(capi.lib().banet_pose_prior_apply_f32(ctypes.byref(lv), ctypes.byref(pose_prior.c) if pose_prior is not None else None,
                                                     capi.ptr(R), capi.ptr(T), capi.ptr(AtA), capi.ptr(Atb), capi.stream()))


POSE_PRIOR_GRAD_OUTPUTS = ("gR", "gT", "gR0", "gT0", "gLambda", "gscale")
PosePriorGrad = collections.namedtuple("PosePriorGrad", POSE_PRIOR_GRAD_OUTPUTS)


def pose_prior_add_grad(level, pose_prior, R, T, gAtA, gAtb, want=POSE_PRIOR_GRAD_OUTPUTS, into=None, overwrite=None):
    """banet_pose_prior_add_grad_f32: the backward of one iteration's pose_prior_apply at the poses R [B,pairs,3,3], T [B,pairs,3].
    gAtA [B,P,P], gAtb [B,P]: the gradients with respect to the post-prior matrices (they pass through to the assembly unchanged
    and are not written) -> PosePriorGrad(gR [B,pairs,3,3], gT [B,pairs,3], gR0, gT0, gLambda [B,m,m], gscale [B]); the outputs not
    named in `want` are None and are not computed.  into: {name: tensor} to write or accumulate into, in place; an output without
    one is allocated and written.  overwrite: {"state": bool, "prior": bool} -- whether gR / gT and gR0 / gT0 / gLambda / gscale are
    written or accumulated into (read-modify-write); default: written exactly where no output of the group comes from `into`.  An
    output allocated here inside an accumulating group starts from zero.  A window's bits depend neither on the batch nor on `want`."""
    lv = level.c
    B, K, pairs = int(lv.B), int(lv.K), max(int(lv.pairs), 1)
    m = 6 * pairs
    P = m + K
    unknown = [w for w in want if w not in POSE_PRIOR_GRAD_OUTPUTS]
    if unknown:
        raise capi.BanetError("pose_prior_add_grad: unknown outputs %s" % unknown)
    if _pose_prior_is_empty(pose_prior):
        raise capi.BanetError("pose_prior_add_grad: the empty pose prior has no backward")
    pose_prior.check(B, int(lv.pairs))
    for name, t, n in (("R", R, B * pairs * 9), ("T", T, B * pairs * 3), ("gAtA", gAtA, B * P * P), ("gAtb", gAtb, B * P)):
        if t.numel() != n:
            raise capi.BanetError("pose_prior_add_grad: %s must hold %d floats" % (name, n))
    into = into or {}
    groups = dict(gR="state", gT="state", gR0="prior", gT0="prior", gLambda="prior", gscale="prior")
    ow = dict(state=not any(groups[n] == "state" and into.get(n) is not None for n in want),
              prior=not any(groups[n] == "prior" and into.get(n) is not None for n in want))
    ow.update(overwrite or {})
    shapes = dict(gR=(B, pairs, 3, 3), gT=(B, pairs, 3), gR0=(B, pairs, 3, 3), gT0=(B, pairs, 3), gLambda=(B, m, m), gscale=(B,))
    dev = gAtA.device
    res, out = {}, capi.PosePriorGrad()
    for name in POSE_PRIOR_GRAD_OUTPUTS:
        t = None
        if name in want:
            t = into.get(name)
            if t is None:
                t = (torch.empty if ow[groups[name]] else torch.zeros)(shapes[name], dtype=torch.float32, device=dev)
            elif t.numel() != int(torch.Size(shapes[name]).numel()):
                raise capi.BanetError("pose_prior_add_grad: into[%r] must hold %s" % (name, shapes[name]))
        res[name] = t
        setattr(out, name, None if t is None else capi.ptr(t).value)
    out.flags = (capi.POSE_PRIOR_GRAD_OVERWRITE_STATE if ow["state"] else 0) | (capi.POSE_PRIOR_GRAD_OVERWRITE_PRIOR if ow["prior"] else 0)
    capi.check(capi.lib().banet_pose_prior_add_grad_f32(ctypes.byref(lv), ctypes.byref(pose_prior.c), capi.ptr(R), capi.ptr(T), capi.ptr(gAtA),
                                                        capi.ptr(gAtb), ctypes.byref(out), capi.stream()))
    return PosePriorGrad(**res)


class _PosePriorApplyDiff(torch.autograd.Function):
    """pose_prior_apply, out of place, with banet_pose_prior_add_grad_f32 as its backward; the prior's tensors enter as inputs so
    that autograd sees them"""

    @staticmethod
    def forward(ctx, level, pose_prior, R, T, AtA, Atb, R0, T0, Lambda):
        A2, b2 = AtA.clone(), Atb.clone()
        pose_prior_apply(level, pose_prior, R, T, A2, b2)
        ctx.level, ctx.pose_prior = level, pose_prior
        ctx.shapes = [t.shape for t in (R, T, R0, T0, Lambda)]
        ctx.save_for_backward(R, T)
        ctx.set_materialize_grads(False)
        return A2, b2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gA, gb):
        if gA is None and gb is None:
            return (None,) * 9
        level = ctx.level
        R, T = ctx.saved_tensors
        B, K = level.B, level.K
        P = 6 * max(level.pairs, 1) + K
        dev = R.device
        gA = torch.zeros(B, P, P, device=dev) if gA is None else capi.f32c(gA)
        gb = torch.zeros(B, P, device=dev) if gb is None else capi.f32c(gb)
        need = ctx.needs_input_grad
        want = tuple(n for n, k in zip(("gR", "gT", "gR0", "gT0", "gLambda"), need[2:4] + need[6:9]) if k)
        g = pose_prior_add_grad(level, ctx.pose_prior, R, T, gA, gb, want=want) if want else PosePriorGrad(*([None] * 6))
        sR, sT, sR0, sT0, sL = ctx.shapes
        rs = lambda t, s: None if t is None else t.reshape(s)           # noqa: E731
        return (None, None, rs(g.gR, sR), rs(g.gT, sT), gA if need[4] else None, gb if need[5] else None, rs(g.gR0, sR0), rs(g.gT0, sT0),
                rs(g.gLambda, sL))


def pose_prior_apply_diff(level, pose_prior, R, T, AtA, Atb):
    """pose_prior_apply attached to the autograd graph, OUT of place -> (AtA', Atb'): the inputs are not modified.  Differentiable
    with respect to AtA, Atb, R, T and the prior's R0, T0 and Lambda (R and R0 as nine free entries each); `scale` stays a float
    here (its gradient exists at the wrapper level: pose_prior_add_grad's gscale).  The backward is one
    banet_pose_prior_add_grad_f32 call that asks only for what some input needs.  Composes with
    dense_train.assemble_differentiable and ba_marginals_diff.  The empty pose prior returns (AtA, Atb) themselves."""
    if _pose_prior_is_empty(pose_prior):
        return AtA, Atb
    pose_prior.check(level.B, level.pairs)
    return _PosePriorApplyDiff.apply(level, pose_prior, capi.f32c(R), capi.f32c(T), capi.f32c(AtA), capi.f32c(Atb), pose_prior.R0,
                                     pose_prior.T0, pose_prior.Lambda)


def lm_level(level, mlp, l2_base, max_iters, early_termination, state, ws=None, params=None, prior=None, pose_prior=None):
    """banet_lm_level_ex_f32: the whole LM loop of one pyramid level, enqueued without host sync.
    params: an `lm_params(...)` value (None = the reference's defaults, legacy/ba.py:5-9).
    prior: a `Prior` (banet_lm_level_prior_f32: its term is added between assembly and solve of every iteration; `bundle` levels,
    no early termination); None = the call path without one.
    pose_prior: a `PosePrior` (banet_lm_level_pose_prior_f32, with `prior` or without; `bundle` and `bundle_camera` levels, no early
    termination); None = the call path without one."""
    L = capi.lib()
    if mlp is not None:
        mlp.check(level.C)
    if pose_prior is not None:
        if early_termination:
            raise capi.BanetError("lm_level: a pose prior excludes early termination")
        pose_prior.check(level.B, level.pairs)
        if prior is not None:
            prior.check(level.B, level.N, level.K)
        pc = ctypes.byref(prior.c) if prior is not None else None
        nb = L.banet_lm_level_pose_prior_workspace_bytes(ctypes.byref(level.c), pc, ctypes.byref(pose_prior.c))
        if nb == 0:
            raise capi.BanetError("lm_level: unsupported level shape, a prior on a level without a depth basis, or a pose prior on a "
                                  "legacy variant / with only some of R0, T0, Lambda")
        if ws is None or ws.numel() < nb:
            ws = capi.workspace(nb, level.device)
        capi.check(L.banet_lm_level_pose_prior_f32(ctypes.byref(level.c), ctypes.byref(mlp.c) if mlp is not None else None, float(l2_base),
                                                   int(max_iters), ctypes.byref(params) if params is not None else None, pc,
                                                   ctypes.byref(pose_prior.c), ctypes.byref(state.c), ctypes.c_void_p(ws.data_ptr()),
                                                   ws.numel(), capi.stream()))
        return ws
    if prior is not None:
        if early_termination:
            raise capi.BanetError("lm_level: a prior excludes early termination")
        prior.check(level.B, level.N, level.K)
        nb = L.banet_lm_level_prior_workspace_bytes(ctypes.byref(level.c), ctypes.byref(prior.c))
        if nb == 0:
            raise capi.BanetError("lm_level: unsupported level shape, or a prior on a level without a depth basis")
        if ws is None or ws.numel() < nb:
            ws = capi.workspace(nb, level.device)
        capi.check(L.banet_lm_level_prior_f32(ctypes.byref(level.c), ctypes.byref(mlp.c) if mlp is not None else None, float(l2_base),
                                              int(max_iters), ctypes.byref(params) if params is not None else None, ctypes.byref(prior.c),
                                              ctypes.byref(state.c), ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
        return ws
    nb = L.banet_lm_level_workspace_bytes(ctypes.byref(level.c))
    if nb == 0:
        raise capi.BanetError("lm_level: unsupported level shape")
    if ws is None or ws.numel() < nb:
        ws = capi.workspace(nb, level.device)
    capi.check(L.banet_lm_level_ex_f32(ctypes.byref(level.c), ctypes.byref(mlp.c) if mlp is not None else None,
                                       float(l2_base), int(max_iters), int(bool(early_termination)),
                                       ctypes.byref(params) if params is not None else None,
                                       ctypes.byref(state.c), ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
    return ws


def lm_level_workspace_bytes(level, prior=None, pose_prior=None):
    if pose_prior is not None:
        return capi.lib().banet_lm_level_pose_prior_workspace_bytes(ctypes.byref(level.c), ctypes.byref(prior.c) if prior is not None else None,
                                                                    ctypes.byref(pose_prior.c))
    if prior is not None:
        return capi.lib().banet_lm_level_prior_workspace_bytes(ctypes.byref(level.c), ctypes.byref(prior.c))
    return capi.lib().banet_lm_level_workspace_bytes(ctypes.byref(level.c))


class SolveTrace:
    """banet_solve_trace_t plus the tensors it points at: the state after every level of one banet_lm_solve_f32 call, row l =
    level l.  fields: which of R / T / Wc / lambda_out / delta / ratio / iters to record (default all; Wc only when the state has
    one); depth: a list of n_levels tensors [B,N_l] (or None entries) that receive depth_l + basis_l . Wc after level l
    (bundlenet.py:397; `bundle` only).  Attributes of fields that are not recorded are None."""
    FIELDS = ("R", "T", "Wc", "lambda_out", "delta", "ratio", "iters")

    def __init__(self, n_levels, state, fields=None, depth=None):
        self.n_levels = int(n_levels)
        self.c = capi.SolveTrace()
        for name in self.FIELDS:
            src = getattr(state, name)
            t = None
            if src is not None and (fields is None or name in fields):
                t = torch.empty((self.n_levels,) + tuple(src.shape), dtype=src.dtype, device=src.device)
                setattr(self.c, name, t.data_ptr())
            setattr(self, name, t)
        self.depth = None
        if depth is not None:
            if len(depth) != self.n_levels:
                raise capi.BanetError("SolveTrace: %d depth outputs for %d levels" % (len(depth), self.n_levels))
            self.depth = list(depth)
            self._depth_ptrs = (capi._FP * self.n_levels)(*[None if t is None else capi.ptr(t).value for t in self.depth])
            self.c.depth = ctypes.cast(self._depth_ptrs, ctypes.POINTER(capi._FP))


def _schedule(levels, mlps, l2_base, iters, early_termination, params, trace):
    """-> (banet_schedule_t without a workspace, the ctypes arrays it points at)"""
    n = len(levels)
    if n == 0 or len(mlps) != n or len(iters) != n:
        raise capi.BanetError("lm_solve: %d levels, %d lambda MLPs, %d iteration counts" % (n, len(mlps), len(iters)))
    if trace is not None and trace.n_levels != n:
        raise capi.BanetError("lm_solve: the trace has %d rows for %d levels" % (trace.n_levels, n))
    lv = (capi.Level * n)(*[p.c for p in levels])         # (copies: later changes of a level's flags need a new call)
    mp = (ctypes.POINTER(capi.Mlp) * n)()
    for i, m in enumerate(mlps):
        if m is not None:
            m.check(levels[i].C)
            mp[i] = ctypes.pointer(m.c)
    it = (ctypes.c_int32 * n)(*[int(v) for v in iters])
    s = capi.Schedule()
    s.levels, s.n_levels = ctypes.cast(lv, ctypes.POINTER(capi.Level)), n
    s.mlps = ctypes.cast(mp, ctypes.POINTER(ctypes.POINTER(capi.Mlp)))
    s.max_iters = ctypes.cast(it, ctypes.POINTER(ctypes.c_int32))
    s.l2_base, s.early_termination = float(l2_base), int(bool(early_termination))
    if params is not None:
        s.params = ctypes.pointer(params)
    if trace is not None:
        s.trace = ctypes.pointer(trace.c)
    return s, (lv, mp, it, params, trace)


def lm_solve_workspace_bytes(levels):
    """banet_lm_solve_workspace_bytes: the maximum of the levels' needs (0: a level is unsupported or the levels disagree)"""
    n = len(levels)
    s = capi.Schedule()
    lv = (capi.Level * max(n, 1))(*[p.c for p in levels])
    s.levels, s.n_levels = ctypes.cast(lv, ctypes.POINTER(capi.Level)), n
    return capi.lib().banet_lm_solve_workspace_bytes(ctypes.byref(s))


def lm_solve(levels, mlps, l2_base, iters, early_termination, state, ws=None, params=None, trace=None, priors=None, pose_priors=None):
    """banet_lm_solve_f32: every level of a coarse -> fine schedule in ONE call -- the sequence of lm_level calls, bit for bit,
    with the state after each level recorded in `trace` (a SolveTrace, or None).  levels / mlps / iters: one LevelProblem,
    MlpWeights (or None) and iteration count per level.  All levels are validated before anything is enqueued.
    priors: one `Prior` or None per level (banet_lm_solve_prior_f32; no early termination); None = the call path without.
    pose_priors: one `PosePrior` or None per level (banet_lm_solve_pose_prior_f32, with `priors` or without; no early termination);
    None = the call path without."""
    L = capi.lib()
    s, keep = _schedule(levels, mlps, l2_base, iters, early_termination, params, trace)
    if pose_priors is not None:
        n = len(levels)
        if len(pose_priors) != n or (priors is not None and len(priors) != n):
            raise capi.BanetError("lm_solve: %d pose priors and %s priors for %d levels" % (len(pose_priors), "no" if priors is None else len(priors), n))
        if early_termination:
            raise capi.BanetError("lm_solve: pose priors exclude early termination")
        pp = (capi.PosePrior * n)()                        # (a zeroed entry is the empty pose prior)
        pr = (capi.Prior * n)() if priors is not None else None
        for i in range(n):
            if pose_priors[i] is not None:
                pose_priors[i].check(levels[i].B, levels[i].pairs)
                pp[i] = pose_priors[i].c
            if priors is not None and priors[i] is not None:
                priors[i].check(levels[i].B, levels[i].N, levels[i].K)
                pr[i] = priors[i].c
        nb = L.banet_lm_solve_pose_prior_workspace_bytes(ctypes.byref(s), pr, pp)
        if nb == 0:
            raise capi.BanetError("lm_solve: unsupported level shape, levels that disagree in B / K / pairs / variant / policy, a prior on "
                                  "a level without a depth basis, or a pose prior on a legacy variant / with only some of R0, T0, Lambda")
        if ws is None or ws.numel() < nb:
            ws = capi.workspace(nb, levels[0].device)
        s.workspace, s.workspace_bytes = ws.data_ptr(), ws.numel()
        capi.check(L.banet_lm_solve_pose_prior_f32(ctypes.byref(s), pr, pp, ctypes.byref(state.c), capi.stream()))
        del keep
        return ws
    if priors is not None:
        n = len(levels)
        if len(priors) != n:
            raise capi.BanetError("lm_solve: %d priors for %d levels" % (len(priors), n))
        if early_termination:
            raise capi.BanetError("lm_solve: priors exclude early termination")
        pr = (capi.Prior * n)()                            # (a zeroed entry is the empty prior)
        for i, p in enumerate(priors):
            if p is not None:
                p.check(levels[i].B, levels[i].N, levels[i].K)
                pr[i] = p.c
        nb = L.banet_lm_solve_prior_workspace_bytes(ctypes.byref(s), pr)
        if nb == 0:
            raise capi.BanetError("lm_solve: unsupported level shape, levels that disagree in B / K / pairs / variant / policy, or a "
                                  "prior on a level without a depth basis")
        if ws is None or ws.numel() < nb:
            ws = capi.workspace(nb, levels[0].device)
        s.workspace, s.workspace_bytes = ws.data_ptr(), ws.numel()
        capi.check(L.banet_lm_solve_prior_f32(ctypes.byref(s), pr, ctypes.byref(state.c), capi.stream()))
        del keep
        return ws
    nb = L.banet_lm_solve_workspace_bytes(ctypes.byref(s))
    if nb == 0:
        raise capi.BanetError("lm_solve: unsupported level shape, or levels that disagree in B / K / pairs / variant / policy")
    if ws is None or ws.numel() < nb:
        ws = capi.workspace(nb, levels[0].device)
    s.workspace, s.workspace_bytes = ws.data_ptr(), ws.numel()
    capi.check(L.banet_lm_solve_f32(ctypes.byref(s), ctypes.byref(state.c), capi.stream()))
    del keep
    return ws


def profile_begin(max_launches):
    capi.check(capi.lib().banet_profile_begin(int(max_launches)))


def profile_end(max_tags=16):
    """-> {points_per_window: (launches, total_ms)} for the assembly kernel since profile_begin"""
    pts = (ctypes.c_int32 * max_tags)()
    cnt = (ctypes.c_int32 * max_tags)()
    ms = (ctypes.c_double * max_tags)()
    nt = ctypes.c_int32(0)
    capi.check(capi.lib().banet_profile_end(max_tags, pts, cnt, ms, ctypes.byref(nt)))
    return {int(pts[i]): (int(cnt[i]), float(ms[i])) for i in range(nt.value)}


# --------------------------------------------------------------------------------------
# per-level preparation (banet_resample_f32 / banet_target_map_f32 / banet_depth_output_f32)
# --------------------------------------------------------------------------------------
def resample(data, warp, clamp=False):
    """data [B,H,W,C], warp [B,N,2] -> [B,N,C].  clamp=False: tf.contrib.resampler.resampler
    (bundlenet.py:290,320,343-344,385); clamp=True: interpolate2d2 (legacy/utils_python.py:177-232)."""
    data, warp = capi.f32c(data), capi.f32c(warp)
    B, H, W, C = data.shape
    N = warp.shape[1]
    if tuple(warp.shape) != (B, N, 2):
        raise capi.BanetError("resample: expected data [B,H,W,C] and warp [B,N,2]; got %s %s" % (tuple(data.shape), tuple(warp.shape)))
    out = torch.empty((B, N, C), dtype=torch.float32, device=data.device)
    capi.check(capi.lib().banet_resample_f32(capi.ptr(data), capi.ptr(warp), capi.ptr(out), B, N, C, H, W,
                                             1 if clamp else 0, capi.stream()))
    return out


def target_map(img):
    """[B,H,W,C] -> [B,H,W,3C] = [f | gx | gy] (grad_fixed + concat: bundlenet.py:92-100,323-324; legacy/ba.py:116-118)."""
    img = capi.f32c(img)
    B, H, W, C = img.shape
    out = torch.empty((B, H, W, 3 * C), dtype=torch.float32, device=img.device)
    capi.check(capi.lib().banet_target_map_f32(capi.ptr(img), capi.ptr(out), B, H, W, C, capi.stream()))
    return out


def depth_output(init_depth, basis, Wc):
    """init_depth [B,...] + basis [B,N,K] . Wc [B,K,1] -> same shape as init_depth (bundlenet.py:397)."""
    init, basis, Wc = capi.f32c(init_depth), capi.f32c(basis), capi.f32c(Wc)
    B, K = basis.shape[0], basis.shape[-1]
    N = basis.numel() // (B * K)
    if init.numel() != B * N or Wc.numel() != B * K:
        raise capi.BanetError("depth_output: inconsistent shapes")
    out = torch.empty_like(init)
    capi.check(capi.lib().banet_depth_output_f32(capi.ptr(init), capi.ptr(basis), capi.ptr(Wc), capi.ptr(out), B, N, K,
                                                 capi.stream()))
    return out


# --------------------------------------------------------------------------------------
# differentiable layer support: per-pixel sampling statistics (sstats.hip)
# --------------------------------------------------------------------------------------
def sample_stats_forward(conv1, conv2, px, py):
    """banet_sample_stats_f32 -> (stats [B,N,8] = (M11, M12, M22, g1, g2, mask, 0, 0), absd [B,C] = sum_n |d|)."""
    conv1, conv2, px, py = capi.f32c(conv1), capi.f32c(conv2), capi.f32c(px), capi.f32c(py)
    B, N, C = conv1.shape
    H, W = conv2.shape[1], conv2.shape[2]
    if conv2.shape[0] != B or conv2.shape[3] != 3 * C or tuple(px.shape) != (B, N) or tuple(py.shape) != (B, N):
        raise capi.BanetError("sample_stats: expected conv1 [B,N,C], conv2 [B,H,W,3C], px / py [B,N]")
    L = capi.lib()
    G = L.banet_sample_stats_blocks(N)
    stats = torch.empty((B, N, 8), dtype=torch.float32, device=conv1.device)
    part = torch.empty((B, G, C), dtype=torch.float32, device=conv1.device)
    capi.check(L.banet_sample_stats_f32(capi.ptr(conv1), capi.ptr(conv2), capi.ptr(px), capi.ptr(py), B, N, C, H, W,
                                        capi.ptr(stats), capi.ptr(part), capi.stream()))
    return stats, part.sum(dim=1)


DETERMINISTIC_GRADIENTS = True   # sample_stats backward: fixed-order per-texel gather (True) or float-atomic scatter (False)


def sample_stats_grad(conv1, conv2, px, py, dstats, dabs, deterministic=None):
    """banet_sample_stats_grad_det_f32 (default: bit-reproducible) / banet_sample_stats_grad_f32 (float-atomic scatter)
    -> (dconv1 [B,N,C], dconv2 [B,H,W,3C], dpos [B,N,2])."""
    conv1, conv2, px, py = capi.f32c(conv1), capi.f32c(conv2), capi.f32c(px), capi.f32c(py)
    dstats, dabs = capi.f32c(dstats), capi.f32c(dabs)
    B, N, C = conv1.shape
    H, W = conv2.shape[1], conv2.shape[2]
    dconv1 = torch.empty_like(conv1)
    dconv2 = torch.zeros_like(conv2)
    dpos = torch.empty((B, N, 2), dtype=torch.float32, device=conv1.device)
    if DETERMINISTIC_GRADIENTS if deterministic is None else deterministic:
        L = capi.lib()
        nb = L.banet_sample_stats_grad_workspace_bytes(B, N, C, H, W)
        if nb == 0:
            raise capi.BanetError("sample_stats_grad: unsupported shape")
        ws = capi.workspace(nb, conv1.device)
        capi.check(L.banet_sample_stats_grad_det_f32(capi.ptr(conv1), capi.ptr(conv2), capi.ptr(px), capi.ptr(py), B, N, C, H, W,
                                                     capi.ptr(dstats), capi.ptr(dabs), capi.ptr(dconv1), capi.ptr(dconv2),
                                                     capi.ptr(dpos), ctypes.c_void_p(ws.data_ptr()), ws.numel(), capi.stream()))
        return dconv1, dconv2, dpos
    capi.check(capi.lib().banet_sample_stats_grad_f32(capi.ptr(conv1), capi.ptr(conv2), capi.ptr(px), capi.ptr(py), B, N, C, H, W,
                                                      capi.ptr(dstats), capi.ptr(dabs), capi.ptr(dconv1), capi.ptr(dconv2),
                                                      capi.ptr(dpos), capi.stream()))
    return dconv1, dconv2, dpos


class _SampleStats(torch.autograd.Function):
    @staticmethod
    def forward(ctx, conv1, conv2, px, py):
        ctx.save_for_backward(conv1, conv2, px, py)
        stats, absd = sample_stats_forward(conv1, conv2, px, py)
        ctx.mark_non_differentiable(stats[..., 5:])
        return stats[..., :5], stats[..., 5], absd

    @staticmethod
    def backward(ctx, dstats5, _dmask, dabs):
        conv1, conv2, px, py = ctx.saved_tensors
        B, N, _ = conv1.shape
        dstats = torch.zeros((B, N, 8), dtype=torch.float32, device=conv1.device)
        dstats[..., :5] = dstats5
        dconv1, dconv2, dpos = sample_stats_grad(conv1, conv2, px, py, dstats, dabs.contiguous())
        return dconv1, dconv2, dpos[..., 0], dpos[..., 1]


def sample_stats(conv1, conv2, px, py):
    """Differentiable (M, g, mask, sum |d|) of bundlenet.py:230-243 without materialising samp / diff / grad:
    returns (stats [B,N,5] = (M11, M12, M22, g1, g2), mask [B,N], absd [B,C])."""
    return _SampleStats.apply(conv1, conv2, px, py)
