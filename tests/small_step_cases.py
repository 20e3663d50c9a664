"""Inputs for the tests of the backward's small step (csrc/smallstep.hip): one generator shared by the CPU module
(test_small_step_cases_cpu.py: the conditions on the inputs, the float32 yardstick, the support limits) and the GPU module
(test_gpu_small_step.py).  No GPU, torch + the oracle's synth only.

A case is one batch of B windows of the `bundle` / `bundle_camera` small step (bundlenet.py:165-190, 241-276 after the
EquationConstruction op): AtA = J^T J of a random Jacobian J [B, N, P], P = 6 pairs + K, rounded to float32.  A RUNG sets how
badly conditioned the damped system is: `dl` makes the LAST column of J (the undamped depth coefficient of the bundle variant)
the first depth column plus dl x noise, `l2_base` scales the damping of all the others."""
import numpy as np
import torch

from oracle import synth

N_POINTS = 4000
SEEDS = (0, 1, 2, 3, 4)

# (dl, l2_base): the ladder, best conditioned first
RUNGS = ((None, 1000.0), (None, 1.0), (0.1, 1e-3), (1e-2, 1e-3), (1e-3, 1e-3), (1e-3, 1e-5))

# condition number of the damped matrix, per rung.  Where it comes from: J has N = 4000 standard normal rows, so J^T J has its
# eigenvalues within N (1 +- sqrt(P / N))^2 (0.6 N .. 1.5 N at P = 183) and every diagonal entry is ~N.
#   rungs 0, 1 (dl none): A = J^T J + lambda diag(J^T J) on all coefficients but the last.  lambda = l2_base ||avg||^(2 + y)
#     with ||avg|| ~ 0.12 sqrt(C) and -1 < y < 1: 1e-3 l2_base .. 10 l2_base over C = 1 .. 256.  The damped block is
#     ~N (1 + lambda), the last coefficient stays at ~N: cond ~ 1 + lambda up to the spread of J^T J (2.5).
#   rungs 2 .. 5 (C = 32: lambda ~ 0.3 l2_base): the damping no longer separates the scales; the difference of the first depth
#     column and the last one has length^2 ~N dl^2, and the damping of the FIRST depth column (half of that direction) adds
#     ~N lambda / 2 to it, against ~2 N at the top (the sum of the two columns): smallest eigenvalue ~N (dl^2 + lambda / 2) / 2,
#     cond ~ 4 / (dl^2 + lambda / 2): 4e2, 1.6e4, 2.7e4, 2.7e6 before the spread of J^T J.  One decade each; rungs 3 and 4
#     are both held up by the damping (dl^2 = 1e-4 and 1e-6 against lambda / 2 ~ 1.5e-4) and differ by a factor below 2.
COND_BANDS = ((1.0, 1e5), (1.0, 40.0), (1e2, 1e3), (3e3, 3e4), (5e3, 5e4), (0.5e6, 0.5e7))
# the band of rung 0 at the ladder's C = 32 (lambda ~ 1e2 .. 1e3), one decade as for the other rungs
COND_BAND_RUNG0_C32 = (1e2, 1e3)

MAX_K = "max"      # K = the largest one banet_small_step_adjoint_workspace_bytes accepts (found by a scan, never a literal)

# ---- what the GPU module runs: (variant, B, C, K, pairs), each on rungs 0 and 1 ...
SHAPE_GROUPS = (
    # P < 32 (the factorisation inside small_post_kernel): bundle, pairs = 1 -- P = 7, 8, 14, 25, 31
    [("bundle", 3, 32, K, 1) for K in (1, 2, 8, 19, 25)] +
    # ... bundle windows -- P = 19, 31, 19
    [("bundle", 3, 32, K, pairs) for pairs, K in ((2, 7), (4, 7), (3, 1))] +
    # ... camera -- P = 6, 12, 18, 30
    [("bundle_camera", 3, 32, 0, pairs) for pairs in (1, 2, 3, 5)] +
    # the switch to spd_solve_kernel: P = 32, 33
    [("bundle", 3, 32, K, 1) for K in (26, 27)] +
    # camera windows on the LDS solve, every diagonal damped: P = 36, 48
    [("bundle_camera", 3, 32, 0, pairs) for pairs in (6, 8)] +
    # the largest supported P
    [("bundle", 3, 32, MAX_K, pairs) for pairs in (1, 7)] +
    # the MLP's code paths by channel count, at P = 14 and P = 39
    [("bundle", 3, C, K, 1) for C in (1, 3, 5, 63, 255, 256) for K in (8, 33)] +
    # the sum over the windows in small_wgrad_kernel
    [("bundle", B, 32, K, 1) for B in (1, 37, 64) for K in (8, 33)]
)
SHAPE_RUNGS = (0, 1)
# ... and the whole ladder on these: P = 14, 31 (in-kernel factorisation), 32, 39, 134 (LDS solve), P = 30 as a 3-target window
LADDER_GROUPS = [("bundle", 3, 32, K, 1) for K in (8, 25, 26, 33, 128)] + [("bundle", 3, 32, 12, 3)]
LADDER_RUNGS = (0, 1, 2, 3, 4, 5)


def all_groups():
    """every (group, rung) of the GPU module, once each (the ladder repeats rungs 0, 1 of some shapes)"""
    out = []
    for grp in SHAPE_GROUPS:
        for r in SHAPE_RUNGS:
            out.append((grp, r))
    for grp in LADDER_GROUPS:
        for r in LADDER_RUNGS:
            if (grp, r) not in out:
                out.append((grp, r))
    return out


def group_id(grp, rung):
    variant, B, C, K, pairs = grp
    return "%s-B%d-C%d-K%s-pairs%d-rung%d" % ("cam" if variant == "bundle_camera" else "bundle", B, C, K, pairs, rung)


def cond_band(grp, rung):
    if rung == 0 and grp[0] == "bundle" and grp[2] == 32:
        return COND_BAND_RUNG0_C32
    return COND_BANDS[rung]


def _r32(x):
    return x.to(torch.float32).to(torch.float64)


def lambda_of(absres, layers, N, pairs, l2_base, camera):
    """lambda [B] as bundlenet.py:243-253 states it, in the dtype of the inputs"""
    avg = (absres / float(N * pairs)).unsqueeze(1)
    h = avg
    for i, (w, b) in enumerate(layers):
        z = torch.matmul(h, w) + b
        h = torch.tanh(z) if i == 4 else torch.nn.functional.selu(z)
    lam = torch.linalg.vector_norm(avg, dim=-1, keepdim=True) ** (2.0 + h)
    return (lam if camera else l2_base * lam).reshape(-1)


def damped_matrix(AtA, lam, camera):
    """bundlenet.py:181-182 (camera: every coefficient) / :264-266 (bundle: all but the last)"""
    diag = torch.diagonal(AtA, dim1=1, dim2=2)
    damp = diag + 1e-5
    if not camera:
        damp = torch.cat([damp[:, :-1], torch.zeros_like(damp[:, :1])], dim=-1)
    return AtA + torch.diag_embed(damp * lam.unsqueeze(-1))


def make_case(variant, B, C, K, pairs, rung, seed, N=N_POINTS):
    """-> dict of float64 tensors whose values are float32 numbers (so that a float32 and a float64 evaluation start from the
    same inputs): AtA [B,P,P], Atb [B,P], absres [B,C], R [B,pairs,3,3], T [B,pairs,3,1], Wc [B,K,1], gR, gT, gW (the upstream
    gradients), layers (five (filters [Cin,Cout], biases [Cout])), l2_base; plus, in float64, the damped matrix `A` [B,P,P] and
    the solution `delta` [B,P] of A delta = Atb."""
    from banet_amd.bundlenet import he_normal_lambda_weights
    camera = variant == "bundle_camera"
    assert (K == 0) == camera
    dl, l2_base = RUNGS[rung]
    P = 6 * pairs + K
    g = torch.Generator().manual_seed(seed + 7 * (rung + 11 * (K + 307 * (pairs + 13 * (C + 311 * B)))))
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    J = rnd(B, N, P)
    if dl is not None and not camera:
        J[..., -1] = J[..., 6 * pairs] + dl * rnd(B, N)
    AtA = _r32(J.transpose(1, 2) @ J)
    AtA = _r32(0.5 * (AtA + AtA.transpose(1, 2)))
    Atb = _r32(rnd(B, P) * 2.0)
    absres = _r32((torch.rand(B, C, generator=g, dtype=torch.float64) * 0.2 + 0.01) * N * pairs)
    rs = np.random.RandomState(1000 * seed + P)
    R = _r32(torch.stack([torch.from_numpy(synth.rodrigues(0.05 * rs.standard_normal(3))) for _ in range(B * pairs)]).reshape(B, pairs, 3, 3))
    T = _r32(rnd(B, pairs, 3, 1) * 0.1)
    Wc = _r32(rnd(B, K, 1) * 0.05)
    gR, gT, gW = _r32(rnd(B, pairs, 3, 3)), _r32(rnd(B, pairs, 3, 1)), _r32(rnd(B, K, 1))
    layers = []
    for w, b in he_normal_lambda_weights(C, 7):
        w = torch.as_tensor(w)
        layers.append((_r32(w.reshape(w.shape[-2], w.shape[-1])), _r32(torch.as_tensor(b).reshape(-1))))
    lam = lambda_of(absres, layers, N, pairs, l2_base, camera)
    A = damped_matrix(AtA, lam, camera)
    delta = torch.linalg.solve(A, Atb.unsqueeze(-1)).reshape(B, P)
    return dict(variant=variant, camera=camera, B=B, C=C, K=K, pairs=pairs, P=P, N=N, l2_base=l2_base, AtA=AtA, Atb=Atb, absres=absres,
                R=R, T=T, Wc=Wc, gR=gR, gT=gT, gW=gW, layers=layers, A=A, delta=delta)


OUTPUTS = ("gAtA", "gAtb", "gabs", "dR", "dT") + tuple("w%d.%s" % (i, k) for i in range(5) for k in ("filters", "biases"))
WEIGHT_OUTPUTS = OUTPUTS[5:]


def rel_err(got, want):
    """max-norm error on the tensor's own max-norm scale"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu().reshape(got.shape)
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


def sym(x):
    return 0.5 * (x + x.transpose(1, 2))
