"""Cases, metric, float32 twin and mutations for the entry-by-entry gate of the literal ops EquationConstruction and
EquationConstructionGrad (eqcon_syrk.hip, eqcon.hip, eqcon_grad.hip): one table shared by the CPU module
(test_eqcon_cases_cpu.py: the conditions on the inputs, the table against the two dispatch rules, the float32 twin, what the
metric sees that the max-norm gate of test_gpu_parity.py does not) and the GPU module (test_gpu_eqcon_entrywise.py).
No GPU here: numpy and the float64 oracle.

The metric.  Every output entry: err = |got - want| / scale.  `want` is the oracle in float64 on the float32 inputs
(equation_construction_gemm forward, equation_construction_grad backward); `scale` is THE SAME FUNCTION on the absolute values of
the inputs -- |J|^T |G|^T |G| |J| for AtA, |J|^T |G|^T |d| for Atb, |G|^T (2 |G| |J| |g0| + |d| |g1|^T) for dJ and the like for dG
and dd: what the entry would be if no two of its terms cancelled, i.e. the size of the numbers its sum is made of.  An entry whose
scale is 0 has no non-zero term and must be exactly 0.  No maximum is taken over a window before the division: an entry of a
small-scale block is held to its own scale, not to the largest entry of the matrix.

The gate is measured.  twin_forward / twin_backward evaluate the kernels' arrangement in float32 numpy, every sum one term after
the other in plain IEEE operations, so the figures do not depend on the host's BLAS or vector width (forward: the per-pixel
Cholesky records with the kernel's clamps, w = L^T J, W^T W, W^T h; backward: M, g, U = J g0, dJ = 2 M U + g g1^T, Q = U J^T,
v = J g1, dG = 2 G Q + d v^T, dd = G v).  F32_ERR[output] is the twin's worst err over the whole table, measured by
test_eqcon_cases_cpu.py, which fails if a case exceeds the constant below; GATE = 4 x F32_ERR: the project's margin for another
summation order and the six-of-nine bf16 products (pose_prior_ref.APPLY_GATE).

Families of inputs (all asymmetric: a transposed tile or swapped operands cannot pass):
  plain       standard normal.
  scaled      columns of J x 2^U(-10,10) -- the first min(6, P), the pose columns, x 2^U(-2,2) --, pixels of G x 2^U(-6,6),
              g0 symmetrised and then scaled by s s^T and g1 by s, s = 2^U(-8,8) per column.
  degenerate  scaled, plus a fifth of the pixels with gy = alpha gx over all channels (rank-1 M), a tenth with gx = 0, a tenth with
              gy = 0, a tenth with G = 0 and d != 0 (the counts rounded up), and, where P >= 3, column P // 2 of J all zero: rows
              and columns of AtA, an entry of Atb, whose scale is 0.
"""
import collections
import functools

import numpy as np

from oracle import banet_oracle as orc

FWD_OUTPUTS = ("AtA", "Atb")
BWD_OUTPUTS = ("dJ", "dG", "dd")
OLD_GATE = 3e-5          # test_gpu_parity.py: max|got - want| / max|want| per tensor
MARGIN = 4               # the project's factor between float32 numpy and a kernel (pose_prior_ref.APPLY_GATE)
TEETH = 10.0             # every mutation is seen at >= TEETH x GATE

# The twin's worst entrywise err over TABLE, per output, rounded up in the third digit.  Measured by
# test_eqcon_cases_cpu.py::test_float32_twin_is_within_its_constant (profiles/eqcon_entrywise.txt has the figure of every case).
F32_ERR = {"AtA": 1.16e-6, "Atb": 3.46e-7, "dJ": 9.63e-7, "dG": 8.23e-7, "dd": 6.74e-7}
GATE = {k: MARGIN * v for k, v in F32_ERR.items()}

Case = collections.namedtuple("Case", "B N C P family")

P_MAX = 304
LDS_BYTES = 160 * 1024


def case_id(c):
    return "B%d-N%d-C%d-P%d-%s" % c


# ---- the two dispatch rules, restated (eqcon.hip eq_nb; eqcon_grad.hip launch_eq_grad_fast) --------------------------------
FWD_CLASSES = (1, 2, 3, 5, 9, 17, 19)                       # template classes; 17 = the one-pass four-wave job kernel, 19 = it + 3 jobs
FWD_CLASS_EDGES = {1: (1, 16), 2: (17, 32), 3: (33, 48), 5: (49, 80), 9: (81, 144), 17: (145, 272), 19: (273, 304)}


def fwd_class(P):
    if P < 1:
        return None
    nb = (P + 15) // 16
    for c in FWD_CLASSES:
        if nb <= c:
            return c
    return None


BWD_FORMS = ("1", "3", "5", "9", "17c", "19c")             # four single-pass forms, two chunked
BWD_FORM_EDGES = {"1": (1, 16), "3": (17, 48), "5": (49, 80), "9": (81, 144), "17c": (145, 272), "19c": (273, 304)}


def bwd_form(P):
    if P < 1:
        return None
    nb = (P + 15) // 16
    if nb <= 1:
        return "1"
    if nb <= 3:
        return "3"
    if nb <= 5:
        return "5"
    if nb <= 9:
        return "9"
    if nb <= 17:
        return "17c"
    if nb <= 19:
        return "19c"
    return None


def bwd_passes(P):
    """the launches of eq_grad_u_kernel<NBK, NB> for P: [(NBK, NB, ob0, blocks of the chunk that hold real columns)]"""
    nb, form = (P + 15) // 16, bwd_form(P)
    if form is None:
        return []
    if form in ("1", "3", "5", "9"):
        k = int(form)
        return [(k, k, 0, nb)]
    out = []
    for ob in range(0, nb, 5):
        real = min(5, nb - ob)
        if form == "17c":
            out.append((17, 5 if nb - ob > 2 else 2, ob, real))
        else:
            out.append((19, 5, ob, real))
    return out


def bwd_tail(P):
    """(NBK, NB, real blocks) of the last chunk of a chunked P, else None"""
    ps = bwd_passes(P)
    return (ps[-1][0], ps[-1][1], ps[-1][3]) if len(ps) > 1 else None


# the tails the table must hold: <17,2> with one block (nb 11, 16) and two (12, 17), <17,5> with three (13), four (14) and five (10, 15),
# <19,5>'s last chunk with three (18) and four (19)
BWD_TAILS = ((17, 2, 1), (17, 2, 2), (17, 5, 3), (17, 5, 4), (17, 5, 5), (19, 5, 3), (19, 5, 4))
BWD_TAIL_NBS = (10, 11, 12, 13, 14, 15, 16, 17, 18, 19)


def channel_trips(C):
    """trips of the channel loop of eq_pixel_records_kernel / eq_grad_gd_kernel: ('even', c += 128) or ('odd', c += 64)"""
    return ("even", (C + 127) // 128) if C % 2 == 0 else ("odd", (C + 63) // 64)


def fwd_groups(B, N):
    """Gr of plan_eq's matrix-pipe branch: workgroups per window"""
    steps = (N + 15) // 16
    return max(1, min((256 + B - 1) // B, (steps + 3) // 4))


def bwd_groups(B, N):
    nblk = (N + 7) // 8
    return max(1, min((256 + B - 1) // B, (nblk + 7) // 8))


def null_form_lds(P):
    """dynamic LDS of eq_construction_grad_kernel (launch_eq_grad): beyond 160 KB the call is BANET_ERR_UNSUPPORTED"""
    return (4 * 32 * (P + 1) + ((P + 3) & ~3) + 32 * 12) * 4


# ---- the table -------------------------------------------------------------------------------------------------------------------
EDGE_PS = (1, 6, 16, 17, 32, 33, 48, 49, 64, 80, 81, 128, 144, 145, 160, 161, 192, 208, 224, 240, 256, 257, 272, 273, 288, 289, 304)
N_AXIS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)
C_AXIS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 255, 256, 300)
P_SMALL, P_CHUNKED = 23, 165                                  # N axis: class 2 / form 3, and nb = 11 (four-wave jobs; <17,5> x 2 + <17,2>)
DEGENERATE_PS = (6, 23, 38, 70, 134, 165, 262, 298)           # one P per class of either op (165 and 262: both tails of the 17 chunks)
UNSUPPORTED_P = 305
NULL_FORM_UNSUPPORTED_P = 314                                 # the first P whose J and U tiles do not fit the LDS


def _table():
    t = []
    # P at both edges of every class and every multiple of 16 that is one; small N, B and C alternating, N ragged in 8, 16 and 32
    for i, P in enumerate(EDGE_PS):
        t.append(Case(1 + i % 2, (40, 21, 35)[i % 3], (6, 5, 4, 7)[i % 4], P, "scaled" if i % 3 else "plain"))
    for i, N in enumerate(N_AXIS):
        t.append(Case(1 + i % 2, N, (5, 4)[i % 2], P_SMALL, "plain"))
        t.append(Case(1, N, (4, 3)[i % 2], P_CHUNKED, "scaled"))
    t.append(Case(300, 40, 4, 6, "scaled"))                   # Gr clamps to 1: a wave runs more than one step
    for i, C in enumerate(C_AXIS):
        t.append(Case(1, (33, 20)[i % 2], C, (38, 70, 6)[i % 3], "scaled"))
    for i, P in enumerate(DEGENERATE_PS):
        t.append(Case(1 + i % 2, 80, (6, 5)[i % 2], P, "degenerate"))
    # more than one workgroup a window (Gr = 2 in both ops), several steps a wave, the last step ragged; and the four-wave job kernel
    # with three and four steps a workgroup (both operand buffers, twice)
    t.append(Case(128, 330, 2, 23, "plain"))
    t.append(Case(128, 100, 3, 165, "scaled"))
    assert len(set(t)) == len(t)
    return tuple(t)


TABLE = _table()
SMALL_CASES = tuple(c for c in TABLE if c.B * c.N * c.P * c.P <= 40 * 80 * 80)   # the literal [N,P,P] form is pinned on these


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _seed(c):
    return (c.B * 1000003 + c.N * 10007 + c.C * 101 + c.P * 7 + {"plain": 0, "scaled": 1, "degenerate": 2}[c.family]) % (2 ** 31)


def degenerate_sets(N):
    """pixel index sets (rank1, gx0, gy0, g0) of the degenerate family: the same for every window of a case"""
    perm = np.random.RandomState(977 + N).permutation(N)
    n5, n10 = -(-N // 5), -(-N // 10)
    cuts = np.cumsum([0, n5, n10, n10, n10])
    return tuple(np.sort(perm[cuts[i]:cuts[i + 1]]) for i in range(4))


@functools.lru_cache(maxsize=None)
def make(c):
    """float32 inputs of a case: dict J [B,N,2,P], G [B,N,C,2], d [B,N,C,1], g0 [B,P,P], g1 [B,P,1] (+ what the family drew)"""
    B, N, C, P, family = c
    rng = np.random.RandomState(_seed(c))
    J = rng.standard_normal((B, N, 2, P))
    G = rng.standard_normal((B, N, C, 2))
    d = rng.standard_normal((B, N, C, 1))
    g0 = rng.standard_normal((B, P, P))
    g0 = g0 + np.swapaxes(g0, 1, 2)                           # symmetric: utils.cu:651's alpha = 2 assumes it
    g1 = rng.standard_normal((B, P, 1))
    out = {}
    if family in ("scaled", "degenerate"):
        e = rng.uniform(-10, 10, (B, P))
        e[:, :min(6, P)] = rng.uniform(-2, 2, (B, min(6, P)))
        # (rounded to float32 first: what the arrays carry then does not hang on the last bit of a platform's pow)
        colscale = (2.0 ** e).astype(np.float32).astype(np.float64)
        pixscale = (2.0 ** rng.uniform(-6, 6, (B, N))).astype(np.float32).astype(np.float64)
        s = (2.0 ** rng.uniform(-8, 8, (B, P))).astype(np.float32).astype(np.float64)
        J = J * colscale[:, None, None, :]
        G = G * pixscale[:, :, None, None]
        g0 = g0 * (s[:, :, None] * s[:, None, :])             # s_i s_j = s_j s_i to the bit: g0 stays exactly symmetric
        g1 = g1 * s[:, :, None]
        out.update(colscale=colscale, pixscale=pixscale, s=s)
    J, G, d, g0, g1 = (np.ascontiguousarray(x, np.float32) for x in (J, G, d, g0, g1))
    if family == "degenerate":
        rank1, gx0, gy0, gz = degenerate_sets(N)
        alpha = rng.uniform(-2, 2, (B, len(rank1))).astype(np.float32)
        alpha = np.where(np.abs(alpha) < 0.25, np.float32(0.25), alpha)
        Gx, Gy = G[..., 0], G[..., 1]                          # views
        Gy[:, rank1] = alpha[:, :, None] * Gx[:, rank1]
        Gx[:, gx0] = 0
        Gy[:, gy0] = 0
        G[:, gz] = 0
        if P >= 3:
            J[..., P // 2] = 0
        out.update(alpha=alpha)
    out.update(J=J, G=G, d=d, g0=g0, g1=g1)
    for v in out.values():
        v.setflags(write=False)
    return out


def _f64(inp, names):
    return [inp[k].astype(np.float64) for k in names]


# ---- float64 answers and scales (computed once per case, shared, never written to) ---------------------------------------------
def _frozen(arrs):
    for a in arrs:
        a.setflags(write=False)
    return tuple(arrs)


@functools.lru_cache(maxsize=None)
def want_forward(c):
    J, G, d = _f64(make(c), "JGd")
    return dict(zip(FWD_OUTPUTS, _frozen(orc.equation_construction_gemm(J, G, d))))


@functools.lru_cache(maxsize=None)
def scale_forward(c):
    J, G, d = (np.abs(x) for x in _f64(make(c), "JGd"))
    return dict(zip(FWD_OUTPUTS, _frozen(orc.equation_construction_gemm(J, G, d))))


def grad64(J, G, d, g0, g1):
    """equation_construction_grad, window by window (its [B,N,C,P] intermediates stay small)"""
    outs = [orc.equation_construction_grad(J[b:b + 1], G[b:b + 1], d[b:b + 1], g0[b:b + 1], g1[b:b + 1]) for b in range(J.shape[0])]
    return [np.concatenate([o[i] for o in outs], axis=0) for i in range(3)]


@functools.lru_cache(maxsize=None)
def want_backward(c):
    return dict(zip(BWD_OUTPUTS, _frozen(grad64(*_f64(make(c), ("J", "G", "d", "g0", "g1"))))))


@functools.lru_cache(maxsize=None)
def scale_backward(c):
    return dict(zip(BWD_OUTPUTS, _frozen(grad64(*(np.abs(x) for x in _f64(make(c), ("J", "G", "d", "g0", "g1")))))))


# ---- the metric ------------------------------------------------------------------------------------------------------------------
Errors = collections.namedtuple("Errors", "worst index nonzero_at_zero_scale nonfinite")


def entry_errors(got, want, scale):
    """err = |got - want| / scale entry by entry -> Errors(worst err, its index, entries that are not exactly 0 where the scale is 0,
    entries that are not finite).  A non-finite entry counts as err = inf."""
    got = np.asarray(got, np.float64).reshape(want.shape)
    live = scale > 0
    err = np.zeros(want.shape)
    np.divide(np.abs(got - want), scale, out=err, where=live)
    bad = ~np.isfinite(got)
    err[bad & live] = np.inf
    i = int(np.argmax(err))
    return Errors(float(err.flat[i]), tuple(int(v) for v in np.unravel_index(i, want.shape)), int(np.count_nonzero(got[~live] != 0)),
                  int(np.count_nonzero(bad)))


def block_errors(got, want, scale):
    """AtA: worst err per 16 x 16 block -> [nb, nb] (the maximum over windows of each block's worst ENTRY: divided first)"""
    got = np.asarray(got, np.float64).reshape(want.shape)
    err = np.zeros(want.shape)
    np.divide(np.abs(got - want), scale, out=err, where=scale > 0)
    err[~np.isfinite(got) & (scale > 0)] = np.inf
    B, P, _ = want.shape
    nb = (P + 15) // 16
    pad = np.zeros((B, nb * 16, nb * 16))
    pad[:, :P, :P] = err
    return pad.reshape(B, nb, 16, nb, 16).max(axis=(0, 2, 4))


def old_metric(got, want):
    """test_gpu_parity.py's relerr: one number per tensor"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def forward_errors(c, AtA, Atb):
    w, s = want_forward(c), scale_forward(c)
    return {"AtA": entry_errors(AtA, w["AtA"], s["AtA"]), "Atb": entry_errors(Atb, w["Atb"], s["Atb"])}


def backward_errors(c, dJ, dG, dd):
    w, s = want_backward(c), scale_backward(c)
    return {k: entry_errors(v, w[k], s[k]) for k, v in zip(BWD_OUTPUTS, (dJ, dG, dd))}


def gate_failures(errors):
    """what of {output: Errors} misses its gate: a list of strings, empty if all is well"""
    out = []
    for k, e in errors.items():
        if e.nonfinite:
            out.append("%s: %d entries not finite" % (k, e.nonfinite))
        if e.nonzero_at_zero_scale:
            out.append("%s: %d entries with scale 0 are not exactly 0" % (k, e.nonzero_at_zero_scale))
        if not e.worst <= GATE[k]:
            out.append("%s: err %.3e at %s > gate %.3e" % (k, e.worst, e.index, GATE[k]))
    return out


# ---- the float32 twin: the kernels' arrangement in float32 numpy ---------------------------------------------------------------
F = np.float32


L22_FLOOR = F(2.0 ** -24)    # eq_pixel_records_kernel: l22^2 >= 2^-24 m22


def _seq_sum(n, term):
    """term(0) + term(1) + ... + term(n - 1) in float32, one term after the other: plain IEEE multiplies and adds, the same bits on
    every host (no BLAS, no pairwise or vectorised reduction whose order depends on the machine)"""
    acc = term(0).astype(F, copy=True)
    for k in range(1, n):
        acc += term(k)
    assert acc.dtype == F
    return acc


def _seq_dot(a, b):
    """sum over the LAST axis of a * b, sequentially"""
    return _seq_sum(a.shape[-1], lambda k: a[..., k] * b[..., k])


def pixel_records32(G, d, l22_floor=L22_FLOOR):
    """eq_pixel_records_kernel: (m11, m12, m22, g1, g2) and (l11, l21, l22, h0, h1) with its clamps, all float32 [B,N].
    l22_floor = 0: the records as they were before the floor (test_eqcon_cases_cpu.py shows what that loses in Atb)."""
    gx, gy, dd = G[..., 0], G[..., 1], d[..., 0]
    m11, m12, m22 = _seq_dot(gx, gx), _seq_dot(gx, gy), _seq_dot(gy, gy)
    g1, g2 = _seq_dot(gx, dd), _seq_dot(gy, dd)
    with np.errstate(divide="ignore", invalid="ignore"):
        l11 = np.sqrt(np.maximum(m11, F(0)))
        i11 = np.where(l11 > 0, F(1) / l11, F(0)).astype(F)
        l21 = m12 * i11
        l22 = np.sqrt(np.maximum(m22 - l21 * l21, F(l22_floor) * m22))
        i22 = np.where(l22 > 0, F(1) / l22, F(0)).astype(F)
        h0 = g1 * i11
        h1 = (g2 - l21 * h0) * i22
    return (m11, m12, m22, g1, g2), (l11, l21, l22, h0, h1)


def twin_forward(c, l22_zero_at=None, l22_floor=L22_FLOOR):
    """w = L^T J, AtA = W^T W, Atb = W^T h in float32 -> (AtA [B,P,P], Atb [B,P,1]).  l22_zero_at: pixels whose l22 (and h1) are
    forced to 0 -- a mutation, not the kernel."""
    inp = make(c)
    J, G, d = inp["J"], inp["G"], inp["d"]
    _, (l11, l21, l22, h0, h1) = pixel_records32(G, d, l22_floor)
    if l22_zero_at is not None:
        l22, h1 = l22.copy(), h1.copy()
        l22[:, l22_zero_at] = 0
        h1[:, l22_zero_at] = 0
    Jx, Jy = J[:, :, 0, :], J[:, :, 1, :]
    W = np.stack([l11[..., None] * Jx + l21[..., None] * Jy, l22[..., None] * Jy], axis=2).reshape(c.B, 2 * c.N, c.P)
    h = np.stack([h0, h1], axis=2).reshape(c.B, 2 * c.N, 1)
    assert W.dtype == F and h.dtype == F
    AtA = _seq_sum(2 * c.N, lambda r: W[:, r, :, None] * W[:, r, None, :])       # over the 2N rows
    Atb = _seq_sum(2 * c.N, lambda r: W[:, r, :] * h[:, r, :])[..., None]
    assert AtA.dtype == F and Atb.dtype == F
    return AtA, Atb


def twin_backward(c):
    """-> (dJ, dG, dd) in float32, arranged as eq_grad_u_kernel / eq_grad_gd_kernel arrange them"""
    inp = make(c)
    J, G, d, g0, g1 = (inp[k] for k in ("J", "G", "d", "g0", "g1"))
    (m11, m12, m22, q1, q2), _ = pixel_records32(G, d)
    U = _seq_sum(c.P, lambda k: J[..., k, None] * g0[:, None, None, k, :])       # [B,N,2,P]: over the rows of g0
    g1r = np.broadcast_to(g1[:, None, :, 0], (c.B, c.N, c.P))
    j0, j1, u0, u1 = J[:, :, 0], J[:, :, 1], U[:, :, 0], U[:, :, 1]
    v0, v1 = _seq_dot(j0, g1r), _seq_dot(j1, g1r)
    dJ = np.stack([F(2) * (m11[..., None] * u0 + m12[..., None] * u1) + q1[..., None] * g1r,
                   F(2) * (m12[..., None] * u0 + m22[..., None] * u1) + q2[..., None] * g1r], axis=2)
    q00, q01, q10, q11 = _seq_dot(u0, j0), _seq_dot(u0, j1), _seq_dot(u1, j0), _seq_dot(u1, j1)
    gx, gy, dd_ = G[..., 0], G[..., 1], d[..., 0]
    e = lambda x: x[..., None]                                      # per pixel -> over its channels
    dG = np.stack([F(2) * (gx * e(q00) + gy * e(q10)) + dd_ * e(v0), F(2) * (gx * e(q01) + gy * e(q11)) + dd_ * e(v1)], axis=3)
    dd = (gx * e(v0) + gy * e(v1))[..., None]
    assert dJ.dtype == F and dG.dtype == F and dd.dtype == F
    return dJ, dG, dd


# ---- mutations of the float64 answer: what a subtly wrong kernel would give ----------------------------------------------------
def smallest_quarter(scale, axes):
    """boolean mask of the quarter block with the smallest scale, window by window: along each of the two `axes`, the half of the
    indices whose largest scale in that window is smallest (an axis of length 1: all of it)"""
    mask = np.ones(scale.shape, bool)
    B = scale.shape[0]
    for ax in axes:
        n = scale.shape[ax]
        if n < 2:
            continue
        size = scale.max(axis=tuple(a for a in range(1, scale.ndim) if a != ax))     # [B, n]
        keep = np.zeros((B, n), bool)
        np.put_along_axis(keep, np.argsort(size, axis=1, kind="stable")[:, :n // 2], True, axis=1)
        shape = [B] + [1] * (scale.ndim - 1)
        shape[ax] = n
        mask &= keep.reshape(shape)
    return mask


# output -> the two axes whose small-scale halves make the quarter: columns x columns; columns; pixels x columns; pixels
QUARTER_AXES = {"AtA": (1, 2), "Atb": (1,), "dJ": (1, 3), "dG": (1,), "dd": (1,)}


def mutate_five_percent(want, scale, output):
    """5 % on the smallest-scale quarter block (Atb, dG, dd: on the smallest-scale half of the columns / pixels)"""
    out = want.copy()
    out[smallest_quarter(scale, QUARTER_AXES[output])] *= 1.05
    return out


def _with(c, **repl):
    x = dict(zip(("J", "G", "d", "g0", "g1"), _f64(make(c), ("J", "G", "d", "g0", "g1"))))
    x.update(repl)
    return x


def mutate_forward(c, kind):
    """the float64 forward answer of a kernel with one fault -> (AtA, Atb)"""
    x = _with(c)
    J, G, d = x["J"], x["G"], x["d"]
    if kind == "column":                                       # column P - 1 read as zero
        J = J.copy()
        J[..., c.P - 1] = 0
    elif kind == "pixel":                                      # pixel N - 1 never visited
        J, G, d = J[:, :-1], G[:, :-1], d[:, :-1]
    elif kind == "channels":                                   # the channel loop's trips after the first never run
        keep = 128 if c.C % 2 == 0 else 64
        G, d = G[:, :, :keep], d[:, :, :keep]
    elif kind == "tile":                                       # the 16 x 16 tile (0, 1) published transposed (and mirrored)
        AtA, Atb = orc.equation_construction_gemm(J, G, d)
        AtA = AtA.copy()
        AtA[:, 0:16, 16:32] = np.swapaxes(AtA[:, 0:16, 16:32], 1, 2).copy()
        AtA[:, 16:32, 0:16] = np.swapaxes(AtA[:, 0:16, 16:32], 1, 2)
        return AtA, Atb
    else:
        raise KeyError(kind)
    return orc.equation_construction_gemm(J, G, d)


def rank1_neighbours(c):
    """pixels next to a rank-1 pixel that are in none of the degenerate sets themselves"""
    sets = degenerate_sets(c.N)
    special = set(np.concatenate(sets).tolist())
    nb = sorted({int(n + o) for n in sets[0] for o in (-1, 1) if 0 <= n + o < c.N and int(n + o) not in special})
    return np.asarray(nb, int)


def mutate_l22(c):
    """l22 (hence h1) read as 0 on the rank-1 pixels' neighbours: the float64 answer without those pixels' second Cholesky row"""
    x = _with(c)
    J, G, d = x["J"], x["G"], x["d"]
    nb = rank1_neighbours(c)
    gx, gy, dd = G[..., 0][:, nb], G[..., 1][:, nb], d[..., 0][:, nb]
    m11, m12, m22 = (gx * gx).sum(-1), (gx * gy).sum(-1), (gy * gy).sum(-1)
    g1, g2 = (gx * dd).sum(-1), (gy * dd).sum(-1)
    l22sq = m22 - m12 * m12 / m11
    r2 = g2 - m12 * g1 / m11                                     # h1 l22
    Jy = J[:, :, 1, :][:, nb]
    AtA, Atb = orc.equation_construction_gemm(J, G, d)
    AtA = AtA - np.einsum("bn,bni,bnj->bij", l22sq, Jy, Jy)
    Atb = Atb - np.einsum("bn,bni->bi", r2, Jy)[..., None]
    return AtA, Atb


def mutate_backward(c, kind):
    """the float64 backward answer of a kernel with one fault -> (dJ, dG, dd)"""
    x = _with(c)
    J, G, d, g0, g1 = (x[k] for k in ("J", "G", "d", "g0", "g1"))
    if kind == "column":                                       # column P - 1 of J read as zero (the outputs keep their shape)
        J = J.copy()
        J[..., c.P - 1] = 0
        return grad64(J, G, d, g0, g1)
    if kind == "pixel":                                        # pixel N - 1 never visited: its rows stay as they were (zero here)
        outs = [o.copy() for o in grad64(J, G, d, g0, g1)]
        for o in outs:
            o[:, -1] = 0
        return outs
    if kind == "channels":                                     # both channel loops stop after their first trip
        keep = 128 if c.C % 2 == 0 else 64
        dJ, dG, dd = grad64(J, G[:, :, :keep], d[:, :, :keep], g0, g1)
        dGf, ddf = np.zeros(G.shape), np.zeros(d.shape)
        dGf[:, :, :keep], ddf[:, :, :keep] = dG, dd
        return dJ, dGf, ddf
    if kind == "g_g1t":                                        # g g1^T dropped from dJ
        dJ, dG, dd = grad64(J, G, d, g0, g1)
        g = np.matmul(np.swapaxes(G, 2, 3), d)                  # [B,N,2,1]
        return dJ - g * np.swapaxes(g1, 1, 2)[:, None], dG, dd
    raise KeyError(kind)
