"""Dense multi-level window solver: every pixel of every pyramid level is a BA point
(SURVEY.md 8(d) "dense mode"; the reference samples N=1024-4096 points instead).

Per level the layer's inputs are the CNN's outputs in their native layouts -- source and
target feature maps NHWC `[B,H_l,W_l,C]`, depth `[B,H_l,W_l]`, basis `[B,H_l,W_l,K]` -- and
the whole coarse->fine LM schedule is enqueued on the current stream without a host sync.
Iteration bodies: `bundle` = bundlenet.py:193-278 (pose + depth basis), `bundle_camera` =
bundlenet.py:122-191, `legacy_lm` / `legacy_fixed` = legacy/ba.py:226-345 / :148-214.
"""
import collections
import os

import torch

from . import ops

DenseMarginals = collections.namedtuple("DenseMarginals", "pose_cov depth_var wfactor logdet status sigma2 damping")
DepthTransfer = collections.namedtuple("DepthTransfer", "Wc depth_map index covered status")


class DensePrior:
    """What DenseBA.solve(prior=...) additionally minimises on every level l (ops.Prior, include/banet_hip.h (5d)):
        level_scale[l] (1/2 Wc^T Lambda Wc - eta^T Wc + 1/2 sum_n w_n (obs_n - depth_n - b_n . Wc)^2)
      coef        (Lambda [B,K,K], eta [B,K] or None), the same on every level (the coefficients are), or None
      depth_obs   one (obs, weight) pair per level, each [B,H_l,W_l] (weight None: 1), or None entries / None
      level_scale one factor per level (default 1).
    pose = (R0 [B,pairs,3,3], T0 [B,pairs,3], Lambda [B,6 pairs,6 pairs]): additionally level_scale[l] 1/2 r^T Lambda r on the poses,
    r = [Log(T_i o T0_i^-1)]_i (ops.PosePrior, header (5f)), the same on every level; `bundle`, and alone also `bundle_camera`."""

    def __init__(self, coef=None, depth_obs=None, level_scale=None, pose=None):
        self.coef = coef
        self.pose = tuple(pose) if pose is not None else None
        self.depth_obs = list(depth_obs) if depth_obs is not None else None
        self.level_scale = list(level_scale) if level_scale is not None else None

    def level_priors(self, problems):
        """-> one ops.Prior per level"""
        n = len(problems)
        if (self.depth_obs is not None and len(self.depth_obs) < n) or (self.level_scale is not None and len(self.level_scale) < n):
            raise ops.capi.BanetError("DensePrior: depth_obs / level_scale need one entry per level (%d)" % n)
        Lambda, eta = self.coef if self.coef is not None else (None, None)
        out = []
        for l, p in enumerate(problems):
            obs = self.depth_obs[l] if self.depth_obs is not None else None
            o, w = obs if obs is not None else (None, None)
            o = o.reshape(p.B, p.N) if o is not None else None
            w = w.reshape(p.B, p.N) if w is not None else None
            out.append(ops.Prior(Lambda, eta, o, w, scale=1.0 if self.level_scale is None else float(self.level_scale[l])))
        return out

    def level_pose_priors(self, problems):
        """-> one ops.PosePrior per level, or None without a pose prior"""
        if self.pose is None:
            return None
        n = len(problems)
        if self.level_scale is not None and len(self.level_scale) < n:
            raise ops.capi.BanetError("DensePrior: level_scale needs one entry per level (%d)" % n)
        R0, T0, Lambda = self.pose
        return [ops.PosePrior(R0, T0, Lambda, scale=1.0 if self.level_scale is None else float(self.level_scale[l])) for l in range(n)]


class DenseLevel:
    def __init__(self, scale, src, tgt, depth, basis=None):
        """tgt [B,H,W,C] (2-frame) or [B,pairs,H,W,C] (multi-frame window: `pairs` target frames that
        share the key frame's src / depth / basis -- SURVEY.md 8(d))"""
        self.scale = float(scale)
        self.src, self.tgt, self.depth, self.basis = src, tgt, depth, basis
        self.pairs = tgt.shape[1] if tgt.dim() == 5 else 1
        self.B, self.H, self.W, self.C = tgt.shape[0], tgt.shape[-3], tgt.shape[-2], tgt.shape[-1]


class DenseBA:
    def __init__(self, intr, levels, lambda_weights, variant="bundle", l2_base=1000.0, batch_invariant=False):
        """intr [B,4] full-resolution (fx,fy,ox,oy); levels: list of DenseLevel coarse->fine;
        lambda_weights: list (one per level) of 5 (filters, biases) pairs.
        batch_invariant: banet_level_t.policy = BANET_POLICY_BATCH_INVARIANT on every level -- kernels, SYRK form and summation
        split chosen from the level alone, so a window's bits do not depend on the batch / shard it is solved in (callers that
        shard one batch unevenly over GPUs and compare results bit for bit; slower below ~8 windows per launch).  Default: the
        launch decides (fastest; results agree to rounding across batchings)."""
        self.variant = variant
        self.levels, self.lambda_weights = list(levels), list(lambda_weights)
        self.l2_base = float(l2_base) if variant == "bundle" else 1.0
        self.intr = intr.contiguous().float()
        dev = self.intr.device
        legacy = variant.startswith("legacy")
        self.problems, self.mlps = [], []
        for lv, lw in zip(levels, lambda_weights):
            B, H, W, C = lv.B, lv.H, lv.W, lv.C
            basis = lv.basis.reshape(B, H * W, -1) if (variant == "bundle") else None
            self.problems.append(ops.LevelProblem(variant, lv.src, lv.tgt, lv.depth.reshape(B, H * W), H, W, C,
                                                  basis=basis, intr=self.intr, scale=lv.scale, dense=True,
                                                  tgt_has_grad=False, normalize_rays=not legacy, pairs=lv.pairs))
            self.mlps.append(None if variant == "legacy_fixed" else ops.MlpWeights(lw, dev))
        if batch_invariant:
            for p in self.problems:
                p.c.policy = ops.capi.POLICY_BATCH_INVARIANT
        self.K = self.problems[0].K
        self.pairs = self.problems[0].pairs
        nb = max(ops.lm_level_workspace_bytes(p) for p in self.problems)
        if nb == 0:
            raise ops.capi.BanetError("DenseBA: unsupported level shape")
        self.ws = ops.capi.workspace(nb, dev)
        self.B = self.problems[0].B
        # The coarsest level (<= 1200 pixels) of a large batch as two half batches on two HIP streams (host-side orchestration only;
        # opt-in: BANET_SPLIT_COARSE=1).  Measured at 32 windows (profiles/r05_run13_*): 40x30 1.37 -> 1.08 ms per 10 iterations, but
        # 80x60 +7 % and 160x120 +13 % when split too -- net zero over a solve, +0.5 % with the coarsest level alone: not the default.
        # Under the default throughput policy the two B / 2 launches choose kernels and summation splits from THEIR batch, so enabling
        # it changes results in the low bits (equal to rounding, like any other batching: DESIGN.md section 6); BATCH_INVARIANT does not.
        self.split_coarse = os.environ.get("BANET_SPLIT_COARSE", "0") == "1"
        self._parts, self._side = {}, None
        self._variant_args = dict(variant=variant, legacy=legacy)

    def _level_parts(self, li, st):
        """two half-batch views of level li (problems over slices of the level tensors, workspaces) + views of the state"""
        lv = self.levels[li]
        # the halves alias the level's tensors: rebuilt whenever one of them (or the level's problem) has been replaced since
        key = (id(self.problems[li]),) + tuple(t.data_ptr() for t in (lv.src, lv.tgt, lv.depth) + ((lv.basis,) if lv.basis is not None else ()))
        if li not in self._parts or self._parts[li][0] != key:
            B = self.B
            cuts = [(0, B // 2), (B // 2, B)]
            parts = []
            for lo, hi in cuts:
                H, W, C = lv.H, lv.W, lv.C
                basis = lv.basis[lo:hi].reshape(hi - lo, H * W, -1) if self.variant == "bundle" else None
                prob = ops.LevelProblem(self.variant, lv.src[lo:hi], lv.tgt[lo:hi], lv.depth[lo:hi].reshape(hi - lo, H * W), H, W, C,
                                        basis=basis, intr=self.intr[lo:hi], scale=lv.scale, dense=True, tgt_has_grad=False,
                                        normalize_rays=not self._variant_args["legacy"], pairs=lv.pairs)
                prob.c.flags, prob.c.policy = self.problems[li].c.flags, self.problems[li].c.policy
                parts.append((lo, hi, prob, ops.capi.workspace(ops.lm_level_workspace_bytes(prob), self.intr.device)))
            self._parts[li] = (key, parts)
        out = []
        for lo, hi, prob, ws in self._parts[li][1]:
            prob.c.flags, prob.c.policy = self.problems[li].c.flags, self.problems[li].c.policy    # (follow later changes of the level's)
            sub = ops.capi.State()
            sub.R, sub.T = st.R[lo:hi].data_ptr(), st.T[lo:hi].data_ptr()
            sub.Wc = st.Wc[lo:hi].data_ptr() if st.Wc is not None else None
            sub.iters, sub.ratio = st.iters[lo:hi].data_ptr(), st.ratio[lo:hi].data_ptr()
            sub.lambda_out, sub.delta = st.lambda_out[lo:hi].data_ptr(), st.delta[lo:hi].data_ptr()
            holder = type("SubState", (), {})()
            holder.c = sub
            out.append((prob, ws, holder))
        return out

    def new_state(self, R=None, T=None, Wc=None):
        dev = self.intr.device
        B, K = self.B, self.K
        R = torch.eye(3, device=dev).repeat(B * self.pairs, 1, 1) if R is None else R
        T = torch.zeros(B * self.pairs, 3, 1, device=dev) if T is None else T
        if K > 0 and Wc is None:
            Wc = torch.zeros(B, K, 1, device=dev)
        R = R.reshape(B, -1, 3, 3) if self.pairs > 1 else R
        T = T.reshape(B, -1, 3, 1) if self.pairs > 1 else T
        return ops.LmState(R, T, Wc if K > 0 else None, P=6 * self.pairs + K, pairs=self.pairs)

    # True: solve() is one banet_lm_solve_f32 call (the level loop, the counts and the snapshots on the C side); False: the
    # level loop below, one banet_lm_level_ex_f32 call per level.  Same bits either way.
    c_schedule = True

    def solve(self, iters_per_level, state=None, early_termination=False, params=None, snapshots=None, level_events=None,
              depth_outputs=None, prior=None):
        """Enqueue the full schedule; returns the state (R,T,Wc updated in place) and the list
        of per-level iteration-count tensors.  params: ops.lm_params(...) (legacy/ba.py:5-9) or None for the
        reference's defaults.  snapshots: a list that receives, per level, a dict of (R, T, W, delta, lam)
        after that level (device tensors, no host sync).  level_events: a list that receives one (start, end) pair of
        torch.cuda.Event per level, recorded on the current stream (per-level times without a host sync).  depth_outputs: a list
        that receives, per level, the depth map depth_l + basis_l . Wc after that level, shaped like the level's depth
        (bundlenet.py:397 output_depths; `bundle` only).  prior: a DensePrior -- depth observations and / or a prior on the
        coefficients, added between assembly and solve of every iteration (`bundle` only, no early termination; the same bits on
        the one-call path and on the per-level path); with pose=(R0, T0, Lambda) a prior on the poses as well, or alone (then also
        `bundle_camera`); None = the call path without one."""
        st = state if state is not None else self.new_state()
        if depth_outputs is not None and self.variant != "bundle":
            raise ops.capi.BanetError("DenseBA.solve: depth_outputs need the `bundle` variant (a depth basis)")
        n = min(len(self.problems), len(iters_per_level))
        priors = pose_priors = None
        if prior is not None:
            pose_only = prior.pose is not None and prior.coef is None and prior.depth_obs is None
            if early_termination or not (self.variant == "bundle" or (pose_only and self.variant == "bundle_camera")):
                raise ops.capi.BanetError("DenseBA.solve: a prior needs the `bundle` variant and excludes early termination")
            if not pose_only:
                priors = prior.level_priors(self.problems[:n])
            pose_priors = prior.level_pose_priors(self.problems[:n])
            need = [ops.lm_level_workspace_bytes(p, priors[l] if priors is not None else None, pose_priors[l] if pose_priors is not None else None)
                    for l, p in enumerate(self.problems[:n])]
            if min(need) == 0:
                raise ops.capi.BanetError("DenseBA.solve: the prior does not fit the levels")
            if self.ws.numel() < max(need):
                self.ws = ops.capi.workspace(max(need), self.intr.device)
        if self.c_schedule and level_events is None and not self.split_coarse and 1 <= n <= 16:
            # one call: counts / snapshots are views of the trace rows (allocated per call), nothing is cloned per level
            depth = None
            if depth_outputs is not None:
                depth = [torch.empty((p.B, p.N), dtype=torch.float32, device=p.device) for p in self.problems[:n]]
            trace = ops.SolveTrace(n, st, fields=None if snapshots is not None else ("iters",), depth=depth)
            ops.lm_solve(self.problems[:n], self.mlps[:n], self.l2_base, list(iters_per_level[:n]), early_termination, st,
                         ws=self.ws, params=params, trace=trace, priors=priors, pose_priors=pose_priors)
            if snapshots is not None:
                snapshots.extend(dict(R=trace.R[l], T=trace.T[l], W=None if trace.Wc is None else trace.Wc[l],
                                      delta=trace.delta[l], lam=trace.lambda_out[l]) for l in range(n))
            if depth_outputs is not None:
                depth_outputs.extend(d.reshape(lv.depth.shape) for d, lv in zip(depth, self.levels))
            return st, [trace.iters[l] for l in range(n)]
        counts = []
        for prob, mlp, its in zip(self.problems, self.mlps, iters_per_level):
            if level_events is not None:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record()
            li = len(counts)
            if self.split_coarse and priors is None and pose_priors is None and self.B >= 16 and prob.N <= 1200 and li < len(self.levels):
                # two half batches, the second on a side stream; joined before the next level (the state tensors are shared)
                dev = self.intr.device
                cur = torch.cuda.current_stream(dev)
                if self._side is None:
                    self._side = torch.cuda.Stream(device=dev)
                (p0, w0, s0), (p1, w1, s1) = self._level_parts(li, st)
                self._side.wait_stream(cur)
                ops.lm_level(p0, mlp, self.l2_base, its, early_termination, s0, ws=w0, params=params)
                with torch.cuda.stream(self._side):
                    ops.lm_level(p1, mlp, self.l2_base, its, early_termination, s1, ws=w1, params=params)
                cur.wait_stream(self._side)
            else:
                ops.lm_level(prob, mlp, self.l2_base, its, early_termination, st, ws=self.ws, params=params,
                             prior=priors[li] if (priors is not None and li < len(priors)) else None,
                             pose_prior=pose_priors[li] if (pose_priors is not None and li < len(pose_priors)) else None)
            if level_events is not None:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record()
                level_events.append((e0, e1))
            counts.append(st.iters.clone())
            if snapshots is not None:
                snapshots.append(dict(R=st.R.clone(), T=st.T.clone(), W=None if st.Wc is None else st.Wc.clone(),
                                      delta=st.delta.clone(), lam=st.lambda_out.clone()))
            if depth_outputs is not None:
                depth_outputs.append(ops.depth_output(prob.keep[2], prob.keep[3], st.Wc).reshape(self.levels[li].depth.shape))
        return st, counts

    def solve_differentiable(self, iters_per_level, R=None, T=None, Wc=None, outputs=None, prior=None, pose_prior_backward=False):
        """The same fixed-count schedule attached to the autograd graph: gradients flow to the levels' src / tgt / depth /
        basis tensors, to the initial (R, T, Wc) and to the lambda weights through the fused backward kernels
        (banet_amd/dense_train.py, csrc/adjoint.hip; the reference differentiates bundlenet.py:376-397 with tf.gradients +
        EquationConstructionGrad).  `bundle` (K <= 256) and the pose-only `bundle_camera` variant; two-frame and multi-frame
        windows.  outputs: a list that receives (R, T, Wc) after each level, attached to the graph.  prior: a DensePrior as in
        solve(prior=) (`bundle` only, K >= 1); its tensors may require grad -- a learned obs_depth / obs_weight, the (Lambda, eta) of
        transfer_prior -- and the levels' depth and basis receive the term's gradient as well.  None or empty: today's launches.
        A prior with pose=: NotImplementedError unless pose_prior_backward=True, which differentiates through the pose prior as well
        (gradients reach R0, T0 and Lambda; `bundle`, and with a pose prior alone also `bundle_camera`); the default keeps the
        earlier refusal until a later change flips it."""
        from . import dense_train
        return dense_train.solve_differentiable(self, self.levels, self.lambda_weights, iters_per_level, R, T, Wc, outputs=outputs,
                                                prior=prior, pose_prior_backward=pose_prior_backward)

    def step_from(self, level_index, R, T, Wc=None):
        """ONE iteration of level `level_index` from the given state -> (state after it; .delta / .lambda_out hold the
        solved update and lambda).  Used by the parity checks to compare single updates from identical states."""
        st = self.new_state(R, T, Wc)
        ops.lm_level(self.problems[level_index], self.mlps[level_index], self.l2_base, 1, False, st, ws=self.ws)
        return st

    def residual(self, level_index, state=None, R=None, T=None, Wc=None, proj=False, differentiable=False):
        """banet_ba_residual_f32 on level `level_index` at a state (an LmState, or R / T / Wc; default: new_state()) ->
        ops.Residual(sq, ab [B,pairs,H,W] float32, mask [B,pairs,H,W] bool, proj [B,pairs,H,W,2] or None, sums [B,pairs,4] =
        (sum sq, sum ab, in-image count, max sq) per window and target frame).  No host sync.
        differentiable=True: the maps are attached to the autograd graph (ops.ba_residual_diff: gradients reach R / T / Wc as given
        and the level's src / tgt / depth / basis tensors through banet_ba_residual_grad_f32); sums is then None."""
        p = self.problems[level_index]
        if differentiable:
            if state is not None:
                R, T, Wc = state.R, state.T, state.Wc
            elif R is None or T is None or (self.K > 0 and Wc is None):
                st = self.new_state(R, T, Wc)
                R, T, Wc = (st.R if R is None else R), (st.T if T is None else T), (st.Wc if Wc is None else Wc)
            sq, ab, mask, pr = ops.ba_residual_diff(p, R, T, Wc if self.K > 0 else None, proj=proj)
            shape = (p.B, p.pairs, int(p.c.H), int(p.c.W))
            return ops.Residual(sq.reshape(shape), ab.reshape(shape), mask.reshape(shape).bool(),
                                pr.reshape(shape + (2,)) if proj else None, None)
        st = state if state is not None else self.new_state(R, T, Wc)
        r = ops.ba_residual(p, st.R, st.T, st.Wc if self.K > 0 else None, proj=proj, sums=True)
        H, W = int(p.c.H), int(p.c.W)
        shape = (p.B, p.pairs, H, W)
        return ops.Residual(r.sq.reshape(shape), r.ab.reshape(shape), r.mask.reshape(shape).bool(),
                            r.proj.reshape(shape + (2,)) if proj else None, r.sums)

    def marginals(self, level_index, state=None, R=None, T=None, Wc=None, damping=0.0, sigma2="residual",
                  want=("pose_cov", "depth_var"), differentiable=False):
        """How sure is the solve?  The posterior marginals of level `level_index` at a state (an LmState, or R / T / Wc; default:
        new_state()): one assembly pass (ops.ba_assemble, the exact SYRK form) for the normal matrix, then ops.ba_marginals ->
        DenseMarginals(pose_cov [B,6 pairs,6 pairs], depth_var [B,H,W], wfactor, logdet, status [B], sigma2 [B] or None, damping [B]
        or None -- the last two as they were passed on).
        sigma2: "residual" = the residual variance at the state, sum_f sum sq / max(C sum_f count - P, 1) from residual().sums;
        None = 1; a float or a tensor [B] is passed through.  damping: a float, a tensor [B], or "lambda" = state.lambda_out (the
        last lambda of the solve).  No host sync.
        differentiable=True: the outputs are attached to the autograd graph -- dense_train.assemble_differentiable, then
        ops.ba_marginals_diff; sigma2="residual" from the maps of ops.ba_residual_diff with torch sums.  Gradients of pose_cov,
        depth_var and logdet reach R / T / Wc as given (or the state's tensors) and the level's src / tgt / depth / basis, and
        damping / sigma2 where they are tensors that require grad; wfactor and status carry none.  The levels the dense adjoint
        takes (bundle, bundle_camera)."""
        if differentiable:
            return self._marginals_differentiable(level_index, state, R, T, Wc, damping, sigma2, want)
        p = self.problems[level_index]
        if isinstance(damping, str):
            if damping != "lambda":
                raise ops.capi.BanetError("DenseBA.marginals: damping is a number, a tensor or \"lambda\"")
            if state is None:
                raise ops.capi.BanetError("DenseBA.marginals: damping=\"lambda\" needs the solved state")
            damping = state.lambda_out
        st = state if state is not None else self.new_state(R, T, Wc)
        wc = st.Wc if self.K > 0 else None
        if isinstance(sigma2, str):
            if sigma2 != "residual":
                raise ops.capi.BanetError("DenseBA.marginals: sigma2 is None, a number, a tensor or \"residual\"")
            sums = ops.ba_residual(p, st.R, st.T, wc, sums=True).sums
            sigma2 = sums[:, :, 0].sum(dim=1) / torch.clamp(p.C * sums[:, :, 2].sum(dim=1) - float(p.P), min=1.0)
        AtA = ops.ba_assemble(p, st.R, st.T, wc)[0]
        m = ops.ba_marginals(p, AtA, damping=damping, sigma2=sigma2, want=want)
        dv = m.depth_var.reshape(p.B, int(p.c.H), int(p.c.W)) if m.depth_var is not None else None
        as_t = lambda v: v if (v is None or torch.is_tensor(v)) else torch.full((p.B,), float(v), dtype=torch.float32, device=p.device)
        return DenseMarginals(m.pose_cov, dv, m.wfactor, m.logdet, m.status, as_t(sigma2), as_t(damping))

    def _marginals_differentiable(self, level_index, state, R, T, Wc, damping, sigma2, want):
        from . import dense_train
        p = self.problems[level_index]
        if isinstance(damping, str):
            if damping != "lambda":
                raise ops.capi.BanetError("DenseBA.marginals: damping is a number, a tensor or \"lambda\"")
            if state is None:
                raise ops.capi.BanetError("DenseBA.marginals: damping=\"lambda\" needs the solved state")
            damping = state.lambda_out
        if state is not None:
            R, T, Wc = state.R, state.T, state.Wc
        elif R is None or T is None or (self.K > 0 and Wc is None):
            st = self.new_state(R, T, Wc)
            R, T, Wc = (st.R if R is None else R), (st.T if T is None else T), (st.Wc if Wc is None else Wc)
        wc = Wc if self.K > 0 else None
        if isinstance(sigma2, str):
            if sigma2 != "residual":
                raise ops.capi.BanetError("DenseBA.marginals: sigma2 is None, a number, a tensor or \"residual\"")
            sq, _, mask, _ = ops.ba_residual_diff(p, R, T, wc)
            sigma2 = sq.sum(dim=(1, 2)) / torch.clamp(p.C * mask.sum(dim=(1, 2)).to(sq.dtype) - float(p.P), min=1.0)
        AtA = dense_train.assemble_differentiable(self, level_index, R, T, wc)[0]
        m = ops.ba_marginals_diff(p, AtA, damping=damping, sigma2=sigma2, want=want)
        dv = m.depth_var.reshape(p.B, int(p.c.H), int(p.c.W)) if m.depth_var is not None else None
        as_t = lambda v: v if (v is None or torch.is_tensor(v)) else torch.full((p.B,), float(v), dtype=torch.float32, device=p.device)
        return DenseMarginals(m.pose_cov, dv, m.wfactor, m.logdet, m.status, as_t(sigma2), as_t(damping))

    transfer_eps = 1e-6    # transfer_depth: weight = covered / (depth_var + transfer_eps)

    def transfer_depth(self, level_index, state, new_depth, new_basis, frame=0, depth_var=None, damping=1e-3):
        """Carry the solved depth of level `level_index` over to a new key frame: target frame `frame` of the window.
          1. ops.depth_reproject at `state` (an LmState): the key frame's depth + basis . Wc in frame `frame`'s pixel grid, z-buffered;
          2. weights: 1 on the covered texels (index >= 0), 0 elsewhere; with depth_var [B,H,W] (DenseBA.marginals(...).depth_var, the
             variance per key-frame pixel) covered / (depth_var gathered by index + transfer_eps);
          3. ops.basis_fit of that map on the new key frame's new_depth [B,H,W] and new_basis [B,H,W,K'] (the level's H, W), damped.
        -> DepthTransfer(Wc [B,K'] = the new key frame's coefficients, depth_map [B,H,W], index [B,H,W] int32, covered [B] = the number
        of covered texels, status [B] int32 as ops.basis_fit).  Five launches plus the weights' torch plumbing; no host sync and no
        autograd (the result is detached from any graph)."""
        p = self.problems[level_index]
        B, H, W = p.B, int(p.c.H), int(p.c.W)
        if not 0 <= int(frame) < p.pairs:
            raise ops.capi.BanetError("DenseBA.transfer_depth: frame %d of a window with %d target frames" % (frame, p.pairs))
        if not (new_depth.is_cuda and new_basis.is_cuda) or (depth_var is not None and not depth_var.is_cuda):
            raise ops.capi.BanetError("banet_amd runs on the GPU only")
        if new_depth.numel() != B * H * W or new_basis.dim() != 4 or new_basis.numel() != B * H * W * new_basis.shape[-1]:
            raise ops.capi.BanetError("DenseBA.transfer_depth: expected new_depth [B,H,W] and new_basis [B,H,W,K'] at the level's %d x %d" % (H, W))
        with torch.no_grad():
            rep = ops.depth_reproject(p, state.R, state.T, state.Wc if self.K > 0 else None)
            depth_map, index = rep.depth[:, frame].contiguous(), rep.index[:, frame].contiguous()
            hit = index >= 0
            weight = hit.to(torch.float32)
            if depth_var is not None:
                if depth_var.numel() != B * H * W:
                    raise ops.capi.BanetError("DenseBA.transfer_depth: depth_var must be [B,H,W]")
                var = torch.gather(depth_var.detach().reshape(B, H * W).float(), 1, index.reshape(B, H * W).clamp(min=0).long())
                weight = weight / (var.reshape(B, H, W) + self.transfer_eps)
            fit = ops.basis_fit(new_depth.detach().reshape(B, H * W), new_basis.detach().reshape(B, H * W, -1), depth_map.reshape(B, H * W),
                                weight=weight.reshape(B, H * W), damping=damping)
            return DepthTransfer(fit.Wc, depth_map, index, hit.reshape(B, -1).sum(dim=1), fit.status)

    def transfer_prior(self, level_index, state, new_depth, new_basis, frame=0, depth_var=None, damping=1e-3):
        """transfer_depth, and what the transferred depth says about the new key frame's coefficients as a prior for the next window's
        solve: the same three steps (the fit's optional outputs do not change its bits) ->
        (DepthTransfer, DensePrior(coef=(fit.normal, fit.rhs), level_scale)) with level_scale[l] = N_l / N_level_index over THIS
        solver's levels, so that the term keeps its weight next to a feature term that grows with the pixel count.  The next window's
        DenseBA (same pyramid, the new key frame's depth and basis) takes it as solve(prior=...), from Wc = the transfer's."""
        p = self.problems[level_index]
        B, H, W = p.B, int(p.c.H), int(p.c.W)
        if not 0 <= int(frame) < p.pairs:
            raise ops.capi.BanetError("DenseBA.transfer_prior: frame %d of a window with %d target frames" % (frame, p.pairs))
        if not (new_depth.is_cuda and new_basis.is_cuda) or (depth_var is not None and not depth_var.is_cuda):
            raise ops.capi.BanetError("banet_amd runs on the GPU only")
        if new_depth.numel() != B * H * W or new_basis.dim() != 4 or new_basis.numel() != B * H * W * new_basis.shape[-1]:
            raise ops.capi.BanetError("DenseBA.transfer_prior: expected new_depth [B,H,W] and new_basis [B,H,W,K'] at the level's %d x %d" % (H, W))
        with torch.no_grad():
            rep = ops.depth_reproject(p, state.R, state.T, state.Wc if self.K > 0 else None)
            depth_map, index = rep.depth[:, frame].contiguous(), rep.index[:, frame].contiguous()
            hit = index >= 0
            weight = hit.to(torch.float32)
            if depth_var is not None:
                if depth_var.numel() != B * H * W:
                    raise ops.capi.BanetError("DenseBA.transfer_prior: depth_var must be [B,H,W]")
                var = torch.gather(depth_var.detach().reshape(B, H * W).float(), 1, index.reshape(B, H * W).clamp(min=0).long())
                weight = weight / (var.reshape(B, H, W) + self.transfer_eps)
            fit = ops.basis_fit(new_depth.detach().reshape(B, H * W), new_basis.detach().reshape(B, H * W, -1), depth_map.reshape(B, H * W),
                                weight=weight.reshape(B, H * W), damping=damping, want=("Wc", "normal", "rhs"))
            scales = [q.N / float(p.N) for q in self.problems]
            return (DepthTransfer(fit.Wc, depth_map, index, hit.reshape(B, -1).sum(dim=1), fit.status),
                    DensePrior(coef=(fit.normal, fit.rhs), level_scale=scales))

    def pose_prior(self, level_index, state, process_noise=None, sigma2=None, damping=0.0):
        """What this window's solve says about its poses, as a prior for a solve that shares them: marginals(level_index, state) ->
        DensePrior(pose=(R0, T0, Lambda), level_scale) with (R0, T0) = the state's poses (copies), Lambda = (pose_cov + Q)^-1 --
        the 6 pairs x 6 pairs inverse in torch, float64, cast to float32 -- and level_scale[l] = N_l / N_level_index as
        transfer_prior.  process_noise Q: None, a number (Q = q I), a tensor [6 pairs] (a diagonal), [6 pairs, 6 pairs] or
        [B, 6 pairs, 6 pairs], in the left tangent [w; t] per target frame.  sigma2 / damping: passed to marginals; the default
        sigma2 = None leaves pose_cov in the units of the normal equations, which is what the solve adds Lambda to.  The next
        DenseBA (same pyramid and target frames) takes it as solve(prior=...)."""
        p = self.problems[level_index]
        m = 6 * p.pairs
        with torch.no_grad():
            cov = self.marginals(level_index, state, damping=damping, sigma2=sigma2, want=("pose_cov",)).pose_cov.double()
            if process_noise is not None:
                q = torch.as_tensor(process_noise, dtype=torch.float64, device=cov.device)
                if q.dim() == 0:
                    q = q * torch.eye(m, dtype=torch.float64, device=cov.device)
                elif q.dim() == 1:
                    q = torch.diag(q)
                if q.shape[-2:] != (m, m):
                    raise ops.capi.BanetError("DenseBA.pose_prior: process_noise must be a number, [%d], [%d,%d] or [B,%d,%d]" % (m, m, m, m, m))
                cov = cov + q
            Lam = torch.linalg.inv(0.5 * (cov + cov.transpose(1, 2)))
            Lam = (0.5 * (Lam + Lam.transpose(1, 2))).float().contiguous()
            R0 = state.R.detach().clone().reshape(p.B, p.pairs, 3, 3)
            T0 = state.T.detach().clone().reshape(p.B, p.pairs, 3)
        return DensePrior(pose=(R0, T0, Lam), level_scale=[q_.N / float(p.N) for q_ in self.problems])

    def cost_trace(self, snapshots, state0=None):
        """Did each level reduce the cost?  snapshots: what solve(snapshots=...) filled; state0: the state that solve started from
        (default: new_state()).  -> [n_levels, 2, B, pairs, 4]: the sums (sum sq, sum ab, in-image count, max sq) of level l's
        maps BEFORE that level (the state after level l - 1) and AFTER it.  Two launches per evaluation, no host sync."""
        st0 = state0 if state0 is not None else self.new_state()
        n = len(snapshots)
        out = torch.empty((n, 2, self.B, self.pairs, 4), dtype=torch.float32, device=self.intr.device)
        R, T, W = st0.R, st0.T, st0.Wc
        for l, snap in enumerate(snapshots):
            p = self.problems[l]
            for k, (r_, t_, w_) in enumerate(((R, T, W), (snap["R"], snap["T"], snap["W"]))):
                ops.ba_residual(p, r_, t_, w_ if self.K > 0 else None, sums=out[l, k])
            R, T, W = snap["R"], snap["T"], snap["W"]
        return out

    def algorithmic_bytes_per_iteration(self, level_index):
        """4*N_l*(C*F + K + 1) per window-iteration (F = 1 + pairs frames)."""
        p = self.problems[level_index]
        return 4 * p.N * (p.C * (1 + p.pairs) + p.K + 1)
