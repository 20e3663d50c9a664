#!/usr/bin/env python3
"""Record the bits of ops.ba_marginals on a handful of tests/marginals_ref.py cases -> an .npz file.

tests/golden/marginals_forward_bits.npz was written by this script on an MI355X from the build BEFORE marg_factor_kernel's
factorisation was lifted into the device function it now shares with marg_grad_factor_kernel (csrc/marginals_common.hpp);
tests/test_gpu_marginals_grad.py compares the current build's outputs with it bit for bit.  Re-record only from a build whose
forward kernel is known to be the reference.

    python3 tools/record_marginals_forward_bits.py OUT.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

# (family, spec, seed): both matrix homes of the factor kernel (LDS up to P = 199, the workspace above), pairs > 1, an
# indefinite window
CASES = (("ladder", (38, 1, 32, 1e2, True, True), 0), ("ladder", (152, 4, 128, 1e4, True, True), 0),
         ("ladder", (191, 1, 185, 1e6, False, False), 0), ("ladder", (262, 1, 256, 1e2, False, True), 0),
         ("ladder", (304, 8, 256, 1e4, True, True), 1), ("indefinite", (38, 1, 32, 1e2, False, True), 0))
WF_STRIDE = (7, 5)          # wfactor is recorded at every 7th row and 5th column (K = 256: 786 KB otherwise)


def run(family, spec, seed, dev):
    """-> dict of numpy arrays: pose_cov, depth_var, wfactor (strided), logdet, status"""
    import marginals_ref as mr
    from banet_amd import _capi as capi, ops
    case = mr.make(family, spec, seed)
    t32 = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dev)

    class Bare:
        pass
    lv = Bare()
    lv.basis = t32(case["basis"])
    lv.c = capi.Level()
    lv.c.B, lv.c.N, lv.c.K, lv.c.pairs = case["B"], case["N"], case["K"], case["pairs"]
    lv.c.basis = lv.basis.data_ptr()
    m = ops.ba_marginals(lv, t32(case["AtA"]), damping=t32(case["damping"]), sigma2=t32(case["sigma2"]), want=ops.MARGINALS_OUTPUTS)
    torch.cuda.synchronize()
    out = {k: getattr(m, k).cpu().numpy() for k in ("pose_cov", "depth_var", "wfactor", "logdet", "status")}
    out["wfactor"] = np.ascontiguousarray(out["wfactor"][:, ::WF_STRIDE[0], ::WF_STRIDE[1]])
    return out


def key(family, spec, seed, name):
    import marginals_ref as mr
    return "%s/%s/seed%d/%s" % (family, mr.spec_id(spec), seed, name)


def main():
    dev = torch.device("cuda:0")
    rec = {}
    for family, spec, seed in CASES:
        for name, v in run(family, spec, seed, dev).items():
            rec[key(family, spec, seed, name)] = v
    np.savez_compressed(sys.argv[1], **rec)
    print("recorded %d arrays, %d bytes" % (len(rec), os.path.getsize(sys.argv[1])))


if __name__ == "__main__":
    main()
