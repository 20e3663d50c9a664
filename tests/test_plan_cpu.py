"""The host-side launch plans (banet_amd/csrc/plan.hpp: plan_gather / plan_syrk / plan_assemble) pinned on the CPU.

plan.hpp is compiled with g++ (tests/native/plan_host.cpp, no ROCm) and swept over level shapes x batch sizes x policies x
CU counts x flag words; the return code and every field of GatherPlan / SyrkPlan / AsmPlan of every case go into one SHA-256
per (CU count, flags word) group, compared with tests/golden/plan_digests.json (which also keeps 8 hex digits per shape, so that a
mismatch can say where it starts).  A changed G or rows is a changed summation
tree, a changed offset is two buffers overlapping: neither may happen silently.  After a DELIBERATE change to the plans,
`python tests/test_plan_cpu.py --regenerate` rewrites the file from the current tree.

Also: the flag names of dev_flags.hpp against their Python block in banet_amd/_capi.py."""
import ctypes
import hashlib
import itertools
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_digests.json")

CUS = (64, 256, 304)
POLICIES = (0, 1, 7)                       # throughput, batch-invariant, not a policy
DENSE_HW = ((4, 4), (7, 9), (30, 20), (30, 21), (30, 40), (60, 80), (120, 160), (240, 320), (480, 640), (960, 1280))   # W = 20 / 21: the strip gather's minimum width
SPARSE_N = (1, 63, 64, 65, 1000, 4096, 100000)
KS = (0, 6, 32, 64, 128, 256)
PAIRS = (1, 2, 4, 5, 7, 8)
BS = (1, 2, 6, 8, 13, 32, 64, 256)
# the bits plan_gather / plan_syrk read, and the combinations they read together
PLAN_FLAGS = ("kDevSparseItems64", "kDevNoQuarterTiles", "kDevGenericGather", "kDevDirectGather", "kDevSyrkNoBf16x6",
              "kDevForcePatchGather", "kDevQuarterTiles", "kDevPatchPairLoop", "kDevForceStripGather", "kDevNoStripGather",
              "kDevStripRows32", "kDevStripFrameLoop", "kDevSyrkF16", "kDevForceQuadGather", "kDevSyrkThreeProducts",
              "kDevNoQuadGather", "kDevNoSyrkF16")
PLAN_FLAG_SETS = (("kDevForceStripGather", "kDevQuarterTiles"), ("kDevForceStripGather", "kDevStripRows32"),
                  ("kDevForcePatchGather", "kDevPatchPairLoop"))


def build_host_lib(out_dir):
    out = os.path.join(str(out_dir), "libplan_host.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "native", "plan_host.cpp")])
    L = ctypes.CDLL(out)
    L.banet_test_plan_fields.restype = ctypes.c_char_p
    L.banet_test_dev_flags.restype = ctypes.c_char_p
    return L


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build_host_lib(tmp_path_factory.mktemp("plan"))


def dev_flags(lib):
    """name -> value (unsigned) of every dev_flags.hpp name the host program lists"""
    return {k: int(v) for k, v in (ln.split("=") for ln in lib.banet_test_dev_flags().decode().split())}


def fields(lib):
    head, *names = lib.banet_test_plan_fields().decode().split()
    assert head == "desc_ints=11"
    return names


def sweep_levels():
    """-> (int32 [n, 10] levels without the flags column, [(chunk name, first row, last row + 1)] one chunk per shape)"""
    rows, chunks = [], []
    for H, W in DENSE_HW:
        n0 = len(rows)
        for (C, grad), K, pairs, B, policy in itertools.product(((64, 0), (127, 0), (128, 0), (128, 1)), KS, PAIRS, BS, POLICIES):
            rows.append((B, H * W, C, K, H, W, 1, grad, pairs, policy))
        chunks.append(("dense %dx%d" % (H, W), n0, len(rows)))
    for N in SPARSE_N:
        n0 = len(rows)
        for (C, grad), K, B, policy in itertools.product(((64, 1), (128, 1), (128, 0)), KS, BS, POLICIES):
            rows.append((B, N, C, K, 48, 64, 0, grad, 1, policy))
        chunks.append(("sparse N=%d" % N, n0, len(rows)))
    return np.asarray(rows, np.int32), chunks


def flag_words(flags):
    """[(label, int32 value)]: 0, every single bit the plans read, the combinations"""
    words = [("0", 0)] + [(n, flags[n]) for n in PLAN_FLAGS] + [("|".join(s), sum(flags[n] for n in s)) for s in PLAN_FLAG_SETS]
    return [(label, v - (1 << 32) if v >= (1 << 31) else v) for label, v in words]


def run_group(lib, levels, word, cus):
    desc = np.ascontiguousarray(np.concatenate([levels, np.full((len(levels), 1), word, np.int32)], axis=1))
    out = np.zeros((len(levels), len(fields(lib))), np.int64)
    lib.banet_test_plan_sweep(desc.ctypes.data_as(ctypes.c_void_p), len(levels), cus, out.ctypes.data_as(ctypes.c_void_p))
    return out


def group_record(out, chunks):
    """what the golden file keeps of a group: the digest of all its cases, and 8 hex digits per shape to find a difference by"""
    return {"sha256": hashlib.sha256(out.tobytes()).hexdigest(),
            "shapes": "".join(hashlib.sha256(out[a:b].tobytes()).hexdigest()[:8] for _, a, b in chunks)}


def all_groups(lib, cus_list=CUS):
    levels, chunks = sweep_levels()
    return {"cus=%d flags=%s" % (cus, label): group_record(run_group(lib, levels, word, cus), chunks)
            for cus in cus_list for label, word in flag_words(dev_flags(lib))}


def write_golden(lib, groups):
    levels, chunks = sweep_levels()
    doc = {"what": "tests/test_plan_cpu.py: SHA-256 over (rc, every plan field) as int64 of every case of a group; "
                   "shapes: 8 hex digits per shape chunk",
           "cases_per_group": len(levels), "fields": fields(lib), "shape_chunks": [c[0] for c in chunks]}
    with open(GOLDEN, "w") as f:             # one entry / one group per line
        f.write("{\n" + "".join(" %s: %s,\n" % (json.dumps(k), json.dumps(v)) for k, v in doc.items()) + ' "groups": {\n' +
                ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in groups.items()) + "\n }\n}\n")


def test_plans_match_the_recorded_digests(lib):
    want = json.load(open(GOLDEN))
    levels, chunks = sweep_levels()
    names = fields(lib)
    assert want["cases_per_group"] == len(levels) and want["fields"] == names and want["shape_chunks"] == [c[0] for c in chunks]
    flags = dev_flags(lib)
    seen, bad = set(), []
    for cus in CUS:
        for label, word in flag_words(flags):
            key = "cus=%d flags=%s" % (cus, label)
            seen.add(key)
            out = run_group(lib, levels, word, cus)
            got = group_record(out, chunks)
            if got == want["groups"].get(key):
                continue
            # readable failure: the group, the first shape whose cases differ, and the first case of that shape as planned now
            ws = want["groups"].get(key, {}).get("shapes", "")
            ci = next((i for i in range(len(chunks)) if got["shapes"][8 * i:8 * i + 8] != ws[8 * i:8 * i + 8]), 0)
            name, a, b = chunks[ci]
            lv = dict(zip("B N C K H W dense tgt_has_grad pairs policy".split(), levels[a].tolist()))
            bad.append("%s: first difference among the %d cases of shape `%s` (rows %d..%d); its first case %s is planned as %s"
                       % (key, b - a, name, a, b - 1, lv, dict(zip(names, out[a].tolist()))))
    assert seen == set(want["groups"]), "groups of the golden file and of the sweep differ: %s" % sorted(seen ^ set(want["groups"]))
    assert not bad, "launch plans differ from tests/golden/plan_digests.json:\n" + "\n".join(bad)


def test_plan_sweep_reaches_every_kernel_and_error(lib):
    """the sweep is worth its digests only if it visits every branch: each gather kernel, each SYRK kind, the refusal of an invalid level"""
    levels, _ = sweep_levels()
    names = fields(lib)
    col = {n: i for i, n in enumerate(names)}
    flags = dev_flags(lib)
    out = np.concatenate([run_group(lib, levels, w, 256) for _, w in flag_words(flags)])
    ok = out[out[:, col["rc"]] == 0]
    assert set(np.unique(out[:, col["rc"]]).tolist()) == {0, -1}      # (K, C <= 256 throughout: BANET_ERR_UNSUPPORTED needs a larger one)
    assert set(np.unique(ok[:, col["g.strip"]]).tolist()) == {0, 8, 16, 32}
    for f, vals in (("g.c128", {0, 1}), ("g.patch", {0, 1}), ("g.quad", {0, 1}), ("g.strip_fp", {0, 1}), ("g.pairloop", {0, 1}),
                    ("g.qshift", {0, 2}), ("g.tile_pts", {16, 64}), ("g.nbands", {1, 8}), ("s.direct", {0, 1, 2, 3}), ("s.x3", {0, 1}),
                    ("s.f16", {0, 1}), ("s.f16_standalone", {0, 1})):
        assert set(np.unique(ok[:, col[f]]).tolist()) == vals, f
    assert (ok[:, col["g.frows"]] != ok[:, col["g.rows"]]).any() and (ok[:, col["g.frows"]] == ok[:, col["g.rows"]]).any()


def test_arena_offsets(lib):
    """(through plan_assemble: every offset it hands out is a multiple of 256 and the regions do not overlap)"""
    levels, _ = sweep_levels()
    col = {n: i for i, n in enumerate(fields(lib))}
    out = run_group(lib, levels, 0, 256)
    ok = out[out[:, col["rc"]] == 0]
    for f in ("g.off_fold", "g.off_queue", "g.partial_bytes", "g.rec_bytes", "s.off_colmax", "s.off_recmax", "s.off_aux", "s.partial_bytes",
              "off_rec", "off_spart", "ws_bytes"):
        assert (ok[:, col[f]] % 256 == 0).all(), f
    assert (ok[:, col["off_rec"]] == ok[:, col["g.partial_bytes"]]).all()
    assert (ok[:, col["off_spart"]] == ok[:, col["off_rec"]] + ok[:, col["g.rec_bytes"]]).all()
    assert (ok[:, col["ws_bytes"]] == ok[:, col["off_spart"]] + ok[:, col["s.partial_bytes"]]).all()
    assert (ok[:, col["g.off_fold"]] <= ok[:, col["g.off_queue"]]).all() and (ok[:, col["g.off_queue"]] < ok[:, col["g.partial_bytes"]]).all()


def test_dev_flags_match_the_python_block(lib):
    """dev_flags.hpp <-> the DEV_* block of banet_amd/_capi.py (kDevFooBar -> DEV_FOO_BAR), and <-> the public BANET_FLAG_* bits"""
    flags = dev_flags(lib)
    hdr = open(os.path.join(ROOT, "banet_amd", "csrc", "dev_flags.hpp")).read()
    assert set(re.findall(r"^\s*(kDev\w+)\s*=", hdr, re.M)) == set(flags)        # the host program lists every name of the header
    src = open(os.path.join(ROOT, "banet_amd", "_capi.py")).read()                 # (read, not imported: _capi imports torch)
    block = {m.group(1): eval(m.group(2)) for m in re.finditer(r"^(DEV_\w+) = ([-()<\d ]+?)\s*(?:#.*)?$", src, re.M)}
    snake = lambda n: "DEV_" + re.sub(r"(?<=[a-z0-9])(?=[A-Z])", "_", n[len("kDev"):]).upper()
    assert {snake(n): v for n, v in flags.items()} == {k: v % (1 << 32) for k, v in block.items()}
    pub = open(os.path.join(ROOT, "include", "banet_hip.h")).read()
    for cname, dev in (("FORCE_PATCH_GATHER", "kDevForcePatchGather"), ("FORCE_STRIP_GATHER", "kDevForceStripGather"),
                       ("FORCE_QUAD_GATHER", "kDevForceQuadGather"), ("NO_QUAD_GATHER", "kDevNoQuadGather"),
                       ("SYRK_THREE_PRODUCTS", "kDevSyrkThreeProducts"), ("SYRK_F16", "kDevSyrkF16"), ("NO_SYRK_F16", "kDevNoSyrkF16")):
        m = re.search(r"BANET_FLAG_%s = (?:\(int\))?(1 << \d+|0x[0-9a-fA-F]+)" % cname, pub)
        assert m and eval(m.group(1)) == flags[dev], cname
    # every bit has one meaning in the plans: the only shared value is the ablation bit that BANET_ABLATE builds read differently
    by_value = {}
    for n, v in flags.items():
        by_value.setdefault(v, []).append(n)
    assert [sorted(ns) for ns in by_value.values() if len(ns) > 1] == [["kDevAblateSourceRows", "kDevSparseItems64"]]


def test_no_raw_flag_numbers_in_the_sources():
    csrc = os.path.join(ROOT, "banet_amd", "csrc")
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith((".hip", ".hpp")):
            for i, line in enumerate(open(os.path.join(csrc, fn)), 1):
                assert not re.search(r"(flags|dbg)\s*&\s*(\d|\(1)", line), "%s:%d spells a flag bit as a number: %s" % (fn, i, line.strip())


if __name__ == "__main__":
    if sys.argv[1:] != ["--regenerate"]:
        sys.exit("usage: python tests/test_plan_cpu.py --regenerate   (rewrites tests/golden/plan_digests.json from the current tree)")
    with tempfile.TemporaryDirectory() as tmp:
        L = build_host_lib(tmp)
        write_golden(L, all_groups(L))
    print("wrote", GOLDEN)
