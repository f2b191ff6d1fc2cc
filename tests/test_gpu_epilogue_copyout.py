"""-m gpu: the staged 16-byte copy-out of gemm_epilogue (csrc/gemm_planes.hip, P2M_EPI_COPYOUT = 1) against the 4-byte walk (= 0), bit
for bit.  The library reads the knob once per process, so each arm is a child process; the six children are started side by side
once per module.
  row sets    the unmodified tests/_child_rows_k1.py (nset 1 .. 129, Ka 32 .. 256 and 96, N 32 .. 256, bias / addend / statistics
              / classes in every combination, launches of more than 1 000 blocks) under P2M_EPI_COPYOUT = 0 and 1: every array
              of the two files is identical - C with its sentinel rows, the statistics partials, the amax words, the count of
              rows written outside the set.  Once with P2M_ROWS_K1 = 1 (k_gemm_rows_k1) and once with 0 (the row-set forms of
              k_gemm_planes_ws);
  the rest    tests/_child_epilogue_copyout.py: three A planes, flat launches, three output planes, pair sums - identical;
  misaligned  C and the addend one float off a 16-byte boundary: the result is bitwise the aligned one in either arm, the
              sentinel words around C and the rows outside the set are intact, and the launch takes the 4-byte kernel;
  dispatch    with the knob on, the launches inside the rule start the staged instantiations (last template argument `true`),
              with it off the others - from the kernel names the profiler saw in the children.
The float64 yardstick of the new path are the existing suites (test_gpu_gemm_epilogue.py, test_gpu_rows_k1.py,
test_gpu_gemm_edges.py, the parity suites), which run under the library's default."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _child_epilogue_copyout as cc
import _child_rows_k1 as ck

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = np.int32(0x7FC0BEEF)
# (child script, P2M_ROWS_K1 or None) x P2M_EPI_COPYOUT
CHILDREN = (("_child_rows_k1.py", "1"), ("_child_rows_k1.py", "0"), ("_child_epilogue_copyout.py", None))


@pytest.fixture(scope="module")
def arms(hip_libs, tmp_path_factory):
    """{(script, P2M_ROWS_K1, P2M_EPI_COPYOUT): npz of that child}."""
    d = tmp_path_factory.mktemp("epi_copyout")
    procs = {}
    for script, k1 in CHILDREN:
        for co in ("0", "1"):
            out = str(d / f"{script[:-3]}_k{k1}_c{co}.npz")
            env = dict(os.environ, P2M_EPI_COPYOUT=co)
            if k1 is not None:
                env["P2M_ROWS_K1"] = k1
            procs[(script, k1, co)] = (out, subprocess.Popen([sys.executable, os.path.join(HERE, script), out], env=env,
                                                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    res = {}
    for key, (out, p) in procs.items():
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, f"{key}: " + log[-3000:]
        res[key] = np.load(out)
    return res


def _identical(off, on):
    """Every array but the launch logs is the same in both files -> {kind: arrays compared}."""
    assert sorted(off.files) == sorted(on.files)
    kinds = {}
    for k in off.files:
        if k.startswith("log::"):
            continue
        assert off[k].shape == on[k].shape and off[k].dtype == on[k].dtype and np.array_equal(off[k], on[k]), k
        kinds[k.split("::")[0]] = kinds.get(k.split("::")[0], 0) + 1
    return kinds


@pytest.mark.parametrize("k1", ("1", "0"))
def test_row_set_table_bitwise(arms, k1):
    off, on = arms[("_child_rows_k1.py", k1, "0")], arms[("_child_rows_k1.py", k1, "1")]
    kinds = _identical(off, on)
    print(f"  P2M_ROWS_K1={k1}: arrays compared bit for bit: {kinds}")
    runs = [c for c in ck.CASES for a in ck.ARITHS if a == "bf16x3" or not c["big"]]
    assert kinds["C"] == len(runs) + len(ck.DISPATCH)
    assert kinds["st"] == sum(c["stats"] for c in runs) and kinds["amax"] == sum(c["amax"] for c in runs)
    assert kinds["out"] == sum(c["big"] for c in ck.CASES)
    for k in on.files:
        if k.startswith("out::"):
            assert int(on[k][0]) == 0, ("rows outside the set were written", k)


def test_beyond_the_table_bitwise(arms):
    off, on = arms[("_child_epilogue_copyout.py", None, "0")], arms[("_child_epilogue_copyout.py", None, "1")]
    kinds = _identical(off, on)
    print(f"  arrays compared bit for bit: {kinds}")
    want = cc.expected_keys()
    for kind in ("C", "st", "amax", "mis", "guard"):
        assert kinds[kind] == want[kind], (kind, kinds[kind], want[kind])
    # (not vacuous: the stored results are numbers, not the prefill)
    for k in on.files:
        if k.startswith("C::flat::") or k.startswith("C::planes::") or k.startswith("C::pairs::"):
            assert not (on[k] == SENTINEL).any(), ("an element was not written", k)


@pytest.mark.parametrize("co", ("0", "1"))
def test_misaligned_bases(arms, co):
    arm = arms[("_child_epilogue_copyout.py", None, co)]
    n = 0
    for k in arm.files:
        if not (k.startswith("mis::") and k.endswith("::aligned")):
            continue
        key = k[len("mis::"):-len("::aligned")]
        a, o = arm[k], arm[f"mis::{key}::offset"]
        guard = int(arm["guard::" + key][0])
        written = int((a != SENTINEL).any(axis=1).sum())
        print(f"  P2M_EPI_COPYOUT={co} {key}: {written} of {a.shape[0]} rows written, guard words lost {guard}")
        assert a.shape == o.shape and np.array_equal(a, o), ("the misaligned result differs from the aligned one", key)
        assert guard == 0, ("sentinel words around the misaligned C were overwritten", key)
        # rows of the set are written whole, the others keep the sentinel whole (row set: B * nset of B * V rows)
        assert ((o != SENTINEL).all(axis=1) | (o == SENTINEL).all(axis=1)).all(), ("a row is written in part", key)
        assert written == (2 * cc.MIS_NSET if "rows_" in key else cc.MIS_M), (key, written)
        n += 1
    assert n == len(cc.ARITHS) * 3 * len(cc.MIS_N)


def test_dispatch_in_the_launch_logs(arms):
    def forms(names):
        names = [str(s) for s in names]
        assert names and all("k_gemm_" in s for s in names), names
        return {re.search(r"<[^<>]*,\s*(true|false)>", s).group(1) for s in names
                if "k_gemm_planes_ws" in s or "k_gemm_rows_k1" in s}

    for k1 in ("1", "0"):
        for co in ("0", "1"):
            arm = arms[("_child_rows_k1.py", k1, co)]
            for d in ck.DISPATCH:
                got = forms(arm["log::" + d["name"]])
                print(f"  P2M_ROWS_K1={k1} P2M_EPI_COPYOUT={co} {d['name']}: {[str(s) for s in arm['log::' + d['name']]]}")
                assert got == {"true" if co == "1" else "false"}, (k1, co, d["name"], got)
    for co in ("0", "1"):
        arm = arms[("_child_epilogue_copyout.py", None, co)]
        print(f"  P2M_EPI_COPYOUT={co}: aligned {[str(s) for s in arm['log::aligned']]}, offset {[str(s) for s in arm['log::offset']]}")
        assert forms(arm["log::aligned"]) == {"true" if co == "1" else "false"}
        assert forms(arm["log::offset"]) == {"false"}
