"""-m gpu: k_gemm_rows_k1 (csrc/gemm_planes.hip), the whole-K kernel of the row-set contractions with one A plane and Ka <= 256 in the
slice arithmetics, against the kernel it replaces (k_gemm_planes_ws) and against float64.

The library reads P2M_ROWS_K1 once per process, so the two paths are two child processes (tests/_child_rows_k1.py, which also
holds the case table), started side by side once per module; every case runs in both, in bf16x3 and in f16x2.
  bitwise     C (all rows: the sentinel outside the set included), the statistics partials and the amax word of the two
              paths are equal bit for bit;
  values      C against gemm_ref.planes_rows_ref in float64 within gemm_ref.tol_fwd, the bound tests/test_gpu_ops.py and
              tests/test_gpu_gemm_edges.py hold the slice arithmetics to; rows outside the set keep the sentinel; the amax word
              is the largest |value stored|, exactly; the statistics within gemm_ref.TOL_STAT_* times the largest class
              weight (3: every term of a weighted sum, and its rounding, is scaled by its weight);
  dispatch    Ka = 288 and a three-plane launch start k_gemm_planes_ws under either setting, a launch inside the rule starts
              k_gemm_rows_k1 exactly when the knob is on - read from the kernel names the profiler saw in the child.
Every figure is printed before it is asserted (pytest -rP)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _child_rows_k1 as ck
import gemm_ref as gr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = np.int32(0x7FC0BEEF)


@pytest.fixture(scope="module")
def arms(hip_libs, tmp_path_factory):
    """{knob: npz of the child run under P2M_ROWS_K1 = knob}."""
    d = tmp_path_factory.mktemp("rows_k1")
    procs = {}
    for knob in ("0", "1"):
        out = str(d / f"arm{knob}.npz")
        procs[knob] = (out, subprocess.Popen([sys.executable, os.path.join(HERE, "_child_rows_k1.py"), out],
                                             env=dict(os.environ, P2M_ROWS_K1=knob), stdout=subprocess.PIPE,
                                             stderr=subprocess.STDOUT, text=True))
    res = {}
    for knob, (out, p) in procs.items():
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, f"P2M_ROWS_K1={knob}: " + log[-3000:]
        res[knob] = np.load(out)
    return res


def test_case_table_covers_what_it_should():
    for f in ck.FLAGS:
        on = sum(bool(c[f]) for c in ck.CASES)
        print(f"  {f}: on in {on} of {len(ck.CASES)} cases")
        assert 4 <= on <= len(ck.CASES) - 4, f
    assert sorted((c["Ka"], c["B"]) for c in ck.CASES if c["big"]) == [(64, 1100), (96, 300), (128, 1030)]
    for key, want in (("nset", ck.NSETS), ("Ka", ck.KAS), ("N", ck.NOUT), ("B", (1, 3))):
        for v in want:
            assert sum(c[key] == v for c in ck.CASES) >= 4, (key, v)
    pairs = {(c["Ka"], c["N"]) for c in ck.CASES}
    assert {(128, 128), (64, 32), (32, 64), (256, 256)} <= pairs, pairs
    assert any(c["stats"] and c["classes"] and c["in_act"] and (c["Ka"], c["N"]) == (128, 128) for c in ck.CASES)


def test_bitwise_equal_to_the_ring_kernel(arms):
    off, on = arms["0"], arms["1"]
    assert sorted(off.files) == sorted(on.files)
    kinds = {}
    for k in off.files:
        if k.startswith("log::"):
            continue
        if k.startswith("out::"):
            assert int(off[k][0]) == 0 and int(on[k][0]) == 0, ("rows outside the set were written", k)
        kinds[k.split("::")[0]] = kinds.get(k.split("::")[0], 0) + 1
        assert off[k].shape == on[k].shape and np.array_equal(off[k], on[k]), k
    print(f"  arrays compared bit for bit: {kinds}")
    runs = [c for c in ck.CASES for a in ck.ARITHS if a == "bf16x3" or not c["big"]]
    assert kinds["C"] == len(runs) + len(ck.DISPATCH)
    assert kinds["st"] == sum(c["stats"] for c in runs) and kinds["amax"] == sum(c["amax"] for c in runs)
    assert kinds["out"] == sum(c["big"] for c in ck.CASES)


def _f32(bits):
    return torch.from_numpy(np.ascontiguousarray(bits)).view(torch.float32)


def test_values_against_float64(arms):
    on = arms["1"]
    worst = {}

    def chk(kind, what, err, tol):
        print(f"    {what}: {kind} err {float(err):.3e}  bound {float(tol):.3e}")
        assert float(err) <= float(tol), (kind, what, float(err), float(tol))
        worst[kind] = max(worst.get(kind, 0.0), float(err) / float(tol))

    for i, case in enumerate(ck.CASES):
        inp = ck.inputs(case, 7000 + i)
        rows, Yref, stref = ck.reference(case, inp)
        what0 = f"case {i}: " + ", ".join(f"{k} {int(v)}" for k, v in case.items())
        for arith in ck.ARITHS[:1] if case["big"] else ck.ARITHS:
            what = f"{what0} [{arith}]"
            bits = on[f"C::{arith}::{i}"]
            if case["big"]:                # (the child kept the set's rows and counted the others: checked with the bits)
                Cset = _f32(bits)
            else:
                outside = np.ones(bits.shape[0], dtype=bool)
                outside[rows.numpy()] = False
                assert (bits[outside] == SENTINEL).all(), ("a row outside the set was written", what)
                Cset = _f32(bits)[rows]
            chk("value", what, (Cset.double() - Yref).abs().max(), gr.tol_fwd(Yref))
            if case["amax"]:
                assert int(on[f"amax::{arith}::{i}"][0]) == int(Cset.abs().max().view(torch.int32)), ("amax word", what)
            if case["stats"]:
                st = _f32(on[f"st::{arith}::{i}"]).double()
                wmax = 3.0 if case["classes"] else 1.0
                chk("stat sum", what, (st[:, 0] - stref[:, 0]).abs().max(), wmax * gr.TOL_STAT_SUM)
                chk("stat M2", what, (st[:, 1] - stref[:, 1]).abs().max(), wmax * gr.TOL_STAT_M2)
    for d in ck.DISPATCH:
        inp = ck.inputs(d, 7900, d["planes"])
        rows, Yref, _ = ck.reference(d, inp, d["planes"])
        chk("value", f"dispatch {d['name']}", (_f32(on["C::dispatch::" + d["name"]])[rows].double() - Yref).abs().max(),
            gr.tol_fwd(Yref))
    for kind, r in worst.items():
        print(f"  WORST {kind}: {r:.3f} of its bound")


def test_dispatch_rule_in_the_launch_log(arms):
    for knob in ("0", "1"):
        for d in ck.DISPATCH:
            names = [str(s) for s in arms[knob]["log::" + d["name"]]]
            print(f"  P2M_ROWS_K1={knob} {d['name']}: {names}")
            new = any("k_gemm_rows_k1" in s for s in names)
            old = any("k_gemm_planes_ws" in s for s in names)
            if knob == "1" and d["name"] == "inside":
                assert new and not old, (knob, d["name"], names)
            else:
                assert old and not new, (knob, d["name"], names)
