"""-m gpu: the narrow-row kernels behind P2M_NARROW_ROWS (csrc/loss.hip k_face_terms / k_vertex_grad in the block order that keeps
a sample on one L2, csrc/basis.hip k_expand_small_rows / _tile_rows, csrc/bn.hip k_class_reduce3, csrc/weights.hip
k_conv_weights_images_tiled) against the kernels they replace, bit for bit, and against float64 where tests/loss_ref.py and
tests/basis_ref.py give a reference (at the bars of those files, through the checkers of tests/test_gpu_loss_edges.py).

The library reads the knob once per process, so each arm is one run of THIS file as a script (python test_gpu_narrow_rows.py
OUT.npz) under the arm's environment, one after the other, each under its own timeout.  The child calls the C ABI on its own
buffers: outputs are prefilled with a NaN bit pattern and lie between guard regions.
  loss          B = 1 and 3; B F and B nv no multiples of 256 (one and several blocks); the fan mesh (a vertex in no face, one in
                a single face); V0 > nv (the fake rows of grad_cam are exactly 0 and the whole of grad_cam is compared); w_edge = 0
                with a degenerate predicted edge (the arm that must not evaluate the edge term: every gradient finite); masks
                absent and present; guard words on both sides of the workspace, which has the size the query gives.
  expand        nc = 3, lde = 32 on a level whose last tile is short, B = 1, 8, 9, with and without classes: every row the
                contractions read (row sets 1 and 2 of row_set_of) is fully written and equal in both arms, within
                basis_ref.expand's bound of float64; any other row is either what knob 0 writes or untouched.
  class reduce  F = 3, B = 1, 3 and 7 (one block of k_class_reduce3, nearly a full one, three), classes of 1, 2, 3, 4 and 8 rows and
                their holes, the last class ending on the last row of a sample: both arms equal, and equal to the fp32 sums taken
                in the order k = 0 .. m-1 (plain IEEE additions: exact).
  images        (Fin, Fout) = (64, 3), (128, 64), (256, 128), (256, 256), (48, 80), both slice arithmetics: the four images with
                the f16x2 trailer as raw bytes, prefilled so that the zero padding columns are shown to be written; in bf16x3 the
                three slices of the forward image add up to W exactly.
Every figure is printed before it is asserted (pytest -rP)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import basis_ref as br                     # noqa: E402
import loss_ref as R                       # noqa: E402
import tile_plan_ref as tp                 # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF
GUARD = 4096
CHILD_TIMEOUT = 240

# ---- the cases (shared by the child and the checks) -------------------------------------------------------------------------------
W_NO_EDGE = (1.0, 0.1, 0.0, 1e-3)
# name -> (case of loss_ref.CASES, B, weights, degenerate edge)
LOSS_CASES = {
    "fan_b3": ("fan", 3, R.WEIGHTS["default"], False),            # B F = 183, B nv = 189: one partial block
    "fan_b1_noedge": ("fan", 1, W_NO_EDGE, False),
    "masks_b3": ("masks", 3, R.WEIGHTS["default"], False),        # nv = 500: several blocks, the last one partial
    "masks_b1_noedge": ("masks", 1, W_NO_EDGE, False),
    "near_gt_b3": ("near_gt", 3, R.WEIGHTS["default"], False),
    "degenerate_noedge": ("one_block", 3, W_NO_EDGE, True),       # bitwise and finite only: no float64 bar for a 0-length edge
}
EXPAND_B = (1, 8, 9)
CLASS_SIZES = (1, 2, 4, 8, 3, 1, 1, 2, 8, 4, 3)                   # the last class (3 rows) ends on the last row of a sample
N_REAL = 300                                                      # >= 256: a tile plan; 300 rows: the last tile is short
REDUCE_B = (1, 3, 7)                                              # 7: three blocks of k_class_reduce3, the last one partial
IMAGE_LAYERS = ((3, 64), (64, 128), (128, 256), (256, 256), (80, 48))      # (Fout, Fin)
IMAGE_COEF = (-0.37, 0.61)
ARITHS = ("bf16x3", "f16x2")


def loss_case(key):
    name, B, weights, degenerate = LOSS_CASES[key]
    c = dict(R.make_case(name))
    assert B <= c["B"]
    for k in ("cam", "gt_mesh", "gt_pose", "valid_mesh", "valid_pose"):
        if c[k] is not None:
            c[k] = np.ascontiguousarray(c[k][:B])
    c["B"] = B
    if degenerate:                       # corners 0 and 1 of face 0 coincide in the prediction: |p0 - p1| = 0
        f = c["faces"][0]
        c["cam"] = c["cam"].copy()
        c["cam"][:, c["perm"][f[1]]] = c["cam"][:, c["perm"][f[0]]]
    return c, weights


def level():
    """(L, V, rep_of): N_REAL real vertices (ring + chords 5 and 17) followed by the isolated fake ones in runs of CLASS_SIZES."""
    F = int(sum(CLASS_SIZES))
    V = N_REAL + F
    i = np.arange(N_REAL)
    A = tp._sym(np.concatenate([i, i, i]), np.concatenate([(i + 1) % N_REAL, (i + 5) % N_REAL, (i + 17) % N_REAL]), V)
    rep = np.arange(V, dtype=np.int32)
    at = N_REAL
    for s in CLASS_SIZES:
        rep[at:at + s] = at
        at += s
    return tp.laplacian(A, V), V, rep


def class_weights(V, rep):
    w = np.ones(V)
    for v in range(V):
        if rep[v] != v:
            w[v] = 0.0
            w[rep[v]] += 1.0
    return w


def expand_input(B, V):
    return br.inputs(8100 + B, (B, V, 3))[0]


def reduce_input(B, V):
    return br.inputs(8200 + B, (B, V, 3))[0]


def image_weight(i, Fout, Fin):
    W = (br.inputs(8300 + i, (Fout, 3 * Fin))[0] / np.sqrt(3.0 * Fin)).astype(np.float32)
    W[0, 0], W[Fout - 1, 3 * Fin - 1] = 0.0, -W[Fout - 1, 3 * Fin - 1]
    return W


# ---- the child: one arm ------------------------------------------------------------------------------------------------------------

def _child(out):
    import torch
    from pose2mesh_release_amd import _lib, loss as L, ops
    hip = _lib.hip()
    vp = ctypes.c_void_p
    res = {}

    def ptr(t):
        return None if t is None else vp(t.data_ptr())

    def st():
        return vp(torch.cuda.current_stream().cuda_stream)

    def cu(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    class Out:                            # n floats prefilled with the sentinel between two guard regions
        def __init__(self, n):
            self.n = n
            self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
            self.t = self.buf[GUARD:GUARD + n].view(torch.float32)

        def bits(self):
            torch.cuda.synchronize()
            return self.buf[GUARD:GUARD + self.n].cpu().numpy()

        def guards(self):
            return np.array([int((self.buf[:GUARD] != SENTINEL).sum()), int((self.buf[GUARD + self.n:] != SENTINEL).sum())])

    # loss
    for key in LOSS_CASES:
        c, w = loss_case(key)
        mod = L.FusedMeshLoss(c["faces"], c["perm_reverse"], c["jreg"], w_vertex=w[0], w_normal=w[1], w_edge=w[2], w_joint=w[3])
        t = mod._tensors(torch.device("cuda:0"))
        B, V0 = c["B"], c["V0"]
        cam, gm, gp = cu(c["cam"]), cu(c["gt_mesh"]), cu(c["gt_pose"])
        vm, vpose = cu(c["valid_mesh"]), cu(c["valid_pose"])
        ws = Out(int(hip.p2m_mesh_loss_workspace(B, mod.nv, mod.nf, mod.J)))
        grad, losses = Out(B * V0 * 3), Out(4)
        _lib.check(hip.p2m_mesh_loss(ptr(cam), V0, ptr(t["perm"]), mod.nv, ptr(gm), ptr(vm), ptr(t["faces"]), mod.nf,
                                     ptr(t["vf_ptr"]), ptr(t["vf_idx"]), ptr(t["jr_ptr"]), ptr(t["jr_idx"]), ptr(t["jr_val"]),
                                     ptr(t["vj_ptr"]), ptr(t["vj_idx"]), ptr(t["vj_val"]), mod.J, ptr(gp), ptr(vpose),
                                     mod.w_vertex, mod.w_normal, mod.w_edge, mod.w_joint, ptr(ws.t), ptr(losses.t), ptr(grad.t),
                                     B, st()), "p2m_mesh_loss")
        res[f"loss::{key}::losses"] = losses.bits()
        res[f"loss::{key}::grad"] = grad.bits().reshape(B, V0, 3)
        res[f"loss::{key}::guards"] = np.concatenate([ws.guards(), grad.guards(), losses.guards()])

    # expand and class reduce
    Lg, V, rep = level()
    for classes in (False, True):
        g = ops.DeviceGraph(Lg, "cuda:0")
        assert g.V == V and g.n_real == N_REAL and g.plan_tiles[0] > 0
        if classes:
            g.set_classes(rep)
            assert g.classes
        for B in EXPAND_B:
            G = cu(expand_input(B, V))
            E = Out(B * V * 32)
            _lib.check(hip.p2m_cheb_expand_small(g.handle, ptr(G), 3, ptr(E.t), 32, B, st()), "p2m_cheb_expand_small")
            res[f"expand::{int(classes)}::{B}"] = E.bits().reshape(B, V, 32)
            res[f"expand::{int(classes)}::{B}::guards"] = E.guards()
        if classes:
            for B in REDUCE_B:
                X = cu(reduce_input(B, V))
                Y = Out(B * V * 3)
                _lib.check(hip.p2m_class_reduce(g.handle, ptr(X), ptr(Y.t), B, 3, st()), "p2m_class_reduce")
                res[f"reduce::{B}"] = Y.bits().reshape(B, V, 3)
                res[f"reduce::{B}::guards"] = Y.guards()

    # weight images
    for arith in ARITHS:
        ops.GEMM_ARITH = arith
        ops.bump_weight_epoch()
        weights = [cu(image_weight(i, fo, fi)) for i, (fo, fi) in enumerate(IMAGE_LAYERS)]
        cws = ops.ConvWeightSet([(i, w, IMAGE_COEF[0], IMAGE_COEF[1]) for i, w in enumerate(weights)], "cuda:0")
        for imgs in cws.images.values():
            for im in imgs:
                im.fill_(0x5A5A)
        cws.refresh()
        torch.cuda.synchronize()
        for i in range(len(IMAGE_LAYERS)):
            for name, im in zip(("f", "ef", "b", "eb"), cws.images[i]):
                res[f"image::{arith}::{i}::{name}"] = im.cpu().numpy()
        res[f"image::{arith}::words"] = cws.words.cpu().numpy()
    np.savez(out, **res)


# ---- the checks ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def arms(hip_libs, tmp_path_factory):
    """{knob: npz of this file run as a child under P2M_NARROW_ROWS = knob}, one child after the other."""
    d = tmp_path_factory.mktemp("narrow_rows")
    res = {}
    for knob in ("0", "1"):
        out = str(d / f"arm{knob}.npz")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, P2M_NARROW_ROWS=knob),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
        assert p.returncode == 0, f"P2M_NARROW_ROWS={knob}: " + p.stdout[-3000:]
        res[knob] = np.load(out)
    assert sorted(res["0"].files) == sorted(res["1"].files)
    return res


def _same(arms, key):
    a, b = arms["0"][key], arms["1"][key]
    assert a.shape == b.shape and a.dtype == b.dtype, key
    diff = int((a != b).sum())
    print(f"  {key}: {a.size} words, {diff} differ between the arms")
    assert diff == 0, key
    return b


def _f64(bits):
    return np.ascontiguousarray(bits).view(np.float32).astype(np.float64)


@pytest.mark.parametrize("key", list(LOSS_CASES))
def test_loss(arms, key):
    import test_gpu_loss_edges as le
    c, w = loss_case(key)
    for knob in ("0", "1"):
        guards = arms[knob][f"loss::{key}::guards"]
        print(f"  P2M_NARROW_ROWS={knob}: guard words lost (workspace, grad_cam, losses; before, after) {guards.tolist()}")
        assert not guards.any(), (knob, key)
    losses = _same(arms, f"loss::{key}::losses")
    grad = _same(arms, f"loss::{key}::grad")
    assert not (grad == SENTINEL).any() and not (losses == SENTINEL).any()
    fake = np.setdiff1d(np.arange(c["V0"]), c["perm"])
    assert fake.size > 0 and not grad[:, fake].any(), "the fake rows of grad_cam are exactly 0"
    gradf, compf = _f64(grad), _f64(losses)
    assert np.isfinite(gradf).all() and np.isfinite(compf).all()
    if LOSS_CASES[key][3]:
        assert compf[2] == 0.0                   # the edge term at w_edge = 0
        return
    le._check_mesh(c, R.case_ref(c, w), compf, gradf, key)


def test_loss_cases_cover_what_they_should():
    shapes = {}
    for key in LOSS_CASES:
        c, w = loss_case(key)
        shapes[key] = (c["B"], c["B"] * c["F"], c["B"] * c["nv"], c["V0"] - c["nv"], w[2], c["valid_mesh"] is not None)
        print(f"  {key}: B, B F, B nv, V0 - nv, w_edge, masks = {shapes[key]}")
        assert (c["B"] * c["F"]) % 256 and (c["B"] * c["nv"]) % 256 and c["V0"] > c["nv"]
    assert {s[0] for s in shapes.values()} == {1, 3}
    assert any(s[1] > 256 and s[2] > 256 for s in shapes.values()) and any(s[1] < 256 for s in shapes.values())
    assert any(s[4] == 0 for s in shapes.values()) and any(s[4] != 0 for s in shapes.values())
    assert any(s[5] for s in shapes.values()) and any(not s[5] for s in shapes.values())
    faces = R.fan_faces()
    counts = np.bincount(faces.reshape(-1), minlength=63)
    assert counts[61] == 0 and counts[62] == 1 and counts[0] == 60


@pytest.mark.parametrize("classes", [0, 1])
def test_expand(arms, classes):
    Lg, V, rep = level()
    plans = tp.Plans(Lg)
    last = plans.plan[0][-1]
    print(f"  plan 0: {len(plans.plan[0])} tiles, the last one holds {last[1]} rows")
    assert 0 < last[1] < tp.RMAX
    w = class_weights(V, rep) if classes else np.ones(V)
    read = w != 0                                   # row sets 1 and 2: the real rows and the representatives
    m = br.merged(Lg)
    for B in EXPAND_B:
        key = f"expand::{classes}::{B}"
        off, on = arms["0"][key], arms["1"][key]
        for knob in ("0", "1"):
            assert not arms[knob][key + "::guards"].any(), (knob, key)
        diff = int((off[:, read] != on[:, read]).sum())
        stale = int((on[:, read] == SENTINEL).sum())
        other_on, other_off = on[:, ~read], off[:, ~read]
        untouched = (other_on == SENTINEL).all(-1)
        as_off = (other_on == other_off).all(-1)
        print(f"  {key}: {int(read.sum())} rows read downstream: {diff} words differ, {stale} not written; {int((~read).sum())} "
              f"other rows per sample: {int(untouched.sum())} untouched, {int((as_off & ~untouched).sum())} as knob 0 writes them")
        assert diff == 0 and stale == 0, key
        assert (untouched | as_off).all(), key
        ref, bound = br.expand(m, expand_input(B, V), 3, 32)
        err = np.abs(_f64(on) - ref)[:, read]
        ok = bound[:, read] > 0
        print(f"  {key}: worst error / bound {float((err[ok] / bound[:, read][ok]).max()):.3f}")
        assert (err <= bound[:, read]).all(), key


def test_class_reduce(arms):
    _, V, rep = level()
    w = class_weights(V, rep).astype(np.int64)
    print(f"  class sizes {sorted(set(w.tolist()))}, the last class: rows {int(rep[V - 1])} .. {V - 1}")
    assert {0, 1, max(CLASS_SIZES)} <= set(w.tolist()) and rep[V - 1] != V - 1
    for B in REDUCE_B:
        key = f"reduce::{B}"
        for knob in ("0", "1"):
            assert not arms[knob][key + "::guards"].any(), (knob, key)
        got = _same(arms, key)
        X = reduce_input(B, V)
        want = np.zeros((B, V, 3), np.float32)
        for v in range(V):
            s = np.zeros((B, 3), np.float32)
            for k in range(w[v]):
                s = s + X[:, v + k]
            want[:, v] = s
        assert (B * V * 3) % 4 != 0, "the last block ends in a partial 16-byte unit"
        assert np.array_equal(got, want.view(np.int32)), key


@pytest.mark.parametrize("arith", ARITHS)
def test_weight_images(arms, arith):
    _same(arms, f"image::{arith}::words")
    for i, (Fout, Fin) in enumerate(IMAGE_LAYERS):
        for name in ("f", "ef", "b", "eb"):
            im = _same(arms, f"image::{arith}::{i}::{name}")
            K = {"f": 3 * Fin, "ef": Fin, "b": 3 * Fout, "eb": Fout}[name]
            assert (im.size > 0) == (K % 16 == 0), (i, name)
            if im.size:              # every slice element was written: the prefill pattern survives only as a chance value
                body = im[:im.size - 8] if arith == "f16x2" else im
                assert float((body == 0x5A5A).mean()) < 1e-3, (i, name)
        if arith == "bf16x3":        # x = h + m + l exactly (p2m_split.h): the forward image gives W back, its padding is zero
            im = arms["1"][f"image::{arith}::{i}::f"].view(np.uint16)
            Npad = -(-Fout // 128) * 128
            sl = im.reshape(3 * Fin // 16, 3, Npad, 16).astype(np.uint32) << 16
            val = sl.view(np.float32).astype(np.float64).sum(1)                  # [k / 16][n][k % 16]
            Wt = val.transpose(0, 2, 1).reshape(3 * Fin, Npad)                   # [k][n], k = kk Fin + fin
            W = image_weight(i, Fout, Fin).astype(np.float64)
            want = W.reshape(Fout, Fin, 3).transpose(2, 1, 0).reshape(3 * Fin, Fout)
            assert np.array_equal(Wt[:, :Fout], want) and not Wt[:, Fout:].any(), i
            assert not im.reshape(3 * Fin // 16, 3, Npad, 16)[:, :, Fout:].any(), "padding columns are zero"


if __name__ == "__main__":
    _child(sys.argv[1])
