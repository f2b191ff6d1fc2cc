"""-m gpu: the renderer held to the device-exact yardstick (render_ref.rasterise_exact: the fp32 depth formula and the 64-bit
key of include/p2m.h evaluated exactly) on the edge-case table of tests/render_edge_cases.py AND on every case of
tests/render_cases.py.  Through the C ABI with guarded, pre-filled outputs: xy_fix equal to the yardstick's; face_id and mesh_id
equal to the yardstick fed the device's xy_fix on EVERY pixel - exact ties, fragments on a clip plane, everything: no pixel is
left out; depth equal BITWISE (+inf on the background); the image by the colour rule of tests/test_gpu_render.py (equal, 1 LSB
only where the float64 value before rounding is within 1e-4 of an integer); background pixels bitwise; status as the case states.
MeshRenderer agrees bit for bit wherever it can express the case.  Then output planes off their 16-byte alignment one at a time
(the pixel-by-pixel arm of the resolve at W % 4 = 0) and a captured graph of a tie case and of the 512-face hand-over."""
import numpy as np
import pytest
import torch

import render_cases as rc
import render_edge_cases as ec
import render_ref as rr
from test_gpu_render import abi_project, abi_render, run_class

pytestmark = pytest.mark.gpu

OUTPUTS = ("image", "face_id", "mesh_id", "depth", "status")


def exact_reference(c, name):
    """(xy_fix of the device - asserted equal to the yardstick's -, project's status, the exact yardstick fed with it)."""
    xy, st = abi_project(c)
    own = [rr.project(c["verts"][b], c["cam"][b], c["H"], c["W"]) for b in range(c["verts"].shape[0])]
    for b, p in enumerate(own):
        safe = p["margin"] > rr.SNAP_MARGIN
        assert (xy[b][safe] == p["xy"][safe]).all(), (name, b, int((xy[b] != p["xy"]).any(1).sum()))
        assert (st[b] & 1) == int(p["clamped"].any()) and (st[b] & ~1) == 0, (name, b)
    same = all((xy[b] == p["xy"]).all() for b, p in enumerate(own))
    return xy, st, (ec.reference(name) if same else rr.render_case_exact(c, xy_fix=xy))


def expected_status(c, xy):
    nv = c["verts"].shape[1]
    ok = ((c["faces"] >= 0) & (c["faces"] < nv)).all(1)
    used = np.zeros(nv, bool)
    used[c["faces"][ok].reshape(-1)] = True                     # (a face with a bad index is never read)
    return [int((np.abs(xy[b][used]) == rr.CLAMP).any()) | (0 if ok.all() else 2) for b in range(c["verts"].shape[0])]


def check_exact(out, ref, c, what):
    for k, im in enumerate(ref):
        assert not im["left_out"].any()
        covered = im["face_id"] >= 0
        for key in ("face_id", "mesh_id"):
            bad = out[key][k] != im[key]
            assert not bad.any(), (what, k, key, int(bad.sum()), np.argwhere(bad)[:4].tolist(),
                                   out[key][k][bad][:4].tolist(), im[key][bad][:4].tolist())
        got, want = out["depth"][k].view(np.uint32), im["depth"].view(np.uint32)
        bad = got != want
        assert not bad.any(), (what, k, "depth", int(bad.sum()), np.argwhere(bad)[:4].tolist(),
                               out["depth"][k][bad][:4].tolist(), im["depth"][bad][:4].tolist())
        assert np.isposinf(out["depth"][k][~covered]).all(), (what, k)
        diff = np.abs(out["image"][k].astype(np.int32) - im["image"].astype(np.int32))
        with np.errstate(invalid="ignore"):
            near = np.abs(im["v"] - np.rint(im["v"])) < 1e-4                  # (NaN on the background: False)
        assert (diff <= np.where(near, 1, 0)).all(), (what, k, "image", int(diff.max()))
        bg = c["background"]
        bgk = np.zeros_like(im["image"]) if bg is None else (bg if bg.ndim == 3 else bg[k])
        assert (out["image"][k][~covered] == bgk[~covered]).all(), (what, k, "background")


@pytest.mark.parametrize("name", ec.CASE_NAMES + rc.CASE_NAMES)
def test_every_pixel_of_every_case(hip_libs, name):
    c = ec.any_case(name)
    xy, st, ref = exact_reference(c, name)
    _, out, _ = abi_render(c)
    check_exact(out, ref, c, name)
    want = expected_status(c, xy)
    assert out["status"].tolist() == want, (name, out["status"].tolist(), want)
    if c.get("arm", ("",))[0] == "status":
        assert want == c["arm"][1], (name, want)
    if name == "status_unreferenced":
        assert st[0] == 1
    if c.get("cls", True):
        _, cls = run_class(c)
        for k in OUTPUTS:
            assert np.array_equal(cls[k].cpu().numpy(), out[k], equal_nan=True), (name, k)
        assert np.array_equal(cls["mask"].cpu().numpy(), out["face_id"] >= 0)


@pytest.mark.parametrize("name", ["tie_two", "hull64_64x64", "scene_identical_list"])
def test_planes_off_their_alignment(hip_libs, name):
    """W % 4 = 0: the aligned render takes the 16-byte arm of the resolve.  Each plane in turn starts one element (the image and
    the background: one byte) behind a 16-byte boundary, which sends the call down the pixel-by-pixel arm: the same bits, and
    nothing written outside the arrays (abi_render asserts the guards)."""
    c = ec.any_case(name)
    assert c["W"] % 4 == 0 and c["background"] is not None
    _, full, _ = abi_render(c)
    assert (full["face_id"] >= 0).any() and (full["face_id"] < 0).any()
    for plane in ("face_id", "mesh_id", "depth", "image", "background"):
        _, out, g = abi_render(c, offset={plane: 1})
        if plane != "background":
            assert g[plane].view.data_ptr() % 16 == (1 if plane == "image" else 4), plane
        for k in OUTPUTS:
            assert np.array_equal(out[k], full[k], equal_nan=True), (name, plane, k)
    _, out, _ = abi_render(c, offset={"face_id": 1, "mesh_id": 2, "depth": 3, "image": 3, "background": 2})
    for k in OUTPUTS:
        assert np.array_equal(out[k], full[k], equal_nan=True), (name, "all", k)


@pytest.mark.parametrize("name", ["tie_three", "big512"])
def test_graph_replay_of_ties_and_the_full_hand_over(hip_libs, name):
    c = ec.case(name)
    r, out = run_class(c)
    eager = {k: v.clone() for k, v in out.items()}
    v, cam, col = (torch.from_numpy(c[k]).cuda() for k in ("verts", "cam", "colours"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = r(v, cam, col, None)
    for t in out.values():
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k, t in eager.items():
        assert torch.equal(out[k], t), (name, k)
    ref = ec.reference(name)[0]
    assert np.array_equal(out["face_id"][0].cpu().numpy(), ref["face_id"]) and (ref["ties"] >= 2).any()
