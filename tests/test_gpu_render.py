"""-m gpu: the renderer on the GPU (p2m_mesh_project, p2m_mesh_render; render.MeshRenderer) against the float64 / exact-integer
yardstick (tests/render_ref.py) on the case table of tests/render_cases.py.  xy_fix must equal the yardstick's exactly (no
vertex of a case lies in the snap margin: tests/test_render_cpu.py); face_id, mesh_id and mask must equal the yardstick FED
THE DEVICE'S xy_fix exactly on every pixel the yardstick can decide (none may be left out where every pixel has one fragment,
0.5 % of the covered pixels at most elsewhere: asserted on the CPU for the yardstick's own coordinates and here again for the
device's); depth within the derived bound; the image equal, 1 LSB allowed only where the float64 value before rounding is within
1e-4 of an integer; background pixels bitwise the background.  Through the C ABI with every output pre-filled inside guard
regions, and through MeshRenderer, which must agree bit for bit.  Then reproducibility, batch independence, graph capture, the
optional outputs and the refusals."""
import ctypes as ct

import numpy as np
import pytest
import torch

import render_cases as rc
import render_ref as rr

pytestmark = pytest.mark.gpu

GUARD = 256


class Guarded:
    """A device array of `shape` inside a buffer with GUARD sentinel elements on both sides, everything pre-filled."""

    def __init__(self, shape, dtype, fill, offset=0):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD + offset,), fill, dtype=dtype, device="cuda")
        self.lo = GUARD + offset                                # (offset: elements by which the array is pushed off 16 bytes)
        self.view = self.buf[self.lo:self.lo + n].view(*shape)
        self.fill = fill

    def ptr(self):
        return ct.c_void_p(self.view.data_ptr())

    def untouched(self, t):
        return bool(torch.isnan(t).all()) if isinstance(self.fill, float) else bool((t == self.fill).all())

    def guards_ok(self):
        return self.untouched(self.buf[:self.lo]) and self.untouched(self.buf[self.lo + self.view.numel():])


def _p(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


def _stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def abi_project(c):
    from pose2mesh_release_amd import _lib
    lib = _lib.hip()
    v, cam = torch.from_numpy(c["verts"]).cuda(), torch.from_numpy(c["cam"]).cuda()
    B, nv = v.shape[:2]
    xy, st = Guarded((B, nv, 2), torch.int32, -77777), Guarded((B,), torch.int32, -77)
    rc_ = lib.p2m_mesh_project(_p(v), _p(cam), B, nv, c["H"], c["W"], xy.ptr(), st.ptr(), _stream())
    torch.cuda.synchronize()
    assert rc_ == 0 and xy.guards_ok() and st.guards_ok()
    return xy.view.cpu().numpy(), st.view.cpu().numpy()


def abi_render(c, want=("image", "face_id", "mesh_id", "depth", "status"), expect_rc=0, offset=None, **over):
    """p2m_mesh_render on a case dict with guarded, pre-filled outputs -> (rc, dict of numpy results, guarded).  offset: {output
    name or "background": elements by which that array starts behind a 16-byte boundary}."""
    offset = offset or {}
    from pose2mesh_release_amd import _lib
    lib = _lib.hip()
    c = dict(c, **over)
    v, cam = torch.from_numpy(c["verts"]).cuda(), torch.from_numpy(c["cam"]).cuda()
    faces = torch.from_numpy(np.ascontiguousarray(c["faces"], np.int32)).cuda()
    col = torch.from_numpy(c["colours"]).cuda()
    B, nv = v.shape[:2]
    nf, H, W = int(c.get("nf", faces.shape[0])), c["H"], c["W"]
    scene = c["mode"] == "scene"
    n = 1 if scene else B
    bg = None if c["background"] is None else torch.from_numpy(c["background"]).cuda()
    if bg is not None and offset.get("background"):
        room = torch.zeros(bg.numel() + offset["background"], dtype=torch.uint8, device="cuda")
        room[offset["background"]:] = bg.reshape(-1)
        bg = room[offset["background"]:].view(bg.shape)
    per = 1 if bg is not None and bg.dim() == 4 else 0
    g = {"image": Guarded((n, max(H, 1), max(W, 1), 3), torch.uint8, 0x5A, offset.get("image", 0)),
         "face_id": Guarded((n, max(H, 1), max(W, 1)), torch.int32, -77, offset.get("face_id", 0)),
         "mesh_id": Guarded((n, max(H, 1), max(W, 1)), torch.int32, -77, offset.get("mesh_id", 0)),
         "depth": Guarded((n, max(H, 1), max(W, 1)), torch.float32, float("nan"), offset.get("depth", 0)),
         "status": Guarded((B,), torch.int32, -77)}
    nb = ct.c_int64(-1)
    rcw = lib.p2m_mesh_render_workspace(B, nf, H, W, 1 if scene else 0, ct.byref(nb))
    if expect_rc == 0:
        assert rcw == 0 and nb.value > 0
    # 16-byte elements: the guarded view stays 16-byte aligned
    ws = Guarded(((max(nb.value, 16) + 15) // 16, 2), torch.int64, 0x2B2B2B2B2B2B2B2B)
    li = np.asarray(c["lights"], np.float32).reshape(-1)
    lights = (ct.c_float * max(1, li.size))(*li.tolist())
    flags = (1 if c["cull"] else 0) | (2 if scene and c["order"] == "depth" else 0)
    flags = c.get("flags", flags)
    rc_ = lib.p2m_mesh_render(_p(v), _p(faces), nf, _p(cam), _p(col), lights, li.size // 4, float(c["ambient"]),
                              float(c["z_range"][0]), float(c["z_range"][1]), flags, _p(bg), per, B, nv, H, W, 1 if scene else 0,
                              *(g[k].ptr() if k in want else None for k in ("image", "face_id", "mesh_id", "depth", "status")),
                              ws.ptr(), _stream())
    torch.cuda.synchronize()
    assert rc_ == expect_rc, (rc_, lib.p2m_last_error_string())
    g["ws"] = ws
    assert all(x.guards_ok() for x in g.values()), "a guard region was written"
    return rc_, {k: x.view.cpu().numpy() for k, x in g.items() if k != "ws"}, g


def renderer_for(c, **kw):
    from pose2mesh_release_amd import render
    return render.MeshRenderer(c["faces"], c["H"], c["W"], mode=c["mode"], order=c["order"], cull=c["cull"], ambient=c["ambient"],
                               lights=c["lights"], z_range=c["z_range"], **kw)


def run_class(c, r=None):
    r = r or renderer_for(c)
    bg = None if c["background"] is None else torch.from_numpy(c["background"]).cuda()
    out = r(torch.from_numpy(c["verts"]).cuda(), torch.from_numpy(c["cam"]).cuda(), torch.from_numpy(c["colours"]).cuda(), bg)
    return r, out


def check_against(out, ref, c, what):
    """The comparison of the module docstring for one call.  Returns the worst depth error / bound."""
    worst = 0.0
    for k, im in enumerate(ref):
        cmp = ~im["left_out"]
        covered = im["face_id"] >= 0
        left = int(im["left_out"].sum())
        assert left == 0 if c["single"] else left <= rc.LEFT_OUT_CAP * covered.sum(), (what, k, left)
        for key in ("face_id", "mesh_id"):
            assert (out[key][k] == im[key])[cmp].all(), (what, k, key, int((out[key][k] != im[key])[cmp].sum()))
        sel = cmp & covered
        d = out["depth"][k].astype(np.float64)
        assert np.isposinf(d[cmp & ~covered]).all(), (what, k)
        if sel.any():
            err, bnd = np.abs(d[sel] - im["depth"][sel]), im["bound"][sel]
            assert (err <= bnd).all(), (what, k, float((err - bnd).max()))       # (a face at z = 0 has bound 0: exact)
            if (bnd > 0).any():
                worst = max(worst, float((err[bnd > 0] / bnd[bnd > 0]).max()))
        got, want = out["image"][k].astype(np.int32), im["image"].astype(np.int32)
        diff = np.abs(got - want)
        with np.errstate(invalid="ignore"):
            near = np.abs(im["v"] - np.rint(im["v"])) < 1e-4                  # (NaN on the background: False)
        assert (diff[cmp] <= np.where(near[cmp], 1, 0)).all(), (what, k, int(diff[cmp].max()))
        bg = c["background"]
        bgk = np.zeros_like(im["image"]) if bg is None else (bg if bg.ndim == 3 else bg[k])
        assert (out["image"][k][cmp & ~covered] == bgk[cmp & ~covered]).all(), (what, k)
    print(f"{what}: worst depth error / bound {worst:.3f}")
    return worst


def device_reference(c, name=None):
    """(xy_fix of the device - asserted equal to the yardstick's -, status, the yardstick fed with it)."""
    xy, st = abi_project(c)
    own = [rr.project(c["verts"][b], c["cam"][b], c["H"], c["W"]) for b in range(c["verts"].shape[0])]
    for b, p in enumerate(own):
        safe = p["margin"] > rr.SNAP_MARGIN
        assert (xy[b][safe] == p["xy"][safe]).all(), (name, b, int((xy[b] != p["xy"]).any(1).sum()))
        assert (st[b] & 1) == int(p["clamped"].any()), (name, b)
    same = all((xy[b] == p["xy"]).all() for b, p in enumerate(own))
    ref = rc.reference(name) if same and name is not None else rr.render_case(c, xy_fix=xy)
    return xy, st, ref


@pytest.mark.parametrize("name", rc.CASE_NAMES)
def test_case_table(hip_libs, name):
    c = rc.case(name)
    xy, st, ref = device_reference(c, name)
    _, out, _ = abi_render(c)
    check_against(out, ref, c, name)
    used = np.zeros(c["verts"].shape[1], bool)
    used[c["faces"].reshape(-1)] = True
    for b in range(c["verts"].shape[0]):                       # status of a render: clamps of the vertices its faces use
        assert out["status"][b] == int((np.abs(xy[b][used]) == rr.CLAMP).any()), (name, b)
    _, cls = run_class(c)
    for k in ("image", "face_id", "mesh_id", "depth", "status"):
        assert np.array_equal(cls[k].cpu().numpy(), out[k], equal_nan=True), (name, k)
    assert np.array_equal(cls["mask"].cpu().numpy(), out["face_id"] >= 0)
    assert cls["image"].dtype == torch.uint8 and cls["mask"].dtype == torch.bool and cls["depth"].dtype == torch.float32


def test_clamped_vertex_sets_the_status_bit(hip_libs):
    c = rc.case("clamped")
    xy, st = abi_project(c)
    assert st[0] == 1 and xy[0, 1, 0] == rr.CLAMP and (np.abs(xy[0, [0, 2, 3, 4, 5]]) < rr.CLAMP).all()
    _, out, _ = abi_render(c)
    assert out["status"][0] == 1 and (out["face_id"] == 1).sum() > 100
    nan = dict(c, verts=c["verts"].copy())
    nan["verts"][0, 1] = np.nan                                # a NaN vertex: clamped like +inf, its fragments fail the depth test
    _, out, _ = abi_render(nan)
    assert out["status"][0] == 1 and (out["face_id"] == 0).sum() == 0 and (out["face_id"] == 1).sum() > 100


def test_bad_face_index_is_reported_and_not_read(hip_libs):
    c = rc.case("tri_small")
    bad = dict(c, faces=np.array([(0, 1, 2), (0, 1, 3), (-1, 1, 2)], np.int64))
    _, out, _ = abi_render(bad)
    _, good, _ = abi_render(c)
    assert out["status"][0] == 2 and np.array_equal(out["face_id"], good["face_id"])
    with pytest.raises(ValueError):
        run_class(bad)


def test_repeatable_and_batch_independent(hip_libs):
    """Two runs are bitwise equal; mesh 2 of B = 3 gives the pixels it gives alone at B = 1."""
    c = rc.case("hull64_65x31_b3")
    _, a, _ = abi_render(c)
    _, b, _ = abi_render(c)
    alone = dict(c, verts=c["verts"][2:3], cam=c["cam"][2:3], colours=c["colours"][2:3], background=c["background"][2:3])
    _, one, _ = abi_render(alone)
    for k in ("image", "face_id", "depth"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert np.array_equal(a[k][2:3], one[k], equal_nan=True), k
    assert (a["mesh_id"][2][a["face_id"][2] >= 0] == 2).all() and (one["mesh_id"][0][one["face_id"][0] >= 0] == 0).all()
    m = rc.case("mano_posed")                                  # many fragments per pixel: the order of arrival must not show
    _, a, _ = abi_render(m)
    _, b, _ = abi_render(m)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_optional_outputs(hip_libs):
    """Every output pointer may be NULL; the others are the same."""
    c = rc.case("hull64_33x47")
    _, full, _ = abi_render(c)
    for k in ("image", "face_id", "mesh_id", "depth", "status"):
        _, part, g = abi_render(c, want=(k,))
        assert np.array_equal(part[k], full[k], equal_nan=True), k
        assert all(g[o].untouched(g[o].view) for o in full if o != k), k


def test_graph_capture_replays_bitwise(hip_libs):
    c = rc.case("scene_depth")
    r, out = run_class(c)
    eager = {k: v.clone() for k, v in out.items()}
    v, cam = torch.from_numpy(c["verts"]).cuda(), torch.from_numpy(c["cam"]).cuda()
    col, bg = torch.from_numpy(c["colours"]).cuda(), torch.from_numpy(c["background"]).cuda()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = r(v, cam, col, bg)
    for t in out.values():
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k, t in eager.items():
        assert torch.equal(out[k], t), k
    assert out["mask"].any()


def test_refusals(hip_libs):
    """CPU tensors raise; 256 meshes in scene mode, five lights, nf >= 2^24 and H or W outside [1, 8192] return
    P2M_ERR_INVALID and launch nothing: the pre-filled outputs stay untouched."""
    from pose2mesh_release_amd import _lib, render
    lib = _lib.hip()
    c = rc.case("tri_small")
    r = renderer_for(c)
    with pytest.raises(_lib.P2MError):
        r(torch.from_numpy(c["verts"]), torch.from_numpy(c["cam"]).cuda())
    with pytest.raises(_lib.P2MError):
        r(torch.from_numpy(c["verts"]).cuda(), torch.from_numpy(c["cam"]))
    with pytest.raises(_lib.P2MError):
        render.project_vertices(torch.from_numpy(c["verts"]), torch.from_numpy(c["cam"]).cuda(), 8, 8)
    five = np.tile(rc.LIGHTS, (5, 1))
    many = dict(c, verts=np.repeat(c["verts"], 256, 0), cam=np.repeat(c["cam"], 256, 0), colours=np.repeat(c["colours"], 256, 0),
                mode="scene", background=None)
    err = -1                                                   # P2M_ERR_INVALID
    for kw in (dict(lights=five), dict(nf=1 << 24), dict(H=0), dict(W=8193), dict(H=8193), dict(flags=4),
               dict(lights=np.array([[0, 0, 0, 1.0]], np.float32))):
        _, _, g = abi_render(c, expect_rc=err, **kw)
        assert all(x.untouched(x.view) for x in g.values()), kw
        assert lib.p2m_last_error_string()
    _, _, g = abi_render(many, expect_rc=err)
    assert all(x.untouched(x.view) for x in g.values())
    ok = dict(many, verts=many["verts"][:255], cam=many["cam"][:255], colours=many["colours"][:255])
    _, out, _ = abi_render(ok)                                 # 255 meshes are fine, and the last one is on top
    assert (out["mesh_id"][out["face_id"] >= 0] == 254).all()
    with pytest.raises(_lib.P2MError):
        run_class(dict(c, lights=five))
    with pytest.raises(_lib.P2MError):
        run_class(many)
    n = ct.c_int64(-5)
    assert lib.p2m_mesh_render_workspace(256, 10, 64, 64, 1, ct.byref(n)) == err and n.value == -5
    assert lib.p2m_mesh_render_workspace(256, 10, 64, 64, 0, ct.byref(n)) == 0 and n.value > 0
