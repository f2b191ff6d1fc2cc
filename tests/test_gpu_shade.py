"""-m gpu: the shading pass on the GPU (p2m_vertex_normals, p2m_mesh_shade; render.vertex_normals, render.MeshShader) against
its numpy yardstick (tests/shade_ref.py) on the case table of tests/shade_cases.py.  The visibility buffer is an INPUT: the
device's own face_id / mesh_id (or a hand-made one) and the device's own snapped coordinates are fed to both the kernel and the
yardstick, so no pixel is left out of any comparison.  normals, bary and attr_out must equal the yardstick's bit for bit, wire
membership on every pixel; the image equals the yardstick's with 1 LSB allowed only where the yardstick's float64 value before
rounding is within 1e-4 of an integer (test_gpu_render.py's rule and constant), on at most 0.5 % of the covered pixels (the cap
tests/test_shade_cpu.py holds the yardstick to); background pixels are bitwise the background; a flat, wire-less image is
p2m_mesh_render's own, with no allowance.  Through the C ABI with every output pre-filled inside guard regions, and through
MeshShader, which must agree bit for bit.  Then reproducibility, batch independence, in-place images, the optional outputs,
graph capture and the refusals."""
import ctypes as ct

import numpy as np
import pytest
import torch

import render_cases as rc
import shade_cases as sc
import shade_ref as sr
import test_gpu_render as tg
from test_gpu_render import Guarded, _p, _stream

pytestmark = pytest.mark.gpu

NEAR_CAP = 0.005
ERR = -1                                                           # P2M_ERR_INVALID


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def abi_normals(n, expect_rc=0, **over):
    """p2m_vertex_normals on a normals case -> (normals [B, nv, 3], status [B], guarded outputs)."""
    from pose2mesh_release_amd import _lib
    lib = _lib.hip()
    v = torch.from_numpy(n["verts"]).cuda()
    faces = torch.from_numpy(np.ascontiguousarray(n["faces"], np.int32)).cuda()
    ptr, idx = torch.from_numpy(n["ptr"]).cuda(), torch.from_numpy(n["idx"]).cuda()
    B, nv = v.shape[:2]
    out, st = Guarded((B, nv, 3), torch.float32, float("nan")), Guarded((B,), torch.int32, -77)
    a = dict(B=B, nv=nv, nf=faces.shape[0], n_idx=idx.numel(), normals=out.ptr(), verts=_p(v))
    a.update(over)
    rc_ = lib.p2m_vertex_normals(a["verts"], _p(faces), _p(ptr), _p(idx), a["n_idx"], a["B"], a["nv"], a["nf"], a["normals"],
                                 st.ptr(), _stream())
    torch.cuda.synchronize()
    assert rc_ == expect_rc, (rc_, lib.p2m_last_error_string())
    assert out.guards_ok() and st.guards_ok()
    return out.view.cpu().numpy(), st.view.cpu().numpy(), (out, st)


def device_normals(c):
    """The device's vertex normals of a render case's meshes, asserted bit for bit the yardstick's."""
    ptr, idx = sr.vertex_face_table(c["faces"], c["verts"].shape[1])
    got, st, _ = abi_normals(dict(verts=c["verts"], faces=c["faces"], ptr=ptr, idx=idx))
    assert same_bits(got, sc.normals_of(c)) and not st.any()
    return got


def _dev(a, off=0):
    """A device copy of a numpy array, `off` elements behind a 16-byte boundary."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    room = torch.zeros(t.numel() + off, dtype=t.dtype, device="cuda")
    room[off:] = t.reshape(-1)
    return room[off:].view(t.shape)


def abi_shade(s, fid, mid, normals_np=None, want=("image", "bary", "attr", "status"), expect_rc=0, off=0, image_over=None, **over):
    """p2m_mesh_shade on a shading case and a visibility buffer, outputs guarded and pre-filled -> (dict of numpy results,
    guarded).  off: elements by which every output (the image: 4 bytes) and the two id planes start behind a 16-byte boundary.
    over: arguments replaced by name (for the refusals)."""
    from pose2mesh_release_amd import _lib
    lib = _lib.hip()
    c = s["c"]
    v, cam = torch.from_numpy(c["verts"]).cuda(), torch.from_numpy(c["cam"]).cuda()
    faces = torch.from_numpy(np.ascontiguousarray(c["faces"], np.int32)).cuda()
    B, nv = v.shape[:2]
    nf, H, W = faces.shape[0], c["H"], c["W"]
    scene = c["mode"] == "scene"
    n = 1 if scene else B
    vc = s["vertex_colours"]
    col = None if vc is not None else torch.from_numpy(c["colours"]).cuda()
    vcol = _dev(vc)
    nrm, att = _dev(normals_np), _dev(s["attrs"])
    C = 0 if s["attrs"] is None else s["attrs"].shape[2]
    bg = _dev(c["background"])
    per = 1 if bg is not None and bg.dim() == 4 else 0
    f_d, m_d = _dev(np.asarray(fid, np.int32), off), _dev(np.asarray(mid, np.int32), off)
    g = {"image": Guarded((n, H, W, 3), torch.uint8, 0x5A, 4 * off),
         "bary": Guarded((n, H, W, 3), torch.float32, float("nan"), off),
         "attr": Guarded((n, H, W, max(C, 1)), torch.float32, float("nan"), off),
         "status": Guarded((B,), torch.int32, -77)}
    li = np.asarray(c["lights"], np.float32).reshape(-1)
    lights = (ct.c_float * max(1, li.size))(*li.tolist())
    T, rgb, only = s["wire"] if s["wire"] is not None else (0, (0, 0, 0), False)
    wire_rgb = (ct.c_uint8 * 3)(*rgb)
    a = dict(face_id=_p(f_d), mesh_id=_p(m_d), verts=_p(v), faces=_p(faces), nf=nf, cam=_p(cam), colours=_p(col), vcol=_p(vcol),
             shared=1 if vc is not None and vc.ndim == 2 else 0, normals=_p(nrm), lights=lights, nl=li.size // 4,
             ambient=float(c["ambient"]), attrs=_p(att), C=C, wire_T=int(T), wire_rgb=wire_rgb, wire_only=int(only), bg=_p(bg),
             per=per, fill=float(s["attr_fill"]), B=B, nv=nv, H=H, W=W, mode=1 if scene else 0,
             image=(g["image"].ptr() if image_over is None else _p(image_over)) if "image" in want else None,
             bary=g["bary"].ptr() if "bary" in want else None,
             attr=g["attr"].ptr() if "attr" in want and C else None,
             status=g["status"].ptr() if "status" in want else None)
    a.update(over)
    rc_ = lib.p2m_mesh_shade(a["face_id"], a["mesh_id"], a["verts"], a["faces"], a["nf"], a["cam"], a["colours"], a["vcol"],
                             a["shared"], a["normals"], a["lights"], a["nl"], a["ambient"], a["attrs"], a["C"], a["wire_T"],
                             a["wire_rgb"], a["wire_only"], a["bg"], a["per"], a["fill"], a["B"], a["nv"], a["H"], a["W"],
                             a["mode"], a["image"], a["bary"], a["attr"], a["status"], _stream())
    torch.cuda.synchronize()
    assert rc_ == expect_rc, (rc_, lib.p2m_last_error_string())
    assert all(x.guards_ok() for x in g.values()), "a guard region was written"
    res = {k: x.view.cpu().numpy() for k, x in g.items()}
    if image_over is not None:
        res["image"] = image_over.cpu().numpy()
    return res, g


def check_against(out, ref, s, what):
    """The comparison of the module docstring for one call; returns the number of pixels that used the one-LSB allowance."""
    c = s["c"]
    cov = ref["covered"]
    assert same_bits(out["bary"], ref["bary"]), (what, "bary", int((bits(out["bary"]) != bits(ref["bary"])).sum()))
    if s["attrs"] is not None:
        assert same_bits(out["attr"], ref["attr"]), (what, "attr", int((bits(out["attr"]) != bits(ref["attr"])).sum()))
    assert np.array_equal(out["status"], ref["status"]), (what, out["status"], ref["status"])
    got, want = out["image"].astype(np.int32), ref["image"].astype(np.int32)
    diff = np.abs(got - want)
    with np.errstate(invalid="ignore"):
        near = np.abs(ref["v"] - np.rint(ref["v"])) < sr.NEAR         # (NaN where nothing was shaded: False)
    assert (diff <= np.where(near, 1, 0)).all(), (what, int(diff.max()), int((diff > np.where(near, 1, 0)).sum()))
    used = int((diff > 0).any(-1).sum())
    assert used <= NEAR_CAP * cov.sum(), (what, used)
    shaded = ~np.isnan(ref["v"]).any(-1)
    n, H, W = cov.shape
    bg = c["background"]
    bgk = np.zeros((n, H, W, 3), np.uint8) if bg is None else np.broadcast_to(bg if bg.ndim == 4 else bg[None], (n, H, W, 3))
    rest = ~shaded & ~ref["wire"]                                     # the background and, with wire_only, the pixels off the wire
    assert (out["image"][rest] == bgk[rest]).all(), what
    if s["wire"] is not None and s["wire"][0] > 0:                     # wire membership, on every pixel
        is_wire = (out["image"] == np.array(s["wire"][1], np.uint8)).all(-1)
        assert np.array_equal(is_wire & cov, ref["wire"]), (what, int((is_wire & cov).sum()), int(ref["wire"].sum()))
    print(f"{what}: {int(cov.sum())} covered pixels, {used} within the one-LSB allowance")
    return used


def device_inputs(s):
    """(xy_fix, face_id, mesh_id, normals or None, the rasteriser's outputs) of a shading case, all the device's own."""
    c = s["c"]
    xy, _ = tg.abi_project(c)
    _, ren, _ = tg.abi_render(c)
    nrm = device_normals(c) if s["smooth"] else None
    return xy, ren["face_id"], ren["mesh_id"], nrm, ren


def reference_for(s, xy, fid, mid, nrm):
    """The yardstick fed the device's buffer, snapped coordinates and (already compared) normals."""
    return sr.shade(s["c"], fid, mid, vertex_colours=s["vertex_colours"], normals=nrm, attrs=s["attrs"], wire=s["wire"],
                    attr_fill=s["attr_fill"], xy_fix=xy)


def shader_for(s, r, **kw):
    from pose2mesh_release_amd import render
    w = s["wire"]
    wire = None if w is None or w[0] == 0 else (w[0] / 256.0, w[1], w[2])
    return render.MeshShader(r, smooth=s["smooth"], wire=wire, attr_fill=s["attr_fill"], **kw)


def run_class(s, in_place=True):
    c = s["c"]
    r, out = tg.run_class(c)
    sh = shader_for(s, r)
    kw = dict(vertex_colours=torch.from_numpy(s["vertex_colours"]).cuda()) if s["vertex_colours"] is not None else \
        dict(colours=torch.from_numpy(c["colours"]).cuda())
    res = sh(out, torch.from_numpy(c["verts"]).cuda(), torch.from_numpy(c["cam"]).cuda(),
             attributes=None if s["attrs"] is None else torch.from_numpy(s["attrs"]).cuda(),
             background=None if c["background"] is None else torch.from_numpy(c["background"]).cuda(), bary=True,
             in_place=in_place, **kw)
    return r, sh, out, res


@pytest.mark.parametrize("name", sc.NORMALS_NAMES)
def test_normals(hip_libs, name):
    n = sc.normals_case(name)
    got, st, _ = abi_normals(n)
    for b in range(n["verts"].shape[0]):
        want, ws = sr.vertex_normals(n["verts"][b], n["faces"], n["ptr"], n["idx"])
        assert same_bits(got[b], want), (name, b, int((bits(got[b]) != bits(want)).sum()))
        assert st[b] == ws == n["status"], (name, b, st[b], ws)
        assert (got[b][n["zero"]] == 0).all()
    if name == "hull_b3":                                            # the class, with a table and with plain faces
        from pose2mesh_release_amd import render
        v = torch.from_numpy(n["verts"]).cuda()
        for faces in (n["faces"], render.vertex_face_table(n["faces"], n["verts"].shape[1])):
            nr, s2 = render.vertex_normals(v, faces)
            assert same_bits(nr.cpu().numpy(), got) and not s2.any()


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_case_table(hip_libs, name):
    s = sc.case(name)
    xy, fid, mid, nrm, ren = device_inputs(s)
    ref = reference_for(s, xy, fid, mid, nrm)
    out, _ = abi_shade(s, fid, mid, nrm)
    check_against(out, ref, s, name)
    assert np.array_equal(ref["covered"], fid >= 0)
    if name == "tri16":
        assert same_bits(out["attr"][ref["covered"]], out["bary"][ref["covered"]])
    # the class: in place over the renderer's own image, bit for bit the C ABI's result
    r, sh, rout, res = run_class(s)
    assert res["image"].data_ptr() == rout["image"].data_ptr()
    assert np.array_equal(res["image"].cpu().numpy(), out["image"]), name
    assert same_bits(res["bary"].cpu().numpy(), out["bary"]) and np.array_equal(res["status"].cpu().numpy(), out["status"])
    if s["attrs"] is not None:
        assert same_bits(res["attributes"].cpu().numpy(), out["attr"])
    if s["smooth"]:
        assert same_bits(res["normals"].cpu().numpy(), nrm) and not res["normals_status"].any()


@pytest.mark.parametrize("name", sc.PLAIN_RENDER_CASES)
def test_plain_image_is_the_rasterisers(hip_libs, name):
    c = rc.case(name)
    _, ren, _ = tg.abi_render(c)
    out, _ = abi_shade(sc._shade(name, c), ren["face_id"], ren["mesh_id"], want=("image", "status"))
    assert np.array_equal(out["image"], ren["image"]), (name, int((out["image"] != ren["image"]).sum()))
    assert (ren["face_id"] >= 0).sum() > 0 and not out["status"].any()


def test_outputs_off_16_byte_alignment(hip_libs):
    """Every output and both id planes 4 bytes behind a 16-byte boundary (W = 64: the 16-byte loads and dword stores must give
    way where the base does not allow them) give what the aligned call gives."""
    for name in ("edge_65x64", "edge_17x33"):
        s = sc.case(name)
        xy, fid, mid, nrm, _ = device_inputs(s)
        a, _ = abi_shade(s, fid, mid, nrm)
        b, _ = abi_shade(s, fid, mid, nrm, off=1)
        assert np.array_equal(a["image"], b["image"]) and same_bits(a["bary"], b["bary"]) and same_bits(a["attr"], b["attr"])


@pytest.mark.parametrize("kind", ["all_background", "bad_ids"])
def test_hand_made_buffers(hip_libs, kind):
    """Buffers no rasteriser wrote: ids that name no face or no mesh are background, set status bit 1 of mesh 0 and are never used
    as an index (the guard regions and the yardstick's values hold)."""
    s = sc.case("hull_nocull_smooth_vcol")
    c = s["c"]
    fid, mid = sc.hand_made(c)[kind]
    xy, _ = tg.abi_project(c)
    nrm = device_normals(c)
    ref = reference_for(s, xy, fid, mid, nrm)
    out, _ = abi_shade(s, fid, mid, nrm)
    check_against(out, ref, s, kind)
    if kind == "all_background":
        assert np.array_equal(out["image"], c["background"]) and (out["attr"] == np.float32(s["attr_fill"])).all()
        assert (out["bary"] == 0).all() and not out["status"].any()
    else:
        assert out["status"].tolist() == [2, 0, 0] and ref["covered"].sum() == 2
        assert (out["image"][0, 0, :3] == c["background"][0, 0, :3]).all()


def test_repeatable_and_batch_independent(hip_libs):
    """Two runs are bitwise equal; mesh 1 of B = 3 gives the normals and the pixels it gives alone at B = 1."""
    s = sc.case("hull_nocull_smooth_vcol")
    c = s["c"]
    xy, fid, mid, nrm, _ = device_inputs(s)
    a, _ = abi_shade(s, fid, mid, nrm)
    b, _ = abi_shade(s, fid, mid, nrm)
    assert np.array_equal(a["image"], b["image"]) and same_bits(a["bary"], b["bary"]) and same_bits(a["attr"], b["attr"])
    alone = dict(c, verts=c["verts"][1:2], cam=c["cam"][1:2], colours=c["colours"][1:2], background=c["background"][1:2])
    s1 = dict(s, c=alone, vertex_colours=s["vertex_colours"][1:2], attrs=s["attrs"][1:2])
    ptr, idx = sr.vertex_face_table(c["faces"], sc.HULL_NV)
    nrm1, _, _ = abi_normals(dict(verts=alone["verts"], faces=c["faces"], ptr=ptr, idx=idx))
    assert same_bits(nrm1, nrm[1:2])
    _, ren1, _ = tg.abi_render(alone)
    assert np.array_equal(ren1["face_id"], fid[1:2])
    one, _ = abi_shade(s1, ren1["face_id"], ren1["mesh_id"], nrm1)
    assert np.array_equal(one["image"], a["image"][1:2]) and same_bits(one["bary"], a["bary"][1:2])
    assert same_bits(one["attr"], a["attr"][1:2])


def test_image_in_place_over_the_rasterisers(hip_libs):
    """image may be the buffer p2m_mesh_render wrote: the pass never reads it."""
    s = sc.case("hull_cull_smooth_vcolshared")
    xy, fid, mid, nrm, ren = device_inputs(s)
    sep, _ = abi_shade(s, fid, mid, nrm)
    buf = torch.from_numpy(ren["image"].copy()).cuda()
    inp, _ = abi_shade(s, fid, mid, nrm, image_over=buf)
    assert np.array_equal(inp["image"], sep["image"]) and (inp["image"] != ren["image"]).any()
    r, sh, rout, res = run_class(s, in_place=False)                  # and the class can leave the renderer's image alone
    assert res["image"].data_ptr() != rout["image"].data_ptr()
    assert np.array_equal(res["image"].cpu().numpy(), sep["image"]) and np.array_equal(rout["image"].cpu().numpy(), ren["image"])


def test_optional_outputs(hip_libs):
    """Every output pointer may be NULL; the others are the same and nothing else is written."""
    s = sc.case("hull_nocull_smooth_vcol")
    xy, fid, mid, nrm, _ = device_inputs(s)
    full, _ = abi_shade(s, fid, mid, nrm)
    for k in ("image", "bary", "attr", "status"):
        rest = tuple(o for o in ("image", "bary", "attr", "status") if o != k)
        part, g = abi_shade(s, fid, mid, nrm, want=rest)
        assert g[k].untouched(g[k].view), k
        for o in rest:
            assert np.array_equal(part[o], full[o], equal_nan=True), (k, o)
    # an image needs no attributes, and bary alone no colours
    part, _ = abi_shade(dict(s, attrs=None), fid, mid, nrm, want=("image",))
    assert np.array_equal(part["image"], full["image"])
    part, _ = abi_shade(dict(s, attrs=None), fid, mid, None, want=("bary",), vcol=None)
    assert same_bits(part["bary"], full["bary"])


def test_graph_capture_replays_bitwise(hip_libs):
    """One capture of render + normals + shade, replayed on new vertices, gives the eager result."""
    s = sc.case("hull_cull_smooth_vcolshared")
    c = s["c"]
    r = tg.renderer_for(c)
    sh = shader_for(s, r)
    new = torch.from_numpy((c["verts"] * np.float32(0.9) + np.float32(0.03)).astype(np.float32)).cuda()
    v, cam = torch.from_numpy(c["verts"]).cuda(), torch.from_numpy(c["cam"]).cuda()
    col, bg = torch.from_numpy(c["colours"]).cuda(), torch.from_numpy(c["background"]).cuda()
    vc, att = torch.from_numpy(s["vertex_colours"]).cuda(), torch.from_numpy(sc._attrs(c, 3, 1)).cuda()

    def both(verts):
        out = r(verts, cam, col, bg)
        return out, sh(out, verts, cam, vertex_colours=vc, attributes=att, background=bg, bary=True)

    out, res = both(new)
    eager = {k: t.clone() for k, t in res.items()}
    eager_id = out["face_id"].clone()
    old_image = both(v)[1]["image"].clone()
    assert not torch.equal(old_image, eager["image"])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, res = both(v)
    v.copy_(new)
    for t in list(res.values()) + [out["face_id"]]:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k, t in eager.items():
        assert torch.equal(res[k].view(torch.uint8), t.view(torch.uint8)), k
    assert torch.equal(out["face_id"], eager_id) and (out["face_id"] >= 0).any()


def test_refusals(hip_libs):
    """CPU tensors raise; every refusal of include/p2m.h returns P2M_ERR_INVALID and launches nothing: the pre-filled outputs stay
    untouched."""
    from pose2mesh_release_amd import _lib, render
    lib = _lib.hip()
    s = sc.case("hull_nocull_smooth_vcol")
    c = s["c"]
    xy, fid, mid, nrm, _ = device_inputs(s)
    room = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")        # (larger than any output of the case)
    odd = ct.c_void_p(room.data_ptr() + 2)
    colours = _p(torch.from_numpy(c["colours"]).cuda())
    five = (ct.c_float * 20)(*([0.0, 0.0, -1.0, 0.1] * 5))
    zero_light = (ct.c_float * 4)(0.0, 0.0, 0.0, 1.0)
    v_d = torch.from_numpy(c["verts"]).cuda()
    for kw in (dict(C=0), dict(C=17), dict(attrs=None), dict(wire_T=-1), dict(wire_T=(1 << 16) + 1), dict(colours=colours),
               dict(vcol=None), dict(bary=odd), dict(attr=odd), dict(verts=odd), dict(normals=odd), dict(face_id=None),
               dict(mesh_id=None), dict(verts=None), dict(faces=None), dict(cam=None), dict(lights=five, nl=5),
               dict(lights=zero_light, nl=1), dict(nf=1 << 24), dict(nf=0), dict(H=0), dict(W=8193), dict(mode=2), dict(mode=1, per=1),
               dict(B=256, mode=1), dict(wire_T=5, wire_rgb=None)):
        out, g = abi_shade(s, fid, mid, nrm, expect_rc=ERR, **kw)
        assert all(x.untouched(x.view) for x in g.values()), kw
        assert lib.p2m_last_error_string()
    # an output over an input: bary over the vertices, the image over the background.  The shared buffer has room for the whole
    # output, whatever the call makes of it
    B, H, W = c["verts"].shape[0], c["H"], c["W"]
    big = torch.zeros(B * H * W * 3, dtype=torch.float32, device="cuda")
    big[:c["verts"].size] = torch.from_numpy(c["verts"].reshape(-1)).cuda()
    before = big.clone()
    out, g = abi_shade(s, fid, mid, nrm, expect_rc=ERR, bary=_p(big), verts=_p(big))
    assert all(x.untouched(x.view) for x in g.values()) and torch.equal(big, before)
    bg_d = torch.from_numpy(c["background"]).cuda()                      # (the image's own size)
    out, g = abi_shade(s, fid, mid, nrm, expect_rc=ERR, image=_p(bg_d), bg=_p(bg_d))
    assert all(x.untouched(x.view) for x in g.values()) and np.array_equal(bg_d.cpu().numpy(), c["background"])
    # the normals
    n = sc.normals_case("hull_b3")
    for kw in (dict(nv=0), dict(nf=0), dict(B=-1), dict(n_idx=-1), dict(normals=odd), dict(verts=None), dict(B=65536)):
        _, _, g = abi_normals(n, expect_rc=ERR, **kw)
        assert all(x.untouched(x.view) for x in g), kw
    v3 = torch.from_numpy(n["verts"]).cuda()
    _, _, g = abi_normals(n, expect_rc=ERR, normals=_p(v3), verts=_p(v3))        # in place over the vertices
    assert np.array_equal(v3.cpu().numpy(), n["verts"])
    # the class
    r, rout = tg.run_class(c)
    sh = render.MeshShader(r)
    cam = torch.from_numpy(c["cam"]).cuda()
    with pytest.raises(_lib.P2MError):
        sh(rout, torch.from_numpy(c["verts"]), cam)
    with pytest.raises(_lib.P2MError):
        sh(rout, v_d, torch.from_numpy(c["cam"]))
    with pytest.raises(_lib.P2MError):
        render.vertex_normals(torch.from_numpy(c["verts"]), c["faces"])
    with pytest.raises(ValueError):
        sh(rout, v_d, cam, colours=(1, 1, 1), vertex_colours=torch.from_numpy(s["vertex_colours"]).cuda())
    with pytest.raises(ValueError):
        render.MeshShader(r, wire=(300.0, (1, 2, 3), False))
