"""-m gpu: the 2D pose overlay on the GPU (p2m_pose_overlay; overlay.PoseOverlay) against the exact-integer yardstick
(tests/overlay_ref.py) on the case table of tests/overlay_cases.py.  The contract is integer, so there is no tolerance anywhere:
dst and status must equal the yardstick on every byte.  Through the C ABI with every output pre-filled inside guard regions and
src / dst pushed 0, 1 and 2 bytes off alignment, then through PoseOverlay, which must agree bit for bit; in place against out of
place, alpha 0, reproducibility, batch independence, graph capture with poses changed in place, status = NULL and the refusals."""
import ctypes as ct

import numpy as np
import pytest
import torch

import overlay_cases as oc
import overlay_ref as orf

pytestmark = pytest.mark.gpu

GUARD = 256
ERR = -1                                                       # P2M_ERR_INVALID


class Guarded:
    """A device array of `shape` inside a buffer with GUARD sentinel elements on both sides, everything pre-filled; offset:
    elements by which the array is pushed off its 16-byte boundary."""

    def __init__(self, shape, dtype, fill, offset=0, data=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD + offset,), fill, dtype=dtype, device="cuda")
        self.lo = GUARD + offset
        self.view = self.buf[self.lo:self.lo + n].view(*shape)
        self.fill = fill
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data)))

    def ptr(self):
        return ct.c_void_p(self.view.data_ptr())

    def untouched(self, t):
        return bool((t == self.fill).all())

    def guards_ok(self):
        return self.untouched(self.buf[:self.lo]) and self.untouched(self.buf[self.lo + self.view.numel():])


def _p(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


def _stream():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pack(c3):
    return int(c3[0]) | int(c3[1]) << 8 | int(c3[2]) << 16


def abi_overlay(c, expect_rc=0, in_place=False, off_src=0, off_dst=0, want_status=True, ws_cut=0, ws_shift=0, null=(), **over):
    """p2m_pose_overlay on a case dict -> (rc, dst, status, src after the call, guarded buffers).  over: arguments handed to the
    entry in place of the case's (B, P, J, C, L, H, W, ... : the buffers keep the case's sizes)."""
    from pose2mesh_release_amd import _lib
    lib = _lib.hip()
    poses = torch.from_numpy(c["poses"]).cuda()
    B, P, J, C = c["poses"].shape
    L, H, W = c["bones"].shape[0], c["H"], c["W"]
    bones = torch.from_numpy(c["bones"]).cuda() if L else None
    colours = torch.from_numpy(c["colours"]).cuda() if c["colours"].size else None
    boxes = None if c["boxes"] is None else torch.from_numpy(c["boxes"]).cuda()
    src = Guarded((B, H, W, 3), torch.uint8, 0x5A, off_src, data=c["src"])
    dst = src if in_place else Guarded((B, H, W, 3), torch.uint8, 0xA5, off_dst)
    status = Guarded((B, P), torch.int32, -77)
    nb = ct.c_int64(-1)
    rcw = lib.p2m_pose_overlay_workspace(B, P, L, 0 if boxes is None else 1, ct.byref(nb))
    assert rcw == 0 and nb.value > 0
    ws = Guarded(((nb.value + 15) // 16 + 1, 2), torch.int64, 0x2B2B2B2B2B2B2B2B)            # 16-byte elements: stays aligned
    a = dict(poses=_p(poses), B=B, P=P, J=J, C=C, bones=_p(bones), L=L, colours=_p(colours), colour_mode=c["colour_mode"],
             boxes=_p(boxes), box_rgb=_pack(c["box_rgb"]), src=src.ptr(), dst=dst.ptr(), H=H, W=W, thr=float(c["thr"]),
             line_h2=c["line_h2"], mark_h2=c["mark_h2"], mark_r16=c["mark_r16"], box_h2=c["box_h2"], alpha256=c["alpha256"],
             status=status.ptr() if want_status else None, workspace=ct.c_void_p(ws.view.data_ptr() + ws_shift),
             workspace_bytes=nb.value - ws_cut, stream=_stream())
    a.update(over)
    for k in null:
        a[k] = None
    rc_ = lib.p2m_pose_overlay(*a.values())
    torch.cuda.synchronize()
    assert rc_ == expect_rc, (rc_, lib.p2m_last_error_string())
    g = dict(src=src, dst=dst, status=status, ws=ws)
    assert all(x.guards_ok() for x in g.values()), "a guard region was written"
    return rc_, dst.view.cpu().numpy(), status.view.cpu().numpy(), src.view.cpu().numpy(), g


def overlay_for(c):
    from pose2mesh_release_amd import overlay
    mark = ("disc", c["mark_h2"] // 2) if c["mark_r16"] < 0 else ("ring", c["mark_r16"] // 16, c["mark_h2"])
    assert (c["mark_r16"] < 0 and c["mark_h2"] % 2 == 0) or c["mark_r16"] % 16 == 0
    return overlay.PoseOverlay(c["bones"], c["H"], c["W"], line=c["line_h2"], mark=mark, thr=c["thr"],
                               colours=c["colours"] if c["colour_mode"] == 0 else None, box_colour=c["box_rgb"], box=c["box_h2"])


def run_class(c, o=None, out=None, image=None):
    o = o or overlay_for(c)
    image = torch.from_numpy(c["src"]).cuda() if image is None else image
    res = o(image, torch.from_numpy(c["poses"]).cuda(),
            colours=torch.from_numpy(c["colours"]).cuda() if c["colour_mode"] == 1 else None,
            boxes=None if c["boxes"] is None else torch.from_numpy(c["boxes"]).cuda(), alpha=c["alpha256"] / 256.0, out=out)
    return o, res, image


@pytest.mark.parametrize("name", oc.CASE_NAMES)
def test_case_table(hip_libs, name):
    """C ABI out of place and in place, and PoseOverlay, against the yardstick: every byte of dst, every status word."""
    c, ref = oc.case(name), oc.reference(name)
    _, dst, st, src_after, g = abi_overlay(c)
    bad = int((dst != ref["dst"]).sum())
    print(f"{name}: {bad} differing bytes of {dst.size}")
    assert bad == 0, (name, bad, np.argwhere((dst != ref["dst"]).any(-1))[:5].tolist())
    assert np.array_equal(st, ref["status"]), (name, st.tolist())
    assert np.array_equal(src_after, c["src"]), "src was written"
    _, dst2, st2, _, _ = abi_overlay(c, in_place=True)
    assert np.array_equal(dst2, ref["dst"]) and np.array_equal(st2, ref["status"]), name
    _, res, image = run_class(c)
    assert res["image"] is image and res["image"].dtype == torch.uint8 and res["status"].dtype == torch.int32
    assert np.array_equal(res["image"].cpu().numpy(), ref["dst"]) and np.array_equal(res["status"].cpu().numpy(), ref["status"])


@pytest.mark.parametrize("name", ["geometry_63x65", "geometry_65x63", "far_ends_130x70", "two_chunks", "invisible", "one_pixel"])
@pytest.mark.parametrize("off_src,off_dst", [(1, 0), (0, 2), (3, 1), (2, 2)])
def test_rows_at_every_byte_phase(hip_libs, name, off_src, off_dst):
    """src and dst pushed off alignment: the 4-byte path must fall back to bytes where a lane's 12 bytes are not aligned."""
    c, ref = oc.case(name), oc.reference(name)
    _, dst, st, _, _ = abi_overlay(c, off_src=off_src, off_dst=off_dst)
    assert np.array_equal(dst, ref["dst"]) and np.array_equal(st, ref["status"])
    _, dst, _, _, _ = abi_overlay(c, in_place=True, off_src=off_src)
    assert np.array_equal(dst, ref["dst"])


def test_class_out_of_place_and_buffers_reused(hip_libs):
    c, ref = oc.case("batch_3"), oc.reference("batch_3")
    out = torch.full(c["src"].shape, 7, dtype=torch.uint8, device="cuda")
    o, res, image = run_class(c, out=out)
    assert res["image"] is out and np.array_equal(out.cpu().numpy(), ref["dst"])
    assert np.array_equal(image.cpu().numpy(), c["src"])
    ws, st = o._bufs[(3, 2, True)]["ws"].data_ptr(), res["status"].data_ptr()
    _, res2, _ = run_class(c, o=o)
    assert o._bufs[(3, 2, True)]["ws"].data_ptr() == ws and res2["status"].data_ptr() == st and len(o._bufs) == 1
    assert np.array_equal(res2["image"].cpu().numpy(), ref["dst"])


def test_presets_on_the_device(hip_libs):
    """keypoints() and coco_skeleton() draw what the yardstick draws with the reference's numbers; host colours are staged."""
    from pose2mesh_release_amd import overlay
    c = oc.case("two_chunks")
    k = overlay.PoseOverlay.keypoints(c["bones"], c["H"], c["W"])
    img = torch.from_numpy(c["src"]).cuda()
    res = k(img, torch.from_numpy(c["poses"]).cuda(), boxes=torch.from_numpy(c["boxes"]).cuda())
    want = orf.overlay_case(dict(c, colours=overlay.rainbow_colours(19), colour_mode=0, thr=0.4, line_h2=2, mark_h2=6,
                                 mark_r16=-1, box_h2=1, box_rgb=(255, 255, 0), alpha256=256))
    assert np.array_equal(res["image"].cpu().numpy(), want["dst"])
    s = overlay.PoseOverlay.coco_skeleton(c["bones"], c["H"], c["W"])
    img = torch.from_numpy(c["src"]).cuda()
    res = s(img, torch.from_numpy(c["poses"][..., :2].copy()).cuda(), colours=(10, 200, 90), alpha=0.5)
    col = np.broadcast_to(np.array([10, 200, 90], np.uint8), (1, 5, 3))
    want = orf.overlay_case(dict(c, poses=c["poses"][..., :2], boxes=None, colours=col, colour_mode=1, line_h2=2, mark_h2=3,
                                 mark_r16=32, alpha256=128))
    assert np.array_equal(res["image"].cpu().numpy(), want["dst"])
    with pytest.raises(ValueError):
        s(img, torch.from_numpy(c["poses"]).cuda())                                   # one colour per person: none given


def test_alpha_zero_leaves_src_bitwise(hip_libs):
    c = oc.case("alpha_0")
    for kw in (dict(), dict(in_place=True), dict(off_src=1, off_dst=3)):
        _, dst, _, _, _ = abi_overlay(c, **kw)
        assert np.array_equal(dst, c["src"]), kw


def test_repeatable_and_batch_independent(hip_libs):
    """Two runs are bitwise equal; image b of B = 3 gives the pixels and status it gives alone."""
    c = oc.case("batch_3")
    _, a, sa, _, _ = abi_overlay(c)
    _, b, sb, _, _ = abi_overlay(c)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)
    for k in range(3):
        alone = dict(c, poses=np.ascontiguousarray(c["poses"][k:k + 1]), boxes=np.ascontiguousarray(c["boxes"][k:k + 1]),
                     colours=np.ascontiguousarray(c["colours"][k:k + 1]), src=np.ascontiguousarray(c["src"][k:k + 1]))
        _, one, so, _, _ = abi_overlay(alone)
        assert np.array_equal(one[0], a[k]) and np.array_equal(so[0], sa[k]), k


def test_graph_capture_follows_the_poses(hip_libs):
    """A captured call replayed after the poses changed in place draws the new poses."""
    c = oc.case("two_chunks")
    o = overlay_for(c)
    poses, boxes = torch.from_numpy(c["poses"]).cuda(), torch.from_numpy(c["boxes"]).cuda()
    src = torch.from_numpy(c["src"]).cuda()
    out = torch.zeros_like(src)
    o(src, poses, boxes=boxes, out=out)                        # the first call of the shape allocates: outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = o(src, poses, boxes=boxes, out=out)
    moved = c["poses"].copy()
    moved[..., 0] = c["W"] - moved[..., 0]
    moved[0, 2, 5, 1] = np.nan
    poses.copy_(torch.from_numpy(moved))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = orf.overlay_case(dict(c, poses=moved))
    assert np.array_equal(res["image"].cpu().numpy(), want["dst"]) and want["status"][0, 2] == 1
    assert np.array_equal(res["status"].cpu().numpy(), want["status"])
    assert not np.array_equal(want["dst"], oc.reference("two_chunks")["dst"])


def test_status_may_be_null(hip_libs):
    c, ref = oc.case("unusable"), oc.reference("unusable")
    _, dst, _, _, g = abi_overlay(c, want_status=False)
    assert np.array_equal(dst, ref["dst"]) and g["status"].untouched(g["status"].view)


def test_bone_index_out_of_range_is_never_followed(hip_libs):
    """The entry cannot see device bones; the kernels must not follow a bad index (that bone draws nothing) and PoseOverlay
    refuses it on the host."""
    c = oc.case("revisit")
    bad = dict(c, bones=np.array([[0, 1], [0, 4], [-1, 2], [1 << 30, 0], [2, 2]], np.int32))
    good = dict(c, bones=np.array([[0, 1], [2, 2]], np.int32), colours=c["colours"][[0, 4]])
    _, dst, _, _, _ = abi_overlay(bad)
    assert np.array_equal(dst, orf.overlay_case(good)["dst"])
    with pytest.raises(ValueError):
        run_class(dict(bad, bones=bad["bones"][:2], colours=c["colours"][:2]))


def test_refusals(hip_libs):
    """Every refusal of the header's list returns P2M_ERR_INVALID and launches nothing: dst and status keep their fill."""
    from pose2mesh_release_amd import _lib
    lib = _lib.hip()
    c = oc.case("batch_3")
    big = 1 << 31
    cases = [dict(null=("poses",)), dict(null=("src",)), dict(null=("dst",)), dict(null=("workspace",)), dict(null=("bones",)),
             dict(null=("colours",)), dict(H=0), dict(H=8193), dict(W=0), dict(W=8193), dict(J=0), dict(J=65), dict(P=0),
             dict(P=65), dict(L=-1), dict(L=65), dict(L=0, null=("boxes",)), dict(C=1), dict(C=4), dict(line_h2=-1),
             dict(line_h2=65), dict(mark_h2=65), dict(box_h2=-1), dict(box_h2=65), dict(mark_r16=-2), dict(mark_r16=1025),
             dict(alpha256=-1), dict(alpha256=257), dict(colour_mode=2), dict(colour_mode=-1), dict(B=-1),
             dict(B=big // (64 * 196) + 1, P=64, L=64), dict(ws_cut=1), dict(ws_shift=8), dict(ws_shift=4)]
    for kw in cases:
        _, _, _, _, g = abi_overlay(c, expect_rc=ERR, **kw)
        assert g["dst"].untouched(g["dst"].view) and g["status"].untouched(g["status"].view), kw
        assert g["ws"].untouched(g["ws"].view), kw
        assert lib.p2m_last_error_string(), kw
    n = ct.c_int64(-5)
    for args in ((1, 0, 1, 0), (1, 65, 1, 0), (1, 1, 65, 0), (1, 1, 0, 0), (-1, 1, 1, 0), (big // (64 * 196) + 1, 64, 64, 1)):
        assert lib.p2m_pose_overlay_workspace(*args, ct.byref(n)) == ERR and n.value == -5, args
    assert lib.p2m_pose_overlay_workspace(1, 1, 0, 1, ct.byref(n)) == 0 and n.value >= 4 * 24
    assert lib.p2m_pose_overlay_workspace(1, 1, 1, 1, None) == ERR
    _, dst, _, _, _ = abi_overlay(c, B=0)                      # B = 0 is a no-op
    assert (dst == 0xA5).all()


def test_class_refusals(hip_libs):
    from pose2mesh_release_amd import _lib
    c = oc.case("revisit")
    o = overlay_for(c)
    img, poses = torch.from_numpy(c["src"]).cuda(), torch.from_numpy(c["poses"]).cuda()
    for args, kw in (((img.cpu(), poses), {}), ((img, poses.cpu()), {}), ((img, poses), dict(out=img.cpu())),
                     ((img, poses), dict(boxes=torch.zeros(1, 1, 4, 2)))):
        with pytest.raises(_lib.P2MError):
            o(*args, **kw)
    for args, kw in (((img.float(), poses), {}), ((img[:, :, :-1], poses), {}), ((img, poses[..., :1]), {}),
                     ((img, poses), dict(alpha=1.5)), ((img, poses), dict(out=torch.zeros(1, 2, 2, 3, dtype=torch.uint8).cuda())),
                     ((img, poses), dict(boxes=torch.zeros(1, 2, 4, 2).cuda())),
                     ((img, poses), dict(colours=torch.zeros(1, 2, 3, dtype=torch.uint8).cuda())),
                     ((img.transpose(1, 2), poses), {})):
        with pytest.raises(ValueError):
            o(*args, **kw)
    assert np.array_equal(img.cpu().numpy(), c["src"])
