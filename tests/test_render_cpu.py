"""CPU: the renderer's yardstick (tests/render_ref.py) audited on the case table of tests/render_cases.py, without a GPU.
The properties no rasteriser may miss - a watertight convex hull is covered exactly once per interior pixel, the mask is the
union of the faces drawn one by one, a mirrored mesh gives the mirrored mask - and the conditions the GPU tests rely on: no
vertex within 1e-9 sub-pixel units of a rounding boundary, the left-out share of every case under its cap (zero where every
pixel has one fragment, 0.5 % of the covered pixels otherwise), the derived depth bound holding for an fp32 run of the
device's formula."""
import numpy as np
import pytest

import render_cases as rc
import render_ref as rr


@pytest.mark.parametrize("name", rc.CASE_NAMES)
def test_case_conditions(name):
    """Per case: no vertex in the snap margin (so xy_fix must match exactly on the GPU), the left-out share under its cap,
    and something to see."""
    c, ref = rc.case(name), rc.reference(name)
    for k, im in enumerate(ref):
        covered = im["face_id"] >= 0
        assert covered.sum() > 0, name
        assert min(float(p["margin"].min()) for p in im["proj"]) > rr.SNAP_MARGIN, name
        left = int(im["left_out"].sum())
        print(f"{name}: covered {int(covered.sum())}, left out {left}, most fragments on a pixel {int(im['count'].max())}")
        if c["single"]:
            assert left == 0 and im["count"].max() == 1, name
        else:
            assert left <= rc.LEFT_OUT_CAP * covered.sum(), name
        assert ((im["mesh_id"] >= 0) == covered).all() and np.isinf(im["depth"][~covered]).all()
        bg = c["background"]
        if bg is None:
            assert (im["image"][~covered] == 0).all()
        else:
            assert (im["image"][~covered] == (bg if bg.ndim == 3 else bg[k])[~covered]).all()


@pytest.mark.parametrize("name", rc.HULL_NAMES + ["mirror_cam"])
def test_watertight_hull_is_covered_exactly_once(name):
    """Every pixel whose centre lies inside the projected hull (by 1/64 pixel) has exactly one fragment, every pixel outside
    it (by the same margin) none: no cracks along shared edges, no double hits."""
    from scipy.spatial import ConvexHull
    c, im = rc.case(name), rc.reference(name)[0]
    p = im["proj"][0]
    pts = np.stack([p["px"], p["py"]], 1)
    eq = ConvexHull(pts).equations                              # n . x + d <= 0 inside, |n| = 1
    jj, ii = np.meshgrid(np.arange(c["W"]) + 0.5, np.arange(c["H"]) + 0.5)
    dist = (eq[:, None, None, 0] * jj + eq[:, None, None, 1] * ii + eq[:, None, None, 2]).max(0)
    inside, outside = dist < -1 / 64, dist > 1 / 64
    assert inside.sum() > 100
    assert (im["count"][inside] == 1).all() and (im["count"][outside] == 0).all() and im["count"].max() == 1


@pytest.mark.parametrize("name", ["hull64_33x47", "top_left", "top_left_flipped", "odd_faces", "tri_small"])
def test_mask_is_the_union_of_single_faces(name):
    c, im = rc.case(name), rc.reference(name)[0]
    mesh = dict(xy=im["proj"][0]["xy"], z=c["verts"][0][:, 2], mirror=False)
    union = np.zeros((c["H"], c["W"]), bool)
    total = np.zeros((c["H"], c["W"]), np.int32)
    for f in range(len(c["faces"])):
        one = rr.rasterise([mesh], c["faces"], c["H"], c["W"], c["cull"], c["z_range"], single_faces=[f])
        union |= one["face_id"] >= 0
        total += one["count"]
    assert (union == (im["face_id"] >= 0)).all() and (total == im["count"]).all()


def test_top_left_rule_on_shared_edges():
    """Shared edges through pixel centres, horizontal, vertical and both diagonals: every centre on one belongs to exactly one
    of the two faces, in both windings, and a square with corners on centres covers [x0, x1) x [y0, y1): 10 x 10 pixels."""
    a, b = rc.reference("top_left")[0], rc.reference("top_left_flipped")[0]
    assert a["on_edge"].sum() > 60 and a["count"].max() == 1 and b["count"].max() == 1
    assert (a["face_id"] == b["face_id"]).all()
    for k, x0 in ((2, 34), (3, 50)):
        sq = np.isin(a["face_id"], (2 * k, 2 * k + 1))
        assert sq.sum() == 100 and sq[2:12, x0:x0 + 10].all()
    for k in (0, 1):                                            # the kites: area 10 x 12 / 2, both halves alike
        assert np.isin(a["face_id"], (2 * k, 2 * k + 1)).sum() == 60
    # the horizontal shared edge (row 8 of quad 0): its centres belong to the face BELOW the edge (a top edge)
    row = a["face_id"][8, 3:12]
    assert (row == 1).all() and (a["face_id"][7, 7] == 0)


@pytest.mark.parametrize("name", ["hull64_64x64", "hull778_33x47", "mano_posed"])
def test_mirror_symmetry(name):
    """x -> -x in the integer domain (X -> 256 W - X) with the faces' winding reversed: the same faces cover the mirrored
    pixels, except centres exactly on an edge, where left edges become right edges."""
    c, im = rc.case(name), rc.reference(name)[0]
    xy = im["proj"][0]["xy"].copy()
    xy[:, 0] = rr.FIX * c["W"] - xy[:, 0]
    mir = rr.rasterise([dict(xy=xy, z=c["verts"][0][:, 2], mirror=False)], c["faces"][:, [0, 2, 1]], c["H"], c["W"], c["cull"],
                       c["z_range"])
    ok = ~(im["on_edge"] | mir["on_edge"][:, ::-1] | im["left_out"] | mir["left_out"][:, ::-1])
    assert ok.sum() > 0.9 * ok.size
    assert (mir["face_id"][:, ::-1] == im["face_id"])[ok].all()
    cov = ok & (im["face_id"] >= 0)                           # (the reversed winding swaps the two terms of the plane sum)
    assert np.abs(mir["depth"][:, ::-1][cov] - im["depth"][cov]).max() < 1e-12


def test_scene_orders():
    """List order: the last mesh paints over the others wherever it has a fragment; depth order: the nearest wins; reversing
    the list changes the list-order picture and not the depth-order one."""
    li, de, rev = (rc.reference(n)[0] for n in ("scene_list", "scene_depth", "scene_list_rev"))
    c = rc.case("scene_list")
    alone = [rr.render_case(dict(c, mode="batch"))[b] for b in range(3)]
    m2 = alone[2]["face_id"] >= 0
    assert (li["mesh_id"][m2] == 2).all() and (rev["mesh_id"][alone[0]["face_id"] >= 0] == 2).all()
    stack = np.stack([a["depth"] for a in alone])
    assert (de["mesh_id"] == np.where(np.isinf(stack.min(0)), -1, stack.argmin(0))).all()
    assert (de["depth"] == stack.min(0)).all()
    assert (li["mesh_id"] != de["mesh_id"]).sum() > 50


def test_crop_cam_to_image():
    """crop_cam_to_image sends a point to the same original-image pixel as the crop's camera followed by the bbox's inverse
    affine (the crop is the h x h square about the bbox centre, run.py:34-41), and restates the reference's arithmetic."""
    from pose2mesh_release_amd import render
    rng = np.random.default_rng(0)
    cam = np.stack([rng.uniform(0.5, 1.5, 5), rng.uniform(-0.3, 0.3, 5), rng.uniform(-0.3, 0.3, 5)], 1)
    bbox = np.stack([rng.uniform(0, 300, 5), rng.uniform(0, 200, 5), rng.uniform(50, 200, 5), rng.uniform(80, 250, 5)], 1)
    W, H = 640, 480
    out = render.crop_cam_to_image(cam, bbox, W, H)
    assert out.shape == (5, 4)
    pts = rng.uniform(-1, 1, (5, 7, 2))
    h = bbox[:, 3][:, None]
    cx, cy = (bbox[:, 0] + bbox[:, 2] / 2)[:, None], (bbox[:, 1] + bbox[:, 3] / 2)[:, None]
    s, tx, ty = (cam[:, k][:, None] for k in range(3))
    crop_x, crop_y = h / 2 * (1 + s * (pts[..., 0] + tx)), h / 2 * (1 + s * (pts[..., 1] + ty))
    want_x, want_y = crop_x + cx - h / 2, crop_y + cy - h / 2
    sx, sy, ox, oy = (out[:, k][:, None] for k in range(4))
    got_x, got_y = W / 2 * (1 + sx * (pts[..., 0] + ox)), H / 2 * (1 + sy * (pts[..., 1] + oy))
    assert np.abs(got_x - want_x).max() < 1e-9 and np.abs(got_y - want_y).max() < 1e-9
    import torch
    t = render.crop_cam_to_image(torch.from_numpy(cam), torch.from_numpy(bbox), W, H)
    assert np.abs(t.numpy() - out).max() < 1e-12


def test_depth_bound_holds_for_an_fp32_run():
    """The device's depth formula run in numpy float32 (the fma as a float64 product and sum rounded once more) against the
    float64 plane value: within the derived bound, and not by orders of magnitude (the bound is not padded)."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(200):
        A = int(rng.integers(1, 1 << 40))
        E0 = rng.integers(0, A + 1, 64)
        E2 = np.minimum(rng.integers(0, A + 1, 64), A - E0)
        z = (rng.standard_normal(3) * 10.0 ** rng.uniform(-2, 2)).astype(np.float32)
        f4 = np.float32
        l1, l2 = E2.astype(f4) / f4(A), E0.astype(f4) / f4(A)
        inner = (l1.astype(np.float64) * np.float64(z[1] - z[0]) + np.float64(z[0])).astype(f4)
        d32 = (l2.astype(np.float64) * np.float64(z[2] - z[0]) + inner.astype(np.float64)).astype(f4)
        z8 = z.astype(np.float64)
        d64 = z8[0] + (E2 / float(A)) * (z8[1] - z8[0]) + (E0 / float(A)) * (z8[2] - z8[0])
        worst = max(worst, float(np.abs(d32 - d64).max() / (rr.DEPTH_ULPS * rr.U32 * np.abs(z8).max())))
    print(f"fp32 depth formula: worst error / bound {worst:.3f}")
    assert 0.02 < worst <= 1.0


def test_refused_shapes_are_python_errors_too():
    from pose2mesh_release_amd import render
    with pytest.raises(ValueError):
        render.MeshRenderer(np.array([[0, 1, 5]]), 8, 8, num_vertex=5)
    with pytest.raises(ValueError):
        render.MeshRenderer(np.zeros((0, 3), np.int64), 8, 8)
    with pytest.raises(ValueError):
        render.MeshRenderer(np.array([[0, 1, 2]]), 8, 8, mode="tiles")
