"""The yardstick of the shading pass (tests/shade_ref.py) against itself on every case of tests/shade_cases.py, without a GPU:
the integer edge values sum to |area2|; its flat, wire-less image is render_ref's image; the wire ties really are ties, in
integers; no case puts more than 0.5 % of its covered pixels within 1e-4 of a rounding boundary (the cap the GPU test may use
for its one-LSB allowance); the normals cases reach the arm they are named for; and the two entry points are declared in
include/p2m.h and bound in _lib.py."""
import os
import re

import numpy as np
import pytest

import render_cases as rc
import render_ref as rr
import shade_cases as sc
import shade_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR_CAP = 0.005


def _pixels(c, fid, mid):
    """Per covered pixel of a buffer the yardstick's rasteriser wrote: (area2, A, Bc, E)."""
    out = []
    xy = np.stack([rr.project(c["verts"][b], c["cam"][b], c["H"], c["W"])["xy"] for b in range(c["verts"].shape[0])])
    for k in range(fid.shape[0]):
        ii, jj = np.nonzero(fid[k] >= 0)
        tri = c["faces"][fid[k][ii, jj]]
        P = xy[mid[k][ii, jj][:, None], tri]
        area2, s, A, Bc, E = sr.edges_at(P, tri, jj.astype(np.int64) * 256 + 128, ii.astype(np.int64) * 256 + 128)
        out.append((ii, jj, area2, A, Bc, E))
    return out


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_edge_values_sum_to_the_area_and_weights_to_one(name):
    s = sc.case(name)
    fid, mid = sc.visibility(s["c"])
    assert (fid >= 0).sum() > 0, name
    for ii, jj, area2, A, Bc, E in _pixels(s["c"], fid, mid):
        assert (E >= 0).all() and (E.sum(1) == np.abs(area2)).all(), name
    ref = sc.reference(name)
    cov = ref["covered"]
    assert np.array_equal(cov, fid >= 0) and not ref["status"].any()
    assert np.abs(ref["bary"][cov].astype(np.float64).sum(1) - 1.0).max() <= 3 * 2.0 ** -23
    assert (ref["bary"][~cov] == 0).all()
    if s["attrs"] is not None:
        assert (ref["attr"][~cov] == np.float32(s["attr_fill"])).all()


def test_identity_attributes_are_the_barycentrics():
    ref = sc.reference("tri16")
    cov = ref["covered"]
    assert cov.sum() > 40 and np.array_equal(ref["attr"][cov], ref["bary"][cov])


@pytest.mark.parametrize("name", sc.PLAIN_RENDER_CASES)
def test_plain_image_is_render_refs(name):
    c = rc.case(name)
    ims = rr.render_case_exact(c)
    fid, mid = np.stack([im["face_id"] for im in ims]), np.stack([im["mesh_id"] for im in ims])
    got = sr.shade(c, fid, mid)
    assert np.array_equal(got["image"], np.stack([im["image"] for im in ims])), name
    assert np.array_equal(got["v"], np.stack([im["v"] for im in ims]), equal_nan=True), name


def test_wire_ties_are_ties():
    c = sc.case("wire_tie")["c"]
    fid, mid = sc.visibility(c)
    (ii, jj, area2, A, Bc, E), = _pixels(c, fid, mid)
    T = sc.TIE_T
    tie = np.zeros(len(ii), bool)
    for p in range(len(ii)):
        lhs = [int(E[p, k]) ** 2 for k in range(3)]
        rhs = [T * T * (int(A[p, k]) ** 2 + int(Bc[p, k]) ** 2) for k in range(3)]
        less = [(T - 1) ** 2 * (int(A[p, k]) ** 2 + int(Bc[p, k]) ** 2) for k in range(3)]
        # on the wire by equality alone: no edge strictly inside T, and every edge outside T - 1
        tie[p] = any(l == r for l, r in zip(lhs, rhs)) and all(l > q for l, q in zip(lhs, less))
    # the column of centres 1.5 pixel from the edge x = 2, and the row 1.5 pixel from the edge y = 2
    assert (jj[tie] == 3).sum() >= 5 and ((jj[tie] == 3) | (ii[tie] == 3)).all()
    on, off, only = sc.reference("wire_tie"), sc.reference("wire_tie_minus"), sc.reference("wire_only")
    assert on["wire"][0][ii[tie], jj[tie]].all() and not off["wire"][0][ii[tie], jj[tie]].any()
    assert (on["image"][0][ii[tie], jj[tie]] == np.array(sc.WIRE_RGB, np.uint8)).all()
    assert on["wire"].sum() == off["wire"].sum() + tie.sum()
    assert not sc.reference("wire_off")["wire"].any()
    plain = sr.shade(c, fid, mid)
    assert np.array_equal(sc.reference("wire_off")["image"], plain["image"])
    cov, w = only["covered"], only["wire"]
    assert np.array_equal(w, on["wire"]) and (cov & ~w).sum() > 10
    assert (only["image"][cov & ~w] == c["background"][None][cov & ~w]).all()


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_few_values_near_a_rounding_boundary(name):
    ref = sc.reference(name)
    v = ref["v"]
    shaded = ~np.isnan(v).any(-1)
    with np.errstate(invalid="ignore"):
        near = (np.abs(v - np.rint(v)) < sr.NEAR).any(-1) & shaded
    assert near.sum() <= NEAR_CAP * ref["covered"].sum(), (name, int(near.sum()), int(ref["covered"].sum()))


def test_cases_reach_their_arms():
    # the mirrored camera flips the facing; without culling back faces are visible
    s = sc.case("hull_nocull_smooth_col")
    c = s["c"]
    fid, mid = sc.visibility(c)
    assert rr.project(c["verts"][1], c["cam"][1], 64, 64)["mirror"] and not rr.project(c["verts"][0], c["cam"][0], 64, 64)["mirror"]
    for (ii, jj, area2, A, Bc, E), b in zip(_pixels(c, fid, mid), range(3)):
        back = (area2 < 0) if b == 1 else (area2 > 0)
        assert back.any() and (~back).any(), b
    fid_c, _ = sc.visibility(sc.case("hull_cull_smooth_col")["c"])
    for (ii, jj, area2, A, Bc, E), b in zip(_pixels(sc.case("hull_cull_smooth_col")["c"], fid_c, _), range(3)):
        assert not ((area2 < 0) if b == 1 else (area2 > 0)).any(), b
    # smooth differs from flat, vertex colours from mesh colours
    assert (sc.reference("hull_cull_smooth_col")["image"] != sc.reference("hull_cull_flat_col")["image"]).mean() > 0.05
    assert (sc.reference("hull_cull_flat_vcol")["image"] != sc.reference("hull_cull_flat_col")["image"]).mean() > 0.05
    # the scene shows both meshes, and the later one over the earlier
    _, mid = sc.visibility(sc.case("scene_two")["c"])
    assert (mid == 0).sum() > 100 and (mid == 1).sum() > 100
    assert sc.visibility(sc.case("edge_1x1")["c"])[0][0, 0, 0] >= 0
    assert sc.reference("edge_17x33")["wire"].sum() > 20


@pytest.mark.parametrize("name", sc.NORMALS_NAMES)
def test_normals_cases(name):
    n = sc.normals_case(name)
    nv = n["verts"].shape[1]
    for b in range(n["verts"].shape[0]):
        nr, st = sr.vertex_normals(n["verts"][b], n["faces"], n["ptr"], n["idx"])
        assert st == n["status"], (name, b, st)
        zero = np.zeros(nv, bool)
        zero[n["zero"]] = True
        assert (nr[zero] == 0).all() and (np.abs((nr[~zero].astype(np.float64) ** 2).sum(1) - 1) < 1e-6).all(), name
    if name == "hull_b3":                        # outward on a convex hull around the origin; the busiest vertex is in
        nr, _ = sr.vertex_normals(n["verts"][0], n["faces"], n["ptr"], n["idx"])
        assert ((nr * n["verts"][0]).sum(1) > 0).all()
        assert np.diff(n["ptr"]).max() >= 7 and np.diff(n["ptr"]).sum() == 3 * len(n["faces"])
    if name == "zero_area":
        good = sc.normals_case("hull_b3")
        nr, _ = sr.vertex_normals(n["verts"][0], n["faces"], n["ptr"], n["idx"])
        ng, _ = sr.vertex_normals(n["verts"][0], good["faces"], good["ptr"], good["idx"])
        assert np.array_equal(nr, ng) and len(n["idx"]) == len(good["idx"]) + 2


def test_table_of_the_package_is_the_yardsticks():
    from pose2mesh_release_amd import render
    _, f = rc.hull(sc.HULL_NV)
    t = render.vertex_face_table(f, sc.HULL_NV)
    ptr, idx = sr.vertex_face_table(f, sc.HULL_NV)
    assert np.array_equal(t.ptr_host, ptr) and np.array_equal(t.idx_host, idx)


def test_entry_points_are_declared_and_bound():
    from pose2mesh_release_amd import _lib
    header = open(os.path.join(ROOT, "include", "p2m.h")).read()
    for sym in ("p2m_vertex_normals", "p2m_mesh_shade"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in _lib.HIP_SYMBOLS, sym
    from pose2mesh_release_amd import build
    assert "shade.hip" in build.HIP_SOURCES and "-ffp-contract=off" in build.HIP_SOURCE_FLAGS["shade.hip"]
