"""CPU: the yardstick of the 2D pose overlay (tests/overlay_ref.py) and its case table (tests/overlay_cases.py) checked against
what they stand for - the analytic coverage, the symmetries of the contract, the blend's bounds, what every case is named for -
and the host side of pose2mesh_release_amd.overlay: the rainbow palette against matplotlib, the presets' numbers, the refusals
that need no device."""
import numpy as np
import pytest

import overlay_cases as oc
import overlay_ref as orf


def test_coverage_within_a_sixteenth_of_the_analytic_value():
    """cov / 16 against clamp(h + 1/2 - dist, 0, 1) in float64 on random segments and pixels: D = floor(16 dist) differs from
    16 dist by less than 1, so the two differ by less than 1/16."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(400):
        a, b = rng.integers(-60, 120, 2), rng.integers(-60, 120, 2)
        if rng.random() < 0.1:
            b = a.copy()
        h2 = int(rng.choice([0, 1, 2, 3, 6, 17, 64]))
        qx, qy = rng.integers(-20, 100, 50).astype(np.int64), rng.integers(-20, 100, 50).astype(np.int64)
        cov = orf.coverage(qx, qy, a, b, h2, -1) / 16.0
        d, w = (b - a).astype(np.float64), np.stack([qx - a[0], qy - a[1]], 1).astype(np.float64)
        L2 = d @ d
        t = np.clip((w @ d) / L2, 0.0, 1.0) if L2 > 0 else np.zeros(len(w))
        dist = np.linalg.norm(w - t[:, None] * d[None], axis=1)
        want = np.clip(h2 / 2.0 + 0.5 - dist, 0.0, 1.0)
        worst = max(worst, float(np.abs(cov - want).max()))
    print(f"largest |cov - analytic| = {worst:.4f}")
    assert worst <= 1.0 / 16.0 + 1e-9


def test_ring_coverage_is_the_disc_distance_folded():
    qy, qx = np.meshgrid(np.arange(-5, 40, dtype=np.int64), np.arange(-5, 40, dtype=np.int64), indexing="ij")
    a = np.array([17, 16])
    D = orf.distance16(qx, qy, a, a)
    for r16, h2 in ((32, 3), (160, 2), (0, 5)):
        assert np.array_equal(orf.coverage(qx, qy, a, a, h2, r16), np.clip(8 * h2 + 8 - np.abs(D - r16), 0, 16))
    assert np.array_equal(orf.coverage(qx, qy, a, a, 5, 0), orf.coverage(qx, qy, a, a, 5, -1))
    assert orf.coverage(qx, qy, a, a, 2, 160)[16 + 5, 17 + 5] == 0 and orf.coverage(qx, qy, a, a, 2, 160)[16 + 5, 27 + 5] == 16


def test_distance_far_pixels_and_extreme_segments():
    """|c| >= 2^26 is rejected as far and is far; below that the exact value is used (checked with Python integers)."""
    import math
    rng = np.random.default_rng(1)
    for _ in range(200):
        a, b = rng.integers(-16383, 16384, 2), rng.integers(-16383, 16384, 2)
        qx, qy = rng.integers(0, 8192, 8).astype(np.int64), rng.integers(0, 8192, 8).astype(np.int64)
        D = orf.distance16(qx, qy, a, b)
        for k in range(8):
            d = (int(b[0] - a[0]), int(b[1] - a[1]))
            w = (int(qx[k] - a[0]), int(qy[k] - a[1]))
            L2, t = d[0] * d[0] + d[1] * d[1], w[0] * d[0] + w[1] * d[1]
            if L2 == 0 or t <= 0:
                num, den = w[0] ** 2 + w[1] ** 2, 1
            elif t >= L2:
                num, den = int(qx[k] - b[0]) ** 2 + int(qy[k] - b[1]) ** 2, 1
            else:
                num, den = (w[0] * d[1] - w[1] * d[0]) ** 2, L2
            exact = math.isqrt(256 * num // den)
            assert D[k] == exact or (exact >= 1544 and D[k] >= 1544), (a, b, qx[k], qy[k], D[k], exact)


def test_yardstick_is_mirror_and_transpose_symmetric():
    c = oc.case("geometry_63x65")
    ref = oc.reference("geometry_63x65")["dst"]
    H, W = c["H"], c["W"]
    t = dict(c, H=W, W=H, src=np.ascontiguousarray(c["src"].transpose(0, 2, 1, 3)),
             poses=np.ascontiguousarray(c["poses"][..., [1, 0, 2]]))
    assert np.array_equal(orf.overlay_case(t)["dst"], ref.transpose(0, 2, 1, 3))
    # mirror x -> W - 1 - x on integer coordinates (truncation is not mirror-symmetric for fractions: snap first)
    snapped = c["poses"].copy()
    snapped[..., :2] = np.trunc(snapped[..., :2])
    base = orf.overlay_case(dict(c, poses=snapped))["dst"]
    assert np.array_equal(base, ref)
    mir = snapped.copy()
    mir[..., 0] = W - 1 - mir[..., 0]
    m = dict(c, poses=mir, src=np.ascontiguousarray(c["src"][:, :, ::-1]))
    assert np.array_equal(orf.overlay_case(m)["dst"], ref[:, :, ::-1])


def test_painted_value_stays_between_the_old_value_and_the_colour():
    m0 = np.arange(256, dtype=np.int64)[:, None, None]
    col = np.arange(256, dtype=np.int64)[None, :, None]
    cov = np.arange(17, dtype=np.int64)[None, None, :]
    m1 = m0 + (((col - m0) * cov + 8) >> 4)
    assert (m1 >= np.minimum(m0, col)).all() and (m1 <= np.maximum(m0, col)).all()
    assert (m1[:, :, 16] == col[:, :, 0]).all() and (m1[:, :, 0] == m0[:, :, 0]).all()


@pytest.mark.parametrize("name", oc.CASE_NAMES)
def test_case_reaches_what_it_is_named_for(name):
    c, ref = oc.case(name), oc.reference(name)
    e = c["expect"]
    B, P = c["poses"].shape[:2]
    assert ref["dst"].shape == c["src"].shape and ref["status"].shape == (B, P)
    plans = [oc.plan(c, ref["prims"][b]) for b in range(B)]
    drawn = [[bool(q["drawn"]) and t > 0 for q, t in zip(ref["prims"][b], ref["touched"][b])] for b in range(B)]
    if "status" in e:
        assert ref["status"].tolist() == e["status"]
    if e.get("all_drawn"):
        assert all(q["drawn"] for b in range(B) for q in ref["prims"][b])
    if "zero_length" in e:
        q = ref["prims"][0][3 * e["zero_length"]]
        assert q["kind"] == "line" and (q["a"] == q["b"]).all() and ref["touched"][0][3 * e["zero_length"]] > 0
    if "wins" in e:
        b, i, j, col = e["wins"]
        assert tuple(ref["dst"][b, i, j]) == col and tuple(c["src"][b, i, j]) != col
    if "hidden_joints" in e:
        b, p, joints = e["hidden_joints"]
        for q in ref["prims"][b]:
            if q["p"] == p:
                i1, i2 = c["bones"][q["l"]]
                uses = {int(i1), int(i2)} if q["kind"] == "line" else None
                if uses is not None and uses & set(joints):
                    assert not q["drawn"]
        assert any(q["drawn"] for q in ref["prims"][b] if q["p"] == p)
    if "min_chunks" in e:
        assert max(pl["chunks"] for pl in plans) >= e["min_chunks"]
        last = [s for s, d in enumerate(drawn[0]) if d]
        assert last and last[-1] >= oc.CHUNK, "nothing is drawn from the second chunk"
    if e.get("full_chunk"):
        assert max(pl["max_kept"] for pl in plans) == oc.CHUNK
    for b, p in e.get("empty_people", []):
        assert not any(d for d, q in zip(drawn[b], ref["prims"][b]) if q["p"] == p)
        assert any(drawn[b])
    for b in e.get("empty_images", []):
        assert not any(drawn[b]) and np.array_equal(ref["dst"][b], c["src"][b]) and plans[b]["tiles_met"] == 0
    if "drawn_slots" in e:
        assert [s for s, q in enumerate(ref["prims"][0]) if q["drawn"]] == e["drawn_slots"]
    if "hole" in e:
        b, i, j = e["hole"]
        marks = [q for q in ref["prims"][b] if q["kind"] == "mark" and tuple(q["a"]) == (j, i)]
        one = np.array([j], np.int64), np.array([i], np.int64)
        assert marks and all(orf.coverage(one[0], one[1], q["a"], q["b"], q["h2"], q["r16"])[0] == 0 for q in marks)
    if e.get("caps"):
        q = ref["prims"][0][0]
        d = q["b"] - q["a"]
        ii, jj = np.nonzero((ref["dst"][0] != c["src"][0]).any(-1))
        t = (jj - q["a"][0]) * d[0] + (ii - q["a"][1]) * d[1]
        assert (t < 0).sum() > 20 and (t > d @ d).sum() > 20, "no painted pixel past an end of the line"
    if "unchanged" in e:
        assert np.array_equal(ref["dst"], c["src"]) == e["unchanged"]
    if name != "alpha_0":
        assert not np.array_equal(ref["dst"], c["src"])


def test_table_covers_the_sizes_and_styles():
    cs = [oc.case(n) for n in oc.CASE_NAMES]
    sizes = {(c["H"], c["W"]) for c in cs}
    assert {(1, 1), (63, 65), (65, 63), (130, 70)} <= sizes
    assert any(c["W"] % 4 == k for c in cs for k in (1,)) and any(c["W"] % 4 == 3 for c in cs) and any(c["W"] % 2 == 0 for c in cs)
    assert {0, 2, 64} <= {c["line_h2"] for c in cs} and {0, 6, 64} <= {c["mark_h2"] for c in cs}
    assert {-1, 0, 32, 160} <= {c["mark_r16"] for c in cs}
    assert {0, 1} == {c["colour_mode"] for c in cs} and {0, 128, 256} <= {c["alpha256"] for c in cs}
    assert {2, 3} == {c["poses"].shape[3] for c in cs}
    assert any(c["bones"].shape[0] == 0 and c["boxes"] is not None for c in cs)
    assert any(c["poses"].shape[2] == 1 for c in cs) and any(c["poses"].shape[1] == 64 for c in cs)
    assert any(c["poses"].shape[0] == 3 for c in cs)


def test_rainbow_colours_equal_matplotlib():
    mpl = pytest.importorskip("matplotlib")
    from pose2mesh_release_amd import overlay
    cmap = mpl.colormaps["rainbow"]
    for L in range(1, 65):
        want = np.array([cmap(i) for i in np.linspace(0, 1, L)])[:, :3]
        bgr = np.rint(want[:, ::-1] * 255.0).astype(np.uint8)
        assert np.array_equal(overlay.rainbow_colours(L), bgr), L
        assert np.array_equal(overlay.rainbow_colours(L, "rgb"), bgr[:, ::-1]), L


def test_rainbow_colours_fixed_values():
    from pose2mesh_release_amd import overlay
    assert overlay.rainbow_colours(1).tolist() == [[255, 0, 128]]
    assert overlay.rainbow_colours(2, "rgb").tolist() == [[128, 0, 255], [255, 0, 0]]
    assert overlay.rainbow_colours(0).shape == (0, 3)
    with pytest.raises(ValueError):
        overlay.rainbow_colours(3, "gbr")


def test_presets_carry_the_reference_numbers():
    from pose2mesh_release_amd import overlay
    bones = [[0, 1], [1, 2]]
    k = overlay.PoseOverlay.keypoints(bones, 48, 64)
    assert (k.line_h2, k.mark_h2, k.mark_r16, k.box_h2, k.per_person) == (2, 6, -1, 1, False)
    assert k.thr == pytest.approx(0.4) and k.box_rgb == (255 | 255 << 8)
    assert np.array_equal(k.palette_host, overlay.rainbow_colours(2))
    s = overlay.PoseOverlay.coco_skeleton(bones, 48, 64)
    assert (s.line_h2, s.mark_h2, s.mark_r16, s.per_person) == (2, 3, 32, True) and s.thr == float("-inf")
    assert overlay.PoseOverlay(bones, 8, 8).__dict__["mark_h2"] == 6


def test_constructor_refusals_on_the_host():
    from pose2mesh_release_amd import overlay
    ok = [[0, 1]]
    for kw in (dict(bones=[[0, -1]]), dict(bones=[[0, 64]]), dict(bones=[[0, 1, 2]]), dict(bones=[[0.0, 1.0]]),
               dict(bones=[[0, 1]] * 65), dict(height=0), dict(width=8193), dict(line=65), dict(mark=("disc", 33)),
               dict(mark=("ring", 65, 1)), dict(mark=("square", 1)), dict(colours=[[1, 2, 3], [4, 5, 6]]),
               dict(box_colour=(1, 2, 256))):
        args = dict(dict(bones=ok, height=8, width=8), **kw)
        with pytest.raises(ValueError):
            overlay.PoseOverlay(**args)
    o = overlay.PoseOverlay([[0, 5]], 8, 8)
    with pytest.raises(ValueError):
        o._check_bones(5)
    o._check_bones(6)


def test_cpu_tensors_raise():
    import torch
    from pose2mesh_release_amd import overlay
    from pose2mesh_release_amd._lib import P2MError
    o = overlay.PoseOverlay([[0, 1]], 8, 8)
    with pytest.raises(P2MError):
        o(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 1, 2, 3))
