"""CPU: the device-exact yardstick of the renderer (render_ref.rasterise_exact) and the edge-case table
(tests/render_edge_cases.py), without a GPU.  Three things the GPU tests of tests/test_gpu_render_edges.py rely on:

  * render_ref.fma32 IS fmaf: bitwise equal to rational arithmetic rounded once, on random triples, on triples built to land on
    and next to fp32 rounding midpoints (where a float64 sum rounded twice goes wrong), and on zero, inf and NaN operands;
  * the two yardsticks agree: on every case of tests/render_cases.py rasterise_exact gives rasterise's face and mesh wherever
    rasterise decides, a depth within rasterise's bound, and the same coverage on every pixel;
  * every edge case reaches the arm it is named for, computed from the case itself - a tie case has tied fragments in front, the
    512-face case has 512 whole-block faces in one flush, the seam case has centres on edges next to the tile borders, ...  A
    case that stops reaching its arm fails here, not silently on the GPU."""
from fractions import Fraction

import numpy as np
import pytest

import render_cases as rc
import render_edge_cases as ec
import render_ref as rr

F32 = np.float32


def round_fraction_to_f32(q):
    """The fp32 nearest to the rational q, ties to even, subnormals and overflow included: exact integer arithmetic."""
    if q == 0:
        return F32(0.0)
    sign, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    e = e if Fraction(2) ** e <= a else e - 1                  # 2^e <= a < 2^(e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = a / quantum
    k = n.numerator // n.denominator
    rest = n - k
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k % 2 == 1):
        k += 1
    v = k * quantum
    if v >= Fraction(2) ** 128:
        return F32(sign * np.inf)
    return F32(sign * float(v))                                # (k < 2^25: exact in float64, and in fp32 by construction)


def _check_triples(a, b, c):
    """-> (mismatches, results): fma32 against Fraction on finite triples, bitwise; a zero of either sign only for an exact 0."""
    got = rr.fma32(a, b, c)
    bad = 0
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got):
        q = Fraction(x) * Fraction(y) + Fraction(z)
        want = round_fraction_to_f32(q)
        if q == 0:
            bad += not (g == 0)
        else:
            bad += not (g.view(np.uint32) == want.view(np.uint32))
    return bad, got


def _random_f32(rng, n, emin=-40, emax=40):
    m = rng.integers(1 << 23, 1 << 24, n).astype(np.float64) * rng.choice([-1.0, 1.0], n)
    return np.ldexp(m, rng.integers(emin, emax, n) - 23).astype(F32)


def test_fma32_is_fmaf_on_random_triples():
    rng = np.random.default_rng(5)
    n = 24000                                                # (31 000 triples here, 9 000 at the midpoints below)
    a, b = _random_f32(rng, n), _random_f32(rng, n)
    # the addend within 2^+-30 of the product (both operands matter), and a share far off; some operands with few bits
    ex = np.frexp(a.astype(np.float64) * b.astype(np.float64))[1]
    c = np.ldexp(rng.integers(1 << 23, 1 << 24, n).astype(np.float64) * rng.choice([-1.0, 1.0], n),
                 ex + rng.integers(-30, 31, n) - 24).astype(F32)
    short = rng.random(n) < 0.3
    a[short] = (a[short].view(np.uint32) & np.uint32(0xFFFFF000)).view(F32)
    b[short] = (b[short].view(np.uint32) & np.uint32(0xFFFFF000)).view(F32)
    # the range of the renderer: weights in [0, 1] as quotients, z differences, z0
    E = rng.integers(0, 1 << 30, 4000)
    A = E + rng.integers(1, 1 << 30, 4000)
    a = np.concatenate([a, E.astype(F32) / A.astype(F32)])
    b = np.concatenate([b, rng.standard_normal(4000).astype(F32)])
    c = np.concatenate([c, rng.standard_normal(4000).astype(F32)])
    # subnormal results and operands, and results at the overflow threshold
    a = np.concatenate([a, _random_f32(rng, 2000, -80, -60), _random_f32(rng, 1000, 60, 64)])
    b = np.concatenate([b, _random_f32(rng, 2000, -80, -60), _random_f32(rng, 1000, 60, 64)])
    c = np.concatenate([c, _random_f32(rng, 2000, -149, -120), _random_f32(rng, 1000, 120, 128)])
    bad, got = _check_triples(a, b, c)
    assert bad == 0, bad
    assert np.isinf(got).any() and ((got != 0) & (np.abs(got) < 2.0 ** -126)).any()      # both ends were reached


def test_fma32_is_fmaf_at_midpoints():
    """product + addend exactly on an fp32 midpoint (ties to even), and 2^-36 or 2^-46 of the product's size off it, where the
    float64 sum lands ON the midpoint and only the TwoSum's remainder knows the side."""
    rng = np.random.default_rng(6)
    n = 9000
    u = 2.0 ** -12
    kind = rng.integers(0, 4, n)
    fa = np.choose(kind, [1.0 + 2.0 ** -23, 1.0 + u, 1.0, 1.5])
    fb = np.choose(kind, [1.0 - 2.0 ** -23, 1.0 - u + u * u, 1.0, 0.5 + 2.0 ** -20])  # products 1 - 2^-46, 1 + 2^-36, 1, .75 + ...
    ea, eb = rng.integers(-30, 30, n), rng.integers(-30, 30, n)
    a = (np.ldexp(fa, ea) * rng.choice([-1.0, 1.0], n)).astype(F32)
    b = np.ldexp(fb, eb).astype(F32)
    ep = np.floor(np.log2(np.abs(a.astype(np.float64) * b.astype(np.float64)) * (1 + 2.0 ** -30))).astype(np.int64)
    ep = np.where(kind == 0, ea + eb, ep)                     # (kind 0's product lies just under 2^(ea + eb): its midpoint)
    # the addend: a 24-bit integer times 2^(ep + 1), so the product's leading bit is half a unit in its last place
    c = (np.ldexp(rng.integers(1 << 23, 1 << 24, n).astype(np.float64), ep + 1) * rng.choice([-1.0, 1.0], n)).astype(F32)
    bad, _ = _check_triples(a, b, c)
    assert bad == 0, bad
    # the audit is about something: a float64 sum rounded to fp32 (two roundings) is wrong on a good share of these
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert (twice.view(np.uint32) != rr.fma32(a, b, c).view(np.uint32)).sum() > n // 10


def test_fma32_special_operands():
    inf, nan = F32(np.inf), F32(np.nan)
    f = rr.fma32
    assert np.isnan(f(inf, 0.0, 1.0)) and np.isnan(f(0.0, inf, 1.0)) and np.isnan(f(inf, 1.0, -inf)) and np.isnan(f(1.0, 1.0, nan))
    assert np.isnan(f(nan, 0.0, 0.0)) and np.isnan(f(0.0, nan, 1.0))
    assert f(inf, 2.0, 1.0) == inf and f(-inf, 2.0, 1.0) == -inf and f(1.0, 1.0, inf) == inf and f(inf, -1.0, -inf) == -inf
    assert f(3.0e38, 3.0e38, 0.0) == inf and f(-3.0e38, 3.0e38, 0.0) == -inf          # overflow of a finite product
    big = F32(3.4028235e38)
    assert f(big, 1.0, F32(2.0 ** 102)) == big and f(big, 1.0, F32(2.0 ** 103)) == inf  # below / on the overflow midpoint
    assert f(-big, 1.0, -F32(2.0 ** 103)) == -inf

    def sign(x):
        return bool(np.signbit(x))
    for a, b, c, neg in ((0.0, 1.0, 0.0, False), (-0.0, 1.0, 0.0, False), (0.0, 1.0, -0.0, False), (-0.0, 1.0, -0.0, True),
                         (0.0, -1.0, -0.0, True), (1.0, 1.0, -1.0, False), (-1.0, 1.0, 1.0, False), (0.5, 0.0, -0.0, False)):
        r = f(F32(a), F32(b), F32(c))
        assert r == 0 and sign(r) == neg, (a, b, c, r)
    assert f(F32(0.25), F32(0.0), F32(0.7)) == F32(0.7) and f(F32(0.0), F32(-3.0), F32(-0.7)) == F32(-0.7)
    tiny = F32(2.0 ** -149)
    assert f(tiny, F32(0.5), F32(0.0)) == 0 and f(tiny, F32(0.75), F32(0.0)) == tiny and f(tiny, F32(0.5), tiny) == tiny * 2


def test_depth_bits_preserve_the_order():
    v = np.array([-np.inf, -3.0e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 0.5, 1.0, 3.0e38, np.inf], F32)
    b = rr.depth_bits(v)
    assert (np.diff(b.astype(np.int64)) > 0).all()
    assert (rr.bits_depth(b).view(np.uint32) == v.view(np.uint32)).all()


@pytest.mark.parametrize("name", rc.CASE_NAMES)
def test_the_two_yardsticks_agree(name):
    for a, b in zip(rc.reference(name), ec.reference(name)):
        cmp, cov = ~a["left_out"], a["face_id"] >= 0
        assert (cov == (b["face_id"] >= 0)).all(), name
        assert (a["face_id"] == b["face_id"])[cmp].all() and (a["mesh_id"] == b["mesh_id"])[cmp].all(), name
        assert (a["count"] == b["count"]).all() and (a["on_edge"] == b["on_edge"]).all(), name
        assert not b["left_out"].any() and b["depth"].dtype == np.float32 and np.isposinf(b["depth"][~cov]).all()
        sel = cmp & cov
        assert (np.abs(b["depth"][sel].astype(np.float64) - a["depth"][sel]) <= a["bound"][sel]).all(), name


def _tile_bbox_pixels(c, b, f, tile):
    """Pixels of face f's clipped bbox inside tile (ty, tx) of mesh b, from the yardstick's own projection."""
    xy = rr.project(c["verts"][b], c["cam"][b], c["H"], c["W"])["xy"]
    i = c["faces"][f]
    x0, y0, x1, y1 = rr.pixel_bbox(xy[i, 0], xy[i, 1], c["H"], c["W"])
    xa, xb = max(x0, 64 * tile[1]), min(x1, 64 * tile[1] + 63)
    ya, yb = max(y0, 64 * tile[0]), min(y1, 64 * tile[0] + 63)
    return max(xb - xa + 1, 0) * max(yb - ya + 1, 0)


@pytest.mark.parametrize("name", ec.CASE_NAMES)
def test_every_case_reaches_its_arm(name):
    c, ref = ec.case(name), ec.reference(name)
    im = ref[0]
    arm = c["arm"]
    H, W = c["H"], c["W"]
    cov = im["face_id"] >= 0
    for p in im["proj"]:                                        # xy_fix must match the device's exactly
        assert float(p["margin"].min()) > rr.SNAP_MARGIN, name
    assert not im["left_out"].any() and ((im["mesh_id"] >= 0) == cov).all() and np.isposinf(im["depth"][~cov]).all()
    bg = c["background"]
    assert (im["image"][~cov] == (0 if bg is None else bg[~cov])).all()
    kept, dropped = im["kept"], im["dropped"]
    if arm[0] == "covered":
        assert cov.any() and not cov.all()
    elif arm[0] in ("tie", "tie_paths"):                       # tied fragments in front, and the stated faces win there
        front = im["ties"] >= 2
        assert front.sum() >= 10 and set(np.unique(im["face_id"][front])) == arm[1], name
        z = c["verts"][0][c["faces"][list(arm[1])[0]], 2]
        assert (z == z[0]).all() and z[0] != 0 or name == "neg_zero"
        assert (im["depth"][front] == z[0]).all()              # constant z: the depth is exactly z0
        if name == "neg_zero":                                 # (-0) - (-0) = +0, and fma(l, +0, -0) = +0
            assert np.signbit(c["verts"][0][:, 2]).all() and not np.signbit(im["depth"][cov]).any()
        if name == "tie_steps_low_wins":                       # 3 and 700: two scan steps, and a full queue between them
            assert (np.array([k[1] for k in kept]) // 256 == 1).sum() >= 10 and len(kept) > 256 + 2
            assert kept[(0, 700)] > 0 and not (im["face_id"] == 700)[front].any()
        if arm[0] == "tie_paths":
            n = sorted(_tile_bbox_pixels(c, 0, f, (0, 0)) for f in (0, 1))
            assert n[0] <= 256 < n[1], n
    elif arm[0] == "scene_tie":                                # every covered pixel is tied over ranks, and `arm[1]` shows
        B = c["verts"].shape[0]
        assert cov.any() and (im["ties"][cov] >= B).all() and (im["mesh_id"][cov] == arm[1]).all()
    elif arm[0] == "scene_rank_vs_face":
        P, R = np.zeros((H, W), bool), np.zeros((H, W), bool)
        P[:, :28], R[:, 28:] = True, True
        three = im["ties"] >= 3
        want = {"depth": ((0, 0), (0, 1)), "list": ((1, 1), (1, 0))}[arm[1]]       # (mesh, face) in P and in R
        for reg, (m, f) in zip((P, R), want):
            assert (three & reg).sum() > 50
            assert (im["mesh_id"][three & reg] == m).all() and (im["face_id"][three & reg] == f).all(), (name, m, f)
    elif arm[0] == "ids":
        for f in arm[1]:
            assert (im["face_id"] == f).sum() >= 1, (name, f)
        if name == "tie_steps_high_nearer":
            both = (im["count"] >= 2) & np.isin(im["face_id"], (3, 700))
            assert both.sum() >= 10 and (im["face_id"][both] == 700).all()
    elif arm[0] == "clip":
        for f in arm[1]:
            assert kept[(0, f)] > 0 and dropped[(0, f)] == 0, (name, f)
        for f in arm[2]:
            assert kept[(0, f)] == 0 and dropped[(0, f)] > 0, (name, f)
        if name == "clip_planes":
            z, (zmin, zmax) = c["verts"][0][::3, 2], c["z_range"]
            assert z[0] == zmax and z[1] == np.nextafter(zmax, F32(np.inf)) and z[2] == zmin
            assert z[3] == np.nextafter(zmin, F32(-np.inf)) and zmin < z[4] < zmax
            assert all((im["face_id"] == f).any() for f in (0, 2, 4))
            assert (im["face_id"] == 4).sum() > kept[(0, 4)] - kept[(0, 2)]              # it shows through faces 1 and 3
    elif arm[0] == "nothing":
        assert not cov.any()
        for f in arm[1]:
            assert kept[(0, f)] == 0 and dropped[(0, f)] > 0
        if name == "cam_sx_zero":
            assert not kept and not dropped and not any(p["clamped"].any() for p in im["proj"])
    elif arm[0] == "crossing":
        for f in arm[1]:
            assert kept[(0, f)] > 50 and dropped[(0, f)] > 50, (name, f)
    elif arm[0] == "big512":
        n = np.array([_tile_bbox_pixels(c, 0, f, (0, 0)) for f in range(len(c["faces"]))])
        assert (n[:512] > 256).all() and len(n) > 512 and (n[512:515] <= 256).all() and n[515] > 256
        assert H <= 64 and W <= 64 and len(kept) == len(n)                                 # one tile, every face in its queue
        z = c["verts"][0][::3, 2]
        assert len(np.unique(z[:512])) == 511 and z[100] == z[300] == z[:512].min()
        pair = (im["ties"] >= 2) & (im["depth"] == z[100])
        assert pair.sum() > 100 and (im["face_id"][pair] == 100).all() and (im["face_id"] == 300).any()
    elif arm[0] == "straddle":
        assert _tile_bbox_pixels(c, 0, arm[1], (0, 0)) > 256 and 0 < _tile_bbox_pixels(c, 0, arm[1], (0, 1)) <= 256
        assert (im["face_id"][:, :64] == arm[1]).any() and (im["face_id"][:, 64:] == arm[1]).any()
    elif arm[0] == "seam":
        for k in (63, 64, 127, 128):
            assert im["on_edge"][:, k].sum() >= 100 and im["on_edge"][k, :].sum() >= 100, (name, k)
        assert im["count"].max() == 1 and (im["count"][:129, :129] == 1).all() and not cov[129, :].any() and not cov[:, 129].any()
    elif arm[0] == "extent":
        long_axis = 0 if H >= W else 1
        line = cov.any(1 - long_axis)
        assert line[0] and line[-1] and (im["face_id"] == 0).any(1 - long_axis).sum() > 6000
        xy = im["proj"][0]["xy"]
        box = rr.pixel_bbox(xy[:3, 0], xy[:3, 1], H, W)                                    # the thin face's bbox: 0 .. 8191
        assert (box[1], box[3]) == (0, H - 1) if H >= W else (box[0], box[2]) == (0, W - 1)
        ends = np.unique(np.concatenate([im["face_id"][:4, :4].ravel(), im["face_id"][-4:, -4:].ravel()]))
        assert len(ends[ends > 0]) >= 2
    elif arm[0] == "scene_skip":
        xy = [p["xy"] for p in im["proj"]]
        assert xy[1][:, 0].min() > 256 * W                                                  # mesh 1: off the image
        assert not any(k[0] in (1, 2) for k in list(kept) + list(dropped))                  # 1, 2: no fragment at all
        m3 = [k for k in kept if k[0] == 3]
        assert len(m3) == 32 and xy[3].min() > 256 * 64 and xy[3].max() < 256 * 128         # mesh 3: inside tile (1, 1)
        for m in (0, 4):                                                                    # 0, 4: in all nine tiles
            hit = {(ty, tx) for ty in range(3) for tx in range(3) for f in range(32) if _tile_bbox_pixels(c, m, f, (ty, tx))}
            assert len(hit) == 9
        assert set(np.unique(im["mesh_id"])) == ({0, 4} if c["order"] == "list" else {0, 3, 4})
    elif arm[0] == "mirror":
        assert im["proj"][0]["mirror"] == arm[1] and cov.sum() > 1000 and im["count"].max() == 1
    elif arm[0] == "shade":
        rgb, v = im["image"][cov].astype(int), im["v"][cov]
        assert cov.sum() > 500
        if arm[1] == "no_light":
            assert len(c["lights"]) == 0 and len(np.unique(rgb, axis=0)) == 1
        elif arm[1] == "four_lights":
            assert len(c["lights"]) == 4 and len(np.unique(rgb, axis=0)) > 20
        elif arm[1] == "saturated":
            assert (v == 255.5).any() and (rgb[v == 255.5] == 255).all() and (c["colours"][0] * c["ambient"] > 1).any()
        elif arm[1] == "negative":
            assert (v[:, 0] < 0).all() and (rgb[:, 0] == 0).all() and (rgb[:, 1] > 0).all()
        elif arm[1] == "behind":
            assert (rgb == 0).all() and (bg[cov] > 0).all()
    elif arm[0] == "status":
        st = []
        nv = c["verts"].shape[1]
        ok = ((c["faces"] >= 0) & (c["faces"] < nv)).all(1)
        for b, r in enumerate(ref):
            used = np.zeros(nv, bool)
            used[c["faces"][ok].reshape(-1)] = True
            st.append(int(r["proj"][0]["clamped"][used].any()) | (0 if ok.all() else 2))
        assert st == arm[1], (name, st)
        if name == "status_unreferenced":
            assert im["proj"][0]["clamped"].any()
        assert cov.any()
    else:
        raise AssertionError(arm)
