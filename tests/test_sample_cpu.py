"""CPU: the definition the sample-noise kernels are held to (tests/sample_ref.py) - its Philox stream against the known
answers, its sampling scheme against histograms of the REAL reference's synthesize_pose (tests/golden/sample_noise_ref.npz,
made by tests/golden/make_golden_sample.py), its deterministic chain against the reference's own functions
(tests/golden/sample_chain.npz), and the robustness audit of the cases the GPU tests compare exactly.

Cost: the three distribution tests (20 000 restated draws each), the two planted faults and the audit take about 90 s
together on 8 cores; everything else is immediate.  They are deterministic (fixed seeds)."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import sample_cases
import sample_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_noise_ref.npz")
N_DRAWS = 20000


def test_philox_known_answers():
    def hx(w):
        return " ".join("%08x" % int(x) for x in w)
    assert hx(sample_ref.philox(0, 0, 0, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hx(sample_ref.philox(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # arrays and scalars agree, and the stream layout: key = seed, counter = (index lo, index hi, joint | stage << 8, block)
    w = sample_ref._words(0x299f31d0a4093822, np.array([0x85a308d3243f6a88], np.uint64), 0x2e, 0x13198a, np.array([0x03707344]))
    assert hx([x[0, 0] for x in w]) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    u = sample_ref.uniforms(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], np.uint64))
    assert u.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]
    assert (u.astype(np.float32).astype(np.float64) == u).all()


def test_philox_header_on_the_host(tmp_path):
    """csrc/p2m_philox.h is plain C++: the kernels' generator, compiled for the host, gives the known answers, the stream
    layout of philox_draw and the restatement's uniforms."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (the package's host library needs one too)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "philox_main.cpp"
    src.write_text('#include <cstdio>\n#include "p2m_philox.h"\n'
                   'static void show(p2m::Philox4 d) { std::printf("%08x %08x %08x %08x\\n", d.w[0], d.w[1], d.w[2], d.w[3]); }\n'
                   'int main() {\n'
                   '  show(p2m::philox4x32_10(0, 0, 0, 0, 0, 0));\n'
                   '  show(p2m::philox4x32_10(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u));\n'
                   '  show(p2m::philox_draw(0x299f31d0a4093822ull, 0x85a308d3243f6a88ull, 0x2e, 0x13198a, 0x03707344u));\n'
                   '  show(p2m::philox_draw(123, (1ull << 32) + 5, 16, 7, 999));\n'
                   '  std::printf("%.9g %.9g\\n", p2m::philox_uniform(0xFFFFFFFFu), p2m::philox_uniform(0x1FFu));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "philox_main"
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", os.path.join(root, "pose2mesh_release_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert lines[0] == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert lines[1] == lines[2] == "d16cfe09 94fdcceb 5001e420 24126ea1"
    w = sample_ref._words(123, np.array([(1 << 32) + 5], np.uint64), 16, 7, np.array([999]))
    assert lines[3] == " ".join("%08x" % int(x[0, 0]) for x in w)
    assert [np.float32(v) for v in lines[4].split()] == [np.float32(1.0 - 2.0 ** -24), np.float32(2.0 ** -24)]


def test_kernel_constants_match_restatement():
    """The literals of csrc/sample.hip - sqrt(-2 ln ks), the candidate counts, the stage numbers - are the restatement's."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "pose2mesh_release_amd", "csrc", "sample.hip")).read()
    for name, want in (("C10", sample_ref.C10), ("C50", sample_ref.C50), ("C85", sample_ref.C85)):
        lit = re.search(r"\b%s = ([0-9.]+)f" % name, src).group(1)
        assert np.float32(lit) == want, (name, lit)
    for name, want in (("N_JITTER", 500), ("N_MISS", 2000), ("N_INV", 500), ("N_GOOD", 125)):
        assert int(re.search(r"\b%s = (\d+)" % name, src).group(1)) == want == getattr(sample_ref, name)
    stages = dict(re.findall(r"\b(ST_[A-Z0-9_]+) = (\d+)", src))
    assert len(stages) == 10 and all(getattr(sample_ref, k) == int(v) for k, v in stages.items())
    assert re.search(r"FAR = 1\.0f \+ 0x1p-10f", src) and sample_ref.FAR == np.float32(1 + 2.0 ** -10)


U = 2.0 ** -24


@pytest.mark.parametrize("name", list(sample_cases.chain_fixture_cases()))
def test_chain_matches_reference(name):
    """The float64 restatement of the deterministic chain against what the reference's own cam2pixel, get_bbox,
    process_bbox, j2d_processing (+ the area from its trans), flip_2d_joint, j3d_processing and standardisation give.

    The restatement is exact up to float64 round-off; the REFERENCE rounds to float32 in three places, and the bars are
    derived from those casts, with u = 2^-24, C = the largest image coordinate of the sample's joints, s = W / bbox_w:
      get_bbox            returns float32: each of x, y, w, h carries <= u C                          -> tight: 2 u C
      process_bbox        float64 on those: centre (x + (w - 1) / 2) <= 1.5 u C, sides <= u C / aspect -> bbox: 4 u C
      get_center_scale    float32 again: centre + u C (<= 2.5 u C), scale relative u
      src / dst triplets  float32: centre, centre + dir and the third point each + u C.  The fitted similarity moves the
                          centre by <= 3.5 u C and errs in scale / angle by <= 2 (2 u C) / (bbox_w / 2) relative - over a
                          lever of <= bbox_w / sqrt(2) from the centre that is <= 6 u C; times s into the crop: <= 10 s u C
      j2d_processing      returns float32: + u max(W, H)                                               -> px: 10 s u C + u H
    and 16 max(s, 1) u C + 2 u H is asserted.  The area is a product of two side lengths, each the difference of two points
    with that error: <= 2 bar (side_1 + side_2), doubled.  pose2d = (px / W - mean) / std: the bar over W std, doubled for
    the error of mean and std themselves.  j3d_processing returns float32: 2 u max |coordinate| on the lift target."""
    g = np.load(os.path.join(os.path.dirname(GOLDEN), "sample_chain.npz"))
    c = sample_cases.chain_fixture_cases()[name]
    r = sample_ref.chain(c["verts"], c["focal"], c["princpt"], rot=c["rot"], flip=c["flip"], **sample_cases.chain_kwargs(c))
    assert (r["status"] == 0).all()
    ref = {k: g[f"{name}_{k}"] for k in ("joint_cam", "img", "tight", "bbox", "px", "area", "flipped", "lift", "pose2d")}
    C = np.abs(ref["img"]).max(axis=(1, 2))
    s = c["W"] / ref["bbox"][:, 2]
    bar = 16 * np.maximum(s, 1) * U * C + 2 * U * c["H"]
    std = (ref["flipped"] / [c["W"], c["H"]]).std(axis=1)
    sides = np.sqrt(ref["area"])
    checks = [("joint_cam", r["joint_cam"], 1e-9 + 0 * C), ("img", r["img"], 1e-9 + 0 * C), ("tight", r["tight"], 2 * U * C),
              ("bbox", r["bbox"], 4 * U * C), ("px", r["px"], bar), ("flipped", r["flipped"], bar),
              ("area", r["area"], 2 * 2 * bar * 2 * sides * 1.5),
              ("lift", r["lift_pose3d"], 2 * U * np.abs(ref["lift"]).max(axis=(1, 2))),
              ("pose2d", r["pose2d"], 2 * bar / (min(c["W"], c["H"]) * std.min(axis=1)))]
    for k, got, b in checks:
        err = np.abs(got - ref[k]).reshape(len(C), -1).max(axis=1)
        print(f"{name} {k}: worst error / bar = {(err / b).max():.3f}")
        assert (err <= b).all(), k


def test_chain_degenerate_and_fit():
    """One vertex: every joint coincides, process_bbox would return None - status bit 0, zero outputs, zero masks.  Given
    reg joints: fit_err is the mean distance after mean alignment, and the masks of data/Human36M/dataset.py:396-400."""
    c = sample_cases.chain_case(3, 1, 41, "coco")
    r = sample_ref.chain(c["verts"], c["focal"], c["princpt"], rot=c["rot"], flip=c["flip"], **sample_cases.chain_kwargs(c))
    assert (r["status"] == 1).all() and not r["mesh_valid"].any() and not r["lift_valid"].any() and not r["reg_valid"].any()
    assert all((r[k] == 0).all() for k in ("pose2d", "mesh", "lift_pose3d", "reg_pose3d"))
    c = sample_cases.chain_case(4, 63, 42, "coco")
    base = sample_ref.chain(c["verts"], c["focal"], c["princpt"], rot=c["rot"], flip=c["flip"], **sample_cases.chain_kwargs(c))
    given = sample_cases.given_joints(c, base)
    r = sample_ref.chain(c["verts"], c["focal"], c["princpt"], rot=c["rot"], flip=c["flip"], given_cam=given, fit_thr=30.0,
                         **sample_cases.chain_kwargs(c))
    assert (np.abs(r["fit_err"] - sample_cases.GIVEN_OFFSET_MM) <= 1e-3).all()      # given is float32 mm: 1e-4 at most
    over = sample_cases.GIVEN_OFFSET_MM > 30.0
    assert np.array_equal(r["status"], np.where(over, 2, 0))
    assert np.array_equal(r["mesh_valid"][:, 0] == 0, over) and np.array_equal(r["lift_valid"][:, 0] == 0, over)
    assert r["reg_valid"].all()
    assert np.allclose(r["reg_pose3d"], given - given[:, :1], atol=1e-3)


def _draws(joints, area, n, seed, fault=None, chunk=1000):
    """n draws of one pose: global indices 0 .. n - 1, in chunks across threads (numpy releases the GIL; the result does not
    depend on the chunking - that is the stream's contract, and test_batching_invariance checks it)."""
    def run(i0):
        m = min(chunk, n - i0)
        return sample_ref.noise_coco(np.repeat(joints[None], m, 0), np.full(m, area, np.float32), sample_ref.COCO_SIGMAS, seed,
                                     i0, fault=fault)[0]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return np.concatenate(list(ex.map(run, range(0, n, chunk))))


def _worst(out, joints, area, ref_hist, ref_zero, n_ref):
    """Largest |p - p_ref| / bar over the bins of all joints (and the zeroed shares), bar = 5 sqrt(pbar (1 - pbar) (1 / n +
    1 / n_ref)) + 1 / n_ref with pbar the pooled share."""
    n = out.shape[0]
    hist, zero = sample_ref.displacement_histogram(out, joints, area, sample_ref.COCO_SIGMAS)
    c = np.concatenate([hist.reshape(17, -1), zero[:, None]], axis=1).astype(np.float64)
    r = np.concatenate([ref_hist.reshape(17, -1), ref_zero[:, None]], axis=1).astype(np.float64)
    pbar = (c + r) / (n + n_ref)
    bar = 5.0 * np.sqrt(pbar * (1.0 - pbar) * (1.0 / n + 1.0 / n_ref)) + 1.0 / n_ref
    return float((np.abs(c / n - r / n_ref) / bar).max())


@pytest.mark.parametrize("name", list(sample_cases.histogram_poses()))
def test_noise_distribution_matches_reference(name):
    """20 000 draws of the restatement against the recorded histogram of 4000 draws of the real synthesize_pose: this ties
    the 'first passing candidate' scheme to the reference.  Fixed seeds: deterministic."""
    g = np.load(GOLDEN)
    joints, area = sample_cases.histogram_poses()[name]
    assert np.array_equal(g[name + "_joints"], joints) and float(g[name + "_area"]) == area, "fixture made for another pose"
    out = _draws(joints, area, N_DRAWS, seed=2024)
    worst = _worst(out, joints, area, g[name + "_hist"], g[name + "_zeroed"], int(g["n_draws"]))
    print(f"{name}: worst |p - p_ref| / bar = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("name,fault", [("all_valid", "swap_radii"), ("valid4_close", "no_pair")])
def test_noise_distribution_rejects_planted_fault(name, fault):
    """The same comparison must fail for a wrong sampler: jitter and good radii exchanged; the pair dependence removed."""
    g = np.load(GOLDEN)
    joints, area = sample_cases.histogram_poses()[name]
    out = _draws(joints, area, 4000, seed=2024, fault=fault)
    worst = _worst(out, joints, area, g[name + "_hist"], g[name + "_zeroed"], int(g["n_draws"]))
    print(f"{name} with {fault}: worst |p - p_ref| / bar = {worst:.3f}")
    assert worst > 1.0


def test_batching_invariance():
    """A sample's result depends on (seed, global index) alone."""
    c = sample_cases.noise_cases()["valid_le10"]
    a = sample_ref.noise_coco(c["joints"], c["area"], sample_ref.COCO_SIGMAS, c["seed"], c["first_index"])
    b = [sample_ref.noise_coco(c["joints"][s], c["area"][s], sample_ref.COCO_SIGMAS, c["seed"], c["first_index"] + s.start)
         for s in (slice(0, 4), slice(4, 9))]
    for k in range(3):
        assert np.array_equal(a[k], np.concatenate([x[k] for x in b]))


def _all_cases():
    cases = dict(sample_cases.noise_cases())
    cases["zeroed_lower"] = sample_cases.zeroed_lower_case()
    return cases


@pytest.mark.parametrize("name", list(_all_cases()))
def test_robustness_audit(name):
    """At most 5 % of the (sample, unit) pairs of a case may be non-robust (a deciding candidate inside the fp32 band of its
    threshold, sample_ref.py's docstring; units declared coincident have margin 0 by construction and do not count) - a
    condition on the seeds of sample_cases.py.  And the band must do its job: an fp32 run of the restatement decides every
    robust unit like the float64 run."""
    c = _all_cases()[name]
    out, kind, robust = sample_ref.noise_coco(c["joints"], c["area"], sample_ref.COCO_SIGMAS, c["seed"], c["first_index"])
    out32, kind32, _ = sample_ref.noise_coco(c["joints"], c["area"], sample_ref.COCO_SIGMAS, c["seed"], c["first_index"],
                                             dtype=np.float32)
    counted = np.ones(9, bool)
    counted[list(c["coincident"])] = False
    share = 1.0 - robust[:, counted].mean()
    print(f"{name}: non-robust units {share:.4f} of {robust[:, counted].size}")
    assert share <= 0.05
    assert all(robust[:, u].sum() == 0 for u in c["coincident"]), "a coincident pair must be flagged"
    rj = robust[:, (np.arange(17) + 1) // 2]                        # per joint
    assert np.array_equal(kind[rj], kind32[rj])
    assert np.isfinite(out32).all() and set(np.unique(kind32)) <= {-1, 0, 1, 2, 4}
    err = np.abs(out32[rj] - out[rj]).max()
    assert err <= 64 * 2.0 ** -24 * (np.abs(c["joints"][:, :, :2]).max() + 400.0), err      # fp32 round-off, nothing else


def test_zeroed_lower_joint_feeds_origin():
    c = sample_cases.zeroed_lower_case()
    out, kind, _ = sample_ref.noise_coco(c["joints"], c["area"], sample_ref.COCO_SIGMAS, c["seed"], c["first_index"])
    assert (kind[:, [1, 11]] == -1).all() and (out[:, [1, 11]] == 0).all()
    assert (kind[:, [2, 12]] >= 0).all() and (out[:, [2, 12], 2] == 1).all()
    assert np.array_equal(out[:, [2, 12], :2], c["joints"][:, [2, 12], :2])      # area 0: every radius is 0


def test_table_noise_statistics():
    """The restated table noise: Bernoulli rate and the moments of the added normals, 5 sigma."""
    J, n = 5, 40000
    mean, std, weight = sample_cases.table(J, 3)
    out, mask = sample_ref.noise_table(np.zeros((n, J, 2), np.float32), mean, std, weight, 288, 384, 77, 0)
    assert not mask[:, 0].any() and mask[:, J - 1].all()
    for j in range(1, J):
        p = float(weight[j])
        assert abs(mask[:, j].mean() - p) <= 5 * np.sqrt(p * (1 - p) / n) + 1e-12
        z = out[mask[:, j], j] / np.array([288 / 256, 384 / 256])
        m = mask[:, j].sum()
        assert (np.abs(z.mean(0) - mean[j]) <= 5 * std[j] / np.sqrt(m)).all()
        assert (np.abs(z.std(0) / std[j] - 1) <= 5 / np.sqrt(2 * m)).all()
